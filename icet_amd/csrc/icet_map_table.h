// icet_amd/csrc/icet_map_table.h -- the voxel map's table as its kernels see it, shared by the translation units that write it: icet_map.hip (add, remove) and
// icet_map_snapshot.hip (load, merge).  The structs and the update step, in the unnamed namespace on purpose: each unit gets its own
// internal copy, and the kernels of icet_map.hip keep the names and the code they had when this text stood in that file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "icet_buffers.h"
#include "icet_map.h"
#include "icet_map_shape.h"

namespace icet {

// THE CELLS SORTED BY KEY (map_sorted_cells, icet_map.hip): the selected (key, entry) pairs, their sorted copy, rocPRIM's scratch and what it holds.  cap: pairs.
struct SortedCells {
    unsigned long long* sel_key = nullptr; unsigned long long* key = nullptr; uint32_t* sel_idx = nullptr; uint32_t* idx = nullptr; void* tmp = nullptr;
    size_t tmp_bytes = 0; int64_t cap = 0;
    BufferGroup mem;
};

namespace {

typedef unsigned long long u64;

// key[size] | count[size] (two's complement) | sum[3][size]
struct MapTable { u64* key; u64* count; u64* sum; uint32_t log2; };
// a shaped map's table (section 25): beside it mom[9][size], the words S_x S_y S_z M_xx M_xy M_xz M_yy M_yz M_zz.  The plain kernels take the plain struct.
struct MapShapeTable : MapTable { u64* mom; };
template <bool kShape> using TableOf = std::conditional_t<kShape, MapShapeTable, MapTable>;
// the device record: kTotCopies copies of the running totals, one 64-byte line each (a block adds to copy blockIdx % kTotCopies, so that the blocks of a launch
// do not all queue on one address; the host sums the copies), then what the last count pass saw and the select pass's cursor
enum { kCtrIn = 0, kCtrKept, kCtrNonfinite, kCtrOutside, kCtrDropped, kTotWords = 8 };
constexpr int kTotCopies = 64;
enum { kCtrOccupied = kTotCopies * kTotWords, kCtrOut, kCtrNegative, kCtrSelected, kCtrWords = kTotCopies * kTotWords + 8 };

#define MAP_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define MAP_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// count += dn, sum_a += d_a in the cell of `key`, claimed on the way if it is new.  False: the probe run met neither the key nor a free entry (the table is full).
// An entry's key changes once, from empty to its key, so a stale read of "empty" only costs the compare-and-swap that then returns the truth.
// more(h, size): what a shaped map adds behind the same claimed entry (table_update_shape); table_update adds nothing.
template <class More>
__device__ __forceinline__ bool table_update_and(const MapTable& t, u64 key, u64 dn, u64 d0, u64 d1, u64 d2, More&& more) {
    const u64 mask = ((u64)1 << t.log2) - 1;
    u64 h = icet_map_rule::mix(key) & mask;                           // h <= mask: inside every array
    for (u64 p = 0; p <= mask; p++) {
        u64 k = __hip_atomic_load(&t.key[h], MAP_RLX_AGENT);
        if (k == icet_map_rule::kEmpty) {
            u64 expected = icet_map_rule::kEmpty;
            k = __hip_atomic_compare_exchange_strong(&t.key[h], &expected, key, __ATOMIC_RELAXED, MAP_RLX_AGENT) ? key : expected;
        }
        if (k == key) {
            const u64 size = mask + 1;
            __hip_atomic_fetch_add(&t.count[h], dn, MAP_RLX_AGENT);
            __hip_atomic_fetch_add(&t.sum[h], d0, MAP_RLX_AGENT);
            __hip_atomic_fetch_add(&t.sum[size + h], d1, MAP_RLX_AGENT);
            __hip_atomic_fetch_add(&t.sum[2 * size + h], d2, MAP_RLX_AGENT);
            more(h, size);
            return true;
        }
        h = (h + 1) & mask;
    }
    return false;
}

__device__ __forceinline__ bool table_update(const MapTable& t, u64 key, u64 dn, u64 d0, u64 d1, u64 d2) {
    return table_update_and(t, key, dn, d0, d1, d2, [](u64, u64) {});
}
// The shaped form: nine more relaxed agent-scope adds, mom[w] += dm[w], behind the same claimed entry.
__device__ __forceinline__ bool table_update_shape(const MapShapeTable& t, u64 key, u64 dn, u64 d0, u64 d1, u64 d2, const u64* dm) {
    return table_update_and(t, key, dn, d0, d1, d2, [&](u64 h, u64 size) {
#pragma unroll
        for (int w = 0; w < icet_map_shape_rule::kWords; w++) __hip_atomic_fetch_add(&t.mom[w * size + h], dm[w], MAP_RLX_AGENT);
    });
}

}  // namespace
}  // namespace icet
