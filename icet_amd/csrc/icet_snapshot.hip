// icet_amd/csrc/icet_snapshot.hip -- a keyframe store's slots to and from the payloads of a snapshot file (include/icet_hip.h icet_keyframe_store_save /
// _load; the format: icet_snapshot.h).  k_snapshot_pack gathers the used part of each named slot -- n_slots SlotHot and SlotFit records,
// the slot_of_voxel row, descriptor, weights and grid where the slot has them -- into one contiguous payload in a staging buffer and sums the payload's
// checksum on the way; k_snapshot_unpack is the reverse.  Neither is ever captured into a graph; no block waits for another.
#include <hip/hip_runtime.h>
#include "icet_internal.h"
#include "icet_snapshot.h"

namespace icet {
namespace {

constexpr int kSnapBlock = 256;
constexpr int kSnapBlocksPerEntry = 8;      // blocks share a payload by 16-byte vectors: a chunk of a few slots still covers the device
static_assert(sizeof(SlotHot) == icet_snapshot::kHotBytes && sizeof(SlotFit) == icet_snapshot::kFitBytes, "the payload keeps the records as they are");

// Words first .. first + 3 of a row of n words (the rows of slot_of_voxel, descriptors and weights start on 4-byte boundaries only); zero behind the row.
__device__ __forceinline__ uint4 load_words(const uint32_t* row, uint32_t first, uint32_t n) {
    uint4 v;
    v.x = first < n ? row[first] : 0u; v.y = first + 1 < n ? row[first + 1] : 0u; v.z = first + 2 < n ? row[first + 2] : 0u; v.w = first + 3 < n ? row[first + 3] : 0u;
    return v;
}
__device__ __forceinline__ void store_words(uint32_t* row, uint32_t first, uint32_t n, const uint4& v) {
    if (first < n) row[first] = v.x;
    if (first + 1 < n) row[first + 1] = v.y;
    if (first + 2 < n) row[first + 2] = v.z;
    if (first + 3 < n) row[first + 3] = v.w;
}

// Where the 16 bytes at offset b of a slot's payload live in the store: part 0 hot, 1 fit, 5 grid (16-byte vectors, index vec); 2 slot_of_voxel, 3 descriptor,
// 4 weights (rows of words: first word, row length).
struct SnapPlace { int part; uint32_t vec, first, n; };
__device__ __forceinline__ SnapPlace snap_place(const icet_snapshot::Layout& l, uint32_t b) {
    SnapPlace p;
    if (b < l.fit) { p.part = 0; p.vec = b >> 4; p.first = 0; p.n = 0; }
    else if (b < l.sov) { p.part = 1; p.vec = (b - l.fit) >> 4; p.first = 0; p.n = 0; }
    else if (b < l.desc) { p.part = 2; p.vec = 0; p.first = (b - l.sov) >> 2; p.n = l.sov_bytes >> 2; }
    else if (b < l.w) { p.part = 3; p.vec = 0; p.first = (b - l.desc) >> 2; p.n = l.desc_bytes >> 2; }
    else if (b < l.grid) { p.part = 4; p.vec = 0; p.first = (b - l.w) >> 2; p.n = l.w_bytes >> 2; }
    else { p.part = 5; p.vec = (b - l.grid) >> 4; p.first = 0; p.n = 0; }
    return p;
}

// kSnapBlocksPerEntry blocks per entry.  Each lane moves 16-byte vectors of the payload and adds their two checksum terms; the terms are summed over the wave,
// then over the block, and one 64-bit integer atomic per block adds them into the entry's word: an integer sum is exact in any order.
__global__ __launch_bounds__(kSnapBlock) void k_snapshot_pack(SnapTables t, const SnapEntry* __restrict__ ent, uint8_t* __restrict__ stage,
                                                              unsigned long long* __restrict__ sums) {
    const int e = (int)blockIdx.x / kSnapBlocksPerEntry, share = (int)blockIdx.x % kSnapBlocksPerEntry;
    const size_t slot = (size_t)ent[e].slot;
    const icet_snapshot::Layout l = icet_snapshot::layout(t.V, ent[e].n_slots, ent[e].flags, t.A, t.Rp, t.G);
    const uint4* hot = reinterpret_cast<const uint4*>(t.hot + slot * t.V);
    const uint4* fit = reinterpret_cast<const uint4*>(t.fit + slot * t.V);
    const uint32_t* sov = reinterpret_cast<const uint32_t*>(t.sov + slot * (size_t)((t.V + 1) & ~1));
    const uint32_t* desc = t.desc + slot * (size_t)t.A * t.Rp;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(t.w) + slot * (size_t)t.A;
    const uint4* grid = reinterpret_cast<const uint4*>(t.grid + slot * ((size_t)t.G * t.G / 32));
    uint4* dst = reinterpret_cast<uint4*>(stage + ent[e].off);
    unsigned long long sum = 0;
    for (uint32_t i = (uint32_t)share * kSnapBlock + threadIdx.x; i < l.size / 16; i += kSnapBlocksPerEntry * kSnapBlock) {
        const SnapPlace p = snap_place(l, i * 16);
        uint4 v;
        switch (p.part) {
            case 0: v = hot[p.vec]; break;
            case 1: v = fit[p.vec]; break;
            case 2: v = load_words(sov, p.first, p.n); break;
            case 3: v = load_words(desc, p.first, p.n); break;
            case 4: v = load_words(w, p.first, p.n); break;
            default: v = grid[p.vec]; break;
        }
        dst[i] = v;
        sum += icet_snapshot::term((uint64_t)v.x | (uint64_t)v.y << 32, 2ull * i) + icet_snapshot::term((uint64_t)v.z | (uint64_t)v.w << 32, 2ull * i + 1);
    }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    __shared__ unsigned long long part[kSnapBlock / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int k = 0; k < kSnapBlock / 64; k++) s += part[k];
        atomicAdd(sums + e, s);
    }
}

// The reverse: payload e of the staging into row ent[e].slot of the store's tables -- n_slots, the used records (those behind stay as they are, as the park
// kernel leaves them), the slot_of_voxel row, descriptor / weights / grid and their "has" words (0 where the entry has none), stamp and pose (0xFF bytes
// where the entry has none).  Tables the store lacks are null: that part of the payload is skipped.
__global__ __launch_bounds__(kSnapBlock) void k_snapshot_unpack(SnapTables t, const SnapEntry* __restrict__ ent, const uint8_t* __restrict__ stage) {
    const int e = (int)blockIdx.x / kSnapBlocksPerEntry, share = (int)blockIdx.x % kSnapBlocksPerEntry;
    const size_t slot = (size_t)ent[e].slot;
    const uint32_t flags = ent[e].flags;
    const icet_snapshot::Layout l = icet_snapshot::layout(t.V, ent[e].n_slots, flags, t.A, t.Rp, t.G);
    uint4* hot = reinterpret_cast<uint4*>(t.hot + slot * t.V);
    uint4* fit = reinterpret_cast<uint4*>(t.fit + slot * t.V);
    uint32_t* sov = reinterpret_cast<uint32_t*>(t.sov + slot * (size_t)((t.V + 1) & ~1));
    uint32_t* desc = t.desc ? t.desc + slot * (size_t)t.A * t.Rp : nullptr;
    uint32_t* w = t.w ? reinterpret_cast<uint32_t*>(t.w) + slot * (size_t)t.A : nullptr;
    uint4* grid = t.grid ? reinterpret_cast<uint4*>(t.grid + slot * ((size_t)t.G * t.G / 32)) : nullptr;
    const uint4* src = reinterpret_cast<const uint4*>(stage + ent[e].off);
    for (uint32_t i = (uint32_t)share * kSnapBlock + threadIdx.x; i < l.size / 16; i += kSnapBlocksPerEntry * kSnapBlock) {
        const SnapPlace p = snap_place(l, i * 16);
        const uint4 v = src[i];
        switch (p.part) {
            case 0: hot[p.vec] = v; break;
            case 1: fit[p.vec] = v; break;
            case 2: store_words(sov, p.first, p.n, v); break;
            case 3: if (desc) store_words(desc, p.first, p.n, v); break;
            case 4: if (w) store_words(w, p.first, p.n, v); break;
            default: if (grid) grid[p.vec] = v; break;
        }
    }
    if (share == 0) {
        if (threadIdx.x < 12) t.pose[(size_t)threadIdx.x * t.cap + slot] = __uint_as_float(ent[e].pose[threadIdx.x]);
        if (threadIdx.x == 12) t.stamp[slot] = ent[e].stamp;
        if (threadIdx.x == 13) t.n_slots[slot] = ent[e].n_slots;
        if (threadIdx.x == 14 && t.app_has) t.app_has[slot] = (flags & icet_snapshot::kFlagDesc) ? 1 : 0;
        if (threadIdx.x == 15 && t.grid_has) t.grid_has[slot] = (flags & icet_snapshot::kFlagGrid) ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_snapshot_pack(const SnapTables& t, const SnapEntry* d_entries, int n_entries, uint8_t* d_stage, unsigned long long* d_sums, hipStream_t st) {
    if (n_entries <= 0) return hipSuccess;
    k_snapshot_pack<<<n_entries * kSnapBlocksPerEntry, kSnapBlock, 0, st>>>(t, d_entries, d_stage, d_sums);
    return hipGetLastError();
}

hipError_t launch_snapshot_unpack(const SnapTables& t, const SnapEntry* d_entries, int n_entries, const uint8_t* d_stage, hipStream_t st) {
    if (n_entries <= 0) return hipSuccess;
    k_snapshot_unpack<<<n_entries * kSnapBlocksPerEntry, kSnapBlock, 0, st>>>(t, d_entries, d_stage);
    return hipGetLastError();
}

}  // namespace icet
