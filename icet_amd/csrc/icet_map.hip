// icet_amd/csrc/icet_map.hip -- the voxel map of the C ABI (include/icet_hip.h icet_voxel_map_*): scans at poses fused into one centroid and
// one count per occupied cell, in an open-addressing hash table in HBM.  The rule -- which rows count, a row's key and offsets, a cell's centroid -- is
// icet_map.h; this file is the kernels around it and the entry points:
//     k_map_add       one launch for all scans of a call, blockIdx -> (scan, chunk of kRowsPerBlock rows), 16-byte loads of 4 consecutive rows per lane.  A lane
//                     first merges the equal keys among its own 4 rows; with kLds the block then reduces its rows in an LDS table of kLdsSlots cells (64-bit ds
//                     compare-and-swap on the key, ds adds on count and sums) and flushes every distinct cell ONCE with global 64-bit atomics; a cell that finds
//                     no LDS slot within kLdsProbes goes to the global table directly.  Without kLds (option "map_lds" 0): one global update per merged run.
//     k_map_cells     a pass over the entries, 16 per thread: <false> counts the cells with count > 0, count >= min_points, count < 0 (tallied in LDS, one
//                     atomic per block and counter); <true> compacts (key, entry) of the cells with count >= min_points (a block claims its places with one atomic)
//     k_map_centroid  one thread per output row, behind rocPRIM's device radix sort of the pairs by key
//     k_map_shape     (a shaped map: icet_voxel_map_enable_shape; the rule: icet_map_shape.h) one thread per output row behind k_map_centroid:
//                     the cell's nine integer moment words, its covariance in double, six Jacobi sweeps for the eigenvalues and the normal.  k_map_add<., true>
//                     carries the nine words beside the three sums through the run merge, the LDS table (kLdsSlotsShape cells), the flush and the direct path
// and the query (icet_voxel_map_query_*; the rule: icet_map_query.h) over the INDEX, the extract's sequence kept as sorted arrays:
//     k_map_query_count   a block reads a chunk of kQueryChunk consecutive cells once and tests them against every pose of the call (poses in LDS, wave64 ballots
//                         and popcounts): one int32 per (query, chunk).  A query whose run of x cells misses the chunk's is not tested (option "map_query_prune")
//     k_map_query_scan    one block per query: exclusive offsets of its chunks, and d_rows / d_total / d_status
//     k_map_query_write   the test again; a kept cell's rank is chunk offset + wave prefix + lane prefix, so the rows keep the index order, which is key order
// and the visibility evidence (icet_voxel_map_evidence_*; the rule: icet_map_evidence.h), per cell of the index, from scans in batches:
//     k_map_image         the add's table and loads; a row's octahedral pixel and range word, one 32-bit atomicMin per run of equal pixels among a lane's 4 rows
//     k_map_image_near    one thread per pixel: the minimum over the pixel's window
//     k_map_evidence      the query's chunks and load shape; the batch's poses in LDS, a block-uniform loop over its scans (pruned by their run of x cells), one
//                         gather from the near image per (cell, scan), two counters per cell added to miss[] / agree[] with plain stores
//     k_map_evidence_decide   the transient byte per cell, which the <true> instantiations of the two query kernels read (ICET_VOXEL_MAP_QUERY_STATIC)
// The host side shares two pieces: CallStage, a call's records and poses (pinned, then on the device, behind a read fence), for an add's scan descriptors and a query's
// sub-map descriptors; and map_sorted_cells (size query, growth, select, sort), which the extract and the index each run over a SortedCells of their own.
// Sums of integers only: no float atomic, no block waits for another block, no fence inside a kernel, and the contents do not depend on the launch shape.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "../../include/icet_hip.h"
#include "icet_ctx.h"
#include "icet_staging.h"
#include "icet_map.h"
#include "icet_map_query.h"
#include "icet_map_evidence.h"
#include "icet_map_shape.h"
#include "icet_map_table.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>

namespace icet {
namespace {

namespace rule = icet_map_rule;
namespace qrule = icet_map_query_rule;
namespace erule = icet_map_evidence_rule;
namespace srule = icet_map_shape_rule;
constexpr int kAddBlock = 256;
constexpr int kRowsPerBlock = 2048;      // a block's chunk of one scan: two trips of 256 lanes x 4 rows
constexpr int kLdsSlots = 1024;          // 36 KB of LDS: key 8 | sums 24 | count 4 bytes per slot
constexpr int kLdsSlotsShape = 512;      // a shaped block: 48 KB, key 8 | sums 24 | count 4 | S 12 (32-bit: 2048 rows x 65535 < 2^27) | M 48 bytes per slot
constexpr int kLdsProbes = 8;
constexpr int kCellBlock = 256;
constexpr int kCellPer = 16;            // entries per thread of a pass over the table
constexpr int kCellSpan = kCellBlock * kCellPer;
constexpr int kQueryBlock = 256;         // a query block: 4 waves, each with kQueryTrips trips of 64 consecutive cells of the index
constexpr int kQueryWaves = kQueryBlock / 64;
constexpr int kQueryTrips = 8;
constexpr int kQueryPerWave = 64 * kQueryTrips;
constexpr int kQueryChunk = kQueryWaves * kQueryPerWave;
static_assert(kQueryChunk == ICET_VOXEL_MAP_QUERY_CHUNK, "the chunk the header names");
static_assert(qrule::kMaxQueries <= kQueryBlock && qrule::kMaxQueries == ICET_VOXEL_MAP_MAX_QUERIES, "a block stages the call's poses in one step per thread");

struct MapScan { const float* ptr; int32_t n, ld, block0, pad; };      // block0: the first block of the scan in the launch
static_assert(sizeof(MapScan) == 24, "ptr | n | ld | block0 | pad");
// MapTable / MapShapeTable, the device record's words (kCtr*) and table_update / table_update_shape: icet_map_table.h, shared with icet_map_snapshot.hip

// m <= 4 rows of one column from row i (a multiple of 4): one 16-byte load where the column's address allows it and all four rows exist.
__device__ __forceinline__ void load_rows(const float* __restrict__ col, int i, int m, float v[4]) {
    const float* p = col + i;
    if (m == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        for (int r = 0; r < 4; r++) v[r] = r < m ? p[r] : 0.f;
    }
}

// kShape: the nine moment words travel with the three sums through every stage -- the lane's run, the LDS table (32-bit S, 64-bit M), the flush and the direct
// path.  Every shaped statement is behind `if constexpr` and the plain kernels take the plain table: the <., false> instantiations are the kernel without shape.
template <bool kLds, bool kShape>
__global__ __launch_bounds__(kAddBlock) void k_map_add(const MapScan* __restrict__ scans, int n_scans, const float* __restrict__ poses, rule::Consts kc, TableOf<kShape> t,
                                                       u64 sign, u64* __restrict__ ctr) {
    constexpr int kSlots = kLds ? (kShape ? kLdsSlotsShape : kLdsSlots) : 1;
    __shared__ u64 lkey[kSlots];
    __shared__ u64 lsum[3][kSlots];
    __shared__ uint32_t lcnt[kSlots];
    __shared__ uint32_t lS[3][kShape ? kSlots : 1];
    __shared__ u64 lM[6][kShape ? kSlots : 1];
    __shared__ uint32_t lctr[5];
    __shared__ float sT[12];
    // the scan of this block: the last one whose first block is not behind it (a scan without rows has no block)
    int lo = 0, hi = n_scans - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (scans[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const MapScan sc = scans[lo];
    const int row0 = ((int)blockIdx.x - sc.block0) * kRowsPerBlock;
    if (row0 < 0 || row0 >= sc.n) return;                             // (the same for every thread of the block)
    const int end = min(sc.n, row0 + kRowsPerBlock);
    if (kLds) for (int s = threadIdx.x; s < kSlots; s += kAddBlock) {
        lkey[s] = rule::kEmpty; lsum[0][s] = 0; lsum[1][s] = 0; lsum[2][s] = 0; lcnt[s] = 0u;
        if constexpr (kShape) { for (int a = 0; a < 3; a++) lS[a][s] = 0u; for (int j = 0; j < 6; j++) lM[j][s] = 0; }
    }
    if (threadIdx.x < 5) lctr[threadIdx.x] = 0u;
    if (threadIdx.x < 12) sT[threadIdx.x] = poses[16 * (size_t)lo + threadIdx.x];
    __syncthreads();
    const float* cx = sc.ptr; const float* cy = cx + sc.ld; const float* cz = cx + 2 * (size_t)sc.ld;
    uint32_t n_in = 0, n_kept = 0, n_nonfinite = 0, n_outside = 0, n_dropped = 0;

    // a run of rows of one cell: into the block's LDS table, or the global table.  rS / rM: the run's moment words (kShape; a run is at most 4 rows)
    auto push = [&](u64 key, uint32_t c, u64 s0, u64 s1, u64 s2, const uint32_t* rS, const u64* rM) {
        if (kLds) {
            uint32_t s = (uint32_t)(rule::mix(key) >> 40) & (kSlots - 1);
            for (int p = 0; p < kLdsProbes; p++) {
                u64 expected = rule::kEmpty;
                if (__hip_atomic_compare_exchange_strong(&lkey[s], &expected, key, __ATOMIC_RELAXED, MAP_RLX_WG) || expected == key) {
                    __hip_atomic_fetch_add(&lcnt[s], c, MAP_RLX_WG);
                    __hip_atomic_fetch_add(&lsum[0][s], s0, MAP_RLX_WG);
                    __hip_atomic_fetch_add(&lsum[1][s], s1, MAP_RLX_WG);
                    __hip_atomic_fetch_add(&lsum[2][s], s2, MAP_RLX_WG);
                    if constexpr (kShape) {
#pragma unroll
                        for (int a = 0; a < 3; a++) __hip_atomic_fetch_add(&lS[a][s], rS[a], MAP_RLX_WG);
#pragma unroll
                        for (int j = 0; j < 6; j++) __hip_atomic_fetch_add(&lM[j][s], rM[j], MAP_RLX_WG);
                    }
                    return;
                }
                s = (s + 1) & (kSlots - 1);
            }
        }
        if constexpr (kShape) {
            u64 dm[srule::kWords];
#pragma unroll
            for (int a = 0; a < 3; a++) dm[a] = sign * (u64)rS[a];
#pragma unroll
            for (int j = 0; j < 6; j++) dm[3 + j] = sign * rM[j];
            if (table_update_shape(t, key, sign * c, sign * s0, sign * s1, sign * s2, dm)) n_kept += c; else n_dropped += c;
        } else {
            if (table_update(t, key, sign * c, sign * s0, sign * s1, sign * s2)) n_kept += c; else n_dropped += c;
        }
    };

    for (int i = row0 + 4 * (int)threadIdx.x; i < end; i += 4 * kAddBlock) {
        const int m = min(4, end - i);
        float x[4], y[4], z[4];
        load_rows(cx, i, m, x); load_rows(cy, i, m, y); load_rows(cz, i, m, z);
        n_in += (uint32_t)m;
        u64 run_key = rule::kEmpty, r0 = 0, r1 = 0, r2 = 0; uint32_t run = 0;
        uint32_t rS[3] = {0u, 0u, 0u}; u64 rM[6] = {0, 0, 0, 0, 0, 0};
        for (int r = 0; r < m; r++) {
            rule::Point pt;
            const int cls = rule::classify(kc, sT, x[r], y[r], z[r], pt);
            if (cls == rule::kRowNonfinite) n_nonfinite++;
            if (cls == rule::kRowOutside) n_outside++;
            if (cls != rule::kRowKept) continue;
            if (run && pt.key != run_key) {
                push(run_key, run, r0, r1, r2, rS, rM); run = 0; r0 = 0; r1 = 0; r2 = 0;
                if constexpr (kShape) { for (int a = 0; a < 3; a++) rS[a] = 0u; for (int j = 0; j < 6; j++) rM[j] = 0; }
            }
            run_key = pt.key; run++; r0 += pt.q[0]; r1 += pt.q[1]; r2 += pt.q[2];
            if constexpr (kShape) {
                uint32_t hS[3], hM[6];
                srule::row_moments(pt.q, hS, hM);
#pragma unroll
                for (int a = 0; a < 3; a++) rS[a] += hS[a];
#pragma unroll
                for (int j = 0; j < 6; j++) rM[j] += hM[j];
            }
        }
        if (run) push(run_key, run, r0, r1, r2, rS, rM);
    }
    if (kLds) {
        __syncthreads();
        for (int s = threadIdx.x; s < kSlots; s += kAddBlock) {
            const u64 key = lkey[s];
            if (key == rule::kEmpty) continue;
            const uint32_t c = lcnt[s];
            if constexpr (kShape) {
                u64 dm[srule::kWords];
#pragma unroll
                for (int a = 0; a < 3; a++) dm[a] = sign * (u64)lS[a][s];
#pragma unroll
                for (int j = 0; j < 6; j++) dm[3 + j] = sign * lM[j][s];
                if (table_update_shape(t, key, sign * c, sign * lsum[0][s], sign * lsum[1][s], sign * lsum[2][s], dm)) n_kept += c; else n_dropped += c;
            } else {
                if (table_update(t, key, sign * c, sign * lsum[0][s], sign * lsum[1][s], sign * lsum[2][s])) n_kept += c; else n_dropped += c;
            }
        }
    }
    if (n_in) atomicAdd(&lctr[0], n_in);
    if (n_kept) atomicAdd(&lctr[1], n_kept);
    if (n_nonfinite) atomicAdd(&lctr[2], n_nonfinite);
    if (n_outside) atomicAdd(&lctr[3], n_outside);
    if (n_dropped) atomicAdd(&lctr[4], n_dropped);
    __syncthreads();
    if (threadIdx.x < 5 && lctr[threadIdx.x]) {
        const u64 v = lctr[threadIdx.x];
        __hip_atomic_fetch_add(&ctr[(blockIdx.x % kTotCopies) * kTotWords + threadIdx.x], threadIdx.x == kCtrKept ? sign * v : v, MAP_RLX_AGENT);
    }
}

// A block walks kCellSpan entries, kCellPer per thread.  Threads tally in LDS and the block touches the device record once per counter: every block of the
// grid adds to the same few words, and adders on one address are what memory-side atomics do worst.  select: the cells of count >= minp are written as
// (key, entry) at places the block claims with one atomic (the order of the places is free: the pairs are sorted next); else they are only counted.
template <bool kSelect>
__global__ __launch_bounds__(kCellBlock) void k_map_cells(MapTable t, long long minp, u64* __restrict__ ctr, u64* __restrict__ sel_key, uint32_t* __restrict__ sel_idx, u64 cap) {
    __shared__ uint32_t tally[3];
    __shared__ u64 base;
    const u64 size = (u64)1 << t.log2, first = (u64)blockIdx.x * kCellSpan + threadIdx.x;      // the grid covers the entries; a table below kCellSpan is one block
    if (threadIdx.x < 3) tally[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t n_out = 0, n_occ = 0, n_neg = 0, mask = 0;
#pragma unroll
    for (int j = 0; j < kCellPer; j++) {
        const u64 i = first + (u64)j * kCellBlock;
        if (i >= size) break;
        const long long c = (long long)t.count[i];
        if (c >= minp) { n_out++; mask |= 1u << j; }
        n_occ += c > 0; n_neg += c < 0;
    }
    if (kSelect) {
        uint32_t at = 0;
        if (n_out) at = atomicAdd(&tally[0], n_out);
        __syncthreads();
        if (threadIdx.x == 0 && tally[0]) base = __hip_atomic_fetch_add(&ctr[kCtrSelected], (u64)tally[0], MAP_RLX_AGENT);
        __syncthreads();
        if (!n_out) return;
        u64 pos = base + at;
        for (int j = 0; j < kCellPer; j++) {
            if (!((mask >> j) & 1u)) continue;
            const u64 i = first + (u64)j * kCellBlock;
            if (pos < cap) { sel_key[pos] = t.key[i]; sel_idx[pos] = (uint32_t)i; }      // (cap: the count pass's cells_out, on the same stream)
            pos++;
        }
    } else {
        if (n_occ) atomicAdd(&tally[0], n_occ);
        if (n_out) atomicAdd(&tally[1], n_out);
        if (n_neg) atomicAdd(&tally[2], n_neg);
        __syncthreads();
        if (threadIdx.x < 3 && tally[threadIdx.x]) __hip_atomic_fetch_add(&ctr[kCtrOccupied + threadIdx.x], (u64)tally[threadIdx.x], MAP_RLX_AGENT);
    }
}

// Row i of the output: the centroid, count and key of the cell with the i-th lowest key.
__global__ __launch_bounds__(kCellBlock) void k_map_centroid(MapTable t, rule::Consts kc, const u64* __restrict__ keys, const uint32_t* __restrict__ idx, long long rows,
                                                             float* __restrict__ xyz, long long ld, long long* __restrict__ d_count, u64* __restrict__ d_key) {
    const long long i = (long long)blockIdx.x * kCellBlock + threadIdx.x;
    if (i >= rows) return;
    const u64 key = keys[i];
    const u64 e = idx[i], size = (u64)1 << t.log2;                    // e < size: k_map_select wrote an entry's index
    const long long n = (long long)t.count[e];
    int32_t c[3];
    rule::key_cells(key, c);
    for (int a = 0; a < 3; a++) xyz[a * ld + i] = rule::centroid(kc, c[a], t.sum[a * size + e], n);
    if (d_count) d_count[i] = n;
    if (d_key) d_key[i] = key;
}

// The shape of row i, behind k_map_centroid over the same sorted cells: the nine words of the cell, its covariance, its eigenvalues and
// its normal.  Any of the four outputs may be null; all are column-major over ld.
struct MapShapeOut { float* cov; float* normal; float* evals; u64* moments; long long ld; };
__global__ __launch_bounds__(kCellBlock) void k_map_shape(MapShapeTable t, srule::Consts kc, const uint32_t* __restrict__ idx, long long rows, MapShapeOut o) {
    const long long i = (long long)blockIdx.x * kCellBlock + threadIdx.x;
    if (i >= rows) return;
    const u64 e = idx[i], size = (u64)1 << t.log2;                    // e < size: an entry's index, as in k_map_centroid
    const long long n = (long long)t.count[e];
    uint64_t w[srule::kWords];
#pragma unroll
    for (int j = 0; j < srule::kWords; j++) w[j] = t.mom[j * size + e];
    if (o.moments) {
#pragma unroll
        for (int j = 0; j < srule::kWords; j++) o.moments[j * o.ld + i] = w[j];      // i < rows <= cap_rows <= ld: inside the caller's columns
    }
    if (!o.cov && !o.normal && !o.evals) return;
    double C[6];
    srule::cov(kc, n, w, C);
    if (o.cov) {
#pragma unroll
        for (int j = 0; j < 6; j++) o.cov[j * o.ld + i] = (float)C[j];
    }
    if (!o.normal && !o.evals) return;
    float ev[3], nm[3];
    srule::eigen(C, ev, nm);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (o.evals) o.evals[a * o.ld + i] = ev[a];
        if (o.normal) o.normal[a * o.ld + i] = nm[a];
    }
}

// ---- the query: sub-maps around poses, out of the sorted index ---------------------------------------------------------------------------
// The index: the cells of count >= 1 by ascending key, as contiguous arrays.  xyz: three columns of `ld` floats.
// trans: the evidence's decision per cell (section 23), read by the STATIC instantiations of the query kernels only.
struct MapIndex { const u64* key; const long long* count; const float* xyz; long long ld, n; const uint8_t* trans; };
// A query's outputs as the device reads them (icet_voxel_map_submap, word for word).
struct MapSubmap { float* xyz; long long ld, cap_rows; long long* count; u64* key; };
static_assert(sizeof(MapSubmap) == sizeof(icet_voxel_map_submap) && sizeof(MapSubmap) == 40, "xyz | ld | cap_rows | count | key");

// What a block knows of the call's queries: the poses, and the run of x cells each can reach (empty for an unusable pose).
struct QueryLds {
    float T[qrule::kMaxQueries][12];
    int32_t lo[qrule::kMaxQueries], hi[qrule::kMaxQueries];
    int32_t wcnt[qrule::kMaxQueries][kQueryWaves];                    // kept cells per (query, wave) of this block's chunk
};
// The cells of one lane: wave w of the block owns cells [w kQueryPerWave, (w + 1) kQueryPerWave) of the chunk, lane l the cells j * 64 + l of those, so that a
// (trip j, lane) order within a wave and the wave order within the block are the index order.
struct QueryCells { float m[kQueryTrips][3]; long long n[kQueryTrips]; };

__device__ __forceinline__ void query_setup(QueryLds& s, const float* __restrict__ poses, int n_q, const qrule::Consts& kc, bool prune) {
    for (int q = threadIdx.x; q < n_q; q += kQueryBlock) {
        for (int j = 0; j < 12; j++) s.T[q][j] = poses[16 * (size_t)q + j];
        qrule::x_interval(kc, s.T[q], prune, s.lo[q], s.hi[q]);
    }
}
template <bool kStatic> __device__ __forceinline__ void query_load(const MapIndex& ix, long long first, QueryCells& c) {
#pragma unroll
    for (int j = 0; j < kQueryTrips; j++) {
        const long long i = first + j * 64;
        bool in = i < ix.n;                                            // a cell behind the index: count 0 takes part in nothing
        if (kStatic) in = in && ix.trans[i] == 0;                      // (ICET_VOXEL_MAP_QUERY_STATIC) nor does a transient cell
        c.n[j] = in ? ix.count[i] : 0;
        for (int a = 0; a < 3; a++) c.m[j][a] = in ? ix.xyz[a * ix.ld + i] : 0.f;
    }
}
// What the count and the write begin with: the run of x cells the block's chunk spans, the call's queries into LDS, the lane's cells into registers.  Returns the
// lane's first cell.  The grid is the chunks of the index, so the chunk's first cell is < ix.n.
template <bool kStatic> __device__ __forceinline__ long long query_begin(QueryLds& s, QueryCells& c, const MapIndex& ix, const float* __restrict__ poses, int n_q, const qrule::Consts& kc, int prune, int32_t& x_first, int32_t& x_last) {
    const long long chunk0 = (long long)blockIdx.x * kQueryChunk, first = chunk0 + (threadIdx.x >> 6) * kQueryPerWave + (threadIdx.x & 63);
    x_first = qrule::key_x(ix.key[chunk0]); x_last = qrule::key_x(ix.key[min(chunk0 + kQueryChunk, ix.n) - 1]);
    query_setup(s, poses, n_q, kc, prune != 0);
    query_load<kStatic>(ix, first, c);
    return first;
}
// Kept cells of this wave per query of the call, into s.wcnt.  A query whose run of x cells misses the chunk's keeps none of its cells and is not tested.
__device__ __forceinline__ void query_count(QueryLds& s, const QueryCells& c, int n_q, const qrule::Consts& kc, int32_t x_first, int32_t x_last) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = 0; q < n_q; q++) {
        int32_t kept = 0;
        if (s.lo[q] <= x_last && s.hi[q] >= x_first) {                // (the same for every thread of the block)
#pragma unroll
            for (int j = 0; j < kQueryTrips; j++) {
                double d[3];
                kept += __popcll(__ballot(qrule::keep(kc, s.T[q], c.m[j][0], c.m[j][1], c.m[j][2], c.n[j], d)));
            }
        }
        if (lane == 0) s.wcnt[q][wave] = kept;
    }
}

// One int32 per (query, chunk): counts[q * n_chunks + chunk].
template <bool kStatic> __global__ __launch_bounds__(kQueryBlock) void k_map_query_count(MapIndex ix, const float* __restrict__ poses, int n_q, qrule::Consts kc, int prune,
                                                                 int32_t* __restrict__ counts, long long n_chunks) {
    __shared__ QueryLds s;
    QueryCells c; int32_t x_first, x_last;
    query_begin<kStatic>(s, c, ix, poses, n_q, kc, prune, x_first, x_last);
    __syncthreads();
    query_count(s, c, n_q, kc, x_first, x_last);
    __syncthreads();
    for (int q = threadIdx.x; q < n_q; q += kQueryBlock) {
        int32_t t = 0;
        for (int w = 0; w < kQueryWaves; w++) t += s.wcnt[q][w];
        counts[(long long)q * n_chunks + blockIdx.x] = t;
    }
}

// One block per query: counts[q][*] -> offs[q][*] (exclusive), and the query's three words.  A thread owns a run of consecutive chunks.
__global__ __launch_bounds__(kQueryBlock) void k_map_query_scan(const int32_t* __restrict__ counts, int32_t* __restrict__ offs, long long n_chunks, const float* __restrict__ poses,
                                                                const MapSubmap* __restrict__ outs, int32_t* __restrict__ d_rows, int32_t* __restrict__ d_total,
                                                                int32_t* __restrict__ d_status) {
    __shared__ int32_t part[kQueryBlock];
    const int q = blockIdx.x;
    const long long per = (n_chunks + kQueryBlock - 1) / kQueryBlock, b = min(n_chunks, (long long)threadIdx.x * per), e = min(n_chunks, b + per);
    const int32_t* cq = counts + (long long)q * n_chunks;
    int32_t* oq = offs + (long long)q * n_chunks;
    int32_t mine = 0;
    for (long long i = b; i < e; i++) mine += cq[i];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int step = 1; step < kQueryBlock; step <<= 1) {              // inclusive scan of the 256 partial sums
        const int32_t v = (int)threadIdx.x >= step ? part[threadIdx.x - step] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int32_t run = part[threadIdx.x] - mine;
    for (long long i = b; i < e; i++) { oq[i] = run; run += cq[i]; }
    if (threadIdx.x == 0) {
        const long long total = part[kQueryBlock - 1], cap = outs[q].cap_rows;
        float T[12];
        for (int j = 0; j < 12; j++) T[j] = poses[16 * (size_t)q + j];
        d_rows[q] = (int32_t)min(total, cap);
        if (d_total) d_total[q] = (int32_t)total;
        if (d_status) d_status[q] = (qrule::pose_ok(T) ? 0 : ICET_VOXEL_MAP_QUERY_BAD_POSE) | (total > cap ? ICET_VOXEL_MAP_TRUNCATED : 0);
    }
}

// The test again, and the rows: a kept cell's rank is its chunk's offset + the kept cells of the waves before its own + those of its wave's earlier trips +
// those of the lanes below it in its trip's ballot -- the index order.  Ranks from cap_rows on are not written.
template <bool kStatic> __global__ __launch_bounds__(kQueryBlock) void k_map_query_write(MapIndex ix, const float* __restrict__ poses, int n_q, qrule::Consts kc, int prune,
                                                                 const int32_t* __restrict__ counts, const int32_t* __restrict__ offs, long long n_chunks,
                                                                 const MapSubmap* __restrict__ outs) {
    __shared__ QueryLds s;
    QueryCells c; int32_t x_first, x_last;
    const long long first = query_begin<kStatic>(s, c, ix, poses, n_q, kc, prune, x_first, x_last);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = threadIdx.x; q < n_q; q += kQueryBlock) {            // (the thread that staged query q) no row of q comes from this chunk: as if pruned
        const long long at = (long long)q * n_chunks + blockIdx.x;
        if (counts[at] == 0 || offs[at] >= outs[q].cap_rows) { s.lo[q] = rule::kCellLimit; s.hi[q] = -rule::kCellLimit; }
    }
    __syncthreads();
    query_count(s, c, n_q, kc, x_first, x_last);
    __syncthreads();
    for (int q = 0; q < n_q; q++) {
        if (!(s.lo[q] <= x_last && s.hi[q] >= x_first)) continue;     // (the same for every thread of the block)
        const MapSubmap o = outs[q];
        long long rank0 = offs[(long long)q * n_chunks + blockIdx.x];
        for (int w = 0; w < wave; w++) rank0 += s.wcnt[q][w];
#pragma unroll
        for (int j = 0; j < kQueryTrips; j++) {
            double d[3];
            const bool kept = qrule::keep(kc, s.T[q], c.m[j][0], c.m[j][1], c.m[j][2], c.n[j], d);
            const u64 mask = __ballot(kept);
            const long long rank = rank0 + __popcll(mask & (((u64)1 << lane) - 1));
            rank0 += __popcll(mask);
            if (!kept || rank >= o.cap_rows) continue;                // rank < cap_rows <= ld: inside the caller's columns
            for (int a = 0; a < 3; a++) o.xyz[a * o.ld + rank] = kc.world ? c.m[j][a] : qrule::row(s.T[q], d, a);
            if (o.count) o.count[rank] = c.n[j];
            if (o.key) o.key[rank] = ix.key[first + j * 64];           // (kept: the cell exists)
        }
    }
}

// ---- the visibility evidence: per cell of the index, how many scans saw through it and how many saw it ----------------------------------
// A batch of scans has two images per scan, img and near, of W x W range words each; scan k of the batch owns words [k W^2, (k + 1) W^2) of both.

// One launch for the scans of a batch, with the add's table and its loads: each row makes one 32-bit atomicMin on its pixel, after a lane has merged the equal
// pixels among its four consecutive rows (the rows of a ring often share one).  ctr[0] += the rows that entered an image, once per block.
__global__ __launch_bounds__(kAddBlock) void k_map_image(const MapScan* __restrict__ scans, int n_scans, erule::Consts kc, uint32_t* __restrict__ img, u64* __restrict__ ctr) {
    __shared__ uint32_t tally;
    int lo = 0, hi = n_scans - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (scans[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const MapScan sc = scans[lo];
    const int row0 = ((int)blockIdx.x - sc.block0) * kRowsPerBlock;
    if (row0 < 0 || row0 >= sc.n) return;                             // (the same for every thread of the block)
    const int end = min(sc.n, row0 + kRowsPerBlock);
    if (threadIdx.x == 0) tally = 0u;
    __syncthreads();
    uint32_t* im = img + ((size_t)lo << (2 * kc.w_log2));
    const float* cx = sc.ptr; const float* cy = cx + sc.ld; const float* cz = cx + 2 * (size_t)sc.ld;
    uint32_t rows = 0;
    for (int i = row0 + 4 * (int)threadIdx.x; i < end; i += 4 * kAddBlock) {
        const int m = min(4, end - i);
        float x[4], y[4], z[4];
        load_rows(cx, i, m, x); load_rows(cy, i, m, y); load_rows(cz, i, m, z);
        int32_t run_pix = -1; uint32_t run_word = erule::kEmptyPixel;
        for (int r = 0; r < m; r++) {
            int32_t pix; uint32_t word;
            if (!erule::row_pixel(kc, x[r], y[r], z[r], pix, word)) continue;      // 0 <= pix < W^2: the rule clamps u and v
            rows++;
            if (pix != run_pix) {
                if (run_pix >= 0) atomicMin(&im[run_pix], run_word);
                run_pix = pix; run_word = word;
            } else {
                run_word = min(run_word, word);
            }
        }
        if (run_pix >= 0) atomicMin(&im[run_pix], run_word);
    }
    if (rows) atomicAdd(&tally, rows);
    __syncthreads();
    if (threadIdx.x == 0 && tally) __hip_atomic_fetch_add(&ctr[0], (u64)tally, MAP_RLX_AGENT);
}

// One thread per pixel of every image of the batch: the minimum over the pixel's window.
__global__ __launch_bounds__(kCellBlock) void k_map_image_near(const uint32_t* __restrict__ img, uint32_t* __restrict__ near, erule::Consts kc, long long total) {
    const long long i = (long long)blockIdx.x * kCellBlock + threadIdx.x;
    if (i >= total) return;
    const int32_t pix = (int32_t)(i & (((long long)1 << (2 * kc.w_log2)) - 1));
    near[i] = erule::near_word(kc, img + (i - pix), pix & (kc.width - 1), pix >> kc.w_log2);
}

struct EvidenceLds { float T[erule::kMaxBatch][12]; int32_t lo[erule::kMaxBatch], hi[erule::kMaxBatch]; };

// The grid is the chunks of the index, with the query's load shape: a lane holds its kQueryTrips cells in registers and reads them once.  The batch's poses are
// staged in LDS; the loop over the scans is block-uniform, and a scan whose run of x cells misses the chunk's is skipped (an unusable pose reaches no cell).  Per
// (cell, scan): one gather from the scan's near image and two counters.  A cell has one owner and the batches follow each other on the stream, so the sums are
// plain loads and stores: no atomics on global memory, no block waits for another.
__global__ __launch_bounds__(kQueryBlock) void k_map_evidence(MapIndex ix, const float* __restrict__ poses, int n_s, erule::Consts kc, int prune,
                                                              const uint32_t* __restrict__ near, int32_t* __restrict__ miss, int32_t* __restrict__ agree) {
    __shared__ EvidenceLds s;
    QueryCells c;
    const long long chunk0 = (long long)blockIdx.x * kQueryChunk, first = chunk0 + (threadIdx.x >> 6) * kQueryPerWave + (threadIdx.x & 63);
    const int32_t x_first = qrule::key_x(ix.key[chunk0]), x_last = qrule::key_x(ix.key[min(chunk0 + kQueryChunk, ix.n) - 1]);
    for (int q = threadIdx.x; q < n_s; q += kQueryBlock) {
        for (int j = 0; j < 12; j++) s.T[q][j] = poses[16 * (size_t)q + j];
        erule::x_interval(kc, s.T[q], prune != 0, s.lo[q], s.hi[q]);
    }
    query_load<false>(ix, first, c);
    __syncthreads();
    int32_t n_miss[kQueryTrips], n_agree[kQueryTrips];
#pragma unroll
    for (int j = 0; j < kQueryTrips; j++) { n_miss[j] = 0; n_agree[j] = 0; }
    for (int q = 0; q < n_s; q++) {
        if (!(s.lo[q] <= x_last && s.hi[q] >= x_first)) continue;     // (the same for every thread of the block)
        const uint32_t* nq = near + ((size_t)q << (2 * kc.w_log2));
#pragma unroll
        for (int j = 0; j < kQueryTrips; j++) {
            int32_t pix; double d2;
            if (c.n[j] <= 0 || !erule::cell_pixel(kc, s.T[q], c.m[j][0], c.m[j][1], c.m[j][2], pix, d2)) continue;
            const int cls = erule::cell_class(kc, d2, nq[pix]);       // 0 <= pix < W^2
            n_miss[j] += cls == erule::kMiss; n_agree[j] += cls == erule::kAgree;
        }
    }
#pragma unroll
    for (int j = 0; j < kQueryTrips; j++) {
        const long long i = first + j * 64;
        if (i >= ix.n || !(n_miss[j] | n_agree[j])) continue;
        miss[i] += n_miss[j]; agree[i] += n_agree[j];
    }
}

// Behind the last batch: the decision per cell, ctr[1] += the transient cells (tallied per block, one atomic per block), and block 0 counts the call's
// unusable poses into ctr[2].
__global__ __launch_bounds__(kCellBlock) void k_map_evidence_decide(const int32_t* __restrict__ miss, const int32_t* __restrict__ agree, uint8_t* __restrict__ trans, long long n,
                                                                    erule::Consts kc, const float* __restrict__ poses, int n_s, u64* __restrict__ ctr) {
    __shared__ uint32_t tally[2];
    if (threadIdx.x < 2) tally[threadIdx.x] = 0u;
    __syncthreads();
    const long long i = (long long)blockIdx.x * kCellBlock + threadIdx.x;
    bool t = false;
    if (i < n) { t = erule::transient(kc, miss[i], agree[i]); trans[i] = t ? 1 : 0; }
    const int in_wave = __popcll(__ballot(t));
    if ((threadIdx.x & 63) == 0 && in_wave) atomicAdd(&tally[0], (uint32_t)in_wave);
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < n_s; k += kCellBlock) {
            float T[12];
            for (int j = 0; j < 12; j++) T[j] = poses[16 * (size_t)k + j];
            if (!qrule::pose_ok(T)) atomicAdd(&tally[1], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (tally[0]) __hip_atomic_fetch_add(&ctr[1], (u64)tally[0], MAP_RLX_AGENT);
        if (blockIdx.x == 0) ctr[2] = tally[1];
    }
}

}  // namespace
}  // namespace icet

using namespace icet;

// THE STAGE OF A CALL: n records of Rec and n poses of 16 floats, each pinned and then copied to the device.  The host writes the pinned side only behind the
// fence, which the call marks behind its last kernel; a call that reads poses the caller left on the device stages the records alone.
template <class Rec> struct CallStage {
    Rec* h_rec = nullptr; Rec* d_rec = nullptr; float* h_pose = nullptr; float* d_pose = nullptr; int32_t cap = 0;
    ReadFence fence; BufferGroup mem;
    ~CallStage() { fence.destroy(); }
    // A call of n begins: the previous call has read the staging; n above the capacity drains the stream (its kernels may still read the device side) and grows.
    hipError_t begin(int32_t n, hipStream_t st) {
        hipError_t e = fence.wait();
        if (e == hipSuccess && n > cap) e = hipStreamSynchronize(st);
        if (e != hipSuccess || n <= cap) return e;
        return static_cast<hipError_t>(grow(mem, cap, n, [&] {
            int a = mem.pinned(h_rec, (size_t)n);
            if (!a) a = mem.device(d_rec, (size_t)n);
            if (!a) a = mem.pinned(h_pose, 16 * (size_t)n);
            if (!a) a = mem.device(d_pose, 16 * (size_t)n);
            return a;
        }));
    }
    // h_rec[0 .. n) is written: the records to the device, and host poses with them.  *dp: the poses as the kernels read them.
    hipError_t upload(int32_t n, const float* poses, bool poses_on_device, hipStream_t st, const float** dp) {
        *dp = poses_on_device ? poses : d_pose;
        const hipError_t e = hipMemcpyAsync(d_rec, h_rec, sizeof(Rec) * (size_t)n, hipMemcpyHostToDevice, st);
        if (e != hipSuccess || poses_on_device) return e;
        std::memcpy(h_pose, poses, sizeof(float) * 16 * (size_t)n);
        return hipMemcpyAsync(d_pose, h_pose, sizeof(float) * 16 * (size_t)n, hipMemcpyHostToDevice, st);
    }
    hipError_t mark_read(hipStream_t st) { return fence.mark(st); }      // behind the call's last kernel
};

// THE CELLS SORTED BY KEY (map_sorted_cells): SortedCells, icet_map_table.h.

// A voxel map: the table, the device record of its totals and the pinned copy a stats call reads, the stages of an add and of a query, the sorted cells of an
// extract and of the index.  Every array belongs to a group; the struct is a heap object that never moves.
struct icet_voxel_map {
    icet_ctx* ctx = nullptr;
    icet_voxel_map_params params{};
    rule::Consts k{};
    std::string err;
    MapTable t{};
    u64* ctr = nullptr; u64* h_rec = nullptr;                         // kCtrWords each: device, pinned
    CallStage<MapScan> add;                                           // an add or remove: the scans' descriptors and poses
    CallStage<MapSubmap> query;                                       // a query: the output descriptors and poses
    SortedCells x_cells;                                              // an extract: its sorted cells; the rows of the host form
    float* x_xyz = nullptr; long long* x_count = nullptr; u64* x_key = nullptr; int64_t cap_x = 0;
    // the shape of section 25: mom[9][size] beside the table once icet_voxel_map_enable_shape has run (null: a plain map); dirty: an add or remove has read rows
    // since the map was created or last cleared; the rows of the host form of extract_shape: 12 float and 9 word columns of cap_xs rows
    u64* mom = nullptr; bool dirty = false;
    float* xs_f = nullptr; u64* xs_w = nullptr; int64_t cap_xs = 0;
    // the index of the queries: the cells of count >= 1 by key -- the key is ix_cells.key, beside it count and three columns of cap_ix centroid floats --; what
    // the build saw; stale after every add, remove and clear
    SortedCells ix_cells; long long* ix_count = nullptr; float* ix_xyz = nullptr; int64_t cap_ix = 0, ix_n = 0;
    struct icet_voxel_map_stats ix_stats{}; bool ix_stale = true;
    int32_t* q_counts = nullptr; int32_t* q_offs = nullptr; int64_t cap_qc = 0;      // a query call's per-(query, chunk) counts and offsets
    // the evidence of section 23, one entry per cell of the index it was computed on: current iff ev_valid and the index is not stale.  ev_img / ev_near: the
    // range images of one batch of scans (cap_img words each); ev_ctr: rows imaged | transient cells | unusable poses | unused, on the device and pinned
    CallStage<MapScan> ev;
    int32_t* ev_miss = nullptr; int32_t* ev_agree = nullptr; uint8_t* ev_trans = nullptr; int64_t cap_ev = 0;
    uint32_t* ev_img = nullptr; uint32_t* ev_near = nullptr; int64_t cap_img = 0;
    u64* ev_ctr = nullptr; u64* ev_h_ctr = nullptr; int32_t cap_evrec = 0;
    bool ev_valid = false;
    // the registration against the Gaussians (section 26; icet_map_register.hip, through map_register_view): generation counts what changes the table -- add, remove,
    // clear, enable_shape --, reg is that file's own state, freed with reg_free when the map goes
    uint64_t generation = 0; void* reg = nullptr; void (*reg_free)(void*) = nullptr;
    // save, load and merge (section 27; icet_map_snapshot.hip, through map_snapshot_view): that file's own state, freed with snap_free when the map goes.  A load or
    // a merge raises generation and sets ix_stale and dirty as an add does
    void* snap = nullptr; void (*snap_free)(void*) = nullptr;
    BufferGroup table, record, xout, index, qcounts, evidence, evimages, evrecord, moments, xshape;
    MapShapeTable shape_table() const { MapShapeTable s; static_cast<MapTable&>(s) = t; s.mom = mom; return s; }
};

#define MAPCHK(m, call) do { const hipError_t e_ = static_cast<hipError_t>(call); if (e_ != hipSuccess) { \
    (void)hipGetLastError(); (m)->err = std::string(#call) + ": " + hipGetErrorString(e_); \
    return e_ == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; } } while (0)

static icet_status enter(icet_voxel_map* m) {
    if (!m) return ICET_ERR_BAD_ARG;
    const icet_status st = enter(m->ctx);
    if (st != ICET_OK) m->err = m->ctx->err;
    return st;
}
static icet_status map_refuse(icet_voxel_map* m, const std::string& why) { m->err = why; return ICET_ERR_BAD_ARG; }
template <class T> static bool elem_aligned(const T* p) { return reinterpret_cast<uintptr_t>(p) % sizeof(T) == 0; }      // (a null pointer is)
static unsigned table_grid(const MapTable& t) { return (unsigned)((((size_t)1 << t.log2) + kCellSpan - 1) / kCellSpan); }  // a pass over the table: k_map_cells

static icet_status map_clear(icet_voxel_map* m) {
    const size_t size = (size_t)1 << m->t.log2;
    hipStream_t st = m->ctx->stream;
    m->ix_stale = true; m->generation++;
    MAPCHK(m, hipMemsetAsync(m->t.key, 0xFF, sizeof(u64) * size, st));
    MAPCHK(m, hipMemsetAsync(m->t.count, 0, sizeof(u64) * size, st));
    MAPCHK(m, hipMemsetAsync(m->t.sum, 0, sizeof(u64) * 3 * size, st));
    if (m->mom) MAPCHK(m, hipMemsetAsync(m->mom, 0, sizeof(u64) * srule::kWords * size, st));
    MAPCHK(m, hipMemsetAsync(m->ctr, 0, sizeof(u64) * kCtrWords, st));
    m->dirty = false;
    return ICET_OK;
}

// The cells as they are now, and the totals, into *out: one pass over the table, the record copied to its pinned twin, the stream drained.
static icet_status map_count(icet_voxel_map* m, int32_t min_points, struct icet_voxel_map_stats* out) {
    hipStream_t st = m->ctx->stream;
    const long long minp = std::max(1, min_points);
    MAPCHK(m, hipMemsetAsync(m->ctr + kCtrOccupied, 0, sizeof(u64) * 4, st));      // occupied, out, negative, selected
    k_map_cells<false><<<table_grid(m->t), kCellBlock, 0, st>>>(m->t, minp, m->ctr, nullptr, nullptr, 0);
    MAPCHK(m, hipGetLastError());
    MAPCHK(m, hipMemcpyAsync(m->h_rec, m->ctr, sizeof(u64) * kCtrWords, hipMemcpyDeviceToHost, st));
    MAPCHK(m, hipStreamSynchronize(st));
    u64 r[kCtrWords] = {0};                                           // the copies of the totals summed (two's complement: the signed one too)
    for (int k = 0; k < kTotCopies; k++) for (int w = 0; w < kTotWords; w++) r[w] += m->h_rec[k * kTotWords + w];
    for (int w = kCtrOccupied; w < kCtrWords; w++) r[w] = m->h_rec[w];
    std::memset(out, 0, sizeof(*out));
    out->points_in = (int64_t)r[kCtrIn]; out->points_kept = (int64_t)r[kCtrKept]; out->points_nonfinite = (int64_t)r[kCtrNonfinite];
    out->points_outside = (int64_t)r[kCtrOutside]; out->points_dropped = (int64_t)r[kCtrDropped];
    out->cells_occupied = (int32_t)r[kCtrOccupied]; out->cells_out = (int32_t)r[kCtrOut]; out->cells_negative = (int32_t)r[kCtrNegative];
    out->status = (r[kCtrDropped] ? ICET_VOXEL_MAP_TABLE_FULL : 0) | (r[kCtrNegative] ? ICET_VOXEL_MAP_NEGATIVE : 0);
    return ICET_OK;
}

static icet_status map_add(icet_voxel_map* m, int32_t n, const icet_dev_scan* scans, const float* poses, bool poses_on_device, int32_t sign, const char* call) {
    ICET_TRY(enter(m));
    // everything is checked before anything is touched
    if (n < 0 || (n > 0 && (!scans || !poses))) return map_refuse(m, std::string(call) + ": bad argument");
    if (!rule::sign_ok(sign)) return map_refuse(m, std::string(call) + ": sign must be +1 (add) or -1 (remove)");
    if (poses_on_device && !elem_aligned(poses)) return map_refuse(m, std::string(call) + ": d_poses is not aligned to 4 bytes");
    int64_t blocks = 0;
    for (int k = 0; k < n; k++) {
        if (!dev_scan_ok(scans[k]) || !elem_aligned(scans[k].ptr)) return map_refuse(m, std::string(call) + ": bad scan descriptor (scans[" + std::to_string(k) + "])");
        blocks += (scans[k].n + kRowsPerBlock - 1) / kRowsPerBlock;
    }
    if (blocks > 0x7FFFFFFF) return map_refuse(m, std::string(call) + ": too many rows in one call");
    if (blocks == 0) return ICET_OK;                                  // nothing to read
    icet_ctx* c = m->ctx;
    m->ix_stale = true; m->dirty = true; m->generation++;             // (from here on the table may change)
    CallStage<MapScan>& s = m->add;
    MAPCHK(m, s.begin(n, c->stream));
    int32_t b0 = 0;
    for (int k = 0; k < n; k++) {
        s.h_rec[k] = MapScan{scans[k].ptr, (int32_t)scans[k].n, (int32_t)scans[k].ld, b0, 0};
        b0 += (int32_t)((scans[k].n + kRowsPerBlock - 1) / kRowsPerBlock);
    }
    const float* dp = nullptr;
    MAPCHK(m, s.upload(n, poses, poses_on_device, c->stream, &dp));
    const u64 sg = sign > 0 ? (u64)1 : ~(u64)0;                       // -1 in two's complement
    if (m->mom) {
        const MapShapeTable ts = m->shape_table();
        if (c->map_lds) k_map_add<true, true><<<(unsigned)blocks, kAddBlock, 0, c->stream>>>(s.d_rec, n, dp, m->k, ts, sg, m->ctr);
        else k_map_add<false, true><<<(unsigned)blocks, kAddBlock, 0, c->stream>>>(s.d_rec, n, dp, m->k, ts, sg, m->ctr);
    } else if (c->map_lds) k_map_add<true, false><<<(unsigned)blocks, kAddBlock, 0, c->stream>>>(s.d_rec, n, dp, m->k, m->t, sg, m->ctr);
    else k_map_add<false, false><<<(unsigned)blocks, kAddBlock, 0, c->stream>>>(s.d_rec, n, dp, m->k, m->t, sg, m->ctr);
    MAPCHK(m, hipGetLastError());
    MAPCHK(m, s.mark_read(c->stream));
    return ICET_OK;
}

// The cells of count >= minp, sorted by key, into sc.key / sc.idx.  n > 0 is the cells_out that map_count just returned for minp: it drained the stream, so nothing
// reads the old buffers when they grow.  They grow to n + headroom pairs (a map that grows scan by scan does not allocate at every call), and also when this
// sort asks for more scratch than they hold: the scratch is what rocPRIM asks for at the capacity, and a smaller sort is not promised to ask less.
// `select` writes the n pairs into sc.sel_key / sc.sel_idx: k_map_cells<true> for the extract and the index (map_sorted_cells below), the snapshot's own pass for a save.
static icet_status map_sort_selected(icet_voxel_map* m, SortedCells& sc, int64_t n, int64_t headroom, MapSelectFn select, void* arg) {
    hipStream_t st = m->ctx->stream;
    size_t tmp_bytes = 0;
    MAPCHK(m, rocprim::radix_sort_pairs(nullptr, tmp_bytes, sc.sel_key, sc.key, sc.sel_idx, sc.idx, (size_t)n, 0, 63, st));
    if (n > sc.cap || tmp_bytes > sc.tmp_bytes) {
        const int64_t need = std::max(n + headroom, sc.cap);
        size_t need_tmp = 0;
        MAPCHK(m, rocprim::radix_sort_pairs(nullptr, need_tmp, sc.sel_key, sc.key, sc.sel_idx, sc.idx, (size_t)need, 0, 63, st));
        need_tmp = std::max(std::max(need_tmp, tmp_bytes), (size_t)16);
        MAPCHK(m, grow(sc.mem, sc.cap, need, [&] {
            int e = sc.mem.device(sc.sel_key, (size_t)need);
            if (!e) e = sc.mem.device(sc.key, (size_t)need);
            if (!e) e = sc.mem.device(sc.sel_idx, (size_t)need);
            if (!e) e = sc.mem.device(sc.idx, (size_t)need);
            if (!e) e = sc.mem.device_bytes(sc.tmp, need_tmp);
            return e;
        }));
        sc.tmp_bytes = need_tmp;
    }
    MAPCHK(m, select(arg, sc, n, st));
    MAPCHK(m, rocprim::radix_sort_pairs(sc.tmp, tmp_bytes, sc.sel_key, sc.key, sc.sel_idx, sc.idx, (size_t)n, 0, 63, st));
    return ICET_OK;
}
static icet_status map_sorted_cells(icet_voxel_map* m, SortedCells& sc, int64_t n, long long minp, int64_t headroom) {
    struct Arg { icet_voxel_map* m; long long minp; } a{m, minp};
    return map_sort_selected(m, sc, n, headroom, [](void* arg, SortedCells& s, int64_t rows, hipStream_t st) {
        const Arg& g = *static_cast<const Arg*>(arg);
        k_map_cells<true><<<table_grid(g.m->t), kCellBlock, 0, st>>>(g.m->t, g.minp, g.m->ctr, s.sel_key, s.sel_idx, (u64)rows);
        return hipGetLastError();
    }, &a);
}

// shaped (extract_shape, section 25): the same rows, and behind k_map_centroid the columns of *shape from k_map_shape.
static icet_status map_extract(icet_voxel_map* m, int32_t min_points, bool to_host, float* xyz, int64_t ld, int64_t cap_rows, int64_t* count, uint64_t* key,
                               bool shaped, const icet_voxel_map_shape* shape, struct icet_voxel_map_stats* out, const char* call) {
    ICET_TRY(enter(m));
    if (cap_rows < 0 || ld < cap_rows || (cap_rows > 0 && !xyz)) return map_refuse(m, std::string(call) + ": bad argument (cap_rows >= 0, ld >= cap_rows, a buffer of rows)");
    if (!to_host && !(elem_aligned(xyz) && elem_aligned(count) && elem_aligned(key)))
        return map_refuse(m, std::string(call) + ": a device pointer is not aligned to its element");
    if (shaped) {
        if (!m->mom) return map_refuse(m, std::string(call) + ": the map has no shape (icet_voxel_map_enable_shape on an empty map)");
        if (!shape) return map_refuse(m, std::string(call) + ": bad argument (a NULL shape descriptor)");
        if (shape->ld < cap_rows || shape->flags != 0 || shape->reserved != 0) return map_refuse(m, std::string(call) + ": bad shape descriptor (ld >= cap_rows, flags and reserved 0)");
        if (!to_host && !(elem_aligned(shape->cov) && elem_aligned(shape->normal) && elem_aligned(shape->evals) && elem_aligned(shape->moments)))
            return map_refuse(m, std::string(call) + ": a device pointer is not aligned to its element");
    }
    hipStream_t st = m->ctx->stream;
    struct icet_voxel_map_stats s;
    ICET_TRY(map_count(m, min_points, &s));
    const int64_t n_out = s.cells_out, rows = std::min(n_out, cap_rows);
    if (n_out > cap_rows) s.status |= ICET_VOXEL_MAP_TRUNCATED;
    if (rows > 0) {
        if (to_host && rows > m->cap_x) {                             // (the count above drained the stream: nothing reads the old buffers)
            BufferGroup& g = m->xout;
            MAPCHK(m, grow(g, m->cap_x, rows, [&] {
                int e = g.device(m->x_xyz, 3 * (size_t)rows);
                if (!e) e = g.device(m->x_count, (size_t)rows);
                if (!e) e = g.device(m->x_key, (size_t)rows);
                return e;
            }));
        }
        if (shaped && to_host && rows > m->cap_xs) {
            BufferGroup& g = m->xshape;
            MAPCHK(m, grow(g, m->cap_xs, rows, [&] { const int e = g.device(m->xs_f, 12 * (size_t)rows); return e ? e : g.device(m->xs_w, srule::kWords * (size_t)rows); }));
        }
        ICET_TRY(map_sorted_cells(m, m->x_cells, n_out, std::max(1, min_points), 0));
        float* dx = to_host ? m->x_xyz : xyz;
        long long* dc = to_host ? (count ? m->x_count : nullptr) : reinterpret_cast<long long*>(count);
        u64* dk = to_host ? (key ? m->x_key : nullptr) : reinterpret_cast<u64*>(key);
        const long long dld = to_host ? rows : ld;
        k_map_centroid<<<(unsigned)((rows + kCellBlock - 1) / kCellBlock), kCellBlock, 0, st>>>(m->t, m->k, m->x_cells.key, m->x_cells.idx, rows, dx, dld, dc, dk);
        MAPCHK(m, hipGetLastError());
        if (shaped) {
            // the host form: cov | normal | evals in 6 + 3 + 3 columns of `rows` floats, the words in 9 columns; a column the caller left out is not computed
            MapShapeOut o{shape->cov, shape->normal, shape->evals, reinterpret_cast<u64*>(shape->moments), (long long)shape->ld};
            if (to_host) o = MapShapeOut{shape->cov ? m->xs_f : nullptr, shape->normal ? m->xs_f + 6 * rows : nullptr, shape->evals ? m->xs_f + 9 * rows : nullptr,
                                         shape->moments ? m->xs_w : nullptr, (long long)rows};
            k_map_shape<<<(unsigned)((rows + kCellBlock - 1) / kCellBlock), kCellBlock, 0, st>>>(m->shape_table(), srule::make_consts(m->params.cell), m->x_cells.idx, rows, o);
            MAPCHK(m, hipGetLastError());
            if (to_host) {
                const size_t wf = sizeof(float) * (size_t)rows, ww = sizeof(u64) * (size_t)rows, sld = (size_t)shape->ld;
                if (shape->cov) MAPCHK(m, hipMemcpy2DAsync(shape->cov, sizeof(float) * sld, o.cov, wf, wf, 6, hipMemcpyDeviceToHost, st));
                if (shape->normal) MAPCHK(m, hipMemcpy2DAsync(shape->normal, sizeof(float) * sld, o.normal, wf, wf, 3, hipMemcpyDeviceToHost, st));
                if (shape->evals) MAPCHK(m, hipMemcpy2DAsync(shape->evals, sizeof(float) * sld, o.evals, wf, wf, 3, hipMemcpyDeviceToHost, st));
                if (shape->moments) MAPCHK(m, hipMemcpy2DAsync(shape->moments, sizeof(u64) * sld, o.moments, ww, ww, srule::kWords, hipMemcpyDeviceToHost, st));
            }
        }
        if (to_host) {
            MAPCHK(m, hipMemcpy2DAsync(xyz, sizeof(float) * (size_t)ld, dx, sizeof(float) * (size_t)rows, sizeof(float) * (size_t)rows, 3, hipMemcpyDeviceToHost, st));
            if (count) MAPCHK(m, hipMemcpyAsync(count, dc, sizeof(int64_t) * (size_t)rows, hipMemcpyDeviceToHost, st));
            if (key) MAPCHK(m, hipMemcpyAsync(key, dk, sizeof(uint64_t) * (size_t)rows, hipMemcpyDeviceToHost, st));
        }
        MAPCHK(m, hipStreamSynchronize(st));
    }
    if (out) *out = s;
    return ICET_OK;
}

// The index of the queries, if the table changed since it was built: extract's sequence -- count, select, sort by key, centroids -- for min_points 1, into the
// index's own buffers.  The count drains the stream (the sort's size is a host value), so nothing reads the old index when it grows.
static icet_status map_index(icet_voxel_map* m) {
    if (!m->ix_stale) return ICET_OK;
    m->ev_valid = false;                                              // (the evidence belongs to the index it was computed on)
    hipStream_t st = m->ctx->stream;
    struct icet_voxel_map_stats s;
    ICET_TRY(map_count(m, 1, &s));
    const int64_t n = s.cells_out;
    m->ix_n = 0;
    if (n > 0) {
        if (n > m->cap_ix) {                                          // (the headroom of the sorted cells below; each capacity guards its own arrays)
            BufferGroup& g = m->index;
            const int64_t need = n + n / 4;
            MAPCHK(m, grow(g, m->cap_ix, need, [&] { const int e = g.device(m->ix_count, (size_t)need); return e ? e : g.device(m->ix_xyz, 3 * (size_t)need); }));
        }
        ICET_TRY(map_sorted_cells(m, m->ix_cells, n, 1, n / 4));
        k_map_centroid<<<(unsigned)((n + kCellBlock - 1) / kCellBlock), kCellBlock, 0, st>>>(m->t, m->k, m->ix_cells.key, m->ix_cells.idx, n, m->ix_xyz, m->cap_ix, m->ix_count, nullptr);
        MAPCHK(m, hipGetLastError());
    }
    m->ix_n = n; m->ix_stats = s; m->ix_stale = false;
    return ICET_OK;
}

static icet_status map_query(icet_voxel_map* m, int32_t n_q, const float* poses, bool poses_on_device, const icet_voxel_map_query* q, const icet_voxel_map_submap* outs,
                             int32_t* d_rows, int32_t* d_total, int32_t* d_status, const char* call) {
    ICET_TRY(enter(m));
    // everything is checked before anything is touched
    const std::string who(call);
    if (n_q < 1 || n_q > qrule::kMaxQueries) return map_refuse(m, who + ": n_q must lie in 1 .. 256");
    if (!poses || !q || !outs || !d_rows) return map_refuse(m, who + ": bad argument (a NULL array)");
    const bool is_static = (q->flags & ICET_VOXEL_MAP_QUERY_STATIC) != 0;
    const int32_t rule_flags = q->flags & ~ICET_VOXEL_MAP_QUERY_STATIC;
    if (!qrule::params_ok(q->min_range, q->max_range, rule_flags, q->reserved)) return map_refuse(m, who + ": the ranges must be finite, the flags known and the reserved words 0");
    if (is_static && !(m->ev_valid && !m->ix_stale))
        return map_refuse(m, who + ": ICET_VOXEL_MAP_QUERY_STATIC needs current evidence (icet_voxel_map_evidence_device after the last add, remove or clear)");
    if ((poses_on_device && !elem_aligned(poses)) || !(elem_aligned(d_rows) && elem_aligned(d_total) && elem_aligned(d_status)))
        return map_refuse(m, who + ": a device pointer is not aligned to its element");
    bool any_rows = false;
    for (int k = 0; k < n_q; k++) {
        const icet_voxel_map_submap& o = outs[k];
        if (!qrule::submap_ok(o.xyz, o.ld, o.cap_rows)) return map_refuse(m, who + ": bad sub-map (outs[" + std::to_string(k) + "]: cap_rows >= 0, ld >= cap_rows, a buffer of rows)");
        if (!(elem_aligned(o.xyz) && elem_aligned(o.count) && elem_aligned(o.key)))
            return map_refuse(m, who + ": a device pointer is not aligned to its element (outs[" + std::to_string(k) + "])");
        any_rows = any_rows || o.cap_rows > 0;
    }
    icet_ctx* c = m->ctx;
    hipStream_t st = c->stream;
    ICET_TRY(map_index(m));
    const long long n_chunks = (m->ix_n + kQueryChunk - 1) / kQueryChunk;
    CallStage<MapSubmap>& s = m->query;
    MAPCHK(m, s.begin(n_q, st));
    const int64_t words = (int64_t)n_q * n_chunks;
    if (words > m->cap_qc) {
        MAPCHK(m, hipStreamSynchronize(st));
        BufferGroup& g = m->qcounts;
        MAPCHK(m, grow(g, m->cap_qc, words, [&] {
            int e = g.device(m->q_counts, (size_t)words);
            if (!e) e = g.device(m->q_offs, (size_t)words);
            return e;
        }));
    }
    for (int k = 0; k < n_q; k++) s.h_rec[k] = MapSubmap{outs[k].xyz, outs[k].ld, outs[k].cap_rows, reinterpret_cast<long long*>(outs[k].count), reinterpret_cast<u64*>(outs[k].key)};
    const float* dp = nullptr;
    MAPCHK(m, s.upload(n_q, poses, poses_on_device, st, &dp));
    const qrule::Consts kc = qrule::make_consts(m->params.cell, q->min_range, q->max_range, q->min_points, rule_flags);
    const MapIndex ix{m->ix_cells.key, m->ix_count, m->ix_xyz, (long long)m->cap_ix, (long long)m->ix_n, is_static ? m->ev_trans : nullptr};
    const int prune = c->map_query_prune;
    if (n_chunks > 0) {
        if (is_static) k_map_query_count<true><<<(unsigned)n_chunks, kQueryBlock, 0, st>>>(ix, dp, n_q, kc, prune, m->q_counts, n_chunks);
        else k_map_query_count<false><<<(unsigned)n_chunks, kQueryBlock, 0, st>>>(ix, dp, n_q, kc, prune, m->q_counts, n_chunks);
        MAPCHK(m, hipGetLastError());
    }
    k_map_query_scan<<<(unsigned)n_q, kQueryBlock, 0, st>>>(m->q_counts, m->q_offs, n_chunks, dp, s.d_rec, d_rows, d_total, d_status);
    MAPCHK(m, hipGetLastError());
    if (n_chunks > 0 && any_rows) {                                   // (a count-only call writes no row)
        if (is_static) k_map_query_write<true><<<(unsigned)n_chunks, kQueryBlock, 0, st>>>(ix, dp, n_q, kc, prune, m->q_counts, m->q_offs, n_chunks, s.d_rec);
        else k_map_query_write<false><<<(unsigned)n_chunks, kQueryBlock, 0, st>>>(ix, dp, n_q, kc, prune, m->q_counts, m->q_offs, n_chunks, s.d_rec);
        MAPCHK(m, hipGetLastError());
    }
    MAPCHK(m, s.mark_read(st));
    return ICET_OK;
}

// The scans of one evidence batch: option "map_evidence_batch", or as many as fit 64 MiB of images (two of W^2 words per scan); 1 .. 256.
static int32_t evidence_batch(const icet_ctx* c, int32_t image_log2) {
    const int64_t per_scan = (int64_t)2 * 4 << (2 * image_log2);
    const int64_t b = c->map_evidence_batch > 0 ? c->map_evidence_batch : ((int64_t)64 << 20) / per_scan;
    return (int32_t)std::min<int64_t>(std::max<int64_t>(b, 1), erule::kMaxBatch);
}

static icet_status map_evidence(icet_voxel_map* m, int32_t n, const icet_dev_scan* scans, const float* poses, bool poses_on_device, const icet_voxel_map_evidence* e,
                                struct icet_voxel_map_evidence_stats* out, const char* call) {
    ICET_TRY(enter(m));
    // everything is checked before anything is touched
    const std::string who(call);
    if (n < 0 || !e || (n > 0 && (!scans || !poses))) return map_refuse(m, who + ": bad argument");
    if (!erule::params_ok(e->min_range, e->max_range, e->margin, e->image_log2, e->window, e->min_miss, e->agree_factor, e->flags))
        return map_refuse(m, who + ": the ranges and the margin must be finite, max_range > 0, margin >= 0, image_log2 4 .. 10, window 0 .. 2, min_miss and agree_factor >= 0, flags 0");
    if (poses_on_device && !elem_aligned(poses)) return map_refuse(m, who + ": d_poses is not aligned to 4 bytes");
    int64_t blocks = 0;
    for (int k = 0; k < n; k++) {
        if (!dev_scan_ok(scans[k]) || !elem_aligned(scans[k].ptr)) return map_refuse(m, who + ": bad scan descriptor (scans[" + std::to_string(k) + "])");
        blocks += (scans[k].n + kRowsPerBlock - 1) / kRowsPerBlock;
    }
    if (blocks > 0x7FFFFFFF) return map_refuse(m, who + ": too many rows in one call");
    icet_ctx* c = m->ctx;
    hipStream_t st = c->stream;
    ICET_TRY(map_index(m));
    m->ev_valid = false;                                              // (from here on the evidence changes)
    const erule::Consts kc = erule::make_consts(m->params.cell, e->min_range, e->max_range, e->margin, e->image_log2, e->window, e->min_miss, e->agree_factor);
    const int64_t w2 = (int64_t)1 << (2 * e->image_log2), cells = m->ix_n;
    const int32_t batch = std::min(evidence_batch(c, e->image_log2), std::max(n, 1));
    // the buffers: each group grows behind a drained stream (an earlier call's kernels may still read the old ones)
    if (!m->cap_evrec) {
        BufferGroup& g = m->evrecord;
        MAPCHK(m, grow(g, m->cap_evrec, 4, [&] { const int a = g.device(m->ev_ctr, 4); return a ? a : g.pinned(m->ev_h_ctr, 4); }));
    }
    if (cells > m->cap_ev) {
        MAPCHK(m, hipStreamSynchronize(st));
        BufferGroup& g = m->evidence;
        const int64_t need = cells + cells / 4;
        MAPCHK(m, grow(g, m->cap_ev, need, [&] {
            int a = g.device(m->ev_miss, (size_t)need);
            if (!a) a = g.device(m->ev_agree, (size_t)need);
            if (!a) a = g.device(m->ev_trans, (size_t)need);
            return a;
        }));
    }
    if (batch * w2 > m->cap_img) {
        MAPCHK(m, hipStreamSynchronize(st));
        BufferGroup& g = m->evimages;
        const int64_t need = batch * w2;
        MAPCHK(m, grow(g, m->cap_img, need, [&] { const int a = g.device(m->ev_img, (size_t)need); return a ? a : g.device(m->ev_near, (size_t)need); }));
    }
    CallStage<MapScan>& s = m->ev;
    const float* dp = nullptr;
    MAPCHK(m, s.begin(n, st));
    if (n > 0) {
        int32_t b0 = 0;
        for (int k = 0; k < n; k++) {                                 // block0: the scan's first block in the launch of its batch
            if (k % batch == 0) b0 = 0;
            s.h_rec[k] = MapScan{scans[k].ptr, (int32_t)scans[k].n, (int32_t)scans[k].ld, b0, 0};
            b0 += (int32_t)((scans[k].n + kRowsPerBlock - 1) / kRowsPerBlock);
        }
        MAPCHK(m, s.upload(n, poses, poses_on_device, st, &dp));
    }
    MAPCHK(m, hipMemsetAsync(m->ev_ctr, 0, sizeof(u64) * 4, st));
    if (cells > 0) {
        MAPCHK(m, hipMemsetAsync(m->ev_miss, 0, sizeof(int32_t) * (size_t)cells, st));
        MAPCHK(m, hipMemsetAsync(m->ev_agree, 0, sizeof(int32_t) * (size_t)cells, st));
    }
    const MapIndex ix{m->ix_cells.key, m->ix_count, m->ix_xyz, (long long)m->cap_ix, (long long)cells, nullptr};
    const long long n_chunks = (cells + kQueryChunk - 1) / kQueryChunk;
    for (int32_t k0 = 0; k0 < n; k0 += batch) {
        const int32_t nb = std::min(batch, n - k0);
        int64_t bb = 0;
        for (int k = k0; k < k0 + nb; k++) bb += (scans[k].n + kRowsPerBlock - 1) / kRowsPerBlock;
        if (bb == 0) continue;                                        // no row: every pixel is empty, and an empty pixel is no evidence
        const long long words = (long long)nb * w2;
        MAPCHK(m, hipMemsetAsync(m->ev_img, 0xFF, sizeof(uint32_t) * (size_t)words, st));
        k_map_image<<<(unsigned)bb, kAddBlock, 0, st>>>(s.d_rec + k0, nb, kc, m->ev_img, m->ev_ctr);
        MAPCHK(m, hipGetLastError());
        k_map_image_near<<<(unsigned)((words + kCellBlock - 1) / kCellBlock), kCellBlock, 0, st>>>(m->ev_img, m->ev_near, kc, words);
        MAPCHK(m, hipGetLastError());
        if (n_chunks == 0) continue;                                  // (an empty map: the images alone, which is how scripts/bench_map_evidence.py times them)
        k_map_evidence<<<(unsigned)n_chunks, kQueryBlock, 0, st>>>(ix, dp + 16 * (size_t)k0, nb, kc, c->map_evidence_prune, m->ev_near, m->ev_miss, m->ev_agree);
        MAPCHK(m, hipGetLastError());
    }
    k_map_evidence_decide<<<(unsigned)std::max<int64_t>(1, (cells + kCellBlock - 1) / kCellBlock), kCellBlock, 0, st>>>(m->ev_miss, m->ev_agree, m->ev_trans, cells, kc, dp, n, m->ev_ctr);
    MAPCHK(m, hipGetLastError());
    MAPCHK(m, s.mark_read(st));
    m->ev_valid = true;
    if (out) {
        MAPCHK(m, hipMemcpyAsync(m->ev_h_ctr, m->ev_ctr, sizeof(u64) * 4, hipMemcpyDeviceToHost, st));
        MAPCHK(m, hipStreamSynchronize(st));
        std::memset(out, 0, sizeof(*out));
        out->rows_imaged = (int64_t)m->ev_h_ctr[0]; out->cells = (int32_t)cells; out->cells_transient = (int32_t)m->ev_h_ctr[1];
        out->scans_bad_pose = (int32_t)m->ev_h_ctr[2]; out->scans_used = n - out->scans_bad_pose;
    }
    return ICET_OK;
}

namespace icet {
bool map_register_view(icet_voxel_map* m, MapRegisterView* v) {
    if (!m) return false;
    *v = MapRegisterView{m->ctx, m->params.cell, m->t.log2, m->t.key, m->t.count, m->t.sum, m->mom, m->generation, &m->reg, &m->reg_free};
    return true;
}
void map_set_error(icet_voxel_map* m, const char* why) { if (m) m->err = why; }
bool map_snapshot_view(icet_voxel_map* m, MapSnapshotView* v) {
    if (!m) return false;
    *v = MapSnapshotView{m->ctx, m->params.cell, m->params.min_range, m->params.max_range, m->t.log2, m->t.key, m->t.count, m->t.sum, m->mom, m->ctr,
                         &m->generation, &m->ix_stale, &m->dirty, &m->snap, &m->snap_free};
    return true;
}
int map_sort_cells(icet_voxel_map* m, SortedCells& sc, int64_t n, MapSelectFn select, void* arg) { return map_sort_selected(m, sc, n, 0, select, arg); }
}  // namespace icet

extern "C" {

icet_status icet_voxel_map_evidence_device(icet_voxel_map* m, int32_t n, const icet_dev_scan* scans, const float* poses, const icet_voxel_map_evidence* e,
                                           struct icet_voxel_map_evidence_stats* out) {
    return map_evidence(m, n, scans, poses, false, e, out, "icet_voxel_map_evidence_device");
}

icet_status icet_voxel_map_evidence_posed_device(icet_voxel_map* m, int32_t n, const icet_dev_scan* scans, const float* d_poses, const icet_voxel_map_evidence* e,
                                                 struct icet_voxel_map_evidence_stats* out) {
    return map_evidence(m, n, scans, d_poses, true, e, out, "icet_voxel_map_evidence_posed_device");
}

icet_status icet_voxel_map_evidence_fetch_device(icet_voxel_map* m, int32_t* d_miss, int32_t* d_agree, uint8_t* d_transient, int64_t cap, int64_t* rows_out) {
    ICET_TRY(enter(m));
    const std::string who("icet_voxel_map_evidence_fetch_device");
    if (!(m->ev_valid && !m->ix_stale)) return map_refuse(m, who + ": no current evidence (icet_voxel_map_evidence_device after the last add, remove or clear)");
    if (cap < m->ix_n) return map_refuse(m, who + ": cap is below the cells of the index");
    if (!(elem_aligned(d_miss) && elem_aligned(d_agree))) return map_refuse(m, who + ": a device pointer is not aligned to its element");
    hipStream_t st = m->ctx->stream;
    const size_t n = (size_t)m->ix_n;
    if (n > 0) {
        if (d_miss) MAPCHK(m, hipMemcpyAsync(d_miss, m->ev_miss, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, st));
        if (d_agree) MAPCHK(m, hipMemcpyAsync(d_agree, m->ev_agree, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, st));
        if (d_transient) MAPCHK(m, hipMemcpyAsync(d_transient, m->ev_trans, n, hipMemcpyDeviceToDevice, st));
    }
    if (rows_out) *rows_out = m->ix_n;
    return ICET_OK;
}

const char* icet_voxel_map_last_error(const icet_voxel_map* m) { return m ? m->err.c_str() : "null voxel map"; }

icet_status icet_voxel_map_create(icet_ctx* c, const icet_voxel_map_params* p, icet_voxel_map** out) {
    if (out) *out = nullptr;
    if (!c) return ICET_ERR_BAD_ARG;
    if (!out || !p) { c->err = "icet_voxel_map_create: bad argument"; return ICET_ERR_BAD_ARG; }
    if (!rule::params_ok(p->cell, p->min_range, p->max_range, p->table_log2, p->flags) || p->reserved[0] || p->reserved[1] || p->reserved[2]) {
        c->err = "icet_voxel_map_create: cell must be finite and > 0, the ranges finite, table_log2 10 .. 30, flags and the reserved words 0";
        return ICET_ERR_BAD_ARG;
    }
    ICET_TRY(enter(c));
    icet_voxel_map* m = new (std::nothrow) icet_voxel_map();
    if (!m) { c->err = "host allocation failed"; return ICET_ERR_NOMEM; }
    m->ctx = c; m->params = *p; m->k = rule::make_consts(p->cell, p->min_range, p->max_range); m->t.log2 = (uint32_t)p->table_log2;
    const size_t size = (size_t)1 << p->table_log2;
    int e = m->table.device(m->t.key, size);
    if (!e) e = m->table.device(m->t.count, size);
    if (!e) e = m->table.device(m->t.sum, 3 * size);
    if (!e) e = m->record.device(m->ctr, (size_t)kCtrWords);
    if (!e) e = m->record.pinned(m->h_rec, (size_t)kCtrWords);
    icet_status st = ICET_OK;
    if (e) { (void)hipGetLastError(); m->err = std::string("icet_voxel_map_create: ") + hipGetErrorString(static_cast<hipError_t>(e)); st = e == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; }
    if (st == ICET_OK) st = map_clear(m);
    if (st != ICET_OK) { c->err = m->err; (void)icet_voxel_map_destroy(m); return st; }
    *out = m;
    return ICET_OK;
}

icet_status icet_voxel_map_destroy(icet_voxel_map* m) {
    if (!m) return ICET_ERR_BAD_ARG;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);              // (an add or an extract may still read or write the table)
    if (m->reg && m->reg_free) m->reg_free(m->reg);
    if (m->snap && m->snap_free) m->snap_free(m->snap);
    delete m;                                                // (every array belongs to a group, every event to a stage)
    return ICET_OK;
}

icet_status icet_voxel_map_clear(icet_voxel_map* m) {
    ICET_TRY(enter(m));
    return map_clear(m);
}

icet_status icet_voxel_map_add_device(icet_voxel_map* m, int32_t n, const icet_dev_scan* scans, const float* poses, int32_t sign) {
    return map_add(m, n, scans, poses, false, sign, "icet_voxel_map_add_device");
}

icet_status icet_voxel_map_add_posed_device(icet_voxel_map* m, int32_t n, const icet_dev_scan* scans, const float* d_poses, int32_t sign) {
    return map_add(m, n, scans, d_poses, true, sign, "icet_voxel_map_add_posed_device");
}

icet_status icet_voxel_map_stats(icet_voxel_map* m, int32_t min_points, struct icet_voxel_map_stats* out) {
    ICET_TRY(enter(m));
    if (!out) return map_refuse(m, "icet_voxel_map_stats: bad argument");
    return map_count(m, min_points, out);
}

icet_status icet_voxel_map_extract_device(icet_voxel_map* m, int32_t min_points, float* d_xyz, int64_t ld, int64_t cap_rows, int64_t* d_count, uint64_t* d_key,
                                          struct icet_voxel_map_stats* out) {
    return map_extract(m, min_points, false, d_xyz, ld, cap_rows, d_count, d_key, false, nullptr, out, "icet_voxel_map_extract_device");
}

icet_status icet_voxel_map_extract(icet_voxel_map* m, int32_t min_points, float* xyz, int64_t ld, int64_t cap_rows, int64_t* count, uint64_t* key,
                                   struct icet_voxel_map_stats* out) {
    return map_extract(m, min_points, true, xyz, ld, cap_rows, count, key, false, nullptr, out, "icet_voxel_map_extract");
}

icet_status icet_voxel_map_enable_shape(icet_voxel_map* m) {
    ICET_TRY(enter(m));
    if (m->mom) return ICET_OK;
    if (m->dirty) return map_refuse(m, "icet_voxel_map_enable_shape: the map has read rows since it was created or last cleared (enable shape on an empty map)");
    const size_t size = (size_t)1 << m->t.log2;
    const int e = m->moments.device(m->mom, srule::kWords * size);      // (a refused allocation leaves the slot null: the map stays plain)
    if (e) { (void)hipGetLastError(); m->err = std::string("icet_voxel_map_enable_shape: ") + hipGetErrorString(static_cast<hipError_t>(e)); return e == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; }
    const hipError_t z = hipMemsetAsync(m->mom, 0, sizeof(u64) * srule::kWords * size, m->ctx->stream);
    if (z != hipSuccess) m->moments.release();
    MAPCHK(m, z);
    m->generation++;
    return ICET_OK;
}

icet_status icet_voxel_map_extract_shape_device(icet_voxel_map* m, int32_t min_points, float* d_xyz, int64_t ld, int64_t cap_rows, int64_t* d_count, uint64_t* d_key,
                                                const icet_voxel_map_shape* shape, struct icet_voxel_map_stats* out) {
    return map_extract(m, min_points, false, d_xyz, ld, cap_rows, d_count, d_key, true, shape, out, "icet_voxel_map_extract_shape_device");
}

icet_status icet_voxel_map_extract_shape(icet_voxel_map* m, int32_t min_points, float* xyz, int64_t ld, int64_t cap_rows, int64_t* count, uint64_t* key,
                                         const icet_voxel_map_shape* shape, struct icet_voxel_map_stats* out) {
    return map_extract(m, min_points, true, xyz, ld, cap_rows, count, key, true, shape, out, "icet_voxel_map_extract_shape");
}

icet_status icet_voxel_map_index(icet_voxel_map* m, struct icet_voxel_map_stats* out) {
    ICET_TRY(enter(m));
    ICET_TRY(map_index(m));
    if (out) *out = m->ix_stats;
    return ICET_OK;
}

icet_status icet_voxel_map_query_device(icet_voxel_map* m, int32_t n_q, const float* poses, const icet_voxel_map_query* q, const icet_voxel_map_submap* outs,
                                        int32_t* d_rows, int32_t* d_total, int32_t* d_status) {
    return map_query(m, n_q, poses, false, q, outs, d_rows, d_total, d_status, "icet_voxel_map_query_device");
}

icet_status icet_voxel_map_query_posed_device(icet_voxel_map* m, int32_t n_q, const float* d_poses, const icet_voxel_map_query* q, const icet_voxel_map_submap* outs,
                                              int32_t* d_rows, int32_t* d_total, int32_t* d_status) {
    return map_query(m, n_q, d_poses, true, q, outs, d_rows, d_total, d_status, "icet_voxel_map_query_posed_device");
}

}  // extern "C"
