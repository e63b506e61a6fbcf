// icet_amd/csrc/icet_map_register.hip -- scans registered against the Gaussians of a shaped voxel map (include/icet_hip.h icet_voxel_map_register_*; DESIGN.md
// section 26).  The rule -- a cell's Gaussian, a row's terms, the damped solve, the retraction, the state machine of a query -- is icet_map_register.h; this file is
// the kernels around it and the entry points:
//     k_mapreg_gauss   one pass over the table, one thread per entry: the dense record {mu[3], W[6], n-or-0} of 80 bytes per slot, so that a row costs one key probe
//                      and one record instead of thirteen scattered words and a 3 x 3 inverse.  Rebuilt in stream order when the map or (sigma_min, min_points) changed
//     k_mapreg_rows    one block per chunk of kChunkRows rows of one query (blockIdx -> (query, chunk), k_map_add's scheme); a block of a terminal query exits at
//                      once.  16-byte loads of 4 consecutive rows per lane; a read-only probe bounded by the table size; 28 double accumulators and two counts per
//                      thread over its rows in row order, then a fixed wave64 butterfly, then the block's waves in order through LDS: one partial per (query, chunk)
//     k_mapreg_rows_nb the same pass under a neighbourhood of K = 7 or 27 cells (params.flags), K a compile-time constant: per row the K keys, their first probes
//                      issued together, each candidate's s from a record that is dropped at once, the winner's slot and s alone kept through the selection and
//                      its record read again for the terms.  The same loads, pose staging, sums and partials as k_mapreg_rows, which flags = 0 still launches
//     k_mapreg_step    one block per query: lane j sums component j of the query's partials in ascending chunk order, thread 0 runs the rule's state machine and
//                      writes the query's state and record
// A call enqueues the Gaussians if stale and 1 + max_iters x (rows, step): no atomics, no fence, no block waits for another, no host round trip.
// The map itself is icet_map.hip's; this file sees it through map_register_view (icet_internal.h) and keeps its own state in the slot the map frees.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include "../../include/icet_hip.h"
#include "icet_ctx.h"
#include "icet_staging.h"
#include "icet_map_register.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>

namespace icet {
namespace {

namespace rr = icet_map_register_rule;
namespace mrule = icet_map_rule;
namespace srule = icet_map_shape_rule;
typedef unsigned long long u64;

constexpr int kRegBlock = 256;
constexpr int kRegWaves = kRegBlock / 64;
constexpr int kRowsPerBlock = rr::kChunkRows;      // two trips of 256 lanes x 4 rows
constexpr int kStepBlock = 64;
static_assert(rr::kMaxQueries == ICET_VOXEL_MAP_MAX_QUERIES && rr::kMaxIters == ICET_VOXEL_MAP_REG_MAX_ITERS, "the limits the header names");
static_assert(rr::kConverged == ICET_VOXEL_MAP_REG_CONVERGED && rr::kIterationCap == ICET_VOXEL_MAP_REG_ITERATION_CAP && rr::kStalled == ICET_VOXEL_MAP_REG_STALLED &&
              rr::kNoOverlap == ICET_VOXEL_MAP_REG_NO_OVERLAP && rr::kBadPose == ICET_VOXEL_MAP_REG_BAD_POSE, "the status words the header names");
static_assert(sizeof(rr::Record) == sizeof(icet_voxel_map_registration) && sizeof(rr::Record) == 328 && offsetof(rr::Record, info) == offsetof(icet_voxel_map_registration, info) &&
              offsetof(rr::Record, g) == offsetof(icet_voxel_map_registration, g) && offsetof(rr::Record, cost) == offsetof(icet_voxel_map_registration, cost) &&
              offsetof(rr::Record, rows_scored) == offsetof(icet_voxel_map_registration, rows_scored) && offsetof(rr::Record, status) == offsetof(icet_voxel_map_registration, status),
              "the rule's record is the header's, word for word");
static_assert(rr::kFlagNeighbours7 == ICET_VOXEL_MAP_REG_NEIGHBOURS_7 && rr::kFlagNeighbours27 == ICET_VOXEL_MAP_REG_NEIGHBOURS_27, "the flags the header names");
static_assert(sizeof(rr::Gauss) == 80, "mu[3] | W[6] | n");
static_assert(sizeof(icet_voxel_map_register_term) == 256 && sizeof(icet_voxel_map_register_params) == 72, "the sizes the header names");

struct RegScan { const float* ptr; int32_t n, ld, block0, chunks; };      // block0: the query's first block in the launch, and its first partial
static_assert(sizeof(RegScan) == 24, "ptr | n | ld | block0 | chunks");
struct RegTable { const u64* key; const u64* count; const u64* sum; const u64* mom; uint32_t log2; };
struct Partial { double v[rr::kSums]; int32_t scored, matched; };

__global__ __launch_bounds__(kRegBlock) void k_mapreg_gauss(RegTable t, rr::Consts kc, rr::Gauss* __restrict__ out) {
    const u64 size = (u64)1 << t.log2, i = (u64)blockIdx.x * kRegBlock + threadIdx.x;
    if (i >= size) return;
    const u64 key = t.key[i];
    if (key == mrule::kEmpty) { out[i].n = 0; return; }               // (a probe ends at an empty key: the rest of the record is never read)
    uint64_t sum[3], w[srule::kWords];
#pragma unroll
    for (int a = 0; a < 3; a++) sum[a] = t.sum[a * size + i];
#pragma unroll
    for (int j = 0; j < srule::kWords; j++) w[j] = t.mom[j * size + i];
    rr::Gauss g;
    rr::gauss(kc, key, (int64_t)t.count[i], sum, w, g);
    out[i] = g;
}

// m <= 4 rows of one column from row i (a multiple of 4): k_map_add's load, one 16-byte load where the column's address allows it and all four rows exist.
__device__ __forceinline__ void load_rows(const float* __restrict__ col, int i, int m, float v[4]) {
    const float* p = col + i;
    if (m == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        for (int r = 0; r < 4; r++) v[r] = r < m ? p[r] : 0.f;
    }
}

// The entry of `key`, or -1: read-only, at most `size` probes (an entry's key never changes once it is set, and nothing writes the table while a call runs).
__device__ __forceinline__ long long probe(const RegTable& t, u64 key) {
    const u64 mask = ((u64)1 << t.log2) - 1;
    u64 h = mrule::mix(key) & mask;                                   // h <= mask: inside every array
    for (u64 p = 0; p <= mask; p++) {
        const u64 k = t.key[h];
        if (k == key) return (long long)h;
        if (k == mrule::kEmpty) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// pass 0 reads the start poses (float, as the caller gave them), a later pass the trial pose of the query's state.  kTerms (icet_debug_voxel_map_register_terms):
// every row's record goes to terms[] as well, through the same loads, probe and arithmetic.
template <bool kTerms>
__global__ __launch_bounds__(kRegBlock) void k_mapreg_rows(const RegScan* __restrict__ scans, int n_q, const float* __restrict__ poses, int pass,
                                                           const rr::State* __restrict__ state, rr::Consts kc, RegTable t, const rr::Gauss* __restrict__ gauss,
                                                           Partial* __restrict__ part, icet_voxel_map_register_term* __restrict__ terms) {
    __shared__ double sv[kRegWaves][rr::kSums];
    __shared__ int32_t sn[kRegWaves][2];
    __shared__ double sP[12];
    // the query of this block: the last one whose first block is not behind it (a query without rows has no block)
    int lo = 0, hi = n_q - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (scans[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const RegScan sc = scans[lo];
    const int row0 = ((int)blockIdx.x - sc.block0) * kRowsPerBlock;
    if (row0 < 0 || row0 >= sc.n) return;                             // (the same for every thread of the block)
    if (pass > 0 && state[lo].status != rr::kIterationCap) return;    // (the same too) a terminal query is frozen
    const int end = min(sc.n, row0 + kRowsPerBlock);
    if (threadIdx.x < 12) {
        const int j = threadIdx.x;
        if (pass == 0) sP[j] = (double)(j < 9 ? poses[16 * (size_t)lo + 4 * (j / 3) + j % 3] : poses[16 * (size_t)lo + 4 * (j - 9) + 3]);
        else sP[j] = j < 9 ? state[lo].trial.R[j] : state[lo].trial.t[j - 9];
    }
    __syncthreads();
    rr::Pose P;
#pragma unroll
    for (int j = 0; j < 9; j++) P.R[j] = sP[j];
#pragma unroll
    for (int a = 0; a < 3; a++) P.t[a] = sP[9 + a];
    const float* cx = sc.ptr; const float* cy = cx + sc.ld; const float* cz = cx + 2 * (size_t)sc.ld;
    rr::Acc acc;
    rr::acc_zero(acc);
    for (int i = row0 + 4 * (int)threadIdx.x; i < end; i += 4 * kRegBlock) {
        const int m = min(4, end - i);
        float x[4], y[4], z[4];
        load_rows(cx, i, m, x); load_rows(cy, i, m, y); load_rows(cz, i, m, z);
        for (int r = 0; r < m; r++) {
            int cls = rr::row_class(kc, x[r], y[r], z[r]);
            uint64_t key = mrule::kEmpty;
            bool matched = false;
            rr::Terms tm;
            if (cls == mrule::kRowKept) {
                double rv[3], w[3];
                const bool in = rr::row_world(kc, P, x[r], y[r], z[r], rv, w, key);
                if (!in) cls = mrule::kRowOutside;
                const long long e = in ? probe(t, key) : -1;
                if (e >= 0 && gauss[e].n > 0) {
                    const rr::Gauss G = gauss[e];                     // e < size: an entry's index
                    rr::match_terms(kc, G, rv, w, tm);
                    matched = true;
                } else {
                    rr::miss_terms(kc, tm);
                }
                rr::acc_row(acc, tm, matched);
            }
            if (kTerms) {
                icet_voxel_map_register_term o;                       // i + r < end <= sc.n: inside the caller's records
                const bool scored = cls == mrule::kRowKept || cls == mrule::kRowOutside;
                o.key = key; o.cls = cls; o.matched = matched ? 1 : 0;
                o.s = scored ? tm.s : 0.0; o.omega = scored ? tm.omega : 0.0; o.rho = scored ? tm.rho : 0.0;
                for (int j = 0; j < 6; j++) o.g[j] = scored ? tm.v[1 + j] : 0.0;
                for (int j = 0; j < 21; j++) o.H[j] = scored ? tm.v[7 + j] : 0.0;
                terms[i + r] = o;
            }
        }
    }
    // the thread, then a fixed butterfly over the wave (every lane ends with the same bits), then the waves in order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < rr::kSums; j++) {
        double v = acc.v[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
        if (lane == 0) sv[wave][j] = v;
    }
    int32_t ns = acc.scored, nm = acc.matched;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { ns += __shfl_xor(ns, off, 64); nm += __shfl_xor(nm, off, 64); }
    if (lane == 0) { sn[wave][0] = ns; sn[wave][1] = nm; }
    __syncthreads();
    Partial* out = part + blockIdx.x;
    if (threadIdx.x < rr::kSums) {
        double s = sv[0][threadIdx.x];
        for (int w = 1; w < kRegWaves; w++) s = s + sv[w][threadIdx.x];
        out->v[threadIdx.x] = s;
    } else if (threadIdx.x < rr::kSums + 2) {
        const int c = threadIdx.x - rr::kSums;
        int32_t s = 0;
        for (int w = 0; w < kRegWaves; w++) s += sn[w][c];
        if (c == 0) out->scored = s; else out->matched = s;
    }
}

// ---- the row pass under a neighbourhood ------------------------------------------------------------------------------------------------------------------------
// k_mapreg_rows' own steps as functions, for k_mapreg_rows_nb: k_mapreg_rows keeps its text, and with it its machine code (scripts/isa_compare.py), word for word.
// The query of this block: the last one whose first block is not behind it (a query without rows has no block).
__device__ __forceinline__ int query_of_block(const RegScan* __restrict__ scans, int n_q) {
    int lo = 0, hi = n_q - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (scans[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    return lo;
}

// The pose of query q in this pass, through sP (12 doubles of LDS) into every thread: pass 0 reads the start pose, a later pass the trial pose of the state.
__device__ __forceinline__ void stage_pose(double* sP, const float* __restrict__ poses, int pass, const rr::State* __restrict__ state, int q, rr::Pose& P) {
    if (threadIdx.x < 12) {
        const int j = threadIdx.x;
        if (pass == 0) sP[j] = (double)(j < 9 ? poses[16 * (size_t)q + 4 * (j / 3) + j % 3] : poses[16 * (size_t)q + 4 * (j - 9) + 3]);
        else sP[j] = j < 9 ? state[q].trial.R[j] : state[q].trial.t[j - 9];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 9; j++) P.R[j] = sP[j];
#pragma unroll
    for (int a = 0; a < 3; a++) P.t[a] = sP[9 + a];
}

// A block's partial from its threads' sums: the thread, then a fixed butterfly over the wave (every lane ends with the same bits), then the waves in order.
__device__ __forceinline__ void reduce_block(const rr::Acc& acc, double (*sv)[rr::kSums], int32_t (*sn)[2], Partial* out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < rr::kSums; j++) {
        double v = acc.v[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
        if (lane == 0) sv[wave][j] = v;
    }
    int32_t ns = acc.scored, nm = acc.matched;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { ns += __shfl_xor(ns, off, 64); nm += __shfl_xor(nm, off, 64); }
    if (lane == 0) { sn[wave][0] = ns; sn[wave][1] = nm; }
    __syncthreads();
    if (threadIdx.x < rr::kSums) {
        double s = sv[0][threadIdx.x];
        for (int w = 1; w < kRegWaves; w++) s = s + sv[w][threadIdx.x];
        out->v[threadIdx.x] = s;
    } else if (threadIdx.x < rr::kSums + 2) {
        const int c = threadIdx.x - rr::kSums;
        int32_t s = 0;
        for (int w = 0; w < kRegWaves; w++) s += sn[w][c];
        if (c == 0) out->scored = s; else out->matched = s;
    }
}

// probe() with the first key already loaded, entries as 32-bit words (the table has at most 2^31 of them: map_register): k = t.key[h], h = mix(key) & mask.
// The same answer as probe(t, key), at most `size` keys compared.
__device__ __forceinline__ int32_t probe_from(const RegTable& t, u64 key, uint32_t h, u64 k) {
    const uint32_t mask = (uint32_t)(((u64)1 << t.log2) - 1);
    for (uint32_t p = 0; p <= mask; p++) {
        if (k == key) return (int32_t)h;
        if (k == mrule::kEmpty) return -1;
        h = (h + 1) & mask;                                           // h <= mask: inside every array
        k = t.key[h];
        if (p == mask) break;                                         // (mask may be all ones: no p + 1 past it)
    }
    return -1;
}

// The cell of the neighbourhood of K cells around `own` that the world point w is scored against (icet_map_register.h: the smallest s, the earlier place on a
// tie): its entry, or -1, and its place.  A batch of cells at a time: their first probes together (independent 8-byte reads that overlap), then the entries,
// then the records kGroup at a time -- each read whole from an entry inside the table (entry 0 for a cell that has none, its s not offered: measured faster than
// a load under the lane's own condition) and dropped once its s is known.  Between batches a thread keeps the winner's entry, place and s and nothing else.
constexpr int kGroup = 3;

// One batch: cell j of the kBatch has the key key_of(j) (kEmpty: outside the grid, read but never probed) and the place place_of(j).  kOrdered: the cells come in
// the order of the places and the plain comparison selects (measured: the (s, place) comparison where it is not needed costs the 7-cell pass 15 %).
template <int kBatch, bool kOrdered, class KeyOf, class PlaceOf>
__device__ __forceinline__ void select_batch(const RegTable& t, const rr::Gauss* __restrict__ gauss, const double w[3], KeyOf key_of, PlaceOf place_of,
                                             rr::Best& best, int32_t& slot) {
    const uint32_t mask = (uint32_t)(((u64)1 << t.log2) - 1);
    uint32_t h[kBatch];
    u64 k0[kBatch];
    int32_t e[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; j++) {
        h[j] = (uint32_t)mrule::mix(key_of(j)) & mask;                // h <= mask: inside every array
        k0[j] = t.key[h[j]];
    }
#pragma unroll
    for (int j = 0; j < kBatch; j++) {
        const u64 key = key_of(j);
        e[j] = key != mrule::kEmpty ? probe_from(t, key, h[j], k0[j]) : -1;
    }
#pragma unroll
    for (int g0 = 0; g0 < kBatch; g0 += kGroup) {
        double s[kGroup]; bool ok[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; j++) {
            if (g0 + j >= kBatch) { ok[j] = false; s[j] = 0.0; continue; }
            const rr::Gauss G = gauss[e[g0 + j] >= 0 ? e[g0 + j] : 0];          // an entry's index, or entry 0: inside the records
            ok[j] = e[g0 + j] >= 0 && G.n > 0;
            s[j] = rr::match_s(G, w);
        }
#pragma unroll
        for (int j = 0; j < kGroup; j++)
            if (g0 + j < kBatch && ok[j] && (kOrdered ? rr::best_offer(best, place_of(g0 + j), s[j]) : rr::best_offer_any(best, place_of(g0 + j), s[j]))) slot = e[g0 + j];
        __builtin_amdgcn_sched_barrier(0);                            // the next group's records are not loaded before these are dropped
    }
}

template <int K>
__device__ __forceinline__ int32_t select_cell(const RegTable& t, const rr::Gauss* __restrict__ gauss, uint64_t own, const double w[3], int& place);

// 7 cells: one batch, in the order of the places, every offset a compile-time constant.
template <>
__device__ __forceinline__ int32_t select_cell<7>(const RegTable& t, const rr::Gauss* __restrict__ gauss, uint64_t own, const double w[3], int& place) {
    rr::Best best;
    rr::best_start(best);
    int32_t slot = -1;
    select_batch<7, true>(t, gauss, w, [&](int j) { uint64_t key; rr::neighbour_key(7, j, own, key); return (u64)key; }, [](int j) { return j; }, best, slot);
    place = best.place;
    return slot;
}

// 27 cells: one batch per x slice (a rolled loop: unrolled, the three batches' loads are hoisted together and the pass spills), the nine (dy, dz) offsets of a
// slice compile-time constants.  The cells are offered out of the order of the places -- the own cell in the middle of the second slice -- which the (s, place)
// comparison of best_offer_any makes the same selection.
template <>
__device__ __forceinline__ int32_t select_cell<27>(const RegTable& t, const rr::Gauss* __restrict__ gauss, uint64_t own, const double w[3], int& place) {
    rr::Best best;
    rr::best_start(best);
    int32_t slot = -1;
    int32_t c[3];
    mrule::key_cells(own, c);
#pragma nounroll
    for (int dx = -1; dx <= 1; dx++) {
        const int32_t cx = c[0] + dx;
        const bool inx = cx > -mrule::kCellLimit && cx < mrule::kCellLimit;
        auto key_of = [&](int j) {
            const int32_t cy = c[1] + (j / 3 - 1), cz = c[2] + (j % 3 - 1);
            const bool in = inx && cy > -mrule::kCellLimit && cy < mrule::kCellLimit && cz > -mrule::kCellLimit && cz < mrule::kCellLimit;
            return in ? (u64)mrule::make_key(cx, cy, cz) : (u64)mrule::kEmpty;
        };
        select_batch<9, false>(t, gauss, w, key_of, [&](int j) { return rr::place27(dx, j / 3 - 1, j % 3 - 1); }, best, slot);
    }
    place = best.place;
    return slot;
}

// k_mapreg_rows under a neighbourhood of K cells: the same launch shape, loads, pose, sums and partial; a record's `matched` is 1 + the winner's place.
template <int K, bool kTerms>
__global__ __launch_bounds__(kRegBlock, 2) void k_mapreg_rows_nb(const RegScan* __restrict__ scans, int n_q, const float* __restrict__ poses, int pass,
                                                                 const rr::State* __restrict__ state, rr::Consts kc, RegTable t, const rr::Gauss* __restrict__ gauss,
                                                                 Partial* __restrict__ part, icet_voxel_map_register_term* __restrict__ terms) {
    __shared__ double sv[kRegWaves][rr::kSums];
    __shared__ int32_t sn[kRegWaves][2];
    __shared__ double sP[12];
    const int lo = query_of_block(scans, n_q);
    const RegScan sc = scans[lo];
    const int row0 = ((int)blockIdx.x - sc.block0) * kRowsPerBlock;
    if (row0 < 0 || row0 >= sc.n) return;                             // (the same for every thread of the block)
    if (pass > 0 && state[lo].status != rr::kIterationCap) return;    // (the same too) a terminal query is frozen
    const int end = min(sc.n, row0 + kRowsPerBlock);
    rr::Pose P;
    stage_pose(sP, poses, pass, state, lo, P);
    const float* cx = sc.ptr; const float* cy = cx + sc.ld; const float* cz = cx + 2 * (size_t)sc.ld;
    rr::Acc acc;
    rr::acc_zero(acc);
    for (int i = row0 + 4 * (int)threadIdx.x; i < end; i += 4 * kRegBlock) {
        const int m = min(4, end - i);
        float x[4], y[4], z[4];
        load_rows(cx, i, m, x); load_rows(cy, i, m, y); load_rows(cz, i, m, z);
        for (int r = 0; r < m; r++) {
            int cls = rr::row_class(kc, x[r], y[r], z[r]);
            uint64_t key = mrule::kEmpty;
            int place = -1;
            rr::Terms tm;
            if (cls == mrule::kRowKept) {
                double rv[3], w[3];
                const bool in = rr::row_world(kc, P, x[r], y[r], z[r], rv, w, key);
                if (!in) cls = mrule::kRowOutside;
                const int32_t e = in ? select_cell<K>(t, gauss, key, w, place) : -1;
                if (e >= 0) {
                    const rr::Gauss G = gauss[e];                     // the winner's record again (e < size: an entry's index)
                    rr::match_terms(kc, G, rv, w, tm);
                } else {
                    rr::miss_terms(kc, tm);
                }
                rr::acc_row(acc, tm, e >= 0);
            }
            if (kTerms) {
                icet_voxel_map_register_term o;                       // i + r < end <= sc.n: inside the caller's records
                const bool scored = cls == mrule::kRowKept || cls == mrule::kRowOutside;
                o.key = key; o.cls = cls; o.matched = place + 1;
                o.s = scored ? tm.s : 0.0; o.omega = scored ? tm.omega : 0.0; o.rho = scored ? tm.rho : 0.0;
                for (int j = 0; j < 6; j++) o.g[j] = scored ? tm.v[1 + j] : 0.0;
                for (int j = 0; j < 21; j++) o.H[j] = scored ? tm.v[7 + j] : 0.0;
                terms[i + r] = o;
            }
        }
    }
    reduce_block(acc, sv, sn, part + blockIdx.x);
}

__global__ __launch_bounds__(kStepBlock) void k_mapreg_step(const RegScan* __restrict__ scans, const float* __restrict__ poses, int pass, rr::Consts kc,
                                                            const Partial* __restrict__ part, rr::State* __restrict__ state, rr::Record* __restrict__ recs) {
    __shared__ rr::Acc tot;
    __shared__ rr::State st;
    __shared__ rr::Record rec;
    const int q = blockIdx.x;
    if (pass > 0 && state[q].status != rr::kIterationCap) return;     // (the same for every thread of the block) frozen: its state and record stay
    const RegScan sc = scans[q];
    const Partial* pq = part + sc.block0;                             // the query's sc.chunks partials, written by this pass's row blocks
    if (threadIdx.x < rr::kSums) {
        double s = 0.0;
        for (int c = 0; c < sc.chunks; c++) s = s + pq[c].v[threadIdx.x];
        tot.v[threadIdx.x] = s;
    } else if (threadIdx.x < rr::kSums + 2) {
        const bool first = threadIdx.x == rr::kSums;
        int32_t s = 0;
        for (int c = 0; c < sc.chunks; c++) s += first ? pq[c].scored : pq[c].matched;
        if (first) tot.scored = s; else tot.matched = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (pass > 0) st = state[q];
        float start[16];
        for (int j = 0; j < 16; j++) start[j] = poses[16 * (size_t)q + j];
        rr::step(kc, pass, start, tot, st, rec);
        state[q] = st;
        recs[q] = rec;
    }
}

// What a map keeps for its registrations, behind the slot of map_register_view: the Gaussians and what they were built from, the stage of a call (the queries'
// descriptors and poses, pinned and on the device, behind a read fence), the partials and the states.
struct RegState {
    rr::Gauss* gauss = nullptr; bool built = false; uint64_t built_gen = 0; double sigma_min = 0.0; int32_t min_points = 0;
    RegScan* h_rec = nullptr; RegScan* d_rec = nullptr; float* h_pose = nullptr; float* d_pose = nullptr; rr::State* state = nullptr; int32_t cap_q = 0;
    Partial* part = nullptr; int64_t cap_part = 0;
    ReadFence fence;
    BufferGroup gmem, stage, work;
    ~RegState() { fence.destroy(); }
};
void reg_free(void* p) { delete static_cast<RegState*>(p); }

icet_status reg_refuse(icet_voxel_map* m, const std::string& why) { map_set_error(m, why.c_str()); return ICET_ERR_BAD_ARG; }

#define REGCHK(m, call) do { const hipError_t e_ = static_cast<hipError_t>(call); if (e_ != hipSuccess) { \
    (void)hipGetLastError(); map_set_error((m), (std::string(#call) + ": " + hipGetErrorString(e_)).c_str()); \
    return e_ == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; } } while (0)

template <class T> bool aligned_to(const T* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// The row pass of the call's neighbourhood: nb = 1 is k_mapreg_rows, the centre-only pass, unchanged.
void launch_rows(int nb, bool terms, unsigned blocks, hipStream_t st, const RegScan* scans, int n_q, const float* poses, int pass, const rr::State* state, const rr::Consts& kc,
                 const RegTable& t, const rr::Gauss* gauss, Partial* part, icet_voxel_map_register_term* d_terms) {
    auto k = nb == 27 ? (terms ? k_mapreg_rows_nb<27, true> : k_mapreg_rows_nb<27, false>)
           : nb == 7 ? (terms ? k_mapreg_rows_nb<7, true> : k_mapreg_rows_nb<7, false>)
                     : (terms ? k_mapreg_rows<true> : k_mapreg_rows<false>);
    k<<<blocks, kRegBlock, 0, st>>>(scans, n_q, poses, pass, state, kc, t, gauss, part, d_terms);
}

// terms: the debug form -- one query, the row pass of the start pose with a record per row, no step.
icet_status map_register(icet_voxel_map* m, int32_t n_q, const icet_dev_scan* scans, const float* poses, bool poses_on_device, const icet_voxel_map_register_params* params,
                         icet_voxel_map_registration* d_records, icet_voxel_map_register_term* d_terms, bool terms, const char* call) {
    MapRegisterView v;
    if (!map_register_view(m, &v)) return ICET_ERR_BAD_ARG;
    const icet_status entered = enter(v.ctx);
    if (entered != ICET_OK) { map_set_error(m, v.ctx->err.c_str()); return entered; }
    // everything is checked before anything is touched
    const std::string who(call);
    icet_voxel_map_register_params p;
    if (params) p = *params;
    else { std::memset(&p, 0, sizeof(p)); p.sigma_min = 0.02; p.scale = 11.3449; p.tol_t = 1e-4; p.tol_r = 1e-5; p.lambda0 = 1e-3; p.min_points = 5; p.min_matched = 50; p.max_iters = 20; }
    if (!v.mom) return reg_refuse(m, who + ": the map has no shape (icet_voxel_map_enable_shape on an empty map)");
    if (v.log2 > 31) return reg_refuse(m, who + ": the table is too large (the row pass keeps an entry in 32 bits)");
    if (n_q < 1 || n_q > rr::kMaxQueries) return reg_refuse(m, who + ": n_q must lie in 1 .. 256");
    if (!scans || !poses || (terms ? !d_terms : !d_records)) return reg_refuse(m, who + ": bad argument (a NULL array)");
    const int nb = rr::neighbours_of(p.flags);                        // 1, 7 or 27 cells per row; 0: flags that name no neighbourhood
    if (!rr::params_ok(p.min_range, p.max_range, p.sigma_min, p.scale, p.tol_t, p.tol_r, p.lambda0, p.max_iters, 0) || nb == 0 || p.reserved[0] || p.reserved[1])
        return reg_refuse(m, who + ": sigma_min, scale and lambda0 must be finite and > 0, the tolerances finite and >= 0, the ranges finite, max_iters 0 .. 64, flags 0 or ONE of "
                                   "ICET_VOXEL_MAP_REG_NEIGHBOURS_7 / _27, the reserved words 0");
    if ((poses_on_device && !aligned_to(poses, 4)) || !aligned_to(d_records, 8) || !aligned_to(d_terms, 8))
        return reg_refuse(m, who + ": a device pointer is not aligned to its element");
    int64_t blocks = 0;
    for (int k = 0; k < n_q; k++) {
        if (!dev_scan_ok(scans[k]) || !aligned_to(scans[k].ptr, 4)) return reg_refuse(m, who + ": bad scan descriptor (scans[" + std::to_string(k) + "])");
        blocks += (scans[k].n + kRowsPerBlock - 1) / kRowsPerBlock;
    }
    if (blocks > 0x7FFFFFFF) return reg_refuse(m, who + ": too many rows in one call");

    hipStream_t st = v.ctx->stream;
    RegState* s = static_cast<RegState*>(*v.reg);
    if (!s) {
        s = new (std::nothrow) RegState();
        if (!s) { map_set_error(m, "host allocation failed"); return ICET_ERR_NOMEM; }
        *v.reg = s; *v.reg_free = reg_free;
    }
    const size_t size = (size_t)1 << v.log2;
    if (!s->gauss) { s->built = false; REGCHK(m, s->gmem.device(s->gauss, size)); }
    // the buffers: each group grows behind a drained stream (an earlier call's kernels may still read the old ones)
    REGCHK(m, s->fence.wait());
    if (n_q > s->cap_q) {
        REGCHK(m, hipStreamSynchronize(st));
        BufferGroup& g = s->stage;
        REGCHK(m, grow(g, s->cap_q, n_q, [&] {
            int a = g.pinned(s->h_rec, (size_t)n_q);
            if (!a) a = g.device(s->d_rec, (size_t)n_q);
            if (!a) a = g.pinned(s->h_pose, 16 * (size_t)n_q);
            if (!a) a = g.device(s->d_pose, 16 * (size_t)n_q);
            if (!a) a = g.device(s->state, (size_t)n_q);
            return a;
        }));
    }
    if (blocks > s->cap_part) {
        REGCHK(m, hipStreamSynchronize(st));
        BufferGroup& g = s->work;
        REGCHK(m, grow(g, s->cap_part, blocks, [&] { return g.device(s->part, (size_t)blocks); }));
    }
    const rr::Consts kc = rr::make_consts(v.cell, p.min_range, p.max_range, p.sigma_min, p.scale, p.tol_t, p.tol_r, p.lambda0, p.min_points, p.min_matched, p.max_iters);
    const RegTable t{v.key, v.count, v.sum, v.mom, v.log2};
    if (!s->built || s->built_gen != v.generation || s->sigma_min != p.sigma_min || s->min_points != kc.min_points) {
        s->built = false;
        k_mapreg_gauss<<<(unsigned)((size + kRegBlock - 1) / kRegBlock), kRegBlock, 0, st>>>(t, kc, s->gauss);
        REGCHK(m, hipGetLastError());
        s->built = true; s->built_gen = v.generation; s->sigma_min = p.sigma_min; s->min_points = kc.min_points;
    }
    int32_t b0 = 0;
    for (int k = 0; k < n_q; k++) {
        const int32_t chunks = (int32_t)((scans[k].n + kRowsPerBlock - 1) / kRowsPerBlock);
        s->h_rec[k] = RegScan{scans[k].ptr, (int32_t)scans[k].n, (int32_t)scans[k].ld, b0, chunks};
        b0 += chunks;
    }
    REGCHK(m, hipMemcpyAsync(s->d_rec, s->h_rec, sizeof(RegScan) * (size_t)n_q, hipMemcpyHostToDevice, st));
    const float* dp = poses;
    if (!poses_on_device) {
        std::memcpy(s->h_pose, poses, sizeof(float) * 16 * (size_t)n_q);
        REGCHK(m, hipMemcpyAsync(s->d_pose, s->h_pose, sizeof(float) * 16 * (size_t)n_q, hipMemcpyHostToDevice, st));
        dp = s->d_pose;
    }
    if (terms) {
        if (blocks > 0) {
            launch_rows(nb, true, (unsigned)blocks, st, s->d_rec, n_q, dp, 0, s->state, kc, t, s->gauss, s->part, d_terms);
            REGCHK(m, hipGetLastError());
        }
    } else {
        rr::Record* recs = reinterpret_cast<rr::Record*>(d_records);
        for (int pass = 0; pass <= p.max_iters; pass++) {
            if (blocks > 0) {
                launch_rows(nb, false, (unsigned)blocks, st, s->d_rec, n_q, dp, pass, s->state, kc, t, s->gauss, s->part, nullptr);
                REGCHK(m, hipGetLastError());
            }
            k_mapreg_step<<<(unsigned)n_q, kStepBlock, 0, st>>>(s->d_rec, dp, pass, kc, s->part, s->state, recs);
            REGCHK(m, hipGetLastError());
        }
    }
    REGCHK(m, s->fence.mark(st));
    return ICET_OK;
}

}  // namespace
}  // namespace icet

using namespace icet;

extern "C" {

icet_status icet_voxel_map_register_device(icet_voxel_map* m, int32_t n_q, const icet_dev_scan* scans, const float* poses, const icet_voxel_map_register_params* params,
                                           icet_voxel_map_registration* d_records) {
    return map_register(m, n_q, scans, poses, false, params, d_records, nullptr, false, "icet_voxel_map_register_device");
}

icet_status icet_voxel_map_register_posed_device(icet_voxel_map* m, int32_t n_q, const icet_dev_scan* scans, const float* d_poses, const icet_voxel_map_register_params* params,
                                                 icet_voxel_map_registration* d_records) {
    return map_register(m, n_q, scans, d_poses, true, params, d_records, nullptr, false, "icet_voxel_map_register_posed_device");
}

icet_status icet_debug_voxel_map_register_terms(icet_voxel_map* m, const icet_dev_scan* scan, const float* pose, const icet_voxel_map_register_params* params,
                                                icet_voxel_map_register_term* d_terms) {
    return map_register(m, 1, scan, pose, false, params, nullptr, d_terms, true, "icet_debug_voxel_map_register_terms");
}

}  // extern "C"
