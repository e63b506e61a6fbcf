// icet_amd/csrc/icet_closure.hip -- the loop-closure query of the keyframe store (include/icet_hip.h icet_keyframe_store_close_device).
// The rule -- distance, key, eligibility, start pose -- is icet_closure.h; this file is the kernels around it:
//     k_closure_set_pose / k_closure_clear_pose   the store's pose table (arrays of `cap` entries: stamp | tx | ty | tz | r0 .. r8; a slot without a pose holds NaN)
//     k_closure_search_tiles                      pass 1: every block reduces its tile of 1024 slots to its K smallest keys for each of the Q queries (a wave per query)
//     k_closure_search_merge                      pass 2: one block per query merges the tiles' lists into the K candidates (the appearance search's pass 2 as well)
//     k_closure_resolve                           one thread per (query, candidate): X0 of its S starts, keyframe index and row count of its registrations
//     k_closure_apply                             the keyframe indices into the indexed loop's table, behind that loop's own descriptor upload
//     k_closure_record                            one thread per query: the winner's row, score, X0, the shift of an appearance query, and the acceptance gate
// Keys are (bits(d2) << 32) | slot, unique per slot, and both passes select minima of u64 keys: no float atomic, no dependence on the launch shape.
#include <hip/hip_runtime.h>
#include "../../include/icet_hip.h"
#include "icet_internal.h"
#include "icet_closure.h"
#include "icet_closure_device.h"

namespace icet {
namespace {

using icet_closure_rule::kNoKey;

// Pass 1.  part[(q * gridDim.x + block) * K + k]: the block's k-th smallest key of query q (kNoKey behind the last).  The block reads its tile of slots once,
// into LDS, for all queries; wave w then takes the queries w, w + 4, ...: a lane holds the keys of 16 slots in registers and the wave selects its K smallest
// (select_tile_smallest).
__global__ __launch_bounds__(kSelectBlock) void k_closure_search_tiles(PoseTable tab, ClosureSearchArgs qa, int n_queries, int K, float r2, int64_t min_gap,
                                                                       unsigned long long* __restrict__ part) {
    __shared__ float lx[kClosureTile], ly[kClosureTile], lz[kClosureTile];
    __shared__ int64_t ls[kClosureTile];
    const int base = blockIdx.x * kClosureTile;
    for (int i = threadIdx.x; i < kClosureTile; i += kSelectBlock) {
        const int slot = base + i;
        const bool in = slot < tab.cap;
        lx[i] = in ? tab.f[slot] : __builtin_nanf("");
        ly[i] = in ? tab.f[(size_t)tab.cap + slot] : __builtin_nanf("");
        lz[i] = in ? tab.f[2 * (size_t)tab.cap + slot] : __builtin_nanf("");
        ls[i] = in ? tab.stamp[slot] : 0;
    }
    __syncthreads();
    select_tile_smallest(n_queries, K, part, [&](int q, int s) {
        return icet_closure_rule::candidate_key(qa.tx[q], qa.ty[q], qa.tz[q], qa.stamp[q], lx[s], ly[s], lz[s], ls[s], r2, min_gap, base + s);
    });
}

// Pass 2.  One block per query: the K smallest of the n_tiles x K keys pass 1 left, by K rounds of "the smallest key above the previous one" (keys are distinct).
__global__ __launch_bounds__(kSelectBlock) void k_closure_search_merge(const unsigned long long* __restrict__ part, int n_tiles, int K,
                                                                       int32_t* __restrict__ cand, unsigned long long* __restrict__ keys) {
    __shared__ uint64_t wmin[2][4];
    const int q = blockIdx.x;
    const unsigned long long* in = part + (size_t)q * n_tiles * K;
    const int n = n_tiles * K;
    uint64_t prev = 0; bool have_prev = false;
    uint64_t reg[kMergeRegs];                                          // the first 256 x kMergeRegs keys stay in registers: read once, not once per round
#pragma unroll
    for (int i = 0; i < kMergeRegs; i++) { const int j = threadIdx.x + kSelectBlock * i; reg[i] = j < n ? in[j] : kNoKey; }
    int k = 0;
    for (; k < K; k++) {
        uint64_t m = kNoKey;
#pragma unroll
        for (int i = 0; i < kMergeRegs; i++) { const uint64_t v = reg[i]; if ((!have_prev || v > prev) && v < m) m = v; }
        for (int i = threadIdx.x + kSelectBlock * kMergeRegs; i < n; i += kSelectBlock) { const uint64_t v = in[i]; if ((!have_prev || v > prev) && v < m) m = v; }
        const uint64_t b = block_min_u64(m, wmin, k);
        if (b == kNoKey) break;
        if (threadIdx.x == 0) { cand[q * K + k] = icet_closure_rule::key_slot(b); keys[q * K + k] = b; }
        prev = b; have_prev = true;
    }
    for (int j = k + threadIdx.x; j < K; j += kSelectBlock) { cand[q * K + j] = -1; keys[q * K + j] = kNoKey; }
}

// One thread per (query, candidate).  x0_base (may be null): Q x K x 6, zeros for a missing candidate.  With n_starts > 0 the registrations
// r = (q K + k) S + s of the indexed call behind it (write_registrations).
__global__ __launch_bounds__(64) void k_closure_resolve(PoseTable tab, ClosurePoseArgs pa, int n_queries, int K, int n_starts, int any_slot,
                                                        const int32_t* __restrict__ cand, float* __restrict__ x0_base, float* __restrict__ x0,
                                                        int32_t* __restrict__ kf_of, int32_t* __restrict__ rows, int32_t* __restrict__ members, int32_t* __restrict__ offs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    write_group_offset(i, n_queries, K, n_starts, offs);
    if (i >= n_queries * K) return;
    const int q = i / K;
    const int slot = cand[i];
    float b[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (slot >= 0) {
        float Rj[9], tj[3];
        for (int a = 0; a < 3; a++) tj[a] = tab.f[(size_t)a * tab.cap + slot];
        for (int a = 0; a < 9; a++) Rj[a] = tab.f[(size_t)(3 + a) * tab.cap + slot];
        icet_closure_rule::start_pose(pa.R[q], pa.t[q], Rj, tj, b);
    }
    if (x0_base) for (int c = 0; c < 6; c++) x0_base[(size_t)i * 6 + c] = b[c];
    write_registrations(i, slot, any_slot, b, pa.off, n_starts, x0, kf_of, rows, members);
}

__global__ void k_closure_apply(int32_t* __restrict__ dst, const int32_t* __restrict__ src, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// One thread per query.  best == nullptr: no registration ran (a store without an occupied slot): every record is "none".  shift_of (null by pose): the
// candidates' shifts of an appearance query, whose record carries the appearance distance in d2 and the winner's shift in reserved0.
__global__ __launch_bounds__(64) void k_closure_record(PoseTable tab, int n_queries, int K, int n_starts, float max_chi2_per_voxel, int min_voxels,
                                                       const int32_t* __restrict__ best, const int32_t* __restrict__ cand, const unsigned long long* __restrict__ keys,
                                                       const int32_t* __restrict__ shift_of, const float* __restrict__ x0, const float* __restrict__ out, const icet_score* __restrict__ score,
                                                       icet_closure* __restrict__ rec) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries) return;
    icet_closure c;
    int nc = 0;
    for (int k = 0; k < K; k++) nc += cand[q * K + k] >= 0 ? 1 : 0;
    int r = best ? best[q] : -1;
    if (r >= 0 && cand[r / n_starts] < 0) r = -1;                     // (a padding registration scores no voxel and is never elected)
    c.n_candidates = nc; c.reg = r; c.reserved0 = 0; c.reserved1[0] = 0; c.reserved1[1] = 0;
    if (r >= 0) {
        const int i = r / n_starts;                                   // q K + k
        const int slot = cand[i];
        c.slot = slot; c.stamp = tab.stamp[slot]; c.d2 = icet_closure_rule::key_d2(keys[i]);
        if (shift_of) c.reserved0 = shift_of[i];
        for (int k = 0; k < 6; k++) c.x0[k] = x0[(size_t)r * 6 + k];
        for (int k = 0; k < 48; k++) c.out[k] = out[(size_t)r * 48 + k];
        c.score = score[r];
        c.accepted = (slot >= 0 && c.score.chi2_per_voxel <= max_chi2_per_voxel && c.score.voxels >= min_voxels) ? 1 : 0;
    } else {
        c.slot = -1; c.stamp = 0; c.d2 = 0.f; c.accepted = 0;
        for (int k = 0; k < 6; k++) c.x0[k] = 0.f;
        for (int k = 0; k < 48; k++) c.out[k] = 0.f;
        c.score.chi2 = 0.f; c.score.chi2_per_voxel = 0.f; c.score.voxels = 0; c.score.points_in = 0; c.score.points = 0; c.score.overlap = 0.f;
        c.score.reserved[0] = 0; c.score.reserved[1] = 0;
    }
    rec[q] = c;
}

// up: pinned host staging, read by the kernel itself (no copy command)
__global__ void k_closure_set_pose(PoseTable tab, const PoseUpload* __restrict__ up, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PoseUpload u = up[i];
    if (u.slot < 0 || u.slot >= tab.cap) return;
    tab.stamp[u.slot] = u.stamp;
    for (int a = 0; a < 12; a++) tab.f[(size_t)a * tab.cap + u.slot] = u.tR[a];
}

__global__ void k_closure_clear_pose(PoseTable tab, StoreParkSlots slots, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int slot = slots.slot[i];
    if (slot < 0 || slot >= tab.cap) return;
    tab.stamp[slot] = -1;
    for (int a = 0; a < 12; a++) tab.f[(size_t)a * tab.cap + slot] = __uint_as_float(0xFFFFFFFFu);      // (the bytes of an empty table: NaN)
}

}  // namespace

int closure_tiles(int32_t cap) { return (int)(((int64_t)cap + kClosureTile - 1) / kClosureTile); }

hipError_t launch_closure_search(const PoseTable& tab, const ClosureSearchArgs& qa, int n_queries, int K, float radius, int64_t min_gap,
                                 unsigned long long* d_part, int32_t* d_cand, unsigned long long* d_keys, hipStream_t st) {
    const int tiles = closure_tiles(tab.cap);
    k_closure_search_tiles<<<tiles, kSelectBlock, 0, st>>>(tab, qa, n_queries, K, icet_closure_rule::radius2(radius), min_gap, d_part);
    ICET_LAUNCH_CHECK();
    return launch_closure_merge(d_part, tiles, n_queries, K, d_cand, d_keys, st);
}

hipError_t launch_closure_merge(const unsigned long long* d_part, int tiles, int n_queries, int K, int32_t* d_cand, unsigned long long* d_keys, hipStream_t st) {
    k_closure_search_merge<<<n_queries, kSelectBlock, 0, st>>>(d_part, tiles, K, d_cand, d_keys);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_closure_resolve(const PoseTable& tab, const ClosurePoseArgs& pa, int n_queries, int K, int n_starts, int any_slot, const int32_t* d_cand,
                                  float* d_x0_base, float* d_x0, int32_t* d_kf_of, int32_t* d_rows, int32_t* d_members, int32_t* d_offs, hipStream_t st) {
    const int n = n_queries * K > n_queries + 1 ? n_queries * K : n_queries + 1;
    k_closure_resolve<<<(n + 63) / 64, 64, 0, st>>>(tab, pa, n_queries, K, n_starts, any_slot, d_cand, d_x0_base, d_x0, d_kf_of, d_rows, d_members, d_offs);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_closure_apply(int32_t* dst, const int32_t* src, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    k_closure_apply<<<(n + 255) / 256, 256, 0, st>>>(dst, src, n);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_closure_record(const PoseTable& tab, int n_queries, int K, int n_starts, float max_chi2_per_voxel, int min_voxels, const int32_t* d_best,
                                 const int32_t* d_cand, const unsigned long long* d_keys, const int32_t* d_shift_of, const float* d_x0, const float* d_out,
                                 const ::icet_score* d_score, ::icet_closure* d_closure, hipStream_t st) {
    k_closure_record<<<(n_queries + 63) / 64, 64, 0, st>>>(tab, n_queries, K, n_starts, max_chi2_per_voxel, min_voxels, d_best, d_cand, d_keys, d_shift_of, d_x0, d_out, d_score,
                                                          d_closure);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_closure_set_pose(const PoseTable& tab, const PoseUpload* h_up, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    k_closure_set_pose<<<(n + 255) / 256, 256, 0, st>>>(tab, h_up, n);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_closure_clear_pose(const PoseTable& tab, const StoreParkSlots& slots, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (n > kStoreParkMax) return hipErrorInvalidValue;
    k_closure_clear_pose<<<1, kStoreParkMax, 0, st>>>(tab, slots, n);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace icet
