// icet_amd/csrc/icet_score.hip -- the registration score (include/icet_hip.h icet_score) and the best-of-group selection:
//     k_gn_score        behind one more point pass at the registration's transform record: per slot the moments, R_noise, dz = M (mu2 - mu1) and
//                       W = pinv(M R_noise M^T) of gn_solve_body, then chi2 = sum dz^T W dz, voxels and points in; one block per registration
//     k_select_best     one wave per group of registrations: the lowest chi2 per voxel among those with at least half the group's best voxel count
//     k_point_sums_dump, k_point_sums_copy, k_fix_debug   test hooks: the point pass's raw per-voxel accumulator records, and its float -> fixed-point conversions on their own
// The loop's own kernels are untouched: this file has a body of its own, written after gn_solve_body's per-voxel front statement by statement.
#include <hip/hip_runtime.h>
#include <math.h>
#include <float.h>
#include "../../include/icet_hip.h"
#include "icet_internal.h"
#include "icet_device_common.h"
#include "icet_device_math.h"
#include "icet_solve_body.h"

namespace icet {
namespace {

static_assert(sizeof(icet_score) == 32, "icet_score is a 32-byte ABI struct");
constexpr int kScoreBlock = 256;

// Registration `pair` (one block) against keyframe row kf_of[pair].  `iter`: the iteration index the moving-voxel gate of ICET_FLAG_REJECT_MOVING is
// evaluated at (the caller's runlen: the iteration the loop would run next).  Leaves every slot's accumulator and the overflow count at zero, as a solve does.
template <bool kRefW>
__global__ __launch_bounds__(kScoreBlock) void k_gn_score(const int32_t* __restrict__ n_slots, const SlotFit* __restrict__ fitS, uint32_t* acc,
                                                          const float* __restrict__ xf_all, int V, int n, int iter, NearOverflow over, int reject_moving,
                                                          const int32_t* __restrict__ kf_of, icet_score* __restrict__ score) {
    // the expressions of gn_solve_body, unfused like there: a voxel's dz and W carry the bits the solve would compute at this transform
#pragma clang fp contract(off)
    const int pair = blockIdx.x;
    const int kf = kf_of ? __builtin_amdgcn_readfirstlane(kf_of[pair]) : pair;
    const uint32_t nov = over.count[pair];                              // block-uniform
    const int ns = n_slots[kf];
    if (nov) {                                                          // undecided points of the point pass: classified here, before any sum is read
        NearOverflow o = over;
        o.slot_of_voxel += ((ptrdiff_t)kf - pair) * ((V + 1) & ~1); o.hotS += ((ptrdiff_t)kf - pair) * V;
        drain_near_overflow(o, pair, V, xf_all + pair * kXf, acc + (size_t)pair * V * kAccWords, nov);
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) over.count[pair] = 0u;
    }
    double chi = 0.0;
    int vox = 0, pin = 0;
    for (int s = threadIdx.x; s < ns; s += kScoreBlock) {               // slot s always on thread s % 256: a registration's sums do not depend on the call
        uint32_t* A = acc + ((size_t)pair * V + s) * kAccWords;
        uint32_t aw[kAccWords];
        {
            const uint4* q = reinterpret_cast<const uint4*>(A);
            uint4 r[5];
#pragma unroll
            for (int k = 0; k < 5; k++) r[k] = q[k];
            __builtin_memcpy(aw, r, sizeof(aw));
            uint4* z = reinterpret_cast<uint4*>(A);
#pragma unroll
            for (int k = 0; k < 5; k++) z[k] = make_uint4(0u, 0u, 0u, 0u);
        }
        const SlotFit f = fitS[(size_t)kf * V + s];
        const uint32_t n2 = aw[0], m = aw[1];
        if (!((int)n2 > n && (int)m > n)) continue;
        long long AF[9];
        __builtin_memcpy(AF, aw + 2, sizeof(AF));
        double sdD[3], sddD[6];
#pragma unroll
        for (int k = 0; k < 3; k++) sdD[k] = (double)AF[k] * kFixInv;
#pragma unroll
        for (int k = 0; k < 6; k++) sddD[k] = (double)AF[3 + k] * kFixInv;
        const double fmD = (double)m, rfmD = 1.0 / fmD;
        const double dbD[3] = {sdD[0] * rfmD, sdD[1] * rfmD, sdD[2] * rfmD};
        const float db[3] = {(float)dbD[0], (float)dbD[1], (float)dbD[2]};
        const double denD = 1.0 / (double)(m - 1);
        const float d2 = (float)(n2 - 1);
        float cov2[6];
        cov2[0] = (float)((sddD[0] - fmD * dbD[0] * dbD[0]) * denD); cov2[1] = (float)((sddD[1] - fmD * dbD[0] * dbD[1]) * denD);
        cov2[2] = (float)((sddD[2] - fmD * dbD[0] * dbD[2]) * denD); cov2[3] = (float)((sddD[3] - fmD * dbD[1] * dbD[1]) * denD);
        cov2[4] = (float)((sddD[4] - fmD * dbD[1] * dbD[2]) * denD); cov2[5] = (float)((sddD[5] - fmD * dbD[2] * dbD[2]) * denD);
        float Rn[6];
#pragma unroll
        for (int k = 0; k < 6; k++) Rn[k] = f.s1n[k] + cov2[k] / d2;
        const float* M = f.M;
        float dz[3];
#pragma unroll
        for (int i = 0; i < 3; i++) dz[i] = M[3 * i] * db[0] + M[3 * i + 1] * db[1] + M[3 * i + 2] * db[2];
        if (reject_moving && iter >= kRejectMovingStartIter &&
            (fabsf(dz[0]) > kRejectMovingThresh || fabsf(dz[1]) > kRejectMovingThresh || fabsf(dz[2]) > kRejectMovingThresh)) continue;
        float MR[9];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            MR[3 * i + 0] = M[3 * i] * Rn[0] + M[3 * i + 1] * Rn[1] + M[3 * i + 2] * Rn[2];
            MR[3 * i + 1] = M[3 * i] * Rn[1] + M[3 * i + 1] * Rn[3] + M[3 * i + 2] * Rn[4];
            MR[3 * i + 2] = M[3 * i] * Rn[2] + M[3 * i + 1] * Rn[4] + M[3 * i + 2] * Rn[5];
        }
        float W9[9];
        if constexpr (kRefW) {
            float Rp9[9];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) Rp9[3 * i + j] = MR[3 * i] * M[3 * j] + MR[3 * i + 1] * M[3 * j + 1] + MR[3 * i + 2] * M[3 * j + 2];
            icetdev::cod_pinv3_lane(Rp9, W9);
        } else {
            float Rp[6], W[6];
            Rp[0] = MR[0] * M[0] + MR[1] * M[1] + MR[2] * M[2];
            Rp[1] = MR[0] * M[3] + MR[1] * M[4] + MR[2] * M[5];
            Rp[2] = MR[0] * M[6] + MR[1] * M[7] + MR[2] * M[8];
            Rp[3] = MR[3] * M[3] + MR[4] * M[4] + MR[5] * M[5];
            Rp[4] = MR[3] * M[6] + MR[4] * M[7] + MR[5] * M[8];
            Rp[5] = MR[6] * M[6] + MR[7] * M[7] + MR[8] * M[8];
            icetdev::pinv3_sym_fast(Rp, 3.0f * FLT_EPSILON, W);
            W9[0] = W[0]; W9[1] = W[1]; W9[2] = W[2]; W9[3] = W[1]; W9[4] = W[3]; W9[5] = W[4]; W9[6] = W[2]; W9[7] = W[4]; W9[8] = W[5];
        }
        // dz^T W dz in double: the voxel's term and the registration's sum carry no cancellation of their own
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) q += (double)dz[i] * (double)W9[3 * i + j] * (double)dz[j];
        chi += q; vox += 1; pin += (int)m;
    }
    // fixed order: DPP totals of the waves, then the waves in index order
    __shared__ double s_chi[kScoreBlock / 64];
    __shared__ int s_vox[kScoreBlock / 64], s_pin[kScoreBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double wc = wave_total(chi);
    const int wvx = wave_total(vox), wpn = wave_total(pin);
    if (lane == 0) { s_chi[wave] = wc; s_vox[wave] = wvx; s_pin[wave] = wpn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0; int v = 0, pi = 0;
        for (int w = 0; w < kScoreBlock / 64; w++) { c += s_chi[w]; v += s_vox[w]; pi += s_pin[w]; }
        const int points = over.desc[pair].n2;
        icet_score r;
        r.chi2 = (float)c;
        r.chi2_per_voxel = v > 0 ? (float)(c / (double)v) : __builtin_inff();
        r.voxels = v; r.points_in = pi; r.points = points;
        r.overlap = points > 0 ? (float)((double)pi / (double)points) : 0.f;
        r.reserved[0] = 0; r.reserved[1] = 0;
        score[pair] = r;
    }
}

// Test hook (icet_debug_point_sums_device): what the point pass left for registration `pair` (one block), copied out raw.  The near-overflow list is drained
// first, exactly as k_gn_score does; then every voxel's 80-byte accumulator record -- n2, m, nine 64-bit fixed-point sums -- goes to dump[pair][voxel] (zeros
// for a voxel without a slot) and the record and the overflow count are left at zero, as a solve leaves them.
__global__ __launch_bounds__(kScoreBlock) void k_point_sums_dump(uint32_t* acc, const float* __restrict__ xf_all, int V, NearOverflow over,
                                                                 const int32_t* __restrict__ kf_of, uint32_t* __restrict__ dump) {
    const int pair = blockIdx.x;
    const int kf = kf_of ? __builtin_amdgcn_readfirstlane(kf_of[pair]) : pair;
    const uint32_t nov = over.count[pair];                              // block-uniform
    if (nov) {
        NearOverflow o = over;
        o.slot_of_voxel += ((ptrdiff_t)kf - pair) * ((V + 1) & ~1); o.hotS += ((ptrdiff_t)kf - pair) * V;
        drain_near_overflow(o, pair, V, xf_all + pair * kXf, acc + (size_t)pair * V * kAccWords, nov);
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) over.count[pair] = 0u;
    }
    const int16_t* map = over.slot_of_voxel + (size_t)kf * ((V + 1) & ~1);
    for (int v = threadIdx.x; v < V; v += kScoreBlock) {
        const int s = map[v];
        uint4* out = reinterpret_cast<uint4*>(dump + ((size_t)pair * V + v) * kAccWords);
        uint4* A = reinterpret_cast<uint4*>(acc + ((size_t)pair * V + (s >= 0 ? s : 0)) * kAccWords);
#pragma unroll
        for (int k = 0; k < 5; k++) {
            uint4 r = make_uint4(0u, 0u, 0u, 0u);
            if (s >= 0) { r = A[k]; A[k] = make_uint4(0u, 0u, 0u, 0u); }
            out[k] = r;
        }
    }
}

// Test hook (icet_debug_gn_terms_device): k_point_sums_dump that leaves every record where it is -- the solve launched behind it consumes (and clears) exactly what
// was copied out.  The overflow list is drained here and its count reset, so that solve finds the list empty and the sums complete.
__global__ __launch_bounds__(kScoreBlock) void k_point_sums_copy(uint32_t* acc, const float* __restrict__ xf_all, int V, NearOverflow over,
                                                                 const int32_t* __restrict__ kf_of, uint32_t* __restrict__ dump) {
    const int pair = blockIdx.x;
    const int kf = kf_of ? __builtin_amdgcn_readfirstlane(kf_of[pair]) : pair;
    const uint32_t nov = over.count[pair];                              // block-uniform
    if (nov) {
        NearOverflow o = over;
        o.slot_of_voxel += ((ptrdiff_t)kf - pair) * ((V + 1) & ~1); o.hotS += ((ptrdiff_t)kf - pair) * V;
        drain_near_overflow(o, pair, V, xf_all + pair * kXf, acc + (size_t)pair * V * kAccWords, nov);
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) over.count[pair] = 0u;
    }
    const int16_t* map = over.slot_of_voxel + (size_t)kf * ((V + 1) & ~1);
    for (int v = threadIdx.x; v < V; v += kScoreBlock) {
        const int s = map[v];
        uint4* out = reinterpret_cast<uint4*>(dump + ((size_t)pair * V + v) * kAccWords);
        const uint4* A = reinterpret_cast<const uint4*>(acc + ((size_t)pair * V + (s >= 0 ? s : 0)) * kAccWords);
#pragma unroll
        for (int k = 0; k < 5; k++) out[k] = s >= 0 ? A[k] : make_uint4(0u, 0u, 0u, 0u);
    }
}

// Test hook (icet_debug_fix): n floats through the three float -> fixed-point conversions of the point pass; out[3 i ..] = to_fix_biased, to_fix_wide_biased, to_fix.
__global__ __launch_bounds__(kScoreBlock) void k_fix_debug(const float* __restrict__ v, unsigned long long* __restrict__ out, int n) {
    const int i = blockIdx.x * kScoreBlock + threadIdx.x;
    if (i >= n) return;
    const float x = v[i];
    out[3 * (size_t)i + 0] = to_fix_biased(x); out[3 * (size_t)i + 1] = to_fix_wide_biased(x); out[3 * (size_t)i + 2] = to_fix(x);
}

// (chi2 per voxel, registration) orders the candidates: lower chi2 per voxel first, ties to the lower index; NaN ranks behind every number.
// r == INT32_MAX: no candidate yet.
__device__ __forceinline__ bool better(float c, int r, float cb, int rb) {
    return rb == INT32_MAX || (r != INT32_MAX && (c < cb || (c == cb && r < rb)));
}

// One wave per group.  members[offs[g] .. offs[g + 1]): the group's registrations in ascending order.
__global__ __launch_bounds__(64) void k_select_best(const int32_t* __restrict__ members, const int32_t* __restrict__ offs, const icet_score* __restrict__ score,
                                                    const float* __restrict__ out, int32_t* __restrict__ best, float* __restrict__ best_out) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int lo = offs[g], hi = offs[g + 1];
    int vmax = 0;
    for (int i = lo + lane; i < hi; i += 64) vmax = max(vmax, score[members[i]].voxels);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) vmax = max(vmax, __shfl_xor(vmax, o, 64));
    const int need = max(1, (vmax + 1) / 2);                            // ceil(voxels_max / 2), at least one voxel
    float cb = 0.f; int rb = INT32_MAX;
    for (int i = lo + lane; i < hi; i += 64) {
        const int r = members[i];
        const icet_score s = score[r];
        if (s.voxels < need) continue;
        const float c = isnan(s.chi2_per_voxel) ? __builtin_inff() : s.chi2_per_voxel;
        if (better(c, r, cb, rb)) { cb = c; rb = r; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float c = __shfl_xor(cb, o, 64); const int r = __shfl_xor(rb, o, 64);
        if (better(c, r, cb, rb)) { cb = c; rb = r; }
    }
    const int r = rb == INT32_MAX ? -1 : rb;
    if (lane == 0) best[g] = r;
    if (best_out && lane < 48) best_out[(size_t)g * 48 + lane] = r >= 0 ? out[(size_t)r * 48 + lane] : 0.f;
}

}  // namespace


hipError_t launch_gn_score(const Workspace& w, const LaunchCfg& c, int iter, icet_score* d_score, hipStream_t st) {
    const NearOverflow over{w.desc, w.slot_of_voxel, w.hotS, w.thr, w.near_over, w.near_over_count, c.T, c.P, c.rt2};
    if (c.ref_w) k_gn_score<true><<<c.n_pairs, kScoreBlock, 0, st>>>(w.n_slots, w.fitS, w.acc, w.xf, c.V, c.n, iter, over, c.reject_moving, c.kf_of, d_score);
    else k_gn_score<false><<<c.n_pairs, kScoreBlock, 0, st>>>(w.n_slots, w.fitS, w.acc, w.xf, c.V, c.n, iter, over, c.reject_moving, c.kf_of, d_score);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_point_sums_dump(const Workspace& w, const LaunchCfg& c, uint32_t* d_dump, hipStream_t st) {
    const NearOverflow over{w.desc, w.slot_of_voxel, w.hotS, w.thr, w.near_over, w.near_over_count, c.T, c.P, c.rt2};
    k_point_sums_dump<<<c.n_pairs, kScoreBlock, 0, st>>>(w.acc, w.xf, c.V, over, c.kf_of, d_dump);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_point_sums_copy(const Workspace& w, const LaunchCfg& c, uint32_t* d_dump, hipStream_t st) {
    const NearOverflow over{w.desc, w.slot_of_voxel, w.hotS, w.thr, w.near_over, w.near_over_count, c.T, c.P, c.rt2};
    k_point_sums_copy<<<c.n_pairs, kScoreBlock, 0, st>>>(w.acc, w.xf, c.V, over, c.kf_of, d_dump);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_fix_debug(const float* d_v, unsigned long long* d_out, int n, hipStream_t st) {
    k_fix_debug<<<(n + kScoreBlock - 1) / kScoreBlock, kScoreBlock, 0, st>>>(d_v, d_out, n);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_select_best(const int32_t* d_members, const int32_t* d_offs, int n_groups, const icet_score* d_score, const float* d_out,
                              int32_t* d_best, float* d_best_out, hipStream_t st) {
    if (n_groups <= 0) return hipSuccess;
    k_select_best<<<n_groups, 64, 0, st>>>(d_members, d_offs, d_score, d_out, d_best, d_best_out);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace icet
