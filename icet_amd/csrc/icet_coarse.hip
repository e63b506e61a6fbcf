// icet_amd/csrc/icet_coarse.hip -- coarse alignment for the keyframe store (include/icet_hip.h icet_keyframe_store_coarse_align_device).
// The rule -- cell, height code, spanning cells, hypotheses, score, winner, start pose -- is icet_coarse.h; this file is the kernels around it:
//     k_coarse_extrema     the per-cell smallest and largest height code of a batch of scans, with integer-maximum atomics into the scratch (two words per cell:
//                          q + 1 and 256 - q, so that both are maxima and 0 is "no point"); a cell's word is read first and the atomic only issued when it would move
//     k_coarse_finish      one thread per cell: the spanning cells to bits (a wave's ballot is two words of a row), into a slot's row of the table, a caller's buffer
//                          or the call's own query grids; the scratch back to zero for the next batch
//     k_coarse_hypotheses  one thread per (query, candidate, hypothesis): the float32 transform of the hypothesis
//     k_coarse_correlate   one block per (query, candidate, hypothesis): the live grid ORed into LDS from the scan's structure points, the slot's grid beside it,
//                          one shift per thread at a time -- rows walked with a funnel shift, AND and popcount per word --, the block's largest key into the
//                          candidate's key with a 64-bit integer maximum
//     k_coarse_resolve     one thread per (query, candidate): the winner decoded, its start pose and match record; the registrations of the one-call form
//     k_coarse_record      one thread per query: the winner's coarse score and shift into the closure record
// Maxima, ORs and sums of integers only: no float atomic, no dependence on the launch shape.  No kernel waits for another block.
#include <hip/hip_runtime.h>
#include "../../include/icet_hip.h"
#include "icet_internal.h"
#include "icet_coarse.h"
#include "icet_closure_device.h"

namespace icet {
namespace {

namespace rule = icet_coarse_rule;

constexpr int kStructBlock = 256;
constexpr int kCorrBlock = 512;
static_assert(sizeof(CoarseHyp) == 48, "m[6] | t[3] | pad");

// Grid (chunks, scans); block b of scan k takes the points [b * per_block, (b + 1) * per_block): three coalesced streams of 4 B per lane.
__global__ __launch_bounds__(kStructBlock) void k_coarse_extrema(AppScans sc, const int32_t* __restrict__ rows, rule::Consts c, uint32_t* scratch, int per_block) {
    const int k = blockIdx.y;
    int n = sc.n[k];
    if (rows) n = max(0, min(rows[k], n));
    const int lo = blockIdx.x * per_block;
    if (lo >= n) return;
    const int hi = min(n, lo + per_block);
    const size_t cells = (size_t)c.G * c.G;
    uint32_t* mx = scratch + (size_t)k * 2 * cells;
    uint32_t* mn = mx + cells;
    const float* x = sc.ptr[k]; const float* y = x + sc.ld[k]; const float* z = x + 2 * (size_t)sc.ld[k];
    for (int i = lo + threadIdx.x; i < hi; i += kStructBlock) {
        int ix, iy, q;
        if (!rule::count_point(c, x[i], y[i], z[i], ix, iy, q)) continue;
        const int cell = ix * c.G + iy;                               // ix, iy < G: inside the table
        const uint32_t up = (uint32_t)q + 1u, dn = 256u - (uint32_t)q;      // q = 0 .. 254
        if (mx[cell] < up) atomicMax(&mx[cell], up);
        if (mn[cell] < dn) atomicMax(&mn[cell], dn);
    }
}

// Grid (G G / 256, scans), one thread per cell.  Row sc.dst[k] of `out` (rows of G W words) gets the scan's spanning cells; has (may be null): the row's "has a
// grid" word.  A row outside 0 .. n_rows - 1 is not written (the host has checked the slots); the scratch is cleared all the same.
__global__ __launch_bounds__(kStructBlock) void k_coarse_finish(AppScans sc, rule::Consts c, uint32_t* scratch, uint32_t* __restrict__ out, int32_t* __restrict__ has, int n_rows) {
    const int k = blockIdx.y;
    const size_t cells = (size_t)c.G * c.G;
    uint32_t* mx = scratch + (size_t)k * 2 * cells;
    uint32_t* mn = mx + cells;
    const int cell = blockIdx.x * kStructBlock + threadIdx.x;         // G G is a multiple of 1024
    const uint32_t up = mx[cell], dn = mn[cell];
    if (up) { mx[cell] = 0u; mn[cell] = 0u; }
    const int row = sc.dst[k];
    if (row < 0 || row >= n_rows) return;                             // (the same for every thread of the block)
    const bool bit = up && rule::cell_spans(c, 256 - (int)dn, (int)up - 1);
    const unsigned long long m = __ballot(bit);
    uint32_t* o = out + (size_t)row * c.G * c.W + (cell >> 5);
    const int lane = threadIdx.x & 63;
    if (lane == 0) o[0] = (uint32_t)m;
    if (lane == 32) o[0] = (uint32_t)(m >> 32);
    if (has && cell == 0) has[row] = 1;
}

__global__ __launch_bounds__(64) void k_coarse_hypotheses(const int32_t* __restrict__ cand, const float* __restrict__ x0_base, int n_qk, int H, int Y, float yaw_step,
                                                          CoarseHyp* __restrict__ hyp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_qk * H) return;
    const int qk = i / H, h = i % H;
    if (cand[qk] < 0) return;
    float X0[6];
    for (int k = 0; k < 6; k++) X0[k] = x0_base[(size_t)qk * 6 + k];
    int y, f;
    rule::hypothesis_of(h, Y, y, f);
    double Rh[9];
    rule::hypothesis_rotation(X0, y, f, yaw_step, Rh);
    CoarseHyp o;
    rule::hypothesis_rows(Rh, o.m);
    o.t[0] = X0[0]; o.t[1] = X0[1]; o.t[2] = X0[2]; o.pad[0] = 0.f; o.pad[1] = 0.f; o.pad[2] = 0.f;
    hyp[i] = o;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint64_t u = __shfl_xor((unsigned long long)v, o, 64); v = u > v ? u : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// Grid (H, K, Q).  LDS: live G W words | buf G (W + 3) words.  buf first holds the scan's own grid (which of its points are structure points), then the slot's grid
// with one zero word in front of every row and two behind it, so that a shifted 64-bit window never leaves the row.  A thread's shift (a, b): live row i meets slot
// row i + a; with sb = b + 32 live word w meets bits sb & 31 .. of padded words w + (sb >> 5) and the next.  Threads of a wave that share `a` read the same words.
__global__ __launch_bounds__(kCorrBlock) void k_coarse_correlate(CoarseTable tab, AppScans sc, const int32_t* __restrict__ rows, rule::Consts c, const int32_t* __restrict__ cand,
                                                                const CoarseHyp* __restrict__ hyp, int K, int H, int Mw, const uint32_t* __restrict__ qgrid,
                                                                unsigned long long* __restrict__ keys, int32_t* __restrict__ live_bits, int32_t* __restrict__ key_bits) {
    extern __shared__ uint32_t sm[];
    __shared__ uint64_t red[kCorrBlock / 64];
    __shared__ uint32_t cnt[2];
    const int h = blockIdx.x, q = blockIdx.z;
    const int qk = q * K + blockIdx.y;
    const int slot = cand[qk];
    if (slot < 0 || slot >= tab.cap) return;                          // (the same for every thread of the block)
    if (!tab.has[slot]) return;
    const int G = c.G, W = c.W, Ws = W + 3, words = G * W;
    uint32_t* live = sm;
    uint32_t* buf = sm + words;
    const uint32_t* own = qgrid + (size_t)q * words;
    for (int i = threadIdx.x; i < words; i += kCorrBlock) { buf[i] = own[i]; live[i] = 0u; }
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
    const CoarseHyp hy = hyp[(size_t)qk * H + h];
    __syncthreads();
    int n = sc.n[q];
    if (rows) n = max(0, min(rows[q], n));
    const float* x = sc.ptr[q]; const float* y = x + sc.ld[q]; const float* z = x + 2 * (size_t)sc.ld[q];
    for (int i = threadIdx.x; i < n; i += kCorrBlock) {
        const float px = x[i], py = y[i], pz = z[i];
        int ix, iy, code;
        if (!rule::count_point(c, px, py, pz, ix, iy, code)) continue;
        if (!((buf[ix * W + (iy >> 5)] >> (iy & 31)) & 1u)) continue;
        float xo, yo;
        rule::transform_xy(hy.m, hy.t, px, py, pz, xo, yo);
        int jx, jy;
        if (!rule::coord_cell(c, xo, jx) || !rule::coord_cell(c, yo, jy)) continue;
        atomicOr(&live[jx * W + (jy >> 5)], 1u << (jy & 31));         // jx, jy < G: inside the grid
    }
    __syncthreads();
    const uint32_t* kg = tab.grid + (size_t)slot * words;
    uint32_t kb = 0u, lb = 0u;
    for (int i = threadIdx.x; i < G * Ws; i += kCorrBlock) {
        const int r = i / Ws, w = i % Ws - 1;
        const uint32_t v = (w >= 0 && w < W) ? kg[r * W + w] : 0u;
        buf[i] = v;
        kb += (uint32_t)__popc(v);
    }
    for (int i = threadIdx.x; i < words; i += kCorrBlock) lb += (uint32_t)__popc(live[i]);
    lb = wave_sum_u32(lb); kb = wave_sum_u32(kb);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&cnt[0], lb); atomicAdd(&cnt[1], kb); }
    __syncthreads();
    const int side = 2 * Mw + 1, n_shifts = side * side;
    uint64_t best = 0;
    for (int t = threadIdx.x; t < n_shifts; t += kCorrBlock) {
        const int a = t / side - Mw, b = t % side - Mw;
        const int sb = b + rule::kMaxWindow;                          // 0 .. 64
        const int wo = sb >> 5;
        const uint32_t sh = (uint32_t)(sb & 31);
        uint32_t S = 0u;
        for (int i = 0; i < G; i++) {
            if ((unsigned)(i + a) >= (unsigned)G) continue;           // the row is shifted off the grid
            const uint32_t* lr = live + i * W;
            const uint32_t* kr = buf + (i + a) * Ws + wo;
            uint32_t lo = kr[0];
            for (int w = 0; w < W; w++) {
                const uint32_t hi = kr[w + 1];
                S += (uint32_t)__popc(lr[w] & __builtin_amdgcn_alignbit(hi, lo, sh));
                lo = hi;
            }
        }
        const uint64_t key = rule::shift_key(S, a, b, h);
        best = key > best ? key : best;
    }
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t m = red[0];
        for (int w = 1; w < kCorrBlock / 64; w++) m = red[w] > m ? red[w] : m;
        atomicMax(&keys[qk], (unsigned long long)m);
        live_bits[(size_t)qk * H + h] = (int32_t)cnt[0];
        if (h == 0) key_bits[qk] = (int32_t)cnt[1];
    }
}

// One thread per (query, candidate).  x0_out / match may each be null.  With n_starts > 0 the registrations r = (q K + k) S + s as k_closure_resolve writes them,
// from fl(X0_coarse + off[s]).
__global__ __launch_bounds__(64) void k_coarse_resolve(rule::Consts c, AppOffsets off, int n_queries, int K, int H, int Y, float yaw_step, int min_score, int n_starts,
                                                       int any_slot, const int32_t* __restrict__ cand, const float* __restrict__ x0_base,
                                                       const unsigned long long* __restrict__ keys, const int32_t* __restrict__ live_bits,
                                                       const int32_t* __restrict__ key_bits, float* __restrict__ x0_out, icet_coarse_match* __restrict__ match,
                                                       float* __restrict__ x0, int32_t* __restrict__ kf_of, int32_t* __restrict__ rows, int32_t* __restrict__ members,
                                                       int32_t* __restrict__ offs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    write_group_offset(i, n_queries, K, n_starts, offs);
    if (i >= n_queries * K) return;
    const int slot = cand[i];
    float X[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    icet_coarse_match m;
    m.score = 0; m.a = 0; m.b = 0; m.h = 0; m.live_bits = 0; m.key_bits = 0; m.found = 0; m.reserved = 0;
    if (slot >= 0) {
        float X0[6];
        for (int k = 0; k < 6; k++) { X0[k] = x0_base[(size_t)i * 6 + k]; X[k] = X0[k]; }
        const uint64_t key = keys[i];
        if (key != 0) {                                               // the slot has a grid
            uint32_t score; int a, b, h;
            rule::key_decode(key, score, a, b, h);
            m.score = (int32_t)score; m.a = a; m.b = b; m.h = h; m.live_bits = live_bits[(size_t)i * H + h]; m.key_bits = key_bits[i];
            if ((int64_t)score >= (int64_t)min_score) {
                m.found = 1;
                int y, f;
                rule::hypothesis_of(h, Y, y, f);
                double Rh[9];
                rule::hypothesis_rotation(X0, y, f, yaw_step, Rh);
                rule::start_pose(c, X0, Rh, a, b, y, f, X);
            }
        }
    }
    if (x0_out) for (int k = 0; k < 6; k++) x0_out[(size_t)i * 6 + k] = X[k];
    if (match) match[i] = m;
    write_registrations(i, slot, any_slot, X, off.off, n_starts, x0, kf_of, rows, members);
}

__global__ __launch_bounds__(64) void k_coarse_record(int n_queries, int n_starts, const icet_coarse_match* __restrict__ match, icet_closure* __restrict__ rec) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries) return;
    const int r = rec[q].reg;
    if (r < 0) return;
    const icet_coarse_match m = match[r / n_starts];
    rec[q].reserved1[0] = m.score;
    rec[q].reserved1[1] = rule::shift_code(m.a, m.b, m.h);
}

}  // namespace

static size_t corr_lds(const rule::Consts& c) { return sizeof(uint32_t) * ((size_t)c.G * c.W + (size_t)c.G * (c.W + 3)); }

hipError_t launch_coarse_prepare(const icet_coarse_rule::Consts& c) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_coarse_correlate), hipFuncAttributeMaxDynamicSharedMemorySize, (int)corr_lds(c));
}

hipError_t launch_coarse_structure(const AppScans& sc, int n_scans, const int32_t* d_rows, const icet_coarse_rule::Consts& c, uint32_t* d_scratch, uint32_t* d_out,
                                   int32_t* d_has, int n_rows, hipStream_t st) {
    if (n_scans <= 0) return hipSuccess;
    if (n_scans > kCoarseBatch) return hipErrorInvalidValue;
    int max_n = 0;
    for (int k = 0; k < n_scans; k++) max_n = sc.n[k] > max_n ? sc.n[k] : max_n;
    if (max_n > 0) {
        // 4096 points per block (16 per thread), at most 256 blocks per scan
        int chunks = (max_n + 4095) / 4096;
        if (chunks > 256) chunks = 256;
        int per_block = (max_n + chunks - 1) / chunks;
        per_block = (per_block + kStructBlock - 1) / kStructBlock * kStructBlock;
        k_coarse_extrema<<<dim3(chunks, n_scans), kStructBlock, 0, st>>>(sc, d_rows, c, d_scratch, per_block);
        ICET_LAUNCH_CHECK();
    }
    k_coarse_finish<<<dim3(c.G * c.G / kStructBlock, n_scans), kStructBlock, 0, st>>>(sc, c, d_scratch, d_out, d_has, n_rows);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_coarse_align(const CoarseTable& tab, const AppScans& sc, const int32_t* d_rows, const icet_coarse_rule::Consts& c, const CoarseSearch& se,
                               const AppOffsets& off, int n_queries, int K, int n_starts, int any_slot, const int32_t* d_cand, const float* d_x0_base,
                               const uint32_t* d_qgrid, CoarseHyp* d_hyp, unsigned long long* d_keys, int32_t* d_live_bits, int32_t* d_key_bits, float* d_x0_out,
                               ::icet_coarse_match* d_match, float* d_x0, int32_t* d_kf_of, int32_t* d_rows_out, int32_t* d_members, int32_t* d_offs, hipStream_t st) {
    if (n_queries > kAppBatch || se.window > rule::kMaxWindow || se.Y > rule::kMaxYaw) return hipErrorInvalidValue;
    const int H = rule::n_hypotheses(se.Y, se.half_turn), n_qk = n_queries * K;
    hipError_t e = hipMemsetAsync(d_keys, 0, sizeof(unsigned long long) * (size_t)n_qk, st);
    if (e != hipSuccess) return e;
    k_coarse_hypotheses<<<(n_qk * H + 63) / 64, 64, 0, st>>>(d_cand, d_x0_base, n_qk, H, se.Y, se.yaw_step, d_hyp);
    ICET_LAUNCH_CHECK();
    k_coarse_correlate<<<dim3(H, K, n_queries), kCorrBlock, corr_lds(c), st>>>(tab, sc, d_rows, c, d_cand, d_hyp, K, H, se.window, d_qgrid, d_keys, d_live_bits, d_key_bits);
    ICET_LAUNCH_CHECK();
    const int n = n_qk > n_queries + 1 ? n_qk : n_queries + 1;
    k_coarse_resolve<<<(n + 63) / 64, 64, 0, st>>>(c, off, n_queries, K, H, se.Y, se.yaw_step, se.min_score, n_starts, any_slot, d_cand, d_x0_base, d_keys, d_live_bits,
                                                  d_key_bits, d_x0_out, d_match, d_x0, d_kf_of, d_rows_out, d_members, d_offs);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_coarse_record(int n_queries, int n_starts, const ::icet_coarse_match* d_match, ::icet_closure* d_closure, hipStream_t st) {
    k_coarse_record<<<(n_queries + 63) / 64, 64, 0, st>>>(n_queries, n_starts, d_match, d_closure);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace icet
