// icet_amd/csrc/icet_appearance.hip -- place recognition by appearance for the keyframe store (include/icet_hip.h icet_keyframe_store_close_appearance_device;
// DESIGN.md section 17).  The rule -- cell, height code, weight, distance, eligibility, start pose -- is icet_appearance.h; this file is the kernels around it:
//     k_app_build          the cells of a batch of scans: a block takes a run of one scan's points, keeps the maxima of its cells in LDS and flushes the cells it
//                          touched into the scan's table of the scratch with integer-maximum atomics
//     k_app_finish         one block per scan: the scratch table to bytes (row-major for a caller, ring-packed columns for the store), the column weights, and the
//                          scratch back to zero for the next batch
//     k_app_set_stamp      stamps without poses
//     k_app_match          one block per slot: every shift's distance to each query, one lane per shift walking the columns in ascending order; the slot's key
//     k_app_select_tiles / k_app_select_merge   the K smallest keys of each query: tiles of 1024 slots, then one block per query (the rounds of icet_closure.hip)
//     k_app_resolve        one thread per (query, candidate): distance, shift, start poses, keyframe index and row count of its registrations
//     k_app_record         one thread per query: the winner's row, score, X0, distance and shift, and the acceptance gate
// Maxima and minima of integers only: no float atomic, no dependence on the launch shape.  No kernel waits for another block.
#include <hip/hip_runtime.h>
#include "../../include/icet_hip.h"
#include "icet_internal.h"
#include "icet_appearance.h"

namespace icet {
namespace {

using icet_closure_rule::kNoKey;
namespace rule = icet_appearance_rule;

constexpr int kBuildBlock = 256;
constexpr int kSelectBlock = 256;
constexpr int kMergeRegs = 16;                      // keys per thread the merge keeps in registers (icet_closure.hip)
static_assert(kClosureTile % kSelectBlock == 0 && kSelectBlock == 256, "four waves per block, whole keys per lane");

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint64_t u = __shfl_xor((unsigned long long)v, o, 64); v = u < v ? u : v; }
    return v;
}

// Grid (chunks, scans).  Block b of scan k takes the points [b * per_block, (b + 1) * per_block) of the scan: x, y and z are three coalesced streams of 4 B per
// lane (the leading dimension of a scan is any number of floats, so the columns are not 16-byte aligned in general).  kLds: the table of the block fits the LDS
// budget; otherwise (rings x sectors above 12288) the points go to the scratch directly.
template <bool kLds>
__global__ __launch_bounds__(kBuildBlock) void k_app_build(AppScans sc, const int32_t* __restrict__ rows, rule::Consts c, uint32_t* __restrict__ scratch, int per_block) {
    extern __shared__ uint32_t tab[];
    const int k = blockIdx.y;
    int n = sc.n[k];
    if (rows) n = max(0, min(rows[k], n));
    const int lo = blockIdx.x * per_block;
    if (lo >= n) return;                                              // (the same for every thread of the block)
    const int hi = min(n, lo + per_block);
    const int cells = c.A * c.Rn;
    uint32_t* out = scratch + (size_t)k * cells;
    if (kLds) {
        for (int i = threadIdx.x; i < cells; i += kBuildBlock) tab[i] = 0u;
        __syncthreads();
    }
    const float* x = sc.ptr[k]; const float* y = x + sc.ld[k]; const float* z = x + 2 * (size_t)sc.ld[k];
    for (int i = lo + threadIdx.x; i < hi; i += kBuildBlock) {
        int ring, sector, q;
        if (!rule::cell_of(c, x[i], y[i], z[i], ring, sector, q)) continue;
        const int cell = ring * c.A + sector;                         // ring < Rn, sector < A: inside the table
        if (kLds) atomicMax(&tab[cell], (uint32_t)q); else atomicMax(&out[cell], (uint32_t)q);
    }
    if (kLds) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += kBuildBlock) { const uint32_t v = tab[i]; if (v) atomicMax(&out[i], v); }
    }
}

// One block per scan, one thread per column.  packed: the store's layout -- column j is Rp words, byte r & 3 of word r >> 2 is ring r -- into row dst[k] of the
// table, and the row's "has a descriptor" word; otherwise D[ring][sector] bytes and A weights into row k of the caller's buffers.
__global__ __launch_bounds__(kBuildBlock) void k_app_finish(AppScans sc, rule::Consts c, uint32_t* __restrict__ scratch, bool packed, AppTable tab,
                                                            uint8_t* __restrict__ d_desc, float* __restrict__ d_weight) {
    const int k = blockIdx.x;
    const int cells = c.A * c.Rn;
    uint32_t* in = scratch + (size_t)k * cells;
    const int row = packed ? sc.dst[k] : k;
    if (packed && (row < 0 || row >= tab.cap)) {                      // (the host has checked the slots; the scratch is cleared all the same)
        for (int i = threadIdx.x; i < cells; i += kBuildBlock) in[i] = 0u;
        return;
    }
    for (int j = threadIdx.x; j < c.A; j += kBuildBlock) {
        uint32_t energy = 0u, word = 0u;
        for (int r = 0; r < c.Rn; r++) {
            const uint32_t v = in[r * c.A + j];
            in[r * c.A + j] = 0u;
            energy += v * v;
            if (packed) {
                word |= v << (8 * (r & 3));
                if ((r & 3) == 3 || r == c.Rn - 1) { tab.desc[((size_t)row * c.A + j) * tab.Rp + (r >> 2)] = word; word = 0u; }
            } else d_desc[(size_t)k * cells + r * c.A + j] = (uint8_t)v;
        }
        const float w = rule::column_weight(energy);
        if (packed) tab.w[(size_t)row * c.A + j] = w; else d_weight[(size_t)k * c.A + j] = w;
    }
    if (packed && threadIdx.x == 0) tab.has[row] = 1;
}

__global__ void k_app_set_stamp(PoseTable tab, AppStamps st, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int slot = st.slot[i];
    if (slot < 0 || slot >= tab.cap) return;
    tab.stamp[slot] = st.stamp[i];
}

// One block of roundup64(A) threads per slot; the slot's columns stay in LDS (stride Rp | 1 words: lane s reads column j + s, and an odd stride keeps the lanes on
// different banks) while the queries pass through one after the other.  Thread s walks j = 0 .. A - 1: the integer product of column j of the query and column
// j + s of the slot, four rings per packed dot instruction, the two float products, and the double sum in ascending j.  A column that is empty on either side
// has G = 0 and a zero weight: its term is +0, which leaves the sum as it is, so it is added like the others and only not counted.
__global__ __launch_bounds__(384) void k_app_match(AppTable tab, const uint32_t* __restrict__ qdesc, const float* __restrict__ qw, int n_queries,
                                                   const int64_t* __restrict__ slot_stamp, AppQueryStamps qs, float max_distance, int64_t min_gap,
                                                   unsigned long long* __restrict__ keys_all, uint16_t* __restrict__ shift_all) {
    extern __shared__ uint32_t sm[];
    __shared__ uint64_t red[6];
    const int slot = blockIdx.x, A = tab.A, Rp = tab.Rp, Rs = Rp | 1;
    if (!tab.has[slot]) {                                             // (the same for every thread of the block)
        for (int q = threadIdx.x; q < n_queries; q += blockDim.x) keys_all[(size_t)q * tab.cap + slot] = kNoKey;
        return;
    }
    uint32_t* cq = sm;                                                // A x Rp
    uint32_t* cc = cq + A * Rp;                                       // A x Rs
    float* wq = reinterpret_cast<float*>(cc + A * Rs);                // A
    float* wc = wq + A;                                               // A
    for (int i = threadIdx.x; i < A * Rp; i += blockDim.x) cc[(i / Rp) * Rs + i % Rp] = tab.desc[(size_t)slot * A * Rp + i];
    for (int i = threadIdx.x; i < A; i += blockDim.x) wc[i] = tab.w[(size_t)slot * A + i];
    const int64_t stamp = slot_stamp[slot];
    const int s = threadIdx.x;
    for (int q = 0; q < n_queries; q++) {
        __syncthreads();                                              // the previous query has been read
        for (int i = threadIdx.x; i < A * Rp; i += blockDim.x) cq[i] = qdesc[(size_t)q * A * Rp + i];
        for (int i = threadIdx.x; i < A; i += blockDim.x) wq[i] = qw[(size_t)q * A + i];
        __syncthreads();
        uint64_t key = kNoKey;
        if (s < A) {
            double sum = 0.0; int m = 0;
            int jj = s;
            for (int j = 0; j < A; j++) {
                uint32_t G = 0u;
                for (int w = 0; w < Rp; w++) G = __builtin_amdgcn_udot4(cq[j * Rp + w], cc[jj * Rs + w], G, false);
                const float a = wq[j], b = wc[jj];
                sum += (double)rule::column_term(G, a, b);
                m += (a > 0.f && b > 0.f) ? 1 : 0;
                jj = jj + 1 == A ? 0 : jj + 1;
            }
            key = rule::shift_key(rule::shift_distance(sum, m, A), s);
        }
        key = wave_min_u64(key);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t best = red[0];
            for (int w = 1; w < (int)(blockDim.x >> 6); w++) best = red[w] < best ? red[w] : best;
            const float d = icet_closure_rule::key_d2(best);
            keys_all[(size_t)q * tab.cap + slot] = rule::candidate_key(d, max_distance, qs.stamp[q], stamp, min_gap, slot);
            shift_all[(size_t)q * tab.cap + slot] = (uint16_t)(uint32_t)best;
        }
    }
}

// Pass 1 of the selection (k_closure_search_tiles without the distance): part[(q * gridDim.x + block) * K + k] is the block's k-th smallest key of query q.
__global__ __launch_bounds__(kSelectBlock) void k_app_select_tiles(const unsigned long long* __restrict__ keys_all, int cap, int n_queries, int K,
                                                                   unsigned long long* __restrict__ part) {
    const int base = blockIdx.x * kClosureTile;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int kPerLane = kClosureTile / 64;
    for (int q = wave; q < n_queries; q += kSelectBlock / 64) {
        uint64_t key[kPerLane];
#pragma unroll
        for (int i = 0; i < kPerLane; i++) {
            const int slot = base + lane + 64 * i;
            key[i] = slot < cap ? keys_all[(size_t)q * cap + slot] : kNoKey;
        }
        unsigned long long* out = part + ((size_t)q * gridDim.x + blockIdx.x) * K;
        int k = 0;
        for (; k < K; k++) {
            uint64_t m = key[0];
#pragma unroll
            for (int i = 1; i < kPerLane; i++) m = key[i] < m ? key[i] : m;
            const uint64_t b = wave_min_u64(m);
            if (b == kNoKey) break;                                   // (the same for every lane)
            if (lane == 0) out[k] = b;
#pragma unroll
            for (int i = 0; i < kPerLane; i++) key[i] = key[i] == b ? kNoKey : key[i];
        }
        for (int j = k + lane; j < K; j += 64) out[j] = kNoKey;
    }
}

// Pass 2: one block per query, K rounds of "the smallest key above the previous one" (keys of distinct slots are distinct).
__global__ __launch_bounds__(kSelectBlock) void k_app_select_merge(const unsigned long long* __restrict__ part, int n_tiles, int K,
                                                                   int32_t* __restrict__ cand, unsigned long long* __restrict__ keys) {
    __shared__ uint64_t wmin[2][4];
    const int q = blockIdx.x;
    const unsigned long long* in = part + (size_t)q * n_tiles * K;
    const int n = n_tiles * K;
    uint64_t prev = 0; bool have_prev = false;
    uint64_t reg[kMergeRegs];
#pragma unroll
    for (int i = 0; i < kMergeRegs; i++) { const int j = threadIdx.x + kSelectBlock * i; reg[i] = j < n ? in[j] : kNoKey; }
    int k = 0;
    for (; k < K; k++) {
        uint64_t m = kNoKey;
#pragma unroll
        for (int i = 0; i < kMergeRegs; i++) { const uint64_t v = reg[i]; if ((!have_prev || v > prev) && v < m) m = v; }
        for (int i = threadIdx.x + kSelectBlock * kMergeRegs; i < n; i += kSelectBlock) { const uint64_t v = in[i]; if ((!have_prev || v > prev) && v < m) m = v; }
        m = wave_min_u64(m);
        if ((threadIdx.x & 63) == 0) wmin[k & 1][threadIdx.x >> 6] = m;
        __syncthreads();
        const uint64_t a = wmin[k & 1][0], b2 = wmin[k & 1][1], c2 = wmin[k & 1][2], d2 = wmin[k & 1][3];
        const uint64_t ab = a < b2 ? a : b2, cd = c2 < d2 ? c2 : d2;
        const uint64_t b = ab < cd ? ab : cd;
        if (b == kNoKey) break;
        if (threadIdx.x == 0) { cand[q * K + k] = icet_closure_rule::key_slot(b); keys[q * K + k] = b; }
        prev = b; have_prev = true;
    }
    for (int j = k + threadIdx.x; j < K; j += kSelectBlock) { cand[q * K + j] = -1; keys[q * K + j] = kNoKey; }
}

// One thread per (query, candidate).  dist / shift / x0_base (each may be null): the candidate's distance (+inf for a missing one), shift (-1) and start pose
// (zeros).  shift_of: the call's own copy of the shifts, for the record.  With n_starts > 0 the registrations r = (q K + k) S + s as k_closure_resolve writes them.
__global__ __launch_bounds__(64) void k_app_resolve(int cap, int A, AppOffsets off, int n_queries, int K, int n_starts, int any_slot, const int32_t* __restrict__ cand,
                                                    const unsigned long long* __restrict__ keys, const uint16_t* __restrict__ shift_all, float* __restrict__ dist,
                                                    int32_t* __restrict__ shift, float* __restrict__ x0_base, int32_t* __restrict__ shift_of, float* __restrict__ x0,
                                                    int32_t* __restrict__ kf_of, int32_t* __restrict__ rows, int32_t* __restrict__ members, int32_t* __restrict__ offs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (offs && i <= n_queries) offs[i] = i * K * n_starts;
    if (i >= n_queries * K) return;
    const int q = i / K;
    const int slot = cand[i];
    const int sh = slot >= 0 ? (int)shift_all[(size_t)q * cap + slot] : -1;
    float b[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (slot >= 0) b[5] = rule::shift_yaw(sh, A);
    if (dist) dist[i] = slot >= 0 ? icet_closure_rule::key_d2(keys[i]) : __builtin_inff();
    if (shift) shift[i] = sh;
    if (shift_of) shift_of[i] = sh;
    if (x0_base) for (int c = 0; c < 6; c++) x0_base[(size_t)i * 6 + c] = b[c];
    for (int s = 0; s < n_starts; s++) {
        const int r = i * n_starts + s;
        for (int c = 0; c < 6; c++) x0[(size_t)r * 6 + c] = slot >= 0 ? b[c] + off.off[s][c] : 0.f;
        kf_of[r] = slot >= 0 ? slot : any_slot;
        rows[r] = slot >= 0 ? INT32_MAX : 0;
        members[r] = r;
    }
}

// One thread per query: k_closure_record with the appearance distance in d2 and the shift in reserved0.  best == nullptr: no registration ran.
__global__ __launch_bounds__(64) void k_app_record(PoseTable tab, int n_queries, int K, int n_starts, float max_chi2_per_voxel, int min_voxels,
                                                   const int32_t* __restrict__ best, const int32_t* __restrict__ cand, const unsigned long long* __restrict__ keys,
                                                   const int32_t* __restrict__ shift_of, const float* __restrict__ x0, const float* __restrict__ out,
                                                   const icet_score* __restrict__ score, icet_closure* __restrict__ rec) {
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
        c.slot = slot; c.stamp = tab.stamp[slot]; c.d2 = icet_closure_rule::key_d2(keys[i]); c.reserved0 = shift_of[i];
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

}  // namespace

#define ICET_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

constexpr int kAppLdsCells = 12288;                 // 48 KB of words: the largest table k_app_build keeps in LDS

hipError_t launch_app_build(const AppScans& sc, int n_scans, const int32_t* d_rows, const icet_appearance_rule::Consts& c, uint32_t* d_scratch, hipStream_t st) {
    if (n_scans <= 0) return hipSuccess;
    if (n_scans > kAppBatch) return hipErrorInvalidValue;
    int max_n = 0;
    for (int k = 0; k < n_scans; k++) max_n = sc.n[k] > max_n ? sc.n[k] : max_n;
    if (max_n == 0) return hipSuccess;                                // nothing to read: the scratch stays zero
    // 4096 points per block (16 per thread), at most 256 blocks per scan
    int chunks = (max_n + 4095) / 4096;
    if (chunks > 256) chunks = 256;
    int per_block = (max_n + chunks - 1) / chunks;
    per_block = (per_block + kBuildBlock - 1) / kBuildBlock * kBuildBlock;
    const int cells = c.A * c.Rn;
    if (cells <= kAppLdsCells) k_app_build<true><<<dim3(chunks, n_scans), kBuildBlock, sizeof(uint32_t) * (size_t)cells, st>>>(sc, d_rows, c, d_scratch, per_block);
    else k_app_build<false><<<dim3(chunks, n_scans), kBuildBlock, 0, st>>>(sc, d_rows, c, d_scratch, per_block);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_app_finish(const AppScans& sc, int n_scans, const icet_appearance_rule::Consts& c, uint32_t* d_scratch, const AppTable* tab,
                             uint8_t* d_desc, float* d_weight, hipStream_t st) {
    if (n_scans <= 0) return hipSuccess;
    if (n_scans > kAppBatch) return hipErrorInvalidValue;
    k_app_finish<<<n_scans, kBuildBlock, 0, st>>>(sc, c, d_scratch, tab != nullptr, tab ? *tab : AppTable{}, d_desc, d_weight);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_app_set_stamp(const PoseTable& tab, const AppStamps& s, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (n > kAppBatch) return hipErrorInvalidValue;
    k_app_set_stamp<<<1, kAppBatch, 0, st>>>(tab, s, n);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_app_search(const AppTable& tab, const PoseTable& poses, const uint32_t* d_qdesc, const float* d_qw, const AppQueryStamps& qs, int n_queries, int K,
                             float max_distance, int64_t min_gap, unsigned long long* d_keys_all, uint16_t* d_shift_all, unsigned long long* d_part,
                             int32_t* d_cand, unsigned long long* d_keys, hipStream_t st) {
    const int threads = (tab.A + 63) / 64 * 64;
    const size_t lds = sizeof(uint32_t) * ((size_t)tab.A * tab.Rp + (size_t)tab.A * (tab.Rp | 1) + 2 * (size_t)tab.A);
    k_app_match<<<tab.cap, threads, lds, st>>>(tab, d_qdesc, d_qw, n_queries, poses.stamp, qs, max_distance, min_gap, d_keys_all, d_shift_all);
    ICET_LAUNCH_CHECK();
    const int tiles = closure_tiles(tab.cap);
    k_app_select_tiles<<<tiles, kSelectBlock, 0, st>>>(d_keys_all, tab.cap, n_queries, K, d_part);
    ICET_LAUNCH_CHECK();
    k_app_select_merge<<<n_queries, kSelectBlock, 0, st>>>(d_part, tiles, K, d_cand, d_keys);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_app_resolve(int cap, int A, const AppOffsets& off, int n_queries, int K, int n_starts, int any_slot, const int32_t* d_cand,
                              const unsigned long long* d_keys, const uint16_t* d_shift_all, float* d_dist, int32_t* d_shift, float* d_x0_base, int32_t* d_shift_of,
                              float* d_x0, int32_t* d_kf_of, int32_t* d_rows, int32_t* d_members, int32_t* d_offs, hipStream_t st) {
    const int n = n_queries * K > n_queries + 1 ? n_queries * K : n_queries + 1;
    k_app_resolve<<<(n + 63) / 64, 64, 0, st>>>(cap, A, off, n_queries, K, n_starts, any_slot, d_cand, d_keys, d_shift_all, d_dist, d_shift, d_x0_base, d_shift_of,
                                               d_x0, d_kf_of, d_rows, d_members, d_offs);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_app_record(const PoseTable& tab, int n_queries, int K, int n_starts, float max_chi2_per_voxel, int min_voxels, const int32_t* d_best,
                             const int32_t* d_cand, const unsigned long long* d_keys, const int32_t* d_shift_of, const float* d_x0, const float* d_out,
                             const ::icet_score* d_score, ::icet_closure* d_closure, hipStream_t st) {
    k_app_record<<<(n_queries + 63) / 64, 64, 0, st>>>(tab, n_queries, K, n_starts, max_chi2_per_voxel, min_voxels, d_best, d_cand, d_keys, d_shift_of, d_x0, d_out,
                                                      d_score, d_closure);
    ICET_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace icet
