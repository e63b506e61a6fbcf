// icet_amd/csrc/icet_appearance.hip -- place recognition by appearance for the keyframe store (include/icet_hip.h icet_keyframe_store_close_appearance_device;
// DESIGN.md section 17).  The rule -- cell, height code, weight, distance, eligibility, start pose -- is icet_appearance.h; this file is the kernels around it:
//     k_app_build          the cells of a batch of scans: a block takes a run of one scan's points, keeps the maxima of its cells in LDS and flushes the cells it
//                          touched into the scan's table of the scratch with integer-maximum atomics
//     k_app_finish         one block per scan: the scratch table to bytes (row-major for a caller, ring-packed columns for the store), the column weights, and the
//                          scratch back to zero for the next batch
//     k_app_set_stamp      stamps without poses
//     k_app_match          one block per slot: every shift's distance to each query, one lane per shift walking the columns in ascending order; the slot's key
//     k_app_select_tiles   the K smallest keys of each query, pass 1: tiles of 1024 slots; pass 2 and the record are icet_closure.hip's (launch_closure_merge,
//                          launch_closure_record with the candidates' shifts)
//     k_app_resolve        one thread per (query, candidate): distance, shift, start poses, keyframe index and row count of its registrations
// Maxima and minima of integers only: no float atomic, no dependence on the launch shape.  No kernel waits for another block.
#include <hip/hip_runtime.h>
#include "../../include/icet_hip.h"
#include "icet_internal.h"
#include "icet_appearance.h"
#include "icet_closure_device.h"

namespace icet {
namespace {

using icet_closure_rule::kNoKey;
namespace rule = icet_appearance_rule;

constexpr int kBuildBlock = 256;

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
    select_tile_smallest(n_queries, K, part, [&](int q, int s) -> uint64_t {
        const int slot = base + s;
        return slot < cap ? keys_all[(size_t)q * cap + slot] : kNoKey;
    });
}

// One thread per (query, candidate).  dist / shift / x0_base (each may be null): the candidate's distance (+inf for a missing one), shift (-1) and start pose
// (zeros).  shift_of: the call's own copy of the shifts, for the record.  With n_starts > 0 the registrations r = (q K + k) S + s as k_closure_resolve writes them.
__global__ __launch_bounds__(64) void k_app_resolve(int cap, int A, AppOffsets off, int n_queries, int K, int n_starts, int any_slot, const int32_t* __restrict__ cand,
                                                    const unsigned long long* __restrict__ keys, const uint16_t* __restrict__ shift_all, float* __restrict__ dist,
                                                    int32_t* __restrict__ shift, float* __restrict__ x0_base, int32_t* __restrict__ shift_of, float* __restrict__ x0,
                                                    int32_t* __restrict__ kf_of, int32_t* __restrict__ rows, int32_t* __restrict__ members, int32_t* __restrict__ offs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    write_group_offset(i, n_queries, K, n_starts, offs);
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
    write_registrations(i, slot, any_slot, b, off.off, n_starts, x0, kf_of, rows, members);
}

}  // namespace

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
    return launch_closure_merge(d_part, tiles, n_queries, K, d_cand, d_keys, st);
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

}  // namespace icet
