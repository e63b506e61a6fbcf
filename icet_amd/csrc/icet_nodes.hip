// icet_amd/csrc/icet_nodes.hip -- the callers on either side of the hot path, on the device (include/icet_nodes.h):
// the per-frame body of the reference's odometry_node / map_maker_node (src/odometry.cpp:46-98,
// src/simpleMapMaker.cpp:86-172) and the HD-map FIFO `EigenQueue` (src/simpleMapMaker.cpp:18-59).
//
// Built only on the public C ABI of icet_hip.h (one single-pair icet_solve_batch_device per frame) plus three small
// HBM-bound kernels of its own:
//   k_range_count / k_range_scan / k_range_scatter   the `row.norm() > minD` filter as a stable stream compaction
//                                                    (12 B read twice + 12 B written per kept row)
//   k_map_add_scan                                    EigenQueue::add_new_scan: the down-sampled rows enter the ring and
//                                                    the whole ring is re-expressed as (row - t) * R^-1 in ONE pass
//                                                    (12 B read + 12 B written per ring row)
// Each row pass is stated once, as a __device__ body; the kernels above and the node group's k_group_* (second half of this file) are its two launch forms.  What a
// stream keeps between frames (StreamState) and the host rules on it are stated once as well, for icet_node and icet_node_group alike.
// Host-side scalar work (pose chaining, quaternion, the 3x3 inverse, std::shuffle of the index vector) stays on the
// host as in the reference: it is O(1) or inherently sequential (Fisher-Yates with one RNG stream).
// No CPU implementation of the solve lives here; without a device every entry point fails with an error status.
#include "../../include/icet_nodes.h"
#include "icet_shuffle.h"
#include "icet_node_tail.h"
#include "icet_buffers.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <numeric>
#include <random>
#include <future>
#include <memory>
#include <thread>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <condition_variable>
#include <deque>
#include <functional>
#include <string>
#include <vector>

namespace {

constexpr int kFB = 256;            // threads per block of the filter kernels
constexpr int kFRows = 8;           // rows per thread: a block owns 2048 consecutive rows

// Where a frame's raw scan is, for filter launches that are part of a captured graph (round 6): the record lives in pinned host memory, the host fills it in before
// every replay and the kernels read it (the same arrangement as the loop's X0) -- the launches themselves (grid from the buffers' CAPACITY) never change.
struct FrameDesc { const float* x; int32_t n, ld; };

__device__ __forceinline__ bool keep_row(float x, float y, float z, float min_range) {
    float d;
    {
#pragma clang fp contract(off)
        float s = x * x + y * y;      // Eigen's row(i).norm(): sqrt of the plain sum of squares (src/odometry.cpp:61-64)
        s = s + z * z;
        d = sqrtf(s);
    }
    return d > min_range;
}

// ---- the row passes.  Each has ONE body (__forceinline__); the node's kernel and the group's find their pointers, their row base and their keep_all and call it ----

// pass 1: kept rows of the block that owns rows [base, base + kFB * kFRows), thread 0 stores the count
__device__ __forceinline__ void count_block(const float* x, const float* y, const float* z, int n, int base, bool keep_all, float min_range, int32_t* count) {
    __shared__ int wsum[kFB / 64];
    int c = 0;
#pragma unroll
    for (int k = 0; k < kFRows; k++) {
        const int i = base + k * kFB + threadIdx.x;
        if (i < n) c += (keep_all || keep_row(x[i], y[i], z[i], min_range)) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < kFB / 64; w++) t += wsum[w]; *count = t; }
}

// pass 2: exclusive scan of n_blocks block counts by one block (at most a few thousand entries); the total goes to *total and, where there is one, to its copy in
// pinned host memory (a host thread may be watching it: the store is followed by a system-scope fence)
__device__ __forceinline__ void scan_block_counts(const int32_t* counts, int32_t* bases, int n_blocks, int32_t* total, int32_t* total_copy) {
    __shared__ int part[kFB];
    const int per = (n_blocks + kFB - 1) / kFB;
    const int lo = threadIdx.x * per, hi = min(n_blocks, lo + per);
    int s = 0;
    for (int i = lo; i < hi; i++) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { int run = 0; for (int t = 0; t < kFB; t++) { const int v = part[t]; part[t] = run; run += v; } *total = run; if (total_copy) { *total_copy = run; __threadfence_system(); } }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; i++) { bases[i] = run; run += counts[i]; }
}

// pass 3: stable scatter, in two halves.  Row order inside a block is k-major (row = base + k * kFB + thread), so the rank of a kept row is: kept rows in earlier
// k-slices + kept rows of lower threads in its own slice.
struct ScatterRows { float vx[kFRows], vy[kFRows], vz[kFRows]; bool keep[kFRows]; int below[kFRows]; };      // a thread's eight rows, in registers
using ScatterCounts = int[kFRows][kFB / 64];                                                                   // kept rows by k-slice and wave, in LDS
// ... first half: load, ballot and rank the eight k-slices (a barrier belongs between the halves)
__device__ __forceinline__ void scatter_rank(const float* x, const float* y, const float* z, int n, int base, bool keep_all, float min_range, ScatterRows& r, ScatterCounts& wcnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kFRows; k++) {
        const int i = base + k * kFB + threadIdx.x;
        r.keep[k] = false; r.vx[k] = r.vy[k] = r.vz[k] = 0.f;
        if (i < n) { r.vx[k] = x[i]; r.vy[k] = y[i]; r.vz[k] = z[i]; r.keep[k] = keep_all || keep_row(r.vx[k], r.vy[k], r.vz[k], min_range); }
        const unsigned long long m = __ballot(r.keep[k]);
        r.below[k] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[k][wave] = __popcll(m);
    }
}
// ... second half: run = kept rows in front of this block; store the kept rows
__device__ __forceinline__ void scatter_store(const ScatterRows& r, const ScatterCounts& wcnt, int run, float* ox, float* oy, float* oz) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kFRows; k++) {
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kFB / 64; w++) { const int cw = wcnt[k][w]; before += (w < wave) ? cw : 0; total += cw; }
        if (r.keep[k]) { const int o = run + before + r.below[k]; ox[o] = r.vx[k]; oy[o] = r.vy[k]; oz[o] = r.vz[k]; }
        run += total;
    }
}

struct RowMove { float tx, ty, tz, i00, i01, i02, i10, i11, i12, i20, i21, i22; };      // a frame's translation and R^-1 (row-major), as the two passes below apply them
inline RowMove row_move(const float* X, const float* Ri) { return RowMove{X[0], X[1], X[2], Ri[0], Ri[1], Ri[2], Ri[3], Ri[4], Ri[5], Ri[6], Ri[7], Ri[8]}; }

// EigenQueue::add_new_scan (src/simpleMapMaker.cpp:34-41): rows [pos, pos + m) (mod cap) take the down-sampled scan
// rows, then EVERY ring row becomes (row - trans) * Rinv.  One pass over the ring (a grid-stride loop in the kernels); this is ring row i.
__device__ __forceinline__ void ring_add_scan_row(int i, float* qx, float* qy, float* qz, int cap, int pos, int m, const float* sx, const float* sy, const float* sz, const int32_t* idx, const RowMove& T) {
    int j = i - pos; if (j < 0) j += cap;                 // position in this frame's write window
    float a, b, c;
    if (j < m) { const int r = idx[j]; a = sx[r]; b = sy[r]; c = sz[r]; }
    else { a = qx[i]; b = qy[i]; c = qz[i]; }
    a -= T.tx; b -= T.ty; c -= T.tz;
    {
#pragma clang fp contract(off)
        qx[i] = (a * T.i00 + b * T.i10) + c * T.i20;
        qy[i] = (a * T.i01 + b * T.i11) + c * T.i21;
        qz[i] = (a * T.i02 + b * T.i12) + c * T.i22;
    }
}

// scan2_in_scan1_frame = (pcl_matrix * rot_mat.inverse()).rowwise() - trans  (src/scanMatcher.cpp:76): rotate first, then subtract; this is row i
__device__ __forceinline__ void align_row(int i, const float* sx, const float* sy, const float* sz, float* ox, float* oy, float* oz, const RowMove& T) {
    const float a = sx[i], b = sy[i], c = sz[i];
    {
#pragma clang fp contract(off)
        ox[i] = ((a * T.i00 + b * T.i10) + c * T.i20) - T.tx;
        oy[i] = ((a * T.i01 + b * T.i11) + c * T.i21) - T.ty;
        oz[i] = ((a * T.i02 + b * T.i12) + c * T.i22) - T.tz;
    }
}

// ---- the node's launch form: pointers in the arguments, or in a pinned FrameDesc where the launch is part of a captured graph; every row goes through keep_row ----
__global__ __launch_bounds__(kFB) void k_range_count(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n,
                                                    float min_range, int32_t* __restrict__ counts, const FrameDesc* __restrict__ fd = nullptr) {
    if (fd) { const FrameDesc d = *fd; x = d.x; y = d.x + d.ld; z = d.x + 2 * (size_t)d.ld; n = d.n; }
    count_block(x, y, z, n, blockIdx.x * kFB * kFRows, false, min_range, counts + blockIdx.x);
}

__global__ __launch_bounds__(kFB) void k_range_scan(const int32_t* __restrict__ counts, int32_t* __restrict__ bases, int n_blocks, int32_t* __restrict__ n_kept, int32_t* __restrict__ n_kept_copy = nullptr) {
    scan_block_counts(counts, bases, n_blocks, n_kept, n_kept_copy);
}

__global__ __launch_bounds__(kFB) void k_range_scatter(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n,
                                                      float min_range, const int32_t* __restrict__ bases,
                                                      float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz, const FrameDesc* __restrict__ fd = nullptr,
                                                      const int32_t* __restrict__ counts = nullptr, int n_blocks = 0, int32_t* __restrict__ n_kept = nullptr, int32_t* __restrict__ n_kept_copy = nullptr) {
    __shared__ ScatterCounts wcnt;
    __shared__ int s_part[kFB / 64], s_tot[kFB / 64];
    if (fd) { const FrameDesc d = *fd; x = d.x; y = d.x + d.ld; z = d.x + 2 * (size_t)d.ld; n = d.n; }
    // counts: pass 2 folded in (a one-launch frame, at most a few hundred blocks): every block adds up the counts of the blocks in front of it itself, block 0 also the
    // total -- k_range_scan's 4.6 us launch is what the frame saves
    int part = 0, tot = 0;
    if (counts) for (int i = threadIdx.x; i < n_blocks; i += kFB) { const int c = counts[i]; tot += c; part += (i < (int)blockIdx.x) ? c : 0; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ScatterRows r;
    scatter_rank(x, y, z, n, blockIdx.x * kFB * kFRows, false, min_range, r, wcnt);
    if (counts) {
        for (int o = 32; o > 0; o >>= 1) { part += __shfl_down(part, o); tot += __shfl_down(tot, o); }
        if (lane == 0) { s_part[wave] = part; s_tot[wave] = tot; }
    }
    __syncthreads();
    int run;
    if (counts) {
        run = 0; int t = 0;
#pragma unroll
        for (int w = 0; w < kFB / 64; w++) { run += s_part[w]; t += s_tot[w]; }
        if (blockIdx.x == 0 && threadIdx.x == 0) { *n_kept = t; if (n_kept_copy) { *n_kept_copy = t; __threadfence_system(); } }
    } else run = bases[blockIdx.x];
    scatter_store(r, wcnt, run, ox, oy, oz);
}

__global__ __launch_bounds__(256) void k_map_add_scan(float* __restrict__ qx, float* __restrict__ qy, float* __restrict__ qz, int cap, int pos, int m,
                                                     const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
                                                     const int32_t* __restrict__ idx, float tx, float ty, float tz,
                                                     float i00, float i01, float i02, float i10, float i11, float i12, float i20, float i21, float i22) {
    const RowMove T{tx, ty, tz, i00, i01, i02, i10, i11, i12, i20, i21, i22};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += gridDim.x * blockDim.x) ring_add_scan_row(i, qx, qy, qz, cap, pos, m, sx, sy, sz, idx, T);
}

__global__ __launch_bounds__(256) void k_align_cloud(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int n,
                                                    float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz, float tx, float ty, float tz,
                                                    float i00, float i01, float i02, float i10, float i11, float i12, float i20, float i21, float i22) {
    const RowMove T{tx, ty, tz, i00, i01, i02, i10, i11, i12, i20, i21, i22};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) align_row(i, sx, sy, sz, ox, oy, oz, T);
}

// getQueue (src/simpleMapMaker.cpp:43-50): oldest row first
__global__ __launch_bounds__(256) void k_map_unroll(const float* __restrict__ qx, const float* __restrict__ qy, const float* __restrict__ qz, int cap, int pos,
                                                   int filled, int rows, float* __restrict__ out, int ld) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += gridDim.x * blockDim.x) {
        const int s = filled ? (pos + i) % cap : i;
        out[i] = qx[s]; out[ld + i] = qy[s]; out[2 * (size_t)ld + i] = qz[s];
    }
}

// The scalars of a frame's tail -- R from the frame's Euler angles, R^-1 (always: the caller ignores it when nothing consumes it), the chained pose and its quaternion
// (icet_node_tail.h) -- compiled ONCE: frame_tail and the test hook icet_debug_node_tail call this body, so what the hook returns is what a frame computes.
using icet_node_tail::quat_of;
__attribute__((noinline)) void node_tail_scalars(const float X[6], const float pose_in[16], float R[9], float Rinv[9], float pose_out[16], float quat[4]) {
    icet_node_tail::tail_scalars(X, pose_in, R, Rinv, pose_out, quat);
}

}  // namespace

void icet_ctx_set_stream(icet_ctx* c, hipStream_t s);      // icet_capi.hip (internal)
void icet_ctx_set_prologue(icet_ctx* c, hipError_t (*fn)(void*, hipStream_t), void* user, int64_t key);      // icet_capi.hip (internal)
void icet_ctx_set_done_flag(icet_ctx* c, int32_t* pinned_word);      // icet_capi.hip (internal)

// ==================================================================================================================================================================
// What a stream keeps between frames, and the host rules on top of it: ONE statement of each, used by icet_node (which embeds one StreamState) and by icet_node_group
// (a vector of them).  The helpers that report a HIP failure take the node or the group itself: anything with an `err` (and, for the copies out, a `stream`, a `device`
// and the parameters `p`).
// ==================================================================================================================================================================
namespace {

struct StreamState {
    bool initialized = false;
    // previous / current filtered scan (column-major, ld = cap rounded to 64)
    float* d_scan[2] = {nullptr, nullptr}; int64_t cap_scan[2] = {0, 0}; int64_t n_scan[2] = {0, 0}; int64_t ld_scan[2] = {0, 0};
    int prev = 0;
    float X0[6] = {0, 0, 0, 0, 0, 0};
    float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::mt19937 gen;                                              // default seed: simpleMapMaker.cpp:258 (one generator per stream)
    icet_shuffle::FastMt fgen;                                     // the same stream written out (icet_shuffle.h); used when it reproduced std::shuffle on this C++ library at creation
    std::vector<std::size_t> indices;
    float* d_map = nullptr; int64_t map_pos = 0; bool map_filled = false;
    int32_t* h_idx = nullptr;                                     // pinned: the frame's down-sample indices (the map kernel can read them in place)
    float* d_aligned = nullptr; int64_t cap_aligned = 0, n_aligned = 0, ld_aligned = 0;     // scanMatcher.cpp:76
    std::vector<float> snail;                                                               // scanMatcher.cpp:27-28,79-84: rows x 3 row-major, host
    icet::BufferGroup fixed, scan_mem[2], aligned_mem;                                      // owners: d_map + h_idx (creation); d_scan[i]; d_aligned.  They free when the stream goes
};

#define NCHK(o, call) do { const hipError_t e_ = static_cast<hipError_t>(call); if (e_ != hipSuccess) { \
    (o)->err = std::string(#call) + ": " + hipGetErrorString(e_); \
    return e_ == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; } } while (0)

bool node_params_ok(const icet_ctx* ctx, const icet_node_params* p) {
    return ctx && p && p->map_capacity >= 0 && p->map_downsample >= 0 && !(p->map_capacity > 0 && p->map_downsample > p->map_capacity) &&
           p->solve.bins_phi > 0 && p->solve.bins_theta > 0 && p->solve.n >= 1 && p->solve.runlen >= 0;
}

// (a few milliseconds, once per process: the written-out generator against this C++ library's std::shuffle)
bool fast_shuffle_ok() { static const bool ok = icet_shuffle::matches_std_shuffle() && icet_shuffle::fast_matches_std_shuffle(); return ok; }

// The map ring (zeroed: Eigen leaves MatrixXf(maxSize, 3) uninitialised; unfilled rows are never returned by getQueue), its pinned index buffer, the snail trail's first row
icet_status stream_create(const icet_node_params& p, StreamState& st) {
    if (p.map_capacity > 0) {
        if (st.fixed.device(st.d_map, 3 * (size_t)p.map_capacity) != 0) return ICET_ERR_NOMEM;
        if (hipMemset(st.d_map, 0, sizeof(float) * 3 * (size_t)p.map_capacity) != hipSuccess) return ICET_ERR_HIP;
        if (st.fixed.pinned(st.h_idx, (size_t)std::max(p.map_downsample, 1)) != 0) return ICET_ERR_NOMEM;
    }
    if (p.flags & ICET_NODE_SNAIL_TRAIL) st.snail.assign(3, 0.f);      // scanMatcher.cpp:27-28: one row at the origin
    return ICET_OK;
}

// No exception may cross the C ABI (std::async and the draw pool can throw std::system_error, the shuffle's vector bad_alloc): f's status, or the exception as one
template <class F> icet_status no_throw(std::string& err, F&& f) {
    try { return f(); }
    catch (const std::bad_alloc&) { err = "out of host memory"; }
    catch (const std::exception& e) { err = std::string("host error: ") + e.what(); }
    catch (...) { err = "host error"; }
    return ICET_ERR_NOMEM;
}

// A kernel stores into pinned host memory and this thread watches the word(s): hipStreamSynchronize answers several microseconds after the queue has drained, so the
// stream is asked only every mask + 1 looks (a frame that failed never stores: then the stream says so), and once more, synchronised, before `what` is given up for lost.
template <class O, class P> icet_status wait_pinned(O* o, P&& arrived, hipStream_t st, long mask, const char* what) {
    for (long spins = 1; !arrived(); spins++)
        if ((spins & mask) == 0 && hipStreamQuery(st) != hipErrorNotReady) break;      // (finished or failed without the store: decided below)
    (void)hipGetLastError();
    if (!arrived()) NCHK(o, hipStreamSynchronize(st));
    if (!arrived()) { o->err = what; return ICET_ERR_HIP; }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return ICET_OK;
}

// Every growth below is icet::grow (icet_buffers.h) behind the caller's drain: a refused one leaves capacity 0 and null pointers, and the next call grows again.
// A scan-sized buffer: (n + n / 8) rows rounded to 64.  drain() makes sure that nothing on the device still reads the old one.
template <class O, class D> icet_status grow_rows(O* o, icet::BufferGroup& g, float*& buf, int64_t& cap, int64_t n, D&& drain) {
    if (n <= cap) return ICET_OK;
    NCHK(o, drain());
    const int64_t c = (n + n / 8 + 63) / 64 * 64;
    NCHK(o, icet::grow(g, cap, c, [&] { return g.device(buf, 3 * (size_t)c); }));
    return ICET_OK;
}
// The range filter's block counts and their bases, n of each
template <class O, class D> icet_status grow_blocks(O* o, icet::BufferGroup& g, int32_t*& counts, int32_t*& bases, int64_t& cap, int64_t n, D&& drain) {
    if (n <= cap) return ICET_OK;
    NCHK(o, drain());
    NCHK(o, icet::grow(g, cap, n, [&] { const int e = g.device(counts, (size_t)n); return e ? e : g.device(bases, (size_t)n); }));
    return ICET_OK;
}

// The frame's down-sample indices into pinned h_idx (simpleMapMaker.cpp:147-158: iota, std::shuffle with the stream's generator, the first map_downsample entries): returns
// how many.  Only the first entries of the shuffled vector are ever used, so only they are tracked while the generator makes its n - 1 draws (icet_shuffle.h).
int draw_downsample(StreamState& st, bool fast, int32_t map_downsample, int64_t nk) {
    if (fast) icet_shuffle::head_of_shuffled_iota((std::size_t)nk, (std::size_t)map_downsample, st.fgen, st.indices);
    else icet_shuffle::head_of_shuffled_iota((std::size_t)nk, (std::size_t)map_downsample, st.gen, st.indices);
    const int m = (int)st.indices.size();
    for (int i = 0; i < m; i++) st.h_idx[i] = (int32_t)st.indices[i];
    return m;
}

int64_t map_rows(const icet_node_params& p, const StreamState& st) { return st.map_filled ? p.map_capacity : st.map_pos; }

// A stream's first cloud is stored as it is and nothing is solved (odometry.cpp:46-52): its result (res is zeroed)
void first_result(const icet_node_params& p, const StreamState& st, int64_t n, icet_node_result* res) {
    res->solved = 0; res->n_kept = n;
    std::memcpy(res->pose, st.pose, sizeof(st.pose)); quat_of(st.pose, res->quat);
    res->map_rows = map_rows(p, st);
}

// The host tail of a solved frame: X and pred_stds from the solve's 48 result floats,
// X0 seeded for the next frame (odometry.cpp:82 / simpleMapMaker.cpp:124), the divergence guard (simpleMapMaker.cpp:129-137), the map ring's bookkeeping
// (simpleMapMaker.cpp:147-158, 34-41), the snail trail (scanMatcher.cpp:79-84), the pose chain X_homo = X_homo * X_homo_i (odometry.cpp:91-98) and the result.
// The device work in between is the caller's: map_dev(X, R^-1, ring position, rows) in front of the ring's bookkeeping, align_dev(X, R^-1) behind it; a failure
// either returns ends the tail there (nothing behind it has changed).  One compiled body (noinline): the same bits whoever calls it.
using TailMapDev = std::function<icet_status(const float* X, const float* Ri, int64_t pos, int m)>;
using TailAlignDev = std::function<icet_status(const float* X, const float* Ri)>;
__attribute__((noinline)) icet_status frame_tail(const icet_node_params& p, StreamState& st, const float* out48, int64_t nk, int m_map, icet_node_result* res,
                                                 const TailMapDev& map_dev, const TailAlignDev& align_dev) {
    float X[6];
    std::memcpy(X, out48, sizeof(X)); std::memcpy(res->pred_stds, out48 + 6, sizeof(float) * 6);
    // seed for the next frame (odometry.cpp:82 / simpleMapMaker.cpp:124), then the guard (simpleMapMaker.cpp:129-137)
    for (int k = 0; k < 6; k++) st.X0[k] = p.seed_x0 ? X[k] : 0.f;
    {
        // each group is guarded only when ITS threshold is set (0 = off, include/icet_nodes.h): a caller who sets one of the two
        // must not have the other group compared against 0
        const float tt = p.trans_thresh, rt = p.rot_thresh;
        if ((tt > 0.f && (std::fabs(X[0]) > tt || std::fabs(X[1]) > tt || std::fabs(X[2]) > tt)) ||
            (rt > 0.f && (std::fabs(X[3]) > rt || std::fabs(X[4]) > rt || std::fabs(X[5]) > rt))) {
            for (int k = 0; k < 6; k++) X[k] = 0.f;
            res->diverged = 1;
        }
    }
    float R[9], Ri[9], P[16], quat[4];
    node_tail_scalars(X, st.pose, R, Ri, P, quat);                // (st.pose is not touched before the chain below commits P)
    // ---- map queue (simpleMapMaker.cpp:147-158, 34-41) ----
    if (p.map_capacity > 0) {
        const int cap = p.map_capacity;
        const icet_status ds = map_dev(X, Ri, st.map_pos, m_map); if (ds != ICET_OK) return ds;
        if (st.map_pos + m_map >= cap) st.map_filled = true;
        st.map_pos = (st.map_pos + m_map) % cap;
    }
    if (p.flags & ICET_NODE_ALIGNED_CLOUD) { const icet_status ds = align_dev(X, Ri); if (ds != ICET_OK) return ds; }
    if (p.flags & ICET_NODE_SNAIL_TRAIL) {                        // snailTrail = (snailTrail * rot_mat.inverse()).rowwise() - trans; append the origin
        std::vector<float>& sn = st.snail;
        for (size_t i = 0; i + 2 < sn.size(); i += 3) {
            const float a = sn[i], b = sn[i + 1], c = sn[i + 2];
            sn[i] = ((a * Ri[0] + b * Ri[3]) + c * Ri[6]) - X[0];
            sn[i + 1] = ((a * Ri[1] + b * Ri[4]) + c * Ri[7]) - X[1];
            sn[i + 2] = ((a * Ri[2] + b * Ri[5]) + c * Ri[8]) - X[2];
        }
        sn.insert(sn.end(), {0.f, 0.f, 0.f});
    }
    // X_homo = X_homo * X_homo_i (odometry.cpp:91-98)
    std::memcpy(st.pose, P, sizeof(P));
    res->solved = 1; res->n_kept = nk;
    std::memcpy(res->X, X, sizeof(X)); std::memcpy(res->pose, P, sizeof(P)); std::memcpy(res->quat, quat, sizeof(quat));
    res->map_rows = map_rows(p, st);
    return ICET_OK;
}

// ---- what the accessors return: rows x 3 into out (column-major, ld) ----
enum StreamRows { kRowsMap, kRowsPrevScan, kRowsAligned, kRowsSnail };
// The two surfaces differ in one thing: icet_node_* reports the row count and THEN refuses an `ld` below it, icet_node_group_* refuses before it writes anything.
template <class O> icet_status stream_rows_out(O* o, const StreamState& st, StreamRows what, bool refuse_first, float* out, int64_t ld, int64_t* rows_out) {
    const int64_t rows = what == kRowsMap ? map_rows(o->p, st) : what == kRowsPrevScan ? (st.initialized ? st.n_scan[st.prev] : 0) :
                         what == kRowsAligned ? st.n_aligned : (int64_t)(st.snail.size() / 3);
    if (refuse_first && out && rows > 0 && ld < rows) return ICET_ERR_BAD_ARG;
    *rows_out = rows;
    if (!out || rows == 0) return ICET_OK;
    if (ld < rows) return ICET_ERR_BAD_ARG;
    if (what == kRowsSnail) {
        for (int64_t i = 0; i < rows; i++) { out[i] = st.snail[3 * i]; out[ld + i] = st.snail[3 * i + 1]; out[2 * ld + i] = st.snail[3 * i + 2]; }
        return ICET_OK;
    }
    if (hipSetDevice(o->device) != hipSuccess) return ICET_ERR_NO_DEVICE;
    const float* src = what == kRowsPrevScan ? st.d_scan[st.prev] : st.d_aligned;
    int64_t lds = what == kRowsPrevScan ? st.ld_scan[st.prev] : st.ld_aligned;
    float* tmp = nullptr; icet::BufferGroup g;                   // (freed at every return: behind the synchronisation below)
    if (what == kRowsMap) {                                       // getQueue: the ring unrolled, oldest row first, through a temporary
        NCHK(o, g.device(tmp, 3 * (size_t)rows));
        const int cap = o->p.map_capacity;
        k_map_unroll<<<std::min((int)((rows + 255) / 256), 2048), 256, 0, o->stream>>>(st.d_map, st.d_map + cap, st.d_map + 2 * (size_t)cap, cap, (int)st.map_pos,
                                                                                        st.map_filled ? 1 : 0, (int)rows, tmp, (int)rows);
        src = tmp; lds = rows;
    }
    hipError_t e = tmp ? hipGetLastError() : hipSuccess;
    if (e == hipSuccess) e = hipMemcpy2DAsync(out, ld * sizeof(float), src, lds * sizeof(float), rows * sizeof(float), 3, hipMemcpyDeviceToHost, o->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    if (e != hipSuccess) { o->err = hipGetErrorString(e); return ICET_ERR_HIP; }
    return ICET_OK;
}

}  // namespace

// The helper thread of a pipelined node: it ENQUEUES the keyframe builds (icet_keyframe_device_n on the context the build goes into, then the event that says it is
// done) while the calling thread enqueues the frame's loop.  A build is ~20 launches or one graph launch of 20 nodes -- 35 to 140 us of host time that used to sit between
// the loop's launch and the build's start, so that the build of frame k ran into frame k + 1, whose loop needs it.  One job at a time in order; the calling thread waits
// for "idle" before it touches anything the helper may be using (kf_wait_idle).
struct FilterLaunch { const FrameDesc* fd; float min_range; int32_t* counts; int32_t* bases; int n_blocks; int32_t* d_cnt; int32_t* h_cnt; float* o; int64_t ld_o; };      // one range filter's three launches
namespace { hipError_t filter_prologue(void* user, hipStream_t st); }
// (f2_ev set: the build is preceded by the keyframe side's own range filter of the raw frame -- the one-launch frame of push_frame -- and f2_ev says when that has read the frame)
struct KfJob { icet_ctx* ctx; icet_params sp; icet_dev_scan b; const int32_t* d_cnt; hipStream_t sk; hipEvent_t done_ev; FilterLaunch f2{}; hipEvent_t f2_ev = nullptr; };
struct KfWorker {
    std::thread th; std::mutex m; std::condition_variable cv; std::deque<KfJob> q;
    long posted = 0, done = 0; bool stop = false; icet_status status = ICET_OK; std::string err; int device = 0;
};

struct icet_node {
    // Keyframe pipelining: scan 2 of frame k is scan 1 of frame k + 1, so the keyframe of a scan is built the
    // moment the scan arrives, on the OTHER of two contexts / streams, while the Gauss-Newton loop of the current pair iterates; the
    // frame-to-pose critical path is then range filter + loop.  kf[owner] holds the parked keyframe of the previous scan.
    // Both contexts are the node's own: a keyframe parked in the caller's context would be lost to the caller's next solve on it.
    icet_ctx* kf[2] = {nullptr, nullptr}; int owner = 0; bool pipelined = false;
    icet_ctx* ctx = nullptr;
    hipStream_t stream = nullptr;
    int device = 0;
    icet_node_params p{};
    std::string err;
    StreamState s;                                                // what the stream keeps between frames
    float* d_stage = nullptr; int64_t cap_stage = 0;              // host scans land here first
    int32_t* d_counts = nullptr; int32_t* d_bases = nullptr; int64_t cap_blocks = 0;
    int32_t* d_nkept = nullptr; int32_t* h_nkept = nullptr;       // d_nkept: TWO counters, one per scan buffer (a frame's count is still read by the keyframe build that runs into the next frame)
    float* d_x0 = nullptr; float* d_out = nullptr; float* h_out = nullptr; float* h_x0 = nullptr;
    bool fast_shuffle = false;                                    // fast_shuffle_ok() at creation
    int32_t* d_idx = nullptr;                                     // the down-sample indices on the device (the frame in phases copies s.h_idx here)
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // [5]: start of the loop on the owner's stream (pipelined)
    bool timing_valid = false, timed_map = false;
    KfWorker* kw = nullptr;                                       // started with the first build that goes through it
    hipEvent_t ev_kfdone[2] = {nullptr, nullptr}; bool kf_built[2] = {false, false};          // per context: its last keyframe build has been enqueued / the event behind it
    // The one-launch frame (round 6, push_frame): the loop's context captures the range filter in front of its loop (FilterLaunch = what its hook enqueues), and the
    // keyframe build of the same scan runs on the other context's stream behind a filter of ITS OWN into a second buffer -- no dependency between the two streams inside a frame.
    FrameDesc* h_frame = nullptr;                                 // pinned, [2]: by scan buffer
    FilterLaunch fl[2];
    float* d_scan_kf[2] = {nullptr, nullptr}; int64_t cap_scan_kf[2] = {0, 0};
    int32_t* d_counts_kf = nullptr; int32_t* d_bases_kf = nullptr; int64_t cap_blocks_kf = 0; int32_t* d_nkept_kf = nullptr;
    hipEvent_t ev_f2 = nullptr;                                   // the keyframe side's filter has read the caller's frame
    int32_t* h_done = nullptr;                                    // pinned, coherent: the frame's last solve stores 1 here behind its results (the host watches it instead of synchronising the stream)
    // owners, one per lifetime: what icet_node_create allocates; h_frame + d_nkept_kf + h_done (ensure_kf_side, once); then one per buffer (pair) that grows on its own
    icet::BufferGroup fixed, kf_fixed, stage_mem, blocks_mem, scan_kf_mem[2], blocks_kf_mem;
#ifdef ICET_DIAG_ENV
    double tr[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long tr_n = 0, tr_seen = 0;       // ICET_NODE_TRACE: host microseconds of push_frame by section, summed (printed by icet_node_destroy)
#endif
};

namespace {

bool kf_worker_start(icet_node* nd) {
    if (nd->kw) return true;
    try {
        KfWorker* w = new KfWorker(); w->device = nd->device;
        w->th = std::thread([w]() {
            (void)hipSetDevice(w->device);
            for (;;) {
                KfJob j;
                { std::unique_lock<std::mutex> lk(w->m); w->cv.wait(lk, [&] { return w->stop || !w->q.empty(); }); if (w->q.empty()) return; j = w->q.front(); w->q.pop_front(); }
                icet_status s = ICET_OK; std::string e;
                bool skip; { std::lock_guard<std::mutex> lk(w->m); skip = w->status != ICET_OK; }      // after a failure the jobs behind it are only counted
                if (!skip && j.f2_ev) {
                    if (filter_prologue(&j.f2, j.sk) != hipSuccess || hipEventRecord(j.f2_ev, j.sk) != hipSuccess) { s = ICET_ERR_HIP; e = "range filter in front of the keyframe build"; }
                }
                if (!skip && s == ICET_OK) {
                    s = icet_keyframe_device_n(j.ctx, &j.sp, 1, &j.b, j.d_cnt);
                    if (s != ICET_OK) e = icet_last_error(j.ctx);
                    else if (hipEventRecord(j.done_ev, j.sk) != hipSuccess) { s = ICET_ERR_HIP; e = "hipEventRecord(keyframe build done)"; }
                }
                { std::lock_guard<std::mutex> lk(w->m); if (s != ICET_OK && w->status == ICET_OK) { w->status = s; w->err = e; } w->done++; }
                w->cv.notify_all();
            }
        });
        nd->kw = w;
        return true;
    } catch (...) { return false; }                               // no thread to be had: the caller enqueues the builds itself
}
void kf_post(icet_node* nd, const KfJob& j) { { std::lock_guard<std::mutex> lk(nd->kw->m); nd->kw->q.push_back(j); nd->kw->posted++; } nd->kw->cv.notify_all(); }
// Blocks until the helper has nothing left to enqueue; a failure of one of its jobs is reported (once) here, to whoever waits next.
icet_status kf_wait_idle(icet_node* nd) {
    if (!nd->kw) return ICET_OK;
    std::unique_lock<std::mutex> lk(nd->kw->m);
    nd->kw->cv.wait(lk, [&] { return nd->kw->done >= nd->kw->posted; });
    const icet_status s = nd->kw->status;
    if (s != ICET_OK) { nd->err = nd->kw->err; nd->kw->status = ICET_OK; nd->kw->err.clear(); }
    return s;
}
void kf_worker_stop(icet_node* nd) {
    if (!nd->kw) return;
    { std::lock_guard<std::mutex> lk(nd->kw->m); nd->kw->stop = true; }
    nd->kw->cv.notify_all();
    if (nd->kw->th.joinable()) nd->kw->th.join();
    delete nd->kw; nd->kw = nullptr;
}

// ---- the one-launch frame (round 6) ----
hipError_t filter_prologue(void* user, hipStream_t st) {          // the hook icet_register_device_n runs in front of its loop (icet_ctx_set_prologue)
    const FilterLaunch& f = *static_cast<const FilterLaunch*>(user);
    k_range_count<<<f.n_blocks, kFB, 0, st>>>(nullptr, nullptr, nullptr, 0, f.min_range, f.counts, f.fd);
    if (f.n_blocks <= 1024) {                                     // the scan folded into the scatter (every block reads at most 4 KB of counts)
        k_range_scatter<<<f.n_blocks, kFB, 0, st>>>(nullptr, nullptr, nullptr, 0, f.min_range, nullptr, f.o, f.o + f.ld_o, f.o + 2 * f.ld_o, f.fd, f.counts, f.n_blocks, f.d_cnt, f.h_cnt);
        return hipGetLastError();
    }
    k_range_scan<<<1, kFB, 0, st>>>(f.counts, f.bases, f.n_blocks, f.d_cnt, f.h_cnt);
    k_range_scatter<<<f.n_blocks, kFB, 0, st>>>(nullptr, nullptr, nullptr, 0, f.min_range, f.bases, f.o, f.o + f.ld_o, f.o + 2 * f.ld_o, f.fd);
    return hipGetLastError();
}
int64_t filter_key(const FilterLaunch& f) {            // everything the hook's launches depend on (FNV-1a): part of the loop's graph key
    const uint64_t v[] = {(uint64_t)(uintptr_t)f.fd, (uint64_t)__builtin_bit_cast(uint32_t, f.min_range), (uint64_t)(uintptr_t)f.counts, (uint64_t)(uintptr_t)f.bases, (uint64_t)f.n_blocks,
                          (uint64_t)(uintptr_t)f.d_cnt, (uint64_t)(uintptr_t)f.h_cnt, (uint64_t)(uintptr_t)f.o, (uint64_t)f.ld_o};
    uint64_t h = 1469598103934665603ull;
    for (uint64_t x : v) for (int b = 0; b < 8; b++) { h ^= (x >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
    return (int64_t)(h | 1ull);
}
// the keyframe side's own filtered copy of scan `which`, its block counters and its row counters
icet_status ensure_kf_side(icet_node* nd, int which, int64_t n) {
    if (!nd->h_done) {                                            // (the last of the fixed set: one that was refused half way is made anew, and nothing has used it)
        icet::BufferGroup& g = nd->kf_fixed;
        g.release();
        NCHK(nd, g.pinned(nd->h_frame, 2)); std::memset(nd->h_frame, 0, 2 * sizeof(FrameDesc));
        NCHK(nd, g.device(nd->d_nkept_kf, 2));
        NCHK(nd, g.pinned(nd->h_done, 1, hipHostMallocCoherent)); *nd->h_done = 0;
    }
    if (!nd->ev_f2) NCHK(nd, hipEventCreateWithFlags(&nd->ev_f2, hipEventDisableTiming));
    const icet_status s = grow_rows(nd, nd->scan_kf_mem[which], nd->d_scan_kf[which], nd->cap_scan_kf[which], n, hipDeviceSynchronize); if (s != ICET_OK) return s;
    return grow_blocks(nd, nd->blocks_kf_mem, nd->d_counts_kf, nd->d_bases_kf, nd->cap_blocks_kf, (nd->cap_scan_kf[which] + kFB * kFRows - 1) / (kFB * kFRows), hipDeviceSynchronize);
}
// a scan buffer of the node: both streams of a pipelined node may still read the old one
icet_status ensure_scan(icet_node* nd, int which, int64_t n) { return grow_rows(nd, nd->s.scan_mem[which], nd->s.d_scan[which], nd->s.cap_scan[which], n, hipDeviceSynchronize); }

// One frame with the raw scan already in HBM (column-major, ld).
icet_status push_frame(icet_node* nd, const float* d_scan, int64_t n, int64_t ld, icet_node_result* res) {
#ifdef ICET_DIAG_ENV
    static const bool trace_on = getenv("ICET_NODE_TRACE") != nullptr;
    auto now_us = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tq[6] = {0, 0, 0, 0, 0, 0}; tq[0] = now_us();
#define ICET_TR(k) do { if (trace_on) tq[k] = now_us(); } while (0)
#else
#define ICET_TR(k) do { } while (0)
#endif
    std::memset(res, 0, sizeof(*res));
    { const icet_status hs = kf_wait_idle(nd); if (hs != ICET_OK) return hs; }      // the previous frame's keyframe build has been enqueued (or says why not)
    hipStream_t st = nd->stream;
    const int cur = nd->s.prev ^ 1;
    nd->timing_valid = false;
    if (!nd->s.initialized) {
        // odometry.cpp:46-52: the first cloud is stored as it is (no range filter) and nothing is solved
        icet_status s = ensure_scan(nd, nd->s.prev, n); if (s != ICET_OK) return s;
        const int64_t l = nd->s.cap_scan[nd->s.prev];
        if (n) NCHK(nd, hipMemcpy2DAsync(nd->s.d_scan[nd->s.prev], l * sizeof(float), d_scan, ld * sizeof(float), n * sizeof(float), 3, hipMemcpyDeviceToDevice, st));
        NCHK(nd, hipStreamSynchronize(st));
        nd->s.n_scan[nd->s.prev] = n; nd->s.ld_scan[nd->s.prev] = l;
        if (nd->pipelined) {
            icet_dev_scan a{nd->s.d_scan[nd->s.prev], n, l};
            icet_params sp = nd->p.solve; sp.flags = (nd->p.flags & ICET_NODE_DOUBLE_W) ? ICET_FLAG_DOUBLE_W : ICET_FLAG_NONE;
            nd->owner = 0;
            icet_status ks = icet_keyframe_device(nd->kf[0], &sp, 1, &a);
            if (ks != ICET_OK) { nd->err = icet_last_error(nd->kf[0]); return ks; }
            NCHK(nd, hipEventRecord(nd->ev_kfdone[0], reinterpret_cast<hipStream_t>(icet_stream(nd->kf[0])))); nd->kf_built[0] = true; nd->kf_built[1] = false;
        }
        nd->s.initialized = true;
        first_result(nd->p, nd->s, n, res);
        return ICET_OK;
    }
    // ---- range filter: stable compaction into the "current" buffer (odometry.cpp:57-70) ----
    icet_status s = ensure_scan(nd, cur, n); if (s != ICET_OK) return s;
    const int64_t lcur = nd->s.cap_scan[cur];
    // Whoever needs the kept-row count on the HOST before the solve can be enqueued (the map maker's shuffle runs over exactly that many
    // indices; the aligned cloud and the unpipelined solve are sized by it) waits for the filter here.  The pipelined odometry frame does
    // not: the solve's two halves take the unfiltered row count as an upper bound for their launch geometry and read the actual count on
    // the device (icet_register_device_n / icet_keyframe_device_n), so the whole frame is enqueued without a host round trip in the middle.
    const bool fast = nd->pipelined && nd->p.map_capacity == 0 && n > 0 &&
                      !(nd->p.flags & (ICET_NODE_NO_RANGE_FILTER | ICET_NODE_ALIGNED_CLOUD | ICET_NODE_SNAIL_TRAIL));
#ifdef ICET_DIAG_ENV      /* the A/B switches of round 5's stream experiments: experiment builds only (make EXTRA=-DICET_DIAG_ENV); the shipped library never reads the environment */
    static const bool loop_on_filter_stream = getenv("ICET_NODE_LOOP_OWN_STREAM") == nullptr;
#else
    constexpr bool loop_on_filter_stream = true;
#endif
    // ... and since round 6 such a frame is ONE launch on the critical path: the loop's context captures the filter in front of its loop (one graph: the loop's first kernel
    // used to start 30-40 us after the filter's last one), and the keyframe build of this scan, on the other stream, filters the raw frame once more for itself instead of
    // waiting for this stream's filter (a dependency between two streams costs more than 20 us of duplicated filter).  ICET_NODE_TIME_PHASES keeps the phases apart.
    // The map maker's frame takes the same shape (round 6): its loop does not need the kept-row count on the host either -- only the down-sample shuffle does, and the
    // host gets the count by watching the pinned word the filter's kernel stores it into, a few microseconds into the frame, while the loop runs.
    const bool map_ok = nd->pipelined && nd->p.map_capacity > 0 && n > 0 && !(nd->p.flags & (ICET_NODE_NO_RANGE_FILTER | ICET_NODE_ALIGNED_CLOUD | ICET_NODE_SNAIL_TRAIL));
    const bool fused = (fast || map_ok) && loop_on_filter_stream && nd->p.solve.runlen > 0 && !(nd->p.flags & ICET_NODE_TIME_PHASES);
    const bool dev_count = fast || fused;                         // the solve's halves read the row count on the device
    const int n_blocks = fused ? (int)((lcur + kFB * kFRows - 1) / (kFB * kFRows)) : (int)((n + kFB * kFRows - 1) / (kFB * kFRows));      // fused: by CAPACITY (the launch does not change with n)
    s = grow_blocks(nd, nd->blocks_mem, nd->d_counts, nd->d_bases, nd->cap_blocks, n_blocks, hipDeviceSynchronize); if (s != ICET_OK) return s;
    if (fused) { s = ensure_kf_side(nd, cur, n); if (s != ICET_OK) return s; }
    int32_t* d_cnt = nd->d_nkept + cur;
    if (!fused) NCHK(nd, hipEventRecord(nd->ev[0], st));         // (the one-launch frame records no timing events: each costs the host 5-10 us IN FRONT of the launch)
    if (nd->p.flags & ICET_NODE_NO_RANGE_FILTER) {               // scanMatcher.cpp:44: the cloud goes to the constructor as it is
        if (n) NCHK(nd, hipMemcpy2DAsync(nd->s.d_scan[cur], lcur * sizeof(float), d_scan, ld * sizeof(float), n * sizeof(float), 3, hipMemcpyDeviceToDevice, st));
        *nd->h_nkept = (int32_t)n;
    } else if (fused) {
        nd->h_frame[cur] = FrameDesc{d_scan, (int32_t)n, (int32_t)ld};                          // what both filters of this frame read
        *static_cast<volatile int32_t*>(nd->h_nkept) = -1;                                      // ("not yet": the map maker's host side watches this word)
        nd->fl[cur] = FilterLaunch{nd->h_frame + cur, nd->p.min_range, nd->d_counts, nd->d_bases, n_blocks, d_cnt, nd->h_nkept, nd->s.d_scan[cur], lcur};
    } else if (n > 0) {
        const float *x = d_scan, *y = d_scan + ld, *z = d_scan + 2 * ld;
        float* o = nd->s.d_scan[cur];
        k_range_count<<<n_blocks, kFB, 0, st>>>(x, y, z, (int)n, nd->p.min_range, nd->d_counts);
        // the kept-row count goes to the host by the kernel's own store into pinned memory: a hipMemcpyAsync of four bytes costs the stream ~20 us on this part (round 5's
        // burst timeline), and the frame's other small copy -- the 48 result floats -- went the same way in round 6 (below)
        k_range_scan<<<1, kFB, 0, st>>>(nd->d_counts, nd->d_bases, n_blocks, d_cnt, nd->h_nkept);
        k_range_scatter<<<n_blocks, kFB, 0, st>>>(x, y, z, (int)n, nd->p.min_range, nd->d_bases, o, o + lcur, o + 2 * lcur);
        NCHK(nd, hipGetLastError());
        if (dev_count) NCHK(nd, hipEventRecord(nd->ev[1], st));   // what the solve streams wait for: the filtered scan
    } else {
        *nd->h_nkept = 0;
    }
    if (!dev_count) NCHK(nd, hipEventRecord(nd->ev[1], st));
    if (!dev_count) NCHK(nd, hipStreamSynchronize(st));           // the solve's launch geometry needs the row count
    // fast: an upper bound until the end-of-frame synchronisation -- the buffer's CAPACITY, which does not change from frame to frame, so that the
    // two halves of the solve see the same launch key every frame and replay their captured graphs (one hipGraphLaunch each instead of ~35 launches)
    int64_t nk = dev_count ? lcur : (int64_t)*nd->h_nkept;
    nd->s.n_scan[cur] = nk; nd->s.ld_scan[cur] = lcur;
    // ---- ICET it(prev, cur, runlen, X0, bins_phi, bins_theta, n, thresh, buff)  (odometry.cpp:76) ----
    // The down-sample indices of this frame (simpleMapMaker.cpp:147-158) depend only on the row count and on the node's RNG stream,
    // and Fisher-Yates over ~10^5 indices costs about as much host time as the solve costs device time: a helper thread shuffles
    // while this one enqueues the solve.  (The previous frame's map kernel, which read d_idx, finished before the row-count sync.)
    int m_map = 0;
    bool flip_owner = false;
    std::future<int> shuffle;
    if (nd->p.map_capacity > 0 && !fused) {
        shuffle = std::async(std::launch::async, [nd, nk]() { return draw_downsample(nd->s, nd->fast_shuffle, nd->p.map_downsample, nk); });
    }
    std::memcpy(nd->h_x0, nd->s.X0, sizeof(nd->s.X0));
    icet_dev_scan a{nd->s.d_scan[nd->s.prev], nd->s.n_scan[nd->s.prev], nd->s.ld_scan[nd->s.prev]}, b{nd->s.d_scan[cur], nk, lcur};
    icet_params sp = nd->p.solve; sp.flags = (nd->p.flags & ICET_NODE_DOUBLE_W) ? ICET_FLAG_DOUBLE_W : ICET_FLAG_NONE;
    hipStream_t so = st;                                          // the stream the result arrives on
    if (nd->pipelined) {
        // the loop against the keyframe parked one frame ago (the host has synchronised the filter's stream above), then -- behind
        // it in host order, beside it on the device -- the keyframe of THIS scan on the other context, for the next frame
        icet_ctx* own = nd->kf[nd->owner]; icet_ctx* oth = nd->kf[nd->owner ^ 1];
        hipStream_t s_own = reinterpret_cast<hipStream_t>(icet_stream(own)), s_oth = reinterpret_cast<hipStream_t>(icet_stream(oth));
        // The loop runs on the FILTER's stream: a dependency between two streams costs ~60 us on this part before the waiting queue starts (measured on the device
        // timeline: filter end -> first loop kernel), and filter -> loop -> result is the frame's critical path.  The context keeps its own stream for its keyframe
        // builds; the build this loop needs (previous frame, that stream) finished long ago as a rule -- an event says so.
        so = loop_on_filter_stream ? st : s_own;
        if (loop_on_filter_stream) {
            // (the build is done, as a rule, by the time the next frame arrives: asking costs the host a microsecond, a wait command in the stream five to ten)
            if (nd->kf_built[nd->owner] && hipEventQuery(nd->ev_kfdone[nd->owner]) != hipSuccess) { (void)hipGetLastError(); NCHK(nd, hipStreamWaitEvent(st, nd->ev_kfdone[nd->owner], 0)); }
            if (dev_count && !fused) NCHK(nd, hipStreamWaitEvent(s_oth, nd->ev[1], 0));
            icet_ctx_set_stream(own, st);
        } else if (dev_count) {                                   // nobody waited for the filter: both solve streams do
            NCHK(nd, hipStreamWaitEvent(so, nd->ev[1], 0));
            NCHK(nd, hipStreamWaitEvent(s_oth, nd->ev[1], 0));
        }
        if (!fused) NCHK(nd, hipEventRecord(nd->ev[5], so));
        // The keyframe side of a one-launch frame is enqueued by the node's HELPER thread, posted BEFORE this thread launches the loop's graph: its
        // ~45 us of enqueueing (three filter launches, an event, a graph of 18 kernels) then run beside the loop's launch and not behind it -- the build, not the loop,
        // is what the next frame waits for, and it used to start 60 us into the frame.  (Round 5, frame in phases: measured, no gain, 4.83-4.93 k frames/s with, 4.82-4.92 k
        // without.)  A failure of the build is reported by the next call that waits for the helper.
        const bool via_helper = fused && !(nd->p.flags & ICET_NODE_SERIAL_ENQUEUE) && kf_worker_start(nd);
        const int64_t lkf = fused ? nd->cap_scan_kf[cur] : 0;
        const FilterLaunch f2{nd->h_frame ? nd->h_frame + cur : nullptr, nd->p.min_range, nd->d_counts_kf, nd->d_bases_kf, (int)((lkf + kFB * kFRows - 1) / (kFB * kFRows)),
                              nd->d_nkept_kf ? nd->d_nkept_kf + cur : nullptr, nullptr, fused ? nd->d_scan_kf[cur] : nullptr, lkf};      // the other stream's own filtered copy of this scan
        if (via_helper) {
            KfJob j{oth, sp, icet_dev_scan{nd->d_scan_kf[cur], lkf, lkf}, nd->d_nkept_kf + cur, s_oth, nd->ev_kfdone[nd->owner ^ 1]};
            j.f2 = f2; j.f2_ev = nd->ev_f2;
            kf_post(nd, j); nd->kf_built[nd->owner ^ 1] = true;
        }
        // X0 is read from pinned host memory by the kernel itself (no H2D command), and k_gn_solve stores the 48 result floats of every iteration straight into pinned
        // host memory (the same pointer is valid on the device): no copy command in the frame.  (runlen 0 is a memset + copy of X0 on the device side: it keeps the
        // device buffer and its copy.)
        float* out_dev = sp.runlen > 0 ? nd->h_out : nd->d_out;
        ICET_TR(1);
        if (fused) { *static_cast<volatile int32_t*>(nd->h_done) = 0; icet_ctx_set_done_flag(own, nd->h_done); }
        if (fused) icet_ctx_set_prologue(own, filter_prologue, &nd->fl[cur], filter_key(nd->fl[cur]));        // filter + loop: one graph, one launch
        s = icet_register_device_n(own, &sp, 1, &b, dev_count ? d_cnt : nullptr, nd->h_x0, out_dev);
        if (fused) { icet_ctx_set_prologue(own, nullptr, nullptr, 0); icet_ctx_set_done_flag(own, nullptr); }
        ICET_TR(2);
        icet_ctx_set_stream(own, s_own);
        if (s != ICET_OK) { nd->err = icet_last_error(own); if (via_helper) (void)kf_wait_idle(nd); return s; }
        if (out_dev != nd->h_out) NCHK(nd, hipMemcpyAsync(nd->h_out, nd->d_out, sizeof(float) * 48, hipMemcpyDeviceToHost, so));
        if (!fused) NCHK(nd, hipEventRecord(nd->ev[2], so));
        if (!via_helper) {
            if (fused) {
                // (the same kept rows in the same order: the same keyframe bits), then the build from it
                NCHK(nd, filter_prologue(const_cast<FilterLaunch*>(&f2), s_oth));
                NCHK(nd, hipEventRecord(nd->ev_f2, s_oth));       // the caller's frame has been read (waited for before this push returns)
                icet_dev_scan bk{nd->d_scan_kf[cur], lkf, lkf};
                s = icet_keyframe_device_n(oth, &sp, 1, &bk, nd->d_nkept_kf + cur);
            } else {
                s = icet_keyframe_device_n(oth, &sp, 1, &b, dev_count ? d_cnt : nullptr);
            }
            if (s != ICET_OK) { nd->err = icet_last_error(oth); return s; }
            NCHK(nd, hipEventRecord(nd->ev_kfdone[nd->owner ^ 1], s_oth)); nd->kf_built[nd->owner ^ 1] = true;
        }
        flip_owner = true;                                        // committed together with nd->s.prev once the frame has succeeded
    } else {
        float* out_dev = sp.runlen > 0 ? nd->h_out : nd->d_out;
        s = icet_solve_batch_device(nd->ctx, &sp, 1, &a, &b, nd->h_x0, out_dev);
        if (s != ICET_OK) { nd->err = icet_last_error(nd->ctx); return s; }
        if (out_dev != nd->h_out) NCHK(nd, hipMemcpyAsync(nd->h_out, nd->d_out, sizeof(float) * 48, hipMemcpyDeviceToHost, st));
        NCHK(nd, hipEventRecord(nd->ev[2], st));
    }
    if (fused && nd->p.map_capacity > 0) {
        // the frame is in flight; its filter's count lands in pinned memory ~25 us in (k_range_scan's own store), the loop runs for another ~230: the down-sample
        // shuffle (simpleMapMaker.cpp:147-158: std::shuffle over exactly that many indices with the node's RNG stream) runs here, on this thread, beside it
        volatile int32_t* hc = nd->h_nkept;
        s = wait_pinned(nd, [hc] { return *hc >= 0; }, st, 4095, "the range filter's row count did not arrive");
        if (s != ICET_OK) { if (nd->kw) (void)kf_wait_idle(nd); return s; }
        m_map = draw_downsample(nd->s, nd->fast_shuffle, nd->p.map_downsample, (int64_t)*hc);      // into pinned h_idx: the map kernel reads it in place (no copy command)
    }
    if (shuffle.valid()) {
        m_map = shuffle.get();
        if (m_map) NCHK(nd, hipMemcpyAsync(nd->d_idx, nd->s.h_idx, sizeof(int32_t) * m_map, hipMemcpyHostToDevice, st));
    }
    ICET_TR(3);
    if (so != st) NCHK(nd, hipStreamSynchronize(so));
    if (fused) {
        // the frame's last kernel stores its 48 result floats and then a 1 into pinned host memory: this thread watches that word -- hipStreamSynchronize answers
        // several microseconds after the queue has drained -- and asks the stream only now and then (a frame that failed never writes the word)
        volatile int32_t* hd = nd->h_done;
        s = wait_pinned(nd, [hd] { return *hd != 0; }, st, 8191, "the frame's result did not arrive");
        if (s != ICET_OK) { if (nd->kw) (void)kf_wait_idle(nd); return s; }
    } else NCHK(nd, hipStreamSynchronize(st));
    ICET_TR(4);
    if (fused) {                                                  // the caller's frame may be released when this returns: the other stream's filter has read it (long done: it started beside this stream's)
        const icet_status hs = kf_wait_idle(nd); if (hs != ICET_OK) return hs;      // (the helper has recorded the event)
        NCHK(nd, hipEventSynchronize(nd->ev_f2));
    }
    if (dev_count) { nk = *nd->h_nkept; nd->s.n_scan[cur] = nk; }   // the filter's count has arrived with everything else
    // ---- the tail (frame_tail): guard, map queue, aligned cloud, snail trail, pose ----
    nd->timed_map = false;
    auto map_dev = [&](const float* X, const float* Ri, int64_t pos, int m) -> icet_status {
        const int cap = nd->p.map_capacity;
        float* q = nd->s.d_map; const float* sc = nd->s.d_scan[cur];
        const int blocks = std::min((cap + 255) / 256, 256 * 8);
        if (!fused) NCHK(nd, hipEventRecord(nd->ev[4], st));
        k_map_add_scan<<<blocks, 256, 0, st>>>(q, q + cap, q + 2 * (size_t)cap, cap, (int)pos, m, sc, sc + lcur, sc + 2 * lcur, fused ? nd->s.h_idx : nd->d_idx,
                                               X[0], X[1], X[2], Ri[0], Ri[1], Ri[2], Ri[3], Ri[4], Ri[5], Ri[6], Ri[7], Ri[8]);
        NCHK(nd, hipGetLastError());
        if (!fused) NCHK(nd, hipEventRecord(nd->ev[3], st));      // not waited for: the next push (or icet_node_map) synchronises the stream
        nd->timed_map = !fused;
        return ICET_OK;
    };
    auto align_dev = [&](const float* X, const float* Ri) -> icet_status {
        if (lcur > nd->s.cap_aligned) {
            NCHK(nd, hipStreamSynchronize(st));
            NCHK(nd, icet::grow(nd->s.aligned_mem, nd->s.cap_aligned, lcur, [&] { return nd->s.aligned_mem.device(nd->s.d_aligned, 3 * (size_t)lcur); }));
        }
        const float* sc = nd->s.d_scan[cur]; float* o = nd->s.d_aligned; const int64_t la = nd->s.cap_aligned;
        if (nk) k_align_cloud<<<(int)std::min<int64_t>((nk + 255) / 256, 2048), 256, 0, st>>>(sc, sc + lcur, sc + 2 * lcur, (int)nk, o, o + la, o + 2 * la, X[0], X[1], X[2],
                                                                                           Ri[0], Ri[1], Ri[2], Ri[3], Ri[4], Ri[5], Ri[6], Ri[7], Ri[8]);
        NCHK(nd, hipGetLastError());
        nd->s.n_aligned = nk; nd->s.ld_aligned = la;
        return ICET_OK;
    };
    s = frame_tail(nd->p, nd->s, nd->h_out, nk, m_map, res, map_dev, align_dev);
    if (s != ICET_OK) return s;
    nd->s.prev = cur;                                               // prev_pcl_matrix = pcl_matrix (odometry.cpp:88)
    if (flip_owner) nd->owner ^= 1;                               // ... and the keyframe parked for it becomes the one the next frame registers against
    nd->timing_valid = !fused;
#ifdef ICET_DIAG_ENV
    if (trace_on && tq[1] > 0) { tq[5] = now_us(); if (++nd->tr_seen > 6) { for (int k = 0; k < 5; k++) nd->tr[k] += tq[k + 1] - tq[k]; nd->tr_n++; } }      // (steady state: the first frames capture their graphs)
#endif
    return ICET_OK;
}
#undef ICET_TR


// No exception crosses the C ABI (no_throw), and
// a frame that fails half way must not leave the node's idea of "previous scan" and the parked keyframe disagreeing: on ANY failure
// the device is drained and the node drops back to "no previous scan" -- the next cloud is stored like the first one
// (odometry.cpp:46-52) and the pose chain continues from where it was.
icet_status push_device(icet_node* nd, const float* d_scan, int64_t n, int64_t ld, icet_node_result* res) {
    const bool was_initialized = nd->s.initialized;
    const icet_status s = no_throw(nd->err, [&] { return push_frame(nd, d_scan, n, ld, res); });
    if (s != ICET_OK && was_initialized) {
        (void)kf_wait_idle(nd);
        (void)hipDeviceSynchronize();
        nd->s.initialized = false; nd->timing_valid = false;
    }
    return s;
}

}  // namespace

extern "C" {

icet_status icet_node_create(icet_ctx* ctx, const icet_node_params* p, icet_node** out) {
    if (!out) return ICET_ERR_BAD_ARG;
    *out = nullptr;
    if (!node_params_ok(ctx, p)) return ICET_ERR_BAD_ARG;
    icet_node* nd = new (std::nothrow) icet_node();
    if (!nd) return ICET_ERR_NOMEM;
    nd->ctx = ctx; nd->p = *p; nd->stream = reinterpret_cast<hipStream_t>(icet_stream(ctx)); nd->device = icet_device(ctx);
    auto fail = [&](icet_status s) { icet_node_destroy(nd); return s; };
    if (hipSetDevice(nd->device) != hipSuccess) return fail(ICET_ERR_NO_DEVICE);
    icet::BufferGroup& m = nd->fixed;
    if (m.device(nd->d_nkept, 2) || m.pinned(nd->h_nkept, 1, hipHostMallocCoherent) || m.device(nd->d_x0, 6) || m.device(nd->d_out, 48) ||
        m.pinned(nd->h_out, 48, hipHostMallocCoherent) || m.pinned(nd->h_x0, 6))
        return fail(ICET_ERR_NOMEM);
    if (p->map_capacity > 0) nd->fast_shuffle = fast_shuffle_ok();
    for (hipEvent_t& e : nd->ev) if (hipEventCreate(&e) != hipSuccess) return fail(ICET_ERR_HIP);
    for (hipEvent_t& e : nd->ev_kfdone) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(ICET_ERR_HIP);
    if (!(p->flags & ICET_NODE_NO_PIPELINE)) {
        for (icet_ctx*& k : nd->kf) { icet_status cs = icet_create(&k, nd->device, nullptr); if (cs != ICET_OK) return fail(cs); }
        nd->pipelined = true;
    }
    { const icet_status ss = stream_create(*p, nd->s); if (ss != ICET_OK) return fail(ss); }
    if (p->map_capacity > 0 && m.device(nd->d_idx, (size_t)std::max(p->map_downsample, 1)) != 0) return fail(ICET_ERR_NOMEM);
    *out = nd;
    return ICET_OK;
}

icet_status icet_node_destroy(icet_node* nd) {
    if (!nd) return ICET_ERR_BAD_ARG;
#ifdef ICET_DIAG_ENV
    if (nd->tr_n) std::fprintf(stderr, "push_frame host us over %ld frames: to-register %.1f | register (loop graph launch) %.1f | keyframe side enqueue %.1f | synchronize %.1f | tail %.1f\n", nd->tr_n,
                               nd->tr[0] / nd->tr_n, nd->tr[1] / nd->tr_n, nd->tr[2] / nd->tr_n, nd->tr[3] / nd->tr_n, nd->tr[4] / nd->tr_n);
#endif
    kf_worker_stop(nd);                      // (drains what it still has to enqueue, then joins)
    (void)hipSetDevice(nd->device);
    (void)hipDeviceSynchronize();            // not the borrowed stream: the context may already be gone
    for (hipEvent_t e : nd->ev) if (e) (void)hipEventDestroy(e);
    if (nd->ev_f2) (void)hipEventDestroy(nd->ev_f2);
    for (hipEvent_t e : nd->ev_kfdone) if (e) (void)hipEventDestroy(e);
    for (icet_ctx* k : nd->kf) if (k) (void)icet_destroy(k);
    delete nd;                               // (its buffer groups and the stream's free here: behind the synchronisation, with the node's device current)
    return ICET_OK;
}

const char* icet_node_last_error(const icet_node* nd) { return nd ? nd->err.c_str() : ""; }

icet_status icet_node_push_device(icet_node* nd, const float* d_scan, int64_t n, int64_t ld, icet_node_result* res) {
    if (!nd || !res || n < 0 || ld < n || (n > 0 && !d_scan) || n >= ((int64_t)1 << 30)) return ICET_ERR_BAD_ARG;
    if (hipSetDevice(nd->device) != hipSuccess) return ICET_ERR_NO_DEVICE;
    return push_device(nd, d_scan, n, ld, res);
}

icet_status icet_node_push_many_device(icet_node* nd, const icet_dev_scan* frames, int32_t n_frames, icet_node_result* results) {
    if (!nd || n_frames < 0 || (n_frames > 0 && (!frames || !results))) return ICET_ERR_BAD_ARG;
    for (int k = 0; k < n_frames; k++)
        if (frames[k].n < 0 || frames[k].ld < frames[k].n || (frames[k].n > 0 && !frames[k].ptr) || frames[k].n >= ((int64_t)1 << 30)) return ICET_ERR_BAD_ARG;
    if (hipSetDevice(nd->device) != hipSuccess) return ICET_ERR_NO_DEVICE;
    { const icet_status hs = kf_wait_idle(nd); if (hs != ICET_OK) { (void)hipDeviceSynchronize(); nd->s.initialized = false; return hs; } }
    // Rounds 4-5 chained a burst's frames on the device (X0 <- X device to device, results parked in HBM, one copy at the end).  That needs two hand-overs between
    // streams per frame -- the build of frame k waits for the loop of frame k - 1 to let go of the context's tables, the loop of frame k + 1 for that build -- at 30 to
    // 60 us each on this part, and ran at 4.0 - 4.7 k frames/s; since a frame is one graph launch (push_frame, round 6) the host in the loop costs ~25 us and frame by
    // frame runs at 5.0 - 5.2 k.  The burst entry is therefore a loop over frames (no Python / FFI call per frame for the caller: that is what it still saves).
    for (int k = 0; k < n_frames; k++) { const icet_status s = push_device(nd, frames[k].ptr, frames[k].n, frames[k].ld, &results[k]); if (s != ICET_OK) return s; }
    return ICET_OK;
}

icet_status icet_node_push(icet_node* nd, const float* scan, int64_t n, int64_t ld, icet_node_result* res) {
    if (!nd || !res || n < 0 || ld < n || (n > 0 && !scan) || n >= ((int64_t)1 << 30)) return ICET_ERR_BAD_ARG;
    if (hipSetDevice(nd->device) != hipSuccess) return ICET_ERR_NO_DEVICE;
    const int64_t l = (n + 63) / 64 * 64;
    if (3 * l > nd->cap_stage) {
        NCHK(nd, hipStreamSynchronize(nd->stream));
        NCHK(nd, icet::grow(nd->stage_mem, nd->cap_stage, 3 * (l + l / 8), [&] { return nd->stage_mem.device(nd->d_stage, 3 * (size_t)(l + l / 8)); }));
    }
    if (n) NCHK(nd, hipMemcpy2DAsync(nd->d_stage, l * sizeof(float), scan, ld * sizeof(float), n * sizeof(float), 3, hipMemcpyHostToDevice, nd->stream));
    return push_device(nd, nd->d_stage, n, l, res);
}

// (stream_rows_out; whatever the helper thread still has to enqueue goes first)
icet_status icet_node_map(icet_node* nd, float* out, int64_t ld, int64_t* rows_out) {
    if (!nd || !rows_out) return ICET_ERR_BAD_ARG;
    (void)kf_wait_idle(nd);
    return stream_rows_out(nd, nd->s, kRowsMap, false, out, ld, rows_out);
}

icet_status icet_node_prev_scan(icet_node* nd, float* out, int64_t ld, int64_t* rows_out) {
    if (!nd || !rows_out) return ICET_ERR_BAD_ARG;
    (void)kf_wait_idle(nd);
    return stream_rows_out(nd, nd->s, kRowsPrevScan, false, out, ld, rows_out);
}

icet_status icet_node_aligned(icet_node* nd, float* out, int64_t ld, int64_t* rows_out) {
    if (!nd || !rows_out) return ICET_ERR_BAD_ARG;
    (void)kf_wait_idle(nd);
    return stream_rows_out(nd, nd->s, kRowsAligned, false, out, ld, rows_out);
}

icet_status icet_node_snail_trail(icet_node* nd, float* out, int64_t ld, int64_t* rows_out) {
    if (!nd || !rows_out) return ICET_ERR_BAD_ARG;
    return stream_rows_out(nd, nd->s, kRowsSnail, false, out, ld, rows_out);
}

icet_status icet_node_last_timing(icet_node* nd, float out_ms[3]) {
    if (!nd || !out_ms) return ICET_ERR_BAD_ARG;
    if (!nd->timing_valid) return ICET_ERR_BAD_ARG;
    float a = 0, b = 0, c = 0;
    NCHK(nd, hipEventElapsedTime(&a, nd->ev[0], nd->ev[1]));
    NCHK(nd, hipEventElapsedTime(&b, nd->pipelined ? nd->ev[5] : nd->ev[1], nd->ev[2]));
    if (nd->timed_map) { NCHK(nd, hipEventSynchronize(nd->ev[3])); NCHK(nd, hipEventElapsedTime(&c, nd->ev[4], nd->ev[3])); }
    out_ms[0] = a; out_ms[1] = b; out_ms[2] = c;
    return ICET_OK;
}

// Test hook, host only: the body frame_tail calls (node_tail_scalars), on the caller's X and pose
icet_status icet_debug_node_tail(const float X[6], const float pose_in[16], float R[9], float Rinv[9], float pose_out[16], float quat[4]) {
    if (!X || !pose_in || !R || !Rinv || !pose_out || !quat) return ICET_ERR_BAD_ARG;
    float P[16];                                                  // (pose_out may be pose_in)
    node_tail_scalars(X, pose_in, R, Rinv, P, quat);
    std::memcpy(pose_out, P, sizeof(P));
    return ICET_OK;
}

}  // extern "C"

// ==================================================================================================================================================================
// Node groups (include/icet_nodes.h, icet_node_group_*): S independent streams that share one icet_node_params, advanced together.  A frame of one stream needs the
// previous frame's X, so one stream is bound by the launch chain of its frame (DESIGN.md sections 10-11); a call of the group carries one frame for each of any
// subset of its streams and pays that chain once:
//   k_group_count / k_group_scan / k_group_scatter   the range filter of every frame of the call -- ragged: a per-call table (the kernels' argument, no copy
//                                                    command) gives each frame its source, rows, destination and first block; first frames and
//                                                    ICET_NODE_NO_RANGE_FILTER streams keep every row (a copy through the same kernels)
//   icet_keyframe_device_n + icet_register_device_n   ONE keyframe build over the named streams' stored previous scans and ONE Gauss-Newton loop over their
//                                                    filtered frames (the raw row counts are the launch bounds, the filter's device-side counts the rows)
//   k_group_map_add_scan                             EigenQueue::add_new_scan of every map-maker stream of the call, one launch
//   k_group_align_cloud                              scan2_in_scan1_frame of every stream of the call
// These five are the second LAUNCH FORM of the row passes at the top of this file, not a second statement of them: each finds its frame (ring, cloud) in the table and
// calls the body the node's kernel calls (count_block, scan_block_counts, scatter_rank / scatter_store, ring_add_scan_row, align_row).  The host state per stream is the
// node's StreamState, its tail the node's frame_tail.  A pair's result does not depend on the batch it is solved in, so every stream gets the
// bits of its own icet_node.
// ==================================================================================================================================================================
namespace {

constexpr int kGroupMaxFrames = 64;          // frames per filter launch: the table is the kernels' argument (kernarg), ~2.3 KB
constexpr int kGroupMaxRings = 32;           // rings / clouds per map or aligned-cloud launch, ~2.8 KB of kernarg
constexpr int kGroupMaxThreads = 16;         // the down-sample draws: this thread and at most 15 helpers, whatever the host's core count

struct GFrame { const float* x; float* o; int32_t n, ld, ldo, keep_all; };      // keep_all: a copy (first frame, ICET_NODE_NO_RANGE_FILTER)
struct GFilterArgs { int32_t n_frames; float min_range; int32_t blk_off[kGroupMaxFrames + 1]; GFrame f[kGroupMaxFrames]; };
struct GRing { float* q; const float* s; const int32_t* idx; int32_t pos, m, lds; RowMove T; };
struct GMapArgs { int32_t n_rings, cap; GRing r[kGroupMaxRings]; };
struct GAlign { const float* s; float* o; int32_t n, lds, ldo; RowMove T; };
struct GAlignArgs { int32_t n; GAlign a[kGroupMaxRings]; };

// the frame that owns block b: the last k with blk_off[k] <= b (a frame without rows owns no block)
__device__ __forceinline__ int group_frame_of(const GFilterArgs& a, int b) {
    int lo = 0, hi = a.n_frames - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.blk_off[mid] <= b) lo = mid; else hi = mid - 1; }
    return lo;
}

// ---- the group's launch form of the row passes: the frame that owns the block (or blockIdx.y's ring / cloud) gives the pointers, the row base and keep_all ----
__global__ __launch_bounds__(kFB) void k_group_count(const GFilterArgs a, int32_t* __restrict__ counts) {
    const int k = group_frame_of(a, blockIdx.x);
    const GFrame f = a.f[k];
    count_block(f.x, f.x + f.ld, f.x + 2 * (size_t)f.ld, f.n, (blockIdx.x - a.blk_off[k]) * kFB * kFRows, f.keep_all, a.min_range, counts + blockIdx.x);
}

// one block per frame; the total is the frame's row count, to the device (the solve's d_rows) and to pinned host memory (the map maker's down-sample draw watches it)
__global__ __launch_bounds__(kFB) void k_group_scan(const GFilterArgs a, const int32_t* __restrict__ counts, int32_t* __restrict__ bases, int32_t* __restrict__ rows, int32_t* __restrict__ h_rows) {
    const int k = blockIdx.x, b0 = a.blk_off[k];
    scan_block_counts(counts + b0, bases + b0, a.blk_off[k + 1] - b0, rows + k, h_rows + k);
}

__global__ __launch_bounds__(kFB) void k_group_scatter(const GFilterArgs a, const int32_t* __restrict__ bases) {
    __shared__ ScatterCounts wcnt;
    const int k = group_frame_of(a, blockIdx.x);
    const GFrame f = a.f[k];
    ScatterRows r;
    scatter_rank(f.x, f.x + f.ld, f.x + 2 * (size_t)f.ld, f.n, (blockIdx.x - a.blk_off[k]) * kFB * kFRows, f.keep_all, a.min_range, r, wcnt);
    __syncthreads();
    scatter_store(r, wcnt, bases[blockIdx.x], f.o, f.o + f.ldo, f.o + 2 * (size_t)f.ldo);
}

__global__ __launch_bounds__(256) void k_group_map_add_scan(const GMapArgs a) {
    const GRing& g = a.r[blockIdx.y];
    const RowMove T = g.T;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.cap; i += gridDim.x * blockDim.x)
        ring_add_scan_row(i, g.q, g.q + a.cap, g.q + 2 * (size_t)a.cap, a.cap, g.pos, g.m, g.s, g.s + g.lds, g.s + 2 * (size_t)g.lds, g.idx, T);
}

__global__ __launch_bounds__(256) void k_group_align_cloud(const GAlignArgs a) {
    const GAlign& g = a.a[blockIdx.y];
    const RowMove T = g.T;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += gridDim.x * blockDim.x)
        align_row(i, g.s, g.s + g.lds, g.s + 2 * (size_t)g.lds, g.o, g.o + g.ldo, g.o + 2 * (size_t)g.ldo, T);
}

// f(0) .. f(n - 1) on the calling thread and up to kGroupMaxThreads - 1 persistent helpers; returns when all have run (the first exception is rethrown here)
class DrawPool {
public:
    ~DrawPool() {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cv_.notify_all();
        for (std::thread& t : th_) if (t.joinable()) t.join();
    }
    void run(int n, const std::function<void(int)>& f) {
        if (n <= 0) return;
        const int want = std::min(n, kGroupMaxThreads) - 1;
        while ((int)th_.size() < want) th_.emplace_back([this] { loop(); });
        { std::lock_guard<std::mutex> lk(m_); f_ = &f; n_ = n; next_ = 0; done_ = 0; err_ = nullptr; gen_++; }
        cv_.notify_all();
        work();
        std::exception_ptr e;
        { std::unique_lock<std::mutex> lk(m_); cv_done_.wait(lk, [&] { return done_ == n_; }); f_ = nullptr; e = err_; err_ = nullptr; }
        if (e) std::rethrow_exception(e);
    }
private:
    void work() {
        for (;;) {
            int i; const std::function<void(int)>* f;
            { std::lock_guard<std::mutex> lk(m_); if (!f_ || next_ >= n_) return; i = next_++; f = f_; }
            try { (*f)(i); } catch (...) { std::lock_guard<std::mutex> lk(m_); if (!err_) err_ = std::current_exception(); }
            bool last; { std::lock_guard<std::mutex> lk(m_); last = ++done_ == n_; }
            if (last) cv_done_.notify_all();
        }
    }
    void loop() {
        long seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [&] { return stop_ || gen_ != seen; }); if (stop_) return; seen = gen_; }
            work();
        }
    }
    std::vector<std::thread> th_; std::mutex m_; std::condition_variable cv_, cv_done_;
    const std::function<void(int)>* f_ = nullptr; int n_ = 0, next_ = 0, done_ = 0; long gen_ = 0; bool stop_ = false; std::exception_ptr err_;
};

}  // namespace

struct icet_node_group {
    icet_ctx* ctx = nullptr; hipStream_t stream = nullptr; int device = 0;
    icet_node_params p{};
    std::string err;
    int32_t n_streams = 0;
    bool fast_shuffle = false;
    std::unique_ptr<StreamState[]> s;                            // n_streams of them, made once: a stream's buffer groups hold the addresses of its pointers
    // per-call tables, by position in the call (the solved frames first): row counts on the device and pinned, X0 and results pinned, results on the device (runlen 0)
    int32_t* d_rows = nullptr; int32_t* h_rows = nullptr; float* h_x0 = nullptr; float* h_out = nullptr; float* d_out = nullptr;
    int32_t* d_counts = nullptr; int32_t* d_bases = nullptr; int64_t cap_blocks = 0;     // the ragged filter's block counts / bases
    icet::BufferGroup fixed, blocks_mem;                         // owners: the per-call tables (creation); d_counts + d_bases
    DrawPool* pool = nullptr;
};

namespace {

icet_status group_push_frames(icet_node_group* g, int32_t n, const int32_t* ids, const icet_dev_scan* frames, icet_node_result* results) {
    for (int i = 0; i < n; i++) std::memset(&results[i], 0, sizeof(icet_node_result));
    hipStream_t hs = g->stream;
    const icet_node_params& p = g->p;
    // the call's order: the frames that are solved (their stream has a previous scan) first -- positions 0 .. K-1 of the row counts are the loop's d_rows --, then first frames
    std::vector<int> order; order.reserve((size_t)n);
    for (int i = 0; i < n; i++) if (g->s[(size_t)ids[i]].initialized) order.push_back(i);
    const int K = (int)order.size();
    for (int i = 0; i < n; i++) if (!g->s[(size_t)ids[i]].initialized) order.push_back(i);
    // ---- buffers: a solved frame goes to its stream's other buffer, a first frame to the "previous" one ----
    auto drain = [hs] { return hipStreamSynchronize(hs); };      // everything of this group runs on one stream
    int64_t total_blocks = 0;
    for (int j = 0; j < n; j++) {
        const int i = order[(size_t)j]; StreamState& st = g->s[(size_t)ids[i]];
        const int to = j < K ? (st.prev ^ 1) : st.prev;
        icet_status s = grow_rows(g, st.scan_mem[to], st.d_scan[to], st.cap_scan[to], frames[i].n, drain); if (s != ICET_OK) return s;
        if (j < K && (p.flags & ICET_NODE_ALIGNED_CLOUD)) { s = grow_rows(g, st.aligned_mem, st.d_aligned, st.cap_aligned, st.cap_scan[to], drain); if (s != ICET_OK) return s; }
        total_blocks += (frames[i].n + kFB * kFRows - 1) / (kFB * kFRows);
    }
    { const icet_status s = grow_blocks(g, g->blocks_mem, g->d_counts, g->d_bases, g->cap_blocks, total_blocks, drain); if (s != ICET_OK) return s; }
    // ---- the range filter of every frame (odometry.cpp:57-70), kGroupMaxFrames frames per launch triple ----
    for (int j = 0; j < n; j++) static_cast<volatile int32_t*>(g->h_rows)[j] = -1;                // ("not yet": watched below)
    int64_t blk0 = 0;
    for (int j0 = 0; j0 < n; j0 += kGroupMaxFrames) {
        GFilterArgs a{};
        a.n_frames = std::min(kGroupMaxFrames, n - j0); a.min_range = p.min_range;
        int32_t nb = 0;
        for (int f = 0; f < a.n_frames; f++) {
            const int j = j0 + f, i = order[(size_t)j]; const StreamState& st = g->s[(size_t)ids[i]];
            const int to = j < K ? (st.prev ^ 1) : st.prev;
            a.blk_off[f] = nb;
            a.f[f] = GFrame{frames[i].ptr, st.d_scan[to], (int32_t)frames[i].n, (int32_t)frames[i].ld, (int32_t)st.cap_scan[to],
                            (j >= K || (p.flags & ICET_NODE_NO_RANGE_FILTER)) ? 1 : 0};
            nb += (int32_t)((frames[i].n + kFB * kFRows - 1) / (kFB * kFRows));
        }
        a.blk_off[a.n_frames] = nb;
        int32_t* counts = g->d_counts + blk0; int32_t* bases = g->d_bases + blk0;
        if (nb) k_group_count<<<nb, kFB, 0, hs>>>(a, counts);
        k_group_scan<<<a.n_frames, kFB, 0, hs>>>(a, counts, bases, g->d_rows + j0, g->h_rows + j0);
        if (nb) k_group_scatter<<<nb, kFB, 0, hs>>>(a, bases);
        NCHK(g, hipGetLastError());
        blk0 += nb;
    }
    // ---- ONE keyframe build over the stored previous scans, ONE loop over the filtered frames ----
    icet_params sp = p.solve; sp.flags = (p.flags & ICET_NODE_DOUBLE_W) ? ICET_FLAG_DOUBLE_W : ICET_FLAG_NONE;
    float* out_dev = sp.runlen > 0 ? g->h_out : g->d_out;        // (the loop stores its results straight into pinned memory; runlen 0 is a copy on the device)
    if (K > 0) {
        std::vector<icet_dev_scan> a((size_t)K), b((size_t)K);
        for (int j = 0; j < K; j++) {
            const int i = order[(size_t)j]; const StreamState& st = g->s[(size_t)ids[i]];
            const int cur = st.prev ^ 1;
            a[(size_t)j] = icet_dev_scan{st.d_scan[st.prev], st.n_scan[st.prev], st.ld_scan[st.prev]};
            b[(size_t)j] = icet_dev_scan{st.d_scan[cur], frames[i].n, st.cap_scan[cur]};           // the raw rows: an upper bound; the filter's count is d_rows[j]
            std::memcpy(g->h_x0 + 6 * (size_t)j, st.X0, sizeof(st.X0));
        }
        icet_status s = icet_keyframe_device_n(g->ctx, &sp, K, a.data(), nullptr);
        if (s == ICET_OK) s = icet_register_device_n(g->ctx, &sp, K, b.data(), g->d_rows, g->h_x0, out_dev);
        if (s != ICET_OK) { g->err = icet_last_error(g->ctx); return s; }
        if (out_dev != g->h_out) NCHK(g, hipMemcpyAsync(g->h_out, g->d_out, sizeof(float) * 48 * (size_t)K, hipMemcpyDeviceToHost, hs));
    }
    // ---- the map maker's down-sample draws (simpleMapMaker.cpp:147-158), each over exactly its frame's kept rows: the counts land in pinned memory early in the
    // call, the draws run on the pool while the loop iterates ----
    std::vector<int> m_map((size_t)K, 0);
    if (p.map_capacity > 0 && K > 0) {
        volatile int32_t* hr = g->h_rows;
        const icet_status s = wait_pinned(g, [&] { for (int j = 0; j < K; j++) if (hr[j] < 0) return false; return true; }, hs, 4095, "the range filter's row counts did not arrive");
        if (s != ICET_OK) return s;
        const bool fast = g->fast_shuffle;
        g->pool->run(K, [&](int j) {
            StreamState& st = g->s[(size_t)ids[order[(size_t)j]]];
            m_map[(size_t)j] = draw_downsample(st, fast, p.map_downsample, (int64_t)hr[j]);
        });
    }
    NCHK(g, hipStreamSynchronize(hs));
    // ---- the tails, stream by stream (frame_tail: the node's own), then the batched map and aligned-cloud launches ----
    std::vector<GRing> rings; std::vector<GAlign> clouds;
    for (int j = 0; j < K; j++) {
        const int i = order[(size_t)j]; StreamState& st = g->s[(size_t)ids[i]];
        const int cur = st.prev ^ 1;
        const int64_t nk = g->h_rows[j];
        st.n_scan[cur] = nk; st.ld_scan[cur] = st.cap_scan[cur];
        auto map_dev = [&](const float* X, const float* Ri, int64_t pos, int m) -> icet_status {
            rings.push_back(GRing{st.d_map, st.d_scan[cur], st.h_idx, (int32_t)pos, m, (int32_t)st.cap_scan[cur], row_move(X, Ri)});
            return ICET_OK;
        };
        auto align_dev = [&](const float* X, const float* Ri) -> icet_status {
            if (nk) clouds.push_back(GAlign{st.d_scan[cur], st.d_aligned, (int32_t)nk, (int32_t)st.cap_scan[cur], (int32_t)st.cap_aligned, row_move(X, Ri)});
            st.n_aligned = nk; st.ld_aligned = st.cap_aligned;
            return ICET_OK;
        };
        const icet_status s = frame_tail(p, st, g->h_out + 48 * (size_t)j, nk, m_map[(size_t)j], &results[i], map_dev, align_dev);
        if (s != ICET_OK) return s;
        st.prev = cur;                                            // prev_pcl_matrix = pcl_matrix (odometry.cpp:88)
    }
    for (int j = K; j < n; j++) {
        const int i = order[(size_t)j]; StreamState& st = g->s[(size_t)ids[i]];
        st.n_scan[st.prev] = frames[i].n; st.ld_scan[st.prev] = st.cap_scan[st.prev];
        st.initialized = true;
        first_result(p, st, frames[i].n, &results[i]);
    }
    for (size_t r0 = 0; r0 < rings.size(); r0 += kGroupMaxRings) {
        GMapArgs a{}; a.n_rings = (int32_t)std::min<size_t>(kGroupMaxRings, rings.size() - r0); a.cap = p.map_capacity;
        for (int r = 0; r < a.n_rings; r++) a.r[r] = rings[r0 + (size_t)r];
        k_group_map_add_scan<<<dim3(std::min((p.map_capacity + 255) / 256, 2048), a.n_rings), 256, 0, hs>>>(a);
        NCHK(g, hipGetLastError());                               // not waited for: the next call (or an accessor) runs behind it on the same stream
    }
    for (size_t c0 = 0; c0 < clouds.size(); c0 += kGroupMaxRings) {
        GAlignArgs a{}; a.n = (int32_t)std::min<size_t>(kGroupMaxRings, clouds.size() - c0);
        int64_t most = 0;
        for (int c = 0; c < a.n; c++) { a.a[c] = clouds[c0 + (size_t)c]; most = std::max<int64_t>(most, a.a[c].n); }
        k_group_align_cloud<<<dim3((unsigned)std::min<int64_t>((most + 255) / 256, 2048), a.n), 256, 0, hs>>>(a);
        NCHK(g, hipGetLastError());
    }
    return ICET_OK;
}

// As push_device for one node: no exception crosses the C ABI (no_throw), and a call that fails after it has started drains the stream and drops every stream it named back to
// "no previous scan" (their next frame is stored like a first one; the pose chain continues)
icet_status group_push(icet_node_group* g, int32_t n, const int32_t* ids, const icet_dev_scan* frames, icet_node_result* results) {
    const icet_status s = no_throw(g->err, [&] { return group_push_frames(g, n, ids, frames, results); });
    if (s != ICET_OK) {
        (void)hipStreamSynchronize(g->stream);
        (void)hipGetLastError();
        for (int i = 0; i < n; i++) g->s[(size_t)ids[i]].initialized = false;
    }
    return s;
}

}  // namespace

extern "C" {

icet_status icet_node_group_create(icet_ctx* ctx, const icet_node_params* p, int32_t n_streams, icet_node_group** out) {
    if (!out) return ICET_ERR_BAD_ARG;
    *out = nullptr;
    if (!node_params_ok(ctx, p) || n_streams <= 0) return ICET_ERR_BAD_ARG;
    icet_node_group* g = new (std::nothrow) icet_node_group();
    if (!g) return ICET_ERR_NOMEM;
    auto fail = [&](icet_status s) { icet_node_group_destroy(g); return s; };
    try {
        g->ctx = ctx; g->p = *p; g->n_streams = n_streams; g->stream = reinterpret_cast<hipStream_t>(icet_stream(ctx)); g->device = icet_device(ctx);
        g->s.reset(new StreamState[(size_t)n_streams]);
        g->pool = new DrawPool();
    } catch (...) { return fail(ICET_ERR_NOMEM); }
    if (hipSetDevice(g->device) != hipSuccess) return fail(ICET_ERR_NO_DEVICE);
    const size_t S = (size_t)n_streams;
    icet::BufferGroup& m = g->fixed;
    if (m.device(g->d_rows, S) || m.pinned(g->h_rows, S, hipHostMallocCoherent) || m.pinned(g->h_x0, 6 * S) || m.pinned(g->h_out, 48 * S, hipHostMallocCoherent) || m.device(g->d_out, 48 * S))
        return fail(ICET_ERR_NOMEM);
    if (p->map_capacity > 0) g->fast_shuffle = fast_shuffle_ok();
    for (size_t i = 0; i < S; i++) { const icet_status ss = stream_create(*p, g->s[i]); if (ss != ICET_OK) return fail(ss); }
    *out = g;
    return ICET_OK;
}

icet_status icet_node_group_destroy(icet_node_group* g) {
    if (!g) return ICET_ERR_BAD_ARG;
    delete g->pool; g->pool = nullptr;                            // (joins the helpers: none is drawing between calls)
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();                                 // not the borrowed stream: the context may already be gone
    delete g;                                                     // (its buffer groups and its streams' free here: behind the synchronisation, with the group's device current)
    return ICET_OK;
}

const char* icet_node_group_last_error(const icet_node_group* g) { return g ? g->err.c_str() : ""; }

icet_status icet_node_group_push_device(icet_node_group* g, int32_t n, const int32_t* stream_ids, const icet_dev_scan* frames, icet_node_result* results) {
    // every argument is checked before anything is touched: a refused call leaves every stream as it was
    if (!g || n < 0 || (n > 0 && (!stream_ids || !frames || !results))) return ICET_ERR_BAD_ARG;
    if (n == 0) return ICET_OK;
    if (n > g->n_streams) return ICET_ERR_BAD_ARG;                // (n distinct ids cannot fit otherwise)
    std::vector<char> seen;
    try { seen.assign((size_t)g->n_streams, 0); } catch (...) { return ICET_ERR_NOMEM; }
    for (int i = 0; i < n; i++) {
        const int32_t id = stream_ids[i];
        if (id < 0 || id >= g->n_streams || seen[(size_t)id]) return ICET_ERR_BAD_ARG;
        seen[(size_t)id] = 1;
        const icet_dev_scan& f = frames[i];
        if (f.n < 0 || f.ld < f.n || (f.n > 0 && !f.ptr) || f.n >= ((int64_t)1 << 30) || f.ld >= ((int64_t)1 << 30)) return ICET_ERR_BAD_ARG;
    }
    if (hipSetDevice(g->device) != hipSuccess) return ICET_ERR_NO_DEVICE;
    return group_push(g, n, stream_ids, frames, results);
}

// (stream_rows_out; everything of a group runs on its one stream, so the copy out is behind the last call's map and aligned-cloud launches)
icet_status icet_node_group_map(icet_node_group* g, int32_t stream, float* out, int64_t ld, int64_t* rows_out) {
    if (!g || !rows_out || stream < 0 || stream >= g->n_streams) return ICET_ERR_BAD_ARG;
    return stream_rows_out(g, g->s[(size_t)stream], kRowsMap, true, out, ld, rows_out);
}

icet_status icet_node_group_prev_scan(icet_node_group* g, int32_t stream, float* out, int64_t ld, int64_t* rows_out) {
    if (!g || !rows_out || stream < 0 || stream >= g->n_streams) return ICET_ERR_BAD_ARG;
    return stream_rows_out(g, g->s[(size_t)stream], kRowsPrevScan, true, out, ld, rows_out);
}

icet_status icet_node_group_aligned(icet_node_group* g, int32_t stream, float* out, int64_t ld, int64_t* rows_out) {
    if (!g || !rows_out || stream < 0 || stream >= g->n_streams) return ICET_ERR_BAD_ARG;
    return stream_rows_out(g, g->s[(size_t)stream], kRowsAligned, true, out, ld, rows_out);
}

icet_status icet_node_group_snail_trail(icet_node_group* g, int32_t stream, float* out, int64_t ld, int64_t* rows_out) {
    if (!g || !rows_out || stream < 0 || stream >= g->n_streams) return ICET_ERR_BAD_ARG;
    return stream_rows_out(g, g->s[(size_t)stream], kRowsSnail, true, out, ld, rows_out);
}

}  // extern "C"
