// icet_amd/csrc/icet_deskew.hip -- the deskewer of the C ABI (include/icet_hip.h icet_deskew_*): the rows of many scans, each scan with the
// motion of its own sweep, carried into the sensor frame at one instant of that sweep.  The rule -- a row's class, its time, its new coordinates -- is
// icet_deskew.h; this file is the two kernels around it and the entry points:
//     k_deskew          one launch for all scans of a call, with k_map_add's addressing: blockIdx -> (scan, chunk of kRowsPerBlock rows) by a search over the scans'
//                       first blocks (64 probes per step), two trips of 256 lanes x 4 consecutive rows, both loaded before the first is worked on.  A column's four
//                       rows are one 16-byte load where the address allows it and all four exist, scalar loads otherwise; the stores follow the same rule on the
//                       DESTINATION's address.  Every row is read once and written once (non-temporal both ways), padding is neither read nor written, and a lane
//                       writes only the rows it read: in place is safe.  The five classes are tallied per block in LDS and added to the scan's record with one
//                       atomic per non-zero counter (integers: the order does not show).
//     k_deskew_twists   one thread per scan: the twist between two consecutive float32 poses in HBM (rule::twist_between), six doubles.
// The host side stages one record and one first block per scan (pinned, then on the device, behind a read fence: the shape of the voxel map's CallStage, in a
// stage of its own).
#include <hip/hip_runtime.h>
#include "../../include/icet_hip.h"
#include "icet_ctx.h"
#include "icet_staging.h"
#include "icet_deskew.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace icet {
namespace {

namespace rule = icet_deskew_rule;
typedef unsigned long long u64;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kRowsPerBlock = 2048;      // a block's chunk of one scan: two trips of 256 lanes x 4 rows
constexpr int kTrips = kRowsPerBlock / (4 * kBlock);
static_assert(kTrips * 4 * kBlock == kRowsPerBlock, "whole trips");
constexpr int kCountWords = 8;           // icet_deskew_counts: moved | zero | nonfinite | bad_time | out_of_range | 3 reserved
static_assert(sizeof(icet_deskew_counts) == 8 * kCountWords && sizeof(icet_deskew_scan) == 128, "the records the header names");
static_assert(rule::kTimeArray == ICET_DESKEW_TIME_ARRAY && rule::kTimeColumnFast == ICET_DESKEW_TIME_COLUMN_FAST && rule::kTimeColumnSlow == ICET_DESKEW_TIME_COLUMN_SLOW,
              "the modes the header names");

// A scan as the device reads it.  block0: the first block of the scan in the launch.
struct DeskewRec {
    const float* src; float* dst; const float* time;
    int32_t n, ld, ld_out, block0, mode, period;
    double t0, inv_span, s_ref, xi[6];
};
static_assert(sizeof(DeskewRec) == 120, "src | dst | time | n | ld | ld_out | block0 | mode | period | t0 | inv_span | s_ref | xi");

// m <= 4 rows of one column from row i (a multiple of 4 within its scan): one 16-byte access where the column's address allows it and all four rows exist.
__device__ __forceinline__ void load_rows(const float* col, int i, int m, float v[4]) {
    const float* p = col + i;
    if (m == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = r < m ? __builtin_nontemporal_load(p + r) : 0.f;      // (r < m: inside the n rows)
    }
}
__device__ __forceinline__ void store_rows(float* col, int i, int m, const float v[4]) {
    float* p = col + i;
    if (m == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        f32x4 q; q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        __builtin_nontemporal_store(q, reinterpret_cast<f32x4*>(p));
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++) if (r < m) __builtin_nontemporal_store(v[r], p + r);
    }
}

// One scan's rows [row0, end) are the block's; both trips are loaded before the first is worked on, so that eight 16-byte loads per lane are in flight.
__global__ __launch_bounds__(kBlock) void k_deskew(const DeskewRec* __restrict__ recs, const int32_t* __restrict__ first, int n_scans, const double* __restrict__ d_twists,
                                                   u64* __restrict__ d_counts) {
    __shared__ uint32_t lctr[rule::kRowClasses];
    // the scan of this block: the last one whose first block is not behind it (a scan without rows has no block).  first[] is ascending and first[0] = 0; a step
    // probes 64 places of the range at once, one per lane, every wave the same way: two dependent loads for up to 4096 scans where a bisection takes twelve.
    int lo = 0, len = n_scans;
    while (len > 1) {
        const int stride = (len + 63) >> 6, at = lo + (int)(threadIdx.x & 63) * stride;
        const bool le = at < lo + len && first[at] <= (int)blockIdx.x;      // (at < n_scans) true for a prefix of the lanes, lane 0 among them
        const int c = __popcll(__ballot(le));
        len = min(stride, lo + len - (lo + (c - 1) * stride));
        lo += (c - 1) * stride;
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    const DeskewRec sc = recs[lo];
    const int row0 = ((int)blockIdx.x - sc.block0) * kRowsPerBlock;
    if (row0 < 0 || row0 >= sc.n) return;                             // (the same for every thread of the block)
    const int end = min(sc.n, row0 + kRowsPerBlock);
    if (threadIdx.x < rule::kRowClasses) lctr[threadIdx.x] = 0u;
    __syncthreads();
    rule::Motion m;
    m.t0 = sc.t0; m.inv_span = sc.inv_span; m.s_ref = sc.s_ref; m.mode = sc.mode; m.period = sc.period;
#pragma unroll
    for (int a = 0; a < 6; a++) m.xi[a] = d_twists ? d_twists[6 * (size_t)lo + a] : sc.xi[a];
    const float* sx = sc.src; const float* sy = sx + sc.ld; const float* sz = sx + 2 * (size_t)sc.ld;
    float* dx = sc.dst; float* dy = dx + sc.ld_out; float* dz = dx + 2 * (size_t)sc.ld_out;
    uint32_t n_rows = 0, n_zero = 0, n_nonfinite = 0, n_bad_time = 0, n_range = 0;

    float x[kTrips][4], y[kTrips][4], z[kTrips][4], t[kTrips][4];
    int mr[kTrips];
#pragma unroll
    for (int k = 0; k < kTrips; k++) {
        const int i = row0 + 4 * (int)threadIdx.x + k * 4 * kBlock;
        mr[k] = max(0, min(4, end - i));                             // the lane's rows of trip k that exist
#pragma unroll
        for (int r = 0; r < 4; r++) t[k][r] = 0.f;
        if (mr[k] == 0) continue;
        load_rows(sx, i, mr[k], x[k]); load_rows(sy, i, mr[k], y[k]); load_rows(sz, i, mr[k], z[k]);
        if (sc.mode == rule::kTimeArray) load_rows(sc.time, i, mr[k], t[k]);
    }
#pragma unroll
    for (int k = 0; k < kTrips; k++) {
        if (mr[k] == 0) continue;
        const int i = row0 + 4 * (int)threadIdx.x + k * 4 * kBlock;
        n_rows += (uint32_t)mr[k];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (r >= mr[k]) continue;
            float o[3];
            const int cls = rule::deskew_row(m, i + r, t[k][r], x[k][r], y[k][r], z[k][r], o);
            n_zero += cls == rule::kRowZero; n_nonfinite += cls == rule::kRowNonfinite; n_bad_time += cls == rule::kRowBadTime; n_range += cls == rule::kRowOutOfRange;
            if (cls == rule::kRowMoved) { x[k][r] = o[0]; y[k][r] = o[1]; z[k][r] = o[2]; }      // (every other class keeps the row's bits)
        }
        store_rows(dx, i, mr[k], x[k]); store_rows(dy, i, mr[k], y[k]); store_rows(dz, i, mr[k], z[k]);
    }
    if (!d_counts) return;                                            // (the same for every thread of the launch)
    const uint32_t n_moved = n_rows - n_zero - n_nonfinite - n_bad_time - n_range;
    if (n_moved) atomicAdd(&lctr[rule::kRowMoved], n_moved);
    if (n_zero) atomicAdd(&lctr[rule::kRowZero], n_zero);
    if (n_nonfinite) atomicAdd(&lctr[rule::kRowNonfinite], n_nonfinite);
    if (n_bad_time) atomicAdd(&lctr[rule::kRowBadTime], n_bad_time);
    if (n_range) atomicAdd(&lctr[rule::kRowOutOfRange], n_range);
    __syncthreads();
    if (threadIdx.x < rule::kRowClasses && lctr[threadIdx.x])
        __hip_atomic_fetch_add(&d_counts[kCountWords * (size_t)lo + threadIdx.x], (u64)lctr[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(64) void k_deskew_twists(const float* __restrict__ poses, int n, double scale, double* __restrict__ twists) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    float T0[16], T1[16];
    for (int j = 0; j < 12; j++) { T0[j] = poses[16 * (size_t)k + j]; T1[j] = poses[16 * (size_t)(k + 1) + j]; }      // (n + 1 poses)
    double xi[6];
    rule::twist_between(T0, T1, scale, xi);
    for (int a = 0; a < 6; a++) twists[6 * (size_t)k + a] = xi[a];
}

// THE STAGE OF A CALL: n records, pinned and then copied to the device.  The host writes the pinned side only behind the fence, which the call marks behind its
// kernel (the voxel map's CallStage without the poses).
struct DeskewStage {
    uint8_t* h_buf = nullptr; uint8_t* d_buf = nullptr; int32_t cap = 0;      // n records, then the n first blocks: one copy
    ReadFence fence; BufferGroup mem;
    ~DeskewStage() { fence.destroy(); }
    static size_t bytes(int32_t n) { return (sizeof(DeskewRec) + sizeof(int32_t)) * (size_t)n; }
    DeskewRec* h_rec() const { return reinterpret_cast<DeskewRec*>(h_buf); }
    int32_t* h_first(int32_t n) const { return reinterpret_cast<int32_t*>(h_buf + sizeof(DeskewRec) * (size_t)n); }
    const DeskewRec* d_rec() const { return reinterpret_cast<const DeskewRec*>(d_buf); }
    const int32_t* d_first(int32_t n) const { return reinterpret_cast<const int32_t*>(d_buf + sizeof(DeskewRec) * (size_t)n); }
    // A call of n begins: the previous call has read the staging; n above the capacity drains the stream (its kernel may still read the device side) and grows.
    hipError_t begin(int32_t n, hipStream_t st) {
        hipError_t e = fence.wait();
        if (e == hipSuccess && n > cap) e = hipStreamSynchronize(st);
        if (e != hipSuccess || n <= cap) return e;
        return static_cast<hipError_t>(grow(mem, cap, n, [&] { const int a = mem.pinned(h_buf, bytes(n)); return a ? a : mem.device(d_buf, bytes(n)); }));
    }
    hipError_t upload(int32_t n, hipStream_t st) { return hipMemcpyAsync(d_buf, h_buf, bytes(n), hipMemcpyHostToDevice, st); }
    hipError_t mark_read(hipStream_t st) { return fence.mark(st); }
};

}  // namespace
}  // namespace icet

using namespace icet;

// A deskewer: the stage of a call, and what the host form stages -- the scans' columns and times on the device (x_buf), the counts on the device and pinned.
struct icet_deskewer {
    icet_ctx* ctx = nullptr;
    std::string err;
    DeskewStage stage;
    float* x_buf = nullptr; int64_t cap_x = 0;
    u64* x_cnt = nullptr; u64* x_h_cnt = nullptr; int32_t cap_cnt = 0;
    BufferGroup xmem, xcnt;
};

#define DSKCHK(h, call) do { const hipError_t e_ = static_cast<hipError_t>(call); if (e_ != hipSuccess) { \
    (void)hipGetLastError(); (h)->err = std::string(#call) + ": " + hipGetErrorString(e_); \
    return e_ == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; } } while (0)

static icet_status enter(icet_deskewer* h) {
    if (!h) return ICET_ERR_BAD_ARG;
    const icet_status st = enter(h->ctx);
    if (st != ICET_OK) h->err = h->ctx->err;
    return st;
}
static icet_status dsk_refuse(icet_deskewer* h, const std::string& why) { h->err = why; return ICET_ERR_BAD_ARG; }
template <class T> static bool elem_aligned(const T* p) { return reinterpret_cast<uintptr_t>(p) % sizeof(T) == 0; }      // (a null pointer is)

// Every argument of a call, before anything is touched: "" or the reason of the refusal.  *blocks: the blocks of the launch.
static std::string deskew_check(int32_t n, const icet_deskew_scan* scans, const char* call, int64_t* blocks) {
    const std::string who(call);
    if (n < 0 || (n > 0 && !scans)) return who + ": bad argument";
    int64_t b = 0;
    for (int k = 0; k < n; k++) {
        const icet_deskew_scan& s = scans[k];
        const std::string at = " (scans[" + std::to_string(k) + "])";
        if (!rule::shape_ok(s.n, s.ld, s.ld_out)) return who + ": bad scan descriptor: n >= 0, n <= ld < 2^30, n <= ld_out < 2^30" + at;
        if (s.n > 0 && (!s.src || !s.dst)) return who + ": a NULL src or dst" + at;
        if (!rule::mode_ok(s.time_mode, s.period)) return who + ": unknown time_mode, or period <= 0 in a column mode" + at;
        if (s.n > 0 && s.time_mode == rule::kTimeArray && !s.time) return who + ": ICET_DESKEW_TIME_ARRAY needs time" + at;
        if (!(elem_aligned(s.src) && elem_aligned(s.dst) && elem_aligned(s.time))) return who + ": a pointer is not aligned to 4 bytes" + at;
        if (rule::overlap(s.src, s.ld, s.dst, s.ld_out, s.n) == 2) return who + ": dst overlaps src without being identical to it" + at;
        b += (s.n + kRowsPerBlock - 1) / kRowsPerBlock;
    }
    if (b > 0x7FFFFFFF) return who + ": too many rows in one call";
    *blocks = b;
    return std::string();
}

// The checked call on device memory: the records staged, the counts zeroed, one launch.
static icet_status deskew_run(icet_deskewer* h, int32_t n, const icet_deskew_scan* scans, const double* d_twists, icet_deskew_counts* d_counts, int64_t blocks) {
    hipStream_t st = h->ctx->stream;
    if (n > 0 && d_counts) DSKCHK(h, hipMemsetAsync(d_counts, 0, sizeof(icet_deskew_counts) * (size_t)n, st));
    if (blocks == 0) return ICET_OK;                                  // nothing to read
    DeskewStage& s = h->stage;
    DSKCHK(h, s.begin(n, st));
    int32_t b0 = 0;
    for (int k = 0; k < n; k++) {
        const icet_deskew_scan& a = scans[k];
        DeskewRec r;
        std::memset(&r, 0, sizeof(r));
        r.src = a.src; r.dst = a.dst; r.time = a.time; r.n = (int32_t)a.n; r.ld = (int32_t)a.ld; r.ld_out = (int32_t)a.ld_out; r.block0 = b0;
        r.mode = a.time_mode; r.period = a.period; r.t0 = a.t0; r.inv_span = a.inv_span; r.s_ref = a.s_ref;
        std::memcpy(r.xi, a.twist, sizeof(r.xi));
        s.h_rec()[k] = r; s.h_first(n)[k] = b0;
        b0 += (int32_t)((a.n + kRowsPerBlock - 1) / kRowsPerBlock);
    }
    DSKCHK(h, s.upload(n, st));
    k_deskew<<<(unsigned)blocks, kBlock, 0, st>>>(s.d_rec(), s.d_first(n), n, d_twists, reinterpret_cast<u64*>(d_counts));
    DSKCHK(h, hipGetLastError());
    DSKCHK(h, s.mark_read(st));
    return ICET_OK;
}

extern "C" {

const char* icet_deskewer_last_error(const icet_deskewer* h) { return h ? h->err.c_str() : "null deskewer"; }

icet_status icet_deskewer_create(icet_ctx* c, icet_deskewer** out) {
    if (out) *out = nullptr;
    if (!c) return ICET_ERR_BAD_ARG;
    if (!out) { c->err = "icet_deskewer_create: bad argument"; return ICET_ERR_BAD_ARG; }
    ICET_TRY(enter(c));
    icet_deskewer* h = new (std::nothrow) icet_deskewer();
    if (!h) { c->err = "host allocation failed"; return ICET_ERR_NOMEM; }
    h->ctx = c;
    *out = h;
    return ICET_OK;
}

icet_status icet_deskewer_destroy(icet_deskewer* h) {
    if (!h) return ICET_ERR_BAD_ARG;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);              // (a call may still read the records)
    delete h;                                                // (every array belongs to a group, the event to the stage)
    return ICET_OK;
}

icet_status icet_deskew_device(icet_deskewer* h, int32_t n, const icet_deskew_scan* scans, const double* d_twists, icet_deskew_counts* d_counts) {
    ICET_TRY(enter(h));
    int64_t blocks = 0;
    const std::string why = deskew_check(n, scans, "icet_deskew_device", &blocks);
    if (!why.empty()) return dsk_refuse(h, why);
    if (!elem_aligned(d_twists) || !elem_aligned(reinterpret_cast<const u64*>(d_counts))) return dsk_refuse(h, "icet_deskew_device: d_twists or d_counts is not aligned to 8 bytes");
    return deskew_run(h, n, scans, d_twists, d_counts, blocks);
}

icet_status icet_deskew(icet_deskewer* h, int32_t n, const icet_deskew_scan* scans, icet_deskew_counts* counts) {
    ICET_TRY(enter(h));
    int64_t blocks = 0;
    const std::string why = deskew_check(n, scans, "icet_deskew", &blocks);
    if (!why.empty()) return dsk_refuse(h, why);
    if (n == 0) return ICET_OK;
    hipStream_t st = h->ctx->stream;
    // the layout on the device: per scan src (3 columns of l), dst (3 columns of l), time (l), l = the rows rounded up to 64
    int64_t words = 0;
    for (int k = 0; k < n; k++) words += 7 * padded_ld(scans[k].n);
    if (words > h->cap_x || n > h->cap_cnt) DSKCHK(h, hipStreamSynchronize(st));
    if (words > h->cap_x) DSKCHK(h, grow(h->xmem, h->cap_x, words, [&] { return h->xmem.device(h->x_buf, (size_t)words); }));
    if (n > h->cap_cnt) DSKCHK(h, grow(h->xcnt, h->cap_cnt, n, [&] {
        const int a = h->xcnt.device(h->x_cnt, kCountWords * (size_t)n);
        return a ? a : h->xcnt.pinned(h->x_h_cnt, kCountWords * (size_t)n);
    }));
    std::vector<icet_deskew_scan> dev(scans, scans + n);
    int64_t o = 0;
    for (int k = 0; k < n; k++) {
        const icet_deskew_scan& a = scans[k];
        const int64_t l = padded_ld(a.n);
        icet_deskew_scan& d = dev[k];
        d.src = h->x_buf + o; d.ld = l; d.dst = h->x_buf + o + 3 * l; d.ld_out = l; d.time = a.time ? h->x_buf + o + 6 * l : nullptr;
        o += 7 * l;
        if (a.n == 0) continue;
        DSKCHK(h, hipMemcpy2DAsync(const_cast<float*>(d.src), sizeof(float) * (size_t)l, a.src, sizeof(float) * (size_t)a.ld, sizeof(float) * (size_t)a.n, 3, hipMemcpyHostToDevice, st));
        if (a.time) DSKCHK(h, hipMemcpyAsync(const_cast<float*>(d.time), a.time, sizeof(float) * (size_t)a.n, hipMemcpyHostToDevice, st));
    }
    ICET_TRY(deskew_run(h, n, dev.data(), nullptr, reinterpret_cast<icet_deskew_counts*>(h->x_cnt), blocks));
    for (int k = 0; k < n; k++) {
        const icet_deskew_scan& a = scans[k];
        if (a.n == 0) continue;
        DSKCHK(h, hipMemcpy2DAsync(a.dst, sizeof(float) * (size_t)a.ld_out, dev[k].dst, sizeof(float) * (size_t)dev[k].ld_out, sizeof(float) * (size_t)a.n, 3, hipMemcpyDeviceToHost, st));
    }
    DSKCHK(h, hipMemcpyAsync(h->x_h_cnt, h->x_cnt, sizeof(u64) * kCountWords * (size_t)n, hipMemcpyDeviceToHost, st));
    DSKCHK(h, hipStreamSynchronize(st));
    if (counts) std::memcpy(counts, h->x_h_cnt, sizeof(icet_deskew_counts) * (size_t)n);
    return ICET_OK;
}

icet_status icet_deskew_twists_from_poses_device(icet_deskewer* h, int32_t n, const float* d_poses, double scale, double* d_twists) {
    ICET_TRY(enter(h));
    if (n < 0 || (n > 0 && (!d_poses || !d_twists))) return dsk_refuse(h, "icet_deskew_twists_from_poses_device: bad argument");
    if (!elem_aligned(d_poses) || !elem_aligned(d_twists)) return dsk_refuse(h, "icet_deskew_twists_from_poses_device: a device pointer is not aligned to its element");
    if (n == 0) return ICET_OK;
    k_deskew_twists<<<(unsigned)((n + 63) / 64), 64, 0, h->ctx->stream>>>(d_poses, n, scale, d_twists);
    DSKCHK(h, hipGetLastError());
    return ICET_OK;
}

icet_status icet_twist_from_pose(const double T[16], double xi[6]) {
    if (!T || !xi) return ICET_ERR_BAD_ARG;
    rule::twist_from_pose(T, xi);
    return ICET_OK;
}

icet_status icet_pose_from_twist(const double xi[6], double s, double T[16]) {
    if (!xi || !T) return ICET_ERR_BAD_ARG;
    rule::pose_from_twist(xi, s, T);
    return ICET_OK;
}

icet_status icet_debug_deskew_rows(const icet_deskew_scan* motion, int64_t n, const float* x, const float* y, const float* z, const float* time,
                                   float* out_x, float* out_y, float* out_z, int32_t* cls) {
    if (!motion || n < 0 || n >= ((int64_t)1 << 30) || !rule::mode_ok(motion->time_mode, motion->period)) return ICET_ERR_BAD_ARG;
    if (n > 0 && (!x || !y || !z || !out_x || !out_y || !out_z || (motion->time_mode == rule::kTimeArray && !time))) return ICET_ERR_BAD_ARG;
    rule::Motion m;
    m.t0 = motion->t0; m.inv_span = motion->inv_span; m.s_ref = motion->s_ref; m.mode = motion->time_mode; m.period = motion->period;
    std::memcpy(m.xi, motion->twist, sizeof(m.xi));
    for (int64_t i = 0; i < n; i++) {
        float o[3];
        const int c = rule::deskew_row(m, (int32_t)i, time ? time[i] : 0.f, x[i], y[i], z[i], o);
        if (c == rule::kRowMoved) { out_x[i] = o[0]; out_y[i] = o[1]; out_z[i] = o[2]; }
        else { uint32_t b[3]; std::memcpy(&b[0], &x[i], 4); std::memcpy(&b[1], &y[i], 4); std::memcpy(&b[2], &z[i], 4);      // (the bits, and out may be the input)
               std::memcpy(&out_x[i], &b[0], 4); std::memcpy(&out_y[i], &b[1], 4); std::memcpy(&out_z[i], &b[2], 4); }
        if (cls) cls[i] = c;
    }
    return ICET_OK;
}

}  // extern "C"
