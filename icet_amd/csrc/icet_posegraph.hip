// icet_amd/csrc/icet_posegraph.hip -- the pose-graph optimiser (include/icet_hip.h icet_pose_graph_optimize[_device]): the kernels, the
// device's backend of the driver, the entry points, and the band solve's test hook.
//
// The odometry chain of a pose graph makes its normal equations block tridiagonal with 6 x 6 blocks; every closure adds one block pair off the band.  The solve of
// the band is the kernel that matters: ONE workgroup of 256 threads factors it by block Cholesky and sweeps it forward and back (a block Thomas recurrence,
// sequential in the node index: one thread walks it, out of chunks of 32 nodes that all threads stage through LDS).  Around it: small kernels that each do one
// thing on plain global arrays, every body in icet_posegraph_body.h, driven from the host by icet_posegraph_driver.h.  No kernel waits on another block.
// Option "pg_solver" replaces the conjugate gradients by a direct solve over the closures' end nodes (icet_posegraph_direct.h): k_pg_z solves the band for
// all their unit columns in one launch, one thread per column.  icet_pose_graph_marginals[_device] reads the marginal covariance of every pose off that solve's
// Z, L and Lk and a selected inverse of the band (icet_posegraph_marginals.h).
#include "icet_ctx.h"
#include "icet_posegraph_driver.h"

#include <string>
#include <vector>

namespace icet {

__global__ __launch_bounds__(kPgThreads) void k_pg_block_tridiag(int N, const double* Dm, const double* Bm, const double* rhs, double* x, double* G, double* W, double* u, int32_t* status) {
    __shared__ PgShared sh;
    pg_block_tridiag(N, Dm, Bm, rhs, x, G, W, u, status, sh);
}

// grid kernels: one thread per global index below `count`
constexpr int kPgGridThreads = 256;
#define ICET_PG_GRID_KERNEL(name, body) \
    __global__ __launch_bounds__(kPgGridThreads) void name(PgArgs a, int count) { \
        const int gi = (int)(blockIdx.x * kPgGridThreads + threadIdx.x); \
        if (gi < count) body(a, gi); \
    }
ICET_PG_GRID_KERNEL(k_pg_init, pg_init)
ICET_PG_GRID_KERNEL(k_pg_chi, pg_chi)
ICET_PG_GRID_KERNEL(k_pg_linearise, pg_linearise)
ICET_PG_GRID_KERNEL(k_pg_assemble, pg_assemble)
ICET_PG_GRID_KERNEL(k_pg_offband, pg_offband)
ICET_PG_GRID_KERNEL(k_pg_hp, pg_hp)
ICET_PG_GRID_KERNEL(k_pg_retract, pg_retract)
ICET_PG_GRID_KERNEL(k_pg_finish, pg_finish)
#undef ICET_PG_GRID_KERNEL

// one-workgroup kernels
__global__ __launch_bounds__(kPgThreads) void k_pg_factor(PgArgs a) { __shared__ PgShared sh; pg_group_factor(a, sh); }
__global__ __launch_bounds__(kPgThreads) void k_pg_precond(PgArgs a) { __shared__ PgShared sh; __shared__ PgRed red; pg_group_precond(a, sh, red); }
__global__ __launch_bounds__(kPgThreads) void k_pg_step(PgArgs a) { __shared__ PgRed red; pg_group_step(a, red); }
__global__ __launch_bounds__(kPgThreads) void k_pg_stats(PgArgs a) { __shared__ PgRed red; pg_group_stats(a, red); }

// the direct solve (icet_posegraph_direct.h).  k_pg_z is the kernel that matters: one thread per column of Z walks the chain forward and back.
#define ICET_PG_GRID_KERNEL(name, body) \
    __global__ __launch_bounds__(kPgGridThreads) void name(PgArgs a, PgDirect d, int count) { \
        const int gi = (int)(blockIdx.x * kPgGridThreads + threadIdx.x); \
        if (gi < count) body(a, d, gi); \
    }
ICET_PG_GRID_KERNEL(k_pg_z, pg_z)
ICET_PG_GRID_KERNEL(k_pg_wm, pg_wm)
ICET_PG_GRID_KERNEL(k_pg_sl, pg_sl)
ICET_PG_GRID_KERNEL(k_pg_ks, pg_ks)
ICET_PG_GRID_KERNEL(k_pg_zw, pg_zw)
ICET_PG_GRID_KERNEL(k_pg_resid, pg_resid)
#undef ICET_PG_GRID_KERNEL
__global__ __launch_bounds__(kPgThreads) void k_pg_chol(PgArgs a, PgDirect d, int which) { pg_group_chol(a, d, which); }
__global__ __launch_bounds__(kPgThreads) void k_pg_band(PgArgs a, PgDirect d) { __shared__ PgShared sh; pg_group_band(a, d, sh); }
__global__ __launch_bounds__(kPgThreads) void k_pg_cap_solve(PgArgs a, PgDirect d) { pg_group_cap_solve(a, d); }

// the marginal covariances (icet_posegraph_marginals.h).  k_pg_selinv is the sequential part; k_pg_marg runs one workgroup per node.
__global__ __launch_bounds__(kPgGridThreads) void k_pg_selinv_prep(PgArgs a, PgMarg mg, int count) {
    const int gi = (int)(blockIdx.x * kPgGridThreads + threadIdx.x);
    if (gi < count) pg_selinv_prep(a, mg, gi);
}
__global__ __launch_bounds__(kPgGridThreads) void k_pg_marg_lt(PgArgs a, PgDirect d, PgMarg mg, int count) {
    const int gi = (int)(blockIdx.x * kPgGridThreads + threadIdx.x);
    if (gi < count) pg_marg_lt(a, d, mg, gi);
}
__global__ __launch_bounds__(kPgThreads) void k_pg_selinv(PgArgs a, PgMarg mg) { __shared__ PgShared sh; pg_group_selinv(a, mg, sh); }
__global__ __launch_bounds__(kPgThreads) void k_pg_marg(PgArgs a, PgDirect d, PgMarg mg) { __shared__ PgMargShared sh; pg_group_marg(a, d, mg, (int)blockIdx.x, sh); }

namespace {

// The device's backend of pg_optimise: launches on the context's stream; the scalars come back through pinned memory.
struct PgDeviceBackend {
    hipStream_t stream = nullptr;
    double* h_sc = nullptr;                 // pinned, kPgScalars
    hipError_t err = hipSuccess;
    bool ok(hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; return e == hipSuccess; }
    bool grid(PgGridKernel k, int count, const PgArgs& a) {
        if (count <= 0) return true;
        const dim3 g((unsigned)((count + kPgGridThreads - 1) / kPgGridThreads)), b(kPgGridThreads);
        switch (k) {
            case kPgInit:      hipLaunchKernelGGL(k_pg_init, g, b, 0, stream, a, count); break;
            case kPgChi:       hipLaunchKernelGGL(k_pg_chi, g, b, 0, stream, a, count); break;
            case kPgLinearise: hipLaunchKernelGGL(k_pg_linearise, g, b, 0, stream, a, count); break;
            case kPgAssemble:  hipLaunchKernelGGL(k_pg_assemble, g, b, 0, stream, a, count); break;
            case kPgOffband:   hipLaunchKernelGGL(k_pg_offband, g, b, 0, stream, a, count); break;
            case kPgHp:        hipLaunchKernelGGL(k_pg_hp, g, b, 0, stream, a, count); break;
            case kPgRetract:   hipLaunchKernelGGL(k_pg_retract, g, b, 0, stream, a, count); break;
            case kPgFinish:    hipLaunchKernelGGL(k_pg_finish, g, b, 0, stream, a, count); break;
        }
        return ok(hipGetLastError());
    }
    bool group(PgGroupKernel k, const PgArgs& a) {
        const dim3 g(1), b(kPgThreads);
        switch (k) {
            case kPgFactor:  hipLaunchKernelGGL(k_pg_factor, g, b, 0, stream, a); break;
            case kPgPrecond: hipLaunchKernelGGL(k_pg_precond, g, b, 0, stream, a); break;
            case kPgStep:    hipLaunchKernelGGL(k_pg_step, g, b, 0, stream, a); break;
            case kPgStats:   hipLaunchKernelGGL(k_pg_stats, g, b, 0, stream, a); break;
        }
        return ok(hipGetLastError());
    }
    bool dgrid(PgDirectGridKernel k, int count, const PgArgs& a, const PgDirect& d) {
        if (count <= 0) return true;
        const dim3 g((unsigned)((count + kPgGridThreads - 1) / kPgGridThreads)), b(kPgGridThreads);
        switch (k) {
            case kPgZ:     hipLaunchKernelGGL(k_pg_z, g, b, 0, stream, a, d, count); break;
            case kPgWm:    hipLaunchKernelGGL(k_pg_wm, g, b, 0, stream, a, d, count); break;
            case kPgSl:    hipLaunchKernelGGL(k_pg_sl, g, b, 0, stream, a, d, count); break;
            case kPgKs:    hipLaunchKernelGGL(k_pg_ks, g, b, 0, stream, a, d, count); break;
            case kPgZw:    hipLaunchKernelGGL(k_pg_zw, g, b, 0, stream, a, d, count); break;
            case kPgResid: hipLaunchKernelGGL(k_pg_resid, g, b, 0, stream, a, d, count); break;
        }
        return ok(hipGetLastError());
    }
    bool dgroup(PgDirectGroupKernel k, const PgArgs& a, const PgDirect& d) {
        const dim3 g(1), b(kPgThreads);
        switch (k) {
            case kPgCholW:    hipLaunchKernelGGL(k_pg_chol, g, b, 0, stream, a, d, 0); break;
            case kPgCholK:    hipLaunchKernelGGL(k_pg_chol, g, b, 0, stream, a, d, 1); break;
            case kPgBand:     hipLaunchKernelGGL(k_pg_band, g, b, 0, stream, a, d); break;
            case kPgCapSolve: hipLaunchKernelGGL(k_pg_cap_solve, g, b, 0, stream, a, d); break;
        }
        return ok(hipGetLastError());
    }
    bool mgrid(PgMargGridKernel k, int count, const PgArgs& a, const PgDirect& d, const PgMarg& mg) {
        if (count <= 0) return true;
        const dim3 g((unsigned)((count + kPgGridThreads - 1) / kPgGridThreads)), b(kPgGridThreads);
        switch (k) {
            case kPgSelinvPrep: hipLaunchKernelGGL(k_pg_selinv_prep, g, b, 0, stream, a, mg, count); break;
            case kPgMargLt:     hipLaunchKernelGGL(k_pg_marg_lt, g, b, 0, stream, a, d, mg, count); break;
        }
        return ok(hipGetLastError());
    }
    bool mgroups(PgMargGroupKernel k, int groups, const PgArgs& a, const PgDirect& d, const PgMarg& mg) {
        if (groups <= 0) return true;
        const dim3 b(kPgThreads);
        switch (k) {
            case kPgSelinv:   hipLaunchKernelGGL(k_pg_selinv, dim3(1), b, 0, stream, a, mg); break;
            case kPgMargNode: hipLaunchKernelGGL(k_pg_marg, dim3((unsigned)groups), b, 0, stream, a, d, mg); break;
        }
        return ok(hipGetLastError());
    }
    bool scalars(const PgArgs& a, double out[kPgScalars]) {
        if (!ok(hipMemcpyAsync(h_sc, a.sc, sizeof(double) * kPgScalars, hipMemcpyDeviceToHost, stream)) || !ok(hipStreamSynchronize(stream))) return false;
        for (int i = 0; i < kPgScalars; i++) out[i] = h_sc[i];
        return true;
    }
    // (the test hook's copies: pageable host memory, complete on return)
    bool fetch(void* host, const void* dev, size_t bytes) { return ok(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream)) && ok(hipStreamSynchronize(stream)); }
    bool put(void* dev, const void* host, size_t bytes) { return ok(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream)) && ok(hipStreamSynchronize(stream)); }
};

// pg_bind's allocator over ONE device block: a first pass with base = nullptr counts the bytes, the second hands them out.  Doubles come first (pg_bind's order),
// so every double is 8-byte aligned; float and int32 arrays follow.
struct PgArena {
    char* base = nullptr; size_t used = 0;
    void* take(size_t bytes) { void* p = base ? base + used : nullptr; used += bytes; return p; }
    double* d(size_t n) { return static_cast<double*>(take(n * sizeof(double))); }
    int32_t* i(size_t n) { return static_cast<int32_t*>(take(n * sizeof(int32_t))); }
    float* f(size_t n) { return static_cast<float*>(take(n * sizeof(float))); }
};

struct PgHostIo {          // the host-pointer form's staging, behind pg_bind's arrays in the same block
    double *poses64 = nullptr, *edge_chi2 = nullptr;
    float *poses = nullptr, *odo_X = nullptr, *odo_info = nullptr, *clo_X = nullptr, *clo_info = nullptr, *poses_out = nullptr;
};

icet_status pg_run(icet_ctx* c, bool host_io, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci, const int32_t* cj,
                   const float* clo_X, const float* clo_info, const uint8_t* fixed, const icet_pose_graph_options* opt, float* poses_out, double* poses64_out,
                   double* edge_chi2, icet_pose_graph_result* result, int32_t K = 0, const double* dbg_p = nullptr, icet_pose_graph_step* dbg = nullptr,
                   icet_pose_graph_direct_step* ddbg = nullptr) {
    ICET_TRY(enter(c));
    const bool hook = dbg || ddbg;
    if (!poses || (!hook && (!poses_out || !result)) || n < 1 || n > pg::kMaxNodes || n_closures < 0 || n_closures > pg::kMaxClosures) { c->err = "icet_pose_graph_optimize: bad argument"; return ICET_ERR_BAD_ARG; }
    if ((n > 1 && (!odo_X || !odo_info)) || (n_closures > 0 && (!ci || !cj || !clo_X || !clo_info))) { c->err = "icet_pose_graph_optimize: null array"; return ICET_ERR_BAD_ARG; }
    if (!pg::closures_ok(n, n_closures, ci, cj)) { c->err = "icet_pose_graph_optimize: a closure's ends are out of range or equal"; return ICET_ERR_BAD_ARG; }
    const icet_pose_graph_options o = opt ? *opt : pg_default_options();
    if (o.gn_iters < 1) { c->err = "icet_pose_graph_optimize: gn_iters < 1"; return ICET_ERR_BAD_ARG; }
    PgGraph graph;
    graph.build(n, n_closures, ci, cj, fixed);
    // the linear solve: the context's option "pg_solver" (the step hook is conjugate gradients, the direct hook direct)
    const int m_ends = (int)graph.ends.size();
    if ((ddbg || (!dbg && c->pg_solver == 1)) && m_ends > kPgDirectMaxEnds) {
        c->err = "icet_pose_graph_optimize: the direct solve takes at most " + std::to_string(kPgDirectMaxEnds) + " end nodes of closures off the band, this graph has " +
                 std::to_string(m_ends) + " (option pg_solver 2 falls back to conjugate gradients)";
        return ICET_ERR_UNSUPPORTED;
    }
    if (ddbg && ddbg->ends_capacity != m_ends) { c->err = "icet_debug_pose_graph_direct: ends_capacity is not the graph's count of end nodes (" + std::to_string(m_ends) + ")"; return ICET_ERR_BAD_ARG; }
    const bool direct = ddbg || (!dbg && (c->pg_solver == 1 || (c->pg_solver == 2 && m_ends >= 1 && m_ends <= kPgDirectMaxEnds)));

    PgArgs a{};
    PgDirect dir{};
    a.N = n; a.C = n_closures; a.E = pg::edge_count(n, n_closures);
    const size_t N = (size_t)n, E = (size_t)a.E, C = (size_t)n_closures, n_items = graph.items.size();
    PgArena arena;
    PgGraphDev gd{};
    PgDirectDev dd{};
    PgHostIo io;
    auto layout = [&]() {
        arena.used = 0;
        gd = pg_bind(a, arena, n_items);
        if (direct) {
            arena.used = (arena.used + 7) & ~(size_t)7;
            dd = pg_bind_direct(a, dir, arena, (size_t)m_ends);
        }
        if (host_io) {
            // (int32 lists end on a multiple of 4 bytes; the doubles of the staging need 8)
            arena.used = (arena.used + 7) & ~(size_t)7;
            io.poses64 = poses64_out ? arena.d(N * 12) : nullptr; io.edge_chi2 = edge_chi2 ? arena.d(2 * E) : nullptr;
            io.poses = arena.f(N * 16); io.odo_X = arena.f((N - 1) * 6); io.odo_info = arena.f((N - 1) * 36); io.clo_X = arena.f(C * 6); io.clo_info = arena.f(C * 36);
            io.poses_out = arena.f(N * 16);
        }
    };
    layout();
    const size_t bytes = arena.used;
    char* block = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&block), bytes));
    arena.base = block;
    layout();

    PgDeviceBackend be;
    be.stream = c->stream;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&be.h_sc), sizeof(double) * kPgScalars, hipHostMallocDefault);
    auto up = [&](void* dst, const void* src, size_t nbytes) { if (e == hipSuccess && nbytes) e = hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice, c->stream); };
    auto down = [&](void* dst, const void* src, size_t nbytes) { if (e == hipSuccess && dst && nbytes) e = hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost, c->stream); };
    up(gd.ei, graph.ei.data(), sizeof(int32_t) * E); up(gd.ej, graph.ej.data(), sizeof(int32_t) * E);
    up(gd.off, graph.off.data(), sizeof(int32_t) * (N + 1)); up(gd.items, graph.items.data(), sizeof(int32_t) * n_items);
    if (direct) { up(dd.ends, graph.ends.data(), sizeof(int32_t) * (size_t)m_ends); up(dd.end_of, graph.end_of.data(), sizeof(int32_t) * N); }
    if (host_io) {
        up(io.poses, poses, sizeof(float) * N * 16); up(io.odo_X, odo_X, sizeof(float) * (N - 1) * 6); up(io.odo_info, odo_info, sizeof(float) * (N - 1) * 36);
        up(io.clo_X, clo_X, sizeof(float) * C * 6); up(io.clo_info, clo_info, sizeof(float) * C * 36);
        a.poses_in = io.poses; a.odo_X = io.odo_X; a.odo_info = io.odo_info; a.clo_X = io.clo_X; a.clo_info = io.clo_info;
        a.poses_out = io.poses_out; a.poses64_out = io.poses64; a.edge_chi2_out = io.edge_chi2;
    } else {
        a.poses_in = poses; a.odo_X = odo_X; a.odo_info = odo_info; a.clo_X = clo_X; a.clo_info = clo_info;
        a.poses_out = poses_out; a.poses64_out = poses64_out; a.edge_chi2_out = edge_chi2;
    }
    icet_pose_graph_result res{};
    bool done = false;
    if (e == hipSuccess) {
        // (the graph's lists and the caller's arrays outlive the synchronisation below; the stream orders the copies before the kernels)
        done = ddbg ? pg_debug_direct_step(be, a, dir, o, K, dbg_p, ddbg)
             : dbg ? pg_debug_step(be, a, o, graph.c_offband, K, dbg_p, dbg)
             : direct ? pg_optimise_direct(be, a, dir, o, &res) : pg_optimise(be, a, o, graph.c_offband, &res);
        if (!done) e = be.err;
    }
    if (done && host_io && !hook) {
        down(poses_out, io.poses_out, sizeof(float) * N * 16); down(poses64_out, io.poses64, sizeof(double) * N * 12); down(edge_chi2, io.edge_chi2, sizeof(double) * 2 * E);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    (void)hipFree(block);
    if (be.h_sc) (void)hipHostFree(be.h_sc);
    if (e != hipSuccess) { c->err = std::string("icet_pose_graph_optimize: ") + hipGetErrorString(e); return e == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; }
    if (result) *result = res;
    return ICET_OK;
}

// The marginal covariances of a graph (icet_pose_graph_marginals[_device], icet_debug_pose_graph_marginals): pg_run's checks, block and staging, pg_marginals in
// the place of the optimiser.
icet_status pg_marg_run(icet_ctx* c, bool host_io, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                        const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, double* cov_out, icet_pose_graph_marginals_result* result,
                        icet_pose_graph_marginals_debug* dbg = nullptr) {
    ICET_TRY(enter(c));
    if (!poses || (!dbg && (!cov_out || !result)) || n < 1 || n > pg::kMaxNodes || n_closures < 0 || n_closures > pg::kMaxClosures) { c->err = "icet_pose_graph_marginals: bad argument"; return ICET_ERR_BAD_ARG; }
    if ((n > 1 && (!odo_X || !odo_info)) || (n_closures > 0 && (!ci || !cj || !clo_X || !clo_info))) { c->err = "icet_pose_graph_marginals: null array"; return ICET_ERR_BAD_ARG; }
    if (!pg::closures_ok(n, n_closures, ci, cj)) { c->err = "icet_pose_graph_marginals: a closure's ends are out of range or equal"; return ICET_ERR_BAD_ARG; }
    PgGraph graph;
    graph.build(n, n_closures, ci, cj, fixed);
    const int m_ends = (int)graph.ends.size();
    if (m_ends > kPgDirectMaxEnds) {
        c->err = "icet_pose_graph_marginals: at most " + std::to_string(kPgDirectMaxEnds) + " end nodes of closures off the band, this graph has " + std::to_string(m_ends);
        return ICET_ERR_UNSUPPORTED;
    }
    if (dbg && dbg->ends_capacity != m_ends) { c->err = "icet_debug_pose_graph_marginals: ends_capacity is not the graph's count of end nodes (" + std::to_string(m_ends) + ")"; return ICET_ERR_BAD_ARG; }

    PgArgs a{};
    PgDirect dir{};
    PgMarg mg{};
    a.N = n; a.C = n_closures; a.E = pg::edge_count(n, n_closures);
    const size_t N = (size_t)n, E = (size_t)a.E, C = (size_t)n_closures, n_items = graph.items.size();
    PgArena arena;
    PgGraphDev gd{};
    PgDirectDev dd{};
    PgHostIo io;
    auto layout = [&]() {
        arena.used = 0;
        gd = pg_bind(a, arena, n_items);
        arena.used = (arena.used + 7) & ~(size_t)7;
        dd = pg_bind_direct(a, dir, arena, (size_t)m_ends);
        arena.used = (arena.used + 7) & ~(size_t)7;
        pg_bind_marg(a, dir, mg, arena, host_io);
        if (host_io) { io.poses = arena.f(N * 16); io.odo_X = arena.f((N - 1) * 6); io.odo_info = arena.f((N - 1) * 36); io.clo_X = arena.f(C * 6); io.clo_info = arena.f(C * 36); }
    };
    layout();
    const size_t bytes = arena.used;
    char* block = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&block), bytes));
    arena.base = block;
    layout();

    PgDeviceBackend be;
    be.stream = c->stream;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&be.h_sc), sizeof(double) * kPgScalars, hipHostMallocDefault);
    auto up = [&](void* dst, const void* src, size_t nbytes) { if (e == hipSuccess && nbytes) e = hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice, c->stream); };
    up(gd.ei, graph.ei.data(), sizeof(int32_t) * E); up(gd.ej, graph.ej.data(), sizeof(int32_t) * E);
    up(gd.off, graph.off.data(), sizeof(int32_t) * (N + 1)); up(gd.items, graph.items.data(), sizeof(int32_t) * n_items);
    up(dd.ends, graph.ends.data(), sizeof(int32_t) * (size_t)m_ends); up(dd.end_of, graph.end_of.data(), sizeof(int32_t) * N);
    if (host_io) {
        up(io.poses, poses, sizeof(float) * N * 16); up(io.odo_X, odo_X, sizeof(float) * (N - 1) * 6); up(io.odo_info, odo_info, sizeof(float) * (N - 1) * 36);
        up(io.clo_X, clo_X, sizeof(float) * C * 6); up(io.clo_info, clo_info, sizeof(float) * C * 36);
        a.poses_in = io.poses; a.odo_X = io.odo_X; a.odo_info = io.odo_info; a.clo_X = io.clo_X; a.clo_info = io.clo_info;
    } else {
        a.poses_in = poses; a.odo_X = odo_X; a.odo_info = odo_info; a.clo_X = clo_X; a.clo_info = clo_info;
        mg.cov = cov_out;
    }
    a.poses_out = nullptr; a.poses64_out = nullptr; a.edge_chi2_out = nullptr;          // (kPgFinish does not run)
    icet_pose_graph_marginals_result res{};
    bool done = false;
    if (e == hipSuccess) {
        PgMargTap tap;
        if (dbg) { tap.D = dbg->D; tap.B = dbg->B; tap.A = dbg->A; tap.band_cov = dbg->band_cov; }
        done = pg_marginals(be, a, dir, mg, &res, dbg ? &tap : nullptr);
        if (!done) e = be.err;
    }
    double* host_cov = dbg ? dbg->cov : cov_out;
    if (done && host_io && host_cov && e == hipSuccess) e = hipMemcpyAsync(host_cov, mg.cov, sizeof(double) * N * 36, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    (void)hipFree(block);
    if (be.h_sc) (void)hipHostFree(be.h_sc);
    if (e != hipSuccess) { c->err = std::string("icet_pose_graph_marginals: ") + hipGetErrorString(e); return e == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; }
    if (dbg) {
        dbg->result = res;
        if (dbg->ends) for (int i = 0; i < m_ends; i++) dbg->ends[i] = graph.ends[(size_t)i];
    }
    if (result) *result = res;
    return ICET_OK;
}

}  // namespace
}  // namespace icet

using namespace icet;

icet_status icet_pose_graph_marginals(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                      const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, double* cov_out,
                                      icet_pose_graph_marginals_result* result) {
    return pg_marg_run(c, true, n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed, cov_out, result);
}

icet_status icet_pose_graph_marginals_device(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                             const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, double* cov_out,
                                             icet_pose_graph_marginals_result* result) {
    return pg_marg_run(c, false, n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed, cov_out, result);
}

// Test hook: the marginals on host arrays with D, B, A, the band's selected inverse and the end nodes copied out.
icet_status icet_debug_pose_graph_marginals(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                            const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, icet_pose_graph_marginals_debug* out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!out || out->ends_capacity < 0 || out->reserved != 0) { c->err = "icet_debug_pose_graph_marginals: bad argument"; return ICET_ERR_BAD_ARG; }
    return pg_marg_run(c, true, n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed, nullptr, nullptr, out);
}

icet_status icet_pose_graph_optimize(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                     const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, const icet_pose_graph_options* opt,
                                     float* poses_out, double* poses64_out, double* edge_chi2, icet_pose_graph_result* result) {
    return pg_run(c, true, n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed, opt, poses_out, poses64_out, edge_chi2, result);
}

icet_status icet_pose_graph_optimize_device(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                            const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, const icet_pose_graph_options* opt,
                                            float* poses_out, double* poses64_out, double* edge_chi2, icet_pose_graph_result* result) {
    return pg_run(c, false, n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed, opt, poses_out, poses64_out, edge_chi2, result);
}

// Test hook: the optimiser's first iteration with its intermediate arrays copied out (pg_debug_step).  The host-pointer form's staging; nothing is finished.
icet_status icet_debug_pose_graph_step(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                       const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, const icet_pose_graph_options* opt,
                                       int32_t K, const double* p, icet_pose_graph_step* out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!out || K < 0 || (K > 0 && (!p || !out->q)) || out->cg_capacity < 0 || (out->cg_capacity > 0 && !out->cg_scalars)) { c->err = "icet_debug_pose_graph_step: bad argument"; return ICET_ERR_BAD_ARG; }
    return pg_run(c, true, n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed, opt, nullptr, nullptr, nullptr, nullptr, K, p, out);
}

// Test hook: the first iteration with the direct solve, its intermediate arrays copied out (pg_debug_direct_step).
icet_status icet_debug_pose_graph_direct(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                         const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, const icet_pose_graph_options* opt,
                                         int32_t K, const double* p, icet_pose_graph_direct_step* out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!out || K < 0 || (K > 0 && (!p || !out->q)) || out->ends_capacity < 0 || out->reserved != 0) { c->err = "icet_debug_pose_graph_direct: bad argument"; return ICET_ERR_BAD_ARG; }
    return pg_run(c, true, n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed, opt, nullptr, nullptr, nullptr, nullptr, K, p, nullptr, out);
}

// Test hook: one block-tridiagonal system through the optimiser's factor and sweeps.  diag, sub: n x 36 doubles (sub[k] is the block at (k, k - 1); sub[0] is not
// read as a coupling and should be zero), rhs and x: n x 6 doubles, all on the host.
icet_status icet_debug_block_tridiag(icet_ctx* c, int32_t n, const double* diag, const double* sub, const double* rhs, double* x, int32_t* status) {
    if (!c || !diag || !sub || !rhs || !x || !status || n < 1 || n > pg::kMaxNodes) return ICET_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n36 = (size_t)n * 36, n6 = (size_t)n * 6;
    double* d = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), sizeof(double) * (4 * n36 + 3 * n6 + 1)));
    double *dD = d, *dB = d + n36, *dG = dB + n36, *dW = dG + n36, *dr = dW + n36, *dx = dr + n6, *du = dx + n6;
    int32_t* ds = reinterpret_cast<int32_t*>(du + n6);
    hipError_t e = hipMemcpyAsync(dD, diag, sizeof(double) * n36, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dB, sub, sizeof(double) * n36, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dr, rhs, sizeof(double) * n6, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { hipLaunchKernelGGL(k_pg_block_tridiag, dim3(1), dim3(kPgThreads), 0, c->stream, (int)n, dD, dB, dr, dx, dG, dW, du, ds); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(x, dx, sizeof(double) * n6, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(status, ds, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (e != hipSuccess) { c->err = std::string("icet_debug_block_tridiag: ") + hipGetErrorString(e); return ICET_ERR_HIP; }
    return ICET_OK;
}
