// icet_amd/csrc/icet_posegraph.hip -- the pose-graph optimiser (include/icet_hip.h icet_pose_graph_optimize[_device]): the kernels, the
// device's backend of the driver, the entry points, and the band solve's test hook.
//
// The odometry chain of a pose graph makes its normal equations block tridiagonal with 6 x 6 blocks; every closure adds one block pair off the band.  The solve of
// the band is the kernel that matters: ONE workgroup of 256 threads factors it by block Cholesky and sweeps it forward and back (a block Thomas recurrence,
// sequential in the node index: one thread walks it, out of chunks of 32 nodes that all threads stage through LDS).  Around it: small kernels that each do one
// thing on plain global arrays, every body in icet_posegraph_body.h, driven from the host by icet_posegraph_driver.h.  No kernel waits on another block.
// Option "pg_solver" replaces the conjugate gradients by a direct solve over the closures' end nodes (icet_posegraph_direct.h): k_pg_z solves the band for
// all their unit columns in one launch, one thread per column.  icet_pose_graph_marginals[_device] reads the marginal covariance of every pose off that solve's
// Z, L and Lk and a selected inverse of the band (icet_posegraph_marginals.h).  icet_pose_graph_optimize_robust[_device] runs the same optimiser under a
// robust kernel (icet_posegraph_robust.h): three small kernels around the unchanged ones.  icet_pose_graph_covariance_columns[_device] and
// icet_pose_graph_gate[_device] run behind the marginals: the blocks (k, t) of H^-1 for a few target nodes, and the Mahalanobis test of candidate closures
// under them (icet_posegraph_cross.h the bodies, icet_posegraph_cross.hip their kernels).
#include "icet_ctx.h"
#include "icet_posegraph_driver.h"

#include <string>
#include <vector>

namespace icet {

__global__ __launch_bounds__(kPgThreads) void k_pg_block_tridiag(int N, const double* Dm, const double* Bm, const double* rhs, double* x, double* G, double* W, double* u, int32_t* status) {
    __shared__ PgShared sh;
    pg_block_tridiag(N, Dm, Bm, rhs, x, G, W, u, status, sh);
}

// grid kernels: one thread per global index below `count`, which follows the body's own arguments
constexpr int kPgGridThreads = 256;
#define ICET_PG_GRID_KERNEL(name, call, ...) \
    __global__ __launch_bounds__(kPgGridThreads) void name(__VA_ARGS__, int count) { \
        const int gi = (int)(blockIdx.x * kPgGridThreads + threadIdx.x); \
        if (gi < count) call; \
    }
ICET_PG_GRID_KERNEL(k_pg_init, pg_init(a, gi), PgArgs a)
ICET_PG_GRID_KERNEL(k_pg_chi, pg_chi(a, gi), PgArgs a)
ICET_PG_GRID_KERNEL(k_pg_linearise, pg_linearise(a, gi), PgArgs a)
ICET_PG_GRID_KERNEL(k_pg_assemble, pg_assemble(a, gi), PgArgs a)
ICET_PG_GRID_KERNEL(k_pg_offband, pg_offband(a, gi), PgArgs a)
ICET_PG_GRID_KERNEL(k_pg_hp, pg_hp(a, gi), PgArgs a)
ICET_PG_GRID_KERNEL(k_pg_retract, pg_retract(a, gi), PgArgs a)
ICET_PG_GRID_KERNEL(k_pg_finish, pg_finish(a, gi), PgArgs a)
// the direct solve (icet_posegraph_direct.h).  k_pg_z is the kernel that matters: one thread per column of Z walks the chain forward and back.
ICET_PG_GRID_KERNEL(k_pg_z, pg_z(a, d, gi), PgArgs a, PgDirect d)
ICET_PG_GRID_KERNEL(k_pg_wm, pg_wm(a, d, gi), PgArgs a, PgDirect d)
ICET_PG_GRID_KERNEL(k_pg_sl, pg_sl(a, d, gi), PgArgs a, PgDirect d)
ICET_PG_GRID_KERNEL(k_pg_ks, pg_ks(a, d, gi), PgArgs a, PgDirect d)
ICET_PG_GRID_KERNEL(k_pg_zw, pg_zw(a, d, gi), PgArgs a, PgDirect d)
ICET_PG_GRID_KERNEL(k_pg_resid, pg_resid(a, d, gi), PgArgs a, PgDirect d)
// the marginal covariances (icet_posegraph_marginals.h)
ICET_PG_GRID_KERNEL(k_pg_selinv_prep, pg_selinv_prep(a, mg, gi), PgArgs a, PgMarg mg)
ICET_PG_GRID_KERNEL(k_pg_marg_lt, pg_marg_lt(a, d, mg, gi), PgArgs a, PgDirect d, PgMarg mg)
// the robust kernels (icet_posegraph_robust.h)
ICET_PG_GRID_KERNEL(k_pg_robust_scale, pg_robust_scale(a, r, gi), PgArgs a, PgRobust r)
ICET_PG_GRID_KERNEL(k_pg_robust_finish, pg_robust_finish(a, r, gi), PgArgs a, PgRobust r)
#undef ICET_PG_GRID_KERNEL

// one-workgroup kernels
__global__ __launch_bounds__(kPgThreads) void k_pg_factor(PgArgs a) { __shared__ PgShared sh; pg_group_factor(a, sh); }
__global__ __launch_bounds__(kPgThreads) void k_pg_precond(PgArgs a) { __shared__ PgShared sh; __shared__ PgRed red; pg_group_precond(a, sh, red); }
__global__ __launch_bounds__(kPgThreads) void k_pg_step(PgArgs a) { __shared__ PgRed red; pg_group_step(a, red); }
__global__ __launch_bounds__(kPgThreads) void k_pg_stats(PgArgs a) { __shared__ PgRed red; pg_group_stats(a, red); }
__global__ __launch_bounds__(kPgThreads) void k_pg_chol(PgArgs a, PgDirect d, int which) { pg_group_chol(a, d, which); }
__global__ __launch_bounds__(kPgThreads) void k_pg_band(PgArgs a, PgDirect d) { __shared__ PgShared sh; pg_group_band(a, d, sh); }
__global__ __launch_bounds__(kPgThreads) void k_pg_cap_solve(PgArgs a, PgDirect d) { pg_group_cap_solve(a, d); }
__global__ __launch_bounds__(kPgThreads) void k_pg_robust_stats(PgArgs a, PgRobust r) { __shared__ PgRed red; pg_group_robust_stats(a, r, red); }
// k_pg_selinv is the marginals' sequential part; k_pg_marg runs one workgroup per node
__global__ __launch_bounds__(kPgThreads) void k_pg_selinv(PgArgs a, PgMarg mg) { __shared__ PgShared sh; pg_group_selinv(a, mg, sh); }
__global__ __launch_bounds__(kPgThreads) void k_pg_marg(PgArgs a, PgDirect d, PgMarg mg) { __shared__ PgMargShared sh; pg_group_marg(a, d, mg, (int)blockIdx.x, sh); }
// the covariance columns' and the gate's kernels and their launch: icet_posegraph_cross.hip
hipError_t pg_launch_cross(PgCrossGroupKernel k, int groups, hipStream_t stream, const PgArgs& a, const PgDirect& d, const PgMarg& mg, const PgCross& x, const PgGate& g);

namespace {

// The device's backend of the driver: launches on the context's stream; the scalars come back through pinned memory.
struct PgDeviceBackend {
    hipStream_t stream = nullptr;
    double* h_sc = nullptr;                 // pinned, kPgScalars
    hipError_t err = hipSuccess;
    bool ok(hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; return e == hipSuccess; }
    // THE launch rule: `blocks` workgroups of `threads` on the stream, nothing for blocks <= 0 (a count or a number of groups that is not positive)
    template <class... Params, class... Args>
    bool launch(void (*kernel)(Params...), int blocks, int threads, const Args&... args) {
        if (blocks <= 0) return true;
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)threads), 0, stream, args...);
        return ok(hipGetLastError());
    }
    static int blocks_for(int count) { return count <= 0 ? 0 : (count + kPgGridThreads - 1) / kPgGridThreads; }
    bool grid(PgGridKernel k, int count, const PgArgs& a) {
        void (*f)(PgArgs, int) = nullptr;
        switch (k) {
            case kPgInit:      f = k_pg_init; break;
            case kPgChi:       f = k_pg_chi; break;
            case kPgLinearise: f = k_pg_linearise; break;
            case kPgAssemble:  f = k_pg_assemble; break;
            case kPgOffband:   f = k_pg_offband; break;
            case kPgHp:        f = k_pg_hp; break;
            case kPgRetract:   f = k_pg_retract; break;
            case kPgFinish:    f = k_pg_finish; break;
        }
        return launch(f, blocks_for(count), kPgGridThreads, a, count);
    }
    bool group(PgGroupKernel k, const PgArgs& a) {
        void (*f)(PgArgs) = nullptr;
        switch (k) {
            case kPgFactor:  f = k_pg_factor; break;
            case kPgPrecond: f = k_pg_precond; break;
            case kPgStep:    f = k_pg_step; break;
            case kPgStats:   f = k_pg_stats; break;
        }
        return launch(f, 1, kPgThreads, a);
    }
    bool dgrid(PgDirectGridKernel k, int count, const PgArgs& a, const PgDirect& d) {
        void (*f)(PgArgs, PgDirect, int) = nullptr;
        switch (k) {
            case kPgZ:     f = k_pg_z; break;
            case kPgWm:    f = k_pg_wm; break;
            case kPgSl:    f = k_pg_sl; break;
            case kPgKs:    f = k_pg_ks; break;
            case kPgZw:    f = k_pg_zw; break;
            case kPgResid: f = k_pg_resid; break;
        }
        return launch(f, blocks_for(count), kPgGridThreads, a, d, count);
    }
    bool dgroup(PgDirectGroupKernel k, const PgArgs& a, const PgDirect& d) {
        switch (k) {
            case kPgCholW:    return launch(k_pg_chol, 1, kPgThreads, a, d, 0);
            case kPgCholK:    return launch(k_pg_chol, 1, kPgThreads, a, d, 1);
            case kPgBand:     return launch(k_pg_band, 1, kPgThreads, a, d);
            case kPgCapSolve: return launch(k_pg_cap_solve, 1, kPgThreads, a, d);
        }
        return false;
    }
    bool mgrid(PgMargGridKernel k, int count, const PgArgs& a, const PgDirect& d, const PgMarg& mg) {
        switch (k) {
            case kPgSelinvPrep: return launch(k_pg_selinv_prep, blocks_for(count), kPgGridThreads, a, mg, count);
            case kPgMargLt:     return launch(k_pg_marg_lt, blocks_for(count), kPgGridThreads, a, d, mg, count);
        }
        return false;
    }
    bool mgroups(PgMargGroupKernel k, int groups, const PgArgs& a, const PgDirect& d, const PgMarg& mg) {
        switch (k) {
            case kPgSelinv:   return launch(k_pg_selinv, groups <= 0 ? 0 : 1, kPgThreads, a, mg);
            case kPgMargNode: return launch(k_pg_marg, groups, kPgThreads, a, d, mg);
        }
        return false;
    }
    bool xgroups(PgCrossGroupKernel k, int groups, const PgArgs& a, const PgDirect& d, const PgMarg& mg, const PgCross& x, const PgGate& g) {
        return ok(pg_launch_cross(k, groups, stream, a, d, mg, x, g));
    }
    bool rgrid(PgRobustGridKernel k, int count, const PgArgs& a, const PgRobust& r) {
        switch (k) {
            case kPgRobustScale:  return launch(k_pg_robust_scale, blocks_for(count), kPgGridThreads, a, r, count);
            case kPgRobustFinish: return launch(k_pg_robust_finish, blocks_for(count), kPgGridThreads, a, r, count);
        }
        return false;
    }
    bool rgroup(PgRobustGroupKernel k, const PgArgs& a, const PgRobust& r) {
        switch (k) {
            case kPgRobustStats: return launch(k_pg_robust_stats, 1, kPgThreads, a, r);
        }
        return false;
    }
    bool scalars(const PgArgs& a, double out[kPgScalars]) {
        if (!ok(hipMemcpyAsync(h_sc, a.sc, sizeof(double) * kPgScalars, hipMemcpyDeviceToHost, stream)) || !ok(hipStreamSynchronize(stream))) return false;
        for (int i = 0; i < kPgScalars; i++) out[i] = h_sc[i];
        return true;
    }
    // (the test hooks' copies, and the robust run's weights at its end: pageable host memory, complete on return)
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
    void align8() { used = (used + 7) & ~(size_t)7; }
};

// What the caller describes: the chain, its closures and the nodes that stay.  Every entry point fills one.
struct PgProblem {
    int32_t n; const float *poses, *odo_X, *odo_info;
    int32_t n_closures; const int32_t *ci, *cj; const float *clo_X, *clo_info;
    const uint8_t* fixed;
};

// One run on the device (pg_run, below).  The entry point names it and says where the arrays are; its plan sets what is bound and staged; its body finds the
// graph, the bound arguments and the backend here.
struct PgFrame {
    icet_ctx* c; const char* name;          // the entry the error texts name
    bool host_io;                           // the problem's arrays and the outputs are the host's: staged in the block (false: device pointers, used as they are)
    PgProblem pb;
    PgGraph graph; int m_ends = 0;          // (from the checks on)
    // the plan: the work arrays bound beyond pg_bind's, and with host_io the outputs staged in the block (a.poses_out, a.poses64_out, a.edge_chi2_out; null otherwise)
    // robust: the robust run's own arrays (a run with a kind); stage_weight: with host_io its edge weights staged in the block (rb.weight_out)
    bool direct = false, marg = false, stage_poses_out = false, stage_poses64 = false, stage_chi2 = false, robust = false, stage_weight = false;
    // cross: the covariance columns' arrays for `targets`; marg_own_cov / own_cols: cov and cols staged in the block whatever host_io says; gate: the gate's
    // lists for g_i, g_j, g_tcol, with host_io its measurements (cand_X, cand_cov: the caller's) and outputs staged; gate_S: the residual covariances asked for
    bool cross = false, marg_own_cov = false, own_cols = false, gate = false, gate_S = false;
    std::vector<int32_t> targets, g_i, g_j, g_tcol;
    const float *cand_X = nullptr, *cand_cov = nullptr;
    PgArgs a{}; PgDirect dir{}; PgMarg mg{}; PgRobust rb{}; PgCross x{}; PgGate gt{};
    PgDeviceBackend be;
    hipError_t e = hipSuccess;              // the first failure of a copy or of the backend
    PgFrame(icet_ctx* c_, const char* name_, bool host_io_, const PgProblem& pb_) : c(c_), name(name_), host_io(host_io_), pb(pb_) {}
    // a result from the block to the host, behind the kernels on the stream (a null dst is skipped)
    void down(void* dst, const void* src, size_t nbytes) { if (e == hipSuccess && dst && nbytes) e = hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost, c->stream); }
};

// THE frame of every pose-graph entry: the checks of the problem (outputs_ok: the entry's own output pointers are there), the graph, then plan() -- the entry's
// own checks behind the graph's, and f's plan --, ONE device block for everything bound and staged, the uploads, body() -- the driver's call and f.down() of
// what goes back; false for a failure of the backend --, the synchronisation and the error mapping.  The block's order: pg_bind | direct | marginals | robust |
// columns | gate | staging,
// the doubles first.  A local BufferGroup owns the block and the pinned scalars: every return frees through it.
template <class Plan, class Body>
icet_status pg_run(PgFrame& f, bool outputs_ok, Plan&& plan, Body&& body) {
    icet_ctx* c = f.c;
    ICET_TRY(enter(c));
    const PgProblem& pb = f.pb;
    const std::string name = f.name;
    const int32_t n = pb.n, n_closures = pb.n_closures;
    if (!pb.poses || !outputs_ok || n < 1 || n > pg::kMaxNodes || n_closures < 0 || n_closures > pg::kMaxClosures) { c->err = name + ": bad argument"; return ICET_ERR_BAD_ARG; }
    if ((n > 1 && (!pb.odo_X || !pb.odo_info)) || (n_closures > 0 && (!pb.ci || !pb.cj || !pb.clo_X || !pb.clo_info))) { c->err = name + ": null array"; return ICET_ERR_BAD_ARG; }
    if (!pg::closures_ok(n, n_closures, pb.ci, pb.cj)) { c->err = name + ": a closure's ends are out of range or equal"; return ICET_ERR_BAD_ARG; }
    PgGraph& graph = f.graph;
    graph.build(n, n_closures, pb.ci, pb.cj, pb.fixed);
    f.m_ends = (int)graph.ends.size();
    ICET_TRY(plan());

    PgArgs& a = f.a;
    a.N = n; a.C = n_closures; a.E = pg::edge_count(n, n_closures);
    const size_t N = (size_t)n, E = (size_t)a.E, C = (size_t)n_closures, n_items = graph.items.size(), m = (size_t)f.m_ends;
    PgArena arena;
    PgGraphDev gd{};
    PgDirectDev dd{};
    PgCrossDev xd{};
    PgGateDev gtd{};
    float *s_cand_X = nullptr, *s_cand_cov = nullptr;
    float *s_poses = nullptr, *s_odo_X = nullptr, *s_odo_info = nullptr, *s_clo_X = nullptr, *s_clo_info = nullptr;      // the staging of the problem's arrays
    auto layout = [&]() {
        arena.used = 0;
        gd = pg_bind(a, arena, n_items);
        if (f.direct) { arena.align8(); dd = pg_bind_direct(a, f.dir, arena, m); }
        if (f.marg) { arena.align8(); pg_bind_marg(a, f.dir, f.mg, arena, f.host_io || f.marg_own_cov); }
        if (f.robust) { arena.align8(); pg_bind_robust(a, f.rb, arena); }
        if (f.cross) { arena.align8(); xd = pg_bind_cross(a, f.dir, f.x, arena, (int)f.targets.size(), f.host_io || f.own_cols); }
        if (f.gate) {
            arena.align8(); gtd = pg_bind_gate(f.gt, arena, (int)f.g_i.size(), f.host_io, f.gate_S);
            if (f.host_io) { s_cand_X = arena.f(f.g_i.size() * 6); s_cand_cov = arena.f(f.g_i.size() * 36); }
        }
        a.poses_out = nullptr; a.poses64_out = nullptr; a.edge_chi2_out = nullptr;
        if (f.host_io) {
            arena.align8();          // (int32 lists end on a multiple of 4 bytes; the doubles of the staging need 8)
            if (f.stage_poses64) a.poses64_out = arena.d(N * 12);
            if (f.stage_chi2) a.edge_chi2_out = arena.d(2 * E);
            if (f.stage_weight) f.rb.weight_out = arena.d(E);
            s_poses = arena.f(N * 16); s_odo_X = arena.f((N - 1) * 6); s_odo_info = arena.f((N - 1) * 36); s_clo_X = arena.f(C * 6); s_clo_info = arena.f(C * 36);
            if (f.stage_poses_out) a.poses_out = arena.f(N * 16);
        }
    };
    layout();
    const size_t bytes = arena.used;
    BufferGroup bufs;
    char* block = nullptr;
    HIPCHK(c, bufs.device(block, bytes));
    arena.base = block;
    layout();

    f.be.stream = c->stream;
    f.e = static_cast<hipError_t>(bufs.pinned(f.be.h_sc, (size_t)kPgScalars, hipHostMallocDefault));
    auto up = [&](void* dst, const void* src, size_t nbytes) { if (f.e == hipSuccess && nbytes) f.e = hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice, c->stream); };
    up(gd.ei, graph.ei.data(), sizeof(int32_t) * E); up(gd.ej, graph.ej.data(), sizeof(int32_t) * E);
    up(gd.off, graph.off.data(), sizeof(int32_t) * (N + 1)); up(gd.items, graph.items.data(), sizeof(int32_t) * n_items);
    if (f.direct) { up(dd.ends, graph.ends.data(), sizeof(int32_t) * m); up(dd.end_of, graph.end_of.data(), sizeof(int32_t) * N); }
    if (f.cross) up(xd.targets, f.targets.data(), sizeof(int32_t) * f.targets.size());
    if (f.gate) {
        const size_t nc = f.g_i.size();
        up(gtd.gi, f.g_i.data(), sizeof(int32_t) * nc); up(gtd.gj, f.g_j.data(), sizeof(int32_t) * nc); up(gtd.tcol, f.g_tcol.data(), sizeof(int32_t) * nc);
        if (f.host_io) { up(s_cand_X, f.cand_X, sizeof(float) * nc * 6); up(s_cand_cov, f.cand_cov, sizeof(float) * nc * 36); f.gt.X = s_cand_X; f.gt.cov = s_cand_cov; }
        else { f.gt.X = f.cand_X; f.gt.cov = f.cand_cov; }
    }
    if (f.host_io) {
        up(s_poses, pb.poses, sizeof(float) * N * 16); up(s_odo_X, pb.odo_X, sizeof(float) * (N - 1) * 6); up(s_odo_info, pb.odo_info, sizeof(float) * (N - 1) * 36);
        up(s_clo_X, pb.clo_X, sizeof(float) * C * 6); up(s_clo_info, pb.clo_info, sizeof(float) * C * 36);
        a.poses_in = s_poses; a.odo_X = s_odo_X; a.odo_info = s_odo_info; a.clo_X = s_clo_X; a.clo_info = s_clo_info;
    } else {
        a.poses_in = pb.poses; a.odo_X = pb.odo_X; a.odo_info = pb.odo_info; a.clo_X = pb.clo_X; a.clo_info = pb.clo_info;
    }
    // (the graph's lists and the caller's arrays outlive the synchronisation below; the stream orders the copies before the kernels)
    if (f.e == hipSuccess && !body()) f.e = f.be.err;
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (f.e == hipSuccess) f.e = es;
    if (f.e != hipSuccess) { c->err = name + ": " + hipGetErrorString(f.e); return f.e == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; }
    return ICET_OK;
}

// ---- the optimiser: icet_pose_graph_optimize[_device] and its two hooks, which report under its name ----------------------------------------------------------
constexpr const char* kPgOptimiseName = "icet_pose_graph_optimize";

// The options (null: the defaults), the first check of every optimiser plan
icet_status pg_options(icet_ctx* c, const icet_pose_graph_options* opt, icet_pose_graph_options* o, const char* name = kPgOptimiseName) {
    *o = opt ? *opt : pg_default_options();
    if (o->gn_iters < 1) { c->err = std::string(name) + ": gn_iters < 1"; return ICET_ERR_BAD_ARG; }
    return ICET_OK;
}
// The direct solve's limit on the end nodes
icet_status pg_direct_limit(icet_ctx* c, int m_ends, const char* name = kPgOptimiseName) {
    if (m_ends <= kPgDirectMaxEnds) return ICET_OK;
    c->err = std::string(name) + ": the direct solve takes at most " + std::to_string(kPgDirectMaxEnds) + " end nodes of closures off the band, this graph has " +
             std::to_string(m_ends) + " (option pg_solver 2 falls back to conjugate gradients)";
    return ICET_ERR_UNSUPPORTED;
}
// A hook's ends_capacity against the graph's count
icet_status pg_ends_capacity(icet_ctx* c, const char* hook, int32_t capacity, int m_ends) {
    if (capacity == m_ends) return ICET_OK;
    c->err = std::string(hook) + ": ends_capacity is not the graph's count of end nodes (" + std::to_string(m_ends) + ")";
    return ICET_ERR_BAD_ARG;
}

// The plan of an optimiser run, plain or robust: the options, then the linear solve by the context's option "pg_solver" (0 conjugate gradients, 1 the direct
// solve, 2 the direct solve where the graph has end nodes within its limit), then the three outputs staged.
icet_status pg_optimise_plan(PgFrame& f, const icet_pose_graph_options* opt, icet_pose_graph_options* o, const double* poses64_out, const double* edge_chi2) {
    icet_ctx* c = f.c;
    ICET_TRY(pg_options(c, opt, o, f.name));
    if (c->pg_solver == 1) ICET_TRY(pg_direct_limit(c, f.m_ends, f.name));
    f.direct = c->pg_solver == 1 || (c->pg_solver == 2 && f.m_ends >= 1 && f.m_ends <= kPgDirectMaxEnds);
    f.stage_poses_out = true; f.stage_poses64 = poses64_out != nullptr; f.stage_chi2 = edge_chi2 != nullptr;
    return ICET_OK;
}

icet_status pg_optimise_entry(icet_ctx* c, bool host_io, const PgProblem& pb, const icet_pose_graph_options* opt, float* poses_out, double* poses64_out,
                              double* edge_chi2, icet_pose_graph_result* result) {
    PgFrame f(c, kPgOptimiseName, host_io, pb);
    icet_pose_graph_options o;
    icet_pose_graph_result res{};
    ICET_TRY(pg_run(f, poses_out && result,
        [&]() { return pg_optimise_plan(f, opt, &o, poses64_out, edge_chi2); },
        [&]() {
            const size_t N = (size_t)f.a.N, E = (size_t)f.a.E;
            if (!host_io) { f.a.poses_out = poses_out; f.a.poses64_out = poses64_out; f.a.edge_chi2_out = edge_chi2; }
            if (!(f.direct ? pg_optimise_direct(f.be, f.a, f.dir, o, &res) : pg_optimise(f.be, f.a, o, f.graph.c_offband, &res))) return false;
            if (host_io) { f.down(poses_out, f.a.poses_out, sizeof(float) * N * 16); f.down(poses64_out, f.a.poses64_out, sizeof(double) * N * 12); f.down(edge_chi2, f.a.edge_chi2_out, sizeof(double) * 2 * E); }
            return true;
        }));
    *result = res;
    return ICET_OK;
}

// ---- the robust run: icet_pose_graph_optimize_robust[_device].  The plan of pg_optimise_entry, the robust arrays bound with a kind, the weights staged. -----------
icet_status pg_robust_entry(icet_ctx* c, bool host_io, const PgProblem& pb, const icet_pose_graph_options* opt, const icet_pose_graph_robust* robust, float* poses_out,
                            double* poses64_out, double* edge_chi2, double* edge_weight, icet_pose_graph_robust_result* result) {
    constexpr const char* kName = "icet_pose_graph_optimize_robust";
    PgFrame f(c, kName, host_io, pb);
    icet_pose_graph_options o;
    icet_pose_graph_robust_result res{};
    ICET_TRY(pg_run(f, poses_out && result,
        [&]() {
            ICET_TRY(pg_optimise_plan(f, opt, &o, poses64_out, edge_chi2));
            if (!pg_robust_args(robust, &f.rb)) { c->err = std::string(kName) + ": the kind, the flags or the scale of `robust` is not one the optimiser takes"; return ICET_ERR_BAD_ARG; }
            f.robust = f.rb.kind != pg::kRobustNone;
            f.stage_weight = edge_weight != nullptr;
            return ICET_OK;
        },
        [&]() {
            const size_t N = (size_t)f.a.N, E = (size_t)f.a.E;
            if (!host_io) { f.a.poses_out = poses_out; f.a.poses64_out = poses64_out; f.a.edge_chi2_out = edge_chi2; f.rb.weight_out = edge_weight; }
            if (!pg_optimise_robust(f.be, f.a, f.dir, f.direct, o, f.graph.c_offband, f.rb, &res)) return false;
            if (host_io) {
                f.down(poses_out, f.a.poses_out, sizeof(float) * N * 16); f.down(poses64_out, f.a.poses64_out, sizeof(double) * N * 12);
                f.down(edge_chi2, f.a.edge_chi2_out, sizeof(double) * 2 * E); f.down(edge_weight, f.rb.weight_out, sizeof(double) * E);
            }
            return true;
        }));
    *result = res;
    return ICET_OK;
}

// ---- the marginal covariances: icet_pose_graph_marginals[_device] and, with dbg, its hook (D, B, A, the band's selected inverse and the end nodes copied out) ------
icet_status pg_marginals_entry(icet_ctx* c, bool host_io, const PgProblem& pb, double* cov_out, icet_pose_graph_marginals_result* result,
                               icet_pose_graph_marginals_debug* dbg = nullptr) {
    PgFrame f(c, "icet_pose_graph_marginals", host_io, pb);
    icet_pose_graph_marginals_result res{};
    ICET_TRY(pg_run(f, dbg || (cov_out && result),
        [&]() {
            if (f.m_ends > kPgDirectMaxEnds) {
                c->err = "icet_pose_graph_marginals: at most " + std::to_string(kPgDirectMaxEnds) + " end nodes of closures off the band, this graph has " + std::to_string(f.m_ends);
                return ICET_ERR_UNSUPPORTED;
            }
            if (dbg) ICET_TRY(pg_ends_capacity(c, "icet_debug_pose_graph_marginals", dbg->ends_capacity, f.m_ends));
            f.direct = true; f.marg = true;          // (the block stages cov with host_io: pg_bind_marg; kPgFinish does not run, so none of its outputs)
            return ICET_OK;
        },
        [&]() {
            if (!host_io) f.mg.cov = cov_out;
            PgMargTap tap;
            if (dbg) { tap.D = dbg->D; tap.B = dbg->B; tap.A = dbg->A; tap.band_cov = dbg->band_cov; }
            if (!pg_marginals(f.be, f.a, f.dir, f.mg, &res, dbg ? &tap : nullptr)) return false;
            if (host_io) f.down(dbg ? dbg->cov : cov_out, f.mg.cov, sizeof(double) * (size_t)f.a.N * 36);
            return true;
        }));
    if (dbg) {
        dbg->result = res;
        if (dbg->ends) for (int i = 0; i < f.m_ends; i++) dbg->ends[i] = f.graph.ends[(size_t)i];
    }
    if (result) *result = res;
    return ICET_OK;
}

// ---- the covariance columns and the gate: icet_pose_graph_covariance_columns[_device], icet_pose_graph_gate[_device] --------------------------------------------
// The plan both share: the marginals' limit, then the targets -- 1 .. 32 distinct nodes in range.
icet_status pg_columns_plan(PgFrame& f, const char* name) {
    icet_ctx* c = f.c;
    if (f.m_ends > kPgDirectMaxEnds) {
        c->err = std::string(name) + ": at most " + std::to_string(kPgDirectMaxEnds) + " end nodes of closures off the band, this graph has " + std::to_string(f.m_ends);
        return ICET_ERR_UNSUPPORTED;
    }
    const size_t T = f.targets.size();
    if (T < 1 || T > (size_t)kPgCrossMaxTargets) { c->err = std::string(name) + ": 1 .. " + std::to_string(kPgCrossMaxTargets) + " distinct target nodes"; return ICET_ERR_BAD_ARG; }
    std::vector<uint8_t> seen((size_t)f.pb.n, 0);
    for (int32_t t : f.targets) {
        if (t < 0 || t >= f.pb.n || seen[(size_t)t]) { c->err = std::string(name) + ": a target is out of range or named twice"; return ICET_ERR_BAD_ARG; }
        seen[(size_t)t] = 1;
    }
    f.direct = true; f.marg = true; f.cross = true;
    return ICET_OK;
}

icet_status pg_columns_entry(icet_ctx* c, bool host_io, const PgProblem& pb, int32_t n_targets, const int32_t* targets, double* cols_out, double* cov_out,
                             icet_pose_graph_marginals_result* result) {
    constexpr const char* kName = "icet_pose_graph_covariance_columns";
    PgFrame f(c, kName, host_io, pb);
    icet_pose_graph_marginals_result res{};
    const bool have = targets && cols_out && result && n_targets >= 1 && n_targets <= kPgCrossMaxTargets;
    if (have) f.targets.assign(targets, targets + n_targets);
    ICET_TRY(pg_run(f, have,
        [&]() { f.marg_own_cov = cov_out == nullptr; return pg_columns_plan(f, kName); },
        [&]() {
            const size_t N = (size_t)f.a.N;
            if (!host_io) { f.x.cols = cols_out; if (cov_out) f.mg.cov = cov_out; }
            if (!pg_columns(f.be, f.a, f.dir, f.mg, f.x, &res)) return false;
            if (host_io) { f.down(cols_out, f.x.cols, sizeof(double) * (size_t)n_targets * N * 36); f.down(cov_out, f.mg.cov, sizeof(double) * N * 36); }
            return true;
        }));
    *result = res;
    return ICET_OK;
}

icet_status pg_gate_entry(icet_ctx* c, bool host_io, const PgProblem& pb, int32_t n_cand, const int32_t* gi, const int32_t* gj, const float* cand_X,
                          const float* cand_cov, double threshold, double* d2_out, double* res_cov_out, int32_t* cand_status, icet_pose_graph_gate_result* result) {
    constexpr const char* kName = "icet_pose_graph_gate";
    PgFrame f(c, kName, host_io, pb);
    icet_pose_graph_gate_result res{};
    const bool have = gi && gj && cand_X && cand_cov && d2_out && cand_status && result && n_cand >= 1 && n_cand <= kPgGateMaxCand;
    ICET_TRY(pg_run(f, have,
        [&]() {
            // the targets: the distinct live nodes, ascending
            if (!pg_gate_targets(pb.n, n_cand, gi, gj, f.targets, f.g_tcol)) { c->err = std::string(kName) + ": a candidate's ends are out of range or equal"; return ICET_ERR_BAD_ARG; }
            if (f.targets.size() > (size_t)kPgCrossMaxTargets) { c->err = std::string(kName) + ": the candidates have more than " + std::to_string(kPgCrossMaxTargets) + " distinct live nodes"; return ICET_ERR_BAD_ARG; }
            f.g_i.assign(gi, gi + n_cand); f.g_j.assign(gj, gj + n_cand);
            f.cand_X = cand_X; f.cand_cov = cand_cov;
            f.gate = true; f.gate_S = res_cov_out != nullptr; f.marg_own_cov = true; f.own_cols = true;
            return pg_columns_plan(f, kName);
        },
        [&]() {
            const size_t nc = (size_t)n_cand;
            if (!host_io) { f.gt.d2 = d2_out; f.gt.S = res_cov_out; f.gt.status = cand_status; }
            if (!pg_gate(f.be, f.a, f.dir, f.mg, f.x, f.gt, threshold > 0.0 ? threshold : pg::kRobustDefaultScale, &res)) return false;
            if (host_io) { f.down(d2_out, f.gt.d2, sizeof(double) * nc); f.down(res_cov_out, f.gt.S, sizeof(double) * nc * 36); f.down(cand_status, f.gt.status, sizeof(int32_t) * nc); }
            return true;
        }));
    *result = res;
    return ICET_OK;
}

}  // namespace
}  // namespace icet

using namespace icet;

icet_status icet_pose_graph_covariance_columns(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                               const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                               int32_t n_targets, const int32_t* targets, double* cols_out, double* cov_out,
                                               icet_pose_graph_marginals_result* result) {
    return pg_columns_entry(c, true, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, n_targets, targets, cols_out, cov_out, result);
}

icet_status icet_pose_graph_covariance_columns_device(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                                      const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                                      int32_t n_targets, const int32_t* targets, double* cols_out, double* cov_out,
                                                      icet_pose_graph_marginals_result* result) {
    return pg_columns_entry(c, false, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, n_targets, targets, cols_out, cov_out, result);
}

icet_status icet_pose_graph_gate(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                 const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, int32_t n_cand, const int32_t* gi,
                                 const int32_t* gj, const float* cand_X, const float* cand_cov, double threshold, double* d2_out, double* res_cov_out,
                                 int32_t* cand_status, icet_pose_graph_gate_result* result) {
    return pg_gate_entry(c, true, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, n_cand, gi, gj, cand_X, cand_cov, threshold, d2_out,
                         res_cov_out, cand_status, result);
}

icet_status icet_pose_graph_gate_device(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                        const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, int32_t n_cand, const int32_t* gi,
                                        const int32_t* gj, const float* cand_X, const float* cand_cov, double threshold, double* d2_out, double* res_cov_out,
                                        int32_t* cand_status, icet_pose_graph_gate_result* result) {
    return pg_gate_entry(c, false, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, n_cand, gi, gj, cand_X, cand_cov, threshold, d2_out,
                         res_cov_out, cand_status, result);
}

// Every entry point hands the eleven arguments that describe the graph on as one PgProblem.
icet_status icet_pose_graph_marginals(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                      const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, double* cov_out,
                                      icet_pose_graph_marginals_result* result) {
    return pg_marginals_entry(c, true, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, cov_out, result);
}

icet_status icet_pose_graph_marginals_device(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                             const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, double* cov_out,
                                             icet_pose_graph_marginals_result* result) {
    return pg_marginals_entry(c, false, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, cov_out, result);
}

// Test hook: the marginals on host arrays with D, B, A, the band's selected inverse and the end nodes copied out.
icet_status icet_debug_pose_graph_marginals(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                            const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                            icet_pose_graph_marginals_debug* out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!out || out->ends_capacity < 0 || out->reserved != 0) { c->err = "icet_debug_pose_graph_marginals: bad argument"; return ICET_ERR_BAD_ARG; }
    return pg_marginals_entry(c, true, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, nullptr, nullptr, out);
}

icet_status icet_pose_graph_optimize(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                     const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, const icet_pose_graph_options* opt,
                                     float* poses_out, double* poses64_out, double* edge_chi2, icet_pose_graph_result* result) {
    return pg_optimise_entry(c, true, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, opt, poses_out, poses64_out, edge_chi2, result);
}

icet_status icet_pose_graph_optimize_device(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                            const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                            const icet_pose_graph_options* opt, float* poses_out, double* poses64_out, double* edge_chi2,
                                            icet_pose_graph_result* result) {
    return pg_optimise_entry(c, false, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, opt, poses_out, poses64_out, edge_chi2, result);
}

icet_status icet_pose_graph_optimize_robust(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                            const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, const icet_pose_graph_options* opt,
                                            const icet_pose_graph_robust* robust, float* poses_out, double* poses64_out, double* edge_chi2, double* edge_weight,
                                            icet_pose_graph_robust_result* result) {
    return pg_robust_entry(c, true, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, opt, robust, poses_out, poses64_out, edge_chi2,
                           edge_weight, result);
}

icet_status icet_pose_graph_optimize_robust_device(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                                   const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                                   const icet_pose_graph_options* opt, const icet_pose_graph_robust* robust, float* poses_out, double* poses64_out,
                                                   double* edge_chi2, double* edge_weight, icet_pose_graph_robust_result* result) {
    return pg_robust_entry(c, false, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed}, opt, robust, poses_out, poses64_out, edge_chi2,
                           edge_weight, result);
}

// Test hook: the optimiser's first iteration with its intermediate arrays copied out (pg_debug_step): conjugate gradients whatever "pg_solver" says.  The
// host-pointer form's staging; nothing is finished.
icet_status icet_debug_pose_graph_step(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                       const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, const icet_pose_graph_options* opt,
                                       int32_t K, const double* p, icet_pose_graph_step* out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!out || K < 0 || (K > 0 && (!p || !out->q)) || out->cg_capacity < 0 || (out->cg_capacity > 0 && !out->cg_scalars)) { c->err = "icet_debug_pose_graph_step: bad argument"; return ICET_ERR_BAD_ARG; }
    PgFrame f(c, kPgOptimiseName, true, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed});
    icet_pose_graph_options o;
    return pg_run(f, true,
        [&]() { ICET_TRY(pg_options(c, opt, &o)); f.stage_poses_out = true; return ICET_OK; },
        [&]() { return pg_debug_step(f.be, f.a, o, f.graph.c_offband, K, p, out); });
}

// Test hook: the first iteration with the direct solve, its intermediate arrays copied out (pg_debug_direct_step).
icet_status icet_debug_pose_graph_direct(icet_ctx* c, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                         const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, const icet_pose_graph_options* opt,
                                         int32_t K, const double* p, icet_pose_graph_direct_step* out) {
    if (!c) return ICET_ERR_BAD_ARG;
    if (!out || K < 0 || (K > 0 && (!p || !out->q)) || out->ends_capacity < 0 || out->reserved != 0) { c->err = "icet_debug_pose_graph_direct: bad argument"; return ICET_ERR_BAD_ARG; }
    PgFrame f(c, kPgOptimiseName, true, PgProblem{n, poses, odo_X, odo_info, n_closures, ci, cj, clo_X, clo_info, fixed});
    icet_pose_graph_options o;
    return pg_run(f, true,
        [&]() {
            ICET_TRY(pg_options(c, opt, &o));
            ICET_TRY(pg_direct_limit(c, f.m_ends));
            ICET_TRY(pg_ends_capacity(c, "icet_debug_pose_graph_direct", out->ends_capacity, f.m_ends));
            f.direct = true; f.stage_poses_out = true;
            return ICET_OK;
        },
        [&]() { return pg_debug_direct_step(f.be, f.a, f.dir, o, K, p, out); });
}

// Test hook: one block-tridiagonal system through the optimiser's factor and sweeps.  diag, sub: n x 36 doubles (sub[k] is the block at (k, k - 1); sub[0] is not
// read as a coupling and should be zero), rhs and x: n x 6 doubles, all on the host.
icet_status icet_debug_block_tridiag(icet_ctx* c, int32_t n, const double* diag, const double* sub, const double* rhs, double* x, int32_t* status) {
    if (!c || !diag || !sub || !rhs || !x || !status || n < 1 || n > pg::kMaxNodes) return ICET_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n36 = (size_t)n * 36, n6 = (size_t)n * 6;
    double* d = nullptr; BufferGroup g;                                      // (freed at every return: behind the synchronisation below)
    HIPCHK(c, g.device(d, 4 * n36 + 3 * n6 + 1));
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
    if (e != hipSuccess) { c->err = std::string("icet_debug_block_tridiag: ") + hipGetErrorString(e); return ICET_ERR_HIP; }
    return ICET_OK;
}
