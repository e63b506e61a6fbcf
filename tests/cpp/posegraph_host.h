// tests/cpp/posegraph_host.h -- the HOST side of the pose graph's driver, written once for the three host programs (test_posegraph_optimize.cpp,
// test_posegraph_direct.cpp, test_posegraph_marginals.cpp): the backend that loops where the device launches, the allocator that makes every work array a heap
// block of its exact size (so the address sanitizer sees any index the device would take out of bounds), the reader of one graph record and the binding of a
// graph to such blocks.  Plain build: a "workgroup" is one thread.  With -DICET_PG_EMU -pthread: four real threads and a barrier; the two must write the same
// bytes.  Include it first: the emulation's macros stand ahead of the driver's include.  A program calls pg_host_start() once before its first run.
#pragma once
#if defined(ICET_PG_EMU)
#include <pthread.h>
static thread_local int pg_emu_tid = 0;
static pthread_barrier_t pg_emu_barrier;
#define ICET_PG_EMU_THREADS 4
#define ICET_PG_DEV static inline
#define ICET_PG_TID pg_emu_tid
#define ICET_PG_SYNC() pthread_barrier_wait(&pg_emu_barrier)
#define ICET_PG_UNROLL
#endif
#include "icet_amd/csrc/icet_posegraph_driver.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#if defined(ICET_PG_EMU)
#include <thread>
#endif

using namespace icet;

inline void pg_host_start() {
#if defined(ICET_PG_EMU)
    pthread_barrier_init(&pg_emu_barrier, nullptr, ICET_PG_EMU_THREADS);
#endif
}

struct HostAlloc {
    std::vector<std::unique_ptr<double[]>> dd;
    std::vector<std::unique_ptr<int32_t[]>> ii;
    double* d(size_t n) { dd.emplace_back(new double[n]); return dd.back().get(); }
    int32_t* i(size_t n) { ii.emplace_back(new int32_t[n]); return ii.back().get(); }
};

struct HostBackend {
    long launches = 0;
    bool grid(PgGridKernel k, int count, const PgArgs& a) {
        launches++;
        for (int gi = 0; gi < count; gi++)
            switch (k) {
                case kPgInit: pg_init(a, gi); break;
                case kPgChi: pg_chi(a, gi); break;
                case kPgLinearise: pg_linearise(a, gi); break;
                case kPgAssemble: pg_assemble(a, gi); break;
                case kPgOffband: pg_offband(a, gi); break;
                case kPgHp: pg_hp(a, gi); break;
                case kPgRetract: pg_retract(a, gi); break;
                case kPgFinish: pg_finish(a, gi); break;
            }
        return true;
    }
    bool dgrid(PgDirectGridKernel k, int count, const PgArgs& a, const PgDirect& d) {
        launches++;
        for (int gi = 0; gi < count; gi++)
            switch (k) {
                case kPgZ: pg_z(a, d, gi); break;
                case kPgWm: pg_wm(a, d, gi); break;
                case kPgSl: pg_sl(a, d, gi); break;
                case kPgKs: pg_ks(a, d, gi); break;
                case kPgZw: pg_zw(a, d, gi); break;
                case kPgResid: pg_resid(a, d, gi); break;
            }
        return true;
    }
    bool mgrid(PgMargGridKernel k, int count, const PgArgs& a, const PgDirect& d, const PgMarg& mg) {
        launches++;
        for (int gi = 0; gi < count; gi++)
            switch (k) {
                case kPgSelinvPrep: pg_selinv_prep(a, mg, gi); break;
                case kPgMargLt: pg_marg_lt(a, d, mg, gi); break;
            }
        return true;
    }
    template <class Body> static void workgroup(Body body) {
#if defined(ICET_PG_EMU)
        std::vector<std::thread> th;
        for (int t = 0; t < kPgThreads; t++) th.emplace_back([&body, t]() { pg_emu_tid = t; body(); });
        for (auto& t : th) t.join();
#else
        body();
#endif
    }
    bool group(PgGroupKernel k, const PgArgs& a) {
        launches++;
        static PgShared sh;
        static PgRed red;
        workgroup([&]() {
            switch (k) {
                case kPgFactor: pg_group_factor(a, sh); break;
                case kPgPrecond: pg_group_precond(a, sh, red); break;
                case kPgStep: pg_group_step(a, red); break;
                case kPgStats: pg_group_stats(a, red); break;
            }
        });
        return true;
    }
    bool dgroup(PgDirectGroupKernel k, const PgArgs& a, const PgDirect& d) {
        launches++;
        static PgShared sh;
        workgroup([&]() {
            switch (k) {
                case kPgCholW: pg_group_chol(a, d, 0); break;
                case kPgCholK: pg_group_chol(a, d, 1); break;
                case kPgBand: pg_group_band(a, d, sh); break;
                case kPgCapSolve: pg_group_cap_solve(a, d); break;
            }
        });
        return true;
    }
    // the group body once per group index: the device runs them as the workgroups of one launch, here one behind the other
    bool mgroups(PgMargGroupKernel k, int groups, const PgArgs& a, const PgDirect& d, const PgMarg& mg) {
        launches++;
        static PgShared sh;
        static PgMargShared msh;
        for (int g = 0; g < groups; g++)
            workgroup([&]() {
                switch (k) {
                    case kPgSelinv: pg_group_selinv(a, mg, sh); break;
                    case kPgMargNode: pg_group_marg(a, d, mg, g, msh); break;
                }
            });
        return true;
    }
    bool scalars(const PgArgs& a, double out[kPgScalars]) { for (int i = 0; i < kPgScalars; i++) out[i] = a.sc[i]; return true; }
    bool fetch(void* host, const void* dev, size_t bytes) { memcpy(host, dev, bytes); return true; }
    bool put(void* dev, const void* host, size_t bytes) { memcpy(dev, host, bytes); return true; }
};

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }
// `count` doubles of NaN, a block of its own: an output of a hook, NaN where the run writes nothing
inline std::unique_ptr<double[]> nan_block(size_t count) { std::unique_ptr<double[]> p(new double[count]); for (size_t i = 0; i < count; i++) p[i] = std::nan(""); return p; }

// One graph record of IN (the format: test_posegraph_optimize.cpp) and the host's lists of it.
struct HostGraph {
    int n = 0, C = 0;
    size_t N = 0, Cc = 0, E = 0;
    icet_pose_graph_options o;
    std::vector<float> poses, odo_X, odo_info, clo_X, clo_info;
    std::vector<int32_t> ci, cj;
    std::vector<uint8_t> fixed;
    PgGraph graph;
    // false: the record is short or its closures are bad; said on stdout
    bool read(FILE* in) {
        int32_t hd[4]; double tol[3];
        if (fread(hd, 4, 4, in) != 4 || fread(tol, 8, 3, in) != 3) { printf("short header\n"); return false; }
        n = hd[0]; C = hd[1];
        N = (size_t)n; Cc = (size_t)C; E = (size_t)pg::edge_count(n, C);
        if (!rd(in, poses, N * 16) || !rd(in, odo_X, (N - 1) * 6) || !rd(in, odo_info, (N - 1) * 36) || !rd(in, ci, Cc) || !rd(in, cj, Cc) || !rd(in, clo_X, Cc * 6) ||
            !rd(in, clo_info, Cc * 36) || !rd(in, fixed, N)) { printf("short graph\n"); return false; }
        if (!pg::closures_ok(n, C, ci.data(), cj.data())) { printf("bad closures\n"); return false; }
        o = pg_default_options();
        o.gn_iters = hd[2]; o.max_pcg = hd[3]; o.dx_tol = tol[0]; o.damping = tol[1]; o.pcg_tol = tol[2];
        graph.build(n, C, ci.data(), cj.data(), fixed.data());
        return true;
    }
};

// A graph bound to heap blocks of the exact sizes: pg_bind's work arrays, with `direct` pg_bind_direct's, the graph's lists copied in, the caller's five arrays
// and, with `outputs`, the optimiser's three outputs (otherwise null: kPgFinish does not run).
struct HostBound {
    PgArgs a{};
    PgDirect dir{};
    HostAlloc al;
    std::unique_ptr<float[]> poses, odo_X, odo_info, clo_X, clo_info, poses_out;
    std::unique_ptr<double[]> poses64, edge_chi2;
    HostBound(const HostGraph& g, bool direct, bool outputs) {
        const size_t N = g.N, Cc = g.Cc, E = g.E, m = g.graph.ends.size();
        a.N = g.n; a.C = g.C; a.E = (int)E;
        const PgGraphDev gd = pg_bind(a, al, g.graph.items.size());
        if (E) { memcpy(gd.ei, g.graph.ei.data(), 4 * E); memcpy(gd.ej, g.graph.ej.data(), 4 * E); }
        memcpy(gd.off, g.graph.off.data(), 4 * (N + 1));
        if (!g.graph.items.empty()) memcpy(gd.items, g.graph.items.data(), 4 * g.graph.items.size());
        if (direct) {
            const PgDirectDev dd = pg_bind_direct(a, dir, al, m);
            if (m) memcpy(dd.ends, g.graph.ends.data(), 4 * m);
            memcpy(dd.end_of, g.graph.end_of.data(), 4 * N);
        }
        poses.reset(new float[N * 16]); odo_X.reset(new float[(N - 1) * 6]); odo_info.reset(new float[(N - 1) * 36]);
        clo_X.reset(new float[Cc * 6]); clo_info.reset(new float[Cc * 36]);
        memcpy(poses.get(), g.poses.data(), 4 * N * 16);
        if (N > 1) { memcpy(odo_X.get(), g.odo_X.data(), 4 * (N - 1) * 6); memcpy(odo_info.get(), g.odo_info.data(), 4 * (N - 1) * 36); }
        if (Cc) { memcpy(clo_X.get(), g.clo_X.data(), 4 * Cc * 6); memcpy(clo_info.get(), g.clo_info.data(), 4 * Cc * 36); }
        a.poses_in = poses.get(); a.odo_X = odo_X.get(); a.odo_info = odo_info.get(); a.clo_X = clo_X.get(); a.clo_info = clo_info.get();
        if (outputs) { poses_out.reset(new float[N * 16]); poses64.reset(new double[N * 12]); edge_chi2.reset(new double[2 * E]); }
        a.poses_out = poses_out.get(); a.poses64_out = poses64.get(); a.edge_chi2_out = edge_chi2.get();
    }
};
