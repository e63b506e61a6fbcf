// tests/cpp/posegraph_robust_host.h -- the HOST side of the pose graph's robust kernels (icet_amd/csrc/icet_posegraph_robust.h), beside posegraph_host.h: the
// backend that also loops over the robust bodies, and a graph bound with the robust run's arrays and the caller's weights, every one a heap block of its exact
// size.  Include it first (it includes posegraph_host.h, whose emulation macros stand ahead of the driver's include).
#pragma once
#include "posegraph_host.h"

struct RobustHostBackend : HostBackend {
    bool rgrid(PgRobustGridKernel k, int count, const PgArgs& a, const PgRobust& r) {
        launches++;
        for (int gi = 0; gi < count; gi++)
            switch (k) {
                case kPgRobustScale: pg_robust_scale(a, r, gi); break;
                case kPgRobustFinish: pg_robust_finish(a, r, gi); break;
            }
        return true;
    }
    bool rgroup(PgRobustGroupKernel k, const PgArgs& a, const PgRobust& r) {
        launches++;
        static PgRed red;
        workgroup([&]() {
            switch (k) {
                case kPgRobustStats: pg_group_robust_stats(a, r, red); break;
            }
        });
        return true;
    }
};

// HostBound with the robust run's arguments: pg_bind_robust's arrays with a kind, the caller's E weights.
struct RobustHostBound : HostBound {
    PgRobust rb{};
    std::unique_ptr<double[]> edge_weight;
    bool ok = false;          // the caller's struct is one the optimiser takes
    RobustHostBound(const HostGraph& g, bool direct, const icet_pose_graph_robust* robust) : HostBound(g, direct, true) {
        ok = pg_robust_args(robust, &rb);
        if (ok && rb.kind != pg::kRobustNone) pg_bind_robust(a, rb, al);
        edge_weight.reset(new double[g.E]);
        rb.weight_out = edge_weight.get();
    }
};
