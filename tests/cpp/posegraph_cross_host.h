// tests/cpp/posegraph_cross_host.h -- the HOST side of the pose graph's covariance columns and gate (icet_amd/csrc/icet_posegraph_cross.h), beside
// posegraph_host.h: the backend that also loops over their group bodies.  Include it first (it includes posegraph_host.h, whose emulation macros stand ahead
// of the driver's include).
#pragma once
#include "posegraph_host.h"

struct CrossHostBackend : HostBackend {
    // the group body once per group index: the device runs them as the workgroups of one launch, here one behind the other
    bool xgroups(PgCrossGroupKernel k, int groups, const PgArgs& a, const PgDirect& d, const PgMarg& mg, const PgCross& x, const PgGate& g) {
        launches++;
        static PgMargShared msh;
        static PgCrossShared xsh;
        static PgGateShared gsh;
        for (int i = 0; i < groups; i++)
            workgroup([&]() {
                switch (k) {
                    case kPgCrossTarget: pg_group_cross_target(a, d, mg, x, i, msh); break;
                    case kPgCrossNode: pg_group_cross_node(a, d, mg, x, i, xsh); break;
                    case kPgGateCand: pg_group_gate(a, mg, x, g, i, gsh); break;
                }
            });
        return true;
    }
};
