// icet_amd/csrc/icet_posegraph_cross.hip -- the kernels of the pose graph's covariance columns and gate (icet_posegraph_cross.h has the bodies, DESIGN.md
// section 20 "Covariance columns and the gate" the design) and their launch.  A translation unit of its own: the kernels of icet_posegraph.hip then compile as
// they did before these existed, instruction for instruction (scripts/isa_compare.py).  icet_posegraph.hip has the backend that calls pg_launch_cross and the
// entry points.
#include "icet_ctx.h"
#include "icet_posegraph_driver.h"

namespace icet {

// one workgroup per target, per node, per candidate
__global__ __launch_bounds__(kPgThreads) void k_pg_cross_target(PgArgs a, PgDirect d, PgMarg mg, PgCross x) { __shared__ PgMargShared sh; pg_group_cross_target(a, d, mg, x, (int)blockIdx.x, sh); }
__global__ __launch_bounds__(kPgThreads) void k_pg_cross_node(PgArgs a, PgDirect d, PgMarg mg, PgCross x) { __shared__ PgCrossShared sh; pg_group_cross_node(a, d, mg, x, (int)blockIdx.x, sh); }
__global__ __launch_bounds__(kPgThreads) void k_pg_gate(PgArgs a, PgMarg mg, PgCross x, PgGate g) { __shared__ PgGateShared sh; pg_group_gate(a, mg, x, g, (int)blockIdx.x, sh); }

// `groups` workgroups of the body k on the stream; nothing for groups <= 0
hipError_t pg_launch_cross(PgCrossGroupKernel k, int groups, hipStream_t stream, const PgArgs& a, const PgDirect& d, const PgMarg& mg, const PgCross& x, const PgGate& g) {
    if (groups <= 0) return hipSuccess;
    const dim3 grid((unsigned)groups), block((unsigned)kPgThreads);
    switch (k) {
        case kPgCrossTarget: hipLaunchKernelGGL(k_pg_cross_target, grid, block, 0, stream, a, d, mg, x); break;
        case kPgCrossNode:   hipLaunchKernelGGL(k_pg_cross_node, grid, block, 0, stream, a, d, mg, x); break;
        case kPgGateCand:    hipLaunchKernelGGL(k_pg_gate, grid, block, 0, stream, a, mg, x, g); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace icet
