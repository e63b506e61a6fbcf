// icet_amd/csrc/icet_posegraph.hip -- the block-tridiagonal solve a pose-graph optimiser needs, behind a test hook.
//
// The odometry chain of a pose graph makes its normal equations block tridiagonal with 6 x 6 blocks; every closure adds one block pair off the band.  The solve of
// the band is the kernel that matters: ONE workgroup of 256 threads factors it by block Cholesky and sweeps it forward and back (a block Thomas recurrence,
// sequential in the node index: one thread walks it, out of chunks of 32 nodes that all threads stage through LDS).  The optimiser around it is not built.
#include "icet_ctx.h"
#include "icet_posegraph_body.h"

#include <cstring>
#include <vector>

namespace icet {

__global__ __launch_bounds__(kPgThreads) void k_pg_block_tridiag(int N, const double* Dm, const double* Bm, const double* rhs, double* x, double* G, double* W, double* u, int32_t* status) {
    __shared__ PgShared sh;
    pg_block_tridiag(N, Dm, Bm, rhs, x, G, W, u, status, sh);
}

}  // namespace icet

using namespace icet;

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
