// icet_amd/csrc/icet_kfstore.hip -- the keyframe store (include/icet_hip.h icet_keyframe_store_*): after a put's keyframe build
// (the unchanged icet_keyframe_device_n path) k_keyframe_store_park copies workspace row b of the four keyframe tables into store row slots[b].
// The store's rows have the layout of the workspace's keyframe side (row stride V, (V + 1) & ~1 for slot_of_voxel), so the indexed loop kernels
// read a slot exactly as they read a parked keyframe.
#include <hip/hip_runtime.h>
#include "icet_internal.h"

namespace icet {
namespace {

constexpr int kParkBlock = 256;
static_assert(sizeof(SlotHot) == 3 * 16 && sizeof(SlotFit) == 5 * 16, "the park kernel copies these records as 3 + 5 16-byte vectors");

// One block per keyframe: block k copies workspace row first + k into store row dst.slot[k] -- n_slots, the first n_slots SlotHot / SlotFit records and the
// whole padded slot_of_voxel row.  The destination rows travel in the argument, so a launch never depends on host memory that a later call rewrites.
__global__ __launch_bounds__(kParkBlock) void k_keyframe_store_park(const SlotHot* __restrict__ hotS, const SlotFit* __restrict__ fitS,
                                                                    const int16_t* __restrict__ slot_of_voxel, const int32_t* __restrict__ n_slots,
                                                                    SlotHot* __restrict__ hot_dst, SlotFit* __restrict__ fit_dst,
                                                                    int16_t* __restrict__ sov_dst, int32_t* __restrict__ n_slots_dst,
                                                                    int V, int first, StoreParkSlots dst) {
    const int b = first + (int)blockIdx.x;
    const size_t d = (size_t)dst.slot[blockIdx.x];
    const int ns = n_slots[b];
    const uint4* hs = reinterpret_cast<const uint4*>(hotS + (size_t)b * V);
    uint4* hd = reinterpret_cast<uint4*>(hot_dst + d * V);
    for (int i = threadIdx.x; i < 3 * ns; i += kParkBlock) hd[i] = hs[i];
    const uint4* fs = reinterpret_cast<const uint4*>(fitS + (size_t)b * V);
    uint4* fd = reinterpret_cast<uint4*>(fit_dst + d * V);
    for (int i = threadIdx.x; i < 5 * ns; i += kParkBlock) fd[i] = fs[i];
    const int row = (V + 1) & ~1;                                  // int16 entries per row: an even count, copied as 32-bit words
    const uint32_t* ms = reinterpret_cast<const uint32_t*>(slot_of_voxel + (size_t)b * row);
    uint32_t* md = reinterpret_cast<uint32_t*>(sov_dst + d * row);
    for (int i = threadIdx.x; i < row / 2; i += kParkBlock) md[i] = ms[i];
    if (threadIdx.x == 0) n_slots_dst[d] = ns;
}

}  // namespace

hipError_t launch_keyframe_store_park(const Workspace& w, int V, int first, int count, const StoreParkSlots& dst,
                                      SlotHot* hot_dst, SlotFit* fit_dst, int16_t* sov_dst, int32_t* n_slots_dst, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    if (count > kStoreParkMax) return hipErrorInvalidValue;
    k_keyframe_store_park<<<count, kParkBlock, 0, st>>>(w.hotS, w.fitS, w.slot_of_voxel, w.n_slots, hot_dst, fit_dst, sov_dst, n_slots_dst, V, first, dst);
    return hipGetLastError();
}

}  // namespace icet
