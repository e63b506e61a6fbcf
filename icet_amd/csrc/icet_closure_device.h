// icet_amd/csrc/icet_closure_device.h -- the device code the closure kernels share (icet_closure.hip, icet_appearance.hip, icet_coarse.hip): the selection of
// the K smallest u64 keys -- minima over a wave and a block, and the K rounds in which a wave takes them out of the keys its lanes hold in registers -- and the
// registrations a (query, candidate) resolves into.
#pragma once
#include <hip/hip_runtime.h>
#include "icet_internal.h"
#include "icet_closure.h"

namespace icet {

constexpr int kSelectBlock = 256;
static_assert(kClosureTile % kSelectBlock == 0 && kSelectBlock == 256, "four waves per block, whole keys per lane");
constexpr int kMergeRegs = 16;                      // keys per thread the merge keeps in registers (4096 per query: 256 tiles x K = 16)
constexpr int kKeysPerLane = kClosureTile / 64;     // keys per lane of a wave that holds a tile

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint64_t u = __shfl_xor((unsigned long long)v, o, 64); v = u < v ? u : v; }
    return v;
}
// The block's minimum of v, known to every thread; wmin: 2 x 4 words, `round` alternates the half in use (one barrier per round).
__device__ __forceinline__ uint64_t block_min_u64(uint64_t v, uint64_t (*wmin)[4], int round) {
    v = wave_min_u64(v);
    if ((threadIdx.x & 63) == 0) wmin[round & 1][threadIdx.x >> 6] = v;
    __syncthreads();
    const uint64_t a = wmin[round & 1][0], b = wmin[round & 1][1], c = wmin[round & 1][2], d = wmin[round & 1][3];
    const uint64_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// Pass 1 of a search, the whole body of its kernel behind whatever the block stages for key_of: wave w takes the queries w, w + 4, ...; a lane holds the keys
// of kKeysPerLane slots of the block's tile in registers -- key_of(q, s): the key of slot s of the tile for query q (distinct keys, or kNoKey) -- and the wave
// selects its K smallest by K rounds of a wave-wide minimum: shuffles only, no barrier inside a query (a block-wide round with its barrier cost 0.5 us, and a
// tile near the queries ran Q x K of them in series).  part[(q * gridDim.x + block) * K + k]: the block's k-th smallest key of query q, kNoKey behind the last.
template <typename KeyOf>
__device__ __forceinline__ void select_tile_smallest(int n_queries, int K, unsigned long long* __restrict__ part, KeyOf key_of) {
    using icet_closure_rule::kNoKey;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = wave; q < n_queries; q += kSelectBlock / 64) {
        uint64_t key[kKeysPerLane];
#pragma unroll
        for (int i = 0; i < kKeysPerLane; i++) key[i] = key_of(q, lane + 64 * i);
        unsigned long long* out = part + ((size_t)q * gridDim.x + blockIdx.x) * K;
        int k = 0;
        for (; k < K; k++) {
            uint64_t m = key[0];
#pragma unroll
            for (int i = 1; i < kKeysPerLane; i++) m = key[i] < m ? key[i] : m;
            const uint64_t b = wave_min_u64(m);
            if (b == kNoKey) break;                                   // (the same for every lane)
            if (lane == 0) out[k] = b;
#pragma unroll
            for (int i = 0; i < kKeysPerLane; i++) key[i] = key[i] == b ? kNoKey : key[i];
        }
        for (int j = k + lane; j < K; j += 64) out[j] = kNoKey;
    }
}

// The tail of a resolve kernel, thread i = q K + k.  offs (may be null): the groups of k_select_best (group = query), written by the first n_queries + 1 threads.
__device__ __forceinline__ void write_group_offset(int i, int n_queries, int K, int n_starts, int32_t* __restrict__ offs) {
    if (offs && i <= n_queries) offs[i] = i * K * n_starts;
}
// The registrations r = i S + s of the indexed call behind it: x0[r] = fl(base + off[s]), kf_of[r] = the slot -- `any_slot`, an occupied one, for a missing
// candidate --, rows[r] = "all of the scan" or 0 (a missing candidate registers a scan of no rows: no point pass, a score without voxels), members[r] = r.
__device__ __forceinline__ void write_registrations(int i, int slot, int any_slot, const float (&base)[6], const float (*off)[6], int n_starts, float* __restrict__ x0,
                                                    int32_t* __restrict__ kf_of, int32_t* __restrict__ rows, int32_t* __restrict__ members) {
    for (int s = 0; s < n_starts; s++) {
        const int r = i * n_starts + s;
        for (int c = 0; c < 6; c++) x0[(size_t)r * 6 + c] = slot >= 0 ? base[c] + off[s][c] : 0.f;
        kf_of[r] = slot >= 0 ? slot : any_slot;
        rows[r] = slot >= 0 ? INT32_MAX : 0;
        members[r] = r;
    }
}

}  // namespace icet
