// icet_amd/csrc/icet_map_snapshot.hip -- a voxel map saved to a file, loaded from one and merged with another (include/icet_hip.h icet_voxel_map_save / _load /
// _snapshot_info / _merge_device; the format and its validation: icet_map_snapshot.h).  Every per-cell word of a map is a 64-bit integer
// sum, so all four are ONE operation -- the words of a set of cells added into a table with sign +1 or -1 -- with the source in a file or in another table:
//     k_map_snap_cells  a pass over the table, 16 entries per thread: <false> counts the claimed entries and those with a non-zero value word (tallied in LDS, one
//                       atomic per block and counter); <true> compacts (key, entry) of the latter (a block claims its places with one atomic), for the sort by key
//                       that the extract and the index use (map_sort_cells, icet_map.hip)
//     k_map_pack        one thread per sorted entry of a chunk: W scattered 8-byte reads through the entry index, coalesced 8-byte stores into the W column pieces
//                       of the staging, and the words' checksum terms by their place in the whole payload: wave64 shuffle, four partials in LDS, ONE atomic per block
//     k_map_merge       one thread per source entry -- of a staged chunk's column pieces, or of another map's table (free keys and all-zero entries skipped) --:
//                       <., ., true> probes the destination read-only and counts the keys it does not hold yet; <., ., false> adds the words times sign through
//                       table_update / table_update_shape (icet_map_table.h), the add's own step
//     k_map_totals      the source's five running totals into the destination's device record, in stream order
// Integers only: no floating point, no scratch, no block waits for another, no fence, nothing captured into a graph.  The map itself is icet_map.hip's; this file
// sees it through map_snapshot_view (icet_internal.h) and keeps its own state in the slot the map frees.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include "../../include/icet_hip.h"
#include "icet_ctx.h"
#include "icet_map_table.h"
#include "icet_map_snapshot.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace icet {
namespace {

namespace rule = icet_map_rule;
namespace srule = icet_map_shape_rule;
namespace msnap = icet_map_snapshot;

constexpr int kSnapBlock = 256;
constexpr int kSnapWaves = kSnapBlock / 64;
constexpr int kSnapPer = 16;             // entries per thread of a pass over the table (k_map_cells' shape)
constexpr int kSnapSpan = kSnapBlock * kSnapPer;
constexpr int kValueWords = 4 + srule::kWords;      // count, three sums, nine moment words
static_assert(msnap::kWordsPlain == 5 && msnap::kWordsShaped == 1 + kValueWords, "key, then the value words");
// this file's own device record
enum { kSnClaimed = 0, kSnNonzero, kSnCursor, kSnNew, kSnSum, kSnWords = 8 };

// A table that is only read: the source of a save or a merge.
struct SnapTable { const u64* key; const u64* count; const u64* sum; const u64* mom; uint32_t log2; };

// The value words of entry i: w[0] count, w[1 .. 3] the sums, and with kShape w[4 .. 12] the moment words.  Returns their OR.
template <bool kShape> __device__ __forceinline__ u64 load_values(const SnapTable& t, u64 i, u64 w[kValueWords]) {
    const u64 size = (u64)1 << t.log2;
    w[0] = t.count[i];
    u64 any = w[0];
#pragma unroll
    for (int a = 0; a < 3; a++) { w[1 + a] = t.sum[a * size + i]; any |= w[1 + a]; }
    if constexpr (kShape) {
#pragma unroll
        for (int j = 0; j < srule::kWords; j++) { w[4 + j] = t.mom[j * size + i]; any |= w[4 + j]; }
    }
    return any;
}

// A block walks kSnapSpan entries, kSnapPer per thread, and touches the device record once per counter (DESIGN.md section 21 on what many adders on one address
// cost).  kSelect: the claimed entries with a non-zero value word are written as (key, entry) at places the block claims with one atomic (their order is free:
// the pairs are sorted next); else they and the claimed entries are only counted.
template <bool kSelect, bool kShape>
__global__ __launch_bounds__(kSnapBlock) void k_map_snap_cells(SnapTable t, u64* __restrict__ ctr, u64* __restrict__ sel_key, uint32_t* __restrict__ sel_idx, u64 cap) {
    __shared__ uint32_t tally[2];
    __shared__ u64 base;
    const u64 size = (u64)1 << t.log2, first = (u64)blockIdx.x * kSnapSpan + threadIdx.x;      // the grid covers the entries; a table below kSnapSpan is one block
    if (threadIdx.x < 2) tally[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t n_claimed = 0, n_out = 0, mask = 0;
#pragma unroll
    for (int j = 0; j < kSnapPer; j++) {
        const u64 i = first + (u64)j * kSnapBlock;
        if (i >= size) break;
        if (t.key[i] == rule::kEmpty) continue;
        n_claimed++;
        u64 w[kValueWords];
        if (load_values<kShape>(t, i, w)) { n_out++; mask |= 1u << j; }
    }
    if (kSelect) {
        uint32_t at = 0;
        if (n_out) at = atomicAdd(&tally[0], n_out);
        __syncthreads();
        if (threadIdx.x == 0 && tally[0]) base = __hip_atomic_fetch_add(&ctr[kSnCursor], (u64)tally[0], MAP_RLX_AGENT);
        __syncthreads();
        if (!n_out) return;
        u64 pos = base + at;
        for (int j = 0; j < kSnapPer; j++) {
            if (!((mask >> j) & 1u)) continue;
            const u64 i = first + (u64)j * kSnapBlock;
            if (pos < cap) { sel_key[pos] = t.key[i]; sel_idx[pos] = (uint32_t)i; }      // (cap: the count pass's figure, on the same stream)
            pos++;
        }
    } else {
        if (n_claimed) atomicAdd(&tally[0], n_claimed);
        if (n_out) atomicAdd(&tally[1], n_out);
        __syncthreads();
        if (threadIdx.x < 2 && tally[threadIdx.x]) __hip_atomic_fetch_add(&ctr[kSnClaimed + threadIdx.x], (u64)tally[threadIdx.x], MAP_RLX_AGENT);
    }
}

// The sum of v over the block into *out: a wave64 shuffle, the waves' partials through LDS, one atomic per block.  An integer sum is exact in any order.
__device__ __forceinline__ void block_add(u64 v, u64* out) {
    __shared__ u64 part[kSnapWaves];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int k = 0; k < kSnapWaves; k++) s += part[k];
        if (s) __hip_atomic_fetch_add(out, s, MAP_RLX_AGENT);
    }
}

// Sorted entries first .. first + len - 1 of the n into the staging: column c of the chunk is stage[c len .. c len + len).  A word's checksum term uses its place
// in the whole payload, so the chunking cannot change the sum.
template <bool kShape>
__global__ __launch_bounds__(kSnapBlock) void k_map_pack(SnapTable t, const u64* __restrict__ skey, const uint32_t* __restrict__ sidx, u64 first, uint32_t len, u64 n,
                                                        u64* __restrict__ stage, u64* __restrict__ ctr) {
    constexpr int kVals = kShape ? kValueWords : 4;
    const uint32_t j = blockIdx.x * kSnapBlock + threadIdx.x;
    u64 sum = 0;
    if (j < len) {
        const u64 at = first + j, key = skey[at], e = sidx[at];      // e < size: the select pass wrote an entry's index
        u64 w[kValueWords];
        load_values<kShape>(t, e, w);
        stage[j] = key;
        sum = msnap::term(key, msnap::word_index(n, 0, at));
#pragma unroll
        for (int c = 0; c < kVals; c++) {
            stage[(size_t)(1 + c) * len + j] = w[c];
            sum += msnap::term(w[c], msnap::word_index(n, 1 + c, at));
        }
    }
    block_add(sum, &ctr[kSnSum]);
}

// The entry of `key`, or -1: read-only, at most `size` probes (nothing writes the table while a dry run reads it).
__device__ __forceinline__ long long probe(const MapTable& t, u64 key) {
    const u64 mask = ((u64)1 << t.log2) - 1;
    u64 h = rule::mix(key) & mask;                                    // h <= mask: inside every array
    for (u64 p = 0; p <= mask; p++) {
        const u64 k = t.key[h];
        if (k == key) return (long long)h;
        if (k == rule::kEmpty) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// The source of a merge: the column pieces of a staged chunk (column c: stage[c len .. c len + len)), or another map's table.
struct MergeSource { const u64* stage; uint32_t len; SnapTable t; };

// kShape: the destination is shaped and the source carries moments, which are merged; else the five plain words are (a shaped source's moments are left out).
// An entry whose merged words are all zero is skipped, by the dry run and the apply alike: it would claim an entry and change nothing.  The source's keys are
// distinct; the claim's compare-and-swap is still needed, because different keys compete for free entries.
template <bool kFromTable, bool kShape, bool kDryRun>
__global__ __launch_bounds__(kSnapBlock) void k_map_merge(TableOf<kShape> dst, MergeSource src, u64 sign, u64* __restrict__ ctr) {
    const u64 i = (u64)blockIdx.x * kSnapBlock + threadIdx.x;
    const u64 total = kFromTable ? (u64)1 << src.t.log2 : (u64)src.len;
    u64 key = rule::kEmpty, w[kValueWords], any = 0;
    if (i < total) {
        if (kFromTable) {
            key = src.t.key[i];
            if (key != rule::kEmpty) any = load_values<kShape>(src.t, i, w);
        } else {
            constexpr int kVals = kShape ? kValueWords : 4;
            key = src.stage[i];
#pragma unroll
            for (int c = 0; c < kVals; c++) { w[c] = src.stage[(size_t)(1 + c) * src.len + i]; any |= w[c]; }
        }
    }
    const bool have = key != rule::kEmpty && any != 0;
    if (kDryRun) {
        const u64 is_new = have && probe(dst, key) < 0 ? 1 : 0;
        block_add(is_new, &ctr[kSnNew]);
    } else if (have) {
        // (below the capacity bound the host checked, a probe run always meets the key or a free entry: nothing is dropped)
        if constexpr (kShape) {
            u64 dm[srule::kWords];
#pragma unroll
            for (int j = 0; j < srule::kWords; j++) dm[j] = sign * w[4 + j];
            (void)table_update_shape(dst, key, sign * w[0], sign * w[1], sign * w[2], sign * w[3], dm);
        } else {
            (void)table_update(dst, key, sign * w[0], sign * w[1], sign * w[2], sign * w[3]);
        }
    }
}

// dst's totals += sign x the source's: a file's five words, or (src_ctr) the sum of another map's kTotCopies copies.  Copy 0 of the destination takes them.
struct SnapTotals { u64 v[5]; };
__global__ __launch_bounds__(64) void k_map_totals(const u64* __restrict__ src_ctr, SnapTotals file, u64 sign, u64* __restrict__ dst_ctr) {
    const int w = threadIdx.x;
    if (w >= 5) return;
    u64 s = file.v[w];
    if (src_ctr) { s = 0; for (int k = 0; k < kTotCopies; k++) s += src_ctr[k * kTotWords + w]; }
    dst_ctr[w] += sign * s;
}

// The staging of a save or a load: `cap` u64 words on the device, two pinned buffers of as many that a chunk's copy and the file I/O of its neighbour alternate
// between, and the events that guard them.  It stays with the map and grows on demand, behind a drained stream: a save does not pay a
// pinned allocation per call.
struct SnapStage {
    u64* d_stage = nullptr; u64* h_buf[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; size_t cap = 0;
    BufferGroup mem;
    hipError_t ensure(size_t words, hipStream_t st) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < 2; k++) if (e == hipSuccess && !ev[k]) e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
        if (e != hipSuccess || words <= cap) return e;
        e = hipStreamSynchronize(st);                                 // (an earlier call's kernels may still read the old buffers)
        if (e != hipSuccess) return e;
        return static_cast<hipError_t>(grow(mem, cap, words, [&] {
            int a = mem.device(d_stage, words);
            for (int k = 0; k < 2; k++) if (!a) a = mem.pinned(h_buf[k], words);
            return a;
        }));
    }
    ~SnapStage() { for (hipEvent_t& e : ev) if (e) (void)hipEventDestroy(e); }
};

// What a map's snapshot calls keep: this file's device record and its pinned twin, the pinned copy of the map's totals a save reads, the sorted cells of a
// save and the staging of a save or a load.  The map drains its stream before it frees this.
struct SnapState {
    u64* d_ctr = nullptr; u64* h_ctr = nullptr; u64* h_tot = nullptr;
    SortedCells cells; SnapStage stage;
    BufferGroup mem;
};
void snap_state_free(void* p) { delete static_cast<SnapState*>(p); }

icet_status snap_refuse(icet_voxel_map* m, const std::string& why) { map_set_error(m, why.c_str()); return ICET_ERR_BAD_ARG; }
icet_status snap_hip_error(icet_voxel_map* m, const char* what, hipError_t e) {
    (void)hipGetLastError();
    map_set_error(m, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
    return e == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP;
}
#define SNAPCHK(m, call) do { const hipError_t e_ = static_cast<hipError_t>(call); if (e_ != hipSuccess) return snap_hip_error(m, #call, e_); } while (0)

icet_status snap_enter(icet_voxel_map* m, const MapSnapshotView& v, SnapState** out) {
    const icet_status st = enter(v.ctx);
    if (st != ICET_OK) { map_set_error(m, v.ctx->err.c_str()); return st; }
    if (!*v.snap) {
        SnapState* s = new (std::nothrow) SnapState();
        if (!s) { map_set_error(m, "host allocation failed"); return ICET_ERR_NOMEM; }
        int e = s->mem.device(s->d_ctr, (size_t)kSnWords);
        if (!e) e = s->mem.pinned(s->h_ctr, (size_t)kSnWords);
        if (!e) e = s->mem.pinned(s->h_tot, (size_t)kTotCopies * kTotWords);
        if (e) { delete s; return snap_hip_error(m, "the snapshot record", static_cast<hipError_t>(e)); }
        *v.snap = s; *v.snap_free = snap_state_free;
    }
    *out = static_cast<SnapState*>(*v.snap);
    return ICET_OK;
}

SnapTable read_table(const MapSnapshotView& v) { return SnapTable{v.key, v.count, v.sum, v.mom, v.log2}; }
unsigned table_grid(uint32_t log2) { return (unsigned)((((size_t)1 << log2) + kSnapSpan - 1) / kSnapSpan); }
unsigned row_grid(uint64_t rows) { return (unsigned)((rows + kSnapBlock - 1) / kSnapBlock); }
int64_t chunk_entries(const icet_ctx* c, uint64_t n) {
    const uint64_t opt = c->map_snapshot_chunk_entries > 0 ? (uint64_t)c->map_snapshot_chunk_entries : (uint64_t)1 << 20;
    return (int64_t)std::max<uint64_t>(1, std::min(opt, n));
}

// The record zeroed and the count pass over `t` enqueued (shaped: a non-zero moment word counts too).
icet_status enqueue_count(icet_voxel_map* m, SnapState* s, const SnapTable& t, bool shaped, hipStream_t st) {
    SNAPCHK(m, hipMemsetAsync(s->d_ctr, 0, sizeof(u64) * kSnWords, st));
    if (shaped) k_map_snap_cells<false, true><<<table_grid(t.log2), kSnapBlock, 0, st>>>(t, s->d_ctr, nullptr, nullptr, 0);
    else k_map_snap_cells<false, false><<<table_grid(t.log2), kSnapBlock, 0, st>>>(t, s->d_ctr, nullptr, nullptr, 0);
    SNAPCHK(m, hipGetLastError());
    return ICET_OK;
}
icet_status fetch_record(icet_voxel_map* m, SnapState* s, hipStream_t st) {
    SNAPCHK(m, hipMemcpyAsync(s->h_ctr, s->d_ctr, sizeof(u64) * kSnWords, hipMemcpyDeviceToHost, st));
    SNAPCHK(m, hipStreamSynchronize(st));
    return ICET_OK;
}

struct SelectArg { SnapTable t; u64* ctr; bool shaped; };
hipError_t select_nonzero(void* arg, SortedCells& sc, int64_t n, hipStream_t st) {
    const SelectArg& a = *static_cast<const SelectArg*>(arg);
    if (a.shaped) k_map_snap_cells<true, true><<<table_grid(a.t.log2), kSnapBlock, 0, st>>>(a.t, a.ctr, sc.sel_key, sc.sel_idx, (u64)n);
    else k_map_snap_cells<true, false><<<table_grid(a.t.log2), kSnapBlock, 0, st>>>(a.t, a.ctr, sc.sel_key, sc.sel_idx, (u64)n);
    return hipGetLastError();
}

// Chunk (first, len) of the n entries from a pinned buffer (W pieces of len words) to its W places in the file.
bool write_chunk(icet_snapshot::Writer& w, const u64* buf, uint64_t n, uint32_t words, uint64_t first, uint64_t len, std::string& err) {
    for (uint32_t c = 0; c < words; c++) {
        if (!icet_snapshot::writer_seek(w, msnap::column_offset(n, c) + 8 * first, err)) return false;
        if (!icet_snapshot::writer_write(w, buf + (size_t)c * len, 8 * len, err)) return false;
    }
    return true;
}

icet_status map_save(icet_voxel_map* m, const MapSnapshotView& v, const char* path) {
    SnapState* s = nullptr;
    ICET_TRY(snap_enter(m, v, &s));
    hipStream_t st = v.ctx->stream;
    const bool shaped = v.mom != nullptr;
    const uint32_t W = msnap::words_of(shaped);
    const SnapTable t = read_table(v);
    // behind whatever was enqueued: the entries to write, and the totals
    ICET_TRY(enqueue_count(m, s, t, shaped, st));
    SNAPCHK(m, hipMemcpyAsync(s->h_tot, v.ctr, sizeof(u64) * kTotCopies * kTotWords, hipMemcpyDeviceToHost, st));
    ICET_TRY(fetch_record(m, s, st));
    const uint64_t n = s->h_ctr[kSnNonzero];
    msnap::Header h{};
    std::memcpy(&h.cell_bits, &v.cell, 4); std::memcpy(&h.min_range_bits, &v.min_range, 4); std::memcpy(&h.max_range_bits, &v.max_range, 4);
    h.flags = shaped ? msnap::kFlagShaped : 0u; h.words = W; h.n = n; h.file_bytes = msnap::file_bytes(n, W);
    for (int w = 0; w < 5; w++) { u64 sum = 0; for (int k = 0; k < kTotCopies; k++) sum += s->h_tot[k * kTotWords + w]; h.totals[w] = (int64_t)sum; }
    std::string err;
    icet_snapshot::Writer wr;
    uint8_t front[msnap::kHeaderBytes] = {0};
    if (!icet_snapshot::writer_open(wr, path, err)) return snap_refuse(m, "icet_voxel_map_save: " + err);
    // from here on every return goes through `fail`: the stream drained, the temporary file removed
    SortedCells& cells = s->cells; SnapStage& stage = s->stage;
    auto fail = [&](icet_status r) { (void)hipStreamSynchronize(st); icet_snapshot::writer_abort(wr); return r; };
    bool io_ok = icet_snapshot::writer_write(wr, front, sizeof(front), err);      // (the header's place; written again when the checksum is known)
    if (io_ok && n > 0) {
        SelectArg sa{t, s->d_ctr, shaped};
        const icet_status sorted = static_cast<icet_status>(map_sort_cells(m, cells, (int64_t)n, select_nonzero, &sa));
        if (sorted != ICET_OK) return fail(sorted);
        const uint64_t chunk = (uint64_t)chunk_entries(v.ctx, n), n_chunks = (n + chunk - 1) / chunk;
        hipError_t he = stage.ensure((size_t)W * chunk, st);
        auto len_of = [&](uint64_t k) { return std::min(chunk, n - k * chunk); };
        // chunk k: pack -> copy into pinned buffer k & 1; chunk k - 1 goes to the file meanwhile
        for (uint64_t k = 0; k < n_chunks && he == hipSuccess && io_ok; k++) {
            const uint64_t first = k * chunk, len = len_of(k);
            if (shaped) k_map_pack<true><<<row_grid(len), kSnapBlock, 0, st>>>(t, cells.key, cells.idx, first, (uint32_t)len, n, stage.d_stage, s->d_ctr);
            else k_map_pack<false><<<row_grid(len), kSnapBlock, 0, st>>>(t, cells.key, cells.idx, first, (uint32_t)len, n, stage.d_stage, s->d_ctr);
            he = hipGetLastError();
            if (he == hipSuccess) he = hipMemcpyAsync(stage.h_buf[k & 1], stage.d_stage, sizeof(u64) * W * len, hipMemcpyDeviceToHost, st);
            if (he == hipSuccess) he = hipEventRecord(stage.ev[k & 1], st);
            if (he == hipSuccess && k > 0) {
                he = hipEventSynchronize(stage.ev[(k - 1) & 1]);
                if (he == hipSuccess) io_ok = write_chunk(wr, stage.h_buf[(k - 1) & 1], n, W, first - chunk, chunk, err);
            }
        }
        if (he == hipSuccess && io_ok) {
            he = hipMemcpyAsync(s->h_ctr, s->d_ctr, sizeof(u64) * kSnWords, hipMemcpyDeviceToHost, st);
            if (he == hipSuccess) he = hipStreamSynchronize(st);
            if (he == hipSuccess) io_ok = write_chunk(wr, stage.h_buf[(n_chunks - 1) & 1], n, W, (n_chunks - 1) * chunk, len_of(n_chunks - 1), err);
        }
        if (he != hipSuccess) return fail(snap_hip_error(m, "icet_voxel_map_save", he));
        if (io_ok && (n & 1)) {                                       // the zero word behind every column of odd length
            const u64 zero = 0;
            for (uint32_t c = 0; c < W && io_ok; c++) io_ok = icet_snapshot::writer_seek(wr, msnap::column_offset(n, c) + 8 * n, err) && icet_snapshot::writer_write(wr, &zero, 8, err);
        }
        h.payload_sum = s->h_ctr[kSnSum] + msnap::padding_sum(n, W);
    }
    if (io_ok) {
        msnap::put_header(front, h);
        msnap::seal(front);
        io_ok = icet_snapshot::writer_rewind(wr, err) && icet_snapshot::writer_write(wr, front, sizeof(front), err) && icet_snapshot::writer_commit(wr, err);
    }
    if (!io_ok) return fail(snap_refuse(m, "icet_voxel_map_save: " + err));
    (void)hipStreamSynchronize(st);
    return ICET_OK;
}

// The source of map_merge: a validated image, or another map.
struct MergeFrom { const uint8_t* img; const msnap::Header* h; const MapSnapshotView* src; };

template <bool kFromTable, bool kDryRun>
hipError_t launch_merge(const MapSnapshotView& v, bool shaped, const MergeSource& src, u64 sign, u64* ctr, hipStream_t st) {
    const uint64_t total = kFromTable ? (uint64_t)1 << src.t.log2 : (uint64_t)src.len;
    MapShapeTable ts; ts.key = v.key; ts.count = v.count; ts.sum = v.sum; ts.log2 = v.log2; ts.mom = v.mom;
    if (shaped) k_map_merge<kFromTable, true, kDryRun><<<row_grid(total), kSnapBlock, 0, st>>>(ts, src, sign, ctr);
    else k_map_merge<kFromTable, false, kDryRun><<<row_grid(total), kSnapBlock, 0, st>>>(static_cast<const MapTable&>(ts), src, sign, ctr);
    return hipGetLastError();
}

// The words of the source's cells into the map's table with `sign`: everything is checked -- the dry run included -- before anything is touched.
icet_status map_merge(icet_voxel_map* m, const MapSnapshotView& v, const MergeFrom& from, int32_t sign, const std::string& who) {
    const bool dst_shaped = v.mom != nullptr, src_shaped = from.src ? from.src->mom != nullptr : from.h->shaped();
    float src_cell;
    if (from.src) src_cell = from.src->cell; else std::memcpy(&src_cell, &from.h->cell_bits, 4);
    if (!rule::sign_ok(sign)) return snap_refuse(m, who + ": sign must be +1 or -1");
    if (std::memcmp(&src_cell, &v.cell, 4) != 0) return snap_refuse(m, who + ": the source's cell differs from the map's (its keys name other cells)");
    if (dst_shaped && !src_shaped) return snap_refuse(m, who + ": a plain source into a shaped map (the moments would no longer belong to the counts)");
    SnapState* s = nullptr;
    ICET_TRY(snap_enter(m, v, &s));
    hipStream_t st = v.ctx->stream;
    const u64 sg = sign > 0 ? (u64)1 : ~(u64)0;                       // -1 in two's complement
    const bool shaped = dst_shaped;                                   // moments are merged iff the destination carries them (the source then does)
    const uint32_t Wd = msnap::words_of(shaped);
    const uint64_t n = from.src ? 0 : from.h->n, size = (uint64_t)1 << v.log2;
    const uint64_t chunk = (uint64_t)chunk_entries(v.ctx, n), n_chunks = n ? (n + chunk - 1) / chunk : 0;
    SnapStage& stage = s->stage;
    auto fail = [&](icet_status r) { (void)hipStreamSynchronize(st); return r; };
    if (n > 0) {
        const hipError_t he = stage.ensure((size_t)Wd * chunk, st);
        if (he != hipSuccess) return snap_hip_error(m, who.c_str(), he);
    }
    // one pass of the source through k_map_merge: a table in one launch, a file chunk by chunk -- the file's columns into pinned buffer k & 1 (once the copy of
    // chunk k - 2 has left it) -> copy -> kernel
    auto pass = [&](auto kDry) -> hipError_t {
        constexpr bool dry = decltype(kDry)::value;
        if (from.src) {
            const MergeSource src{nullptr, 0u, read_table(*from.src)};
            return launch_merge<true, dry>(v, shaped, src, sg, s->d_ctr, st);
        }
        hipError_t he = hipSuccess;
        for (uint64_t k = 0; k < n_chunks && he == hipSuccess; k++) {
            const uint64_t first = k * chunk, len = std::min(chunk, n - first);
            if (k >= 2) he = hipEventSynchronize(stage.ev[k & 1]);
            if (he != hipSuccess) break;
            for (uint32_t c = 0; c < Wd; c++) std::memcpy(stage.h_buf[k & 1] + (size_t)c * len, from.img + msnap::column_offset(n, c) + 8 * first, 8 * len);
            he = hipMemcpyAsync(stage.d_stage, stage.h_buf[k & 1], sizeof(u64) * Wd * len, hipMemcpyHostToDevice, st);
            if (he == hipSuccess) he = hipEventRecord(stage.ev[k & 1], st);
            const MergeSource src{stage.d_stage, (uint32_t)len, SnapTable{}};
            if (he == hipSuccess) he = launch_merge<false, dry>(v, shaped, src, sg, s->d_ctr, st);
        }
        if (he == hipSuccess && n_chunks > 0) he = hipStreamSynchronize(st);      // (the pinned buffers are free for the next pass)
        return he;
    };
    // the claimed entries of the destination, and the source's keys it does not hold yet
    icet_status r = enqueue_count(m, s, read_table(v), false, st);
    if (r != ICET_OK) return fail(r);
    hipError_t he = pass(std::true_type{});
    if (he != hipSuccess) return fail(snap_hip_error(m, who.c_str(), he));
    r = fetch_record(m, s, st);
    if (r != ICET_OK) return fail(r);
    const uint64_t claimed = s->h_ctr[kSnClaimed], fresh = s->h_ctr[kSnNew];
    if (claimed + fresh > size)
        return fail(snap_refuse(m, who + ": the table is too small (" + std::to_string(claimed) + " claimed entries + " + std::to_string(fresh) + " new keys > " + std::to_string(size) +
                                   " entries): merge into a larger map"));
    // from here on the table changes, as in an add
    *v.ix_stale = true; *v.dirty = true; (*v.generation)++;
    he = pass(std::false_type{});
    if (he != hipSuccess) return fail(snap_hip_error(m, who.c_str(), he));
    SnapTotals tot{};
    if (!from.src) for (int w = 0; w < 5; w++) tot.v[w] = (u64)from.h->totals[w];
    k_map_totals<<<1, 64, 0, st>>>(from.src ? from.src->ctr : nullptr, tot, sg, v.ctr);
    he = hipGetLastError();
    if (he == hipSuccess && !from.src) he = hipStreamSynchronize(st);      // a load returns behind its last kernel; a merge is asynchronous from here
    if (he != hipSuccess) return fail(snap_hip_error(m, who.c_str(), he));
    return ICET_OK;
}

}  // namespace
}  // namespace icet

using namespace icet;

extern "C" {

icet_status icet_voxel_map_save(icet_voxel_map* map, const char* path) {
    MapSnapshotView v;
    if (!map_snapshot_view(map, &v)) return ICET_ERR_BAD_ARG;
    if (!path) return snap_refuse(map, "icet_voxel_map_save: bad argument (a NULL path)");
    return map_save(map, v, path);
}

icet_status icet_voxel_map_load(icet_voxel_map* map, const char* path, int32_t sign) {
    MapSnapshotView v;
    if (!map_snapshot_view(map, &v)) return ICET_ERR_BAD_ARG;
    const std::string who("icet_voxel_map_load");
    if (!path) return snap_refuse(map, who + ": bad argument (a NULL path)");
    // the file, read and validated on the host, then held against the map
    std::vector<uint8_t> img; msnap::Header h; std::string err;
    if (!msnap::read_file(path, img, h, err)) return snap_refuse(map, who + ": " + err);
    const MergeFrom from{img.data(), &h, nullptr};
    return map_merge(map, v, from, sign, who);
}

icet_status icet_voxel_map_snapshot_info(const char* path, struct icet_voxel_map_snapshot_info* out) {
    static_assert(sizeof(struct icet_voxel_map_snapshot_info) == 96, "the record of include/icet_hip.h (the ctypes mirror of icet_amd/api.py)");
    if (!path || !out) return ICET_ERR_BAD_ARG;
    std::vector<uint8_t> img; msnap::Header h; std::string err;
    if (!msnap::read_file(path, img, h, err)) return ICET_ERR_BAD_ARG;
    std::memset(out, 0, sizeof(*out));
    std::memcpy(&out->cell, &h.cell_bits, 4); std::memcpy(&out->min_range, &h.min_range_bits, 4); std::memcpy(&out->max_range, &h.max_range_bits, 4);
    out->shaped = h.shaped() ? 1 : 0; out->words_per_entry = (int32_t)h.words; out->entries = (int64_t)h.n;
    out->points_in = h.totals[0]; out->points_kept = h.totals[1]; out->points_nonfinite = h.totals[2]; out->points_outside = h.totals[3]; out->points_dropped = h.totals[4];
    out->file_bytes = (int64_t)h.file_bytes; out->payload_checksum = h.payload_sum;
    return ICET_OK;
}

icet_status icet_voxel_map_merge_device(icet_voxel_map* dst, icet_voxel_map* src, int32_t sign) {
    MapSnapshotView v, sv;
    if (!map_snapshot_view(dst, &v)) return ICET_ERR_BAD_ARG;
    const std::string who("icet_voxel_map_merge_device");
    if (!map_snapshot_view(src, &sv)) return snap_refuse(dst, who + ": bad argument (a NULL source)");
    if (dst == src) return snap_refuse(dst, who + ": the source is the destination");
    if (sv.ctx != v.ctx) return snap_refuse(dst, who + ": the two maps are on different contexts");
    const MergeFrom from{nullptr, nullptr, &sv};
    return map_merge(dst, v, from, sign, who);
}

}  // extern "C"
