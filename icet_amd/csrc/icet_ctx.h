// icet_amd/csrc/icet_ctx.h -- what the two host translation units share: the context (icet_capi.hip owns it), the keyframe store that borrows one (icet_store.hip
// owns it; the indexed registrations read its tables), the argument checks, the two protocols around the context -- who writes the pinned descriptor staging and
// when (staging_*), and how an entry that enqueues begins (enter) --, and the indexed registrations both run.
#pragma once
#include "../../include/icet_hip.h"
#include "icet_internal.h"
#include "icet_buffers.h"
#include "icet_appearance.h"
#include "icet_coarse.h"

#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

namespace icet {
// A READ FENCE: a pinned staging that the host writes and a copy or kernel on the stream reads when it RUNS.  The owner calls wait() before the host writes the
// staging again and mark(stream) behind whatever it enqueued to read it; destroy() goes with the owner.  The codes are the runtime's: an owner wraps them in its
// own check macro.  (The descriptor staging, staging_* below, is not one of these: it has a second reader, the replayed graph, and rules under capture.)
struct ReadFence {
    hipEvent_t ev = nullptr; bool pending = false;                // pending: a reader was marked and not waited for since
    hipError_t wait() {
        if (!pending) return hipSuccess;
        const hipError_t e = hipEventSynchronize(ev);
        if (e == hipSuccess) pending = false;
        return e;
    }
    hipError_t mark(hipStream_t stream) {
        hipError_t e = ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ev, stream);
        if (e == hipSuccess) pending = true;
        return e;
    }
    void destroy() { if (ev) (void)hipEventDestroy(ev); ev = nullptr; pending = false; }
};
}  // namespace icet

struct icet_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    icet::Workspace w;
    icet::Tuning tune;                    // icet_set_option
    int32_t kf_pairs = 0; icet_params kf_params{};      // a keyframe parked by icet_keyframe_device (0 pairs = none)
    int max_lds = 160 * 1024;       // hipDeviceAttributeMaxSharedMemoryPerBlock of the device
    int lds_rank_ok = 0;            // this device passed lds_rank_selftest (icet_create)
    uint32_t kf_row_mask = 0xFFFFFFFFu;   // the row's bits of a word of w.src as the last keyframe build left it (packed rows, LaunchCfg::packed_rows): icet_debug_fetch hands out plain rows
    std::string err;
    // host staging (pinned) for descriptors and results
    icet::PairDesc* h_desc = nullptr; int32_t* h_seg = nullptr; int32_t h_cap_pairs = 0;
    bool desc_kf_valid = false, desc_reg_valid = false;   // the pinned descriptors hold what the last icet_keyframe_device_n / icet_register_device_n call wrote (any other writer, and a re-allocation, clears both)
    icet::PairDesc* h_desc_rt = nullptr; int32_t h_cap_rt = 0;       // ICET_FLAG_ROUNDTRIP_SCAN2: descriptors of the round-tripped copy of scan 2
    icet::PairDesc* h_desc_reg = nullptr; int32_t* h_kf_of = nullptr;  // staging of an indexed call (icet_register_indexed_device), w.cap_regs (+ 1): apart from h_desc, whose scan-1 halves the same_desc shortcut keeps
    int64_t ws_gen = 0;                                          // counts re-allocations of workspace buffers (part of the indexed call's graph key)
    // device staging for host-pointer entry points
    float* d_stage1 = nullptr; float* d_stage2 = nullptr; int64_t cap_stage1 = 0, cap_stage2 = 0;
    float* d_out = nullptr; float* d_x0 = nullptr; int32_t cap_out_pairs = 0;
    float* h_out = nullptr;
    // aux (single pair): every side table of a solve lives in ONE device block (`d_pack`, words of 4 bytes, layout aux_layout()) behind the
    // 48 result floats, so that results and side tables come back in one DMA into the pinned `h_pack`
    icet::AuxDev aux_dev{}; int aux_V = 0, aux_runlen = 0;
    uint32_t* d_pack = nullptr; uint32_t* h_pack = nullptr; size_t cap_pack = 0;
    float* h_pts2 = nullptr; float* d_pts2 = nullptr; size_t cap_pts2 = 0;   // `points2` (scan 2 under the last iteration's transform): device buffer + pinned host copy
    float* h_x0 = nullptr;                                       // pinned, 6 x cap_out_pairs
    icet_score* d_score = nullptr; icet_score* h_score = nullptr; int32_t cap_score = 0;     // scores of the host-pointer entry points (device + pinned)
    int32_t* d_sel = nullptr; int32_t* h_sel = nullptr; int64_t cap_sel = 0;                // icet_select_best_device: the groups' members | offsets (device + pinned staging)
    icet::ReadFence sel_read;                                                                // the copy out of h_sel
    float* d_sph1 = nullptr; int32_t* d_idx1 = nullptr; size_t cap_side1 = 0;      // points1Spherical / pointIndices1 on request (icet_sidetables.hip)
    float* d_sph2 = nullptr; int32_t* d_vox2 = nullptr; size_t cap_side2 = 0;      // points2Spherical / the rows' voxels on request
    // host-pointer entry points: scan 2 is uploaded on a stream of its own, beside the keyframe build of scan 1
    hipStream_t st_copy = nullptr; hipEvent_t ev_s2 = nullptr;
    hipEvent_t ev_kf = nullptr, ev_kfd = nullptr, ev_prev = nullptr, ev_pts2 = nullptr;   // keyframe built / its tables on the host / transform of the last iteration known / points2 on the host
    // icet_solve_begin .. icet_solve_end
    struct Pending { bool active = false; float* x_out = nullptr; float* ps_out = nullptr; float* cov_out = nullptr; icet_aux aux{}; bool has_aux = false;
                     int V = 0, rl = 0; int64_t n2 = 0; bool kf_tables = false, kf_done = false, pts2 = false, pts2_dev = false, tail_ints = false, side1 = false, side2 = false; int64_t n1 = 0;
                     const float* scan2 = nullptr; int64_t ld2 = 0; } pend;
    // timing
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr;
    std::vector<hipEvent_t> ev_acc;
    float last_ms[4] = {0, 0, 0, 0};
    bool timing_valid = false;
    int last_iters = 0;
    // Large device batches are cut into contiguous parts, each solved by a helper context on its own stream, so that
    // the keyframe build of one part (latency / LDS bound) overlaps the Gauss-Newton loop of another (VALU bound).
    std::vector<icet_ctx*> helpers;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_stage = nullptr; int stage_at = 0;            // see LaunchCfg::stage_event
    hipEvent_t ev_desc = nullptr; bool desc_in_flight = false;   // the last copy or kernel that read the pinned descriptor staging (staging_mark_read / staging_wait, below: nobody else touches them)
    // Small device batches whose launch geometry repeats call after call are replayed from a captured hipGraph (option "graph"): the ~33
    // launches of a single-pair solve then cost one hipGraphLaunch on the host, and the command processor runs them back to back.
    // What a captured graph depends on apart from the staging it re-reads (graph_key_of, icet_capi.hip): two calls with equal keys enqueue the same launches with
    // the same arguments.  Compared with memcmp: value-initialised, every member 8 bytes wide, no padding (the static_assert below the struct).
    enum GraphEntry : int64_t { kEntrySolve, kEntryKeyframe, kEntryLoop, kEntryIndexed };      // icet_solve_batch_device, icet_keyframe_device_n, icet_register_device_n, register_indexed
    struct GraphKey {
        int64_t entry, mode;                                   // GraphEntry; the IndexedMode of an indexed call (0 elsewhere)
        const void* x0; const void* out; const void* extra;    // the caller's argument pointers; extra: d_rows of the two halves, d_score of a scored call
        int64_t ws_gen, src_id, src_gen;                       // indexed calls: any workspace buffer moved; the keyframe tables -- 0 / 0 the context's own, else a store's id and generation
        int64_t prologue_key; const void* done_flag; int64_t flags;      // the prologue's key (0: none), the word the last solve raises, icet_params::flags
        const void* ws[9];                                     // desc, thr, lut, r1, counts, near_over, acc, fit_items, tile_vr
        int64_t launch[29];                                   // what the launches take of the plan (launch_key_of, icet_capi.hip)
    };
    struct GraphSlot {
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; GraphKey key{}, seen{}; bool have_seen = false, have_graph = false;
        void reset() { if (have_graph) { (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph); } graph = nullptr; exec = nullptr; have_graph = false; }      // (have_seen stays: the key may be captured again)
    };
    int pg_solver = 0;                                         // icet_pose_graph_optimize: 0 conjugate gradients, 1 the direct solve, 2 auto (option "pg_solver")
    bool capturing = false; int graph_mode = -1;               // -1: replay batches of <= 8 pairs whose launch key repeats; 0 never; 1 same as -1
    GraphSlot g_solve, g_keyframe, g_loop, g_indexed;          // the whole solve (icet_solve_batch_device), its two halves (icet_keyframe_device_n / icet_register_device_n), indexed registrations
    GraphSlot g_scored, g_score;                               // indexed registrations + score (icet_register_indexed_scored_device), the score of given poses (icet_score_indexed_device)
    hipEvent_t ev_graph = nullptr; bool graph_in_flight = false;      // the last replay, which re-reads that staging when it runs (staging_mark_replay / staging_wait)
    // A caller inside this library (the sequential nodes, icet_nodes.hip) can put work of its own at the head of the NEXT icet_register_device_n call's launch
    // sequence -- enqueued on the context's stream right before the loop's first kernel, captured into the same graph: the range filter and the loop of a frame
    // are then ONE hipGraphLaunch (round 6: the loop's graph used to start 30-40 us after the filter's last kernel).  `prologue_key` names what the hook's
    // launches depend on (buffers, grid): it is part of the graph key.  Cleared by the caller after the call (icet_ctx_set_prologue).
    // A ragged throughput batch is laid out XCD-balanced (solve_device_part): slot s of the internal tables holds the caller's pair h_seg[n_pairs + 1 + s]
    bool perm_active = false; int32_t perm_pairs = 0;
    hipError_t (*prologue)(void*, hipStream_t) = nullptr; void* prologue_user = nullptr; int64_t prologue_key = 0;
    // ... and have the LAST solve of the next icet_register_device_n call store 1 into a word of (coherent) pinned host memory once the results are written: the caller
    // watches that word instead of synchronising the stream (icet_ctx_set_done_flag; part of the graph key)
    int32_t* done_flag = nullptr;
    // icet_sync after ONE small device-resident solve (icet_solve_batch_device, replayed graph) watches a word of its own the same way: h_sync_word, raised by that solve's
    // last kernel.  armed_calls counts such solves since the last icet_sync; anything else enqueued on the context (or a second solve, whose reset of the word races with the
    // first one's store) makes it 2 or more and icet_sync synchronises the stream as before.
    int32_t* h_sync_word = nullptr; int armed_calls = 2;
    int map_lds = 1;                                             // option "map_lds": a voxel map's add reduces a block's rows in LDS first (icet_map.hip)
    int map_query_prune = 1;                                     // option "map_query_prune": a voxel map's query skips the chunks outside a pose's run of x cells
    int map_evidence_prune = 1;                                  // option "map_evidence_prune": the same for the scans of a voxel map's evidence (icet_map.hip)
    int map_evidence_batch = 0;                                  // option "map_evidence_batch": scans per batch of range images; 0: as many as fit 64 MiB, 1 .. 256
    int64_t map_snapshot_chunk_entries = 0;                    // option "map_snapshot_chunk_entries": entries per chunk of a voxel map's save / load (0: 2^20; icet_map_snapshot.hip)
    int64_t snapshot_chunk_bytes = 0;                          // option "snapshot_chunk_bytes": payload bytes per chunk of a store's save / load (0: 64 MiB)
    // Who owns what w and the pointers above point at: one group per set of arrays that grows together (the ensure_* functions of icet_capi.hip).  delete frees them (last member: gone first).
    struct Mem {
        icet::BufferGroup pairs, regs, scan1, fit, scan2, lut, keep_mask, keep_list, keep_pairs, counts, tile_vr, rt2, rt_desc;      // what w points at (+ the pinned staging sized with it)
        icet::BufferGroup out, stage1, stage2, pack, pts2, side1, side2, score, sel, sync_word;
    } mem;
};
static_assert(std::has_unique_object_representations_v<icet_ctx::GraphKey> && sizeof(icet_ctx::GraphKey) == 8 * (20 + 29), "GraphKey is compared with memcmp: 8-byte integers and pointers, no padding");

// A keyframe store (include/icet_hip.h icet_keyframe_store_*): `capacity` rows of the four keyframe tables in the layout of the workspace's
// keyframe side (row stride V; (V + 1) & ~1 for slot_of_voxel), on the borrowed context's device.  A put builds on the context and parks into rows of its own
// (k_keyframe_store_park); the indexed calls read a row the way they read a parked keyframe.  id (never reused) and gen (bumped when the tables move) name
// the tables in the graph key of an indexed call.
struct icet_keyframe_store {
    icet_ctx* ctx = nullptr;
    icet_params shape{};                       // bins_phi, bins_theta, n, thresh, buff, flags & (TRUE_SORT | HALF_GAP_BOUNDS); runlen 0
    int V = 0; int32_t capacity = 0;
    icet::SlotHot* hotS = nullptr; icet::SlotFit* fitS = nullptr; int16_t* slot_of_voxel = nullptr; int32_t* n_slots = nullptr;
    std::vector<uint8_t> occupied;             // capacity: the rows a put has filled
    int64_t id = 0, gen = 0;
    std::string err;
    // the pose table: ONE allocation of capacity x 56 bytes at pose_stamp -- stamp[capacity] | tx | ty | tz | r0 .. r8 --, 0xFF bytes
    // (NaN, stamp -1) where a slot has no pose; set_pose stages through h_pose (pinned), which its kernel reads when it runs (pose_read: it has)
    int64_t* pose_stamp = nullptr;
    icet::PoseTable pose_table() const { return icet::PoseTable{pose_stamp, reinterpret_cast<float*>(pose_stamp + capacity), capacity}; }
    icet::PoseUpload* h_pose = nullptr; int32_t cap_h_pose = 0; icet::ReadFence pose_read;
    // buffers of a query (icet_keyframe_store_close_device), grown on demand: the search's per-tile lists; per (query, candidate); per registration; per query
    unsigned long long* q_part = nullptr; size_t cap_part = 0;
    unsigned long long* q_keys = nullptr; int32_t* q_cand = nullptr; int32_t cap_qk = 0;
    float* q_x0 = nullptr; float* q_out = nullptr; icet_score* q_score = nullptr; int32_t* q_kf_of = nullptr; int32_t* q_rows = nullptr; int32_t* q_members = nullptr; int32_t cap_qr = 0;
    int32_t* q_offs = nullptr; int32_t* q_best = nullptr;       // kClosureMaxQueries + 1, kClosureMaxQueries
    // place recognition by appearance: null until icet_keyframe_store_enable_appearance
    struct Appearance {
        icet_appearance_rule::Consts k{}; int Rp = 0;             // Rp: words per column, ceil(rings / 4)
        icet_appearance_params params{};                          // as enable_appearance took them (a snapshot file names them)
        uint32_t* desc = nullptr; float* w = nullptr; int32_t* has = nullptr;      // the table: capacity rows (AppTable)
        std::vector<uint8_t> has_h;                               // capacity: the slots a put has given a descriptor
        uint32_t* scratch = nullptr;                              // kAppBatch x rings x sectors words, zero between calls
        uint32_t* qdesc = nullptr; float* qw = nullptr; int32_t* qhas = nullptr;   // the descriptors of a call's queries: a table of kAppBatch rows
        unsigned long long* keys_all = nullptr; uint16_t* shift_all = nullptr; size_t cap_all = 0;      // n_queries x capacity, grown on demand
        int32_t* shift_of = nullptr;                              // kClosureMaxQueries x kClosureMaxCandidates: the candidates' shifts, for the record
        icet::BufferGroup table, work, all;                       // owners: desc / w / has (swapped by a reserve); keys_all / shift_all (cap_all); everything else
    };
    Appearance* app = nullptr;
    icet::AppTable app_table() const { return icet::AppTable{app->desc, app->w, app->has, capacity, app->k.A, app->Rp}; }
    // coarse alignment: null until icet_keyframe_store_enable_coarse
    struct Coarse {
        icet_coarse_rule::Consts k{};
        icet_coarse_params params{};                              // as enable_coarse took them (a snapshot file names them)
        uint32_t* grid = nullptr; int32_t* has = nullptr;         // the table: capacity rows of G x G / 32 words (CoarseTable)
        std::vector<uint8_t> has_h;                               // capacity: the slots a put has given a grid
        uint32_t* scratch = nullptr;                              // kCoarseBatch x 2 x G x G words, zero between calls
        uint32_t* qgrid = nullptr;                                // the own grids of a call's queries: kAppBatch rows
        // per (query, candidate) of the largest call: base starts, coarse starts, matches, keys, slot bit counts; per hypothesis: transforms and live bit counts
        float* base = nullptr; icet_coarse_match* match = nullptr; unsigned long long* keys = nullptr; int32_t* key_bits = nullptr;
        icet::CoarseHyp* hyp = nullptr; int32_t* live_bits = nullptr;
        icet::BufferGroup table, work;                            // owners: grid / has (swapped by a reserve); everything else
        size_t row_words() const { return (size_t)k.G * (size_t)k.W; }
    };
    Coarse* coarse = nullptr;
    icet::CoarseTable coarse_table() const { return icet::CoarseTable{coarse->grid, coarse->has, capacity}; }
    // who owns the arrays of this struct (icet_buffers.h): the four tables + the pose table, which a reserve swaps for larger ones; the pinned pose staging; the
    // query buffers, one group per capacity (fixed-size, cap_part, cap_qk, cap_qr)
    icet::BufferGroup tables, pose_stage, q_fixed, q_part_mem, q_qk_mem, q_qr_mem;
};

namespace icet {

#define HIPCHK(ctx, call) do { const hipError_t e_ = static_cast<hipError_t>(call); if (e_ != hipSuccess) { \
    (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); \
    return e_ == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; } } while (0)

#define ICET_TRY(call) do { const icet_status s_ = (call); if (s_ != ICET_OK) return s_; } while (0)

static inline bool params_ok(const icet_params* p) {
    if (!p) return false;
    if (p->runlen < 0 || p->runlen > 4096) return false;
    if (p->bins_phi <= 0 || p->bins_theta <= 0 || p->n < 1) return false;
    return true;
}

// ---- the pinned descriptor staging: h_desc / h_seg, h_desc_reg / h_kf_of, h_desc_rt ------------------------------------------------
// The host writes any of them only behind staging_wait; whoever enqueues a reader calls staging_mark_read behind it; nobody else touches the two flags.

// Before the host writes the staging: the last copy out of it has run, and so has the last replayed graph, which re-reads it when it RUNS.
static inline icet_status staging_wait(icet_ctx* c) {
    if (c->desc_in_flight) { HIPCHK(c, hipEventSynchronize(c->ev_desc)); c->desc_in_flight = false; }
    if (c->graph_in_flight) { HIPCHK(c, hipEventSynchronize(c->ev_graph)); c->graph_in_flight = false; }
    return ICET_OK;
}
// The stream has been synchronised: nothing reads the staging.
static inline void staging_idle(icet_ctx* c) { c->desc_in_flight = false; c->graph_in_flight = false; }
// Behind the copy or kernel that reads the staging.  A captured event cannot be waited for on the host -- the replay path orders the staging itself (ev_graph) --,
// so a capture records nothing; in_capture_too: the caller's path is one no graph replays, and it records whatever the flag says.
static inline icet_status staging_mark_read(icet_ctx* c, bool in_capture_too = false) {
    if (c->capturing && !in_capture_too) return ICET_OK;
    if (!c->ev_desc) HIPCHK(c, hipEventCreateWithFlags(&c->ev_desc, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_desc, c->stream)); c->desc_in_flight = true;
    return ICET_OK;
}
// Behind a replayed graph, which re-reads the staging when it runs (run_or_replay, which created ev_graph before its first capture).
static inline icet_status staging_mark_replay(icet_ctx* c) { HIPCHK(c, hipEventRecord(c->ev_graph, c->stream)); c->graph_in_flight = true; return ICET_OK; }
// n descriptors (hd) and seg_words segment words (hs) to wv.desc / wv.seg_off, one of three ways: the caller's next kernel copies the pinned words itself; a small
// batch: k_upload_desc reads them (no copy command, no memcpy node); else two copies.  The caller marks the staging read behind whichever reads it.
static inline icet_status staging_upload(icet_ctx* c, const Workspace& wv, const PairDesc* hd, const int32_t* hs, int32_t n, size_t seg_words, bool by_next_kernel) {
    if (by_next_kernel) return ICET_OK;
    if (n <= kUploadDescMaxPairs) { HIPCHK(c, launch_upload_desc(wv, hd, hs, n, c->stream)); return ICET_OK; }
    HIPCHK(c, hipMemcpyAsync(wv.desc, hd, sizeof(PairDesc) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(wv.seg_off, hs, sizeof(int32_t) * seg_words, hipMemcpyHostToDevice, c->stream));
    return ICET_OK;
}

// ---- the entry step -------------------------------------------------------------------------------------------------------------------
// An entry that enqueues on the context's stream begins with enter(): the context (or store) is there, its device is current, and the sync word is disarmed, so
// that icet_sync behind it synchronises the stream.  The one arming entry, icet_solve_batch_device, begins with use_device() and counts armed_calls itself
// (solve_device_part).  Every extern "C" function that takes a context or a store:
//   disarms (enter)          icet_keyframe_device[_n], icet_register_device[_n], icet_register_indexed[_scored]_device, icet_score_indexed_device, icet_debug_point_sums_device,
//                            icet_debug_gn_terms_device (register_indexed); icet_solve_indexed[_scored], icet_score_indexed, icet_solve_batch, icet_solve_begin / icet_solve
//                            (all three also drain, or icet_solve_end does); icet_select_best_device; icet_keyframe_store_create (*), _put_device, _register[_scored]_device,
//                            _score_device, _set_pose, _set_stamp, _candidates[_appearance]_device, _describe_device, _coarse_grid_device, _coarse_align_device,
//                            _close[_appearance|_coarse]_device; icet_keyframe_store_save, _load (drain as well); icet_pose_graph_optimize[_device],
//                            icet_debug_pose_graph_step, _direct, icet_pose_graph_marginals[_device], icet_debug_pose_graph_marginals (pg_run: drains as well);
//                            icet_voxel_map_create, _clear, _add_device, _add_posed_device; _stats, _extract_device, _extract (drain as well; icet_map.hip);
//                            icet_voxel_map_index, _query_device, _query_posed_device (drain only when the index is stale and they rebuild it);
//                            icet_voxel_map_evidence_device, _evidence_posed_device (the same, and when their buffers grow or *out is asked for), _evidence_fetch_device
//                            icet_voxel_map_register_device, _register_posed_device, icet_debug_voxel_map_register_terms (drain only when their buffers grow; icet_map_register.hip)
//                            icet_voxel_map_save, _load (drain as well), _merge_device (drains once, for its capacity check; icet_map_snapshot.hip)
//                            icet_deskewer_create, icet_deskew_device, icet_deskew_twists_from_poses_device (drain only when the records' stage grows); icet_deskew (drains as well; icet_deskew.hip)
//   arms or disarms itself   icet_solve_batch_device
//   drains before it returns icet_debug_gn_tail, icet_debug_pinv3, icet_debug_pinv3_double, icet_debug_fix, icet_debug_spherical, icet_debug_block_tridiag (copy in, one kernel, copy out,
//                            synchronise); icet_debug_fetch, icet_keyframe_store_debug_fetch, icet_keep_stats (synchronise, then blocking copies);
//                            icet_last_timing[_iters] (synchronise); icet_solve_end; icet_keyframe_store_reserve, _enable_appearance, _enable_coarse, _destroy;
//                            icet_voxel_map_destroy; icet_deskewer_destroy; icet_destroy; icet_sync (the only one that re-arms: armed_calls = 0; icet_solve_indexed and its kin do the same behind their own drain)
//   enqueues nothing         icet_reserve (allocations and blocking memsets; a growth synchronises first), icet_solve_keyframe_tables (waits for an event),
//                            icet_set_option, icet_last_error, icet_stream, icet_device, icet_create (armed_calls starts at 2), icet_keyframe_store_last_error, icet_voxel_map_last_error,
//                            icet_deskewer_last_error, icet_twist_from_pose, icet_pose_from_twist, icet_debug_deskew_rows (no context)
// (*) the one entry the audit found enqueuing (two memsets of the new tables) without draining or disarming.
static inline icet_status use_device(icet_ctx* c) {
    if (!c) return ICET_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return ICET_OK;
}
static inline icet_status enter(icet_ctx* c) {
    const icet_status s = use_device(c);
    if (s == ICET_OK) c->armed_calls = 2;
    return s;
}
static inline icet_status enter(icet_keyframe_store* s) {
    if (!s) return ICET_ERR_BAD_ARG;
    const icet_status st = enter(s->ctx);
    if (st != ICET_OK) s->err = s->ctx->err;
    return st;
}

// What makes a keyframe: two calls with the same values here read and write the same tables.
static inline bool same_keyframe_shape(const icet_params& a, const icet_params& b) {
    return a.bins_phi == b.bins_phi && a.bins_theta == b.bins_theta && a.n == b.n && a.thresh == b.thresh && a.buff == b.buff &&
           !((a.flags ^ b.flags) & (ICET_FLAG_TRUE_SORT | ICET_FLAG_HALF_GAP_BOUNDS));
}

// The indexed registrations of icet_register_indexed_device (mode kIdxRegister), the same followed by the score (kIdxScored: d_score), or the score of the poses
// d_x0 alone (kIdxScoreOnly: no iteration, d_out unused).  src: the keyframe tables -- nullptr the context's parked keyframe (kf_index: parked keyframes), or a
// keyframe store (kf_index: its occupied slots; icet_keyframe_store_register_device and its kin).  dev: keyframe index and row count of every registration as
// kernels in front of the call left them on the device (a closure query; never captured into a graph).
enum IndexedMode { kIdxRegister = 0, kIdxScored = 1, kIdxScoreOnly = 2, kIdxDump = 3, kIdxTerms = 4 };      // kIdxDump (icet_debug_point_sums_device): kIdxScoreOnly with the raw per-voxel sums (d_dump) in place of the score
// kIdxTerms (icet_debug_gn_terms_device): the point pass at d_x0, the raw sums copied out and LEFT IN PLACE (d_dump), the transform record, then the production solve of
// iteration runlen - 1 on those very records: its H^T W H and H^T W dz, and its results in d_out.  Never captured into a graph.
struct GnTermsOut { float* xf; float* htwh; float* htwdz; };
struct IndexedDev { const int32_t* kf_of; const int32_t* rows; };
__attribute__((visibility("hidden")))
icet_status register_indexed(icet_ctx* c, const icet_params* p, int32_t n_regs, const int32_t* kf_index, const icet_dev_scan* scan2, const float* d_x0, float* d_out,
                             icet_score* d_score, IndexedMode mode, const icet_keyframe_store* src = nullptr, const IndexedDev* dev = nullptr, uint32_t* d_dump = nullptr, const GnTermsOut* terms = nullptr);

}  // namespace icet
