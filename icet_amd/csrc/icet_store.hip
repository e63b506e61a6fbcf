// icet_amd/csrc/icet_store.hip -- the keyframe store of the C ABI (include/icet_hip.h icet_keyframe_store_*; DESIGN.md sections 15 - 19): slots of keyframes on a
// borrowed context's device, their poses, descriptors and grids, and the closure queries.  The registrations themselves are the context's indexed call
// (register_indexed, icet_capi.hip); the kernels are icet_kfstore.hip, icet_closure.hip, icet_appearance.hip, icet_coarse.hip and icet_snapshot.hip.
#include "../../include/icet_hip.h"
#include "icet_ctx.h"
#include "icet_closure.h"
#include "icet_appearance.h"
#include "icet_coarse.h"
#include "icet_snapshot.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace icet;

extern "C" {

// ---- the keyframe store ----------------------------------------------------------------------------------------
#define STORECHK(s, call) do { const hipError_t e_ = static_cast<hipError_t>(call); if (e_ != hipSuccess) { \
    (s)->err = std::string(#call) + ": " + hipGetErrorString(e_); \
    return e_ == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP; } } while (0)

constexpr size_t kPoseBytes = sizeof(int64_t) + 12 * sizeof(float);      // the pose table, per slot (icet_keyframe_store::pose_table)

// The slots a call names: every one a slot of the store -- an occupied one, unless the call is the put that fills it -- and none named twice.
static icet_status slots_ok(icet_keyframe_store* s, int32_t n, const int32_t* slots, bool occupied, const char* call) {
    std::vector<uint8_t> named((size_t)s->capacity, 0);
    for (int k = 0; k < n; k++) {
        const int32_t sl = slots[k];
        const std::string which = "slots[" + std::to_string(k) + "] = " + std::to_string(sl);
        if (!occupied && (sl < 0 || sl >= s->capacity)) { s->err = which + " is not a slot (0 .. " + std::to_string(s->capacity - 1) + ")"; return ICET_ERR_BAD_ARG; }
        if (occupied && (sl < 0 || sl >= s->capacity || !s->occupied[(size_t)sl])) { s->err = which + " is not an occupied slot of the store (capacity " + std::to_string(s->capacity) + ")"; return ICET_ERR_BAD_ARG; }
        if (named[(size_t)sl]) { s->err = "slot " + std::to_string(sl) + " is named twice in one " + call; return ICET_ERR_BAD_ARG; }
        named[(size_t)sl] = 1;
    }
    return ICET_OK;
}

// The n device scans of a call.
static icet_status scans_ok(icet_keyframe_store* s, int32_t n, const icet_dev_scan* scan) {
    if (n > 0 && !scan) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    for (int k = 0; k < n; k++) if (!dev_scan_ok(scan[k])) { s->err = "bad scan descriptor"; return ICET_ERR_BAD_ARG; }
    return ICET_OK;
}

// The allocators of the store's tables: each allocates INTO a group (the store's own, or the local one a reserve builds beside it), always in the same order, so
// that two groups filled by the same allocator can be swapped.  All or nothing for the caller: what a failed run got is freed with its group.
static_assert(kPoseBytes == 7 * sizeof(int64_t), "the pose table is allocated as 7 words of 8 bytes per slot");
static int store_alloc(BufferGroup& g, int V, int32_t cap, SlotHot*& hot, SlotFit*& fit, int16_t*& sov, int32_t*& ns, int64_t*& pose) {
    int e = g.device(hot, (size_t)cap * V);
    if (!e) e = g.device(fit, (size_t)cap * V);
    if (!e) e = g.device(sov, (size_t)cap * ((V + 1) & ~1));
    if (!e) e = g.device(ns, (size_t)cap);
    if (!e) e = g.device(pose, 7 * (size_t)cap);
    return e;
}

// The descriptor table of `cap` rows (row: `row_words` words of columns, `cols` weights).
static int app_alloc_table(BufferGroup& g, size_t row_words, size_t cols, int32_t cap, uint32_t*& desc, float*& w, int32_t*& has) {
    int e = g.device(desc, row_words * (size_t)cap);
    if (!e) e = g.device(w, cols * (size_t)cap);
    if (!e) e = g.device(has, (size_t)cap);
    return e;
}

// The grid table of `cap` rows of `row_words` words.
static int coarse_alloc_table(BufferGroup& g, size_t row_words, int32_t cap, uint32_t*& grid, int32_t*& has) {
    int e = g.device(grid, row_words * (size_t)cap);
    if (!e) e = g.device(has, (size_t)cap);
    return e;
}

// (e: a hipError_t, as the runtime or a group returned it)
static icet_status store_fail(icet_keyframe_store* s, const char* what, int e) {
    (void)hipGetLastError();
    s->err = std::string(what) + ": " + hipGetErrorString(static_cast<hipError_t>(e));
    return e == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP;
}

const char* icet_keyframe_store_last_error(const icet_keyframe_store* s) { return s ? s->err.c_str() : "null store"; }

icet_status icet_keyframe_store_create(icet_ctx* c, const icet_params* p, int32_t capacity, icet_keyframe_store** out) {
    if (out) *out = nullptr;
    if (!c) return ICET_ERR_BAD_ARG;
    if (!out || !p || p->bins_phi <= 0 || p->bins_theta <= 0 || p->n < 1 || capacity < 1) { c->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if ((int64_t)p->bins_phi * p->bins_theta > kMaxVoxels) { c->err = "bins_phi*bins_theta exceeds the voxel limit (10000)"; return ICET_ERR_UNSUPPORTED; }
    const int V = p->bins_phi * p->bins_theta;
    if ((size_t)V * 12 + 8 + 4096 > (size_t)c->max_lds) { c->err = "grid too fine for this device's LDS (k_bin_scatter keeps 12 B per voxel in one block)"; return ICET_ERR_UNSUPPORTED; }
    ICET_TRY(enter(c));                                      // (the memsets below are enqueued and not waited for)
    icet_keyframe_store* s = new (std::nothrow) icet_keyframe_store();
    if (!s) { c->err = "host allocation failed"; return ICET_ERR_NOMEM; }
    static std::atomic<int64_t> next_id{1};
    s->ctx = c; s->V = V; s->capacity = capacity; s->id = next_id++;
    s->shape = *p; s->shape.runlen = 0; s->shape.flags = p->flags & (ICET_FLAG_TRUE_SORT | ICET_FLAG_HALF_GAP_BOUNDS);
    int z = store_alloc(s->tables, V, capacity, s->hotS, s->fitS, s->slot_of_voxel, s->n_slots, s->pose_stamp);
    s->occupied.assign((size_t)capacity, 0);
    if (z == hipSuccess) z = hipMemsetAsync(s->pose_stamp, 0xFF, kPoseBytes * (size_t)capacity, c->stream);      // no slot has a pose
    if (z == hipSuccess) z = hipMemsetAsync(s->n_slots, 0, sizeof(int32_t) * (size_t)capacity, c->stream);
    if (z != hipSuccess) { const icet_status st = store_fail(s, "keyframe store", z); c->err = s->err; (void)icet_keyframe_store_destroy(s); return st; }
    *out = s;
    return ICET_OK;
}

icet_status icet_keyframe_store_destroy(icet_keyframe_store* s) {
    if (!s) return ICET_ERR_BAD_ARG;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);              // (a put or a registration may still read or write the tables)
    s->pose_read.destroy();
    delete s->app;                                           // (every array belongs to a group of its struct)
    delete s->coarse;
    delete s;
    return ICET_OK;
}

icet_status icet_keyframe_store_reserve(icet_keyframe_store* s, int32_t capacity) {
    if (!s) return ICET_ERR_BAD_ARG;
    if (capacity <= s->capacity) return ICET_OK;
    icet_ctx* c = s->ctx;
    STORECHK(s, hipSetDevice(c->device));
    STORECHK(s, hipStreamSynchronize(c->stream));            // nothing on the stream reads the old tables any more
    // Every new table goes into a LOCAL group beside the one it will replace.  A failure returns: the locals free what they got and the store is untouched.
    SlotHot* hot = nullptr; SlotFit* fit = nullptr; int16_t* sov = nullptr; int32_t* ns = nullptr; int64_t* pose = nullptr;
    uint32_t* adesc = nullptr; float* aw = nullptr; int32_t* ahas = nullptr;
    uint32_t* cgrid = nullptr; int32_t* chas = nullptr;
    BufferGroup tables, app_table, coarse_table;             // (behind their slots: a group nulls them when it goes)
    const size_t old = (size_t)s->capacity, V = (size_t)s->V;
    const size_t arow = s->app ? (size_t)s->app->k.A * (size_t)s->app->Rp : 0, acol = s->app ? (size_t)s->app->k.A : 0;
    int e = store_alloc(tables, s->V, capacity, hot, fit, sov, ns, pose);
    if (e == hipSuccess && s->app) e = app_alloc_table(app_table, arow, acol, capacity, adesc, aw, ahas);
    if (e == hipSuccess && s->coarse) e = coarse_alloc_table(coarse_table, s->coarse->row_words(), capacity, cgrid, chas);
    // descriptors (a store with appearance enabled): the first `old` rows carried over, no descriptor behind them
    if (e == hipSuccess && s->app) {
        e = hipMemsetAsync(ahas, 0, sizeof(int32_t) * (size_t)capacity, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ahas, s->app->has, sizeof(int32_t) * old, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(adesc, s->app->desc, sizeof(uint32_t) * arow * old, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(aw, s->app->w, sizeof(float) * acol * old, hipMemcpyDeviceToDevice, c->stream);
    }
    // grids (a store with coarse alignment enabled): likewise
    if (e == hipSuccess && s->coarse) {
        e = hipMemsetAsync(chas, 0, sizeof(int32_t) * (size_t)capacity, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(chas, s->coarse->has, sizeof(int32_t) * old, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cgrid, s->coarse->grid, sizeof(uint32_t) * s->coarse->row_words() * old, hipMemcpyDeviceToDevice, c->stream);
    }
    // poses and stamps: the new table starts empty (0xFF), then every array's first `old` entries are carried over
    if (e == hipSuccess) e = hipMemsetAsync(pose, 0xFF, kPoseBytes * (size_t)capacity, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(pose, s->pose_stamp, sizeof(int64_t) * old, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpy2DAsync(pose + capacity, sizeof(float) * (size_t)capacity, s->pose_stamp + old, sizeof(float) * old, sizeof(float) * old, 12, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hot, s->hotS, sizeof(SlotHot) * old * V, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(fit, s->fitS, sizeof(SlotFit) * old * V, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sov, s->slot_of_voxel, sizeof(int16_t) * old * ((V + 1) & ~(size_t)1), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ns, s->n_slots, sizeof(int32_t) * old, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ns + old, 0, sizeof(int32_t) * ((size_t)capacity - old), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);                   // (no copy still writes what the local groups are about to free)
        return store_fail(s, "keyframe store reserve", e);
    }
    // the swap: every slot of the store now points at its new table, and the local groups free the old ones as they go out of scope
    if (s->coarse) { s->coarse->table.swap(coarse_table); s->coarse->has_h.resize((size_t)capacity, 0); }
    if (s->app) {
        s->app->table.swap(app_table); s->app->has_h.resize((size_t)capacity, 0);
        s->app->cap_all = 0;                                     // (the per-slot buffers of a search are sized by the capacity)
    }
    s->tables.swap(tables);
    s->capacity = capacity; s->occupied.resize((size_t)capacity, 0);
    s->gen++;                                                // the tables moved: no graph captured against the old ones is replayed
    return ICET_OK;
}

static icet_status app_put_batch(icet_keyframe_store* s, const icet_dev_scan* scan, const int32_t* d_rows, int cnt, const StoreParkSlots& dst);
static icet_status coarse_put_batch(icet_keyframe_store* s, const icet_dev_scan* scan, const int32_t* d_rows, int cnt, const StoreParkSlots& dst);

icet_status icet_keyframe_store_put_device(icet_keyframe_store* s, int32_t n, const int32_t* slots, const icet_dev_scan* scan1, const int32_t* d_rows) {
    ICET_TRY(enter(s));
    icet_ctx* c = s->ctx;
    if (n < 0 || (n > 0 && (!slots || !scan1))) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (n == 0) return ICET_OK;
    // everything is checked before anything is touched: a refused put leaves every slot and the context's parked keyframe as they were
    icet_status st = slots_ok(s, n, slots, false, "put");
    if (st == ICET_OK) st = scans_ok(s, n, scan1);
    if (st != ICET_OK) return st;
    // the build: icet_keyframe_device_n in the store's shape (a replayed graph for <= 8 scans included), then the copy into the slots, never captured
    st = icet_keyframe_device_n(c, &s->shape, n, scan1, d_rows);
    c->kf_pairs = 0;                                         // a put is a keyframe build on the context: its own parked keyframe is gone
    if (st != ICET_OK) { s->err = c->err; return st; }
    for (int first = 0; first < n; first += kStoreParkMax) {
        const int cnt = std::min(kStoreParkMax, n - first);
        StoreParkSlots dst{};
        for (int k = 0; k < cnt; k++) dst.slot[k] = slots[first + k];
        const hipError_t e = launch_keyframe_store_park(c->w, s->V, first, cnt, dst, s->hotS, s->fitS, s->slot_of_voxel, s->n_slots, c->stream);
        if (e != hipSuccess) {
            for (int k = first; k < n; k++) s->occupied[(size_t)slots[k]] = 0;    // (what these rows hold is unknown)
            s->err = std::string("k_keyframe_store_park: ") + hipGetErrorString(e);
            return ICET_ERR_HIP;
        }
        for (int k = 0; k < cnt; k++) s->occupied[(size_t)dst.slot[k]] = 1;
        const hipError_t pe = launch_closure_clear_pose(s->pose_table(), dst, cnt, c->stream);      // a new keyframe: whatever pose the slot had is not its pose
        if (pe != hipSuccess) { s->err = std::string("k_closure_clear_pose: ") + hipGetErrorString(pe); return ICET_ERR_HIP; }
        if (s->app) {                                            // the scans' descriptors into the same slots, behind the park
            const icet_status as = app_put_batch(s, scan1 + first, d_rows ? d_rows + first : nullptr, cnt, dst);
            if (as != ICET_OK) return as;
        }
        if (s->coarse) {                                         // and their grids
            const icet_status cs = coarse_put_batch(s, scan1 + first, d_rows ? d_rows + first : nullptr, cnt, dst);
            if (cs != ICET_OK) return cs;
        }
    }
    return ICET_OK;
}

icet_status icet_keyframe_store_register_device(icet_keyframe_store* s, const icet_params* p, int32_t n_regs, const int32_t* slot_index,
                                                const icet_dev_scan* scan2, const float* d_x0, float* d_out) {
    if (!s) return ICET_ERR_BAD_ARG;
    const icet_status st = register_indexed(s->ctx, p, n_regs, slot_index, scan2, d_x0, d_out, nullptr, kIdxRegister, s);
    if (st != ICET_OK) s->err = s->ctx->err;
    return st;
}

icet_status icet_keyframe_store_register_scored_device(icet_keyframe_store* s, const icet_params* p, int32_t n_regs, const int32_t* slot_index,
                                                       const icet_dev_scan* scan2, const float* d_x0, float* d_out, icet_score* d_score) {
    if (!s) return ICET_ERR_BAD_ARG;
    const icet_status st = register_indexed(s->ctx, p, n_regs, slot_index, scan2, d_x0, d_out, d_score, kIdxScored, s);
    if (st != ICET_OK) s->err = s->ctx->err;
    return st;
}

icet_status icet_keyframe_store_score_device(icet_keyframe_store* s, const icet_params* p, int32_t n_regs, const int32_t* slot_index,
                                             const icet_dev_scan* scan2, const float* d_X, icet_score* d_score) {
    if (!s) return ICET_ERR_BAD_ARG;
    const icet_status st = register_indexed(s->ctx, p, n_regs, slot_index, scan2, d_X, nullptr, d_score, kIdxScoreOnly, s);
    if (st != ICET_OK) s->err = s->ctx->err;
    return st;
}

// Test hook: one occupied slot's tables on the host (what: 0 n_slots, 1 SlotHot words, 2 SlotFit words, 3 slot_of_voxel int16).  Synchronises the context's stream.
icet_status icet_keyframe_store_debug_fetch(icet_keyframe_store* s, int32_t slot, int32_t what, void* out, int64_t count) {
    if (!s) return ICET_ERR_BAD_ARG;
    if (!out || count < 0 || slot < 0 || slot >= s->capacity || !s->occupied[(size_t)slot]) { s->err = "bad argument or empty slot"; return ICET_ERR_BAD_ARG; }
    icet_ctx* c = s->ctx;
    STORECHK(s, hipSetDevice(c->device));
    STORECHK(s, hipStreamSynchronize(c->stream));
    int32_t ns = 0;
    STORECHK(s, hipMemcpy(&ns, s->n_slots + slot, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (what == 4) {                                          // the pose: 12 strided floats into a row-major 4 x 4
        if (count > 16) { s->err = "count too large"; return ICET_ERR_BAD_ARG; }
        float tR[12], T[16];
        const PoseTable tab = s->pose_table();
        STORECHK(s, hipMemcpy2D(tR, sizeof(float), tab.f + slot, sizeof(float) * (size_t)tab.cap, sizeof(float), 12, hipMemcpyDeviceToHost));
        for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) T[4 * a + b] = tR[3 + 3 * a + b]; T[4 * a + 3] = tR[a]; }
        T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
        std::memcpy(out, T, sizeof(float) * (size_t)count);
        return ICET_OK;
    }
    if (what == 6 || what == 7) {                             // the slot's descriptor: D[ring][sector] bytes out of the ring-packed columns; its weights
        if (!s->app || !s->app->has_h[(size_t)slot]) { s->err = "the slot has no descriptor"; return ICET_ERR_BAD_ARG; }
        const int A = s->app->k.A, Rn = s->app->k.Rn, Rp = s->app->Rp;
        if (count > (what == 6 ? (int64_t)A * Rn : (int64_t)A)) { s->err = "count too large"; return ICET_ERR_BAD_ARG; }
        if (what == 7) { if (count > 0) STORECHK(s, hipMemcpy(out, s->app->w + (size_t)slot * A, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost)); return ICET_OK; }
        std::vector<uint32_t> words((size_t)A * Rp);
        STORECHK(s, hipMemcpy(words.data(), s->app->desc + (size_t)slot * A * Rp, sizeof(uint32_t) * words.size(), hipMemcpyDeviceToHost));
        uint8_t* o = static_cast<uint8_t*>(out);
        for (int64_t i = 0; i < count; i++) { const int r = (int)(i / A), j = (int)(i % A); o[i] = (uint8_t)(words[(size_t)j * Rp + (r >> 2)] >> (8 * (r & 3))); }
        return ICET_OK;
    }
    if (what == 8) {                                          // the slot's grid: G rows of G / 32 words
        if (!s->coarse || !s->coarse->has_h[(size_t)slot]) { s->err = "the slot has no grid"; return ICET_ERR_BAD_ARG; }
        if (count > (int64_t)s->coarse->row_words()) { s->err = "count too large"; return ICET_ERR_BAD_ARG; }
        if (count > 0) STORECHK(s, hipMemcpy(out, s->coarse->grid + (size_t)slot * s->coarse->row_words(), sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToHost));
        return ICET_OK;
    }
    const void* src = nullptr; int64_t cap = 0; size_t elem = 4;
    switch (what) {
        case 5: src = s->pose_stamp + slot; cap = 1; elem = 8; break;
        case 0: src = s->n_slots + slot; cap = 1; break;
        case 1: src = s->hotS + (size_t)slot * s->V; cap = (int64_t)ns * (int64_t)(sizeof(SlotHot) / 4); break;
        case 2: src = s->fitS + (size_t)slot * s->V; cap = (int64_t)ns * (int64_t)(sizeof(SlotFit) / 4); break;
        case 3: src = s->slot_of_voxel + (size_t)slot * ((s->V + 1) & ~1); cap = s->V; elem = 2; break;
        default: s->err = "unknown table id"; return ICET_ERR_BAD_ARG;
    }
    if (count > cap) { s->err = "count too large"; return ICET_ERR_BAD_ARG; }
    if (count > 0) STORECHK(s, hipMemcpy(out, src, (size_t)count * elem, hipMemcpyDeviceToHost));
    return ICET_OK;
}

// ---- the loop-closure query ------------------------------------------------------------------------------------
void icet_pose_step_from_x(const float X[6], float T[16]) { if (X && T) icet_closure_rule::pose_step_from_X(X, T); }

icet_status icet_keyframe_store_set_pose(icet_keyframe_store* s, int32_t n, const int32_t* slots, const float* poses, const int64_t* stamps) {
    ICET_TRY(enter(s));
    icet_ctx* c = s->ctx;
    if (n < 0 || (n > 0 && (!slots || !poses || !stamps))) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (n == 0) return ICET_OK;
    const icet_status ok = slots_ok(s, n, slots, true, "set_pose");
    if (ok != ICET_OK) return ok;
    STORECHK(s, s->pose_read.wait());                            // the previous set_pose's kernel has read the staging
    if (n > s->cap_h_pose) STORECHK(s, grow(s->pose_stage, s->cap_h_pose, n, [&] { return s->pose_stage.pinned(s->h_pose, (size_t)n); }));
    for (int k = 0; k < n; k++) {
        PoseUpload& u = s->h_pose[k];
        const float* T = poses + 16 * (size_t)k;
        u.slot = slots[k]; u.pad = 0; u.stamp = stamps[k];
        for (int a = 0; a < 3; a++) { u.tR[a] = T[4 * a + 3]; for (int b = 0; b < 3; b++) u.tR[3 + 3 * a + b] = T[4 * a + b]; }
    }
    STORECHK(s, launch_closure_set_pose(s->pose_table(), s->h_pose, n, c->stream));
    STORECHK(s, s->pose_read.mark(c->stream));
    return ICET_OK;
}

static icet_status n_queries_ok(icet_keyframe_store* s, int32_t n_queries) {
    if (n_queries < 1 || n_queries > kClosureMaxQueries) { s->err = "n_queries must be 1 .. " + std::to_string(kClosureMaxQueries); return ICET_ERR_BAD_ARG; }
    return ICET_OK;
}

// The arguments every query shares, its scans apart (scans_ok); K as the query names it.  Candidates come by pose -- poses and stamps, a radius in metres -- or by
// appearance: the radius member is the largest distance, and stamps only matter with a stamp gap.
static icet_status query_ok(icet_keyframe_store* s, bool by_pose, int32_t n_queries, const float* poses, const int64_t* stamps, const icet_closure_query* q) {
    if (!by_pose && !s->app) { s->err = "appearance is not enabled on this store"; return ICET_ERR_BAD_ARG; }
    const icet_status st = n_queries_ok(s, n_queries);
    if (st != ICET_OK) return st;
    if (!q || (by_pose && (!poses || !stamps))) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (q->max_candidates < 1 || q->max_candidates > kClosureMaxCandidates) { s->err = "max_candidates must be 1 .. " + std::to_string(kClosureMaxCandidates); return ICET_ERR_BAD_ARG; }
    if (!(q->radius >= 0.f)) { s->err = by_pose ? "radius must be a number >= 0" : "max_distance (the radius member) must be a number >= 0"; return ICET_ERR_BAD_ARG; }
    if (!by_pose && q->min_stamp_gap > 0 && !stamps) { s->err = "min_stamp_gap > 0 needs the queries' stamps"; return ICET_ERR_BAD_ARG; }
    return ICET_OK;
}

static icet_status closure_ensure(icet_keyframe_store* s, int32_t n_queries, int K, int n_regs) {
    icet_ctx* c = s->ctx;
    const size_t need_part = (size_t)n_queries * (size_t)closure_tiles(s->capacity) * (size_t)K;
    const int32_t qk = n_queries * K;
    if (need_part <= s->cap_part && qk <= s->cap_qk && n_regs <= s->cap_qr && s->q_best) return ICET_OK;
    STORECHK(s, hipStreamSynchronize(c->stream));              // no query in flight reads the buffers that move
    // (the fixed pair's capacity is its last pointer, set after the last allocation; the other three grow by grow(), icet_buffers.h)
    if (!s->q_best) { s->q_fixed.release(); STORECHK(s, s->q_fixed.device(s->q_offs, (size_t)kClosureMaxQueries + 1)); STORECHK(s, s->q_fixed.device(s->q_best, (size_t)kClosureMaxQueries)); }
    if (need_part > s->cap_part) STORECHK(s, grow(s->q_part_mem, s->cap_part, need_part, [&] { return s->q_part_mem.device(s->q_part, need_part); }));
    if (qk > s->cap_qk) { BufferGroup& g = s->q_qk_mem; STORECHK(s, grow(g, s->cap_qk, qk, [&] { const int e = g.device(s->q_keys, (size_t)qk); return e ? e : g.device(s->q_cand, (size_t)qk); })); }
    if (n_regs > s->cap_qr) {
        BufferGroup& g = s->q_qr_mem;
        const size_t r = (size_t)n_regs;
        STORECHK(s, grow(g, s->cap_qr, n_regs, [&] {
            int e = g.device(s->q_x0, r * 6);
            if (!e) e = g.device(s->q_out, r * 48);
            if (!e) e = g.device(s->q_score, r);
            if (!e) e = g.device(s->q_kf_of, r);
            if (!e) e = g.device(s->q_rows, r);
            if (!e) e = g.device(s->q_members, r);
            return e;
        }));
    }
    return ICET_OK;
}

static void copy_start_offsets(float (*off)[6], const float* start_offsets, int n_starts) {
    if (start_offsets) for (int i = 0; i < n_starts; i++) for (int k = 0; k < 6; k++) off[i][k] = start_offsets[6 * i + k];
}

// Step 1 by pose: candidates into cand, their keys into s->q_keys.
static icet_status pose_search(icet_keyframe_store* s, int32_t n_queries, const float* poses, const int64_t* stamps, const icet_closure_query* query, int32_t* cand) {
    ClosureSearchArgs qa;
    std::memset(&qa, 0, sizeof(qa));
    for (int q = 0; q < n_queries; q++) { const float* T = poses + 16 * (size_t)q; qa.tx[q] = T[3]; qa.ty[q] = T[7]; qa.tz[q] = T[11]; qa.stamp[q] = stamps[q]; }
    STORECHK(s, launch_closure_search(s->pose_table(), qa, n_queries, query->max_candidates, query->radius, query->min_stamp_gap, s->q_part, cand, s->q_keys, s->ctx->stream));
    return ICET_OK;
}

// Step 2, by pose (poses given) or by appearance: each candidate's base start -- and for the appearance calls its distance and shift -- into the buffers that are
// given and, with n_starts > 0, its registrations fl(base + off[s]) into x0 and the store's per-registration buffers.
static icet_status resolve_candidates(icet_keyframe_store* s, const float* poses, int32_t n_queries, int K, const AppOffsets& off, int n_starts, int any_slot,
                                      const int32_t* cand, float* d_dist, int32_t* d_shift, int32_t* shift_of, float* d_x0_base, float* x0) {
    const bool regs = n_starts > 0;
    int32_t* kf_of = regs ? s->q_kf_of : nullptr; int32_t* rows = regs ? s->q_rows : nullptr; int32_t* members = regs ? s->q_members : nullptr; int32_t* offs = regs ? s->q_offs : nullptr;
    if (!poses) {
        STORECHK(s, launch_app_resolve(s->capacity, s->app->k.A, off, n_queries, K, n_starts, any_slot, cand, s->q_keys, s->app->shift_all, d_dist, d_shift, d_x0_base, shift_of,
                                       x0, kf_of, rows, members, offs, s->ctx->stream));
        return ICET_OK;
    }
    ClosurePoseArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    for (int q = 0; q < n_queries; q++) {
        const float* T = poses + 16 * (size_t)q;
        for (int a = 0; a < 3; a++) { pa.t[q][a] = T[4 * a + 3]; for (int b = 0; b < 3; b++) pa.R[q][3 * a + b] = T[4 * a + b]; }
    }
    static_assert(sizeof(pa.off) == sizeof(off.off), "one table of start offsets");
    std::memcpy(pa.off, off.off, sizeof(pa.off));
    STORECHK(s, launch_closure_resolve(s->pose_table(), pa, n_queries, K, n_starts, any_slot, cand, d_x0_base, x0, kf_of, rows, members, offs, s->ctx->stream));
    return ICET_OK;
}

icet_status icet_keyframe_store_candidates_device(icet_keyframe_store* s, int32_t n_queries, const float* poses, const int64_t* stamps,
                                                  const icet_closure_query* query, int32_t* d_cand, float* d_x0_base) {
    ICET_TRY(enter(s));
    icet_status st = query_ok(s, true, n_queries, poses, stamps, query);
    if (st != ICET_OK) return st;
    if (!d_cand) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    const int K = query->max_candidates;
    st = closure_ensure(s, n_queries, K, 0);
    if (st != ICET_OK) return st;
    st = pose_search(s, n_queries, poses, stamps, query, d_cand);
    if (st == ICET_OK && d_x0_base) st = resolve_candidates(s, poses, n_queries, K, AppOffsets{}, 0, -1, d_cand, nullptr, nullptr, nullptr, d_x0_base, nullptr);
    return st;
}

// ---- loop closure by appearance ----------------------------------------------------------------------------------
static void app_scans(const icet_dev_scan* scan, int cnt, const int32_t* dst, AppScans& sc) {
    std::memset(&sc, 0, sizeof(sc));
    for (int k = 0; k < cnt; k++) { sc.ptr[k] = scan[k].ptr; sc.n[k] = (int32_t)scan[k].n; sc.ld[k] = (int32_t)scan[k].ld; sc.dst[k] = dst ? dst[k] : k; }
}

// The descriptors of the cnt <= kAppBatch scans a put has just parked, into the rows of their slots.
static icet_status app_put_batch(icet_keyframe_store* s, const icet_dev_scan* scan, const int32_t* d_rows, int cnt, const StoreParkSlots& dst) {
    icet_ctx* c = s->ctx;
    AppScans sc; app_scans(scan, cnt, dst.slot, sc);
    const AppTable tab = s->app_table();
    hipError_t e = launch_app_build(sc, cnt, d_rows, s->app->k, s->app->scratch, c->stream);
    if (e == hipSuccess) e = launch_app_finish(sc, cnt, s->app->k, s->app->scratch, &tab, nullptr, nullptr, c->stream);
    if (e != hipSuccess) {
        for (int k = 0; k < cnt; k++) s->app->has_h[(size_t)dst.slot[k]] = 0;     // (what these rows hold is unknown)
        s->err = std::string("k_app_build: ") + hipGetErrorString(e);
        return ICET_ERR_HIP;
    }
    for (int k = 0; k < cnt; k++) s->app->has_h[(size_t)dst.slot[k]] = 1;
    return ICET_OK;
}

icet_status icet_keyframe_store_enable_appearance(icet_keyframe_store* s, const icet_appearance_params* ap) {
    static_assert(sizeof(icet_appearance_params) == 32, "the record of include/icet_hip.h (the ctypes mirror of icet_amd/api.py)");
    if (!s) return ICET_ERR_BAD_ARG;
    icet_ctx* c = s->ctx;
    if (s->app) { s->err = "appearance is already enabled on this store"; return ICET_ERR_BAD_ARG; }
    icet_appearance_params d{};
    d.sectors = 120; d.rings = 20; d.rho_max = 80.f; d.z_lo = -3.f; d.z_hi = 12.f;
    if (ap) d = *ap;
    if (!icet_appearance_rule::params_ok(d.sectors, d.rings, d.rho_max, d.z_lo, d.z_hi) || d.reserved[0] || d.reserved[1] || d.reserved[2]) {
        s->err = "appearance parameters out of range (sectors even 8 .. 360, rings 1 .. 64, rho_max > 0, z_hi > z_lo, reserved words zero)"; return ICET_ERR_BAD_ARG;
    }
    STORECHK(s, hipSetDevice(c->device));
    STORECHK(s, hipStreamSynchronize(c->stream));
    auto* a = new (std::nothrow) icet_keyframe_store::Appearance();
    if (!a) { s->err = "host allocation failed"; return ICET_ERR_NOMEM; }
    a->k = icet_appearance_rule::make_consts(d.sectors, d.rings, d.rho_max, d.z_lo, d.z_hi);
    a->params = d;
    a->Rp = (d.rings + 3) / 4;
    const size_t A = (size_t)a->k.A, row = A * (size_t)a->Rp, cells = A * (size_t)a->k.Rn;
    BufferGroup& g = a->work;
    int e = app_alloc_table(a->table, row, A, s->capacity, a->desc, a->w, a->has);
    if (e == hipSuccess) e = g.device(a->scratch, cells * kAppBatch);
    if (e == hipSuccess) e = g.device(a->qdesc, row * kAppBatch);
    if (e == hipSuccess) e = g.device(a->qw, A * kAppBatch);
    if (e == hipSuccess) e = g.device(a->qhas, (size_t)kAppBatch);
    if (e == hipSuccess) e = g.device(a->shift_of, (size_t)kClosureMaxQueries * kClosureMaxCandidates);
    if (e == hipSuccess) e = hipMemsetAsync(a->has, 0, sizeof(int32_t) * (size_t)s->capacity, c->stream);          // no slot has a descriptor
    if (e == hipSuccess) e = hipMemsetAsync(a->scratch, 0, sizeof(uint32_t) * cells * kAppBatch, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); delete a; return store_fail(s, "enable_appearance", e); }
    a->has_h.assign((size_t)s->capacity, 0);
    s->app = a;
    return ICET_OK;
}

icet_status icet_keyframe_store_describe_device(icet_keyframe_store* s, int32_t n, const icet_dev_scan* scan, const int32_t* d_rows, uint8_t* d_desc, float* d_weight) {
    ICET_TRY(enter(s));
    icet_ctx* c = s->ctx;
    if (!s->app) { s->err = "appearance is not enabled on this store"; return ICET_ERR_BAD_ARG; }
    if (n < 0 || (n > 0 && (!scan || !d_desc || !d_weight))) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (scans_ok(s, n, scan) != ICET_OK) return ICET_ERR_BAD_ARG;
    if (n == 0) return ICET_OK;
    const size_t A = (size_t)s->app->k.A, cells = A * (size_t)s->app->k.Rn;
    for (int first = 0; first < n; first += kAppBatch) {
        const int cnt = std::min(kAppBatch, n - first);
        AppScans sc; app_scans(scan + first, cnt, nullptr, sc);
        STORECHK(s, launch_app_build(sc, cnt, d_rows ? d_rows + first : nullptr, s->app->k, s->app->scratch, c->stream));
        STORECHK(s, launch_app_finish(sc, cnt, s->app->k, s->app->scratch, nullptr, d_desc + cells * (size_t)first, d_weight + A * (size_t)first, c->stream));
    }
    return ICET_OK;
}

icet_status icet_keyframe_store_set_stamp(icet_keyframe_store* s, int32_t n, const int32_t* slots, const int64_t* stamps) {
    ICET_TRY(enter(s));
    icet_ctx* c = s->ctx;
    if (n < 0 || (n > 0 && (!slots || !stamps))) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (n == 0) return ICET_OK;
    const icet_status ok = slots_ok(s, n, slots, true, "set_stamp");
    if (ok != ICET_OK) return ok;
    for (int first = 0; first < n; first += kAppBatch) {
        const int cnt = std::min(kAppBatch, n - first);
        AppStamps st{};
        for (int k = 0; k < cnt; k++) { st.slot[k] = slots[first + k]; st.stamp[k] = stamps[first + k]; }
        STORECHK(s, launch_app_set_stamp(s->pose_table(), st, cnt, c->stream));
    }
    return ICET_OK;
}

static icet_status app_ensure(icet_keyframe_store* s, int32_t n_queries) {
    icet_ctx* c = s->ctx;
    const size_t need = (size_t)n_queries * (size_t)s->capacity;
    if (need <= s->app->cap_all) return ICET_OK;
    STORECHK(s, hipStreamSynchronize(c->stream));              // no query in flight reads the buffers that move
    BufferGroup& g = s->app->all;
    STORECHK(s, grow(g, s->app->cap_all, need, [&] { const int e = g.device(s->app->keys_all, need); return e ? e : g.device(s->app->shift_all, need); }));
    return ICET_OK;
}

// The queries' descriptors and the search: candidates into cand, their keys into s->q_keys.
static icet_status app_search(icet_keyframe_store* s, int32_t n_queries, const icet_dev_scan* scan2, const int64_t* stamps, const icet_closure_query* query, int32_t* cand) {
    icet_ctx* c = s->ctx;
    AppScans sc; app_scans(scan2, n_queries, nullptr, sc);
    const AppTable qtab{s->app->qdesc, s->app->qw, s->app->qhas, kAppBatch, s->app->k.A, s->app->Rp};
    AppQueryStamps qs{};
    if (stamps) for (int q = 0; q < n_queries; q++) qs.stamp[q] = stamps[q];
    STORECHK(s, launch_app_build(sc, n_queries, nullptr, s->app->k, s->app->scratch, c->stream));
    STORECHK(s, launch_app_finish(sc, n_queries, s->app->k, s->app->scratch, &qtab, nullptr, nullptr, c->stream));
    STORECHK(s, launch_app_search(s->app_table(), s->pose_table(), s->app->qdesc, s->app->qw, qs, n_queries, query->max_candidates, query->radius, query->min_stamp_gap,
                                  s->app->keys_all, s->app->shift_all, s->q_part, cand, s->q_keys, c->stream));
    return ICET_OK;
}

icet_status icet_keyframe_store_candidates_appearance_device(icet_keyframe_store* s, int32_t n_queries, const icet_dev_scan* scan2, const int64_t* stamps,
                                                             const icet_closure_query* query, int32_t* d_cand, float* d_dist, int32_t* d_shift, float* d_x0_base) {
    ICET_TRY(enter(s));
    icet_status st = query_ok(s, false, n_queries, nullptr, stamps, query);
    if (st == ICET_OK) st = scans_ok(s, n_queries, scan2);
    if (st != ICET_OK) return st;
    if (!d_cand) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    const int K = query->max_candidates;
    st = closure_ensure(s, n_queries, K, 0);
    if (st == ICET_OK) st = app_ensure(s, n_queries);
    if (st != ICET_OK) return st;
    st = app_search(s, n_queries, scan2, stamps, query, d_cand);
    if (st == ICET_OK && (d_dist || d_shift || d_x0_base)) st = resolve_candidates(s, nullptr, n_queries, K, AppOffsets{}, 0, -1, d_cand, d_dist, d_shift, nullptr, d_x0_base, nullptr);
    return st;
}

// ---- coarse alignment -------------------------------------------------------------------------------------------
// The grids of the cnt <= kStoreParkMax scans a put has just parked, into the rows of their slots.
static icet_status coarse_put_batch(icet_keyframe_store* s, const icet_dev_scan* scan, const int32_t* d_rows, int cnt, const StoreParkSlots& dst) {
    icet_ctx* c = s->ctx;
    const CoarseTable tab = s->coarse_table();
    for (int first = 0; first < cnt; first += kCoarseBatch) {
        const int m = std::min(kCoarseBatch, cnt - first);
        AppScans sc; app_scans(scan + first, m, dst.slot + first, sc);
        const hipError_t e = launch_coarse_structure(sc, m, d_rows ? d_rows + first : nullptr, s->coarse->k, s->coarse->scratch, tab.grid, tab.has, tab.cap, c->stream);
        if (e != hipSuccess) {
            for (int k = first; k < cnt; k++) s->coarse->has_h[(size_t)dst.slot[k]] = 0;      // (what these rows hold is unknown)
            s->err = std::string("k_coarse_extrema: ") + hipGetErrorString(e);
            return ICET_ERR_HIP;
        }
        for (int k = 0; k < m; k++) s->coarse->has_h[(size_t)dst.slot[first + k]] = 1;
    }
    return ICET_OK;
}

icet_status icet_keyframe_store_enable_coarse(icet_keyframe_store* s, const icet_coarse_params* cp) {
    static_assert(sizeof(icet_coarse_params) == 32 && sizeof(icet_coarse_search) == 32 && sizeof(icet_coarse_match) == 32, "the records of include/icet_hip.h (the ctypes mirrors of icet_amd/api.py)");
    if (!s) return ICET_ERR_BAD_ARG;
    icet_ctx* c = s->ctx;
    if (s->coarse) { s->err = "coarse alignment is already enabled on this store"; return ICET_ERR_BAD_ARG; }
    icet_coarse_params d{};
    d.cells = 256; d.cell = 0.25f; d.z_lo = -3.f; d.z_hi = 12.f; d.min_span = 0.5f;
    if (cp) d = *cp;
    if (!icet_coarse_rule::params_ok(d.cells, d.cell, d.z_lo, d.z_hi, d.min_span) || d.reserved[0] || d.reserved[1] || d.reserved[2]) {
        s->err = "coarse parameters out of range (cells a multiple of 32, 64 .. 512, cell > 0, z_hi > z_lo, min_span > 0, reserved words zero)"; return ICET_ERR_BAD_ARG;
    }
    STORECHK(s, hipSetDevice(c->device));
    STORECHK(s, hipStreamSynchronize(c->stream));
    auto* a = new (std::nothrow) icet_keyframe_store::Coarse();
    if (!a) { s->err = "host allocation failed"; return ICET_ERR_NOMEM; }
    a->k = icet_coarse_rule::make_consts(d.cells, d.cell, d.z_lo, d.z_hi, d.min_span);
    a->params = d;
    const size_t row = a->row_words(), cells = (size_t)a->k.G * (size_t)a->k.G;
    constexpr size_t kQK = (size_t)kClosureMaxQueries * kClosureMaxCandidates, kH = 2 * (2 * icet_coarse_rule::kMaxYaw + 1);
    BufferGroup& g = a->work;
    int e = launch_coarse_prepare(a->k);
    if (e == hipSuccess) e = coarse_alloc_table(a->table, row, s->capacity, a->grid, a->has);
    if (e == hipSuccess) e = g.device(a->scratch, 2 * cells * kCoarseBatch);
    if (e == hipSuccess) e = g.device(a->qgrid, row * kAppBatch);
    if (e == hipSuccess) e = g.device(a->base, 6 * kQK);
    if (e == hipSuccess) e = g.device(a->match, kQK);
    if (e == hipSuccess) e = g.device(a->keys, kQK);
    if (e == hipSuccess) e = g.device(a->key_bits, kQK);
    if (e == hipSuccess) e = g.device(a->hyp, kQK * kH);
    if (e == hipSuccess) e = g.device(a->live_bits, kQK * kH);
    if (e == hipSuccess) e = hipMemsetAsync(a->has, 0, sizeof(int32_t) * (size_t)s->capacity, c->stream);          // no slot has a grid
    if (e == hipSuccess) e = hipMemsetAsync(a->scratch, 0, sizeof(uint32_t) * 2 * cells * kCoarseBatch, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); delete a; return store_fail(s, "enable_coarse", e); }
    a->has_h.assign((size_t)s->capacity, 0);
    s->coarse = a;
    return ICET_OK;
}

icet_status icet_keyframe_store_coarse_grid_device(icet_keyframe_store* s, int32_t n, const icet_dev_scan* scan, const int32_t* d_rows, uint32_t* d_grid) {
    ICET_TRY(enter(s));
    icet_ctx* c = s->ctx;
    if (!s->coarse) { s->err = "coarse alignment is not enabled on this store"; return ICET_ERR_BAD_ARG; }
    if (n < 0 || (n > 0 && (!scan || !d_grid))) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (scans_ok(s, n, scan) != ICET_OK) return ICET_ERR_BAD_ARG;
    if (n == 0) return ICET_OK;
    for (int first = 0; first < n; first += kCoarseBatch) {
        const int cnt = std::min(kCoarseBatch, n - first);
        AppScans sc; app_scans(scan + first, cnt, nullptr, sc);
        STORECHK(s, launch_coarse_structure(sc, cnt, d_rows ? d_rows + first : nullptr, s->coarse->k, s->coarse->scratch, d_grid + s->coarse->row_words() * (size_t)first,
                                            nullptr, cnt, c->stream));
    }
    return ICET_OK;
}

static icet_status coarse_search_ok(icet_keyframe_store* s, const icet_coarse_search* se) {
    if (!s->coarse) { s->err = "coarse alignment is not enabled on this store"; return ICET_ERR_BAD_ARG; }
    if (!se) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (se->window < 0 || se->window > icet_coarse_rule::kMaxWindow) { s->err = "window must be 0 .. 32"; return ICET_ERR_BAD_ARG; }
    if (se->n_yaw < 0 || se->n_yaw > icet_coarse_rule::kMaxYaw) { s->err = "n_yaw must be 0 .. 8"; return ICET_ERR_BAD_ARG; }
    if (!std::isfinite(se->yaw_step)) { s->err = "yaw_step must be finite"; return ICET_ERR_BAD_ARG; }
    if (se->half_turn != 0 && se->half_turn != 1) { s->err = "half_turn must be 0 or 1"; return ICET_ERR_BAD_ARG; }
    if (se->min_score < 1) { s->err = "min_score must be >= 1"; return ICET_ERR_BAD_ARG; }
    if (se->reserved[0] || se->reserved[1] || se->reserved[2]) { s->err = "reserved words must be zero"; return ICET_ERR_BAD_ARG; }
    return ICET_OK;
}

// The queries' own grids, then the search of their candidates (d_cand, d_x0_base on the device).
static icet_status coarse_run(icet_keyframe_store* s, int32_t n_queries, const icet_dev_scan* scan2, const int32_t* d_rows, int K, const icet_coarse_search* se,
                              const AppOffsets& off, int n_starts, int any_slot, const int32_t* d_cand, const float* d_x0_base, float* d_x0_out, icet_coarse_match* d_match,
                              float* d_x0) {
    icet_ctx* c = s->ctx;
    icet_keyframe_store::Coarse* a = s->coarse;
    for (int first = 0; first < n_queries; first += kCoarseBatch) {
        const int cnt = std::min(kCoarseBatch, n_queries - first);
        AppScans sc; app_scans(scan2 + first, cnt, nullptr, sc);
        STORECHK(s, launch_coarse_structure(sc, cnt, d_rows ? d_rows + first : nullptr, a->k, a->scratch, a->qgrid + a->row_words() * (size_t)first, nullptr, cnt, c->stream));
    }
    AppScans all; app_scans(scan2, n_queries, nullptr, all);
    const CoarseSearch cs{se->window, se->n_yaw, se->half_turn, se->min_score, se->yaw_step};
    STORECHK(s, launch_coarse_align(s->coarse_table(), all, d_rows, a->k, cs, off, n_queries, K, n_starts, any_slot, d_cand, d_x0_base, a->qgrid, a->hyp, a->keys,
                                    a->live_bits, a->key_bits, d_x0_out, d_match, d_x0, s->q_kf_of, s->q_rows, s->q_members, n_starts > 0 ? s->q_offs : nullptr, c->stream));
    return ICET_OK;
}

icet_status icet_keyframe_store_coarse_align_device(icet_keyframe_store* s, int32_t n_queries, const icet_dev_scan* scan2, const int32_t* d_rows, int32_t K,
                                                    const int32_t* d_cand, const float* d_x0_base, const icet_coarse_search* search, float* d_x0_out,
                                                    icet_coarse_match* d_match) {
    ICET_TRY(enter(s));
    icet_status st = coarse_search_ok(s, search);
    if (st == ICET_OK) st = n_queries_ok(s, n_queries);
    if (st != ICET_OK) return st;
    if (K < 1 || K > kClosureMaxCandidates) { s->err = "K must be 1 .. " + std::to_string(kClosureMaxCandidates); return ICET_ERR_BAD_ARG; }
    if (!scan2 || !d_cand || !d_x0_base) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (scans_ok(s, n_queries, scan2) != ICET_OK) return ICET_ERR_BAD_ARG;
    const AppOffsets off{};
    return coarse_run(s, n_queries, scan2, d_rows, K, search, off, 0, -1, d_cand, d_x0_base, d_x0_out, d_match, nullptr);
}

// ---- the closure pipeline behind the three query calls (DESIGN.md sections 16 - 18) ---------------------------------------------------------------------
// Candidates by pose (by_pose: poses and stamps given) or by appearance; with `search` the coarse alignment of every candidate's base start sits between the
// candidates and the starts.  A query is never captured into a graph: its search kernels take this call's poses and scans as arguments.
static icet_status close_pipeline(icet_keyframe_store* s, const icet_params* p, int32_t n_queries, const icet_dev_scan* scan2, bool by_pose, const float* poses,
                                  const int64_t* stamps, const icet_closure_query* query, const icet_coarse_search* search, const float* start_offsets,
                                  icet_closure* d_closure, int32_t* d_cand, float* d_x0, float* d_out, icet_score* d_score, icet_coarse_match* d_match) {
    static_assert(sizeof(icet_closure) == 288 && sizeof(icet_closure) % 16 == 0 && sizeof(icet_closure_query) == 32, "the records of the query (include/icet_hip.h; the ctypes mirrors of icet_amd/api.py)");
    icet_ctx* c = s->ctx;
    // everything is checked before anything is touched
    icet_status st = search ? coarse_search_ok(s, search) : ICET_OK;
    if (st == ICET_OK) st = query_ok(s, by_pose, n_queries, poses, stamps, query);
    if (st == ICET_OK) st = scans_ok(s, n_queries, scan2);
    if (st != ICET_OK) return st;
    if (!params_ok(p) || !d_closure) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    if (query->n_starts < 1 || query->n_starts > kClosureMaxStarts) { s->err = "n_starts must be 1 .. " + std::to_string(kClosureMaxStarts); return ICET_ERR_BAD_ARG; }
    if (!same_keyframe_shape(s->shape, *p)) { s->err = "the grid, n, thresh, buff or keyframe-shaping flags differ from the keyframe store's shape"; return ICET_ERR_BAD_ARG; }
    if (c->tune.keep != 0) { s->err = "indexed registrations run the plain point pass: option \"keep\" must be 0"; return ICET_ERR_UNSUPPORTED; }
    const int K = query->max_candidates, S = query->n_starts, R = n_queries * K * S;
    st = closure_ensure(s, n_queries, K, R);
    if (st == ICET_OK && !by_pose) st = app_ensure(s, n_queries);
    if (st != ICET_OK) return st;
    int32_t any = -1;                                           // an occupied slot, for the padding registrations to name
    for (int32_t j = 0; j < s->capacity && any < 0; j++) if (s->occupied[(size_t)j]) any = j;
    const int any_slot = any < 0 ? 0 : any;
    AppOffsets off{};
    copy_start_offsets(off.off, start_offsets, S);
    int32_t* cand = d_cand ? d_cand : s->q_cand;
    float* x0 = d_x0 ? d_x0 : s->q_x0;
    float* out = d_out ? d_out : s->q_out;
    icet_score* score = d_score ? d_score : s->q_score;
    icet_coarse_match* match = d_match || !search ? d_match : s->coarse->match;
    int32_t* shift_of = by_pose ? nullptr : s->app->shift_of;      // the candidates' shifts, for the record of a query by appearance
    // 1 search
    st = by_pose ? pose_search(s, n_queries, poses, stamps, query, cand) : app_search(s, n_queries, scan2, stamps, query, cand);
    if (st != ICET_OK) return st;
    // 2 resolve: the candidates' starts and registrations -- with the coarse stage their base starts, which it moves and turns into the registrations itself
    if (!search) st = resolve_candidates(s, poses, n_queries, K, off, S, any_slot, cand, nullptr, nullptr, shift_of, nullptr, x0);
    else {
        st = resolve_candidates(s, poses, n_queries, K, AppOffsets{}, 0, -1, cand, nullptr, nullptr, shift_of, s->coarse->base, nullptr);
        if (st == ICET_OK) st = coarse_run(s, n_queries, scan2, nullptr, K, search, off, S, any_slot, cand, s->coarse->base, nullptr, match, x0);
    }
    if (st != ICET_OK) return st;
    const int32_t* best = nullptr;
    if (any < 0) {                                              // nothing to register against: every query ends without a winner
        if (d_out) STORECHK(s, hipMemsetAsync(d_out, 0, sizeof(float) * 48 * (size_t)R, c->stream));
        if (d_score) STORECHK(s, hipMemsetAsync(d_score, 0, sizeof(icet_score) * (size_t)R, c->stream));
    } else {
        // 3 the indexed loop in scored mode
        std::vector<int32_t> idx((size_t)R, any);
        std::vector<icet_dev_scan> regs((size_t)R);
        for (int r = 0; r < R; r++) regs[(size_t)r] = scan2[r / (K * S)];
        const IndexedDev dev{s->q_kf_of, s->q_rows};
        st = register_indexed(c, p, R, idx.data(), regs.data(), x0, out, score, kIdxScored, s, &dev);
        if (st != ICET_OK) { s->err = c->err; return st; }
        // 4 the best of each query
        STORECHK(s, launch_select_best(s->q_members, s->q_offs, n_queries, score, out, s->q_best, nullptr, c->stream));
        best = s->q_best;
    }
    // 5 the records
    STORECHK(s, launch_closure_record(s->pose_table(), n_queries, K, S, query->max_chi2_per_voxel, query->min_voxels, best, cand, s->q_keys, shift_of, x0, out, score, d_closure,
                                      c->stream));
    if (search) STORECHK(s, launch_coarse_record(n_queries, S, match, d_closure, c->stream));
    return ICET_OK;
}

icet_status icet_keyframe_store_close_device(icet_keyframe_store* s, const icet_params* p, int32_t n_queries, const icet_dev_scan* scan2,
                                             const float* poses, const int64_t* stamps, const icet_closure_query* query, const float* start_offsets,
                                             icet_closure* d_closure, int32_t* d_cand, float* d_x0, float* d_out, icet_score* d_score) {
    ICET_TRY(enter(s));
    return close_pipeline(s, p, n_queries, scan2, true, poses, stamps, query, nullptr, start_offsets, d_closure, d_cand, d_x0, d_out, d_score, nullptr);
}

icet_status icet_keyframe_store_close_appearance_device(icet_keyframe_store* s, const icet_params* p, int32_t n_queries, const icet_dev_scan* scan2,
                                                        const int64_t* stamps, const icet_closure_query* query, const float* start_offsets,
                                                        icet_closure* d_closure, int32_t* d_cand, float* d_x0, float* d_out, icet_score* d_score) {
    ICET_TRY(enter(s));
    return close_pipeline(s, p, n_queries, scan2, false, nullptr, stamps, query, nullptr, start_offsets, d_closure, d_cand, d_x0, d_out, d_score, nullptr);
}

icet_status icet_keyframe_store_close_coarse_device(icet_keyframe_store* s, const icet_params* p, int32_t n_queries, const icet_dev_scan* scan2,
                                                    const float* poses, const int64_t* stamps, const icet_closure_query* query,
                                                    const icet_coarse_search* search, const float* start_offsets, icet_closure* d_closure, int32_t* d_cand,
                                                    float* d_x0, float* d_out, icet_score* d_score, icet_coarse_match* d_match) {
    ICET_TRY(enter(s));
    if (!search) return coarse_search_ok(s, search);          // (refused: the coarse call needs its search)
    return close_pipeline(s, p, n_queries, scan2, poses != nullptr, poses, stamps, query, search, start_offsets, d_closure, d_cand, d_x0, d_out, d_score, d_match);
}

// ---- snapshots: a store to a file and back (the format and its validation: icet_snapshot.h) ------------------------------------------
namespace snap = icet_snapshot;

// What a save or a load holds while it runs: the entries (pinned and on the device), the payload checksums, one device staging and two pinned buffers that a
// chunk's copy and the file I/O of the chunk before it alternate between.
struct SnapBuffers {
    SnapEntry* h_ent = nullptr; SnapEntry* d_ent = nullptr; unsigned long long* d_sums = nullptr; unsigned long long* h_sums = nullptr;
    uint8_t* d_stage = nullptr; uint8_t* h_buf[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr};
    BufferGroup mem;                                         // owns the seven buffers
};
static void snap_free(icet_keyframe_store* s, SnapBuffers& b) {
    (void)hipStreamSynchronize(s->ctx->stream);              // (nothing in flight reads or writes what goes)
    b.mem.release();
    for (hipEvent_t& e : b.ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
}
static hipError_t snap_alloc(SnapBuffers& b, size_t n_entries, size_t chunk_bytes, bool sums) {
    const size_t ne = n_entries ? n_entries : 1, cb = chunk_bytes ? chunk_bytes : 16;
    int e = b.mem.pinned(b.h_ent, ne);
    if (e == hipSuccess) e = b.mem.device(b.d_ent, ne);
    if (e == hipSuccess && sums) e = b.mem.device(b.d_sums, ne);
    if (e == hipSuccess && sums) e = b.mem.pinned(b.h_sums, ne);
    if (e == hipSuccess) e = b.mem.device(b.d_stage, cb);
    for (int k = 0; k < 2; k++) {
        if (e == hipSuccess) e = b.mem.pinned(b.h_buf[k], cb);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b.ev[k], hipEventDisableTiming);
    }
    if (e != hipSuccess) (void)hipGetLastError();
    return static_cast<hipError_t>(e);
}

// Entries first .. into chunks of at most `budget` payload bytes, never splitting one: chunk k holds entries cut[k] .. cut[k + 1] - 1.
static std::vector<size_t> snap_chunks(const std::vector<snap::Entry>& ent, uint64_t budget) {
    std::vector<size_t> cut{0};
    uint64_t in = 0;
    for (size_t k = 0; k < ent.size(); k++) {
        if (in > 0 && in + ent[k].bytes > budget) { cut.push_back(k); in = 0; }
        in += ent[k].bytes;
    }
    if (!ent.empty()) cut.push_back(ent.size());
    return cut;
}

static void snap_header_of(const icet_keyframe_store* s, snap::Header& h) {
    static_assert(sizeof(icet_appearance_params) == sizeof(h.app) && sizeof(icet_coarse_params) == sizeof(h.coarse), "the feature blocks of a snapshot's header");
    std::memset(&h, 0, sizeof(h));
    h.bins_phi = s->shape.bins_phi; h.bins_theta = s->shape.bins_theta; h.n = s->shape.n;
    std::memcpy(&h.thresh_bits, &s->shape.thresh, 4); std::memcpy(&h.buff_bits, &s->shape.buff, 4);
    h.shape_flags = (uint32_t)s->shape.flags & snap::kShapeFlags; h.V = s->V;
    if (s->app) { h.features |= snap::kHasAppearance; std::memcpy(h.app, &s->app->params, sizeof(h.app)); }
    if (s->coarse) { h.features |= snap::kHasCoarse; std::memcpy(h.coarse, &s->coarse->params, sizeof(h.coarse)); }
}

// The store's tables as the snapshot kernels take them; A, Rp, G size the payloads (a load: the file's).
static SnapTables snap_tables(const icet_keyframe_store* s, int A, int Rp, int G) {
    const PoseTable pt = s->pose_table();
    SnapTables t{};
    t.hot = s->hotS; t.fit = s->fitS; t.sov = s->slot_of_voxel; t.n_slots = s->n_slots;
    if (s->app) { t.desc = s->app->desc; t.w = s->app->w; t.app_has = s->app->has; }
    if (s->coarse) { t.grid = s->coarse->grid; t.grid_has = s->coarse->has; }
    t.stamp = pt.stamp; t.pose = pt.f; t.cap = s->capacity; t.V = s->V; t.A = A; t.Rp = Rp; t.G = G;
    return t;
}

static uint64_t snap_budget(const icet_ctx* c, const std::vector<snap::Entry>& ent) {
    uint64_t budget = c->snapshot_chunk_bytes > 0 ? (uint64_t)c->snapshot_chunk_bytes : (uint64_t)64 << 20, total = 0;
    for (const snap::Entry& e : ent) { budget = std::max(budget, e.bytes); total += e.bytes; }      // entries never split: at least the largest
    return std::min(budget, std::max<uint64_t>(total, 16));
}

static void snap_dev_entry(SnapEntry& d, const snap::Entry& e, int32_t slot, uint64_t off) {
    std::memset(&d, 0, sizeof(d));
    d.slot = slot; d.n_slots = e.n_slots; d.flags = e.flags; d.stamp = e.stamp; d.off = off;
    std::memcpy(d.pose, e.pose, sizeof(d.pose));
}

icet_status icet_keyframe_store_save(icet_keyframe_store* s, const char* path, int32_t n, const int32_t* slots) {
    ICET_TRY(enter(s));
    icet_ctx* c = s->ctx;
    if (!path || (slots && n < 0)) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    // everything is checked before anything is touched
    std::vector<int32_t> which;
    if (slots) {
        const icet_status ok = slots_ok(s, n, slots, true, "save");
        if (ok != ICET_OK) return ok;
        which.assign(slots, slots + n);
        std::sort(which.begin(), which.end());
    } else {
        for (int32_t j = 0; j < s->capacity; j++) if (s->occupied[(size_t)j]) which.push_back(j);
    }
    if (c->tune.keep != 0) { s->err = "the store's calls run with option \"keep\" 0"; return ICET_ERR_UNSUPPORTED; }
    STORECHK(s, hipStreamSynchronize(c->stream));              // behind whatever was enqueued: the puts and poses this save is to hold
    const size_t cap = (size_t)s->capacity, ne = which.size();
    std::vector<int32_t> ns(cap);
    std::vector<uint8_t> poses(kPoseBytes * cap);
    STORECHK(s, hipMemcpy(ns.data(), s->n_slots, sizeof(int32_t) * cap, hipMemcpyDeviceToHost));
    STORECHK(s, hipMemcpy(poses.data(), s->pose_stamp, kPoseBytes * cap, hipMemcpyDeviceToHost));
    // the directory, laid out on the host
    snap::Header h;
    snap_header_of(s, h);
    h.n_entries = (uint32_t)ne;
    std::vector<snap::Entry> ent(ne);
    uint64_t at = snap::directory_end(h.n_entries);
    for (size_t k = 0; k < ne; k++) {
        snap::Entry& e = ent[k];
        const size_t sl = (size_t)which[k];
        e.slot = which[k]; e.n_slots = ns[sl];
        if (e.n_slots < 0 || e.n_slots > s->V) { s->err = "slot " + std::to_string(which[k]) + " holds a row count outside 0 .. V"; return ICET_ERR_HIP; }
        std::memcpy(&e.stamp, poses.data() + sizeof(int64_t) * sl, sizeof(int64_t));
        bool ff = true;
        for (size_t j = 0; j < 12; j++) { std::memcpy(&e.pose[j], poses.data() + sizeof(int64_t) * cap + sizeof(float) * (j * cap + sl), 4); ff = ff && e.pose[j] == 0xFFFFFFFFu; }
        e.flags = (ff ? 0u : snap::kFlagPose) | (s->app && s->app->has_h[sl] ? snap::kFlagDesc : 0u) | (s->coarse && s->coarse->has_h[sl] ? snap::kFlagGrid : 0u);
        e.off = at; e.bytes = snap::layout(s->V, e.n_slots, e.flags, h.A(), h.Rp(), h.G()).size; e.sum = 0;
        at += e.bytes;
    }
    h.file_bytes = at;
    const uint64_t budget = snap_budget(c, ent);
    const std::vector<size_t> cut = snap_chunks(ent, budget);
    snap::Writer w;
    std::vector<uint8_t> front((size_t)snap::directory_end(h.n_entries), 0);
    if (!snap::writer_open(w, path, s->err)) return ICET_ERR_BAD_ARG;
    if (!snap::writer_write(w, front.data(), front.size(), s->err)) { snap::writer_abort(w); return ICET_ERR_BAD_ARG; }      // (its place; written again when the checksums are known)
    SnapBuffers b;
    hipError_t he = snap_alloc(b, ne, (size_t)budget, true);
    bool io_ok = true;
    if (he == hipSuccess && ne > 0) {
        for (size_t k = 0; k + 1 < cut.size(); k++) for (size_t i = cut[k]; i < cut[k + 1]; i++) snap_dev_entry(b.h_ent[i], ent[i], ent[i].slot, ent[i].off - ent[cut[k]].off);
        he = hipMemcpyAsync(b.d_ent, b.h_ent, sizeof(SnapEntry) * ne, hipMemcpyHostToDevice, c->stream);
        if (he == hipSuccess) he = hipMemsetAsync(b.d_sums, 0, sizeof(unsigned long long) * ne, c->stream);
        const SnapTables t = snap_tables(s, h.A(), h.Rp(), h.G());
        auto chunk_bytes = [&](size_t k) { return (size_t)(ent[cut[k + 1] - 1].off + ent[cut[k + 1] - 1].bytes - ent[cut[k]].off); };
        // chunk k: pack -> copy into pinned buffer k & 1; chunk k - 1 goes to the file meanwhile
        for (size_t k = 0; k + 1 < cut.size() && he == hipSuccess && io_ok; k++) {
            he = launch_snapshot_pack(t, b.d_ent + cut[k], (int)(cut[k + 1] - cut[k]), b.d_stage, b.d_sums + cut[k], c->stream);
            if (he == hipSuccess) he = hipMemcpyAsync(b.h_buf[k & 1], b.d_stage, chunk_bytes(k), hipMemcpyDeviceToHost, c->stream);
            if (he == hipSuccess) he = hipEventRecord(b.ev[k & 1], c->stream);
            if (he == hipSuccess && k > 0) {
                he = hipEventSynchronize(b.ev[(k - 1) & 1]);
                if (he == hipSuccess) io_ok = snap::writer_write(w, b.h_buf[(k - 1) & 1], chunk_bytes(k - 1), s->err);
            }
        }
        if (he == hipSuccess && io_ok) {
            const size_t last = cut.size() - 2;
            he = hipMemcpyAsync(b.h_sums, b.d_sums, sizeof(unsigned long long) * ne, hipMemcpyDeviceToHost, c->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
            if (he == hipSuccess) io_ok = snap::writer_write(w, b.h_buf[last & 1], chunk_bytes(last), s->err);
        }
    }
    if (he == hipSuccess && io_ok) {
        for (size_t k = 0; k < ne; k++) ent[k].sum = b.h_sums[k];
        snap::put_header(front.data(), h, kSlotLayoutVersion);
        for (size_t k = 0; k < ne; k++) snap::put_entry(front.data() + snap::kHeaderBytes + (size_t)snap::kEntryBytes * k, ent[k]);
        snap::seal(front.data(), h.n_entries);
        io_ok = snap::writer_rewind(w, s->err) && snap::writer_write(w, front.data(), front.size(), s->err) && snap::writer_commit(w, s->err);
    }
    if (he != hipSuccess) s->err = std::string("keyframe store save: ") + hipGetErrorString(he);
    if (he != hipSuccess || !io_ok) snap::writer_abort(w);
    snap_free(s, b);
    return he != hipSuccess ? (he == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP) : (io_ok ? ICET_OK : ICET_ERR_BAD_ARG);
}

icet_status icet_keyframe_store_load(icet_keyframe_store* s, const char* path, int32_t slot_offset) {
    ICET_TRY(enter(s));
    icet_ctx* c = s->ctx;
    if (!path) { s->err = "bad argument"; return ICET_ERR_BAD_ARG; }
    // the file, read and validated on the host, then held against the store: everything is checked before anything is touched
    std::vector<uint8_t> img; snap::Header h; std::vector<snap::Entry> ent;
    if (!snap::read_file(path, kSlotLayoutVersion, img, h, ent, s->err, nullptr)) return ICET_ERR_BAD_ARG;
    snap::Header mine;
    snap_header_of(s, mine);
    if (h.bins_phi != mine.bins_phi || h.bins_theta != mine.bins_theta || h.n != mine.n || h.thresh_bits != mine.thresh_bits || h.buff_bits != mine.buff_bits ||
        h.shape_flags != mine.shape_flags) { s->err = "the grid, n, thresh, buff or keyframe-shaping flags of the file differ from the keyframe store's shape"; return ICET_ERR_BAD_ARG; }
    for (const snap::Entry& e : ent) {
        const int64_t target = (int64_t)e.slot + (int64_t)slot_offset;
        if (target < 0 || target >= s->capacity) {
            s->err = "slot " + std::to_string(e.slot) + " + slot_offset " + std::to_string(slot_offset) + " is not a slot (0 .. " + std::to_string(s->capacity - 1) + "): reserve first";
            return ICET_ERR_BAD_ARG;
        }
    }
    if ((h.features & snap::kHasAppearance) && s->app && std::memcmp(h.app, mine.app, sizeof(h.app)) != 0) { s->err = "the file's appearance parameters differ from the store's"; return ICET_ERR_BAD_ARG; }
    if ((h.features & snap::kHasCoarse) && s->coarse && std::memcmp(h.coarse, mine.coarse, sizeof(h.coarse)) != 0) { s->err = "the file's coarse parameters differ from the store's"; return ICET_ERR_BAD_ARG; }
    if (c->tune.keep != 0) { s->err = "the store's calls run with option \"keep\" 0"; return ICET_ERR_UNSUPPORTED; }
    const size_t ne = ent.size();
    if (ne == 0) return ICET_OK;
    const uint64_t budget = snap_budget(c, ent);
    const std::vector<size_t> cut = snap_chunks(ent, budget);
    SnapBuffers b;
    hipError_t he = snap_alloc(b, ne, (size_t)budget, false);
    if (he == hipSuccess) {
        for (size_t k = 0; k + 1 < cut.size(); k++) for (size_t i = cut[k]; i < cut[k + 1]; i++) snap_dev_entry(b.h_ent[i], ent[i], ent[i].slot + slot_offset, ent[i].off - ent[cut[k]].off);
        he = hipMemcpyAsync(b.d_ent, b.h_ent, sizeof(SnapEntry) * ne, hipMemcpyHostToDevice, c->stream);
        const SnapTables t = snap_tables(s, h.A(), h.Rp(), h.G());
        // chunk k: the file's bytes into pinned buffer k & 1 (once the copy of chunk k - 2 has left it) -> copy -> unpack
        for (size_t k = 0; k + 1 < cut.size() && he == hipSuccess; k++) {
            const size_t bytes = (size_t)(ent[cut[k + 1] - 1].off + ent[cut[k + 1] - 1].bytes - ent[cut[k]].off);
            if (k >= 2) he = hipEventSynchronize(b.ev[k & 1]);
            if (he != hipSuccess) break;
            std::memcpy(b.h_buf[k & 1], img.data() + ent[cut[k]].off, bytes);
            he = hipMemcpyAsync(b.d_stage, b.h_buf[k & 1], bytes, hipMemcpyHostToDevice, c->stream);
            if (he == hipSuccess) he = hipEventRecord(b.ev[k & 1], c->stream);
            if (he == hipSuccess) he = launch_snapshot_unpack(t, b.d_ent + cut[k], (int)(cut[k + 1] - cut[k]), b.d_stage, c->stream);
        }
        if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    }
    // the host mirrors follow (after a failure what the target rows hold is unknown: they count as empty)
    for (const snap::Entry& e : ent) {
        const size_t sl = (size_t)(e.slot + slot_offset);
        s->occupied[sl] = he == hipSuccess;
        if (s->app) s->app->has_h[sl] = he == hipSuccess && (e.flags & snap::kFlagDesc);
        if (s->coarse) s->coarse->has_h[sl] = he == hipSuccess && (e.flags & snap::kFlagGrid);
    }
    if (he != hipSuccess) s->err = std::string("keyframe store load: ") + hipGetErrorString(he);
    snap_free(s, b);
    return he == hipSuccess ? ICET_OK : (he == hipErrorOutOfMemory ? ICET_ERR_NOMEM : ICET_ERR_HIP);
}

icet_status icet_keyframe_store_snapshot_info(const char* path, icet_snapshot_info* info) {
    static_assert(sizeof(icet_snapshot_info) == 120, "the record of include/icet_hip.h (the ctypes mirror of icet_amd/api.py)");
    if (!path || !info) return ICET_ERR_BAD_ARG;
    std::vector<uint8_t> img; snap::Header h; std::vector<snap::Entry> ent; std::string err;
    if (!snap::read_file(path, kSlotLayoutVersion, img, h, ent, err, nullptr)) return ICET_ERR_BAD_ARG;
    std::memset(info, 0, sizeof(*info));
    info->shape.bins_phi = h.bins_phi; info->shape.bins_theta = h.bins_theta; info->shape.n = h.n;
    std::memcpy(&info->shape.thresh, &h.thresh_bits, 4); std::memcpy(&info->shape.buff, &h.buff_bits, 4);
    info->shape.flags = (int32_t)h.shape_flags;
    info->V = h.V; info->entries = (int32_t)h.n_entries; info->highest_slot = ent.empty() ? -1 : ent.back().slot;
    info->has_appearance = (h.features & snap::kHasAppearance) != 0; info->has_coarse = (h.features & snap::kHasCoarse) != 0;
    std::memcpy(&info->appearance, h.app, sizeof(h.app)); std::memcpy(&info->coarse, h.coarse, sizeof(h.coarse));
    info->file_bytes = (int64_t)h.file_bytes;
    return ICET_OK;
}

icet_status icet_keyframe_store_snapshot_slots(const char* path, int32_t cap, int32_t* slots, int64_t* stamps, int32_t* n_out) {
    if (!path || cap < 0 || !n_out || (cap > 0 && !slots)) return ICET_ERR_BAD_ARG;
    std::vector<uint8_t> img; snap::Header h; std::vector<snap::Entry> ent; std::string err;
    if (!snap::read_file(path, kSlotLayoutVersion, img, h, ent, err, nullptr)) return ICET_ERR_BAD_ARG;
    for (size_t k = 0; k < ent.size() && k < (size_t)cap; k++) { slots[k] = ent[k].slot; if (stamps) stamps[k] = ent[k].stamp; }
    *n_out = (int32_t)ent.size();
    return ICET_OK;
}

}  // extern "C"
