// icet_amd/csrc/icet_snapshot.h -- the snapshot file of a keyframe store (include/icet_hip.h icet_keyframe_store_save / _load): the
// layout, the checksum and the validation, free of HIP, as ONE text that the library's host code, its kernels (the checksum term and the payload layout) and
// the stand-alone test tests/cpp/test_snapshot.cpp compile.  Little-endian; every section starts on a 16-byte boundary; every byte of a file is under a
// checksum; reserved bytes and alignment padding are zero.
//
//   header      160 bytes (kHeaderBytes)
//   directory   n_entries x 128 bytes (kEntryBytes), ascending slots
//   payloads    one per entry, back to back in directory order
//
// Header:  0 magic "ICETKFS1" | 8 version u32 | 12 header bytes u32 | 16 bins_phi | 20 bins_theta | 24 n | 28 thresh bits | 32 buff bits | 36 shape flags
//          (TRUE_SORT | HALF_GAP_BOUNDS) | 40 V | 44 sizeof(SlotHot) | 48 sizeof(SlotFit) | 52 slot-layout version | 56 n_entries | 60 feature bits (1 appearance
//          parameters present, 2 coarse parameters present) | 64 icet_appearance_params (32 B, zero when absent) | 96 icet_coarse_params (32 B, zero when absent) |
//          128 file bytes u64 | 136 checksum of header + directory, taken with this word zero, u64 | 144 16 reserved bytes.
// Entry:   0 slot i32 | 4 n_slots i32 | 8 flags u32 (1 pose, 2 descriptor, 4 grid) | 12 reserved | 16 stamp i64 | 24 the pose table's 12 floats t | R as bits
//          (0xFF bytes without a pose) | 72 payload offset u64 | 80 payload bytes u64 | 88 payload checksum u64 | 96 32 reserved bytes.
// Payload: n_slots SlotHot | n_slots SlotFit | the padded slot_of_voxel row, (V + 1) & ~1 int16 | with a descriptor: A Rp words of columns, then A weights
//          (the store's AppTable row) | with a grid: G G / 8 bytes -- each part padded with zero bytes to 16.
#pragma once
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define ICET_SNAP_HD __host__ __device__
#else
#define ICET_SNAP_HD
#endif

namespace icet_snapshot {

constexpr uint32_t kVersion = 1, kHeaderBytes = 160, kEntryBytes = 128;
constexpr uint32_t kHotBytes = 48, kFitBytes = 80;               // sizeof(SlotHot), sizeof(SlotFit) (icet_internal.h)
constexpr uint32_t kFlagPose = 1, kFlagDesc = 2, kFlagGrid = 4;  // an entry's flags
constexpr uint32_t kHasAppearance = 1, kHasCoarse = 2;           // the header's feature bits
constexpr uint32_t kShapeFlags = 2 | 8;                          // ICET_FLAG_TRUE_SORT | ICET_FLAG_HALF_GAP_BOUNDS
constexpr int32_t kMaxV = 10000;                                 // kMaxVoxels: slot ids travel as int16
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

// ---- the checksum: c = sum_i mix(w_i + (i + 1) kGolden) mod 2^64 over the little-endian u64 words of a byte range.  An exact integer sum: any order of
// summation gives the same value.  mix (the splitmix64 finaliser) is a bijection, so changing any one word changes the sum.
ICET_SNAP_HD inline uint64_t mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
    return z;
}
ICET_SNAP_HD inline uint64_t term(uint64_t w, uint64_t i) { return mix(w + (i + 1) * kGolden); }

inline uint64_t checksum(const uint8_t* p, uint64_t bytes) {      // bytes: a multiple of 8
    uint64_t c = 0;
    for (uint64_t i = 0; i < bytes / 8; i++) { uint64_t w; memcpy(&w, p + 8 * i, 8); c += term(w, i); }
    return c;
}

// ---- the payload of one entry: byte offsets of its parts, each a multiple of 16.  A: sectors, Rp: ceil(rings / 4), G: cells (0 where the file has none).
struct Layout { uint32_t hot, fit, sov, desc, w, grid, size; uint32_t sov_bytes, desc_bytes, w_bytes; };
ICET_SNAP_HD inline uint32_t pad16(uint32_t b) { return (b + 15u) & ~15u; }
ICET_SNAP_HD inline Layout layout(int32_t V, int32_t n_slots, uint32_t flags, int32_t A, int32_t Rp, int32_t G) {      // 0 <= n_slots <= V <= kMaxV, A <= 4096, Rp <= 64, G <= 4096: below 2^31
    Layout l;
    l.hot = 0; l.fit = kHotBytes * (uint32_t)n_slots; l.sov = l.fit + kFitBytes * (uint32_t)n_slots;
    l.sov_bytes = 2u * (((uint32_t)V + 1u) & ~1u);
    l.desc = l.sov + pad16(l.sov_bytes);
    l.desc_bytes = (flags & kFlagDesc) ? 4u * (uint32_t)A * (uint32_t)Rp : 0u;
    l.w = l.desc + pad16(l.desc_bytes);
    l.w_bytes = (flags & kFlagDesc) ? 4u * (uint32_t)A : 0u;
    l.grid = l.w + pad16(l.w_bytes);
    l.size = l.grid + ((flags & kFlagGrid) ? (uint32_t)G * (uint32_t)G / 8u : 0u);
    return l;
}

struct Header {
    int32_t bins_phi, bins_theta, n; uint32_t thresh_bits, buff_bits, shape_flags;
    int32_t V; uint32_t n_entries, features;
    uint32_t app[8], coarse[8];                 // icet_appearance_params / icet_coarse_params as words
    uint64_t file_bytes;
    int32_t A() const { return (features & kHasAppearance) ? (int32_t)app[0] : 0; }
    int32_t Rp() const { return (features & kHasAppearance) ? ((int32_t)app[1] + 3) / 4 : 0; }
    int32_t G() const { return (features & kHasCoarse) ? (int32_t)coarse[0] : 0; }
};
struct Entry { int32_t slot, n_slots; uint32_t flags; int64_t stamp; uint32_t pose[12]; uint64_t off, bytes, sum; };

inline uint32_t get32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t get64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
inline void put32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }
inline void put64(uint8_t* p, uint64_t v) { memcpy(p, &v, 8); }

inline uint64_t directory_end(uint32_t n_entries) { return (uint64_t)kHeaderBytes + (uint64_t)kEntryBytes * n_entries; }

// Header and directory entries into their bytes (the header's checksum word is left zero: seal() fills it in).
inline void put_header(uint8_t* p, const Header& h, uint32_t layout_version) {
    memset(p, 0, kHeaderBytes);
    memcpy(p, "ICETKFS1", 8);
    put32(p + 8, kVersion); put32(p + 12, kHeaderBytes);
    put32(p + 16, (uint32_t)h.bins_phi); put32(p + 20, (uint32_t)h.bins_theta); put32(p + 24, (uint32_t)h.n);
    put32(p + 28, h.thresh_bits); put32(p + 32, h.buff_bits); put32(p + 36, h.shape_flags);
    put32(p + 40, (uint32_t)h.V); put32(p + 44, kHotBytes); put32(p + 48, kFitBytes); put32(p + 52, layout_version);
    put32(p + 56, h.n_entries); put32(p + 60, h.features);
    for (int k = 0; k < 8; k++) { put32(p + 64 + 4 * k, h.app[k]); put32(p + 96 + 4 * k, h.coarse[k]); }
    put64(p + 128, h.file_bytes);
}
inline void put_entry(uint8_t* p, const Entry& e) {
    memset(p, 0, kEntryBytes);
    put32(p, (uint32_t)e.slot); put32(p + 4, (uint32_t)e.n_slots); put32(p + 8, e.flags); put64(p + 16, (uint64_t)e.stamp);
    for (int k = 0; k < 12; k++) put32(p + 24 + 4 * k, e.pose[k]);
    put64(p + 72, e.off); put64(p + 80, e.bytes); put64(p + 88, e.sum);
}
// The checksum of header + directory into the header (img: at least directory_end(n_entries) bytes).
inline void seal(uint8_t* img, uint32_t n_entries) {
    put64(img + 136, 0);
    put64(img + 136, checksum(img, directory_end(n_entries)));
}

inline bool all_zero(const uint8_t* p, uint64_t n) { for (uint64_t i = 0; i < n; i++) if (p[i]) return false; return true; }

// The whole image, before anything is touched.  On success h and e (n_entries of them, the caller's array of at least max_entries) describe it; on refusal
// *why names the first failed check.  e may be null when only the header and the checks are wanted.
// layout_version: kSlotLayoutVersion of icet_internal.h.  Floats are not inspected.  All size arithmetic is in 64 bits, checked against overflow.
inline bool validate(const uint8_t* img, uint64_t size, uint32_t layout_version, Header* h, Entry* e, uint64_t max_entries, const char** why) {
    const char* dummy; if (!why) why = &dummy;
#define ICET_SNAP_FAIL(msg) do { *why = msg; return false; } while (0)
    if (!img || size < kHeaderBytes) ICET_SNAP_FAIL("shorter than a header");
    if (memcmp(img, "ICETKFS1", 8) != 0) ICET_SNAP_FAIL("not a keyframe-store snapshot (magic)");
    if (get32(img + 8) != kVersion) ICET_SNAP_FAIL("unknown format version");
    if (get32(img + 12) != kHeaderBytes) ICET_SNAP_FAIL("header size");
    if (get32(img + 44) != kHotBytes || get32(img + 48) != kFitBytes) ICET_SNAP_FAIL("record sizes differ from this library's");
    if (get32(img + 52) != layout_version) ICET_SNAP_FAIL("slot-layout version differs from this library's");
    Header hd;
    hd.bins_phi = (int32_t)get32(img + 16); hd.bins_theta = (int32_t)get32(img + 20); hd.n = (int32_t)get32(img + 24);
    hd.thresh_bits = get32(img + 28); hd.buff_bits = get32(img + 32); hd.shape_flags = get32(img + 36);
    hd.V = (int32_t)get32(img + 40); hd.n_entries = get32(img + 56); hd.features = get32(img + 60);
    for (int k = 0; k < 8; k++) { hd.app[k] = get32(img + 64 + 4 * k); hd.coarse[k] = get32(img + 96 + 4 * k); }
    hd.file_bytes = get64(img + 128);
    if (hd.bins_phi < 1 || hd.bins_theta < 1 || hd.n < 1 || (int64_t)hd.bins_phi * hd.bins_theta > kMaxV || hd.V != hd.bins_phi * hd.bins_theta) ICET_SNAP_FAIL("grid shape");
    if (hd.shape_flags & ~kShapeFlags) ICET_SNAP_FAIL("shape flags");
    if (hd.features & ~(kHasAppearance | kHasCoarse)) ICET_SNAP_FAIL("feature bits");
    if (!all_zero(img + 144, 16)) ICET_SNAP_FAIL("reserved header bytes are not zero");
    if (hd.features & kHasAppearance) {
        const int32_t sectors = (int32_t)hd.app[0], rings = (int32_t)hd.app[1];
        if (sectors < 8 || sectors > 360 || (sectors & 1) || rings < 1 || rings > 64 || hd.app[5] || hd.app[6] || hd.app[7]) ICET_SNAP_FAIL("appearance parameters");
    } else if (!all_zero(img + 64, 32)) ICET_SNAP_FAIL("appearance parameters without their feature bit");
    if (hd.features & kHasCoarse) {
        const int32_t cells = (int32_t)hd.coarse[0];
        if (cells < 64 || cells > 512 || (cells & 31) || hd.coarse[5] || hd.coarse[6] || hd.coarse[7]) ICET_SNAP_FAIL("coarse parameters");
    } else if (!all_zero(img + 96, 32)) ICET_SNAP_FAIL("coarse parameters without their feature bit");
    if (hd.file_bytes != size) ICET_SNAP_FAIL("the file's size differs from the size its header names");
    if (hd.n_entries > (size - kHeaderBytes) / kEntryBytes) ICET_SNAP_FAIL("more entries than the file can hold");
    const uint64_t dir_end = directory_end(hd.n_entries);
    {   // header + directory under their checksum, taken with the checksum word zero
        uint64_t c = 0;
        for (uint64_t i = 0; i < dir_end / 8; i++) c += term(i == 136 / 8 ? 0 : get64(img + 8 * i), i);
        if (c != get64(img + 136)) ICET_SNAP_FAIL("header / directory checksum");
    }
    if (e && hd.n_entries > max_entries) ICET_SNAP_FAIL("more entries than the caller's array holds");
    uint64_t at = dir_end;                      // payloads lie back to back in directory order: inside the file, aligned, not overlapping, adding up
    int64_t prev = -1;
    for (uint32_t k = 0; k < hd.n_entries; k++) {
        const uint8_t* p = img + kHeaderBytes + (uint64_t)kEntryBytes * k;
        Entry en;
        en.slot = (int32_t)get32(p); en.n_slots = (int32_t)get32(p + 4); en.flags = get32(p + 8); en.stamp = (int64_t)get64(p + 16);
        for (int j = 0; j < 12; j++) en.pose[j] = get32(p + 24 + 4 * j);
        en.off = get64(p + 72); en.bytes = get64(p + 80); en.sum = get64(p + 88);
        if (get32(p + 12) || !all_zero(p + 96, 32)) ICET_SNAP_FAIL("reserved directory bytes are not zero");
        if (en.slot < 0 || (int64_t)en.slot <= prev) ICET_SNAP_FAIL("slots are not strictly ascending from 0");
        prev = en.slot;
        if (en.n_slots < 0 || en.n_slots > hd.V) ICET_SNAP_FAIL("n_slots outside 0 .. V");
        if (en.flags & ~(kFlagPose | kFlagDesc | kFlagGrid)) ICET_SNAP_FAIL("entry flags");
        if ((en.flags & kFlagDesc) && !(hd.features & kHasAppearance)) ICET_SNAP_FAIL("a descriptor without appearance parameters");
        if ((en.flags & kFlagGrid) && !(hd.features & kHasCoarse)) ICET_SNAP_FAIL("a grid without coarse parameters");
        bool ff = true; for (int j = 0; j < 12; j++) ff = ff && en.pose[j] == 0xFFFFFFFFu;
        if (ff == ((en.flags & kFlagPose) != 0)) ICET_SNAP_FAIL("pose flag and pose bytes disagree");
        const Layout l = layout(hd.V, en.n_slots, en.flags, hd.A(), hd.Rp(), hd.G());
        if (en.off & 15u) ICET_SNAP_FAIL("payload offset is not 16-byte aligned");
        if (en.off > size || en.bytes > size - en.off) ICET_SNAP_FAIL("payload outside the file");       // (no sum that could wrap)
        if (en.off != at) ICET_SNAP_FAIL(en.off < at ? "payloads overlap" : "gap between payloads");
        if (en.bytes != l.size) ICET_SNAP_FAIL("payload size differs from its layout");
        at += en.bytes;
        const uint8_t* q = img + en.off;
        if (checksum(q, en.bytes) != en.sum) ICET_SNAP_FAIL("payload checksum");
        // content: what keeps a kernel that reads these tables inside them
        const uint8_t* sov = q + l.sov;
        for (int32_t v = 0; v < hd.V; v++) { int16_t s; memcpy(&s, sov + 2 * v, 2); if (s < -1 || s >= en.n_slots) ICET_SNAP_FAIL("slot_of_voxel entry outside -1 .. n_slots - 1"); }
        for (int32_t i = 0; i < en.n_slots; i++) {
            const int32_t vh = (int32_t)get32(q + l.hot + (uint64_t)kHotBytes * i + 36), vf = (int32_t)get32(q + l.fit + (uint64_t)kFitBytes * i + 76);
            if (vh < 0 || vh >= hd.V || vf < 0 || vf >= hd.V) ICET_SNAP_FAIL("a record's voxel outside 0 .. V - 1");
            int16_t sh, sf; memcpy(&sh, sov + 2 * vh, 2); memcpy(&sf, sov + 2 * vf, 2);
            if (sh != i || sf != i) ICET_SNAP_FAIL("slot_of_voxel does not lead back to the record");
        }
        if (!all_zero(sov + l.sov_bytes, pad16(l.sov_bytes) - l.sov_bytes) || !all_zero(q + l.desc + l.desc_bytes, pad16(l.desc_bytes) - l.desc_bytes) ||
            !all_zero(q + l.w + l.w_bytes, pad16(l.w_bytes) - l.w_bytes)) ICET_SNAP_FAIL("alignment padding is not zero");
        if (e) e[k] = en;
    }
    if (at != size) ICET_SNAP_FAIL("the sizes do not add up to the file's size");
    if (h) *h = hd;
    return true;
#undef ICET_SNAP_FAIL
}

// ---- icet_snapshot.cpp: the file itself (no HIP) ----------------------------------------------------------------------------------------------------------
// A whole file into memory and through validate().  false: err says why; *opened tells a file that could not be opened or read from one that was refused.
bool read_file(const char* path, uint32_t layout_version, std::vector<uint8_t>& img, Header& h, std::vector<Entry>& e, std::string& err, bool* opened);
// A file written beside its final name (path + ".tmp") and renamed when complete: a failed save leaves nothing at `path`.
struct Writer { FILE* f = nullptr; std::string path, tmp; };
bool writer_open(Writer& w, const char* path, std::string& err);
bool writer_write(Writer& w, const void* p, uint64_t bytes, std::string& err);
bool writer_rewind(Writer& w, std::string& err);
bool writer_seek(Writer& w, uint64_t offset, std::string& err);      // the next write goes to `offset` from the file's start (a voxel map's columns, icet_map_snapshot.h)
bool writer_commit(Writer& w, std::string& err);          // close and rename
void writer_abort(Writer& w);                             // close and remove the temporary file

}  // namespace icet_snapshot
