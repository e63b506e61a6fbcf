// icet_amd/csrc/icet_map_snapshot.h -- the snapshot file of a voxel map (include/icet_hip.h icet_voxel_map_save / _load / _snapshot_info):
// the layout, the checksum and the validation, free of HIP, as ONE text that the library's host code, its kernels (the checksum term and the column layout) and
// the stand-alone test tests/cpp/test_map_snapshot.cpp compile.  Little-endian; every part starts on a 16-byte boundary; every byte of a file is under a
// checksum; reserved bytes and alignment padding are zero.  The checksum rule is icet_snapshot.h's.
//
//   header      128 bytes (kHeaderBytes)
//   payload     W columns of n u64 words each, a column of odd length padded with one zero word: key | count | sum x | sum y | sum z | (a shaped map) the nine
//               moment words S_x S_y S_z M_xx M_xy M_xz M_yy M_yz M_zz (icet_map_shape.h)
//
// Header:  0 magic "ICETVXM1" | 8 version u32 | 12 header bytes u32 | 16 cell bits | 20 min_range bits | 24 max_range bits | 28 flags (bit 0: shaped) |
//          32 words per entry W (5 plain, 14 shaped) | 36 reserved u32 | 40 entries n u64 | 48 points_in | 56 points_kept | 64 points_nonfinite | 72 points_outside |
//          80 points_dropped (i64 each) | 88 file bytes u64 | 96 checksum of the payload, one word index over all of it, u64 | 104 checksum of the header, taken
//          with this word zero, u64 | 112 16 reserved bytes.
// Entries: every claimed entry of the table with at least one non-zero value word, by strictly ascending key.  A cell that a remove emptied (all words zero) is
//          not written: it cannot be told from an absent cell.  A negative count, or a zero count beside non-zero sums, is written as it is.  So the file is a
//          function of the map's contents alone: table size, insertion order and call boundaries do not show in it.
#pragma once
#include <errno.h>
#include <new>
#include "icet_snapshot.h"

namespace icet_map_snapshot {

using icet_snapshot::get32; using icet_snapshot::get64; using icet_snapshot::put32; using icet_snapshot::put64; using icet_snapshot::term;

constexpr uint32_t kVersion = 1, kHeaderBytes = 128;
constexpr uint32_t kFlagShaped = 1;
constexpr uint32_t kWordsPlain = 5, kWordsShaped = 14;      // key, count, three sums; and the nine moment words
constexpr uint64_t kMaxEntries = (uint64_t)1 << 30;          // the largest table
constexpr uint32_t kOffHeaderSum = 104;

struct Header {
    uint32_t cell_bits, min_range_bits, max_range_bits, flags, words;
    uint64_t n;
    int64_t totals[5];                          // points_in, points_kept, points_nonfinite, points_outside, points_dropped
    uint64_t file_bytes, payload_sum;
    bool shaped() const { return (flags & kFlagShaped) != 0; }
};

ICET_SNAP_HD inline uint32_t words_of(bool shaped) { return shaped ? kWordsShaped : kWordsPlain; }
ICET_SNAP_HD inline uint64_t column_words(uint64_t n) { return (n + 1) & ~(uint64_t)1; }                  // a column's words with its padding: 8 n bytes padded to 16
ICET_SNAP_HD inline uint64_t word_index(uint64_t n, uint32_t column, uint64_t entry) { return column * column_words(n) + entry; }      // the checksum's index of a payload word
inline uint64_t column_offset(uint64_t n, uint32_t column) { return (uint64_t)kHeaderBytes + 8 * column * column_words(n); }           // n <= kMaxEntries: below 2^38
inline uint64_t file_bytes(uint64_t n, uint32_t words) { return column_offset(n, words); }

// What the padding words add to the payload checksum (they are zero, their terms are not): a pack kernel sums the entries' words, the host adds this.
inline uint64_t padding_sum(uint64_t n, uint32_t words) {
    uint64_t c = 0;
    if (n & 1) for (uint32_t col = 0; col < words; col++) c += term(0, word_index(n, col, n));
    return c;
}

// A key as the map's rule forms it (icet_map.h make_key): three 21-bit fields c + 2^20 with |c| < 2^20, so each lies in 1 .. 2^21 - 1 and the key below 2^63.
inline bool key_ok(uint64_t key) {
    if (key >> 63) return false;
    for (int a = 0; a < 3; a++) { const uint64_t f = (key >> (21 * a)) & 0x1FFFFF; if (f < 1) return false; }
    return true;
}

// The header into its bytes (the header's checksum word is left zero: seal() fills it in).
inline void put_header(uint8_t* p, const Header& h) {
    memset(p, 0, kHeaderBytes);
    memcpy(p, "ICETVXM1", 8);
    put32(p + 8, kVersion); put32(p + 12, kHeaderBytes);
    put32(p + 16, h.cell_bits); put32(p + 20, h.min_range_bits); put32(p + 24, h.max_range_bits); put32(p + 28, h.flags); put32(p + 32, h.words);
    put64(p + 40, h.n);
    for (int k = 0; k < 5; k++) put64(p + 48 + 8 * k, (uint64_t)h.totals[k]);
    put64(p + 88, h.file_bytes); put64(p + 96, h.payload_sum);
}
inline void seal(uint8_t* p) {
    put64(p + kOffHeaderSum, 0);
    put64(p + kOffHeaderSum, icet_snapshot::checksum(p, kHeaderBytes));
}

// The whole image, before anything is touched.  On success *h describes it; on refusal *why names the first failed check.  Floats are not inspected.  Every
// size is compared in 64 bits without a sum that could wrap: n <= 2^30 bounds W pad16(8 n) by 2^38.
inline bool validate(const uint8_t* img, uint64_t size, Header* h, const char** why) {
    const char* dummy; if (!why) why = &dummy;
#define ICET_MSNAP_FAIL(msg) do { *why = msg; return false; } while (0)
    if (!img || size < kHeaderBytes) ICET_MSNAP_FAIL("shorter than a header");
    if (memcmp(img, "ICETVXM1", 8) != 0) ICET_MSNAP_FAIL("not a voxel-map snapshot (magic)");
    if (get32(img + 8) != kVersion) ICET_MSNAP_FAIL("unknown format version");
    if (get32(img + 12) != kHeaderBytes) ICET_MSNAP_FAIL("header size");
    Header hd;
    hd.cell_bits = get32(img + 16); hd.min_range_bits = get32(img + 20); hd.max_range_bits = get32(img + 24); hd.flags = get32(img + 28); hd.words = get32(img + 32);
    hd.n = get64(img + 40);
    for (int k = 0; k < 5; k++) hd.totals[k] = (int64_t)get64(img + 48 + 8 * k);
    hd.file_bytes = get64(img + 88); hd.payload_sum = get64(img + 96);
    if (hd.flags & ~kFlagShaped) ICET_MSNAP_FAIL("flags");
    if (hd.words != words_of(hd.shaped())) ICET_MSNAP_FAIL("words per entry against the shaped flag (5 plain, 14 shaped)");
    if (get32(img + 36) || !icet_snapshot::all_zero(img + 112, 16)) ICET_MSNAP_FAIL("reserved header bytes are not zero");
    if (hd.n > kMaxEntries) ICET_MSNAP_FAIL("more entries than the largest table holds");
    if (hd.file_bytes != size) ICET_MSNAP_FAIL("the file's size differs from the size its header names");
    if (size - kHeaderBytes != 8 * (uint64_t)hd.words * column_words(hd.n)) ICET_MSNAP_FAIL("the file's size differs from header + W columns of n words");
    {   // the header under its checksum, taken with the checksum word zero
        uint64_t c = 0;
        for (uint64_t i = 0; i < kHeaderBytes / 8; i++) c += term(i == kOffHeaderSum / 8 ? 0 : get64(img + 8 * i), i);
        if (c != get64(img + kOffHeaderSum)) ICET_MSNAP_FAIL("header checksum");
    }
    const uint8_t* pay = img + kHeaderBytes;
    if (icet_snapshot::checksum(pay, size - kHeaderBytes) != hd.payload_sum) ICET_MSNAP_FAIL("payload checksum");
    // content: what keeps a kernel that merges these columns sane
    const uint64_t n = hd.n, cw = column_words(n);
    if (n & 1) for (uint32_t c = 0; c < hd.words; c++) if (get64(pay + 8 * (c * cw + n))) ICET_MSNAP_FAIL("alignment padding is not zero");
    uint64_t prev = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t key = get64(pay + 8 * i);
        if (!key_ok(key)) ICET_MSNAP_FAIL("a key is not a cell's (2^63 or above, or a zero field)");
        if (i > 0 && key <= prev) ICET_MSNAP_FAIL("keys are not strictly ascending");
        prev = key;
        uint64_t any = 0;
        for (uint32_t c = 1; c < hd.words; c++) any |= get64(pay + 8 * (c * cw + i));
        if (!any) ICET_MSNAP_FAIL("an entry whose value words are all zero");
    }
    if (h) *h = hd;
    return true;
#undef ICET_MSNAP_FAIL
}

// A whole file into memory and through validate().  false: err says why.
inline bool read_file(const char* path, std::vector<uint8_t>& img, Header& h, std::string& err) {
    FILE* f = fopen(path, "rb");
    if (!f) { err = std::string("cannot open ") + path + ": " + strerror(errno); return false; }
    bool ok = fseek(f, 0, SEEK_END) == 0;
    const long end = ok ? ftell(f) : -1;
    ok = ok && end >= 0 && fseek(f, 0, SEEK_SET) == 0;
    if (ok) {
        try { img.resize((size_t)end); } catch (const std::bad_alloc&) { fclose(f); err = std::string("no memory for ") + path; return false; }
        ok = end == 0 || fread(img.data(), 1, (size_t)end, f) == (size_t)end;
    }
    fclose(f);
    if (!ok) { err = std::string("cannot read ") + path; return false; }
    const char* why = "";
    if (!validate(img.data(), img.size(), &h, &why)) { err = std::string(path) + " is refused: " + why; return false; }
    return true;
}

}  // namespace icet_map_snapshot
