// tests/cpp/test_map_snapshot.cpp -- the voxel map's snapshot format (icet_amd/csrc/icet_map_snapshot.h) as a stand-alone host program:
// the header the library and its kernels compile, held to itself here (and under AddressSanitizer + UBSan) and to the NumPy model by tests/test_map_snapshot_host.py.
//   selftest              write -> parse returns every field; every proper prefix and every single-byte change of a 37-entry shaped file is refused; images
//                         with valid checksums and bad contents are refused, each from a heap block of exactly its size
//   write PATH            the program's own 37-entry shaped file
//   rewrite SRC DST       SRC through validate() and written again from what it returned (exit 2: refused, the reason on stderr)
//   info PATH             the header's fields, one line
#include "../../icet_amd/csrc/icet_map_snapshot.h"

#include <stdlib.h>

namespace ms = icet_map_snapshot;

struct Image { ms::Header h; std::vector<uint64_t> keys; std::vector<std::vector<uint64_t>> cols; };      // cols: W - 1 columns of n words

static uint64_t key_of(uint32_t x, uint32_t y, uint32_t z) { return ((uint64_t)x << 42) | ((uint64_t)y << 21) | z; }

// n entries of a shaped or plain map by a fixed formula: ascending keys around the grid's middle, words of every kind (negative, zero beside non-zero).
static Image make_image(uint64_t n, bool shaped) {
    Image im;
    memset(&im.h, 0, sizeof(im.h));
    const float cell = 0.25f, mn = 1.5f, mx = 80.f;
    memcpy(&im.h.cell_bits, &cell, 4); memcpy(&im.h.min_range_bits, &mn, 4); memcpy(&im.h.max_range_bits, &mx, 4);
    im.h.flags = shaped ? ms::kFlagShaped : 0u; im.h.words = ms::words_of(shaped); im.h.n = n;
    const int64_t tot[5] = {123456, 120000 - 77, 12, 3400, 0};
    for (int k = 0; k < 5; k++) im.h.totals[k] = tot[k];
    im.cols.assign(im.h.words - 1, std::vector<uint64_t>(n));
    for (uint64_t i = 0; i < n; i++) {
        im.keys.push_back(key_of((1u << 20) - 3 + (uint32_t)(i / 7), (1u << 20) + (uint32_t)(i % 7), 1 + (uint32_t)i));
        for (uint32_t c = 0; c + 1 < im.h.words; c++) im.cols[c][i] = icet_snapshot::mix(i * 31 + c) >> (c == 0 ? 44 : 8);
    }
    if (n > 2) { im.cols[0][1] = (uint64_t)-5; im.cols[0][2] = 0; }   // a negative count; a zero count beside non-zero sums
    im.h.file_bytes = ms::file_bytes(n, im.h.words);
    return im;
}

// The image's bytes as the format lays them out; the header is written as it stands in im.h (a test may make it lie) with both checksums valid.
static std::vector<uint8_t> bytes_of(const Image& im, uint64_t pad_word = 0) {
    const uint64_t n = im.keys.size(), cw = ms::column_words(n);
    const uint32_t W = (uint32_t)im.cols.size() + 1;
    std::vector<uint8_t> out((size_t)(ms::kHeaderBytes + 8 * W * cw), 0);
    for (uint32_t c = 0; c < W; c++) {
        for (uint64_t i = 0; i < n; i++) ms::put64(out.data() + ms::kHeaderBytes + 8 * (c * cw + i), c == 0 ? im.keys[i] : im.cols[c - 1][i]);
        if (n & 1) ms::put64(out.data() + ms::kHeaderBytes + 8 * (c * cw + n), pad_word);
    }
    ms::Header h = im.h;
    h.payload_sum = icet_snapshot::checksum(out.data() + ms::kHeaderBytes, out.size() - ms::kHeaderBytes);
    ms::put_header(out.data(), h);
    ms::seal(out.data());
    return out;
}

// validate() on a heap block of exactly `size` bytes: a read behind the image is the sanitizer's to report.
static bool check(const std::vector<uint8_t>& img, uint64_t size, ms::Header* h, const char** why) {
    uint8_t* p = (uint8_t*)malloc(size ? size : 1);
    if (size) memcpy(p, img.data(), size);
    const bool ok = ms::validate(p, size, h, why);
    free(p);
    return ok;
}

static int fail(const char* what) { fprintf(stderr, "FAILED: %s\n", what); return 1; }

static int refused(const Image& im, const char* name, const char* want, uint64_t pad_word = 0) {
    const std::vector<uint8_t> b = bytes_of(im, pad_word);
    const char* why = "";
    if (check(b, b.size(), nullptr, &why)) { fprintf(stderr, "FAILED: accepted %s\n", name); return 1; }
    if (!strstr(why, want)) { fprintf(stderr, "FAILED: %s refused for \"%s\", not for \"%s\"\n", name, why, want); return 1; }
    return 0;
}

static int selftest() {
    int images = 0;
    for (int shaped = 0; shaped < 2; shaped++) {
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)37}) {
            const Image im = make_image(n, shaped != 0);
            const std::vector<uint8_t> b = bytes_of(im);
            ms::Header h; const char* why = "";
            if (!check(b, b.size(), &h, &why)) return fail(why);
            if (h.cell_bits != im.h.cell_bits || h.min_range_bits != im.h.min_range_bits || h.max_range_bits != im.h.max_range_bits || h.flags != im.h.flags ||
                h.words != im.h.words || h.n != n || memcmp(h.totals, im.h.totals, sizeof(h.totals)) != 0 || h.file_bytes != b.size() ||
                h.payload_sum != icet_snapshot::checksum(b.data() + ms::kHeaderBytes, b.size() - ms::kHeaderBytes))
                return fail("write -> parse does not return every field");
            if (b.size() % 16 != 0 || b.size() != ms::kHeaderBytes + 8 * (uint64_t)h.words * ((n + 1) & ~(uint64_t)1)) return fail("the file's size");
            {   // the sum a pack kernel forms: the entries' words by their place in the whole payload, and the host's padding terms
                uint64_t c = ms::padding_sum(n, h.words);
                for (uint32_t col = 0; col < h.words; col++)
                    for (uint64_t i = 0; i < n; i++) c += ms::term(col == 0 ? im.keys[i] : im.cols[col - 1][i], ms::word_index(n, col, i));
                if (c != h.payload_sum) return fail("the payload checksum by columns differs from the checksum of the bytes");
            }
            for (uint64_t cut = 0; cut < b.size(); cut++) if (check(b, cut, nullptr, nullptr)) return fail("a proper prefix was accepted");
            images++;
        }
    }
    {   // every byte set to each of the 255 other values: a single-byte change is never accepted
        const Image im = make_image(37, true);
        std::vector<uint8_t> b = bytes_of(im);
        for (size_t i = 0; i < b.size(); i++) {
            const uint8_t keep = b[i];
            for (int v = 1; v < 256; v++) {
                b[i] = (uint8_t)(keep ^ v);
                if (ms::validate(b.data(), b.size(), nullptr, nullptr)) { fprintf(stderr, "FAILED: byte %zu changed to %u accepted\n", i, b[i]); return 1; }
            }
            b[i] = keep;
        }
        if (!ms::validate(b.data(), b.size(), nullptr, nullptr)) return fail("the restored image");
    }
    // valid checksums, bad contents
    int bad = 0;
    { Image im = make_image(37, true); std::swap(im.keys[10], im.keys[11]); bad += refused(im, "keys out of order", "ascending"); }
    { Image im = make_image(37, true); im.keys[11] = im.keys[10]; bad += refused(im, "equal keys", "ascending"); }
    { Image im = make_image(37, true); im.keys[0] &= ~(uint64_t)0x1FFFFF; bad += refused(im, "a zero z field", "key"); }
    { Image im = make_image(37, true); im.keys[5] &= ~((uint64_t)0x1FFFFF << 21); bad += refused(im, "a zero y field", "key"); }
    { Image im = make_image(37, true); im.keys[5] &= ((uint64_t)1 << 42) - 1; bad += refused(im, "a zero x field", "key"); }
    { Image im = make_image(37, true); im.keys[36] |= (uint64_t)1 << 63; bad += refused(im, "a key of 2^63 or above", "key"); }
    { Image im = make_image(37, true); im.keys[36] = ~(uint64_t)0; bad += refused(im, "the empty key", "key"); }
    { Image im = make_image(37, true); for (auto& c : im.cols) c[20] = 0; bad += refused(im, "an all-zero entry", "all zero"); }
    { Image im = make_image(37, false); for (auto& c : im.cols) c[0] = 0; bad += refused(im, "an all-zero plain entry", "all zero"); }
    { Image im = make_image(37, true); bad += refused(im, "non-zero padding", "padding", 1); }
    { Image im = make_image(37, true); im.h.flags = 0; bad += refused(im, "14 words without the shaped flag", "words per entry"); }
    { Image im = make_image(37, false); im.h.flags = ms::kFlagShaped; bad += refused(im, "5 words with the shaped flag", "words per entry"); }
    { Image im = make_image(37, true); im.h.words = 13; bad += refused(im, "13 words", "words per entry"); }
    { Image im = make_image(37, true); im.h.flags = 3; bad += refused(im, "an unknown flag", "flags"); }
    for (uint64_t n : {(uint64_t)36, (uint64_t)39, (uint64_t)40, (uint64_t)1 << 30, ((uint64_t)1 << 30) + 1, ~(uint64_t)0, ((uint64_t)1 << 61) + 37}) {
        Image im = make_image(37, true); im.h.n = n;                 // (38 shares 37's size: its 38th key is the zero padding word, refused as a key)
        bad += refused(im, "n against the size", n > ms::kMaxEntries ? "more entries" : "size");
    }
    { Image im = make_image(37, true); im.h.n = 38; bad += refused(im, "n = 38 on 37 entries", "key"); }
    { Image im = make_image(37, true); im.h.file_bytes += 16; bad += refused(im, "a size the file does not have", "size"); }
    if (bad) return 1;
    printf("map snapshot ok: %d images\n", images);
    return 0;
}

static bool read_all(const char* path, std::vector<uint8_t>& b) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[4096]; size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + got);
    fclose(f);
    return true;
}
static bool write_all(const char* path, const std::vector<uint8_t>& b) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(b.data(), 1, b.size(), f) == b.size();
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "selftest") return selftest();
    if (mode == "write" && argc == 3) return write_all(argv[2], bytes_of(make_image(37, true))) ? 0 : 1;
    if ((mode == "rewrite" && argc == 4) || (mode == "info" && argc == 3)) {
        std::vector<uint8_t> b;
        if (!read_all(argv[2], b)) return 1;
        ms::Header h; const char* why = "";
        if (!check(b, b.size(), &h, &why)) { fprintf(stderr, "refused: %s\n", why); return 2; }
        if (mode == "info") {
            printf("%u %u %u %u %u %llu %lld %lld %lld %lld %lld %llu %llu\n", h.cell_bits, h.min_range_bits, h.max_range_bits, h.flags, h.words, (unsigned long long)h.n,
                   (long long)h.totals[0], (long long)h.totals[1], (long long)h.totals[2], (long long)h.totals[3], (long long)h.totals[4],
                   (unsigned long long)h.file_bytes, (unsigned long long)h.payload_sum);
            return 0;
        }
        Image im; im.h = h;
        const uint64_t cw = ms::column_words(h.n);
        im.cols.assign(h.words - 1, std::vector<uint64_t>((size_t)h.n));
        for (uint64_t i = 0; i < h.n; i++) {
            im.keys.push_back(ms::get64(b.data() + ms::kHeaderBytes + 8 * i));
            for (uint32_t c = 1; c < h.words; c++) im.cols[c - 1][i] = ms::get64(b.data() + ms::kHeaderBytes + 8 * (c * cw + i));
        }
        return write_all(argv[3], bytes_of(im)) ? 0 : 1;
    }
    fprintf(stderr, "usage: test_map_snapshot selftest | write PATH | rewrite SRC DST | info PATH\n");
    return 64;
}
