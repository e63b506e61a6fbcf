// icet_amd/csrc/icet_snapshot.cpp -- the snapshot file of a keyframe store on the host (icet_snapshot.h): reading a whole file through
// the validation, and writing one beside its final name.  No HIP: the device side is icet_snapshot.hip, the calls are icet_store.hip's.
#include "icet_snapshot.h"

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <new>

namespace icet_snapshot {

bool read_file(const char* path, uint32_t layout_version, std::vector<uint8_t>& img, Header& h, std::vector<Entry>& e, std::string& err, bool* opened) {
    if (opened) *opened = false;
    FILE* f = std::fopen(path, "rb");
    if (!f) { err = std::string("cannot open ") + path + ": " + std::strerror(errno); return false; }
    bool ok = std::fseek(f, 0, SEEK_END) == 0;
    const long end = ok ? std::ftell(f) : -1;
    ok = ok && end >= 0 && std::fseek(f, 0, SEEK_SET) == 0;
    if (ok) {
        try { img.resize((size_t)end); } catch (const std::bad_alloc&) { std::fclose(f); err = std::string("no memory for ") + path; return false; }
        ok = end == 0 || std::fread(img.data(), 1, (size_t)end, f) == (size_t)end;
    }
    std::fclose(f);
    if (!ok) { err = std::string("cannot read ") + path; return false; }
    if (opened) *opened = true;
    // the header says how many entries to expect: never more than the file could hold
    const uint64_t cap = img.size() >= kHeaderBytes ? (img.size() - kHeaderBytes) / kEntryBytes : 0;
    const uint64_t n = img.size() >= kHeaderBytes ? get32(img.data() + 56) : 0;
    try { e.assign((size_t)(n < cap ? n : cap), Entry{}); } catch (const std::bad_alloc&) { err = std::string("no memory for ") + path; return false; }
    const char* why = "";
    if (!validate(img.data(), img.size(), layout_version, &h, e.data(), e.size(), &why)) { err = std::string(path) + " is refused: " + why; return false; }
    e.resize(h.n_entries);
    return true;
}

bool writer_open(Writer& w, const char* path, std::string& err) {
    w.path = path; w.tmp = w.path + ".tmp";
    w.f = std::fopen(w.tmp.c_str(), "wb");
    if (!w.f) { err = "cannot open " + w.tmp + ": " + std::strerror(errno); return false; }
    return true;
}

bool writer_write(Writer& w, const void* p, uint64_t bytes, std::string& err) {
    if (bytes && std::fwrite(p, 1, (size_t)bytes, w.f) != (size_t)bytes) { err = "cannot write " + w.tmp + ": " + std::strerror(errno); return false; }
    return true;
}

bool writer_rewind(Writer& w, std::string& err) {
    if (std::fseek(w.f, 0, SEEK_SET) != 0) { err = "cannot seek in " + w.tmp + ": " + std::strerror(errno); return false; }
    return true;
}

bool writer_seek(Writer& w, uint64_t offset, std::string& err) {
    if (fseeko(w.f, (off_t)offset, SEEK_SET) != 0) { err = "cannot seek in " + w.tmp + ": " + std::strerror(errno); return false; }
    return true;
}

bool writer_commit(Writer& w, std::string& err) {
    const bool closed = std::fclose(w.f) == 0;
    w.f = nullptr;
    if (!closed || std::rename(w.tmp.c_str(), w.path.c_str()) != 0) { err = "cannot finish " + w.path + ": " + std::strerror(errno); std::remove(w.tmp.c_str()); return false; }
    return true;
}

void writer_abort(Writer& w) {
    if (w.f) { std::fclose(w.f); w.f = nullptr; }
    if (!w.tmp.empty()) std::remove(w.tmp.c_str());
}

}  // namespace icet_snapshot
