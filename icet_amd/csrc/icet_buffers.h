// icet_amd/csrc/icet_buffers.h -- who owns device and pinned memory: a BufferGroup is a set of allocations with ONE lifetime.  The structs the launch functions
// take (Workspace, AuxDev, the store's tables) stay plain views of raw pointers; a group allocates INTO such a pointer (the slot), remembers the allocation and the
// slot's address, and frees the one and nulls the other in release().  The owning structs are heap objects that never move, so a slot's address stays good.
// Nothing of HIP in here: the runtime is reached through the four functions of icet::mem (the library: icet_capi.hip; a host test: malloc).
#pragma once
#include <cstddef>
#include <cstdlib>
#include <utility>
#include <vector>

namespace icet {
namespace mem {      // each returns 0 or the runtime's error code (a hipError_t in the library)
int dev_alloc(void** p, size_t bytes);
int dev_free(void* p);
int pinned_alloc(void** p, size_t bytes, unsigned flags);
int pinned_free(void* p);
}  // namespace mem

class BufferGroup {
public:
    BufferGroup() = default;
    BufferGroup(const BufferGroup&) = delete;
    BufferGroup& operator=(const BufferGroup&) = delete;
    ~BufferGroup() { release(); }
    // `count` elements into `slot` (which must be null: a group grows by release() and allocation anew).  On failure the slot stays null and what the group already
    // holds stays live.  count == 0: nothing to own, the slot stays null.
    template <class T> int device(T*& slot, size_t count) { return take(reinterpret_cast<void**>(&slot), count * sizeof(T), false, 0); }
    template <class T> int pinned(T*& slot, size_t count, unsigned flags = 0) { return take(reinterpret_cast<void**>(&slot), count * sizeof(T), true, flags); }
    int device_bytes(void*& slot, size_t bytes) { return take(&slot, bytes, false, 0); }      // (a table without an element type)
    // Frees every allocation exactly once and nulls every slot; the group is empty afterwards (a second call frees nothing).
    void release() {
        for (const Rec& r : recs_) { *r.slot = nullptr; (void)(r.pinned ? mem::pinned_free(r.p) : mem::dev_free(r.p)); }
        recs_.clear();
    }
    // Exchanges the allocations of two groups of the SAME shape (as many allocations of the same kinds, made in the same order), slot by slot: every slot stays
    // with its group and now points at the other's memory.  Not a general swap or move: a group is bound to the addresses of its slots, so two groups can only
    // trade memory that fits each other's slots.  Grow-then-swap: a new table is built in a local group by the allocator that built the old one, filled, and
    // changes places with it; the local group then frees the old table, and a failure before the swap leaves the old group untouched.  Groups of different
    // shapes are a programming error: the process is aborted, in every build, before anything is exchanged.
    void swap(BufferGroup& o) {
        bool same = recs_.size() == o.recs_.size();
        for (size_t k = 0; same && k < recs_.size(); k++) same = recs_[k].pinned == o.recs_[k].pinned;
        if (!same) std::abort();
        for (size_t k = 0; k < recs_.size(); k++) {
            std::swap(recs_[k].p, o.recs_[k].p);
            *recs_[k].slot = recs_[k].p; *o.recs_[k].slot = o.recs_[k].p;
        }
    }
    bool empty() const { return recs_.empty(); }

private:
    struct Rec { void* p; void** slot; bool pinned; };
    std::vector<Rec> recs_;
    int take(void** slot, size_t bytes, bool pinned, unsigned flags) {
        if (*slot != nullptr) std::abort();                  // (a programming error, in every build: the slot would lose its owner)
        if (bytes == 0) return 0;
        recs_.reserve(recs_.size() + 1);                    // (the record's own memory first: nothing below can fail between the allocation and its record)
        void* p = nullptr;
        const int e = pinned ? mem::pinned_alloc(&p, bytes, flags) : mem::dev_alloc(&p, bytes);
        if (e != 0) return e;
        *slot = p;
        recs_.push_back(Rec{p, slot, pinned});
        return 0;
    }
};

// THE GROW STEP of a group that one capacity guards (the caller has seen need > cap and drained whatever may still read the old buffers): the capacity goes to 0 and
// the group is released, `allocate` makes the new allocations (0, or the first error code), and only when all of them succeeded is the capacity set.  A refusal
// returns the runtime's code and leaves capacity 0 and every slot null (what the refused growth did get is freed), so the next call grows again: at every return
// a non-zero capacity means live buffers, and a null pointer means capacity 0.
template <class C, class N, class F> int grow(BufferGroup& g, C& cap, N need, F&& allocate) {
    cap = 0; g.release();
    const int e = static_cast<int>(allocate());
    if (e == 0) cap = static_cast<C>(need); else g.release();
    return e;
}

}  // namespace icet
