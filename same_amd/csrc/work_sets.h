// work_sets.h -- the protocol of a reader call's work buffer (same_merge_acc_score, _score_detail, _score_map, _score_features, _unpack:
// window_internal.h lays the buffers).  Plain C++ (no HIP, nothing dereferenced): tests/native/work_sets_test.cpp walks it alone.
//
// THE PROTOCOL.  A buffer is laid ONCE for a size and filled ONCE into its idle state; it holds two sets of the words a call counts into,
// used alternately: a call counts into one set and its first kernel clears the other, which the next call counts into, so a set costs no
// fill.  From a call's first enqueue until the wait that follows returns the buffer is IN DOUBT -- marked not laid, so that whatever
// fails in between makes the next call lay and fill it again.
#pragma once
#include <cstdint>

namespace win {

struct WorkSets {
    int64_t laid = 0;     // rows or words the buffer is laid for; 0: not laid, or a call failed half way
    int set = 0;          // the set the next call counts into
    int64_t dirty = 0;    // words of the OTHER set the call before counted into: the next call's first kernel clears them (the detail call's)

    bool fits(int64_t n) const { return laid > 0 && laid >= n; }
    // laid and filled for n: both sets idle, set 0 the first to count into
    void laid_anew(int64_t n) { *this = WorkSets{n, 0, 0}; }
    // the call's first wait returned: the next call counts into the other set, whose `counted` words of this one it clears first
    void flip(int64_t counted = 0) {
        set ^= 1;
        dirty = counted;
    }
};

// The in-doubt window, scoped: enqueueing begins where it is made, sound() says the wait returned.  Every return in between -- the
// early returns of SAME_TRY, HIP_TRY, SAME_COPY and SAME_WAIT among them -- leaves the buffer not laid without doing anything.
struct InDoubt {
    WorkSets &w;
    const int64_t laid;
    explicit InDoubt(WorkSets &sets) : w(sets), laid(sets.laid) { w.laid = 0; }
    InDoubt(const InDoubt &) = delete;
    void sound() { w.laid = laid; }
};

}  // namespace win
