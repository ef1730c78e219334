// work_sets_test.cpp -- the protocol of a reader call's work buffer (same_amd/csrc/work_sets.h) alone: no GPU, no HIP, no library.  The
// calls are modelled as same_merge_acc_score, _score_detail and _unpack compose them from the transitions, with a switch that makes a
// device call "fail" (the early return of SAME_TRY, HIP_TRY, SAME_COPY or SAME_WAIT) -- what no GPU test may provoke.  Built with
// -fsanitize=address,undefined by tests/test_work_sets_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "work_sets.h"

using namespace win;

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

namespace {

constexpr int64_t SMALL = 7, BIG = 300;           // two sizes a buffer is asked for

// the head of every call: laid for too few (or never, or a call failed half way) the buffer is laid again and filled; -> the fill went through
bool ensure_laid(WorkSets &ws, int64_t n, bool fails = false) {
    if (ws.fits(n)) return true;
    InDoubt laying(ws);
    if (fails) return false;
    ws.laid_anew(n);
    return true;
}
// one in-doubt phase: enqueue, copy, wait; -> the wait returned
bool phase(WorkSets &ws, bool fails) {
    InDoubt doubt(ws);
    if (fails) return false;
    doubt.sound();
    return true;
}
// a whole call for n that counts `counted` words (the detail call's; 0: the score call's, the unpack call's first phase)
bool call(WorkSets &ws, int64_t n, int64_t counted, bool fails = false) {
    if (!ensure_laid(ws, n)) return false;
    if (!phase(ws, fails)) return false;
    ws.flip(counted);
    return true;
}

void never_fits(const WorkSets &ws) {
    for (int64_t n : {(int64_t)1, (int64_t)2, SMALL, BIG, (int64_t)1 << 40}) CHECK(!ws.fits(n));
}

void named_sequences() {
    WorkSets ws;
    never_fits(ws);                               // never laid
    CHECK(ws.laid == 0 && ws.set == 0 && ws.dirty == 0);

    // a completed call restores exactly what was laid and flips the set once
    CHECK(call(ws, SMALL, 0));
    CHECK(ws.laid == SMALL && ws.set == 1 && ws.dirty == 0);
    CHECK(ws.fits(1) && ws.fits(SMALL) && !ws.fits(SMALL + 1));
    CHECK(call(ws, SMALL - 1, 0));                // a smaller call fits: nothing is laid again, the set flips back
    CHECK(ws.laid == SMALL && ws.set == 0);

    // a scope left without "the wait returned" leaves "not laid": the next call lays anew, set 0, nothing dirty
    CHECK(call(ws, SMALL, 5));
    CHECK(ws.set == 1 && ws.dirty == 5);
    CHECK(!call(ws, SMALL, 5, true));
    CHECK(ws.laid == 0);
    never_fits(ws);
    CHECK(ensure_laid(ws, SMALL));
    CHECK(ws.laid == SMALL && ws.set == 0 && ws.dirty == 0);

    // a fill that fails while the buffer is laid again leaves "not laid" too
    CHECK(!ensure_laid(ws, BIG, true));
    never_fits(ws);

    // the unpack call: three phases on one set, ONE flip, after the first wait; the later phases restore without flipping
    CHECK(ensure_laid(ws, BIG));
    const int set = ws.set;
    CHECK(phase(ws, false));
    ws.flip();
    CHECK(ws.laid == BIG && ws.set == (set ^ 1));
    CHECK(phase(ws, false) && ws.laid == BIG && ws.set == (set ^ 1));
    CHECK(phase(ws, false) && ws.laid == BIG && ws.set == (set ^ 1));
    CHECK(!phase(ws, true));                      // ... and a later phase that fails leaves the buffer in doubt as the first does
    never_fits(ws);

    // the detail call: the dirty count after a completed call is that call's word count; "laid anew" resets set and dirty count
    WorkSets ds;
    CHECK(call(ds, SMALL, SMALL) && ds.dirty == SMALL && ds.set == 1);
    CHECK(call(ds, 3, 3) && ds.dirty == 3 && ds.set == 0 && ds.laid == SMALL);
    CHECK(call(ds, SMALL, SMALL) && ds.set == 1);
    CHECK(call(ds, BIG, BIG));                    // too small: laid anew (set 0, nothing dirty), counted into, flipped
    CHECK(ds.laid == BIG && ds.set == 1 && ds.dirty == BIG);
    ds.laid_anew(SMALL);
    CHECK(ds.laid == SMALL && ds.set == 0 && ds.dirty == 0);

    // the detail call marks two buffers: a failure leaves both in doubt, a completed call flips only its own
    WorkSets score, detail;
    CHECK(ensure_laid(score, BIG) && ensure_laid(detail, SMALL));
    {
        InDoubt doubt_score(score), doubt(detail);
        CHECK(!score.fits(1) && !detail.fits(1));
        doubt_score.sound();
        doubt.sound();
        detail.flip(SMALL);
    }
    CHECK(score.laid == BIG && score.set == 0 && detail.laid == SMALL && detail.set == 1);
    {
        InDoubt doubt_score(score), doubt(detail);
    }
    never_fits(score);
    never_fits(detail);
}

// ---- every sequence of up to five transitions against the invariants ---------------------------------------------------------------
long walked = 0;

void invariants(const WorkSets &ws) {
    CHECK(ws.set == 0 || ws.set == 1);
    CHECK(ws.laid == 0 || ws.laid == SMALL || ws.laid == BIG);
    CHECK(ws.dirty >= 0 && ws.dirty <= BIG);
    CHECK(ws.fits(1) == (ws.laid > 0));
    if (ws.laid == 0) never_fits(ws);
}

void walk(const WorkSets &from, int depth) {
    if (depth == 0) return;
    for (int t = 0; t < 9; ++t) {
        WorkSets ws = from;
        const int set = ws.set;
        const int64_t laid = ws.laid;
        switch (t) {
        case 0: CHECK(ensure_laid(ws, SMALL) && ws.fits(SMALL)); break;
        case 1: CHECK(ensure_laid(ws, BIG) && ws.laid == BIG); break;
        case 2: CHECK(!ensure_laid(ws, BIG + 1, true) && ws.laid == 0); break;
        case 3: CHECK(call(ws, SMALL, 0) && ws.dirty == 0); break;
        case 4: CHECK(call(ws, BIG, BIG) && ws.dirty == BIG && ws.laid == BIG); break;
        case 5: CHECK(!call(ws, SMALL, SMALL, true) && ws.laid == 0); break;
        case 6: CHECK(phase(ws, false) && ws.laid == laid && ws.set == set); break;
        case 7: CHECK(!phase(ws, true) && ws.laid == 0 && ws.set == set); break;
        default: ws.flip(SMALL); CHECK(ws.set == (set ^ 1) && ws.laid == laid);
        }
        if ((t == 3 || t == 4) && from.fits(t == 3 ? SMALL : BIG)) CHECK(ws.set == (set ^ 1) && ws.laid == laid);   // it fitted: one flip
        if ((t == 3 || t == 4) && !from.fits(t == 3 ? SMALL : BIG)) CHECK(ws.set == 1);                             // laid anew: set 0, one flip
        ++walked;
        invariants(ws);
        walk(ws, depth - 1);
    }
}

}  // namespace

int main() {
    named_sequences();
    WorkSets ws;
    invariants(ws);
    walk(ws, 5);
    CHECK(walked > 50000);
    std::printf("%ld states walked\nok\n", walked);
    return 0;
}
