// window_state.h -- a window's LOGICAL state: which arrays and which pair list are the window's right now, which saved ones stand behind
// them, and which results still hold.  Plain C++ (no HIP, no buffers, nothing dereferenced): the window calls of window_*.hip own the
// buffers and the kernels, and change the state only through the transitions below; tests/native/window_state_test.cpp walks them alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace win {

// A window's pair list: row a of the aligned side owns pairs [prow[a], prow[a + 1]); pair p is (pairs[2p] = aligned row, pairs[2p + 1] =
// the reference's number in the window), jsec[p] that reference's SECTION row, cost64[p] its cost; P pairs.  The stage call makes one;
// the priority prune, the k-NN prefix and the caller's removal each derive a second from one (source and destination of their kernels)
// and turn the window to it.
struct PairList {
    int32_t *prow = nullptr, *pairs = nullptr, *jsec = nullptr;
    double *cost64 = nullptr;
    int64_t P = 0;
};

// The aligned side and the pair list a call works on: the count block ([0] aligned rows in the box, [1] reference rows, [2] kept, [3]
// pairs), the kept cells (index among the box's rows, section row, type code, XY, size; n_ua of them) and their pairs.  The stage call lays
// one in the `stage` buffer, a caller's triangulation a smaller one in the `caller` buffer.
struct View {
    unsigned long long *counts = nullptr;
    int32_t *ua = nullptr, *rows_ua = nullptr, *type_c = nullptr;
    double *axy_c = nullptr, *size_c = nullptr;
    int64_t n_ua = 0;
    PairList list;
};

// A caller's selection kept for a window that was turned back to the stage call's arrays (hold_caller): the node mask, the renumbering,
// the compacted view (cs: its pair arrays hold `cap` pairs) and the renumbered triangles stay in the `caller` buffer as prepare_caller
// laid them, and same_window_caller_pairs pushes the window's current list through the mask into cs.
struct Held {
    int on = 0;                                 // the window is as a stage call leaves it AND `caller` holds a selection for it
    View cs;
    const uint8_t *valid = nullptr;             // [st0.n_ua] the node mask
    const int32_t *newidx = nullptr;            // [st0.n_ua] kept cell as staged -> kept cell left, or -1
    unsigned long long *st = nullptr;           // the cell scan's words (a scan::arg)
    size_t back_bytes = 0;                      // counts + kept XY + kept rows: what takes the stage block's place in the pinned block
    int64_t cap = 0;
};

enum Staged { UNSTAGED = 0, STAGED_NO_PAIRS = 1, STAGED = 2 };     // STAGED_NO_PAIRS: a side of the box is empty (src/same.py:1003 raises)
enum Source { FROM_HOST = 0, FROM_DEVICE = 1, FROM_CALLER = 2 };   // whose triangles a finish call filters

// THE STATE MACHINE: per call what it requires of the state, what it leaves, what it invalidates (the transition that says so).
// "results" = finished, filtered, Tr.  A view is the stage call's or the compacted one; "the list as staged" is what as_staged() answers.
//
//   call                      requires                 leaves                                                    invalidates
//   stage                     --                       cur = the stage view, sk = its list, k = k_staged;        everything (begin_stage)
//                                                      staged, once the counts are back
//   priority_pairs            may_prune                pr = the list it read, cur.list = what is left of it,     -- (a window without pairs: no change)
//                                                      prio_ok (pruned)
//   knn_prefix(k)             may_prefix(k)            a compacted window turned back to st0 and HELD            caller_sel, caller_ok (hold_caller);
//                                                      (hold_caller); cur.list = the prefix, sk at k_staged;     prio_ok, pr, results (staged_at)
//                                                      k (staged_at)
//   recost                    may_recost               as knn_prefix(k_staged), sk's costs written again         as knn_prefix
//   caller_tris, both forms   may_select               st0 = the view it starts from: st0 again where the        held; results where the window was
//     (classifying / the                               window was compacted, else cur (restart_caller)           compacted (restart_caller)
//     host's mask)
//     -> a cosine at the                               caller_sel, n_sel; cur as it started (selected)           --
//        threshold
//     -> otherwise                                     ... and cur = the compacted view, caller_ok, n_caller,    dd_ok, results (compacted)
//                                                      held's pointers with held.on = 0 (compacted)
//   caller_pairs              may_push_pairs, and      st0 = cur, cur = held.cs with the pushed list,            held.on, dd_ok, results (compacted)
//                             held.on or no kept cell  caller_sel, caller_ok (compacted)
//   delaunay                  may_triangulate          dd_ok where the device answered (triangulated)            dd_ok, first
//   filter_finish             may_finish_from:         Tr, filtered, finished (finished_with); a window with a   results, first (results_void)
//     FROM_HOST               pairs_possible           cosine at the threshold: none of them
//     FROM_DEVICE             ... and dd_ok
//     FROM_CALLER             ... and caller_ok
//   refinish                  has_results              the results again, from the caller's matching             --
//   collect                   has_results              --                                                        --
//   fetch                     is_staged; signs, weights, match: finished; triangles: has_triangles; caller triangles: caller_sel; staged pairs: as_staged()
//
// A failed batch leaves its windows UNSTAGED (win::fail_batch).  dd_ok survives a prefix, a prune and a recost: they leave the aligned
// side alone, and a window that was compacted lost it already (hold_caller does not void a triangulation made OF the compacted window:
// the device's triangulation and a caller's are two routes, no caller mixes them).
struct State {
    View cur;                                   // the window NOW: what every kernel of the next call reads
    View st0;                                   // caller_sel: the view the caller's removal started from (caller_ok: cur is the compacted one)
    Held held;
    PairList pr;                                // prio_ok: the list the priority prune read
    PairList sk;                                // the list as the stage call put it (k_staged its k): what every prefix is derived from
    int k = 0, k_staged = 0;                    // k: the current list's
    int64_t n_sel = 0, n_caller = 0;            // the window's triangles of the caller's before / after the removal
    int64_t Tr = 0;                             // triangles the finish call kept
    Staged staged = UNSTAGED;
    int finished = 0, filtered = 0;             // the finish call's results (match, signs, weights) / its triangles hold
    int caller_sel = 0, caller_ok = 0;          // sel_tris valid; the window is the compacted one and caller_out its triangles
    int prio_ok = 0;                            // cur.list is a priority prune's
    int dd_ok = 0;                              // dd_tris holds the device's triangulation of the window's cells

    // ---- predicates: what the calls REQUIRE of the state (their arguments' checks stay with them) ---------------------------------
    bool is_staged() const { return staged >= STAGED_NO_PAIRS; }
    bool pairs_possible() const { return staged == STAGED; }
    bool may_prune() const { return is_staged() && !prio_ok && !caller_sel && !caller_ok && !filtered && !finished; }
    bool may_prefix(int k_) const { return is_staged() && k_ <= k_staged; }
    bool may_recost() const { return is_staged(); }
    bool may_select() const { return pairs_possible(); }
    bool may_push_pairs() const { return pairs_possible() && !filtered && !finished && !caller_ok && !caller_sel; }
    bool may_triangulate() const { return pairs_possible(); }
    bool may_finish_from(Source s) const { return (s == FROM_CALLER ? caller_ok : s == FROM_DEVICE ? dd_ok : 1) && pairs_possible(); }
    bool has_results() const { return finished && pairs_possible(); }
    bool has_triangles() const { return finished || filtered; }

    // THE PAIR LIST AS STAGED: the list before the priority prune filtered it and before the caller's removal took the unconstrained
    // nodes' rows (in that order: the prune's source is the older one); the window's own list where neither ran.  A k-NN prefix IS a
    // staged list (it resets both).  It is what SAME_WINDOW_STAGED_PAIRS hands out, and its reference rows (jsec, P of them) are the
    // frame the model's reference limits are read over: the frame is the prune's, src/same.py:1055-1085 does not compact the reference
    // side again.
    const PairList &as_staged() const { return prio_ok ? pr : caller_ok ? st0.list : cur.list; }

    // ---- transitions: each the one place that says what it invalidates ------------------------------------------------------------
    // what a finish call left holds no more
    void results_void() {
        filtered = finished = 0;
        Tr = 0;
    }
    // a stage call at k begins: nothing of the window's past holds (the call lays cur and sk out; staged is set with its counts)
    void begin_stage(int k_) {
        *this = State{};
        k = k_staged = k_;
    }
    // the window's pair list is `l`, as a stage call at k leaves it: nothing derived from an earlier list holds any more
    void staged_at(int k_, const PairList &l) {
        cur.list = l;
        k = k_;
        prio_ok = 0;
        pr = PairList{};
        results_void();
    }
    // a window the caller's removal compacted goes back to the view it started from, the caller's work HELD for caller_pairs; -> whether
    // it was turned back (its pinned block then holds the compacted counts, XY and rows: held.back_bytes of the staged ones are to come
    // back).  Selected but left as staged -- a cosine at the threshold --: nothing is held
    bool hold_caller() {
        const bool turned = caller_ok != 0;
        if (turned) {
            held.cs = cur;
            cur = st0;
            held.on = 1;
        }
        caller_sel = caller_ok = 0;
        return turned;
    }
    // the priority prune read `src` and left `left` of it
    void pruned(const PairList &src, const PairList &left) {
        pr = src;                               // the list as staged stays what as_staged() answers
        cur.list = left;
        prio_ok = 1;
    }
    // a caller_tris call begins: a second call (the host's mask) starts from the view the first started from; a selection held for a
    // k-NN prefix is overwritten (this call works from the list as it is)
    void restart_caller() {
        if (caller_ok) {
            cur = st0;
            results_void();                     // (they were the compacted window's: a cosine at the threshold now leaves the staged one)
        }
        caller_ok = caller_sel = 0;
        held = Held{};
        st0 = cur;
    }
    // the caller's triangles of the window are selected; the window itself is left as it was
    void selected(int64_t n) {
        n_sel = n;
        caller_sel = 1;
    }
    // the window is the compacted one: `v` without its unconstrained nodes, n_left of the caller's triangles left
    void compacted(const View &v, int64_t n_left) {
        cur = v;
        n_caller = n_left;
        caller_sel = caller_ok = 1;
        held.on = 0;
        dd_ok = 0;
        results_void();
    }
    void triangulated() { dd_ok = 1; }
    void finished_with(int64_t n_tris) {
        Tr = n_tris;
        filtered = finished = 1;
    }
};

}  // namespace win
