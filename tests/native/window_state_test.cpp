// window_state_test.cpp -- the window's state machine (same_amd/csrc/window_state.h) alone: no GPU, no HIP, no library.  The window calls
// are modelled as the library composes them from the transitions; views and lists carry distinct fake addresses that are never
// dereferenced.  Named call sequences against literal expectations, every sequence of up to five calls against the invariants, and every
// predicate against the boolean expression the calls used to spell out.  Built with -fsanitize=address,undefined by
// tests/test_window_state_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "window_state.h"

using namespace win;

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

namespace {

// the buffers a window's lists and views live in
enum Tag { NONE = 0, STAGE = 1, KPRE = 2, PRIO = 3, CALLER = 4 };

template <class T>
T *fake(int tag, int field) { return reinterpret_cast<T *>(static_cast<uintptr_t>(0x100000 * tag + 0x1000 * field + 0x40)); }

PairList list_in(Tag t, int64_t P) {
    PairList l;
    l.prow = fake<int32_t>(t, 1);
    l.pairs = fake<int32_t>(t, 2);
    l.jsec = fake<int32_t>(t, 3);
    l.cost64 = fake<double>(t, 4);
    l.P = P;
    return l;
}
View view_in(Tag t, int64_t n, int64_t P) {
    View v;
    v.counts = fake<unsigned long long>(t, 5);
    v.ua = fake<int32_t>(t, 6);
    v.rows_ua = fake<int32_t>(t, 7);
    v.type_c = fake<int32_t>(t, 8);
    v.axy_c = fake<double>(t, 9);
    v.size_c = fake<double>(t, 10);
    v.n_ua = n;
    v.list = list_in(t, P);
    return v;
}
bool same(const PairList &a, const PairList &b) {
    return a.prow == b.prow && a.pairs == b.pairs && a.jsec == b.jsec && a.cost64 == b.cost64 && a.P == b.P;
}
bool same(const View &a, const View &b) {
    return a.counts == b.counts && a.ua == b.ua && a.rows_ua == b.rows_ua && a.type_c == b.type_c && a.axy_c == b.axy_c &&
           a.size_c == b.size_c && a.n_ua == b.n_ua && same(a.list, b.list);
}
Tag where(const PairList &l) {
    for (Tag t : {STAGE, KPRE, PRIO, CALLER})
        if (l.prow == fake<int32_t>(t, 1)) return t;
    return NONE;
}
Tag where(const View &v) {
    for (Tag t : {STAGE, CALLER})
        if (v.counts == fake<unsigned long long>(t, 5)) return t;
    return NONE;
}

constexpr int K0 = 10, K1 = 5;                    // the staged k, a smaller one
constexpr int64_t N0 = 100, N1 = 90;              // kept cells as staged / after the caller's removal
constexpr int64_t P_SK = 1000, P_KPRE = 500;      // pairs of the staged list / of its prefix at K1

// ---- the calls, as the library composes them ---------------------------------------------------------------------------------
// same_window_stage: begin_stage, prepare_stage's layout, collect_stage's counts
void stage(State &s, int k) {
    s.begin_stage(k);
    s.cur = view_in(STAGE, 0, 0);
    s.sk = s.cur.list;
    s.cur.n_ua = N0;
    s.cur.list.P = s.sk.P = P_SK;
    s.staged = STAGED;
}
// same_window_priority_pairs: a tenth of the list goes
void prune(State &s) {
    CHECK(s.may_prune());
    const PairList src = s.cur.list;
    s.pruned(src, list_in(PRIO, src.P - src.P / 10));
}
// same_window_knn_prefix / same_window_recost (win::restage_batch); -> whether the window was turned back
bool prefix(State &s, int k) {
    CHECK(s.may_prefix(k));
    const bool turned = s.hold_caller();
    s.staged_at(k, k == s.k_staged ? s.sk : list_in(KPRE, P_KPRE));
    return turned;
}
bool recost(State &s) {
    CHECK(s.may_recost());
    const bool turned = s.hold_caller();
    s.staged_at(s.k_staged, s.sk);
    return turned;
}
// same_window_caller_tris, either form: `near` = a cosine at the threshold (the window is left as staged)
void caller(State &s, bool near) {
    CHECK(s.may_select());
    s.restart_caller();
    const View next = view_in(CALLER, N1, s.cur.list.P - s.cur.list.P / 10);
    s.selected(300);
    if (near) return;
    s.compacted(next, 250);
    s.held.valid = fake<uint8_t>(CALLER, 11);
    s.held.newidx = fake<int32_t>(CALLER, 12);
    s.held.st = fake<unsigned long long>(CALLER, 13);
    s.held.back_bytes = 64 + 20 * (size_t)N0;
    s.held.cap = P_SK;
}
// same_window_caller_pairs
bool may_push(const State &s) { return s.may_push_pairs() && s.held.on; }
void push_pairs(State &s) {
    CHECK(may_push(s));
    s.st0 = s.cur;
    View cs = s.held.cs;
    cs.list.P = s.cur.list.P - s.cur.list.P / 10;
    s.compacted(cs, s.n_caller);
}
// same_window_delaunay, answered
void delaunay(State &s) {
    CHECK(s.may_triangulate());
    s.dd_ok = 0;
    s.triangulated();
}
// same_window_filter_finish over the triangles the window has
Source source_of(const State &s) { return s.caller_ok ? FROM_CALLER : s.dd_ok ? FROM_DEVICE : FROM_HOST; }
void finish(State &s) {
    CHECK(s.may_finish_from(source_of(s)));
    s.results_void();
    s.finished_with(77);
}

struct Flags {
    int staged, finished, filtered, caller_sel, caller_ok, prio_ok, dd_ok, held_on;
};
#define EXPECT(s, view_, list_, as_staged_, k_, ...)             \
    do {                                                         \
        const Flags f_ = __VA_ARGS__;                            \
        CHECK(where((s).cur) == (view_));                        \
        CHECK(where((s).cur.list) == (list_));                   \
        CHECK(where((s).as_staged()) == (as_staged_));           \
        CHECK((s).k == (k_) && (s).k_staged == K0);              \
        CHECK((int)(s).staged == f_.staged);                     \
        CHECK((s).finished == f_.finished);                      \
        CHECK((s).filtered == f_.filtered);                      \
        CHECK((s).caller_sel == f_.caller_sel);                  \
        CHECK((s).caller_ok == f_.caller_ok);                    \
        CHECK((s).prio_ok == f_.prio_ok);                        \
        CHECK((s).dd_ok == f_.dd_ok);                            \
        CHECK((s).held.on == f_.held_on);                        \
    } while (0)

void named_sequences() {
    //                                                    staged fin filt sel ok prio dd held
    {   // stage -> prune -> prefix(k') -> prune
        State s;
        stage(s, K0);
        EXPECT(s, STAGE, STAGE, STAGE, K0, {2, 0, 0, 0, 0, 0, 0, 0});
        CHECK(s.cur.list.P == P_SK && s.cur.n_ua == N0);
        prune(s);
        EXPECT(s, STAGE, PRIO, STAGE, K0, {2, 0, 0, 0, 0, 1, 0, 0});
        CHECK(s.cur.list.P == 900 && s.as_staged().P == P_SK && !s.may_prune());
        CHECK(!prefix(s, K1));
        EXPECT(s, STAGE, KPRE, KPRE, K1, {2, 0, 0, 0, 0, 0, 0, 0});
        CHECK(s.pr.prow == nullptr && s.cur.list.P == P_KPRE);
        prune(s);
        EXPECT(s, STAGE, PRIO, KPRE, K1, {2, 0, 0, 0, 0, 1, 0, 0});
        CHECK(s.cur.list.P == 450 && s.as_staged().P == P_KPRE && same(s.sk, list_in(STAGE, P_SK)));
    }
    {   // stage -> device triangulation -> caller (compacted) -> prefix (held) -> push pairs -> finish -> prefix
        State s;
        stage(s, K0);
        delaunay(s);
        EXPECT(s, STAGE, STAGE, STAGE, K0, {2, 0, 0, 0, 0, 0, 1, 0});
        caller(s, false);
        EXPECT(s, CALLER, CALLER, STAGE, K0, {2, 0, 0, 1, 1, 0, 0, 0});
        CHECK(s.cur.n_ua == N1 && s.st0.n_ua == N0 && s.n_sel == 300 && s.n_caller == 250 && s.cur.list.P == 900 && !may_push(s));
        CHECK(prefix(s, K1));
        EXPECT(s, STAGE, KPRE, KPRE, K1, {2, 0, 0, 0, 0, 0, 0, 1});
        CHECK(s.cur.n_ua == N0 && where(s.held.cs) == CALLER && s.held.cs.n_ua == N1 && s.held.back_bytes == 2064 && s.n_caller == 250);
        CHECK(!s.may_finish_from(FROM_CALLER) && !s.may_finish_from(FROM_DEVICE) && s.may_finish_from(FROM_HOST));
        push_pairs(s);
        EXPECT(s, CALLER, CALLER, KPRE, K1, {2, 0, 0, 1, 1, 0, 0, 0});
        CHECK(s.cur.n_ua == N1 && s.cur.list.P == 450 && s.as_staged().P == P_KPRE && where(s.st0) == STAGE && s.n_sel == 300);
        finish(s);
        EXPECT(s, CALLER, CALLER, KPRE, K1, {2, 1, 1, 1, 1, 0, 0, 0});
        CHECK(s.Tr == 77 && s.has_results() && s.has_triangles() && !s.may_prune() && !s.may_push_pairs());
        CHECK(prefix(s, K0));
        EXPECT(s, STAGE, STAGE, STAGE, K0, {2, 0, 0, 0, 0, 0, 0, 1});
        CHECK(s.Tr == 0 && !s.has_results());
    }
    {   // stage -> caller (a cosine at the threshold: left as staged) -> caller with the host's mask -> caller again
        State s;
        stage(s, K0);
        caller(s, true);
        EXPECT(s, STAGE, STAGE, STAGE, K0, {2, 0, 0, 1, 0, 0, 0, 0});
        CHECK(s.n_sel == 300 && where(s.st0) == STAGE && !s.may_prune() && !s.may_finish_from(FROM_CALLER));
        caller(s, false);
        EXPECT(s, CALLER, CALLER, STAGE, K0, {2, 0, 0, 1, 1, 0, 0, 0});
        CHECK(where(s.st0) == STAGE && s.st0.n_ua == N0);
        caller(s, false);                         // from st0 again, not from the compacted view
        EXPECT(s, CALLER, CALLER, STAGE, K0, {2, 0, 0, 1, 1, 0, 0, 0});
        CHECK(where(s.st0) == STAGE && s.st0.n_ua == N0 && s.cur.list.P == 900);
        State left = s;
        caller(left, true);                       // a cosine at the threshold on the second go: the window as staged, nothing held
        EXPECT(left, STAGE, STAGE, STAGE, K0, {2, 0, 0, 1, 0, 0, 0, 0});
        CHECK(!prefix(left, K1) && !left.held.on);
    }
    {   // stage -> prune -> caller -> prefix -> prune -> push pairs
        State s;
        stage(s, K0);
        prune(s);
        caller(s, false);
        EXPECT(s, CALLER, CALLER, STAGE, K0, {2, 0, 0, 1, 1, 1, 0, 0});
        CHECK(where(s.st0.list) == PRIO && s.cur.list.P == 810 && s.as_staged().P == P_SK);
        CHECK(prefix(s, K1));
        EXPECT(s, STAGE, KPRE, KPRE, K1, {2, 0, 0, 0, 0, 0, 0, 1});
        prune(s);
        EXPECT(s, STAGE, PRIO, KPRE, K1, {2, 0, 0, 0, 0, 1, 0, 1});
        push_pairs(s);
        EXPECT(s, CALLER, CALLER, KPRE, K1, {2, 0, 0, 1, 1, 1, 0, 0});
        CHECK(where(s.st0.list) == PRIO && s.cur.list.P == 405 && s.as_staged().P == P_KPRE);
    }
    {   // stage -> caller -> recost -> push pairs
        State s;
        stage(s, K0);
        caller(s, false);
        CHECK(recost(s));
        EXPECT(s, STAGE, STAGE, STAGE, K0, {2, 0, 0, 0, 0, 0, 0, 1});
        CHECK(same(s.cur.list, s.sk));
        push_pairs(s);
        EXPECT(s, CALLER, CALLER, STAGE, K0, {2, 0, 0, 1, 1, 0, 0, 0});
        CHECK(s.cur.list.P == 900 && s.cur.n_ua == N1);
    }
    {   // prefix at k_staged: turned back to sk, no derived list
        State s;
        stage(s, K0);
        prefix(s, K1);
        prune(s);
        CHECK(!prefix(s, K0));
        EXPECT(s, STAGE, STAGE, STAGE, K0, {2, 0, 0, 0, 0, 0, 0, 0});
        CHECK(same(s.cur.list, s.sk) && s.pr.prow == nullptr && !s.may_prefix(K0 + 1));
    }
    {   // stage of a window that was compacted and held: everything cleared
        State s;
        stage(s, K0);
        prune(s);
        delaunay(s);
        caller(s, false);
        finish(s);
        prefix(s, K1);
        CHECK(s.held.on);
        s.begin_stage(7);
        CHECK(s.staged == UNSTAGED && !s.is_staged() && s.k == 7 && s.k_staged == 7);
        CHECK(!s.finished && !s.filtered && !s.caller_sel && !s.caller_ok && !s.prio_ok && !s.dd_ok && !s.held.on);
        CHECK(s.Tr == 0 && s.n_sel == 0 && s.n_caller == 0 && s.held.cap == 0 && s.held.back_bytes == 0 && !s.held.valid && !s.held.newidx && !s.held.st);
        for (const View *v : {&s.cur, &s.st0, &s.held.cs}) CHECK(same(*v, View{}));
        for (const PairList *l : {&s.pr, &s.sk}) CHECK(same(*l, PairList{}));
    }
}

// ---- every sequence of up to five calls --------------------------------------------------------------------------------------
struct Walk {
    State s;
    PairList at_finish;          // the list the finish call's results are of
    View view_at_finish;
};
long walked = 0;

void invariants(const Walk &w) {
    const State &s = w.s;
    CHECK(!s.held.on || (!s.caller_ok && !s.caller_sel));
    CHECK(!s.caller_ok || s.caller_sel);
    if (s.finished) CHECK(same(s.cur.list, w.at_finish) && same(s.cur, w.view_at_finish) && s.filtered && s.Tr == 77);
    else CHECK(!s.filtered && s.Tr == 0);
    const PairList &want = s.prio_ok ? s.pr : s.caller_ok ? s.st0.list : s.cur.list;
    CHECK(same(s.as_staged(), want));
    CHECK(where(s.cur) == STAGE || where(s.cur) == CALLER);
    CHECK((where(s.cur) == CALLER) == (s.caller_ok != 0));
    CHECK(where(s.cur.list) != NONE);
    CHECK((where(s.cur.list) == CALLER) == (s.caller_ok != 0));          // the compacted view's arrays hold the compacted / pushed list only
    CHECK(same(s.sk, list_in(STAGE, P_SK)) && s.k_staged == K0 && s.staged == STAGED);
    CHECK(where(s.as_staged()) == (s.k == K0 ? STAGE : KPRE));           // the list as staged is the staged list at the current k
    CHECK(s.as_staged().P == (s.k == K0 ? P_SK : P_KPRE));
    if (s.prio_ok) CHECK(where(s.pr) != NONE); else CHECK(s.pr.prow == nullptr);
    if (s.caller_sel) CHECK(where(s.st0) == STAGE && s.st0.n_ua == N0);
    if (s.held.on) CHECK(where(s.held.cs) == CALLER && s.held.cs.n_ua == N1 && s.held.valid && s.held.newidx && s.held.cap == P_SK && s.n_caller == 250);
    CHECK(s.cur.n_ua == (s.caller_ok ? N1 : N0));
}

void walk(const Walk &from, int depth) {
    if (depth == 0) return;
    for (int t = 0; t < 9; ++t) {
        Walk w = from;
        State &s = w.s;
        switch (t) {
        case 0: if (!s.may_prune()) continue; prune(s); break;
        case 1: if (!s.may_prefix(K1)) continue; prefix(s, K1); break;
        case 2: if (!s.may_prefix(K0)) continue; prefix(s, K0); break;
        case 3: if (!s.may_recost()) continue; recost(s); break;
        case 4: if (!s.may_select()) continue; caller(s, false); break;
        case 5: if (!s.may_select()) continue; caller(s, true); break;
        case 6: if (!may_push(s)) continue; push_pairs(s); break;
        case 7: if (!s.may_triangulate()) continue; delaunay(s); break;
        default:
            if (!s.may_finish_from(source_of(s))) continue;
            finish(s);
            w.at_finish = s.cur.list;
            w.view_at_finish = s.cur;
        }
        ++walked;
        invariants(w);
        walk(w, depth - 1);
    }
}

// ---- every predicate against the expression the calls spelled out -------------------------------------------------------------
void truth_table() {
    const PairList a = list_in(STAGE, 1), b = list_in(PRIO, 2), c = list_in(KPRE, 3);
    for (int st = 0; st < 3; ++st)
        for (int bits = 0; bits < 128; ++bits) {
            State s;
            s.staged = (Staged)st;
            const int staged = st, finished = bits & 1, filtered = bits >> 1 & 1, caller_sel = bits >> 2 & 1, caller_ok = bits >> 3 & 1,
                      prio_ok = bits >> 4 & 1, dd_ok = bits >> 5 & 1, held_on = bits >> 6 & 1;
            s.finished = finished; s.filtered = filtered; s.caller_sel = caller_sel; s.caller_ok = caller_ok;
            s.prio_ok = prio_ok; s.dd_ok = dd_ok; s.held.on = held_on;
            s.k_staged = K0;
            s.cur.list = a; s.pr = b; s.st0.list = c;
            CHECK(s.is_staged() == (staged >= 1));
            CHECK(s.pairs_possible() == (staged == 2));
            CHECK(s.may_prune() == (staged >= 1 && (!prio_ok && !caller_sel && !caller_ok && !filtered && !finished)));
            for (int k : {K0 - 1, K0, K0 + 1}) CHECK(s.may_prefix(k) == (staged >= 1 && k <= K0));
            CHECK(s.may_recost() == (staged >= 1));
            CHECK(s.may_select() == (staged == 2));
            CHECK(s.may_push_pairs() == (staged == 2 && !filtered && !finished && !caller_ok && !caller_sel));
            CHECK(s.may_triangulate() == (staged == 2));
            CHECK(s.may_finish_from(FROM_HOST) == (staged == 2));
            CHECK(s.may_finish_from(FROM_DEVICE) == (dd_ok && staged == 2));
            CHECK(s.may_finish_from(FROM_CALLER) == (caller_ok && staged == 2));
            CHECK(s.has_results() == (finished && staged == 2));
            CHECK(s.has_triangles() == (finished || filtered));
            CHECK(same(s.as_staged(), prio_ok ? b : caller_ok ? c : a));
        }
}

}  // namespace

int main() {
    named_sequences();
    Walk w;
    stage(w.s, K0);
    invariants(w);
    walk(w, 5);
    CHECK(walked > 1000);
    truth_table();
    std::printf("%ld states walked\nok\n", walked);
    return 0;
}
