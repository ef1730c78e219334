"""The window merge calls (csrc/window_merge.hip: same_window_collect, same_merge_acc_begin / load / resolve / finish / plain / fetch /
columns / columns_layer, same_section_set_codes; csrc/merge.hip's de-duplication behind resolve) driven at the LIBRARY (W.MergeAccumulator,
W.resolve_accumulators, W.plain_accumulators, DeviceSection.set_codes) against the plain host statement of tests/merge_check.py -- on
row families sized to a scan block's, a sort block's and a look-back window's edge, with duplicate pairs every key of which decides in
turn, flag bytes that differ in bit 1 alone, window ids up to 2^31 - 1, codes far sparser than rows, two probe chains that wrap past the
pair table's end; on windows whose cells lie exactly on a trim edge, calls of up to 23 windows, accumulators that grow with rows in
place, a compacted view, several accumulators laid end to end, id codes, hand-made seams; the table's columns as bit patterns; and the
calls' refusals.  Every comparison is exact equality of integer arrays or bit patterns.  tests/test_merge_check_cpu.py proves without
a GPU that each input has the property its case is about and that a kernel wrong in one of eleven ways would give another answer."""
import numpy as np
import pytest

import caller_check as C
import merge_check as K

pytestmark = pytest.mark.gpu

_SECTIONS, _WINDOWS, _HELD = {}, {}, {}


def _W():
    from same_amd import windows as W

    return W


def _sections(case, types=None):
    """(moving DeviceSection, reference DeviceSection) of a case, uploaded once (`types`: the moving side's type columns, default the case's)"""
    key = (id(case), None if types is None else types.shape[1])
    if key not in _SECTIONS:
        W = _W()
        tm = case.get("types_m", case.get("types")) if types is None else types
        tr = case["types_r"][:, :tm.shape[1]]
        mov = W.Section(case["mov_xy"], np.ascontiguousarray(tm), case.get("type_id"), case.get("size"))
        ref = W.Section(case["ref_xy"], np.ascontiguousarray(tr), None, None)
        _SECTIONS[key] = (W.DeviceSection(mov), W.DeviceSection(ref), case)
    return _SECTIONS[key][:2]


def _finished(st, dmov, dref, case, box, seed=0):
    """stage the window and finish it with a shuffled triangulation of its kept cells -> its pair list"""
    W = _W()
    counts = st.stage(dmov, dref, box, case.get("radius", C.RADIUS), case.get("k", C.KNN), 1.0)
    assert counts[2] >= 3
    xy = st.fetch(W._W_ALIGNED_XY)
    st.finish(C.shuffled_triangulation(xy, np.random.default_rng(seed)), K.PENALTY)
    return st.fetch(W._W_PAIRS)


def _window(tag):
    """a finished window of tests/merge_check.WINDOWS (made once) -> dict(st, case, box, pairs, dmov, dref)"""
    if tag not in _WINDOWS:
        W = _W()
        case, box = K.window_of(tag)
        dmov, dref = _sections(case)
        st = W.DeviceWindow()
        _WINDOWS[tag] = dict(st=st, case=case, box=box, pairs=_finished(st, dmov, dref, case, box), dmov=dmov, dref=dref, tag=tag)
    return _WINDOWS[tag]


def _pool():
    """23 finished windows of very different sizes: the seven of WINDOWS (the 16 385-cell one third) and sixteen boxes of the base case"""
    W = _W()
    tags = ["edge/255", "zero", "edge/16385", "edge/256", "base/interior", "edge/257", "base/sliver"]
    out = [_window(t) for t in tags]
    if "pool" not in _WINDOWS:
        rng = np.random.default_rng(2323)
        case = C.base_case()
        dmov, dref = _sections(case)
        more = []
        for q in range(16):
            x0, y0 = rng.uniform(0, 170, 2)
            box = (float(x0), float(x0 + rng.uniform(20, 120)), float(y0), float(y0 + rng.uniform(20, 120)))
            st = W.DeviceWindow()
            more.append(dict(st=st, case=case, box=box, pairs=_finished(st, dmov, dref, case, box, seed=q), dmov=dmov, dref=dref, tag=f"pool/{q}"))
        _WINDOWS["pool"] = more
    return out + _WINDOWS["pool"]


def _view(w, name, mp=None):
    """put the matching `name` on the finished window (same_window_refinish) -> its current view: what collect reads"""
    W = _W()
    st = w["st"]
    rows, xy = st.fetch(W._W_ALIGNED_ROWS), st.fetch(W._W_ALIGNED_XY)
    mp = K.matching(name, w["pairs"], xy) if mp is None else mp
    match_row, flag, _stats = st.refinish(mp, K.PENALTY)
    return dict(rows=rows, xy=xy, match_row=match_row, flag=flag)


def _collect(acc, call):
    """one same_window_collect call; call = [(window, view, trim, window id, plan position)] -> the statement's rows of the call"""
    acc.collect([c[0]["st"] for c in call], [c[2] for c in call], [c[3] for c in call], [c[4] for c in call])
    return np.concatenate([K.collect_rows(c[1]["rows"], c[1]["xy"], c[1]["match_row"], c[1]["flag"], c[2], c[3], c[4]) for c in call])


def _same(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (tag, next(q for q in range(len(got)) if got[q] != want[q]))


def _plain_is(accs, rows, tag):
    W = _W()
    acc = W.plain_accumulators(accs)
    assert acc is accs[0] and acc.n_final == len(rows), (tag, acc.n_final, len(rows))
    _same(acc.final_rows(), K.plain(rows), tag)


def _resolve_is(accs, want, dmov, dref, tag):
    """resolve -> counts and REST; finish without winners -> the rows final already; finish with the host's winners -> FINAL"""
    W = _W()
    counts, rest = W.resolve_accumulators(accs, dmov, dref)
    print(tag, counts)
    assert counts == want["counts"], (tag, counts, want["counts"])
    _same(rest, want["rest"], (tag, "rest"))
    _same(accs[0].finish(np.zeros(0, np.int32)), K.finish(want, []), (tag, "no winners"))
    won = K.winners(rest)
    final = accs[0].finish(won)
    _same(final, K.finish(want, won), (tag, "final"))
    return final


def _acc():
    if "acc" not in _HELD:
        _HELD["acc"] = _W().MergeAccumulator()
    return _HELD["acc"]


def _load_is(acc, fam, tag):
    acc.load(fam["a"], fam["r"], fam["flags"], fam["wid"], fam["pos"], fam["cidx"], fam["n_codes_a"], fam["n_codes_r"])
    return _resolve_is([acc], K.resolve_family(fam), None, None, tag)


# ---- the load path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", K.LOAD_CASES)
def test_loaded_rows_resolve_and_finish_as_the_statement(name, n):
    """Every row family at every size it takes: load -> resolve -> finish.  The four counts, the REST records in the de-duplication's
    order and the FINAL records are the statement's; finishing without winners gives exactly the rows that were final already.  One
    accumulator serves all cases, in whatever order they run."""
    final = _load_is(_acc(), K.family(name, n), (name, n))
    if name in ("alone", "one pair", "keys", "flag bits", "wid extremes"):
        assert len(final) == (min(n, 1) if name == "one pair" else n if name == "alone" else len(np.unique(K.family(name, n)["pair"])))


def test_one_accumulator_through_passes_of_every_kind():
    """largest, 0, 1, the largest of another family, sparse codes, a small one -- loaded passes alternating with collected ones (with
    seams, with all_seam, plain) on ONE accumulator: every pass gives its own answer, nothing of the pass before survives."""
    W = _W()
    acc = W.MergeAccumulator()
    seam = K.seam_case()
    w = dict(case=seam, box=seam["box"], st=W.DeviceWindow())
    w["dmov"], w["dref"] = _sections(seam)
    w["pairs"] = _finished(w["st"], w["dmov"], w["dref"], seam, seam["box"])
    view = _view(w, "all first candidate")
    n = len(seam["mov_xy"])
    trims = K.seam_trims()
    passes = [("load", "stars and chains", 16385), ("collect", dict(near=True, reach=K.SEAM_REACH)), ("load", "alone", 0),
              ("collect", dict(all_seam=True)), ("load", "one pair", 1), ("collect", dict(plain=True)), ("load", "keys", 16385),
              ("collect", dict(near=True, reach=0.0)), ("load", "sparse codes", 257), ("collect", dict()), ("load", "alone", 255)]
    try:
        for q, p in enumerate(passes):
            if p[0] == "load":
                _load_is(acc, K.family(p[1], p[2]), (q,) + p)
                continue
            how = p[1]
            near = (seam["near_start"], seam["near_boxes"]) if how.get("near") else None
            acc.begin(n, near, how.get("reach", 0.0), how.get("all_seam", False))
            rows = np.concatenate([_collect(acc, [(w, view, trims[b], b, K.SEAM_POS[b])]) for b in range(K.SEAM_BANDS)])      # (a window once per call)
            assert len(rows) == n
            if how.get("plain"):
                _plain_is([acc], rows, q)
                continue
            seams = "all" if how.get("all_seam") else (seam["near_start"], seam["near_boxes"], how["reach"], seam["mov_xy"], seam["ref_xy"]) if near else None
            want = K.resolve(rows, None, None, n, n, seams)
            assert want["counts"][2] == (n if how.get("all_seam") else 0 if near is None else want["counts"][2])
            _resolve_is([acc], want, w["dmov"], w["dref"], (q, "collect", sorted(how)))
    finally:
        acc.close()
        w["st"].close()


# ---- the collect path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", K.WINDOWS)
def test_collect_of_one_window_is_the_statement(tag):
    """Every window family under every matching and every trim it can take: begin, collect, plain -> collect_rows' records."""
    w = _window(tag)
    acc = _acc()
    seen = 0
    for name in K.MATCHINGS:
        view = _view(w, name)
        for q, kind in enumerate(K.TRIMS):
            trim = K.trim_of(kind, w["box"], view["xy"])
            if trim is None:
                continue
            acc.begin(len(view["rows"]))
            rows = _collect(acc, [(w, view, trim, 7 + q, q - 1)])
            _plain_is([acc], rows, (tag, name, kind))
            seen += len(rows)
            if name == "all first candidate" and kind == "whole":
                assert len(rows) == len(view["rows"]) and (tag[:5] != "edge/" or len(rows) == int(tag[5:]))
    assert seen > 0


def _pool_calls(n_windows, n_calls):
    """the first `n_windows` windows of the pool under cycling matchings and trims, split into `n_calls` collect calls"""
    pool = _pool()[:n_windows]
    items = []
    for q, w in enumerate(pool):
        view = _view(w, "all first candidate" if w["tag"] == "edge/16385" else K.MATCHINGS[(q + 1) % 4])
        kinds = [k for k in K.TRIMS if K.trim_of(k, w["box"], view["xy"]) is not None]
        kind = "whole" if w["tag"] == "edge/16385" else kinds[(3 * q) % len(kinds)]
        items.append((w, view, K.trim_of(kind, w["box"], view["xy"]), 100 + q, q))
    cuts = np.linspace(0, n_windows, n_calls + 1).astype(int)
    return [items[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


@pytest.mark.parametrize("n_calls", [1, 2, 3])
@pytest.mark.parametrize("n_windows", [1, 8, 9, 17, 23])
def test_collect_of_many_windows(n_windows, n_calls):
    """1, 8, 9, 17 and 23 windows (launch groups of eight) in one, two and three calls into one accumulator: windows of 43 to 16 385
    cells, some of which give no row for their matching or their trim, the 16 385-cell window among 255-cell ones -- the rows are
    collect_rows' of the windows, in call order."""
    if n_calls > n_windows:
        n_calls = n_windows
    calls = _pool_calls(n_windows, n_calls)
    acc = _acc()
    acc.begin(sum(len(c[1]["rows"]) for call in calls for c in call))
    rows = np.concatenate([_collect(acc, call) for call in calls])
    if n_windows >= 8:
        per = [len(K.collect_rows(c[1]["rows"], c[1]["xy"], c[1]["match_row"], c[1]["flag"], c[2], 0, 0)) for call in calls for c in call]
        assert min(per) == 0 and max(per) >= 16385 and len(set(per)) >= 4
    _plain_is([acc], rows, (n_windows, n_calls))


@pytest.mark.parametrize("expected", [0, 1])
def test_a_second_collect_grows_the_arrays_with_rows_in_place(expected):
    """begun for 0 / 1 rows: the first collect allocates, the second finds the arrays too small with the first call's rows in them
    (reserve_rows with have > 0): they move along."""
    W = _W()
    acc = W.MergeAccumulator()              # a fresh one: its arrays start at nothing
    try:
        small, large = _window("edge/255"), _window("edge/16385")
        acc.begin(expected)
        rows = [_collect(acc, [(small, _view(small, "all first candidate"), small["box"], 1, 0)])]
        rows.append(_collect(acc, [(large, _view(large, "every second cell"), large["box"], 2, 1)]))
        assert len(rows[0]) == 255 and len(rows[1]) == 8193 > 4096 * 1.25          # past the first allocation's 4096 + slack
        _plain_is([acc], np.concatenate(rows), expected)
    finally:
        acc.close()


def test_collect_reads_the_view_a_callers_compaction_left(oracle):
    """A window whose unconstrained nodes same_window_caller_tris removed (the host's mask, as tests/test_gpu_window_front_calls.py makes
    it) before its finish: cidx and a_row are those of the compacted view."""
    W = _W()
    from same_amd.triangles import cos_threshold

    case = C.base_case()
    mov = W.Section(case["mov_xy"], case["types_m"], case["type_id"], case["size"])
    ref = W.Section(case["ref_xy"], case["types_r"], None, None)
    dmov, dref = W.DeviceSection(mov), W.DeviceSection(ref)
    grid = C.GRIDS["cell 25"]
    dmov.bin(*grid)
    dref.bin(*grid)
    caller = W.DeviceCallerTris(dmov, case["tris"])
    st = W.DeviceWindow()
    acc = _acc()
    try:
        box = (100.0, 200.0, 100.0, 200.0)
        st.stage(dmov, dref, box, C.RADIUS, C.KNN, 1.0)
        staged = dict(rows=st.fetch(W._W_ALIGNED_ROWS), xy=st.fetch(W._W_ALIGNED_XY), pairs=st.fetch(W._W_PAIRS), costs=st.fetch(W._W_COSTS))
        _sel, valid, n_left, _p2, _c2, _t2 = C.window_statement(staged["rows"], case["tris"], staged["xy"], case["type_id"][staged["rows"]],
                                                                staged["pairs"].astype(np.int64), staged["costs"], C.RADIUS, 15, True, oracle)
        en, thr = cos_threshold(15)
        args = (C.RADIUS, en, thr, float(8 * np.spacing(abs(thr))), True)
        got = W.caller_tris_windows([st], caller, *args, removed=[(~valid).astype(np.uint8)])[0]
        assert got[1] == int((~valid).sum()) > 0 and got[3] == n_left
        _k, _a, near, _row, _flag, _stats = W.filter_finish_windows([st], None, *args, K.PENALTY, from_caller=True)[0]
        assert near == 0
        w = dict(st=st, pairs=st.fetch(W._W_PAIRS))
        for name in ("all first candidate", "every second cell"):
            view = _view(w, name)
            assert np.array_equal(view["rows"], staged["rows"][valid]) and len(view["rows"]) == n_left
            acc.begin(n_left)
            rows = _collect(acc, [(w, view, box, 4, 2)])
            assert len(rows) and np.array_equal(view["rows"][rows["cidx"]], rows["a_row"])
            assert not np.array_equal(staged["rows"][rows["cidx"]], rows["a_row"])        # (the staged view's numbers are others)
            _plain_is([acc], rows, name)
    finally:
        caller.close()
        st.close()
        dref.close()
        dmov.close()


EMPTY_PATTERNS = {2: ("rows rows", "empty rows", "rows empty", "empty empty"),
                  3: ("rows rows rows", "empty rows rows", "rows empty rows", "rows rows empty", "empty empty rows", "empty empty empty")}


@pytest.mark.parametrize("n_accs", [2, 3])
def test_accumulators_are_laid_end_to_end_in_list_order(n_accs):
    """Two and three accumulators of one context handed to resolve and to plain: the first empty, a middle one empty, all empty -- the
    rows are the accumulators' rows in list order.  The windows are boxes of ONE section pair that overlap, under different matchings:
    duplicate pairs and contested cells across the accumulators."""
    W = _W()
    pool = [w for w in _pool() if w["case"] is C.base_case()]
    dmov, dref = pool[0]["dmov"], pool[0]["dref"]
    n_sec = len(C.base_case()["mov_xy"])
    accs = [W.MergeAccumulator() for _ in range(n_accs)]
    try:
        for pattern in EMPTY_PATTERNS[n_accs]:
            for how in ("plain", "resolve"):
                rows, at = [], 0
                for acc, kind in zip(accs, pattern.split()):
                    acc.begin(0 if kind == "empty" else 64)
                    if kind == "rows":
                        for _call in range(2):
                            w = pool[at % len(pool)]
                            view = _view(w, ("all first candidate", "last candidate", "every second cell")[at % 3])
                            rows.append(_collect(acc, [(w, view, w["box"], 50 - at, at)]))
                            at += 1
                rows = np.concatenate(rows) if rows else np.zeros(0, K.ROWS)
                if how == "plain":
                    _plain_is(accs, rows, (pattern, how))
                else:
                    want = K.resolve(rows, None, None, n_sec, n_sec, None)
                    _resolve_is(accs, want, dmov, dref, (pattern, how))
                    if "rows" in pattern:
                        assert want["counts"][1] < want["counts"][0] or want["counts"][2] > 0
    finally:
        for acc in accs:
            acc.close()


# ---- the resolve path with sections ----------------------------------------------------------------------------------------------------
def test_resolve_follows_the_sections_id_codes():
    """same_section_set_codes on both sections: a permutation (the final order follows the code, not the row); fewer codes than rows,
    two rows sharing a code (contested); None; set, then set back to None."""
    W = _W()
    w = _window("zero")
    dmov, dref, n = w["dmov"], w["dref"], len(w["case"]["mov_xy"])
    rng = np.random.default_rng(11)
    acc = _acc()
    shared = np.arange(n)
    shared[n // 2 + 1:] -= 1                      # rows n // 2 and n // 2 + 1 share a code: n - 1 codes
    cases = [("permutation", rng.permutation(n), rng.permutation(n), n), ("shared", shared, shared[::-1].copy(), n - 1), ("none", None, None, n),
             ("permutation again", rng.permutation(n), rng.permutation(n), n), ("back to none", None, None, n)]
    try:
        for tag, ca, cr, n_codes in cases:
            dmov.set_codes(ca, n_codes)
            dref.set_codes(cr, n_codes)
            acc.begin(2 * n)
            view = _view(w, "all first candidate")
            rows = [_collect(acc, [(w, view, w["box"], 3, 0)])]
            view = _view(w, "last candidate")
            rows.append(_collect(acc, [(w, view, w["box"], 1, 1)]))
            rows = np.concatenate(rows)
            want = K.resolve(rows, ca, cr, n_codes, n_codes, None)
            final = _resolve_is([acc], want, dmov, dref, tag)
            assert want["counts"][2] > 0 and len(final) > 0
            if ca is not None and tag != "shared":
                assert np.all(np.diff(ca[final["a_row"]]) > 0) and not np.all(np.diff(final["a_row"]) > 0)
    finally:
        dmov.set_codes(None, n)
        dref.set_codes(None, n)


@pytest.mark.parametrize("contested", [False, True])
def test_seams_are_the_statements(contested):
    """Hand-made (near_start, near_boxes) over the seam lattice, collected band by band: an aligned cell on x0 and on x1, references
    exactly `reach` outside a box and one nextafter further, reach 0, a position with an empty range, positions -1 and n_pos, all_seam
    -- alone, and combined with contested rows: every second band collected a second time under a larger window id (duplicates, the first
    copy of which survives) and reference codes that bands 0 and 1 share column by column (their rows are contested, at a seam or not)."""
    W = _W()
    seam = K.seam_case()
    w = dict(case=seam, box=seam["box"], st=W.DeviceWindow())
    w["dmov"], w["dref"] = _sections(seam)
    acc = _acc()
    n = len(seam["mov_xy"])
    codes_r = None
    if contested:
        codes_r = np.arange(n)
        codes_r[1::K.SEAM_BANDS] = codes_r[0::K.SEAM_BANDS]
    try:
        w["dref"].set_codes(codes_r, n)
        w["pairs"] = _finished(w["st"], w["dmov"], w["dref"], seam, seam["box"])
        assert len(w["pairs"]) == n
        view = _view(w, "all first candidate")
        assert np.array_equal(view["match_row"], np.arange(n))
        trims = K.seam_trims()
        for reach, all_seam in ((0.0, False), (K.SEAM_REACH, False), (K.SEAM_REACH, True)):
            acc.begin(n, (seam["near_start"], seam["near_boxes"]), reach, all_seam)
            rows = [_collect(acc, [(w, view, trims[b], b, K.SEAM_POS[b])]) for b in range(K.SEAM_BANDS)]                       # (a window once per call)
            if contested:
                rows += [_collect(acc, [(w, view, trims[b], 10 + b, K.SEAM_POS[b])]) for b in range(0, K.SEAM_BANDS, 2)]
            rows = np.concatenate(rows)
            seams = "all" if all_seam else (seam["near_start"], seam["near_boxes"], reach, seam["mov_xy"], seam["ref_xy"])
            want = K.resolve(rows, None, codes_r, n, n, seams)
            _resolve_is([acc], want, w["dmov"], w["dref"], (reach, all_seam, contested))
            flags = want["rest"]["flags"]
            if all_seam:
                assert want["counts"][1:] == (n, n, 0) and (flags & 4 == 4).all()
            elif contested:
                assert want["counts"][0] > n == want["counts"][1] and 0 < np.count_nonzero(flags & 4) < len(flags) < n
            else:
                assert 0 < np.count_nonzero(flags & 4) == len(flags) < n
    finally:
        w["dref"].set_codes(None, n)
        w["st"].close()


# ---- the columns -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 1, 3])
def test_columns_are_the_statements_bit_for_bit(T):
    """After finish and after plain, T type columns, no and four extra columns per side, 1 / 7 / 255 / 256 / 257 final rows, with and
    without a types layer: the pooled pinned block's two arrays equal the statement's, bit for bit -- NaN payloads, -0.0, infinities,
    denormals and negative int64 ids among the values."""
    from same_amd import _lib

    W = _W()
    case = K.columns_case()
    dmov, dref = _sections(case, case["types"][:, :T])
    layer = W.DeviceTypesLayer(dmov, case["layer"][:, :T])
    ctx = dmov.ctx
    extra = [_lib.DeviceBuffer(ctx, case["extra"][q].nbytes).upload(case["extra"][q]) for q in range(8)]
    w = dict(st=W.DeviceWindow(), case=case, box=case["box"])
    acc = _acc()
    n_sec = len(case["mov_xy"])
    try:
        assert W.PINNED_BLOCKS.out == 0
        w["pairs"] = _finished(w["st"], dmov, dref, case, case["box"])
        rows_r = w["st"].fetch(W._W_ROWS_R)
        view = _view(w, None, K.own_matching(w["pairs"], w["st"].fetch(W._W_ALIGNED_ROWS), rows_r))
        assert np.array_equal(view["match_row"], view["rows"]) and len(view["rows"]) == n_sec
        for n in K.COLUMN_ROWS:
            for how in ("finish", "plain"):
                acc.begin(n)
                rows = _collect(acc, [(w, view, K.trim_for(n, case["box"], view["xy"]), 9, 3)])
                assert len(rows) == n
                if how == "plain":
                    W.plain_accumulators([acc])
                    final = K.plain(rows)
                else:
                    want = K.resolve(rows, None, None, n_sec, n_sec, None)
                    final = _resolve_is([acc], want, dmov, dref, (T, n, how))
                assert acc.n_final == n == len(final)
                for use_layer in (False, True):
                    for n_extra in (0, 4):
                        em, er = extra[:n_extra], extra[4:4 + n_extra]
                        got = acc.columns(dmov, dref, n, T, em, er, layer=layer if use_layer else None)
                        assert got is not None
                        ctx.sync()
                        types = (case["layer"] if use_layer else case["types"])[:, :T]
                        wide, flags = K.columns(final, types, case["mov_xy"], case["ref_xy"], [case["extra"][q] for q in range(n_extra)],
                                                [case["extra"][4 + q] for q in range(n_extra)])
                        assert got[0].shape == wide.shape == (T + 4 + 2 * n_extra + 3, n) and got[1].shape == flags.shape == (2, n)
                        assert np.array_equal(got[0], wide), (T, n, how, use_layer, n_extra)
                        assert np.array_equal(got[1], flags), (T, n, how, use_layer, n_extra)
                        del got                                   # the last arrays over the block: it goes back to the pool
                        assert W.PINNED_BLOCKS.out == 0
    finally:
        for b in extra:
            b.free()
        layer.close()
        w["st"].close()


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(code, call, *args, **kw):
    """the call raises with `code`; a pinned block a refused columns call took is back in the pool (the raised error's frames held it)"""
    import gc

    from same_amd import _lib

    with pytest.raises(_lib.SameHipError) as e:
        call(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    del e
    if _W().PINNED_BLOCKS.out:
        gc.collect()
    assert _W().PINNED_BLOCKS.out == 0


def test_refusals_leave_the_accumulator_usable():
    """Every refusal the code states comes back as SAME_EINVAL / SAME_ERANGE; after each group the same accumulator runs a full pass
    that equals the statement."""
    from same_amd import _lib

    W = _W()
    EINVAL, ERANGE = _lib.SAME_EINVAL, _lib.SAME_ERANGE
    w = _window("zero")
    dmov, dref, n = w["dmov"], w["dref"], len(w["case"]["mov_xy"])
    acc, other = W.MergeAccumulator(), W.MergeAccumulator()
    fam = K.family("probe chain", K.PROBE_ROWS)
    lib, ctx = acc.ctx.lib, acc.ctx
    other_ctx = _lib.Context(ctx.device)
    foreign, unfinished = W.DeviceWindow(other_ctx), W.DeviceWindow()
    box = w["box"]

    def full_pass(tag):
        _load_is(acc, fam, (tag, "loaded pass"))
        acc.begin(n)
        view = _view(w, "all first candidate")
        rows = np.concatenate((_collect(acc, [(w, view, box, 2, 0)]), _collect(acc, [(w, _view(w, "last candidate"), box, 1, 1)])))
        return _resolve_is([acc], K.resolve(rows, None, None, n, n, None), dmov, dref, (tag, "collected pass"))

    try:
        view = _view(w, "all first candidate")
        one = ([w["st"]], [box], [0], [0])
        # collect
        acc.begin(n)
        _refused(EINVAL, acc.collect, [w["st"]], [box], [-1], [0])                         # a negative window id
        unfinished.stage(dmov, dref, box, C.RADIUS, C.KNN, 1.0)
        _refused(EINVAL, acc.collect, [unfinished], [box], [0], [0])                       # staged, not finished
        omov, oref = (W.DeviceSection(s.section, ctx=other_ctx) for s in (dmov, dref))
        try:
            foreign.stage(omov, oref, box, C.RADIUS, C.KNN, 1.0)
            foreign.finish(C.shuffled_triangulation(foreign.fetch(W._W_ALIGNED_XY), np.random.default_rng(0)), K.PENALTY)
            _refused(EINVAL, acc.collect, [foreign], [box], [0], [0])                      # a window of another context
        finally:
            foreign.close()
            oref.close()
            omov.close()
        rows = _collect(acc, [(w, view, box, 0, 0)])
        _refused(EINVAL, acc.finish, np.zeros(0, np.int32))                                # finish before resolve
        _refused(EINVAL, acc.columns, dmov, dref, len(rows), 3)                            # columns before resolve
        _refused(EINVAL, W.resolve_accumulators, [acc, acc], dmov, dref)                   # one accumulator twice in a list
        _refused(EINVAL, W.plain_accumulators, [acc, acc])
        want = K.resolve(rows, None, None, n, n, None)
        counts, rest = W.resolve_accumulators([acc], dmov, dref)
        assert counts == want["counts"]
        _refused(EINVAL, acc.collect, *one)                                                # collect into a resolved accumulator
        _refused(EINVAL, W.resolve_accumulators, [acc], dmov, dref)                        # resolve twice
        _refused(EINVAL, acc.columns, dmov, dref, counts[3], 3)                            # columns before finish
        _refused(EINVAL, acc.finish, np.zeros(counts[2] + 1, np.int32))                    # n_winners > n_rest
        final = acc.finish(np.zeros(0, np.int32))
        _same(final, K.finish(want, []), "after refusals")
        _refused(EINVAL, acc.columns, dmov, dref, len(final) + 1, 3)                       # a wrong n_final
        buffers = [_lib.DeviceBuffer(ctx, 8 * n) for _ in range(5)]
        _refused(EINVAL, acc.columns, dmov, dref, len(final), 3, buffers)                  # five extras
        _refused(EINVAL, acc.columns, dmov, dref, len(final), 3, (), buffers)
        for b in buffers:
            b.free()
        # fetch
        out = np.empty(len(final) + 1, W.FINAL_RECORD)
        assert lib.same_merge_acc_fetch(acc.handle, 1, out.ctypes.data, out.nbytes) == EINVAL          # a wrong byte count
        assert lib.same_merge_acc_fetch(acc.handle, 1, out.ctypes.data, out.nbytes - 2 * 24) == EINVAL
        assert lib.same_merge_acc_fetch(acc.handle, 7, out.ctypes.data, out.nbytes - 24) == EINVAL     # an unknown selector
        assert lib.same_merge_acc_fetch(acc.handle, 0, out.ctypes.data, 0) == EINVAL                   # REST after finish
        _same(acc.final_rows(), final, "fetched after refused fetches")
        full_pass("after the collect refusals")
        # the loaded path
        acc.load(fam["a"], fam["r"], fam["flags"], fam["wid"], fam["pos"], fam["cidx"], fam["n_codes_a"], fam["n_codes_r"])
        _refused(EINVAL, W.plain_accumulators, [acc])                                      # plain on a loaded accumulator
        _refused(EINVAL, W.resolve_accumulators, [acc], dmov, dref)                        # loaded rows carry their codes: no sections
        other.begin(0)
        _refused(EINVAL, W.resolve_accumulators, [acc, other], None, None)                 # ... and no second accumulator
        want = K.resolve_family(fam)
        counts, rest = W.resolve_accumulators([acc], None, None)
        assert counts == want["counts"] and counts[2] > 0
        _same(rest, want["rest"], "loaded after refusals")
        bad = rest["row"][:2].copy()
        bad[1] = len(fam["a"])
        _refused(ERANGE, acc.finish, bad)                                                  # a winner row out of range
        bad[1] = -1
        _refused(ERANGE, acc.finish, bad)
        _refused(EINVAL, acc.finish, np.zeros(counts[2] + 1, np.int32))
        won = K.winners(rest)
        _same(acc.finish(won), K.finish(want, won), "loaded, finished after refusals")
        _refused(EINVAL, acc.columns, dmov, dref, acc.n_final, 3)                          # columns on a loaded accumulator
        a = fam["a"].copy()
        a[5] = fam["n_codes_a"]
        _refused(ERANGE, acc.load, a, fam["r"], fam["flags"], fam["wid"], fam["pos"], fam["cidx"], fam["n_codes_a"], fam["n_codes_r"])
        r = fam["r"].copy()
        r[-1] = fam["n_codes_r"]
        _refused(ERANGE, acc.load, fam["a"], r, fam["flags"], fam["wid"], fam["pos"], fam["cidx"], fam["n_codes_a"], fam["n_codes_r"])
        full_pass("after the load refusals")
        # begin
        for reach in (-1.0, float("nan"), float("inf"), -float("inf")):
            _refused(EINVAL, acc.begin, n, None, reach)
        _refused(EINVAL, acc.begin, n, (np.array([0, 2, 1], np.int32), np.zeros((2, 4))), 1.0)         # near_start decreases
        _refused(EINVAL, acc.begin, -1)
        full_pass("after the begin refusals")
        # a refused begin leaves the pass so far as it was
        acc.begin(n)
        rows = _collect(acc, [(w, _view(w, "every second cell"), box, 3, 0)])
        _refused(EINVAL, acc.begin, n, (np.array([0, 2, 1], np.int32), np.zeros((2, 4))), 1.0)
        _refused(EINVAL, acc.begin, n, (np.array([1, 1, 2], np.int32), np.zeros((2, 4))), 1.0)
        _refused(EINVAL, acc.begin, n, None, float("nan"))
        assert len(rows) > 0
        _plain_is([acc], rows, "after a refused begin")
    finally:
        unfinished.close()
        other.close()
        acc.close()
        other_ctx.close()


def test_the_pool_of_pinned_blocks_is_empty_and_the_windows_close():
    """the module's cached windows, sections and accumulator are handed back; no pinned block is out"""
    import gc

    W = _W()
    for w in [v for k, v in _WINDOWS.items() if k != "pool"] + _WINDOWS.get("pool", []):
        w["st"].close()
    _WINDOWS.clear()
    if "acc" in _HELD:
        _HELD.pop("acc").close()
    for dmov, dref, _case in _SECTIONS.values():
        dref.close()
        dmov.close()
    _SECTIONS.clear()
    gc.collect()
    assert W.PINNED_BLOCKS.out == 0
