"""tests/merge_check.py without a GPU: its statement of the window merge against the other statements the project holds (the oracle's
de-duplication, merge.py's _resolve_rows and seam_rows, the reference's recorded rows in tests/golden); every row and window family has
the property it was made for; every deliberately wrong statement gives another answer on at least one family -- so a kernel wrong in
that way fails tests/test_gpu_merge_library.py --; and the merge's prototypes in the header, the bindings and the record sizes agree."""
import os
import re

import numpy as np
import pytest

import merge_check as K
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _viol(fam):
    return (fam["flags"] & 1) != 0


# ---- the statement against the other statements ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", K.LOAD_CASES)
def test_statement_is_the_oracles_and_the_host_merges(oracle, name, n):
    from same_amd import merge as M

    fam = K.family(name, n)
    assert len(fam["a"]) == n <= 40_000
    if n == 0:
        res = K.resolve_family(fam)
        assert res["counts"] == (0, 0, 0, 0) and len(K.finish(res, K.winners(res["rest"]))) == 0
        return
    kept = K.dedup(_viol(fam), fam["wid"], fam["a"], fam["r"])
    assert np.array_equal(kept, oracle.merge_dedup(_viol(fam), fam["wid"], fam["a"], fam["r"]))
    res = K.resolve_family(fam)
    final = K.finish(res, K.winners(res["rest"]))
    want = M._resolve_rows(fam["a"], fam["r"], _viol(fam), fam["wid"], oracle.merge_dedup)
    rows = K.loaded_rows(fam)
    assert K.same_records(final, K._final(rows, want))
    assert res["counts"][0] == n and res["counts"][1] == len(kept) and res["counts"][2] + res["counts"][3] == len(kept)
    # nothing but the rows final already without winners; they never reach the host
    alone = K.finish(res, [])
    assert len(alone) == res["counts"][3] and not np.isin(alone["a_row"], res["rest"]["ac"]).any()


def test_statement_reproduces_the_references_recorded_rows(oracle):
    g = load_golden("merge_dedup")
    for tag in ("a", "b"):
        rows, viol = g[f"{tag}_in"], g[f"{tag}_in_viol"]
        v = np.where(np.isnan(viol), True, viol != 0)                       # fillna(True) (src/helpers.py:746-751)
        rec = K.rows_of(rows[:, 1], rows[:, 2], v.astype(np.uint8), rows[:, 0], 0, np.arange(len(rows)))
        res = K.resolve(rec, None, None, rows[:, 1].max() + 1, rows[:, 2].max() + 1)
        final = K.finish(res, K.winners(res["rest"]))
        assert np.array_equal(final["cidx"], g[f"{tag}_out_rows"]), tag
        assert np.array_equal(np.column_stack((final["wid"], final["a_row"], final["r_row"])), g[f"{tag}_out"])
        assert np.array_equal(final["flags"] & 1, g[f"{tag}_out_viol"])
    from test_host_rows import _merge_input
    import pandas as pd

    g = load_golden("unpack_merge")
    table = pd.concat(_merge_input(), ignore_index=True)
    from same_amd.merge import _violation_flags
    v = _violation_flags(table["filtered_violation"])
    a, r, w = (table[c].to_numpy().astype(np.int64) for c in ("Aligned_Cell_Num_Old", "Ref_Cell_Num_Old", "window_id"))
    res = K.resolve(K.rows_of(a, r, v.astype(np.uint8), w, 0, np.arange(len(a))), None, None, a.max() + 1, r.max() + 1)
    final = K.finish(res, K.winners(res["rest"]))
    assert np.array_equal(np.column_stack((final["wid"], final["a_row"], final["r_row"])), g["merge_rows"])
    assert np.array_equal(final["flags"] & 1, g["merge_viol"])


def _plan():
    """a hand-made plan: six windows side by side, 100 wide, dealt to two ranks; the rows of rank 0's windows: cells on every trim edge,
    references exactly `reach` beyond a foreign trim and one nextafter further, cells in the middle, rows of unknown position"""
    trims = [(100.0 * p, 100.0 * (p + 1), 0.0, 50.0) for p in range(6)]
    plan = [dict(trim=t) for t in trims]
    owner = np.array([0, 1, 0, 0, 1, 0])
    reach = 7.5
    pos, a, r = [], [], []
    for p in np.flatnonzero(owner == 0):
        x0, x1 = trims[p][0], trims[p][1]
        out = np.nextafter
        for ax, rx in ((x0, x0), (x0 + 50, x0 + 50), (x0 + 50, x0 - reach), (x0 + 50, out(x0 - reach, -np.inf)), (x0 + 50, x1 + reach),
                       (x0 + 50, out(x1 + reach, np.inf)), (out(x1, -np.inf), x0 + 50), (x0 + 20, x0 + 20 - 2 * reach), (x0 + 50, x1),
                       (x0 + 50, out(x1, -np.inf)), (x0 + 50, x0 + reach)):
            for ay, ry in ((25.0, 25.0), (0.0, -reach), (25.0, 50.0 + reach), (25.0, out(50.0 + reach, np.inf)), (out(50.0, -np.inf), 49.0)):
                pos.append(p); a.append((ax, ay)); r.append((rx, ry))
    pos += [-1, -1]
    a += [(250.0, 25.0)] * 2
    r += [(250.0, 25.0)] * 2
    return plan, owner, reach, np.array(pos), np.array(a), np.array(r)


def test_seam_rule_is_merge_pys():
    from same_amd import merge as M

    plan, owner, reach, pos, a, r = _plan()
    rows = K.rows_of(np.arange(len(pos)), np.arange(len(pos)), 0, 0, pos, 0)
    for use_reach in (reach, 0.0):
        start, boxes = M.seam_tables(plan, owner, 0, use_reach)
        want = M.seam_rows(pos, lambda b, e: (a[b:e, 0], a[b:e, 1], r[b:e, 0], r[b:e, 1]), plan, owner, 0, use_reach)
        got = K.seam_of(rows, (start, boxes, use_reach, a, r))
        assert np.array_equal(got, want) and 0 < want.sum() < len(want)
        assert want[pos < 0].all() and not want[pos == 3].all()
        for wrong in (dict(ref_test="half open"), dict(aligned_test="closed"), dict(out_of_range=False)):
            if use_reach or "aligned_test" not in wrong:
                assert not np.array_equal(K.seam_of(rows, (start, boxes, use_reach, a, r), **wrong), want), wrong
    # a position past the table is a seam; the product's own rule has no such position
    assert K.seam_of(K.rows_of([0], [0], 0, 0, len(plan), 0), (start, boxes, reach, a, r)).all()
    assert not K.seam_of(rows, None).any() and K.seam_of(rows, "all").all()


# ---- each family has the property it was made for --------------------------------------------------------------------------------------
def test_sizes_are_the_block_edges_they_claim():
    blocks = lambda n: -(-n // K.SCAN_NT)
    assert K.SCAN_NT in K.SIZES and K.SORT_BLOCK in K.SIZES and blocks(255) == blocks(256) == 1 and blocks(257) == 2
    pad = lambda n: max(K.SORT_BLOCK, 1 << (n - 1).bit_length())
    assert pad(2048) == 2048 and pad(2049) == 4096 and pad(4097) == 8192           # one and two global strides (j >= 2048)
    strides = lambda n: sum(1 for k in range(12, pad(n).bit_length()) for j in range(11, k) if (1 << k) <= pad(n))
    assert (strides(2048), strides(2049), strides(4097)) == (0, 1, 3)
    assert blocks(16385) == K.LOOKBACK + 1 and blocks(16384) == K.LOOKBACK
    assert max(n for _f, n in K.LOAD_CASES) <= 40_000


def test_alone_and_one_pair():
    for n in K.FAMILIES["alone"][1]:
        res = K.resolve_family(K.family("alone", n))
        assert res["counts"] == (n, n, 0, n)
    for n in K.FAMILIES["one pair"][1]:
        fam = K.family("one pair", n)
        res = K.resolve_family(fam)
        assert res["counts"] == (n, 1, 0, 1) and len(np.unique(fam["a"])) == 1 == len(np.unique(fam["r"]))
        if n >= 255:
            assert len(np.unique(fam["flags"])) == 4 and len(np.unique(fam["wid"])) == 3


@pytest.mark.parametrize("n", K.FAMILIES["keys"][1])
def test_keys_family(n):
    fam = K.family("keys", n)
    viol, wid, pair = _viol(fam), fam["wid"], fam["pair"]
    counts = np.bincount(pair)
    assert counts.min() >= 2 and counts.max() <= 4
    kept = K.dedup(viol, wid, fam["a"], fam["r"])
    seen = set()
    for row in kept:
        others = np.flatnonzero(pair == pair[row])
        if len(set(viol[others])) == 2:
            seen.add("viol")
            assert not viol[row] and wid[row] > wid[others[viol[others]]].max()        # the non-violating row of the LARGER window id
        elif len(set(wid[others])) > 1:
            seen.add("wid")
            assert wid[row] == wid[others].min() and len(set(wid[others])) == len(others)
        else:
            seen.add("row")
            assert row == others.min()
            if n > 2:
                assert row != others.max()
    assert seen == ({"viol", "wid", "row"} if n >= 255 else {"viol"})


@pytest.mark.parametrize("n", K.FAMILIES["flag bits"][1])
def test_flag_bits_family(n):
    fam = K.family("flag bits", n)
    flags, pair = fam["flags"], fam["pair"]
    only_bit1 = [p for p in range(pair.max() + 1) if len(set(flags[pair == p] & 1)) == 1 and len(set(flags[pair == p] & 2)) == 2
                 and len(set(fam["wid"][pair == p])) == 1]
    assert len(only_bit1) >= (20 if n >= 255 else 1)
    # in some of them a row with bit 1 set is the earliest: a mask of 3 would give the pair to a later row
    assert n < 255 or any(flags[np.flatnonzero(pair == p)[0]] & 2 for p in only_bit1)
    if n >= 255:
        assert set(flags.tolist()) == {0, 1, 2, 3}
        final = K.finish(K.resolve_family(fam), [])
        assert set(final["flags"].tolist()) == {0, 1, 2, 3}                           # FinalRec.flags keeps both bits


def test_wid_extremes_and_sparse_codes():
    for n in K.FAMILIES["wid extremes"][1]:
        fam = K.family("wid extremes", n)
        assert set(fam["wid"].tolist()) <= set(K.WID_EXTREMES) and (n < 255 or set(fam["wid"].tolist()) == set(K.WID_EXTREMES))
        assert fam["wid"].max() < 2 ** 31
    for n in K.FAMILIES["sparse codes"][1]:
        fam = K.family("sparse codes", n)
        assert fam["n_codes_a"] == fam["n_codes_r"] == K.SPARSE_CODES == 100_000 and n <= 257
        if n >= 2:
            for codes in (fam["a"], fam["r"]):
                assert codes.min() == 0 and codes.max() == K.SPARSE_CODES - 1
        if n >= 7:
            assert K.resolve_family(fam)["counts"] == (n, n - 1, 2, n - 3)


def test_probe_chain_family():
    fam = K.family("probe chain", K.PROBE_ROWS)
    assert fam["slots"] == K.table_slots(2048) == 4096 and len(fam["a"]) == 2048
    assert K.mix64(np.array([1, 2 ** 63 + 5], np.uint64)).tolist() == [0x5692161D100B05E5, K.mix64(np.array([2 ** 63 + 5], np.uint64))[0]]
    home = K.home_slot(fam["a"], fam["r"], 4096)
    pair = fam["a"].astype(np.int64) << 32 | fam["r"]
    for h in K.PROBE_HOMES:
        at = home == h
        assert len(np.unique(pair[at])) >= 200 and (np.bincount(np.unique(pair[at], return_inverse=True)[1]) == 3).all()
        assert (fam["a"][at] < 1024).all() and (fam["r"][at] < 1024).all()
    # both chains pass the table's last slot: 200 pairs from 4094 and 200 from 4095 cannot sit in two slots
    assert K.PROBE_HOMES == (4095, 4094) and 4095 + 200 > 4096
    # every home slot has at least 202 candidate pairs below 1024 x 1024
    ga, gr = np.meshgrid(np.arange(1024), np.arange(1024), indexing="ij")
    assert np.bincount(K.home_slot(ga.ravel(), gr.ravel(), 4096), minlength=4096).min() >= 202
    rest = (fam["a"] >= 1024)
    assert (fam["r"][rest] >= 1024).all() and len(np.unique(fam["a"][rest])) == rest.sum() == len(np.unique(fam["r"][rest]))


def test_stars_and_chains_family():
    for n in K.FAMILIES["stars and chains"][1]:
        fam = K.family("stars and chains", n)
        res = K.resolve_family(fam)
        assert res["counts"] == (n, n, n, 0)                                         # everything contested, nothing final on the device
    fam = K.family("stars and chains", K.STARS_NATURAL)
    assert np.count_nonzero(fam["a"] == 0) == 300 and np.count_nonzero(fam["r"] == 300) == 300 and K.STARS_NATURAL == 1111
    path = (fam["a"] > 300) & (fam["r"] > 300)
    assert path.sum() == 511 and np.bincount(fam["a"][path]).max() == 2 and np.bincount(fam["r"][path]).max() == 2


# ---- the window families ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", K.WINDOWS)
def test_window_families_and_trims(oracle, tag):
    case, box = K.window_of(tag)
    views = {name: K.host_view(case, box, oracle, name) for name in K.MATCHINGS}
    v = views["all first candidate"]
    n = len(v["rows"])
    if tag.startswith("edge/"):
        assert n == int(tag[5:])
    assert n >= 40 and (v["match_row"] >= 0).all() and not (views["none"]["match_row"] >= 0).any()
    assert np.array_equal(views["every second cell"]["match_row"] >= 0, np.arange(n) % 2 == 0)
    m = K.marked_cell(v["xy"])
    on_edge = views["only cells on a trim edge"]["match_row"] >= 0
    assert on_edge[m] and 1 <= on_edge.sum() < n
    for kind in K.TRIMS:
        trim = K.trim_of(kind, box, v["xy"])
        if trim is None:
            assert kind == "-0.0 edge" and tag != "zero"
            continue
        got = K.collect_rows(v["rows"], v["xy"], v["match_row"], v["flag"], trim, 3, 5)
        assert np.all(np.diff(got["cidx"]) > 0) and np.array_equal(got["a_row"], v["rows"][got["cidx"]])
        assert np.array_equal(got["flags"], v["flag"][got["cidx"]]) and (got["wid"] == 3).all() and (got["pos"] == 5).all()
        inside = np.zeros(n, bool)
        inside[got["cidx"]] = True
        if kind in ("whole", "infinite"):
            assert inside.all()
        elif kind in ("tx0 == tx1", "inverted", "NaN edge"):
            assert not inside.any()
        else:
            assert inside.any() and not inside.all()
        if kind == "lower edges on a cell":
            assert inside[m]
            assert len(K.collect_rows(v["rows"], v["xy"], on_edge.astype(np.int32) - 1, v["flag"], trim, 0, 0)) >= 1
        if kind == "upper edges on a cell":
            assert not inside[m]
        if kind == "-0.0 edge":
            assert np.signbit(trim[0]) and trim[0] == 0.0 and v["xy"][m, 0] == 0.0 and not np.signbit(v["xy"][m, 0])
            assert np.array_equal(inside, v["xy"][:, 0] >= 0.0) and inside[m] and (v["xy"][:, 0] < 0).any()
            below = K.collect_rows(v["rows"], v["xy"], v["match_row"], v["flag"], (box[0], -0.0, box[2], box[3]), 0, 0)     # -0.0 as the upper edge
            assert len(below) and (case["mov_xy"][below["a_row"], 0] < 0.0).all()


def test_seam_case(oracle):
    case = K.seam_case()
    v = K.host_view(case, case["box"], oracle, "all first candidate")
    n = len(case["mov_xy"])
    assert np.array_equal(v["rows"], np.arange(n)) and np.array_equal(v["match_row"], np.arange(n)) and len(v["pairs"]) == n
    assert len(case["near_start"]) == K.SEAM_N_POS + 1 and case["near_start"][-1] == len(case["near_boxes"])
    assert np.all(np.diff(case["near_start"]) >= 0) and case["near_start"][3] == case["near_start"][4]
    rows = np.concatenate([K.collect_rows(v["rows"], v["xy"], v["match_row"], v["flag"], t, b, K.SEAM_POS[b]) for b, t in enumerate(K.seam_trims())])
    assert len(rows) == n and np.array_equal(np.bincount(rows["wid"]), np.full(K.SEAM_BANDS, 6))
    x = case["mov_xy"][rows["a_row"], 0]
    at = lambda reach: K.seam_of(rows, (case["near_start"], case["near_boxes"], reach, case["mov_xy"], case["ref_xy"]))
    s0, s = at(0.0), at(K.SEAM_REACH)
    band = lambda b: rows["wid"] == b
    assert x[band(0) & s0].tolist() == [4.0, 8.0] and x[band(0) & s].tolist() == [4.0, 8.0, 12.0]      # on x0: a seam; on x1: not, but for the reach
    assert x[band(1) & s].tolist() == [4.0, 8.0, 12.0] and x[band(1) & s0].tolist() == [8.0]             # references exactly `reach` outside
    assert x[band(2) & s].tolist() == [8.0]                                                                # one nextafter further out
    assert case["ref_xy"][1 * K.SEAM_BANDS, 0] == 5.0 - K.SEAM_REACH and case["ref_xy"][3 * K.SEAM_BANDS, 0] == 11.5 + K.SEAM_REACH
    assert not (band(3) | band(7)).__and__(s).any() and s[band(5) | band(6)].all() and s0[band(5) | band(6)].all()
    assert x[band(4) & s0].tolist() == [16.0] and x[band(4) & s].tolist() == [16.0, 20.0]


# ---- the families discriminate ---------------------------------------------------------------------------------------------------------
def _collect_differs(oracle, tags, **wrong):
    for tag in tags:
        case, box = K.window_of(tag)
        v = K.host_view(case, box, oracle, "all first candidate")
        for kind in K.TRIMS:
            trim = K.trim_of(kind, box, v["xy"])
            if trim is not None and not K.same_records(K.collect_rows(v["rows"], v["xy"], v["match_row"], v["flag"], trim, 0, 0),
                                                       K.collect_rows(v["rows"], v["xy"], v["match_row"], v["flag"], trim, 0, 0, **wrong)):
                return True
    return False


def _resolve_differs(names, **wrong):
    hit = []
    for name, n in K.LOAD_CASES:
        if name in names:
            fam = K.family(name, n)
            right, other = K.resolve_family(fam), K.resolve_family(fam, **wrong)
            if not (K.same_records(right["rest"], other["rest"]) and np.array_equal(right["row_of"], other["row_of"])):
                hit.append((name, n))
    return hit


def _seam_differs(oracle, **wrong):
    case = K.seam_case()
    v = K.host_view(case, case["box"], oracle, "all first candidate")
    rows = np.concatenate([K.collect_rows(v["rows"], v["xy"], v["match_row"], v["flag"], t, b, K.SEAM_POS[b]) for b, t in enumerate(K.seam_trims())])
    out = []
    for reach in (0.0, K.SEAM_REACH):
        seams = (case["near_start"], case["near_boxes"], reach, case["mov_xy"], case["ref_xy"])
        n = len(case["mov_xy"])
        out.append(not K.same_records(K.resolve(rows, None, None, n, n, seams)["rest"], K.resolve(rows, None, None, n, n, seams, **wrong)["rest"]))
    return any(out)


def test_a_closed_upper_trim_edge_is_caught(oracle):
    assert _collect_differs(oracle, K.WINDOWS, upper="closed")
    assert _collect_differs(oracle, ("edge/255",), upper="closed") and _collect_differs(oracle, ("zero",), upper="closed")


def test_an_open_lower_trim_edge_is_caught(oracle):
    assert _collect_differs(oracle, ("edge/256",), lower="open") and _collect_differs(oracle, ("zero",), lower="open")


def test_a_violation_mask_of_3_is_caught():
    hit = _resolve_differs(("flag bits",), mask=3)
    assert {n for _f, n in hit} >= {255, 256, 257, 2047, 2048, 2049, 4097, 16385}
    assert not _resolve_differs(("keys", "wid extremes"), mask=3)                      # (their flags use bit 0 alone)


def test_the_later_row_winning_a_tie_is_caught():
    assert len(_resolve_differs(("keys",), tie="later")) >= 8 and _resolve_differs(("one pair",), tie="later")


def test_signed_window_ids_are_caught():
    assert len(_resolve_differs(("wid extremes",), wid_order="signed")) >= 8
    assert not _resolve_differs(("keys", "flag bits", "alone"), wid_order="signed")    # small ids alone do not tell


def test_wrong_seam_tests_are_caught(oracle):
    assert _seam_differs(oracle, ref_test="half open")
    assert _seam_differs(oracle, aligned_test="closed")
    assert _seam_differs(oracle, out_of_range=False)


def test_final_rows_by_row_number_are_caught():
    hit = 0
    for name, n in K.LOAD_CASES:
        res = K.resolve_family(K.family(name, n))
        w = K.winners(res["rest"])
        hit += not K.same_records(K.finish(res, w), K.finish(res, w, order="row"))
    assert hit >= 40


def test_cidx_of_the_staged_view_is_caught(oracle):
    """a window whose view a caller's compaction shortened: the cells' indices among the cells as staged are other numbers"""
    case, box = K.window_of("base/interior")
    v = K.host_view(case, box, oracle, "all first candidate")
    keep = np.arange(len(v["rows"])) % 3 != 1
    cur = {k: v[k][keep] for k in ("rows", "xy", "match_row", "flag")}
    right = K.collect_rows(cur["rows"], cur["xy"], cur["match_row"], cur["flag"], box, 0, 0)
    wrong = K.collect_rows(cur["rows"], cur["xy"], cur["match_row"], cur["flag"], box, 0, 0, staged_rows=v["rows"])
    assert np.array_equal(right["cidx"], np.arange(keep.sum())) and not K.same_records(right, wrong)
    assert np.array_equal(right["a_row"], wrong["a_row"])


def test_a_byte_block_at_a_multiple_of_8_rows_is_caught():
    rng = np.random.default_rng(9)
    for n in (1, 7, 255, 256, 257):
        final = np.zeros(n, K.FINAL)
        final["a_row"], final["r_row"], final["flags"] = rng.integers(0, 30, n), rng.integers(0, 30, n), rng.integers(0, 4, n)
        xy = rng.random((30, 2))
        wide, flags = K.columns(final, rng.random((30, 3)), xy, xy, (rng.random(30),), ())
        assert wide.shape == (3 + 4 + 1 + 3, n) and flags.shape == (2, n)
        back = K.split_image(K.block_image(wide, flags), len(wide), n)
        assert np.array_equal(back[0], wide) and np.array_equal(back[1], flags)
        shifted = K.split_image(K.block_image(wide, flags, byte_rows="multiple of 8"), len(wide), n)
        assert np.array_equal(shifted[1], flags) == (n % 8 == 0), n


def test_columns_are_bit_patterns():
    final = np.zeros(3, K.FINAL)
    final["a_row"], final["r_row"], final["cidx"], final["wid"], final["pos"], final["flags"] = [2, 0, 1], [1, 1, 0], [5, 6, 7], [1, 2, 3], [-1, 0, 4], [1, 2, 3]
    nan = np.array([0x7FF8000000000123, 0xFFF0000000000001, 0x8000000000000000], np.uint64).view(np.float64)
    ids = np.array([-5, 2 ** 62, -2 ** 63], np.int64)
    xy = np.array([[-0.0, 5e-324], [np.inf, -np.inf], [1.0, 2.0]])
    wide, flags = K.columns(final, nan.reshape(3, 1), xy, xy, (ids,), (nan,))
    assert wide[0].tolist() == [0x8000000000000000, 0x7FF8000000000123, 0xFFF0000000000001]
    assert wide[1].tolist() == K._bits(xy[[2, 0, 1], 0]).tolist() and wide[5].tolist() == ids[[2, 0, 1]].view(np.uint64).tolist()
    assert wide[6].tolist() == [0xFFF0000000000001, 0xFFF0000000000001, 0x7FF8000000000123]
    assert wide[9].view(np.int64).tolist() == [-1, 0, 4] and flags.tolist() == [[0, 1, 1], [1, 0, 1]]


# ---- the header and the bindings --------------------------------------------------------------------------------------------------------
def test_merge_entry_points_are_declared_and_bound():
    from same_amd import _lib
    from same_amd import windows as W

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    lib = _lib.load()
    for name in ("same_section_set_codes", "same_merge_acc_begin", "same_window_collect", "same_merge_acc_load", "same_merge_acc_resolve",
                 "same_merge_acc_finish", "same_merge_acc_plain", "same_merge_acc_fetch", "same_merge_acc_columns",
                 "same_merge_acc_columns_layer", "same_host_alloc", "same_host_free"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl is not None, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(_lib._PROTOTYPES[name]), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    size = lambda macro: int(re.search(r"#define " + macro + r" (\d+)", header).group(1))
    assert W.REST_RECORD.itemsize == size("SAME_MERGE_REST_BYTES") == K.REST.itemsize and W.REST_RECORD == K.REST
    assert W.FINAL_RECORD.itemsize == size("SAME_MERGE_FINAL_BYTES") == K.FINAL.itemsize and W.FINAL_RECORD == K.FINAL
    assert (size("SAME_MERGE_REST"), size("SAME_MERGE_FINAL")) == (0, 1)
    assert K.LAUNCH_WINDOWS == 8 and "SAME_LAUNCH_WINDOWS = 8" in open(os.path.join(ROOT, "same_amd", "csrc", "common.h")).read().replace("  ", " ")
