"""The parts of the type-matrix variants (same_amd.sliding_window_variants, csrc/window_recost.hip) that need no GPU: the entry points'
declarations, the argument checks, the host statement of a recost (tests/variant_check.recost: oracle.pair_cost_arrays over the staged
pairs with the variant's moving rows) in both cost types, and the proof that the inputs tests/test_gpu_window_variants.py drives the
library with hold the shapes the kernel can go wrong at."""
import os

import numpy as np
import pandas as pd
import pytest

import caller_check as C
import variant_check as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_and_exported():
    from same_amd import _lib

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    for decl, name in (("int same_types_layer_create(", "same_types_layer_create"), ("void same_types_layer_destroy(", "same_types_layer_destroy"),
                       ("int same_window_recost(", "same_window_recost"), ("int same_merge_acc_columns_layer(", "same_merge_acc_columns_layer")):
        assert decl in header and name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    assert _lib._PROTOTYPES["same_window_recost"] == [_lib.c_vp, _lib.c_int, _lib.c_vp, _lib.c_vp, _lib.c_vp, _lib.c_dbl, _lib.c_vp]
    assert _lib._PROTOTYPES["same_merge_acc_columns_layer"] == _lib._PROTOTYPES["same_merge_acc_columns"][:2] + [_lib.c_vp] + \
        _lib._PROTOTYPES["same_merge_acc_columns"][2:]
    assert _lib.load().same_abi_version() == 9
    srcs = open(os.path.join(ROOT, "same_amd", "csrc", "Makefile")).read()
    assert "window_recost.hip" in srcs and os.path.exists(os.path.join(ROOT, "same_amd", "csrc", "window_recost.hip"))


def test_public_function_is_exported():
    import same_amd
    from same_amd import sweep, variants

    assert same_amd.sliding_window_variants is variants.sliding_window_variants and "sliding_window_variants" in same_amd.__all__
    assert "dist_ct_coeff" not in sweep.SWEEP_KEYS and "radius" not in sweep.SWEEP_KEYS


def _frames(n=400, seed=0):
    from same_amd import synth

    ref = synth.make_cells(n, 6, seed=seed)
    return synth.to_frame(ref), synth.to_frame(synth.make_jittered(ref, seed=seed + 1)), list(synth.type_columns(6))


def _bad_variants(mov, cols):
    good = mov[cols].to_numpy(dtype=np.float64)
    return [
        ([], "non-empty"),
        (None, "non-empty"),
        ({"a": good}, "non-empty"),
        ("noise", "non-empty"),
        (good, "non-empty"),                                             # one matrix in place of the list
        ([good[:-1]], "shape"),
        ([good[:, :-1]], "shape"),
        ([None, good.ravel()], "shape"),
        ([good[None]], "shape"),
        ([mov[cols[:-1]]], "lacks the commonCT columns"),
        ([mov[cols].iloc[:-1]], "shape"),
        ([np.full(good.shape, "x", dtype=object)], "float64"),
    ]


@pytest.mark.parametrize("which", range(12))
def test_invalid_variants_raise_before_any_job_or_device(monkeypatch, which):
    from same_amd import incumbent, sweep, variants, window_api

    def no_job(*a, **k):
        raise AssertionError("the window job (and with it the device) was reached before the arguments were checked")

    for module in (window_api, incumbent, sweep, variants):
        monkeypatch.setattr(module, "_WindowJob", no_job)
    ref, mov, cols = _frames()
    bad, message = _bad_variants(mov, cols)[which]
    for kw in (dict(commonCT=cols), dict()):                              # commonCT given, and inferred from the cell_type labels
        with pytest.raises(ValueError) as e:
            variants.sliding_window_variants(ref, mov, bad, **kw)
        assert message in str(e.value), (which, str(e.value))


def test_invalid_param_sets_raise_by_the_sweeps_own_check(monkeypatch):
    from same_amd import variants

    monkeypatch.setattr(variants, "_WindowJob", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a job was made")))
    ref, mov, cols = _frames()
    for sets, message in (([], "non-empty"), ([{"radius": 30}], "radius"), ({"knn": 4}, "non-empty")):
        with pytest.raises(ValueError) as e:
            variants.sliding_window_variants(ref, mov, [None], commonCT=cols, param_sets=sets)
        assert message in str(e.value)


def test_valid_variants_pass_the_checks_and_moving_variant_is_the_contract():
    from same_amd import variants

    ref, mov, cols = _frames()
    good = mov[cols].to_numpy(dtype=np.float64)
    frame = pd.DataFrame(good[:, ::-1] * 2.0, columns=cols[::-1], index=np.arange(len(mov))[::-1] + 5)    # other column order, other index
    frame["extra"] = 1
    mats = variants._checked_variants([None, good.astype(np.float32), (good * 3).tolist(), frame], len(mov), cols)
    assert mats[0] is None and all(m.dtype == np.float64 and m.flags.c_contiguous and m.shape == good.shape for m in mats[1:])
    assert np.array_equal(mats[1], good.astype(np.float32).astype(np.float64)) and np.array_equal(mats[3], good * 2.0)
    assert variants._common_types(ref, mov, ref, mov, None) == sorted(set(ref["cell_type"]))
    # moving_v: a copy, the commonCT columns replaced and float64, everything else and the caller's frame untouched
    before = mov.copy()
    mov_v = variants.moving_variant(mov, cols, mats[3])
    pd.testing.assert_frame_equal(mov, before, check_exact=True)
    assert list(mov_v.columns) == list(mov.columns) and mov_v.index.equals(mov.index)
    for t, c in enumerate(cols):
        assert mov_v[c].dtype == np.float64 and np.array_equal(mov_v[c].to_numpy(), mats[3][:, t])
    pd.testing.assert_frame_equal(mov_v.drop(columns=cols), mov.drop(columns=cols), check_exact=True)

    class Meta:            # a MetaCell-like object: a shallow copy whose .metacell_df is replaced
        def __init__(self, df):
            self.metacell_df, self.metacell_delaunay, self.other = df, object(), [1]

    mc = Meta(mov)
    mc_v = variants.moving_variant(mc, cols, mats[1])
    assert mc_v is not mc and mc_v.metacell_delaunay is mc.metacell_delaunay and mc_v.other is mc.other and mc.metacell_df is mov
    assert np.array_equal(mc_v.metacell_df[cols].to_numpy(), mats[1])


def test_sets_of_the_window_walk_name_their_variant():
    """the walk's own argument check, which needs no device: a variant index outside the list, variants without sets"""
    from same_amd import windows as W

    for kw in (dict(sets=[(4, None, 10.0, 2)], variants=[None, None]), dict(variants=[None]), dict(sets=[(4, None, 10.0)], variants=[])):
        with pytest.raises(ValueError):
            next(W.iter_device_windows(None, None, None, None, [], ctx=object(), **kw))


# ---- the host statement and the inputs of the GPU tests --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def staged(oracle):
    """per family: its staged list on the host, and the statement's costs under the section's own types and both variants, both dtypes"""
    out = {}
    for tag, case, box, radius, k in V.families(oracle):
        rows, rows_r, pairs = C.host_stage(case["mov_xy"], case["ref_xy"], box, radius, k, oracle)
        l1, l2 = V.variants_of(case["types_m"], 5)
        costs = {(name, dt): V.recost(case["mov_xy"], case["ref_xy"], types, case["types_r"], rows, rows_r, pairs, 1.0, dt, oracle)
                 for name, types in (("own", case["types_m"]), ("L1", l1), ("L2", l2)) for dt in ("float64", "float32")}
        out[tag] = dict(T=case["types_m"].shape[1], rows=rows, rows_r=rows_r, pairs=pairs, costs=costs, case=case, l1=l1, l2=l2)
    return out


def test_statement_is_the_pair_cost_of_the_variants_rows(staged, oracle):
    """the statement against the cost expression written out in numpy (src/same.py:1180-1189), row by row, left to right"""
    for tag in ("T3/65", "T20/big", "T65/127", "K/base/interior", "K/contention"):
        s = staged[tag]
        case, pairs = s["case"], s["pairs"]
        for name, types in (("own", case["types_m"]), ("L1", s["l1"]), ("L2", s["l2"])):
            for dt in (np.float64, np.float32):
                a, r = types[s["rows"]].astype(dt)[pairs[:, 0]], case["types_r"][s["rows_r"]].astype(dt)[pairs[:, 1]]
                axy, rxy = case["mov_xy"][s["rows"]].astype(dt)[pairs[:, 0]], case["ref_xy"][s["rows_r"]].astype(dt)[pairs[:, 1]]
                acc = np.zeros(len(pairs), dt)
                for t in range(a.shape[1]):
                    acc = acc + np.abs(a[:, t] - r[:, t])
                want = dt(1.0) * acc + (dt(1.0) * dt(0.001)) * (np.abs(axy[:, 0] - rxy[:, 0]) + np.abs(axy[:, 1] - rxy[:, 1]))
                got = s["costs"][(name, np.dtype(dt).name)]
                assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64)), (tag, name, dt)


def test_inputs_hold_the_shapes_the_kernel_can_go_wrong_at(staged):
    assert set(staged) == set(V.tags())
    P = {tag: len(s["pairs"]) for tag, s in staged.items()}
    # windows with 0 pairs (nothing in the box; rows and no pair), fewer than 64, 1 and 63 mod 64, enough for the LDS form
    assert P["T4/nothing"] == 0 and len(staged["T4/nothing"]["rows_r"]) == 0
    assert P["K/base/empty"] == 0 and len(staged["K/base/empty"]["rows_r"]) > 0 and P["K/base/beside"] == 0
    for T in V.T_VALUES:
        assert (P[f"T{T}/63"], P[f"T{T}/65"], P[f"T{T}/127"]) == (63, 65, 127)
        assert P[f"T{T}/big"] >= V.LDS_MIN_PAIRS and staged[f"T{T}/big"]["T"] == T
    assert P["T4/63"] < 64 and P["T4/65"] % 64 == 1 and P["T4/127"] % 64 == 63
    assert 0 < P["K/base/no triangle"] < 64
    # every T the kernel's forms part at: 1 (no LDS form), 2, pitches T|1 = T + 1 and T, 63 / 64 / 65 around a wave's width, a block that fits
    # in float and not in double, one that fits in neither
    assert set(V.T_VALUES) >= {1, 2, 3, 4, 20, 63, 64, 65}
    form = {T: (V.takes_lds(T, 8, P[f"T{T}/big"]), V.takes_lds(T, 4, P[f"T{T}/big"])) for T in V.T_VALUES}
    assert form[1] == (False, False) and all(form[T] == (True, True) for T in (2, 3, 4, 20, 63, 64, 65))
    assert form[200] == (False, True) and form[300] == (False, False)
    assert V.lds_waves(127, 8) == 1 and V.lds_waves(128, 8) == 0 and V.lds_waves(20, 8) == 4       # 64 x (T|1) doubles outgrow 64 KB from T = 128
    assert not V.takes_lds(4, 8, P["T4/127"])                                                   # a short list: one lane gathers its row
    # the families of the other pair-list calls: more than one launch block, the scan block edges, one reference 700 rows name
    assert P["K/base/whole"] > 20 * 256 and P["K/tie"] > 100 * 200 and P["K/contention"] == 700 * 8
    assert [len(staged[f"K/edge/{n}"]["rows"]) for n in C.EDGE_ROWS] == list(C.EDGE_ROWS)
    # every window with pairs: at least one pair's cost differs between any two of the three type matrices, in both cost types
    for tag, s in staged.items():
        if P[tag]:
            for dt in ("float64", "float32"):
                own, l1, l2 = (s["costs"][(name, dt)] for name in ("own", "L1", "L2"))
                assert (own != l1).any() and (own != l2).any() and (l1 != l2).any(), (tag, dt)
