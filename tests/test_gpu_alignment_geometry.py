"""csrc/align.hip on the MI355X over the geometry families of tests/alignment_families.py: every kernel instantiation (k = 1 ... 8 in
registers, 9 ... 64 in LDS), every branch of the grid and of the early stop, under random labels and under the rank probe that puts
each query's label on its k-th or (k+1)-th neighbour.  Flags against the host statement (tests/alignment_check.py, itself held to
cKDTree by tests/test_alignment_geometry_cpu.py), frames against a cKDTree restatement, 200 000 queries against one cKDTree query, the
block shapes through the raw call with guarded outputs, and a context shared with knn_prune."""
import functools

import numpy as np
import pandas as pd
import pytest

import alignment_check as ac
import alignment_families as af

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name, k, labelling):
    """-> (family, qcode, tcode, expected bit or None, the statement's flag, the statement's nearest)"""
    fam = af.family(name)
    qc, tc, expect = af.labels(fam, k, labelling)
    sflag, snear, _, _ = ac.statement(fam.qxy, qc, fam.txy, tc, k)
    return fam, qc, tc, expect, sflag, snear


def _grid(name):
    return [(k, lab) for k in af.ks_of(af.family(name)) for lab in af.LABELLINGS]


@pytest.mark.parametrize("name", af.NAMES)
def test_flags_equal_the_statement(name):
    from same_amd import ops

    for k, lab in _grid(name):
        fam, qc, tc, expect, sflag, snear = _case(name, k, lab)
        flag, nearest = ops.check_alignment(fam.qxy, qc, fam.txy, tc, k)
        bad = np.flatnonzero(flag != sflag)
        assert not len(bad), (name, k, lab, len(bad), bad[:5], flag[bad[:5]], sflag[bad[:5]])
        if k == 1:
            assert np.array_equal(nearest, snear), (name, lab)
        else:
            assert nearest is None
        if expect is not None:
            dec = (flag & ac.DECIDED) > 0
            assert np.array_equal((flag[dec] & ac.MATCH) > 0, expect[dec]), (name, k)


@pytest.mark.parametrize("name", af.NAMES)
def test_frames_equal_ckdtree(name):
    from same_amd.eval_utils import check_alignment

    for k, lab in _grid(name):
        fam, qc, tc, expect, sflag, _ = _case(name, k, lab)
        q, t = af.frames(fam, qc, tc)
        doubt = int(((sflag & ac.DECIDED) == 0).sum())
        try:
            match, idx = af.restatement(fam, qc, tc, k)
        except IndexError as e:   # scipy finds no neighbour where every distance overflows, and the reference's lookup raises
            assert name == "scale_1e160" and doubt == len(q)
            with pytest.raises(type(e)):
                check_alignment(q, t, "X", "Y", kNN=k)
            continue
        df, score, stats = check_alignment(q, t, "X", "Y", kNN=k, return_stats=True)
        want = q.copy()
        want.loc[:, f"_{k}NN_match"] = match
        if k == 1:
            want.loc[:, "_1NN_match_ctype"] = tc.astype(np.int64)[idx]
        pd.testing.assert_frame_equal(df, want, check_exact=True)
        assert score == match.mean(), (name, k, lab)
        assert stats == {"rows": len(q), "rows_decided_on_device": len(q) - doubt, "rows_resolved_on_host": doubt, "kNN": k}, (name, k, lab)
        if name == "scale_1e-150":
            assert doubt == len(q)
        elif not fam.degenerate:
            assert doubt <= 0.01 * len(q)


SIZE_NQ, SIZE_NT, SAMPLE = 200_000, 20_000, 5_000


@pytest.mark.parametrize("k", af.SIZE_KS)
@pytest.mark.parametrize("name", af.SIZE_NAMES)
def test_200k_queries_against_ckdtree(name, k):
    """The families whose statement-sized check leaves no row in doubt (test_alignment_geometry_cpu.py) are held to the 0.999 bar of
    the uniform 200k test; cluster_outliers to the 1 % condition."""
    from same_amd import ops
    from same_amd.eval_utils import check_alignment

    fam = af.family(name, SIZE_NQ, SIZE_NT)
    qc, tc, expect = af.labels(fam, k, "rank")
    bar = 0.99 if name == "cluster_outliers" else 0.999
    # the inputs are within the bar before the device is asked: the statement on a sample of the queries
    pick = np.random.default_rng(k).choice(SIZE_NQ, SAMPLE, replace=False)
    sflag, snear, _, _ = ac.statement(fam.qxy[pick], qc[pick], fam.txy, tc, k, block=256)
    sdec = (sflag & ac.DECIDED) > 0
    assert sdec.sum() >= bar * SAMPLE, (name, k, int(sdec.sum()))
    assert np.array_equal((sflag[sdec] & ac.MATCH) > 0, expect[pick][sdec])

    q, t = af.frames(fam, qc, tc)
    df, score, stats = check_alignment(q, t, "X", "Y", kNN=k, return_stats=True)
    got = df[f"_{k}NN_match"].to_numpy()
    idx = af.neighbours(fam, k)[:, :k]
    match = (tc[idx] == qc[:, None]).any(axis=1)
    bad = np.flatnonzero(got != match)
    assert not len(bad), (name, k, len(bad), bad[:5])
    assert score == match.mean()
    assert stats["rows_decided_on_device"] >= bar * SIZE_NQ, (name, k, stats)
    flag, nearest = ops.check_alignment(fam.qxy, qc, fam.txy, tc, k)
    dec = (flag & ac.DECIDED) > 0
    assert dec.sum() == stats["rows_decided_on_device"]
    assert np.array_equal((flag[dec] & ac.MATCH) > 0, expect[dec]) and not flag[~dec].any()
    assert np.array_equal(flag[pick], sflag), (name, k)
    if k == 1:
        assert np.array_equal(df["_1NN_match_ctype"].to_numpy(), idx[:, 0])
        assert np.array_equal(nearest[dec], idx[dec, 0]) and (nearest[~dec] == -1).all() and np.array_equal(nearest[pick], snear)


def _raw(ctx, qxy, qc, txy, tc, k, guard=1):
    """same_check_alignment with `guard` extra elements after each output, pre-filled"""
    n_q = len(qxy)
    flag = np.full(n_q + guard, 0xA5, np.uint8)
    nearest = np.full(n_q + guard, -77, np.int32)
    with ctx.lock:
        ctx.check(ctx.lib.same_check_alignment(ctx.handle, qxy.ctypes.data, n_q, qc.ctypes.data, txy.ctypes.data, len(txy), tc.ctypes.data, k,
                                               flag.ctypes.data, nearest.ctypes.data if k == 1 else None), "same_check_alignment")
    assert (flag[n_q:] == 0xA5).all() and (nearest[n_q:] == -77).all() and (k == 1 or (nearest == -77).all())
    return flag[:n_q], nearest[:n_q] if k == 1 else None


@pytest.mark.parametrize("k", [1, 8, 9, 64])
def test_block_shapes_with_guarded_outputs(k):
    from same_amd import _lib

    ctx = _lib.default_context()
    for n_q in af.BLOCK_NQ:
        fam = af.family(f"nq_{n_q}", n_t=5000)
        for lab in af.LABELLINGS:
            qc, tc, expect = af.labels(fam, k, lab)
            flag, nearest = _raw(ctx, fam.qxy, qc, fam.txy, tc, k)
            sflag, snear, _, _ = ac.statement(fam.qxy, qc, fam.txy, tc, k)
            assert np.array_equal(flag, sflag), (n_q, k, lab)
            if k == 1:
                assert np.array_equal(nearest, snear), (n_q, lab)
            if expect is not None:   # uniform points: nothing in doubt, every bit is the probe's
                assert np.array_equal(flag, np.where(expect, ac.DECIDED | ac.MATCH, ac.DECIDED)), (n_q, k)


def test_one_context_across_calls_and_knn_prune(oracle):
    """The call shares scratch slots with knn_prune and the window path: each call on a shared context gives its own answer."""
    from same_amd import _lib, ops

    ctx = _lib.default_context()
    calls = [("aniso", 3, "rank"), ("nt_16", 16, "rank"), ("cluster_outliers", 1, "random"), ("nq_65", 64, "rank"), ("aniso", 3, "rank")]
    rng = np.random.default_rng(11)
    axy, rxy = rng.random((1200, 2)) * 300, rng.random((900, 2)) * 300
    want_prune = oracle.knn_prune(axy, rxy, 25.0, 32)
    for name, k, lab in calls:
        fam, qc, tc, _, sflag, snear = _case(name, k, lab)
        flag, nearest = ops.check_alignment(fam.qxy, qc, fam.txy, tc, k, ctx=ctx)
        assert np.array_equal(flag, sflag), (name, k)
        if k == 1:
            assert np.array_equal(nearest, snear), name
        got = ops.knn_prune(axy, rxy, 25.0, 32, ctx=ctx)
        assert all(np.array_equal(a, b) for a, b in zip(got, want_prune)), name
