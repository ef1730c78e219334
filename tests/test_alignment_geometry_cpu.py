"""The geometry families of tests/alignment_families.py on the CPU: the host statement of the device rule (tests/alignment_check.py)
against cKDTree on every decided row, at every k and under both labellings, and the conditions the GPU comparison
(tests/test_gpu_alignment_geometry.py) rests on -- few rows in doubt outside the degenerate families, some inside them, and each
family reaching the branch of align_geometry it is named for."""
import numpy as np
import pytest

import alignment_check as ac
import alignment_families as af

DOUBT_SHARE = 0.01


def _decided(flag):
    return (flag & ac.DECIDED) > 0


@pytest.mark.parametrize("name", af.NAMES)
def test_statement_equals_ckdtree_on_decided_rows(name):
    fam = af.family(name)
    n_q, n_t = len(fam.qxy), len(fam.txy)
    ks = af.ks_of(fam)
    assert ks and ks[-1] == min(n_t, 64)
    doubt_random = 0
    for k in ks:
        idx = af.neighbours(fam, k)[:, :k]
        found = (idx < n_t).all(axis=1)   # scipy reports no neighbour where the distance overflows
        for labelling in af.LABELLINGS:
            qc, tc, expect = af.labels(fam, k, labelling)
            flag, nearest, _, _ = ac.statement(fam.qxy, qc, fam.txy, tc, k)
            dec = _decided(flag)
            where = (name, k, labelling)
            assert found[dec].all(), where
            want = (tc[np.minimum(idx, n_t - 1)] == qc[:, None]).any(axis=1)
            assert np.array_equal((flag[dec] & ac.MATCH) > 0, want[dec]), where
            assert not (flag[~dec]).any(), where
            if k == 1:
                assert np.array_equal(nearest[dec], idx[dec, 0]) and (nearest[~dec] == -1).all(), where
            if expect is not None:
                assert np.array_equal((flag[dec] & ac.MATCH) > 0, expect[dec]), where
            doubt = int((~dec).sum())
            if fam.degenerate:
                # under the rank probe the label sits on the k-th boundary, so a tie there is a row in doubt at every k; a random
                # label out of 5 is nearly always in S once k is large, and then the row is decided whatever B holds
                assert doubt > 0 or labelling == "random", where
                doubt_random += doubt if labelling == "random" else 0
            else:
                assert doubt <= DOUBT_SHARE * n_q, (where, doubt)
            if name in ("scale_1e160", "scale_1e-150"):
                assert doubt == n_q, where
    assert doubt_random > 0 or not fam.degenerate, name


@pytest.mark.parametrize("name", [n for n in af.SIZE_NAMES if n != "cluster_outliers"])
def test_size_families_have_no_row_in_doubt(name):
    """what lets the 200 000-query GPU test hold these families to the 0.999 bar of the uniform case"""
    fam = af.family(name)
    for k in af.SIZE_KS:
        qc, tc, _ = af.labels(fam, k, "rank")
        assert _decided(ac.statement(fam.qxy, qc, fam.txy, tc, k)[0]).all(), (name, k)


def test_families_cover_the_issue_and_only_five_are_degenerate():
    assert set(af.DEGENERATE) == {"lattice", "duplicates", "single_point", "scale_1e-150", "scale_1e160"}
    assert {f"nq_{n}" for n in (1, 63, 64, 65, 255, 256, 257)} <= set(af.NAMES)
    assert {f"nt_{n}" for n in af.ALL_KS} <= set(af.NAMES) and af.ALL_KS == (*range(1, 10), 16, 33, 63, 64)
    assert all(len(af.family(f"nt_{n}").txy) == n for n in af.ALL_KS)
    assert all(len(af.family(f"nq_{n}").qxy) == n for n in af.BLOCK_NQ)


def test_families_reach_their_branches():
    """align_geometry restated (alignment_families.grid_of): each family lands in the branch it names"""
    g = {(n, k): af.grid_of(af.family(n).txy, k) for n in af.NAMES for k in af.ks_of(af.family(n), (1, 8, 64))}
    assert all(g["hline", k]["gy"] == 1 and g["hline", k]["gx"] > 100 for k in (1, 8, 64))
    assert g["hline", 1]["floored"] and g["hline", 1]["gx"] in (4096, 4097) and not g["hline", 64]["floored"]
    assert all(g["vline", k]["gx"] == 1 and g["vline", k]["gy"] > 10 for k in (1, 8, 64))
    assert all((g["single_point", k]["gx"], g["single_point", k]["gy"], g["single_point", k]["cell"]) == (1, 1, 1.0) for k in (1, 8, 64))
    assert g["nt_1", 1]["gx"] * g["nt_1", 1]["gy"] == 1
    assert g["aniso", 1]["gy"] == 1 and g["aniso", 1]["gx"] > 1000
    for k in (1, 8, 64):   # the whole cluster in one cell, outliers rings away
        c = g["cluster_outliers", k]
        t = af.family("cluster_outliers").txy
        n_c = (9 * len(t)) // 10
        cx, cy = np.floor((t[:n_c, 0] - c["x0"]) / c["cell"]), np.floor((t[:n_c, 1] - c["y0"]) / c["cell"])
        assert len(set(zip(cx.tolist(), cy.tolist()))) == 1 and c["gx"] >= 8 and c["gy"] >= 8
        assert (af.CLUSTER_SIDE / (2 * af.CLUSTER_BOX)) ** 2 <= 1e-7
    for n, frac in (("offset_1e9", 1e-4), ("offset_4e6", 0.02)):   # the magnitude term of the slack against the cell
        t = af.family(n).txy
        assert np.ldexp(np.abs(t).max(), -40) > frac * g[n, 1]["cell"]
    assert g["scale_1e160", 1]["gx"] * g["scale_1e160", 1]["gy"] == 1 and g["scale_1e150", 1]["gx"] > 10
    assert g["scale_1e-150", 1]["gx"] > 10
    # no family reaches the growth loop, and none can: with area >= ext^2 / n and cell >= sqrt(area / n),
    # (w / cell + 1) * (h / cell + 1) <= n + n + 1 + 1
    assert all(v["grew"] == 0 for v in g.values())
    q = af.family("outside").qxy
    e = af.OUTSIDE_EXT
    sides = set(zip(*((q.T > e).astype(int) - (q.T < 0).astype(int)).tolist()))
    assert sides == {(sx, sy) for sx in (-1, 0, 1) for sy in (-1, 0, 1)} - {(0, 0)}
    out = np.maximum(np.maximum(-q, q - e), 0.0).max(axis=1) / e
    assert out.min() < 1e-8 and out.max() > 500.0
