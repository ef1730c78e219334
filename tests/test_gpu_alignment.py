"""eval_utils.check_alignment on the MI355X (csrc/align.hip): the reference's frames of tests/golden/check_alignment.npz exactly, the
device's flags against the host statement (tests/alignment_check.py), and large random inputs against a vectorised cKDTree
restatement."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import alignment_check as ac
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


def _cases():
    g = load_golden("check_alignment")
    for name in g["cases"]:
        name = str(name)
        q_lab = ac.decode_labels(g[f"{name}_q_kind"], g[f"{name}_q_text"])
        t_lab = ac.decode_labels(g[f"{name}_t_kind"], g[f"{name}_t_text"])
        q = pd.DataFrame({"X": g[f"{name}_q_xy"][:, 0], "Y": g[f"{name}_q_xy"][:, 1]})
        q["cell_type"] = pd.Series(q_lab, dtype=object)
        t = pd.DataFrame({"X": g[f"{name}_t_xy"][:, 0], "Y": g[f"{name}_t_xy"][:, 1]})
        t["cell_type"] = pd.Series(t_lab, dtype=object)
        yield g, name, q, t


def test_frames_equal_the_reference():
    from same_amd.eval_utils import check_alignment

    hosted = 0
    for g, name, q, t in _cases():
        for k in g[f"{name}_ks"].tolist():
            if f"{name}_k{k}_error" in g:
                with pytest.raises(Exception) as e:
                    check_alignment(q, t, "X", "Y", kNN=k)
                assert type(e.value).__name__ == str(g[f"{name}_k{k}_error"])
                continue
            df, score, stats = check_alignment(q, t, "X", "Y", kNN=k, return_stats=True)
            want = q.copy()
            col = f"_{k}NN_match"
            want.loc[:, col] = g[f"{name}_k{k}_match"].astype(bool) if len(q) else []
            assert str(want[col].dtype) == str(g[f"{name}_k{k}_match_dtype"])
            if k == 1:
                want.loc[:, "_1NN_match_ctype"] = ac.decode_labels(g[f"{name}_k1_ctype_kind"], g[f"{name}_k1_ctype_text"])
            pd.testing.assert_frame_equal(df, want, check_exact=True)
            ref_score = float(g[f"{name}_k{k}_score"][0])
            assert (np.isnan(score) and np.isnan(ref_score)) or score == ref_score, (name, k)
            assert stats["rows"] == len(q) == stats["rows_decided_on_device"] + stats["rows_resolved_on_host"]
            hosted += stats["rows_resolved_on_host"]
    assert hosted > 0


@pytest.mark.parametrize("ks", [(1, 3, 8, 16, 64)])
def test_device_flags_equal_the_statement(ks):
    from same_amd import ops
    from same_amd.eval_utils import _label_codes

    for g, name, q, t in _cases():
        if not len(q):
            continue
        qc, tc = _label_codes(q["cell_type"].to_numpy(), t["cell_type"].to_numpy())
        qxy, txy = q[["X", "Y"]].to_numpy(), t[["X", "Y"]].to_numpy()
        for k in ks:
            if k > len(t):
                continue
            flag, nearest = ops.check_alignment(qxy, qc, txy, tc, k)
            sflag, snear, _, _ = ac.statement(qxy, qc, txy, tc, k)
            assert np.array_equal(flag, sflag), (name, k, np.flatnonzero(flag != sflag)[:5])
            if k == 1:
                assert np.array_equal(nearest, snear), name


def _restatement(q, t, k):
    """the reference's rule with one vectorised cKDTree query"""
    from scipy.spatial import cKDTree

    _, idx = cKDTree(t[["X", "Y"]]).query(q[["X", "Y"]], k=k)
    qt, tt = q["cell_type"].to_numpy(), t["cell_type"].to_numpy()
    if k == 1:
        return qt == tt[idx], tt[idx]
    return (tt[idx] == qt[:, None]).any(axis=1), None


def _random(n, seed):
    rng = np.random.default_rng(seed)
    types = np.array([f"type_{i}" for i in range(12)], dtype=object)
    q = pd.DataFrame({"X": rng.random(n) * 5000, "Y": rng.random(n) * 5000, "cell_type": types[rng.integers(0, 12, n)]})
    t = pd.DataFrame({"X": rng.random(n) * 5000, "Y": rng.random(n) * 5000, "cell_type": types[rng.integers(0, 12, n)]})
    return q, t


@pytest.mark.parametrize("k", [1, 8])
def test_200k_random_against_ckdtree(k):
    from same_amd.eval_utils import check_alignment

    q, t = _random(200_000, 7 + k)
    df, score, stats = check_alignment(q, t, "X", "Y", kNN=k, return_stats=True)
    match, ctype = _restatement(q, t, k)
    assert np.array_equal(df[f"_{k}NN_match"].to_numpy(), match)
    if k == 1:
        assert np.array_equal(df["_1NN_match_ctype"].to_numpy(), ctype)
    assert score == match.mean() and stats["rows_decided_on_device"] >= 0.999 * len(q)


def test_1m_run_completes_within_its_timeout():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_gpu_alignment import _random\n"
            "from same_amd.eval_utils import check_alignment\n"
            "q, t = _random(1_000_000, 3)\n"
            "df, score, st = check_alignment(q, t, 'X', 'Y', kNN=8, return_stats=True)\n"
            "assert st['rows'] == 1_000_000 and 0.0 < score < 1.0\n"
            "print('ok', score, st)\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
