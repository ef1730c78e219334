"""eval_utils.check_alignment (csrc/align.hip) on the CPU: the ABI surface, the host statement of the device rule
(tests/alignment_check.py) against the reference's answers recorded in tests/golden/check_alignment.npz, the argument checks that run
before anything reaches a device, and the fixture's generator."""
import ctypes
import filecmp
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import alignment_check as ac
from conftest import ROOT, load_golden


def _cases():
    g = load_golden("check_alignment")
    for name in g["cases"]:
        name = str(name)
        q_lab = ac.decode_labels(g[f"{name}_q_kind"], g[f"{name}_q_text"])
        t_lab = ac.decode_labels(g[f"{name}_t_kind"], g[f"{name}_t_text"])
        yield g, name, g[f"{name}_q_xy"], q_lab, g[f"{name}_t_xy"], t_lab


def test_entry_point_declared_exported_and_built():
    from same_amd import _lib

    header = open(os.path.join(ROOT, "include", "same_hip.h")).read()
    assert "#define SAME_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    assert "#define SAME_ALIGN_MAX_KNN 64" in header and _lib.ALIGN_MAX_KNN == 64
    assert "int same_check_alignment(" in header and "src/eval_utils.py:6-53" in header
    assert "same_check_alignment" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "same_check_alignment")


def test_public_name():
    import same_amd
    from same_amd import eval_utils

    assert same_amd.check_alignment is eval_utils.check_alignment and "check_alignment" in same_amd.__all__


def test_label_codes_follow_python_equality():
    from same_amd.eval_utils import _label_codes

    q = np.array([1.0, 1, True, "1", None, float("nan"), "a", 0, False], dtype=object)
    t = np.array([1, "1", None, float("nan"), "a", 0.0], dtype=object)
    qc, tc = _label_codes(q, t)
    want = np.array([[a == b for b in t] for a in q])
    assert np.array_equal(qc[:, None] == tc[None, :], want)


def test_statement_reproduces_the_reference_on_decided_rows():
    from same_amd.eval_utils import _label_codes

    seen = 0
    for g, name, q_xy, q_lab, t_xy, t_lab in _cases():
        if not len(q_xy):
            continue
        qc, tc = _label_codes(q_lab, t_lab)
        for k in g[f"{name}_ks"].tolist():
            if f"{name}_k{k}_error" in g:
                continue
            flag, nearest, _, _ = ac.statement(q_xy, qc, t_xy, tc, k)
            dec = (flag & ac.DECIDED) > 0
            want = g[f"{name}_k{k}_match"].astype(bool)
            assert np.array_equal((flag[dec] & ac.MATCH) > 0, want[dec]), (name, k)
            if k == 1:
                want_ct = ac.decode_labels(g[f"{name}_k1_ctype_kind"], g[f"{name}_k1_ctype_text"])
                got = ac.encode_labels(t_lab[nearest[dec]])
                exp = ac.encode_labels(want_ct[dec])
                assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), name
            seen += int(dec.sum())
    assert seen > 10000


def test_tie_families_have_rows_in_doubt():
    from same_amd.eval_utils import _label_codes

    g = load_golden("check_alignment")
    ties = {str(n) for n in g["tie_families"]}
    in_doubt = {}
    for g, name, q_xy, q_lab, t_xy, t_lab in _cases():
        if name not in ties:
            continue
        qc, tc = _label_codes(q_lab, t_lab)
        in_doubt[name] = sum(int(((ac.statement(q_xy, qc, t_xy, tc, k)[0] & ac.DECIDED) == 0).sum()) for k in (1, 3, 8))
    assert set(in_doubt) == ties and all(v > 0 for v in in_doubt.values()), in_doubt


def _frames(n=50, seed=0):
    rng = np.random.default_rng(seed)
    q = pd.DataFrame({"X": rng.random(n), "Y": rng.random(n), "cell_type": rng.choice(["a", "b"], n)})
    return q, q.sample(frac=1.0, random_state=1).reset_index(drop=True)


@pytest.mark.parametrize("change, kw, exc, message", [
    ("drop", {}, ValueError, "must contain the columns"),
    ("nan_q", {}, ValueError, "finite"),
    ("inf_t", {}, ValueError, "finite"),
    (None, {"kNN": 0}, ValueError, "kNN"),
    (None, {"kNN": -2}, ValueError, "kNN"),
    (None, {"kNN": 2.5}, ValueError, "kNN"),
    (None, {"kNN": 65}, ValueError, "SAME_ALIGN_MAX_KNN"),
    ("small_t", {"kNN": 8}, IndexError, "out-of-bounds"),
    ("empty_t", {"kNN": 1}, IndexError, "out-of-bounds"),
])
def test_argument_errors_raise_before_any_device_work(monkeypatch, change, kw, exc, message):
    from same_amd import _lib, eval_utils, ops

    def no_device(*a, **k):
        raise AssertionError("the device was reached before the arguments were checked")

    monkeypatch.setattr(ops, "check_alignment", no_device)
    monkeypatch.setattr(_lib, "default_context", no_device)
    q, t = _frames()
    if change == "drop":
        t = t.drop(columns=["cell_type"])
    elif change == "nan_q":
        q.loc[3, "X"] = np.nan
    elif change == "inf_t":
        t.loc[5, "Y"] = np.inf
    elif change == "small_t":
        t = t.iloc[:5]
    elif change == "empty_t":
        t = t.iloc[:0]
    with pytest.raises(exc, match=message):
        eval_utils.check_alignment(q, t, "X", "Y", **kw)


def test_raises_without_a_gpu():
    """No device: the call raises like every other product function, never answers from cKDTree alone (an empty query included)."""
    from same_amd import _lib, eval_utils

    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    q, t = _frames()
    for qq in (q, q.iloc[:0]):
        with pytest.raises(_lib.SameHipError):
            eval_utils.check_alignment(qq, t, "X", "Y", kNN=3)


def test_fixture_regenerates_byte_for_byte(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from ref_loader import REF_SRC

    if not os.path.isdir(REF_SRC):
        pytest.skip("the reference is not mounted")
    env = dict(os.environ, SAME_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, "-B", os.path.join(ROOT, "tools", "gen_golden_alignment.py")], env=env, check=True,
                   capture_output=True, timeout=600)
    assert filecmp.cmp(tmp_path / "check_alignment.npz", os.path.join(ROOT, "tests", "golden", "check_alignment.npz"), shallow=False)
