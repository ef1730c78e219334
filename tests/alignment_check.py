"""Host statement of the device rule of eval_utils.check_alignment (csrc/align.hip), for small inputs, and the label coding of the
fixture tests/golden/check_alignment.npz (tools/gen_golden_alignment.py).

The rule, in numpy: d2 = dx*dx + dy*dy in fp64 against every template point; d_k = the k-th smallest; B = the points within
d_k * REL + ABS of d_k, S = the points below B.  k > 1 is decided when the label is in S (match), in no member of B (no match) or
|S| + |B| <= k (match); k == 1 only when |S| = 0 and |B| = 1, and then the nearest template row is that member of B.  A row whose
d_k is not finite (d2 overflowed) is in doubt, as in the kernel."""
import numpy as np

REL, ABS = 1e-12, 1e-300   # ALIGN_REL, ALIGN_ABS of csrc/align.hip
MATCH, DECIDED = 1, 2      # SAME_ALIGN_MATCH, SAME_ALIGN_DECIDED


def statement(qxy, qcode, txy, tcode, k, block=2048):
    """-> (flag (n_q,) uint8 [bit0 match, bit1 decided], nearest (n_q,) int32 (k == 1; -1 where in doubt) or None, |S|, |B|)."""
    qxy, txy = np.asarray(qxy, np.float64).reshape(-1, 2), np.asarray(txy, np.float64).reshape(-1, 2)
    qcode, tcode = np.asarray(qcode, np.int32), np.asarray(tcode, np.int32)
    n_q = len(qxy)
    flag = np.zeros(n_q, np.uint8)
    nearest = np.full(n_q, -1, np.int32) if k == 1 else None
    n_s, n_b = np.zeros(n_q, np.int64), np.zeros(n_q, np.int64)
    for b in range(0, n_q, block):
        q = qxy[b:b + block]
        dx = txy[None, :, 0] - q[:, None, 0]
        dy = txy[None, :, 1] - q[:, None, 1]
        with np.errstate(over="ignore", invalid="ignore"):
            d2 = dx * dx + dy * dy
            dk = np.partition(d2, k - 1, axis=1)[:, k - 1]
            m = dk * REL + ABS
            lo, hi = (dk - m)[:, None], (dk + m)[:, None]
        S, B = d2 < lo, (d2 >= lo) & (d2 <= hi)
        eq = tcode[None, :] == qcode[b:b + block, None]
        ms, mb = (S & eq).any(1), (B & eq).any(1)
        ns, nb = S.sum(1), B.sum(1)
        if k == 1:
            dec = (ns == 0) & (nb == 1)
            match = mb
            nearest[b:b + block] = np.where(dec & np.isfinite(dk), B.argmax(1), -1)
        else:
            dec = ms | ~mb | (ns + nb <= k)
            match = ms | (mb & (ns + nb <= k))
        dec = dec & np.isfinite(dk)   # the kernel's isfinite(dk) guard
        flag[b:b + block] = np.where(dec, DECIDED | np.where(match, MATCH, 0), 0)
        n_s[b:b + block], n_b[b:b + block] = ns, nb
    return flag, nearest, n_s, n_b


# ---- labels in the fixture: every label as (kind, text), so that mixed Python objects travel without pickling
KINDS = ("str", "int", "float", "bool", "none", "nan")


def encode_labels(values):
    kind, text = [], []
    for v in values:
        if v is None:
            kind.append(4), text.append("")
        elif isinstance(v, (bool, np.bool_)):
            kind.append(3), text.append(str(bool(v)))
        elif isinstance(v, (int, np.integer)):
            kind.append(1), text.append(str(int(v)))
        elif isinstance(v, (float, np.floating)):
            kind.append(5 if v != v else 2), text.append(repr(float(v)))
        else:
            kind.append(0), text.append(str(v))
    return np.array(kind, np.uint8), np.array(text, dtype=str)


def decode_labels(kind, text):
    out = np.empty(len(kind), dtype=object)
    conv = (str, int, float, lambda s: s == "True", lambda s: None, lambda s: float("nan"))
    for i, (c, s) in enumerate(zip(kind.tolist(), text.tolist())):
        out[i] = conv[c](s)
    return out
