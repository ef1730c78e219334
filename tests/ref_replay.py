"""Record and replay the reference's outputs for tests/test_oracle_vs_reference_fuzz.py.

Recording (only where the reference is mounted): every call the fuzz tests make into the reference goes through a Recorder, which
runs the reference and stores what it returned, plus a digest of the arguments, under the function's name.  Replaying (everywhere
else, the suite's default): a Replayer stands in for the reference namespace and hands back the stored outputs in call order,
after checking that the arguments digest to what was recorded -- so the cases the oracle is compared on are exactly the recorded
ones, or the test says so.  The stored form is data only (an .npz of arrays plus one JSON string per call; no pickle): nested
dicts / lists / tuples / sets, numpy arrays and scalars, pandas Series and DataFrames with their dtypes."""
import hashlib
import json
import types

import numpy as np
import pandas as pd


class _Enc:
    """Turns a value into a JSON-able tree; array leaves are appended to one flat buffer per dtype (`self.blobs`) and named by
    (dtype, shape, offset) in the tree."""

    def __init__(self, blobs, sort_sets=False):
        self.blobs, self.sort_sets = blobs, sort_sets

    def _nd(self, a):
        parts = self.blobs.setdefault(a.dtype.str, [])
        off = sum(len(p) for p in parts)
        parts.append(np.ascontiguousarray(a).ravel())
        return {"nd": [a.dtype.str, list(a.shape), off]}

    def _column(self, s):
        v = s.to_numpy()
        if v.dtype == object:
            return {"obj": [self(x) for x in v]}
        return self._nd(v)

    def __call__(self, v):
        if isinstance(v, np.generic):                 # before float: np.float64 is a float
            return {"np": v.dtype.str, "v": self(v.item())}
        if v is None or isinstance(v, (bool, str)):
            return v
        if isinstance(v, int):
            return {"int": str(v)}
        if isinstance(v, float):
            return {"float": float.hex(v)}
        if isinstance(v, np.ndarray):
            return {"objarr": [self(x) for x in v.ravel()], "shape": list(v.shape)} if v.dtype == object else self._nd(v)
        if isinstance(v, pd.DataFrame):
            return {"df": [self(c) for c in v.columns], "cols": [self._column(v[c]) for c in v.columns],
                    "index": self._column(v.index.to_series())}
        if isinstance(v, pd.Series):
            return {"series": self._column(v), "index": self._column(v.index.to_series()), "name": self(v.name)}
        if isinstance(v, dict):
            return {"dict": [[self(k), self(x)] for k, x in v.items()]}
        if isinstance(v, (set, frozenset)):
            items = sorted(v, key=repr) if self.sort_sets else list(v)
            return {"set": [self(x) for x in items]}
        if isinstance(v, tuple):
            return {"tuple": [self(x) for x in v]}
        if isinstance(v, list):
            return {"list": [self(x) for x in v]}
        raise TypeError(f"cannot record a {type(v).__name__}")


def _decode(t, arrays):
    if t is None or isinstance(t, (bool, str)):
        return t
    (kind, body), = ((k, t[k]) for k in t if k not in ("shape", "cols", "index", "name", "v"))
    if kind == "nd":
        dtype, shape, off = body
        return arrays[dtype][off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape).copy()
    if kind == "int":
        return int(body)
    if kind == "float":
        return float.fromhex(body)
    if kind == "np":
        return np.dtype(body).type(_decode(t["v"], arrays))
    if kind == "obj":
        out = np.empty(len(body), dtype=object)
        out[:] = [_decode(x, arrays) for x in body] if body else []
        return out
    if kind == "objarr":
        out = np.empty(len(body), dtype=object)
        out[:] = [_decode(x, arrays) for x in body] if body else []
        return out.reshape(t["shape"])
    if kind == "df":
        cols = [_decode(c, arrays) for c in body]
        index = pd.Index(_decode(t["index"], arrays))
        df = pd.DataFrame({q: pd.Series(_decode(c, arrays), index=index) for q, c in enumerate(t["cols"])}, index=index)
        df.columns = pd.Index(cols, dtype=object)
        return df
    if kind == "series":
        return pd.Series(_decode(body, arrays), index=pd.Index(_decode(t["index"], arrays)), name=_decode(t["name"], arrays))
    if kind == "dict":
        return {_decode(k, arrays): _decode(x, arrays) for k, x in body}
    if kind == "set":
        return {_decode(x, arrays) for x in body}
    if kind == "tuple":
        return tuple(_decode(x, arrays) for x in body)
    if kind == "list":
        return [_decode(x, arrays) for x in body]
    raise ValueError(f"unknown recorded kind {kind!r}")


def digest(args, kwargs):
    """A digest of a call's arguments: the structure, dtypes, shapes and bytes of every array in it."""
    blobs = {}
    tree = _Enc(blobs, sort_sets=True)((list(args), kwargs))
    h = hashlib.sha256(json.dumps(tree, sort_keys=True).encode())
    for dtype in sorted(blobs):
        for a in blobs[dtype]:
            h.update(a.tobytes())
    return h.hexdigest()


class Recorder:
    """Wraps `namespace.module.function` for the names given; `save(path)` writes what the calls returned."""

    def __init__(self, namespace, names):
        self.blobs, self.calls = {}, {}
        self.view = types.SimpleNamespace()
        for dotted in names:
            mod, fn = dotted.split(".")
            sub = getattr(self.view, mod, None)
            if sub is None:
                sub = types.SimpleNamespace()
                setattr(self.view, mod, sub)
            setattr(sub, fn, self._wrap(dotted, getattr(getattr(namespace, mod), fn)))

    def _wrap(self, dotted, fn):
        def call(*args, **kwargs):
            d = digest(args, kwargs)
            out = fn(*args, **kwargs)
            seq = self.calls.setdefault(dotted, [])
            tree = _Enc(self.blobs)(out)
            seq.append({"args": d, "out": tree})
            return out

        return call

    def save(self, path):
        dtypes = sorted(self.blobs)
        np.savez_compressed(path, calls=np.array(json.dumps(self.calls, sort_keys=True)), dtypes=np.array(dtypes),
                            **{f"blob{q}": np.concatenate(self.blobs[d]) for q, d in enumerate(dtypes)})


class Replayer:
    """The same attribute paths as a Recorder's view; every call returns the next recorded output of that function."""

    def __init__(self, path):
        with np.load(path, allow_pickle=False) as z:
            self.arrays = {str(d): z[f"blob{q}"] for q, d in enumerate(z["dtypes"])}
            self.calls = json.loads(str(z["calls"][()]))
        self.cursor = {}
        for dotted in self.calls:
            mod, fn = dotted.split(".")
            sub = getattr(self, mod, None)
            if sub is None:
                sub = types.SimpleNamespace()
                setattr(self, mod, sub)
            setattr(sub, fn, self._replay(dotted))

    def _replay(self, dotted):
        def call(*args, **kwargs):
            q = self.cursor.get(dotted, 0)
            seq = self.calls[dotted]
            assert q < len(seq), f"{dotted}: more calls than were recorded ({len(seq)})"
            assert digest(args, kwargs) == seq[q]["args"], (
                f"{dotted} call {q}: the arguments differ from the recorded ones (the seeded inputs changed: record again)")
            self.cursor[dotted] = q + 1
            return _decode(seq[q]["out"], self.arrays)

        return call

