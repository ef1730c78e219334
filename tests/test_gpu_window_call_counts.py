"""What the window path's five pair-list calls ask of the HIP runtime (csrc/window_stage.hip's batch driver): launches, fills, copies
and waits of every call of one sweep sequence over ONE batch of nine windows -- more than a launch group of 8, one window whose box
holds rows of both sections and keeps none (no kept row, no pair: it drops out of the live list of every call after the stage call) -- on
the base case of tests/caller_check.py.  The calls share one driver; a change to it that adds or drops a launch, a copy or a wait shows
here as a changed tuple."""
import numpy as np
import pytest

import caller_check as C

pytestmark = pytest.mark.gpu

K_SMALL = 3

# eight boxes of at most 64 cells of the cell-25 grid (the cell-run path: a whole-section box would wait inside its stage call), unions
# of cells and boxes that cut through them, and EMPTY_BOX in the middle of the first launch group
BOXES = [(100.0, 200.0, 100.0, 200.0), (150.0, 152.0, 0.0, 300.0), (0.0, 100.0, 0.0, 100.0), C.EMPTY_BOX, (37.0, 150.0, 12.0, 160.0),
         (200.0, 300.0, 150.0, 300.0), (10.0, 35.0, 10.0, 35.0), (120.0, 290.0, 30.0, 110.0), (55.5, 95.5, 205.0, 290.0)]

# (launches, fills, copies, waits) per call, as observed with this very test body on the library of commit ad2fd1b (the last one
# before the calls were given one batch driver) on an MI355X: the driver must ask the runtime for exactly what the five hand-written
# copies of the batch skeleton asked for
EXPECTED = {
    "stage": (14, 0, 0, 1),                   # two launch groups: 9 windows
    "priority": (6, 0, 0, 1),                 # one group from here on: 8 live windows
    "caller_tris": (9, 0, 0, 1),
    "prefix k=3": (4, 0, 0, 1),
    "priority again": (6, 0, 0, 1),
    "caller_pairs": (4, 0, 0, 1),
    "prefix staged k": (0, 0, 8, 1),          # no launch: the staged counts, XY and rows of the 8 compacted windows, a copy each
}


def test_one_sweep_sequence_asks_the_runtime_for_what_it_always_did(oracle):
    from same_amd import windows as W
    from same_amd.triangles import cos_threshold

    case, codes = C.base_case(), C.base_codes()
    mov = W.Section(case["mov_xy"], case["types_m"], case["type_id"], case["size"])
    ref = W.Section(case["ref_xy"], case["types_r"], None, None)
    dmov, dref = W.DeviceSection(mov, np.float64), W.DeviceSection(ref, np.float64)
    dmov.set_label_codes(codes["code_m"])
    dref.set_label_codes(codes["code_r"])
    dmov.bin(*C.GRIDS["cell 25"])
    dref.bin(*C.GRIDS["cell 25"])
    caller = W.DeviceCallerTris(dmov, case["tris"])
    en, thr = cos_threshold(15)
    states = [W.DeviceWindow() for _ in BOXES]
    ctx = states[0].ctx
    seen = {}

    def counted(name, call, *args):
        before = ctx.stats()
        out = call(states, *args)
        after = ctx.stats()
        seen[name] = tuple(after[w] - before[w] for w in ("launches", "fills", "copies", "waits"))
        return out

    try:
        # the radius is known to the reference's prune index before anything is counted (built once per section and radius)
        states[0].stage(dmov, dref, BOXES[0], C.RADIUS, C.KNN, 1.0)
        staged = counted("stage", W.stage_windows, dmov, dref, BOXES, C.RADIUS, C.KNN, 1.0)
        assert [c[2] > 0 and c[3] > 0 for c in staged] == [b != C.EMPTY_BOX for b in BOXES] and all(c[0] > 0 and c[1] > 0 for c in staged)
        counted("priority", W.priority_windows)
        got = counted("caller_tris", W.caller_tris_windows, caller, C.RADIUS, en, thr, float(8 * np.spacing(abs(thr))), True)
        assert all(g[2] == 0 for g in got)                         # no cosine at the threshold: every window is compacted
        counted(f"prefix k={K_SMALL}", W.prefix_windows, K_SMALL)
        counted("priority again", W.priority_windows)
        counted("caller_pairs", W.caller_pairs_windows)
        counted("prefix staged k", W.prefix_windows, C.KNN)
    finally:
        for s in states:
            s.close()
        caller.close()
        dmov.close()
        dref.close()
    print("observed:", seen)
    assert seen == EXPECTED
    assert all(v[3] == 1 for k, v in seen.items() if k != "prefix staged k")
