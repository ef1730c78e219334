"""How the window path triangulates: the Qhull helper pool (the default), and two opt-in routes that give the same tables --
libsame_hip's own triangulator (`same_delaunay2d`) instead of scipy.spatial.Delaunay where that is provably the same thing, and the
device's (`same_window_delaunay`).

The reference triangulates every window's kept aligned cells with Qhull through scipy (src/same.py:1023); at ~1.6 us per point
that is three quarters of a cfg 5 pass, on the host, with the GPU waiting (`qhull_wait_share` 0.8).  libsame_hip's triangulator is
6-9 times faster, holds no GIL (plain threads instead of helper processes and pipes) and answers ONLY when its answer is beyond
doubt the SET of triangles Qhull gives (include/same_hip.h, csrc/delaunay.cpp; otherwise SAME_EUNSURE -> scipy is asked, as ever).
What it cannot give is Qhull's ORDER of the triangles and of their corners, and the reference's numbers touch that order in three
places (an XY-order edge whose ends share a coordinate; a signed area within rounding of zero; equal smallest perimeters among a
node's same-type triangles).  The device counts those places per window (`order ties`, same_window_filter_finish), and a window
with a count other than zero -- or with a cosine at the angle threshold, which the host re-decides -- is finished again with
scipy's simplices (windows.iter_device_windows).  A window's match rows, flags and sweep counters are therefore the reference's
either way; what does differ is the order of a window's kept TRIANGLES on the device (`fetch_triangles`, signs, weights), which is
why `run_same` / `sliding_window_matching` -- they hand the triangle list to the solver, index = constraint id -- keep scipy.

Use: optim_params["hip_delaunay"] = "native" (or $SAME_DELAUNAY=native) with `sliding_window_incumbent` on resident frames; the
default is "qhull".  "device" triangulates on the GPU instead (csrc/delaunay_dev.hip, same_window_delaunay): the filter's kept
triangles are the Delaunay triangles that pass it, and those are the triangles with an empty circumcircle among the ones that pass a
slack screen of it -- a local rule, one thread per point.  The device answers for the same SET as the host's triangulator does (every
sign clear of `GUARD` x Qhull's allowance, the same formula: csrc/qhull_margin.h), its candidates never leave the device
(same_window_filter_finish, SAME_TRIS_DEVICE), and a window it refuses goes to the Qhull helpers, started on the first refusal.  The ORDER rule
above is the same rule: windows.iter_device_windows re-finishes a window with order ties or a cosine at the threshold with scipy's
simplices.  `DeviceTriangulator.stats` (and `last_device_stats()` for the last pass of `sliding_window_incumbent`) count a pass's
windows submitted, refused and re-finished, each window once.

Every route is a `Triangulator` -- `QHULL` (the helper pool), windows.TriangulationCache, `NativeTriangulator`, `DeviceTriangulator`
-- and hands out `Ticket`s; that protocol is all windows.iter_device_windows knows of them.  `triangulator_for(optim_params)` picks the
route of a pass.  tests/test_delaunay_cpu.py (sets of triangles against scipy, fallbacks, tickets), tests/test_gpu_delaunay.py and
tests/test_gpu_device_delaunay.py (tables of every route bit-identical; forced ties), tests/test_gpu_delaunay_library.py (the two
device calls against their host statement, array equal, on hostile sets), tools/delaunay_margin.py (where Qhull itself stops being
exact).
"""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib, qhull_pool

# x Qhull's round-off allowance: 60 x the largest ratio (0.27) at which Qhull's triangles differed from the exact ones in 6 000
# calibration sets (an edge's property, not a set's: larger sets have smaller margins only because they have more edges) -- calibrated,
# not proven
GUARD = 16.0


def mode(optim_params=None):
    """'native' | 'device' | 'qhull' from optim_params['hip_delaunay'], else $SAME_DELAUNAY, else 'qhull'."""
    m = (optim_params or {}).get("hip_delaunay") or os.environ.get("SAME_DELAUNAY") or "qhull"
    m = str(m).lower()
    if m not in ("native", "device", "qhull"):
        raise ValueError(f"hip_delaunay / SAME_DELAUNAY must be 'native', 'device' or 'qhull', not {m!r}")
    return m


def device_filtered_triangles(points, radius, min_angle_deg, ctx=None, guard=GUARD, with_status=False):
    """(k, 3) int32 counter-clockwise triangles: the Delaunay triangles of `points` ((n, 2) float64) that pass a slack screen of the
    reference's side / angle filter -- a superset of what filter_triangles_by_radius(points, Delaunay(points).simplices, radius, ...)
    keeps, and exactly the triangles of scipy's triangulation that pass the screen -- made on the GPU (same_delaunay_filtered), or None
    when the device refuses the set (duplicates, cocircular or collinear points, no angle threshold, a list longer than its buffer: ask
    scipy).  with_status: (that, the status: 0 or a mask of _lib.SAME_DD_* reasons)."""
    import ctypes

    from . import ops
    from .triangles import cos_threshold

    ctx = ops._ctx(ctx)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(pts)
    angle_enabled, cos_thr = cos_threshold(min_angle_deg)
    out = np.empty((max(2 * n, 1), 3), np.int32)
    n_tris, status = ctypes.c_int64(0), ctypes.c_int(0)
    with ctx.lock:
        ctx.check(ctx.lib.same_delaunay_filtered(ctx.handle, pts.ctypes.data, n, float(abs(radius)), int(angle_enabled), float(cos_thr),
                                                 float(guard), out.ctypes.data, len(out), ctypes.byref(n_tris), ctypes.byref(status)),
                  "same_delaunay_filtered")
    tris = None if status.value else out[:n_tris.value].copy()
    return (tris, status.value) if with_status else tris


def native_simplices(points, guard=GUARD, with_margin=False):
    """(Tr, 3) int32 counter-clockwise triangles of the Delaunay triangulation of `points` ((n, 2) float64), or None when the library
    would not answer for Qhull (SAME_EUNSURE).  Raises when libsame_hip is missing: there is no second implementation."""
    import ctypes

    lib = _lib.load()
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(pts)
    out = np.empty((max(2 * n - 5, 1), 3), np.int32)
    n_tris, margin = ctypes.c_int64(0), ctypes.c_double(0.0)
    rc = lib.same_delaunay2d(pts.ctypes.data, n, out.ctypes.data, len(out), ctypes.byref(n_tris), float(guard), ctypes.byref(margin))
    if rc == _lib.SAME_EUNSURE:
        return (None, margin.value) if with_margin else None
    if rc != 0:
        raise _lib.SameHipError(rc, "same_delaunay2d")
    tris = out[:n_tris.value]
    return (tris, margin.value) if with_margin else tris


class Ticket:
    """One window's triangulation, whichever route makes it: a known answer, a pending one (a Qhull helper's ticket, or a native thread's
    future) or the candidates same_window_delaunay left on the device.  `.result()` = the simplices (None: the candidates on the device);
    `.native` (after `.result()`) = they are not Qhull's own, and `.qhull()` = scipy's, asked for now.  What the owner counts, it is told:
    `owner._answered` once when a pending answer arrives, `owner._refinished` when scipy's simplices replace a native answer."""

    def __init__(self, owner, points, pending=None, simplices=None, native=False, key=None):
        self.owner, self.points, self.key = owner, points, key
        self._pending, self._simplices, self.native = pending, simplices, native

    def result(self):
        if self._pending is not None:
            self._simplices, self.native = self.owner._answered(self, self._pending.result())
            self._pending = None
        return self._simplices

    def qhull(self):
        """scipy's simplices for a window whose numbers hang on Qhull's order (asked for now: nobody could know before)"""
        if self.native:
            self._simplices, self.native = qhull_pool.pool().submit(self.points).result(), False
            self.owner._refinished()
        return self.result()


class Triangulator:
    """What windows.iter_device_windows asks of a triangulation route -- every route is one of these:
      lookahead()       how many windows to stage ahead of the batch being finished
      warm              whether to start the Qhull helpers before the first window (only where they are what answers: a route that asks
                        them only for the windows it refuses starts them on the first refusal)
      submit(points, key=None) -> Ticket        at stage time; `key` is the window's id
      before_finish(states, tickets, radius, angle_enabled, cos_thr)   once per batch, right before its filter + finish call
    and, for its tickets: `_answered(ticket, what the pending answer brought) -> (simplices, native)`, `_refinished()`."""

    warm = False

    def lookahead(self):
        return 0

    def before_finish(self, states, tickets, radius, angle_enabled, cos_thr):
        pass

    def _answered(self, ticket, simplices):
        return simplices, False

    def _refinished(self):
        pass


class QhullTriangulator(Triangulator):
    """The default route: scipy's simplices from the Qhull helper pool (qhull_pool), one window ahead per helper."""

    warm = True

    def lookahead(self):
        return qhull_pool.lookahead()

    def submit(self, points, key=None):
        return Ticket(self, points, pending=qhull_pool.pool().submit(points))


QHULL = QhullTriangulator()           # (it holds nothing: the pool is the process's)


class NativeTriangulator(Triangulator):
    """`submit(points, key=None) -> ticket` like the Qhull helper pool's, answered by same_delaunay2d on a thread of this process
    (ctypes drops the GIL for the call).  `threads`: default one and a half per CPU of this process's share ($SAME_DELAUNAY_THREADS).
    A set the library leaves to Qhull goes to a Qhull helper from the triangulator's thread, windows ahead of its use.  Where most
    windows end up with scipy anyway (sections on a lattice; whole-number coordinates: order ties in every window) the triangulator
    steps aside: after `WINDOW` tickets of which more than half went back to scipy, the next `BYPASS` go to the helpers directly."""

    WINDOW, BYPASS = 16, 128

    def __init__(self, threads=None, guard=GUARD):
        from collections import deque

        if threads is None:
            # one and a half threads per CPU of this process's share (as the Qhull helpers have it): the worker threads and the runtime's
            # own threads take CPU time too, and a triangulator thread that is descheduled holds a window back.  Same lease, back to back
            # (profiles/r06_native_threads_ab.log): two ranks on 16 CPUs 4 400-4 850 windows/s with 8 threads each, 5 260-5 350 with 12;
            # one rank 3 930-4 280 with 16 and 3 630-4 330 with 24 (no difference beyond the lease's noise)
            share = qhull_pool.cpu_budget() / qhull_pool.cpu_sharers()[0]
            threads = int(os.environ.get("SAME_DELAUNAY_THREADS", "0")) or min(32, max(1, int(1.5 * share)))
        self.threads, self.guard = max(1, int(threads)), float(guard)
        self.pool = ThreadPoolExecutor(self.threads, thread_name_prefix="same-delaunay")
        self.submitted = self.asked_qhull = self.bypassed = 0
        self._recent, self._bypass, self._lock = deque(maxlen=self.WINDOW), 0, threading.Lock()
        _lib.load()

    def lookahead(self):
        return self.threads          # its own threads triangulate the windows ahead; the helpers only answer what it refuses

    def _note(self, sent_back):
        with self._lock:
            self.asked_qhull += bool(sent_back)
            self._recent.append(bool(sent_back))
            if len(self._recent) == self.WINDOW and 2 * sum(self._recent) > self.WINDOW:
                self._bypass = self.BYPASS
                self._recent.clear()

    def _work(self, pts):
        tris = native_simplices(pts, self.guard)
        if tris is not None:
            return tris, None
        return None, qhull_pool.pool().submit(pts)

    def _answered(self, ticket, answer):
        tris, asked = answer
        if tris is None:                        # left to Qhull by the library: a helper has been at it since
            tris = asked.result()
            self._note(True)
            return tris, False
        self._note(False)
        return tris, True

    def _refinished(self):
        self._note(True)

    def submit(self, points, key=None):
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        with self._lock:
            self.submitted += 1
            bypass = self._bypass > 0
            if bypass:
                self._bypass -= 1
                self.bypassed += 1
        if bypass:
            return QHULL.submit(pts)
        return Ticket(self, pts, pending=self.pool.submit(self._work, pts))

    def reset(self):
        """forget what the recent windows did (a new job may be nothing like the last)"""
        with self._lock:
            self._recent.clear()
            self._bypass = 0

    def close(self):
        self.pool.shutdown(wait=True)


_shared, _shared_lock = None, threading.Lock()


def shared():
    """The process's triangulator (threads are started once)."""
    global _shared
    with _shared_lock:
        if _shared is None:
            _shared = NativeTriangulator()
        return _shared


class DeviceTriangulator(Triangulator):
    """The route of optim_params["hip_delaunay"] = "device": the windows are triangulated on the device (same_window_delaunay) right
    before their filter + finish call, and a window the device refuses is handed to a Qhull helper (the pool is started on the first
    refusal).  `stats`: windows submitted to the device, refused by it, and re-finished with scipy's simplices after an answer (order
    ties, a cosine at the angle threshold) -- each window counted once, whichever threads walk them."""

    def __init__(self, guard=GUARD):
        self.guard = float(guard)
        self._lock = threading.Lock()
        self.stats = {"submitted": 0, "refused": 0, "refinished": 0}

    def submit(self, points, key=None):
        return Ticket(self, points, native=True)        # the device's candidates, unless before_finish finds it refused

    def before_finish(self, states, tickets, radius, angle_enabled, cos_thr):
        from ._trace import stage
        from .windows import triangulate_windows

        with stage("triangulate (device)"):
            status, _n = triangulate_windows(states, radius, angle_enabled, cos_thr, self.guard)
            for ticket, refused in zip(tickets, status.tolist()):
                if refused:                                  # a helper has it now
                    ticket.native, ticket._pending = False, qhull_pool.pool().submit(ticket.points)
            self.note(submitted=len(tickets), refused=int(np.count_nonzero(status)))

    def _refinished(self):
        self.note(refinished=1)

    def note(self, submitted=0, refused=0, refinished=0):
        with self._lock:
            self.stats["submitted"] += submitted
            self.stats["refused"] += refused
            self.stats["refinished"] += refinished


_last_device = None


def last_device_stats():
    """The counts of the last pass `sliding_window_incumbent` made with hip_delaunay = "device" in this process (None before one)."""
    return None if _last_device is None else dict(_last_device.stats)


def triangulator_for(optim_params=None):
    """The route of a pass of `sliding_window_incumbent` for mode(optim_params): "qhull" -> the helper pool (QHULL); "native" -> the
    process's NativeTriangulator (shared()), its recent history forgotten; "device" -> a fresh DeviceTriangulator, whose counts
    last_device_stats() reports."""
    global _last_device
    m = mode(optim_params)
    if m == "native":
        tr = shared()
        tr.reset()
        return tr
    if m == "device":
        _last_device = DeviceTriangulator()
        return _last_device
    return QHULL
