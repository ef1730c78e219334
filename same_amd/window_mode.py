"""How a window of sliding_window_incumbent is matched, as ONE value (`WindowMode`: csrc/window_finish.hip's FinishMode on the Python
side), and the checks of the optim_params keys that choose it (`incumbent_mode`, `refine_mode`, `transport_capacity`; the keys are
described in incumbent.py's module text)."""
import functools
import numbers
from dataclasses import dataclass

import numpy as np

from . import _lib
from .params import init_gurobi_params, init_optim_params

INCUMBENTS = ("greedy", "assignment", "transport")          # optim_params["hip_incumbent"]; "greedy" without the key
REFINES = ("local", "capacity")               # optim_params["hip_refine"]; None without the key
CALLER_DELAUNAY = (None, "host", "device")    # optim_params["hip_caller_delaunay"]; None without the key
PRIORITY_PRUNE = (None, "host", "device")     # optim_params["hip_priority_prune"]; None without the key
REFINE_ROUNDS = 32                             # optim_params["hip_refine_rounds"] without the key
_CODES = dict(zip(INCUMBENTS, (_lib.SAME_INCUMBENT_GREEDY, _lib.SAME_INCUMBENT_ASSIGNMENT, _lib.SAME_INCUMBENT_TRANSPORT)))


@dataclass(frozen=True)
class WindowMode:
    """`incumbent`: the start -- "greedy" (src/init_helpers.py:104-133), "assignment" (the optimal one-to-one assignment, csrc/assign.hip)
    or "transport" (the optimum of the model without its triangle term within `capacity`; the same kernel's transport form).
    `refine`: the local search on the lazy model's objective from that start, before the sweeps (csrc/refine.hip) -- None, "local"
    (one-to-one) or "capacity" (within `capacity`) -- for at most `rounds` rounds at `delaunay_penalty`; rounds 0 without a search.
    `capacity` = (max_matches, ref_metacell_match_multiplier or None, penalty_coeff), the model's reference capacities: there exactly
    when the start or the search reads them.  "transport" does not go with "local"."""

    incumbent: str = "greedy"
    refine: str = None
    rounds: int = 0
    delaunay_penalty: float = 0.0
    capacity: tuple = None

    def __post_init__(self):
        if self.incumbent not in INCUMBENTS or self.refine not in (None,) + REFINES or (self.refine is None) != (self.rounds == 0):
            raise ValueError(f"not a window mode (a start of {INCUMBENTS}, a search of {REFINES} or None, rounds >= 1 with one): {self}")
        if self.incumbent == "transport" and self.refine == "local":
            raise ValueError("hip_refine='local' keeps every reference to one match; on hip_incumbent='transport' use "
                             "hip_refine='capacity'")
        if self.capacity is None and self.incumbent == "transport":
            raise ValueError("incumbent='transport' needs its capacity, and a refine on it the same one")
        if self.capacity is None and self.refine == "capacity":
            raise ValueError("refine='capacity' needs its capacity")
        if self.capacity is not None and self.incumbent != "transport" and self.refine != "capacity":
            raise ValueError("capacity goes with incumbent='transport'")

    @classmethod
    def default(cls):
        """the greedy start, no search: what `mode=None` means everywhere"""
        return _DEFAULT

    @classmethod
    def from_params(cls, optim_params, gurobi_params=None, moving=None):
        """The mode that optim_params["hip_incumbent"] / ["hip_refine"] ask for, every key checked before anything reaches a device:
        the checks of `incumbent_mode`, `refine_mode` and `transport_capacity`, in that order, over one completion of the params."""
        op = _Params.of(optim_params)
        incumbent, search, capacity = incumbent_mode(op, gurobi_params, moving), refine_mode(op), transport_capacity(op)
        caller_delaunay_route(op)
        priority_prune_route(op)
        if search is None:
            return cls(incumbent, capacity=capacity)
        return cls(incumbent, op["hip_refine"], *search[:2], search[2] if op["hip_refine"] == "capacity" else capacity)

    @property
    def incumbent_code(self):
        return _CODES[self.incumbent]

    @property
    def search_args(self):
        """the library's (rounds_cap, delaunay_penalty); rounds_cap 0 = no search"""
        return int(self.rounds), float(self.delaunay_penalty)

    def c_capacity(self):
        """the library's same_window_capacity, None without one"""
        if self.capacity is None:
            return None
        mm, mult, pc = self.capacity
        return _lib.WindowCapacity(int(mm), 0 if mult is None else int(mult), float(pc))

    @property
    def finish_width(self):
        """int64 words of a window's stats record from the finish call"""
        if self.capacity is None:
            return _lib.SAME_WINDOW_STATS
        return _lib.SAME_WINDOW_STATS_TRANSPORT if self.incumbent == "transport" else _lib.SAME_WINDOW_STATS_CAP

    @property
    def refinish_width(self):
        """... and from the re-finish call, which runs no start"""
        return _lib.SAME_WINDOW_STATS_CAP if self.refine == "capacity" else _lib.SAME_WINDOW_STATS

    def records(self, s, start=True):
        """a window's stats words -> (the start's record {"rounds", "flags", "objective"[, "ref_extra_matches_start"]}, the search's
        record {"rounds", "moves", "settled", "objective_start", "objective"[, "ref_extra_matches"]}), each None when the mode has none.
        `s` holds `finish_width` words.  A re-finish ran no start and hands in only `refinish_width` words: it MUST pass start=False
        (the start's record is then None; the transport start's word 16 is not there to be read)."""
        f = s.view(np.float64)
        asg = {"rounds": int(s[6]), "flags": int(s[8]), "objective": float(f[9])} if start and self.incumbent != "greedy" else None
        if asg is not None and self.incumbent == "transport":        # (SAME_WINDOW_STATS_TRANSPORT words)
            asg["ref_extra_matches_start"] = int(s[16])
        rfn = None if self.refine is None else {"rounds": int(s[10]), "moves": int(s[11]), "settled": int(s[12]),
                                                "objective_start": float(f[13]), "objective": float(f[14])}
        if self.refine == "capacity":                                # (SAME_WINDOW_STATS_CAP words)
            rfn["ref_extra_matches"] = int(s[15])
        return asg, rfn


_DEFAULT = WindowMode()


class _Params(dict):
    """the caller's optim_params; `.full`: completed by init_optim_params, on first need and once"""

    @functools.cached_property
    def full(self):
        return init_optim_params(**self)

    @classmethod
    def of(cls, optim_params):
        return optim_params if isinstance(optim_params, cls) else cls(optim_params or {})


def incumbent_mode(optim_params, gurobi_params=None, moving=None):
    """optim_params["hip_incumbent"] checked before anything reaches a device -> "greedy" | "assignment" | "transport".  The assignment
    is the reference's Hungarian start (src/init_helpers.py:135-175) without its size cap: it needs max_matches == 1 (:97-98, the
    reference's own message), and it equals the reference's dense big-M problem only while every no-match cost no_match_penalty * size is
    below init_big_m / 2 (gurobi_params), which is checked over every aligned cell of `moving`.  The transport start takes any
    max_matches >= 1; its penalty_coeff, max_matches and ref_metacell_match_multiplier pass the checks of hip_refine="capacity"
    (`transport_capacity` gives the triple)."""
    from .window_api import ResidentFrames

    op = _Params.of(optim_params)
    mode = op.get("hip_incumbent", "greedy")
    if not isinstance(mode, str) or mode not in INCUMBENTS:
        raise ValueError(f"optim_params['hip_incumbent'] must be one of {INCUMBENTS}, not {mode!r}")
    if mode == "greedy":
        return mode
    if mode == "transport":
        _capacity_of(op.full, "hip_incumbent='transport'")
        return mode
    if op.full["max_matches"] != 1:
        raise ValueError("init_method='hungarian' requires max_matches == 1.")
    big_m = float(init_gurobi_params(**dict(gurobi_params or {}))["init_big_m"])
    frame = moving.moving_arg if isinstance(moving, ResidentFrames) else moving
    frame = getattr(frame, "metacell_df", frame)
    if frame is not None and len(frame):
        size = frame["size"].to_numpy(dtype=np.float64) if "size" in frame.columns else np.ones(1)
        worst = float(op.full["no_match_penalty"]) * size
        if not np.all(worst < big_m / 2):
            raise ValueError(f"hip_incumbent='assignment': a no-match cost no_match_penalty * size ({np.nanmax(worst):g}) is not below "
                             f"init_big_m / 2 ({big_m / 2:g}); the sparse problem would differ from the reference's big-M one")
    return mode


def caller_delaunay_route(optim_params):
    """optim_params["hip_caller_delaunay"] checked -> "host" (None or without the key: a caller's triangulation takes the general route
    of sliding_window_incumbent, window by window on the host) | "device" (it stays on the device route: csrc/window_caller.hip)"""
    route = (optim_params or {}).get("hip_caller_delaunay")
    if not (route is None or isinstance(route, str)) or route not in CALLER_DELAUNAY:
        raise ValueError(f"optim_params['hip_caller_delaunay'] must be None, 'host' or 'device', not {route!r}")
    return "host" if route is None else route


def priority_prune_route(optim_params):
    """optim_params["hip_priority_prune"] checked -> "host" (None or without the key: a job with ignore_knn_if_matched takes the general
    route of sliding_window_incumbent, its pairs filtered window by window on the host) | "device" (it stays on the device route:
    csrc/window_priority.hip).  Without ignore_knn_if_matched the key changes nothing."""
    route = (optim_params or {}).get("hip_priority_prune")
    if not (route is None or isinstance(route, str)) or route not in PRIORITY_PRUNE:
        raise ValueError(f"optim_params['hip_priority_prune'] must be None, 'host' or 'device', not {route!r}")
    return "host" if route is None else route


def _capacity_of(full, what):
    """(max_matches, ref_metacell_match_multiplier or None, penalty_coeff) of the completed optim_params `full`, checked for `what`
    (hip_refine="capacity" and hip_incumbent="transport" read the model's reference capacities by the same rule)"""
    pc, mm, mult = full["penalty_coeff"], full["max_matches"], full["ref_metacell_match_multiplier"]
    if isinstance(pc, bool) or not isinstance(pc, numbers.Real) or not np.isfinite(float(pc)) or float(pc) < 0:
        raise ValueError(f"optim_params['penalty_coeff'] must be finite and >= 0 for {what}, not {pc!r}")
    if isinstance(mm, bool) or not isinstance(mm, numbers.Integral) or mm < 1:
        raise ValueError(f"optim_params['max_matches'] must be an int >= 1 for {what}, not {mm!r}")
    if mult is not None and (isinstance(mult, bool) or not isinstance(mult, numbers.Integral) or mult < 1):
        raise ValueError(f"optim_params['ref_metacell_match_multiplier'] must be None or an int >= 1 for {what}, "
                         f"not {mult!r}")
    return int(mm), None if mult is None else int(mult), float(pc)


def transport_capacity(optim_params):
    """the capacity triple of hip_incumbent="transport" (checked), None for the other starts"""
    op = _Params.of(optim_params)
    if op.get("hip_incumbent", "greedy") != "transport":
        return None
    return _capacity_of(op.full, "hip_incumbent='transport'")


def refine_mode(optim_params):
    """optim_params["hip_refine"] / ["hip_refine_rounds"] / ["delaunay_penalty"] (and for "capacity" ["penalty_coeff"] /
    ["max_matches"] / ["ref_metacell_match_multiplier"]) checked before anything reaches a device -> None (no search),
    (rounds_cap, delaunay_penalty) ("local") or (rounds_cap, delaunay_penalty, (max_matches, multiplier or None, penalty_coeff))"""
    op = _Params.of(optim_params)
    mode = op.get("hip_refine")
    if mode is None:
        return None
    if not isinstance(mode, str) or mode not in REFINES:
        raise ValueError(f"optim_params['hip_refine'] must be None or one of {REFINES}, not {mode!r}")
    cap = op.get("hip_refine_rounds", REFINE_ROUNDS)
    if isinstance(cap, bool) or not isinstance(cap, numbers.Integral) or cap < 1:
        raise ValueError(f"optim_params['hip_refine_rounds'] must be a positive int, not {cap!r}")
    dp = op.full["delaunay_penalty"]
    if isinstance(dp, bool) or not isinstance(dp, numbers.Real) or not np.isfinite(float(dp)) or float(dp) < 0:
        raise ValueError(f"optim_params['delaunay_penalty'] must be finite and >= 0 for hip_refine, not {dp!r}")
    if mode == "local":
        return int(cap), float(dp)
    return int(cap), float(dp), _capacity_of(op.full, "hip_refine='capacity'")
