"""What the barebone mirror (mppi_numba_amd/barebone.py) sends to the library: which calls, with which arguments, in
which order -- and when it sends nothing.  No device and no built library: barebone.py reaches the library through
_lib.call and _lib.ptr alone, looked up on the module at call time, and both are replaced by a recorder here.

A scenario is a short script of public calls and edits of `params`.  After every step it keeps the calls made, the
ValueError raised (its message) and track_offset.  The recorder answers mppi_planner_get_track_offsets with FETCHED (not
0), so that an offset fetched from the library and one zeroed by the mirror can be told apart.

The expected traces, tests/golden/barebone_mirror_calls.json, were recorded at commit bc1f000 -- before the mirror's
bookkeeping became one record per held set and one table-driven sync routine -- by running this module as a script
against that checkout.  They are not regenerated from the code under test: a different trace means the code is wrong."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mppi_numba_amd import _lib, barebone  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "barebone_mirror_calls.json")
FETCHED = 5  # what the recorder's library answers a fetch of the track offsets with
B = 2

# arguments the library writes: they are rendered as dtype and shape alone (the mirror hands over uninitialised memory)
OUTPUTS = {"mppi_planner_solve": (2,), "mppi_planner_closed_loop": (7, 8, 9)}  # (and every array of a mppi_planner_get_*)


def render(arg, output=False):
    if arg is None or isinstance(arg, (bool, int, float, str)):
        return arg
    if isinstance(arg, np.ndarray):
        out = {"dtype": arg.dtype.str, "shape": list(arg.shape)}
        if not output:
            out["data"] = arg.tolist()
        return out
    if isinstance(arg, C.Structure):
        return {name: render(getattr(arg, name)) for name, _ in arg._fields_ if not name.startswith("_")}
    if isinstance(arg, C.Array):
        return list(arg)
    if isinstance(arg, C._SimpleCData):
        return arg.value
    if hasattr(arg, "_obj"):  # a byref
        return render(arg._obj)
    raise TypeError("an argument the recorder cannot render: {!r}".format(arg))


class Recorder:
    def __init__(self):
        self.log = []

    def call(self, name, *args):
        args = [a for a in args if not isinstance(getattr(a, "_obj", a), C.c_void_p)]  # the handle is left out
        outputs = range(len(args)) if name.startswith("mppi_planner_get_") else OUTPUTS.get(name, ())
        self.log.append([name] + [render(a, i in outputs) for i, a in enumerate(args)])
        if name == "mppi_planner_get_track_offsets":
            args[1][:] = FETCHED

    def drain(self):
        log, self.log = self.log, []
        return log


class Run:
    """One scenario: the planner under test and the steps taken so far."""

    def __init__(self, recorder):
        self.recorder, self.steps, self.planner = recorder, [], None

    def make(self, batch=False):
        cfg = barebone.Config(T=0.4, dt=0.1, num_control_rollouts=64, num_vis_state_rollouts=2, seed=1,
                              enforce_recommended_limits=False, crowd=True)
        assert cfg.num_steps == 4
        self.step("construct", lambda: setattr(self, "planner", barebone.MPPI_Batch(cfg, B) if batch else barebone.MPPI_Numba(cfg)))
        return self.planner

    def step(self, label, action):
        error = None
        try:
            action()
        except ValueError as exc:
            error = str(exc)
        offset = self.planner.track_offset
        self.steps.append({"step": label, "calls": self.recorder.drain(), "error": error,
                           "track_offset": offset if isinstance(offset, int) else offset.tolist()})

    def value(self, label, get):
        """A public attribute or property, rendered beside the calls it made."""
        got = get()
        got = [render(g) for g in got] if isinstance(got, (list, tuple)) else render(got)
        self.steps.append({"step": label, "calls": self.recorder.drain(), "value": got})

    def close(self):
        self.planner._handle = None  # (so that __del__ does not reach for a real library)
        self.recorder.drain()
        return self.steps


# ---------------------------------------------------------------------------------------------------- values
def arr(values, dtype=np.float64):
    return np.array(values, dtype=dtype)


def base(**more):
    p = dict(dt=0.1, x0=arr([0.0, 0.25, 0.5]), xgoal=arr([2.0, 1.0]), goal_tolerance=0.25, dist_weight=10, lambda_weight=1.0,
             num_opt=1, u_std=arr([0.5, 0.25]), vrange=arr([0.0, 1.0]), wrange=arr([-1.0, 1.0]),
             obstacle_positions=arr([[1.0, 1.0], [1.5, 0.5]]), obstacle_radius=arr([0.25, 0.5]), obs_penalty=100.0)
    p.update(more)
    return p


def without(params, *keys):
    return {k: v for k, v in params.items() if k not in keys}


TRACKS = [[[1.0, 1.0], [1.25, 1.0], [1.5, 1.0]], [[1.5, 0.5], [1.5, 0.75], [1.5, 1.0]]]            # (K, L, 2) = (2, 3, 2)
SAMPLES = [TRACKS, [[[1.0, 1.0], [1.0, 1.25], [1.0, 1.5]], [[1.5, 0.5], [1.25, 0.5], [1.0, 0.5]]]]   # (S, K, L, 2)
WALLS = [[[0.0, 2.0], [2.0, 2.0]], [[2.0, 2.0], [2.0, 0.0]]]                                      # (W, 2, 2)
WALL_TRACKS = [[[[0.0, 2.0], [2.0, 2.0]], [[0.0, 1.75], [2.0, 1.75]], [[0.0, 1.5], [2.0, 1.5]]],
               [[[2.0, 2.0], [2.0, 0.0]], [[1.75, 2.0], [1.75, 0.0]], [[1.5, 2.0], [1.5, 0.0]]]]  # (W, L, 2, 2)
GOAL_TRACK = [[2.0, 1.0], [2.25, 1.0], [2.5, 1.0]]                                                # (L, 2)
FOOTPRINT = [[0.25, 0.0, 0.125], [-0.25, 0.0, 0.125]]                                             # (F, 3)
RINGS = [[0.25, 4.0], [0.5, 1.0]]                                                                 # (R, 2)
X0S = [[0.0, 0.25, 0.5], [0.5, 0.0, 0.25]]
GOALS = [[2.0, 1.0], [1.0, 2.0]]


def changed(values, dtype=np.float64):
    out = arr(values, dtype)
    out.reshape(-1)[-1] += 0.125
    return out


def cycle(r, key, values, restore=None):
    """The life of one params-owned kind: first hand-over, the same values in a fresh array (nothing), a control step,
    one float changed, the same values with another dtype, the key removed (`restore`: what comes back in its place),
    and a solve after that."""
    pl = r.planner
    pl.params[key] = arr(values)
    r.step(key + " first", pl.solve)
    pl.params[key] = arr(values)
    r.step(key + " fresh array", pl.solve)
    r.step(key + " control step", lambda: pl.shift_and_update(arr(X0S[0]), np.zeros((4, 2), np.float32)))
    pl.params[key] = changed(values)
    r.step(key + " one float changed", pl.solve)
    pl.params[key] = changed(values, np.float32)
    r.step(key + " another dtype", pl.solve)
    del pl.params[key]
    pl.params.update(restore or {})
    r.step(key + " removed", pl.solve)
    r.step(key + " removed, again", pl.rollout)


def refusals(r, key, bad, **more):
    """Values of `key` that its pack function refuses, each in a solve of its own."""
    pl = r.planner
    for label, value in bad:
        pl.params.update(more)
        pl.params[key] = value
        r.step("{} refused: {}".format(key, label), pl.solve)
    del pl.params[key]


def single(r, **more):
    pl = r.make()
    params = base(**more)
    r.step("setup", lambda: pl.setup(params))
    return pl


def batch(r, params=None, **sets):
    pl = r.make(batch=True)
    params = base() if params is None else params
    r.step("setup", lambda: pl.setup(params, arr(X0S), arr(GOALS), **sets))
    return pl


# ---------------------------------------------------------------------------------------------------- scenarios
def static_discs(r):
    pl = single(r)
    r.step("first solve", pl.solve)
    r.step("second solve", pl.solve)
    cycle(r, "obstacle_positions", [[1.0, 1.0], [1.5, 0.5]])
    pl.params["obstacle_positions"] = arr([[1.0, 1.0], [1.5, 0.5]])
    r.step("positions back", pl.solve)
    pl.params["obstacle_radius"] = arr([0.25, 0.5], np.float32)
    r.step("radii of another dtype", pl.solve)
    del pl.params["obstacle_radius"]
    r.step("positions without radii", pl.solve)
    pl.params["obstacle_radius"] = arr([0.25, 0.75])
    r.step("radii back, one changed", pl.get_state_rollout)
    r.step("update", pl.update)
    r.step("sample_noise", pl.sample_noise)


def no_discs_at_first(r):
    pl = single(r)
    pl.params = without(pl.params, "obstacle_positions", "obstacle_radius", "obs_penalty", "dist_weight")
    r.step("first solve, no discs", pl.solve)
    r.step("second solve, no discs", pl.solve)
    pl.params["cvar_alpha"] = 0.5
    r.step("cvar_alpha without samples", pl.solve)
    pl.params["cvar_alpha"] = 1.5
    r.step("cvar_alpha out of range", pl.solve)


def disc_tracks(r):
    pl = single(r)
    r.step("static discs first", pl.solve)
    del pl.params["obstacle_positions"]
    cycle(r, "obstacle_tracks", TRACKS, restore={"obstacle_positions": arr([[1.0, 1.0], [1.5, 0.5]])})
    pl.params["obstacle_tracks"] = arr(TRACKS)
    r.step("both positions and tracks", pl.solve)
    del pl.params["obstacle_positions"]
    r.step("tracks alone", pl.solve)
    pl.params["obstacle_radius"] = arr([0.25, 0.75])
    r.step("radii changed", pl.solve)
    refusals(r, "obstacle_tracks", [("(K, L, 3)", np.zeros((2, 3, 3))), ("no rows", np.zeros((2, 0, 2))),
                                    ("three tracks, two radii", np.zeros((3, 2, 2)))])
    r.step("tracks removed, no positions", pl.solve)
    pl.params["obstacle_tracks"] = arr(TRACKS)[:, :1]
    r.step("tracks of one row", pl.solve)
    r.step("control step with tracks of one row", lambda: pl.shift_and_update(arr(X0S[0]), np.zeros((4, 2), np.float32), 2))


def disc_samples(r):
    pl = single(r, cvar_alpha=0.5)
    r.step("static discs first", pl.solve)
    r.step("sample_costs without samples", pl.sample_costs)
    del pl.params["obstacle_positions"]
    cycle(r, "obstacle_track_samples", SAMPLES, restore={"obstacle_positions": arr([[1.0, 1.0], [1.5, 0.5]])})
    del pl.params["obstacle_positions"]
    pl.params["obstacle_track_samples"] = arr(SAMPLES)
    r.step("samples again", pl.solve)
    r.step("record_sample_costs", pl.record_sample_costs)
    r.step("sample_costs", pl.sample_costs)
    pl.params["obstacle_radius"] = arr([0.25, 0.75])
    r.step("radii changed", pl.solve)
    pl.params["obstacle_positions"] = arr([[1.0, 1.0]])
    r.step("samples and positions", pl.solve)
    del pl.params["obstacle_positions"]
    pl.params["obstacle_tracks"] = arr(TRACKS)
    r.step("samples and tracks", pl.solve)
    del pl.params["obstacle_tracks"]
    refusals(r, "obstacle_track_samples", [("(K, L, 2)", np.zeros((2, 3, 2))), ("no rows", np.zeros((2, 2, 0, 2))),
                                           ("17 samples", np.zeros((17, 2, 1, 2))), ("three discs, two radii", np.zeros((1, 3, 1, 2)))])
    pl.params["obstacle_tracks"] = arr(TRACKS)
    r.step("samples removed, plain tracks in their place", pl.solve)
    r.step("control step", lambda: pl.shift_and_update(arr(X0S[0]), np.zeros((4, 2), np.float32)))
    del pl.params["obstacle_tracks"]
    pl.params["obstacle_track_samples"] = np.zeros((2, 2, 0, 2))
    r.step("bad samples while plain tracks are held", pl.solve)
    pl.params["obstacle_track_samples"] = arr(SAMPLES)
    r.step("samples while plain tracks are held", pl.solve)
    pl.params = without(pl.params, "obstacle_track_samples", "obstacle_radius")
    r.step("samples removed, no discs", pl.solve)


def static_walls(r):
    pl = single(r, wall_halfwidth=0.125)
    r.step("a half-width without walls", pl.solve)
    cycle(r, "wall_segments", WALLS)
    pl.params["wall_segments"] = arr(WALLS)
    r.step("walls back", pl.solve)
    pl.params["wall_halfwidth"] = arr([0.125, 0.25])
    r.step("a half-width per wall", pl.solve)
    pl.params["wall_halfwidth"] = arr([0.125, 0.25], np.float32)
    r.step("half-widths of another dtype", pl.solve)
    pl.params["wall_halfwidth"] = arr([0.125, 0.25, 0.5])
    r.step("three half-widths, two walls", pl.solve)
    del pl.params["wall_halfwidth"]
    r.step("no half-width", pl.solve)
    refusals(r, "wall_segments", [("(W, 2, 3)", np.zeros((2, 2, 3)))])
    r.step("walls removed", pl.solve)


def wall_tracks(r):
    pl = single(r, wall_halfwidth=0.125)
    r.step("first solve", pl.solve)
    cycle(r, "wall_tracks", WALL_TRACKS, restore={"wall_segments": arr(WALLS)})
    pl.params["wall_tracks"] = arr(WALL_TRACKS)
    r.step("both wall_segments and wall_tracks", pl.solve)
    del pl.params["wall_segments"]
    r.step("wall tracks in place of walls", pl.solve)
    pl.params["wall_segments"] = arr(WALLS)
    r.step("wall_segments beside wall tracks that are held", pl.solve)
    del pl.params["wall_segments"]
    pl.params["wall_halfwidth"] = arr([0.125, 0.25])
    r.step("a half-width per wall", pl.solve)
    refusals(r, "wall_tracks", [("(W, 2, 2)", np.zeros((2, 2, 2))), ("(W, L, 2, 3)", np.zeros((2, 3, 2, 3))),
                                ("no rows", np.zeros((2, 0, 2, 2))), ("three walls, two half-widths", np.zeros((3, 2, 2, 2)))])
    r.step("wall tracks removed", pl.solve)
    pl.params["wall_tracks"] = arr(WALL_TRACKS)[:, :1]
    r.step("wall tracks of one row", pl.solve)
    r.step("control step with wall tracks of one row", lambda: pl.shift_and_update(arr(X0S[0]), np.zeros((4, 2), np.float32)))


def goal_track(r):
    pl = single(r)
    r.step("first solve", pl.solve)
    r.value("goal_now, static", lambda: pl.goal_now)
    del pl.params["xgoal"]
    pl.params["goal_track"] = arr(GOAL_TRACK)
    r.value("goal_now ahead of the hand-over", lambda: pl.goal_now)
    cycle(r, "goal_track", GOAL_TRACK, restore={"xgoal": arr([2.0, 1.0])})
    pl.params["goal_track"] = arr(GOAL_TRACK)
    r.step("both xgoal and goal_track", pl.solve)
    del pl.params["xgoal"]
    r.step("goal track alone", pl.solve)
    r.step("control step", lambda: pl.shift_and_update(arr(X0S[0]), np.zeros((4, 2), np.float32), 2))
    r.value("goal_now two rows on", lambda: pl.goal_now)
    refusals(r, "goal_track", [("(L, 3)", np.zeros((3, 3))), ("(L,)", np.zeros(4)), ("no rows", np.zeros((0, 2)))])
    pl.params["goal_track"] = arr(GOAL_TRACK)[:1]
    r.step("a goal track of one row", pl.solve)
    r.step("control step with a goal track of one row", lambda: pl.shift_and_update(arr(X0S[0]), np.zeros((4, 2), np.float32)))
    del pl.params["goal_track"]
    pl.params["xgoal"] = arr([2.0, 1.0])
    r.step("goal track removed", pl.solve)


def footprint(r):
    pl = single(r)
    r.step("first solve", pl.solve)
    cycle(r, "footprint", FOOTPRINT)
    refusals(r, "footprint", [("nine discs", np.zeros((9, 3))), ("(F, 2)", np.zeros((2, 2))), ("no discs", np.zeros((0, 3)))])
    r.step("after the refusals", pl.solve)


def clearance_rings(r):
    pl = single(r)
    r.step("first solve", pl.solve)
    cycle(r, "clearance_rings", RINGS)
    refusals(r, "clearance_rings", [("five rings", np.zeros((5, 2))), ("(R, 3)", np.zeros((2, 3)))])
    r.step("after the refusals", pl.solve)


def noise_smoothing(r):
    pl = single(r)
    r.step("first solve", pl.solve)
    cycle(r, "noise_smoothing", 0.5)
    cycle(r, "noise_smoothing", [0.5, 0.25])
    refusals(r, "noise_smoothing", [("(3,)", np.zeros(3)), ("(1, 2)", np.zeros((1, 2)))])
    r.step("after the refusals", pl.solve)


def rings_and_samples(r):
    pl = single(r, clearance_rings=arr(RINGS))
    r.step("rings first", pl.solve)
    del pl.params["clearance_rings"], pl.params["obstacle_positions"]
    pl.params["obstacle_track_samples"] = arr(SAMPLES)
    r.step("rings go, samples come", pl.solve)
    del pl.params["obstacle_track_samples"]
    pl.params.update(clearance_rings=arr(RINGS), obstacle_positions=arr([[1.0, 1.0], [1.5, 0.5]]))
    r.step("samples go, rings come", pl.solve)
    pl.params.update(obstacle_track_samples=arr(SAMPLES))
    del pl.params["obstacle_positions"]
    r.step("samples beside rings that are held (the library refuses; the recorder does not)", pl.solve)


def everything_at_once(r):
    pl = single(r)
    every = dict(goal_track=arr(GOAL_TRACK), noise_smoothing=0.5, wall_tracks=arr(WALL_TRACKS), wall_halfwidth=0.125,
                 footprint=arr(FOOTPRINT), clearance_rings=arr(RINGS), obstacle_tracks=arr(TRACKS))
    pl.params = without(dict(pl.params, **every), "xgoal", "obstacle_positions")
    r.step("every kind in one solve", pl.solve)
    r.step("nothing changed", pl.solve)
    r.step("control step", lambda: pl.shift_and_update(arr(X0S[0]), np.zeros((4, 2), np.float32)))
    pl.params = dict(without(pl.params, *every), xgoal=arr([2.0, 1.0]), wall_segments=arr(WALLS), wall_halfwidth=0.125,
                     obstacle_track_samples=arr(SAMPLES))
    r.step("every kind gone or exchanged in one solve", pl.solve)
    r.step("reset", pl.reset)
    r.step("setup after reset", lambda: pl.setup(base(wall_segments=arr(WALLS), wall_halfwidth=0.125)))
    r.step("solve after reset: what is held is still known", pl.solve)


def closed_loop(r):
    pl = single(r)
    r.step("closed loop, static goal", lambda: pl.closed_loop(3))
    pl.params = dict(without(pl.params, "xgoal"), goal_track=arr(GOAL_TRACK), x0=arr(X0S[0]))
    r.step("closed loop, goal track and a start", lambda: pl.closed_loop(2, goal_tolerance=0.0, x_init=arr(X0S[1])))


def batch_disc_sets(r):
    shared = base(obstacle_tracks=arr(TRACKS))
    del shared["obstacle_positions"]
    pl = batch(r, shared)
    r.step("shared tracks", pl.solve)
    r.step("control step", lambda: pl.shift_and_update(arr(X0S), np.zeros((B, 4, 2), np.float32)))
    sets = [(arr(TRACKS), arr([0.25, 0.5])), (arr(TRACKS)[:1], arr([0.75]))]
    r.step("per-problem tracks while the shared ones are held", lambda: pl.set_obstacle_sets(sets))
    r.step("solve: the per-problem tracks win", pl.solve)
    r.step("control step", lambda: pl.shift_and_update_on_device(arr(X0S), 2))
    r.step("the same sets again", lambda: pl.set_obstacle_sets([(arr(t, np.float32), arr(q, np.float32)) for t, q in sets]))
    r.step("sets changed", lambda: pl.set_obstacle_sets([sets[0], (changed(arr(TRACKS)[:1]), arr([0.75]))]))
    r.value("obstacle_sets", lambda: [x for pair in pl.obstacle_sets for x in pair])
    static = [(arr([[1.0, 1.0]]), arr([0.25])), (np.zeros((0, 2)), np.zeros(0))]
    r.step("static sets after track sets", lambda: pl.set_obstacle_sets(static))
    r.step("solve: the shared tracks are handed over again", pl.solve)
    r.step("a call that mixes the two", lambda: pl.set_obstacle_sets([sets[0], static[0]]))
    r.step("track sets after static sets", lambda: pl.set_obstacle_sets(sets))
    r.step("sets whose rows differ", lambda: pl.set_obstacle_sets([sets[0], (arr(TRACKS)[:, :2], arr([0.25, 0.5]))]))
    r.step("a set without rows", lambda: pl.set_obstacle_sets([sets[0], (np.zeros((1, 0, 2)), arr([0.25]))]))
    r.step("a set of the wrong shape", lambda: pl.set_obstacle_sets([sets[0], (np.zeros((1, 3, 3)), arr([0.25]))]))
    r.step("two tracks, one radius", lambda: pl.set_obstacle_sets([sets[0], (arr(TRACKS), arr([0.25]))]))
    r.step("rows that differ and one radius", lambda: pl.set_obstacle_sets([sets[0], (arr(TRACKS)[:, :2], arr([0.25]))]))
    r.step("no rows and one radius", lambda: pl.set_obstacle_sets([sets[0], (np.zeros((2, 0, 2)), arr([0.25]))]))
    r.step("one radius, then a set of the wrong shape", lambda: pl.set_obstacle_sets(
        [(arr(TRACKS), arr([0.25])), (np.zeros((1, 3, 3)), arr([0.25]))]))
    r.step("solve: the per-problem tracks are still held", pl.solve)
    r.step("a call that mixes the two, the static set first: the tracks held go first", lambda: pl.set_obstacle_sets([static[0], sets[0]]))
    r.step("track sets again", lambda: pl.set_obstacle_sets(sets))
    r.step("None", lambda: pl.set_obstacle_sets(None))
    r.step("solve: the shared tracks are handed over again", pl.solve)
    pl.params = dict(without(pl.params, "obstacle_tracks"), obstacle_positions=arr([[1.0, 1.0], [1.5, 0.5]]))
    r.step("static sets beside shared static discs", lambda: pl.set_obstacle_sets(static))
    r.step("solve", pl.solve)
    pl.params = dict(without(pl.params, "obstacle_positions"), obstacle_track_samples=arr(SAMPLES))
    r.step("samples in params while obstacle_sets are held", pl.solve)
    r.step("None", lambda: pl.set_obstacle_sets(None))
    r.step("solve: the samples are handed over", pl.solve)
    r.step("obstacle_sets while samples are held", lambda: pl.set_obstacle_sets(static))
    del pl.params["obstacle_track_samples"]
    r.step("obstacle_sets while samples are still held, the key gone", lambda: pl.set_obstacle_sets(sets))


def batch_wall_sets(r):
    pl = batch(r, base(wall_tracks=arr(WALL_TRACKS), wall_halfwidth=0.125))
    r.step("shared wall tracks", pl.solve)
    r.step("control step", lambda: pl.shift_and_update(arr(X0S), np.zeros((B, 4, 2), np.float32)))
    sets = [(arr(WALL_TRACKS), 0.125), (arr(WALL_TRACKS)[:1], arr([0.25]))]
    r.step("per-problem wall tracks while the shared ones are held", lambda: pl.set_wall_sets(sets))
    r.step("solve: the per-problem sets win", pl.solve)
    r.step("control step", lambda: pl.shift_and_update_on_device(arr(X0S)))
    r.step("the same sets again", lambda: pl.set_wall_sets([(arr(t, np.float32), np.float32(h)) for t, h in sets]))
    r.step("sets changed", lambda: pl.set_wall_sets([sets[0], (changed(arr(WALL_TRACKS)[:1]), arr([0.25]))]))
    r.value("wall_sets", lambda: [x for pair in pl.wall_sets for x in pair])
    pl.params["wall_tracks"] = np.zeros((2, 2, 2))
    r.step("solve: shared wall tracks of a bad shape beside per-problem sets", pl.solve)
    pl.params["wall_tracks"] = np.zeros((2, 0, 2, 2))
    r.step("solve: shared wall tracks without rows beside per-problem sets", pl.solve)
    pl.params["wall_tracks"] = arr(WALL_TRACKS)
    static = [(arr(WALLS), 0.125), (np.zeros((0, 2, 2)), 0.0)]
    r.step("static sets: tracks of one row", lambda: pl.set_wall_sets(static))
    r.step("control step with sets of one row", lambda: pl.shift_and_update(arr(X0S), np.zeros((B, 4, 2), np.float32)))
    r.step("a call that mixes the two", lambda: pl.set_wall_sets([sets[0], static[0]]))
    r.step("sets whose rows differ", lambda: pl.set_wall_sets([sets[0], (arr(WALL_TRACKS)[:, :2], 0.125)]))
    r.step("a set without rows", lambda: pl.set_wall_sets([sets[0], (np.zeros((1, 0, 2, 2)), 0.125)]))
    r.step("a set of the wrong shape", lambda: pl.set_wall_sets([sets[0], (np.zeros((1, 3, 2, 3)), 0.125)]))
    r.step("two walls, three half-widths", lambda: pl.set_wall_sets([sets[0], (arr(WALL_TRACKS), arr([0.125, 0.25, 0.5]))]))
    r.step("rows that differ and three half-widths", lambda: pl.set_wall_sets([sets[0], (arr(WALL_TRACKS)[:, :2], arr([0.125, 0.25, 0.5]))]))
    r.step("no rows and three half-widths", lambda: pl.set_wall_sets([sets[0], (np.zeros((2, 0, 2, 2)), arr([0.125, 0.25, 0.5]))]))
    r.step("three half-widths, then a set of the wrong shape", lambda: pl.set_wall_sets(
        [(arr(WALL_TRACKS), arr([0.125, 0.25, 0.5])), (np.zeros((1, 3, 2, 3)), 0.125)]))
    r.step("None", lambda: pl.set_wall_sets(None))
    r.step("None again", lambda: pl.set_wall_sets(None))
    r.step("solve: the shared wall tracks are handed over again", pl.solve)
    r.step("per-problem sets again", lambda: pl.set_wall_sets(sets))
    del pl.params["wall_tracks"]
    r.step("solve: the shared key has gone while per-problem sets are held", pl.solve)
    r.step("None", lambda: pl.set_wall_sets(None))
    r.step("solve: nothing shared to hand over", pl.solve)


def batch_goal_tracks(r):
    pl = batch(r, dict(without(base(), "xgoal"), goal_track=arr(GOAL_TRACK)))
    r.step("shared goal track", pl.solve)
    r.step("control step", lambda: pl.shift_and_update(arr(X0S), np.zeros((B, 4, 2), np.float32)))
    r.value("goal_now, shared", lambda: pl.goal_now)
    tracks = [arr(GOAL_TRACK), arr(GOAL_TRACK)[::-1]]
    r.step("per-problem goal tracks while the shared one is held", lambda: pl.set_goal_tracks(tracks))
    r.step("solve: the per-problem tracks win", pl.solve)
    r.step("control step", lambda: pl.shift_and_update_on_device(arr(X0S)))
    r.value("goal_now, per problem", lambda: pl.goal_now)
    r.step("the same tracks again", lambda: pl.set_goal_tracks(arr(tracks, np.float32)))
    r.step("tracks changed", lambda: pl.set_goal_tracks([tracks[0], changed(GOAL_TRACK)]))
    r.value("goal_tracks", lambda: pl.goal_tracks)
    pl.params["goal_track"] = np.zeros((3, 3))
    r.step("solve: a shared goal track of a bad shape beside per-problem tracks", pl.solve)
    pl.params["goal_track"] = arr(GOAL_TRACK)
    r.step("one track for two problems", lambda: pl.set_goal_tracks(tracks[:1]))
    r.step("tracks whose rows differ", lambda: pl.set_goal_tracks([tracks[0], tracks[1][:2]]))
    r.step("a track without rows", lambda: pl.set_goal_tracks([tracks[0], np.zeros((0, 2))]))
    r.step("a track of the wrong shape", lambda: pl.set_goal_tracks([tracks[0], np.zeros((3, 3))]))
    r.step("tracks of one row", lambda: pl.set_goal_tracks([t[:1] for t in tracks]))
    r.step("control step with tracks of one row", lambda: pl.shift_and_update(arr(X0S), np.zeros((B, 4, 2), np.float32)))
    r.step("None", lambda: pl.set_goal_tracks(None))
    r.step("None again", lambda: pl.set_goal_tracks(None))
    r.step("solve: the shared goal track is handed over again", pl.solve)
    r.step("per-problem tracks again", lambda: pl.set_goal_tracks(tracks))
    pl.params = dict(without(pl.params, "goal_track"), xgoal=arr(GOALS[0]))
    r.step("solve: the shared key has gone while per-problem tracks are held", pl.solve)
    r.step("None", lambda: pl.set_goal_tracks(None))
    r.value("goal_now, static goals", lambda: pl.goal_now)
    r.step("solve: nothing shared to hand over", pl.solve)


def batch_setup_with_sets(r):
    pl = batch(r, obstacle_sets=[(arr(TRACKS), arr([0.25, 0.5]))] * B, wall_sets=[(arr(WALL_TRACKS), 0.125)] * B,
               goal_tracks=arr([GOAL_TRACK] * B))
    r.step("solve", pl.solve)
    r.step("control step", lambda: pl.shift_and_update(arr(X0S), np.zeros((B, 4, 2), np.float32)))
    r.step("state rollout of problem 1", lambda: pl.get_state_rollout(1))
    r.step("closed loop of a batch", lambda: pl.closed_loop(2))


def _fleets(r, name, on, other):
    pl = batch(r)
    turn_on = lambda: on(pl)  # noqa: E731
    pl.params["footprint"] = arr(FOOTPRINT)
    r.step(name + " while the footprint key is there, not handed over", turn_on)
    r.step("solve: the footprint is handed over", pl.solve)
    r.step(name + " while the footprint key is there", turn_on)
    del pl.params["footprint"]
    r.step(name + " while the footprint is held, the key gone: cleared first", turn_on)
    r.value("fleet", lambda: pl.fleet)
    r.value("fleet_bodies", lambda: pl.fleet_bodies)
    r.step("the other kind of fleet meanwhile", lambda: other(pl))
    r.step("solve beside the fleet", pl.solve)
    pl.params["footprint"] = arr(FOOTPRINT)
    r.step("solve: a footprint beside the fleet", pl.solve)
    del pl.params["footprint"]
    pl.params.update(wall_tracks=arr(WALL_TRACKS), wall_halfwidth=0.125)
    r.step("solve: wall tracks beside the fleet", pl.solve)
    pl.params["wall_segments"] = arr(WALLS)
    r.step("solve: wall tracks and walls beside the fleet", pl.solve)
    del pl.params["wall_tracks"]
    r.step("solve: walls beside the fleet", pl.solve)
    r.step("wall sets beside the fleet", lambda: pl.set_wall_sets([(arr(WALLS), 0.125)] * B))
    r.step("set_wall_sets(None) beside the fleet", lambda: pl.set_wall_sets(None))
    r.step("refresh", pl.refresh_fleet)
    r.step("off", lambda: pl.set_fleet(None))
    r.step("wall sets", lambda: pl.set_wall_sets([(arr(WALLS), 0.125)] * B))
    r.step(name + " while wall sets are held", turn_on)
    r.step("wall sets go", lambda: pl.set_wall_sets(None))
    pl.params = dict(without(pl.params, "wall_segments"), wall_tracks=arr(WALL_TRACKS))
    r.step(name + " while the wall_tracks key is there, not handed over", turn_on)
    r.step("solve: wall tracks beside the fleet", pl.solve)
    r.step("off", lambda: pl.set_fleet(None))
    r.step("solve: the wall tracks are handed over", pl.solve)
    r.step(name + " while wall tracks are held", turn_on)
    del pl.params["wall_tracks"]
    r.step(name + " while wall tracks are held, the key gone", turn_on)
    r.step("solve: the wall tracks go", pl.solve)
    r.step(name + " at last", turn_on)
    r.step("off through set_fleet_bodies(None)", lambda: pl.set_fleet_bodies(None))
    return pl


def fleet(r):
    pl = _fleets(r, "set_fleet", lambda pl: pl.set_fleet(arr([0.25, 0.5]), 0.125), lambda pl: pl.set_fleet_bodies(arr(FOOTPRINT)))
    r.step("bad radii", lambda: pl.set_fleet(arr([0.25, -0.5])))
    r.step("fleet_walls while off", pl.fleet_walls)
    r.step("on, a scalar radius", lambda: pl.set_fleet(0.25))
    r.step("fleet_walls", pl.fleet_walls)
    r.step("fleet_body_walls of a disc fleet", pl.fleet_body_walls)


def fleet_bodies(r):
    pl = _fleets(r, "set_fleet_bodies", lambda pl: pl.set_fleet_bodies(arr(FOOTPRINT), 0.125), lambda pl: pl.set_fleet(0.25))
    r.step("a bad body", lambda: pl.set_fleet_bodies(arr([[0.0, 0.0, -0.25]])))
    r.step("on", lambda: pl.set_fleet_bodies(arr(FOOTPRINT)))
    r.step("fleet_body_walls", pl.fleet_body_walls)
    r.step("fleet_walls of a fleet of bodies", pl.fleet_walls)


def fleet_after_reset(r):
    pl = batch(r, base(footprint=arr(FOOTPRINT)))
    r.step("solve: the footprint is handed over", pl.solve)
    r.step("reset", pl.reset)
    r.step("set_fleet without params: the footprint held is cleared first", lambda: pl.set_fleet(0.25))


SCENARIOS = (static_discs, no_discs_at_first, disc_tracks, disc_samples, static_walls, wall_tracks, goal_track, footprint,
             clearance_rings, noise_smoothing, rings_and_samples, everything_at_once, closed_loop, batch_disc_sets,
             batch_wall_sets, batch_goal_tracks, batch_setup_with_sets, fleet, fleet_bodies, fleet_after_reset)


def trace(scenario, patch):
    recorder = Recorder()
    patch(_lib, "call", recorder.call)
    patch(_lib, "ptr", lambda array, ctype: array)
    run = Run(recorder)
    try:
        scenario(run)
    finally:
        steps = run.close()
    return json.loads(json.dumps(steps))  # (tuples become lists, as they are in the golden file)


@pytest.mark.parametrize("scenario", SCENARIOS, ids=[s.__name__ for s in SCENARIOS])
def test_mirror_calls(scenario, monkeypatch):
    with open(GOLDEN) as f:
        want = json.load(f)[scenario.__name__]
    got = trace(scenario, monkeypatch.setattr)
    assert [s["step"] for s in got] == [s["step"] for s in want]
    for have, expect in zip(got, want):
        assert have == expect, "step {!r}".format(expect["step"])


def test_the_golden_file_holds_these_scenarios_and_no_others():
    with open(GOLDEN) as f:
        assert sorted(json.load(f)) == sorted(s.__name__ for s in SCENARIOS)


if __name__ == "__main__":  # record the golden traces (at the commit the docstring names, not from the code under test)
    traces = {s.__name__: trace(s, setattr) for s in SCENARIOS}
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(
            " {}: [\n{}\n ]".format(json.dumps(name), ",\n".join("  " + json.dumps(step, separators=(",", ":")) for step in steps))
            for name, steps in traces.items()) + "\n}\n")
    print("{}: {} scenarios, {} steps, {} calls".format(GOLDEN, len(traces), sum(len(s) for s in traces.values()),
                                                        sum(len(step["calls"]) for s in traces.values() for step in s)))
