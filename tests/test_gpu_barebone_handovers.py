"""The hand-overs of the barebone mode at the library itself (csrc/barebone_api.h): every setter is called through _lib.call
on the planner's handle, so the Python mirror's key caches -- which never reach the library with an unchanged set -- are not
in the path.  Per setter: the same values again (fresh arrays at other addresses) cost nothing a solve can see -- no new
capture, the track offsets untouched, the controls of a twin handle that was not handed the repeat, bit for bit; a refused
hand-over leaves the handle as it was; one changed float drops the captured graphs and makes row 0 "now" again exactly
where the rows are counted; a cleared set leaves the controls of a twin that never held it.

Two problems of 128 rollouts (two tiles each), 8 steps, crowd mode (every setter is legal there), graphs of two iterations
and three iterations a solve: at this size no launch produces the next iteration's noise ahead, so every solve begins with
one direct iteration (run_iterations) and a solve of two would never reach a graph -- with three, each solve is one direct
iteration and one graph, which the test asserts (replays go up).  The twins share the seed and are solved in lock-step
from zero controls, so their Philox counters agree."""
import collections
import ctypes as C

import numpy as np
import pytest

from test_gpu_barebone_batch import make_params
from test_gpu_barebone_crowd import cfg_of

pytestmark = pytest.mark.gpu

B, N, T = 2, 128, 8
X0S = np.float32([[0.0, 0.0, np.pi / 4], [0.5, -0.4, 0.3]])
GOALS = np.float32([[3.0, 2.5], [3.5, 1.0]])
NAN = np.float32(np.nan)


def f32(values):
    return np.ascontiguousarray(values, dtype=np.float32)


def i32(values):
    return np.ascontiguousarray(values, dtype=np.int32)


# three discs on the way of both problems; as tracks they drift by 0.1 m a row
DISC_POS = f32([[0.6, 0.55], [1.0, 0.1], [0.9, -0.3]])
DISC_RAD = f32([0.25, 0.3, 0.2])
DISC_TRACKS = f32(DISC_POS[:, None, :] + 0.1 * np.arange(3)[None, :, None])  # (3 discs, 3 rows, 2)
DISC_SAMPLES = f32(np.stack([DISC_TRACKS, DISC_TRACKS + 0.15]))  # (2 samples, 3 discs, 3 rows, 2)
# two walls: a thick one whose band holds both starts (a rollout is hit until it has left it), a thin one across problem 1's
# way; as tracks they drift likewise
WALL_SEG = f32([[0.2, 0.1, 0.4, -0.2], [0.9, -0.8, 1.2, 0.3]])
WALL_HW = f32([0.5, 0.1])
WALL_TRACKS = f32(WALL_SEG[:, None, :] + 0.1 * np.arange(3)[None, :, None])  # (2 walls, 3 rows, 4)
GOAL_TRACKS = f32(GOALS[:, None, :] - 0.5 * np.arange(3)[None, :, None])  # (B tracks, 3 rows, 2)

# fn: the setter; args: what is handed over, in the setter's order (arrays as pointers); vary: which of them gets one float
# changed; clear: the arguments that clear the set; refuse: (index, value) -- args with that one replaced must be refused
# (an array: its last element set to the value); resets: a change makes row 0 "now" again
Kind = collections.namedtuple("Kind", "fn args vary clear refuse resets")
KINDS = {
    "shared_discs": Kind("mppi_planner_set_disc_obstacles", (DISC_POS, DISC_RAD, 3), 0, (None, None, 0), (2, -1), False),
    "own_discs": Kind("mppi_planner_set_instance_disc_obstacles", (B, i32([2, 1]), DISC_POS, DISC_RAD), 2,
                      (0, None, None, None), (0, 3), False),
    "disc_tracks": Kind("mppi_planner_set_disc_tracks", (B, i32([2, 1]), 3, DISC_TRACKS, DISC_RAD), 3,
                        (0, None, 0, None, None), (0, 3), True),
    "disc_samples": Kind("mppi_planner_set_disc_track_samples", (2, 3, 3, DISC_SAMPLES, DISC_RAD), 3,
                         (0, 0, 0, None, None), (4, -0.5), True),
    "walls": Kind("mppi_planner_set_walls", (WALL_SEG, WALL_HW, 2), 0, (None, None, 0), (1, -0.5), False),
    "wall_tracks": Kind("mppi_planner_set_wall_tracks", (B, i32([1, 1]), 3, WALL_TRACKS, WALL_HW), 3,
                        (0, None, 0, None, None), (3, NAN), True),
    "wall_tracks_of_one_row": Kind("mppi_planner_set_wall_tracks", (1, i32([2]), 1, WALL_SEG, WALL_HW), 3,
                                   (0, None, 0, None, None), (4, -0.5), False),
    "goal_tracks": Kind("mppi_planner_set_goal_tracks", (B, 3, GOAL_TRACKS), 2, (0, 0, None), (2, NAN), True),
    "goal_tracks_of_one_row": Kind("mppi_planner_set_goal_tracks", (1, 1, f32([[1.5, 2.5]])), 2, (0, 0, None), (0, 3), False),
    # (the solves start from zero controls, so the others' plans stand at their starts, 0.64 m apart: within these half-widths)
    "fleet": Kind("mppi_planner_set_fleet", (B, f32([[0.9], [0.8]])), 1, (0, None), (1, -0.5), False),
    "footprint": Kind("mppi_planner_set_footprint", (f32([[0.3, 0.0, 0.25], [-0.3, 0.0, 0.2]]), 2), 0, (None, 0), (0, -0.5), False),
    "rings": Kind("mppi_planner_set_clearance_rings", (f32([[0.2, 500.0], [0.5, 100.0]]), 2), 0, (None, 0), (0, NAN), False),
}


def hand_over(planner, fn, args):
    """Straight to the library, every array as a fresh copy: what is held is still alive, so the addresses differ."""
    from mppi_numba_amd import _lib
    fresh = [np.array(a) if isinstance(a, np.ndarray) else a for a in args]
    assert all(f.ctypes.data != a.ctypes.data for f, a in zip(fresh, args) if isinstance(a, np.ndarray))
    _lib.call(fn, planner._handle, *[_lib.ptr(a, C.c_int if a.dtype == np.int32 else C.c_float) if isinstance(a, np.ndarray) else a
                                     for a in fresh])


def replaced(args, index, value):
    """args with one of them replaced: an int by the value, an array by a copy whose last element is the value."""
    args = list(args)
    if isinstance(args[index], np.ndarray):
        args[index] = args[index].copy()
        args[index].reshape(-1)[-1] = value
    else:
        args[index] = value
    return tuple(args)


def offsets_of(planner):
    from mppi_numba_amd import _lib
    out = np.full(B, -1, dtype=np.int32)
    _lib.call("mppi_planner_get_track_offsets", planner._handle, B, _lib.ptr(out, C.c_int))
    return out.tolist()


def set_offsets(planners, offset):
    from mppi_numba_amd import _lib
    for planner in planners:
        _lib.call("mppi_planner_set_track_offsets", planner._handle, B, _lib.ptr(i32([offset] * B), C.c_int))


def solve_all(planners):
    """One library solve each from zero controls, in lock-step: handles that hold the same scene give the same bits."""
    from mppi_numba_amd import _lib
    out = []
    for planner in planners:
        planner.set_u(np.zeros((B, T, 2), dtype=np.float32))
        u = np.empty((B, T, 2), dtype=np.float32)
        _lib.call("mppi_planner_solve", planner._handle, None, None, _lib.ptr(u, C.c_float))
        assert np.isfinite(u).all()
        out.append(u)
    return out


def handle(kind, held):
    """A settled handle: the mirror has solved once (without an obstacle key it clears the shared discs then, and hands
    nothing over afterwards); the shared discs are the scene every other kind is held beside."""
    from mppi_numba_amd.barebone import MPPI_Batch
    planner = MPPI_Batch(cfg_of(N, T, True), B)
    planner.setup(make_params(0.1, 1.0, num_opt=3), X0S, GOALS)
    planner.set_graph_replay(True, 2)
    planner.solve()
    if kind != "shared_discs":
        hand_over(planner, KINDS["shared_discs"].fn, KINDS["shared_discs"].args)
    if held:
        hand_over(planner, KINDS[kind].fn, KINDS[kind].args)
    return planner


def assert_bits(got, want, what):
    assert (got.view(np.int32) == want.view(np.int32)).all(), "%s: %d of %d values differ" % (what, (got != want).sum(), got.size)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_hand_over(kind):
    from mppi_numba_amd import _lib
    k = KINDS[kind]
    subject, twin, never = handle(kind, True), handle(kind, True), handle(kind, False)
    everyone = (subject, twin, never)
    for _ in range(3):  # (three iterations a solve: the buffer parities come round within four solves, each with a graph of its own)
        solve_all(everyone)

    # the same again, in fresh arrays: no capture, the offsets untouched, the twin's controls
    set_offsets(everyone, 2)
    solve_all(everyone)
    before = subject.graph_stats()
    hand_over(subject, k.fn, k.args)
    assert offsets_of(subject) == [2, 2]
    u, u_twin, u_never = solve_all(everyone)
    after = subject.graph_stats()
    assert after["captures"] == before["captures"], "the same %s again: a new capture" % kind
    assert after["replays"] > before["replays"], "the solve replayed no graph: the captures prove nothing"
    assert offsets_of(subject) == [2, 2]
    assert_bits(u, u_twin, "the same %s again" % kind)
    assert not np.array_equal(u_twin, u_never), "bad input: the %s change nothing, a cleared set could not be told from a held one" % kind

    # a refused hand-over: the handle as it was
    with pytest.raises(_lib.MppiError):
        hand_over(subject, k.fn, replaced(k.args, *k.refuse))
    assert offsets_of(subject) == [2, 2]
    u, u_twin, _ = solve_all(everyone)
    assert subject.graph_stats()["captures"] == before["captures"], "a refused hand-over of %s: a new capture" % kind
    assert_bits(u, u_twin, "after a refused hand-over of %s" % kind)

    # one float changed: new graphs; row 0 is "now" again where the set counts rows
    changed = replaced(k.args, k.vary, k.args[k.vary].reshape(-1)[-1] + np.float32(0.125))
    hand_over(subject, k.fn, changed)
    assert offsets_of(subject) == ([0, 0] if k.resets else [2, 2])
    solve_all(everyone)
    assert subject.graph_stats()["captures"] > before["captures"], "other %s: the captured graphs were kept" % kind

    # cleared: the controls of the twin that never held the set
    hand_over(subject, k.fn, k.clear)
    set_offsets(everyone, 2)
    u, _, u_never = solve_all(everyone)
    assert_bits(u, u_never, "%s cleared" % kind)
