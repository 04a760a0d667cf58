"""The guide round the walls of the barebone planner (params['guide'], mppi_planner_set_guide): a shortest-path field from
every problem's goal over a grid whose cells the static walls block (k_guide_field), and goal rows on the shortest path from
the start (k_guide_rows), which the rollouts meet as a goal track.  Field, rows and status are compared bit for bit with
tests/guide_model.py (pinned on the CPU by tests/test_guide_model.py); costs with a twin handle that is handed the fetched
rows as goal tracks, the path the oracle already pins."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import guide_model as model
from test_gpu_barebone_batch import ERR_INVALID, assert_bits, make_params
from test_gpu_barebone_crowd import cfg_of, inputs
from test_gpu_barebone_tracks import rollout_with
from wall_model import hit

pytestmark = pytest.mark.gpu

N, T = 128, 20
NO_WALLS = (np.zeros((0, 2, 2), np.float32), np.zeros(0, np.float32))
ROOM = (np.array([[[1.0, 0.0], [1.0, 1.5]]], np.float32), np.float32([0.0]))  # a wall across the lower part of a 2 x 2 room
BOX = (np.array([[[0.5, 0.5], [1.5, 0.5]], [[1.5, 0.5], [1.5, 1.5]], [[1.5, 1.5], [0.5, 1.5]], [[0.5, 1.5], [0.5, 0.5]]], np.float32),
       np.float32([0.0] * 4))


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


def guide_of(origin, res, shape, inflate=None, lead=None, pace=None):
    g = dict(origin=origin, resolution=res, shape=shape)
    for key, value in (("inflate", inflate), ("lead", lead), ("pace", pace)):
        if value is not None:
            g[key] = value
    return g


def task_params(guide, walls, x0, goal, num_opt=1):
    p = make_params(0.1, 1.0, num_opt=num_opt)
    p["x0"], p["xgoal"] = np.asarray(x0, np.float64), np.asarray(goal, np.float64)
    p["wall_segments"], p["wall_halfwidth"] = walls
    p["guide"] = guide
    return p


def model_of(p, t, x0=None, goal=None):
    """The model's (field, rows, status) of a problem of params p (the defaults as barebone.py forms them)."""
    g = p["guide"]
    grid = model.Grid(g["origin"], g["resolution"], g["shape"], g.get("inflate"))
    pace = g.get("pace", float(p["vrange"][1]) * float(p["dt"]))
    lead = g.get("lead", 2.0 * pace)
    x0 = p["x0"] if x0 is None else x0
    goal = p["xgoal"] if goal is None else goal
    D = model.field(grid, p["wall_segments"], p["wall_halfwidth"], goal)
    rows, status, _ = model.rows(grid, D, x0, goal, t, lead, pace)
    return D, rows, status


@functools.lru_cache(maxsize=None)
def spiral():
    """A rectangular spiral of walls in a 19.2 m square, 0.6 m from turn to turn: from its mouth to its middle the shortest
    path is thousands of cells of 0.1 m long."""
    lo, hi, s = 0.5, 18.7, 0.6
    pts, length, k = [(lo, lo)], hi - lo, 0
    steps = ((1, 0), (0, 1), (-1, 0), (0, -1))
    while length > s:
        dx, dy = steps[k % 4]
        pts.append((pts[-1][0] + dx * length, pts[-1][1] + dy * length))
        k += 1
        if k >= 3 and k % 2 == 1:
            length -= s
    pts = np.float32(pts)
    seg = np.stack([pts[:-1], pts[1:]], axis=1)
    return seg, np.zeros(len(seg), np.float32)


def five_walls():
    rng = np.random.default_rng(11)
    a = rng.uniform(0.3, 2.8, (5, 2))
    seg = np.stack([a, a + rng.uniform(-1.2, 1.2, (5, 2))], axis=1).astype(np.float32)
    return seg, rng.uniform(0.0, 0.05, 5).astype(np.float32)


# name -> (guide, walls, start, goal, T, expected status)
CASES = {
    "1x1": (guide_of((0.0, 0.0), 0.5, (1, 1)), NO_WALLS, (0.1, 0.1, 0.0), (0.4, 0.3), T, 0),
    "1x7": (guide_of((0.0, 0.0), 0.5, (1, 7)), NO_WALLS, (0.1, 0.1, 0.0), (3.4, 0.4), T, 0),
    "7x1": (guide_of((0.0, 0.0), 0.5, (7, 1)), NO_WALLS, (0.1, 0.1, 0.0), (0.4, 3.4), T, 0),
    "5x9": (guide_of((-1.0, 2.0), 0.25, (5, 9), lead=0.25, pace=0.25), NO_WALLS, (-0.9, 2.1, 0.0), (1.1, 3.1), T, 0),
    "33x31 five walls": (guide_of((0.0, 0.0), 0.1, (33, 31), inflate=0.0708, lead=0.2, pace=0.1), five_walls(), (0.15, 0.15, 0.0), (2.9, 3.1), T, 0),
    "192x192 spiral": (guide_of((0.0, 0.0), 0.1, (192, 192), lead=1.0, pace=0.5), spiral(), (0.8, 0.8, 0.0), (9.5, 9.9), T, 0),
    "128x127 (static and dynamic LDS cross 64 KiB)": (guide_of((0.0, 0.0), 0.1, (128, 127), lead=1.0, pace=0.5), (np.float32([[[6.0, 0.0], [6.0, 9.0]], [[3.0, 12.7], [3.0, 4.0]], [[9.0, 12.7], [9.5, 3.0]]]), np.float32([0.0, 0.1, 0.05])),
                                                      (1.0, 1.0, 0.0), (11.0, 1.0), T, 0),
    "sealed pocket": (guide_of((0.0, 0.0), 0.25, (12, 12)), BOX, (1.0, 1.0, 0.0), (2.6, 2.6), T, 2),
    "blocked goal": (guide_of((0.0, 0.0), 0.25, (8, 8)), ROOM, (0.1, 0.1, 0.0), (1.0, 0.6), T, 1),
    "goal and start outside the grid": (guide_of((0.0, 0.0), 0.25, (8, 8), lead=0.25, pace=0.25), ROOM, (-5.0, 0.1, 0.0), (9.0, -4.0), T, 0),
    "start inside the inflated band": (guide_of((0.0, 0.0), 0.25, (8, 8), lead=0.0, pace=0.25), ROOM, (0.8, 0.6, 0.0), (1.9, 0.1), T, 0),
    "lead and pace zero": (guide_of((0.0, 0.0), 0.25, (8, 8), lead=0.0, pace=0.0), ROOM, (0.1, 0.1, 0.0), (1.9, 0.1), T, 0),
    "a short path": (guide_of((0.0, 0.0), 0.25, (8, 8), lead=0.5, pace=0.25), ROOM, (0.1, 0.1, 0.0), (1.9, 0.1), 2 * T, 0),
    "T = 1": (guide_of((0.0, 0.0), 0.25, (8, 8), lead=0.5, pace=0.25), ROOM, (0.1, 0.1, 0.0), (1.9, 0.1), 1, 0),
    "T = 70": (guide_of((0.0, 0.0), 0.1, (33, 31), inflate=0.0708, lead=0.2, pace=0.05), five_walls(), (0.15, 0.15, 0.0), (2.9, 3.1), 70, 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_field_rows_and_status_equal_the_model(name):
    from mppi_numba_amd.barebone import MPPI_Numba
    guide, walls, x0, goal, t, expected = CASES[name]
    p = task_params(guide, walls, x0, goal)
    D, rows, status = model_of(p, t)
    assert status == expected, "bad input: the model's status is %d" % status
    if name == "192x192 spiral":
        grid = model.Grid(guide["origin"], guide["resolution"], guide["shape"])
        c0 = (int(model.cell_of(x0[1], 0.0, 0.1, 192)), int(model.cell_of(x0[0], 0.0, 0.1, 192)))
        assert 12 * 2000 < D[c0] < model.UNREACHED, "bad input: the spiral's path is %d units long" % D[c0]
        assert grid.nx * grid.ny == model.CELLS_MAX
    if name == "a short path":
        assert (rows[-5:] == np.float32(goal)).all() and (rows[0] != np.float32(goal)).any()
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.setup(p)
    planner.refresh_guide()
    got = planner.guide_field()
    assert got.shape == D.shape and got.dtype == np.uint32
    assert (got == D).all(), "%s: %d of %d cells differ" % (name, (got != D).sum(), D.size)
    assert planner.guide_status() == status
    assert_bits(planner.guide_rows(), rows, "%s: rows vs the model" % name)
    assert (planner.goal_now == np.float32(goal)).all(), "goal_now stays the true goal"
    assert planner.guide_fields_built == 1


def test_a_batch_of_three_goals():
    from mppi_numba_amd.barebone import MPPI_Batch
    guide, walls = guide_of((0.0, 0.0), 0.1, (33, 31), inflate=0.0708, lead=0.2, pace=0.1), five_walls()
    x0s = np.float32([[0.15, 0.15, 0.0], [2.9, 0.2, 1.0], [1.5, 3.2, -2.0]])
    goals = np.float32([[2.9, 3.1], [0.2, 2.2], [1.5, 0.1]])
    p = task_params(guide, walls, x0s[0], goals[0])
    batch = MPPI_Batch(cfg_of(N, T, True), 3)
    batch.setup(p, x0s, goals)
    batch.refresh_guide()
    field, rows, status = batch.guide_field(), batch.guide_rows(), batch.guide_status()
    assert field.shape == (3, 33, 31) and rows.shape == (3, T + 1, 2) and status.shape == (3,)
    fields = []
    for b in range(3):
        D, want, st = model_of(p, T, x0s[b], goals[b])
        assert (field[b] == D).all(), "problem %d: %d cells differ" % (b, (field[b] != D).sum())
        assert_bits(rows[b], want, "problem %d: rows vs the model" % b)
        assert st == 0, "bad input: problem %d has status %d in the model" % (b, st)
        assert status[b] == 0
        fields.append(D)
    assert (fields[0] != fields[1]).any() and (fields[1] != fields[2]).any(), "bad input: the goals share a field"
    assert (batch.goal_now == goals).all()


# ---------------------------------------------------------------------- costs: the rows are a goal track
def room_task(crowd, footprint):
    """The task of make_params in a room of three walls; without crowd mode: two discs and no walls."""
    p = make_params(0.1, 1.0)
    p["xgoal"] = np.array([2.6, 2.4])
    p["obstacle_positions"], p["obstacle_radius"] = np.float32([[1.0, 1.2], [1.8, 1.4]]), np.float32([0.3, 0.25])
    seg = np.float32([[[0.8, 0.2], [2.4, 0.6]], [[0.2, 1.0], [0.4, 2.6]], [[1.6, 1.9], [2.2, 1.7]]])
    p["wall_segments"], p["wall_halfwidth"] = (seg, np.float32([0.05, 0.1, 0.0])) if crowd else NO_WALLS
    if footprint:
        from mppi_numba_amd.barebone import rectangle_footprint
        p["footprint"] = rectangle_footprint(0.5, 0.3, 0.4)
    p["guide"] = guide_of((-0.5, -0.5), 0.1, (36, 38), inflate=0.1, lead=0.6, pace=0.15)
    return p


def twin_params(p, table):
    q = {k: v for k, v in p.items() if k not in ("guide", "xgoal")}
    q["goal_track"] = table
    return q


@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("kind", ["default, two discs", "crowd, walls", "crowd, footprint"])
def test_costs_equal_a_twin_that_is_handed_the_rows_as_goal_tracks(kind, offset):
    """offset 3: disc tracks are held and "now" is their row 3; the twin's table is then the guide's rows behind three junk
    rows, which the guide's launch never reads: GoalRows::relative."""
    from mppi_numba_amd.barebone import MPPI_Numba, constant_velocity_tracks
    crowd, footprint = kind != "default, two discs", kind == "crowd, footprint"
    t = T
    p = room_task(crowd, footprint)
    if offset:
        p["obstacle_tracks"] = constant_velocity_tracks(p.pop("obstacle_positions"), [[0.1, 0.0], [0.0, -0.1]], 0.1, t + 1)
    rng = np.random.default_rng(5)
    u_in, noise = inputs(rng, N, t)
    guided, twin = MPPI_Numba(cfg_of(N, t, crowd)), MPPI_Numba(cfg_of(N, t, crowd))
    guided.set_params(p)
    guided.move_mppi_task_vars_to_device()
    guided.set_track_offset(offset)
    costs, _, _, kernel = rollout_with(guided, u_in, noise)
    rows = guided.guide_rows()
    assert kernel.endswith(" goal_rows=%d guide=38x36" % (t + 1)) == (not footprint) and " goal_rows=%d guide=38x36" % (t + 1) in kernel, kernel
    assert kernel.startswith("k_rollout_barebone_crowd" if crowd else "k_rollout_barebone exact"), kernel
    want_rows = model_of(p, t)[1]
    assert_bits(rows, want_rows, "rows vs the model")
    assert len(np.unique(rows, axis=0)) > 5, "bad input: the carrots do not move"
    junk = np.float32([[9.0, -9.0], [-7.0, 3.0], [0.0, 0.0]])[:offset]
    twin.set_params(twin_params(p, np.concatenate([junk, rows])))
    twin.move_mppi_task_vars_to_device()
    twin.set_track_offset(offset)
    want, _, _, twin_kernel = rollout_with(twin, u_in, noise)
    assert " goal_rows=%d" % (t + 1 + offset) in twin_kernel and "guide" not in twin_kernel, twin_kernel
    assert_bits(costs, want, "%s, offset %d: the guide vs goal tracks of its rows" % (kind, offset))
    static = MPPI_Numba(cfg_of(N, t, crowd))
    static.set_params({k: v for k, v in p.items() if k != "guide"})
    static.move_mppi_task_vars_to_device()
    static.set_track_offset(offset)
    assert (rollout_with(static, u_in, noise)[0] != costs).any(), "bad input: the guide changes no cost"


@pytest.mark.parametrize("crowd", [False, True])
def test_costs_of_a_batch_equal_a_twin_with_goal_tracks(crowd):
    from mppi_numba_amd.barebone import MPPI_Batch
    B, t = 2, T
    p = room_task(crowd, False)
    x0s = np.float32([[0.0, 0.0, np.pi / 4], [2.5, 0.0, 2.0]])
    goals = np.float32([[2.6, 2.4], [0.0, 2.8]])
    rng = np.random.default_rng(6)
    pairs = [inputs(rng, N, t) for _ in range(B)]
    u_in, noise = np.stack([u for u, _ in pairs]), np.stack([e for _, e in pairs])
    guided, twin = MPPI_Batch(cfg_of(N, t, crowd), B), MPPI_Batch(cfg_of(N, t, crowd), B)
    guided.setup(p, x0s, goals)
    costs, _, _, kernel = rollout_with(guided, u_in, noise)
    assert kernel.endswith(" goal_rows=%d guide=38x36" % (t + 1)) and "problems=2" in kernel, kernel
    rows = guided.guide_rows()
    for b in range(B):
        assert_bits(rows[b], model_of(p, t, x0s[b], goals[b])[1], "problem %d: rows vs the model" % b)
    assert (rows[0] != rows[1]).any()
    twin.setup({k: v for k, v in p.items() if k != "guide"}, x0s, goals, goal_tracks=rows)
    want, _, _, twin_kernel = rollout_with(twin, u_in, noise)
    assert twin_kernel.endswith(" goal_rows=%d" % (t + 1)), twin_kernel
    assert_bits(costs, want, "a batch of two: the guide vs goal tracks of its rows")


# ---------------------------------------------------------------------- refresh
def loop_task(num_opt=2):
    return task_params(guide_of((0.0, 0.0), 0.1, (33, 31), inflate=0.0708, lead=0.6, pace=0.1), five_walls(), (0.15, 0.15, 0.8),
                       (2.9, 3.1), num_opt=num_opt)


def test_the_rows_follow_the_start_and_the_field_is_built_only_when_it_must():
    from mppi_numba_amd.barebone import MPPI_Numba
    p = loop_task()
    planner = MPPI_Numba(cfg_of(N, T, True))
    planner.setup(p)
    useq = planner.solve()
    assert planner.guide_fields_built == 1
    assert_bits(planner.guide_rows(), model_of(p, T)[1], "rows of the first solve")
    x1 = np.array([0.45, 0.62, 0.9])
    planner.shift_and_update(x1, useq, num_shifts=1)
    planner.solve()
    rows1 = model_of(p, T, x0=x1)[1]
    assert (rows1 != model_of(p, T)[1]).any(), "bad input: the rows do not move with the start"
    assert_bits(planner.guide_rows(), rows1, "rows of the second solve, from the new start")
    assert planner.guide_fields_built == 1, "a new start builds no field"
    # the same guide and walls again, as new objects: nothing
    planner.params["guide"] = dict(p["guide"])
    planner.params["wall_segments"] = p["wall_segments"].copy()
    planner.solve()
    assert planner.guide_fields_built == 1, "an unchanged hand-over builds no field"
    # a new goal: one build
    planner.params["xgoal"] = np.array([0.2, 2.2])
    planner.solve()
    assert planner.guide_fields_built == 2
    q = dict(p, xgoal=np.array([0.2, 2.2]))
    assert model_of(q, T, x0=x1)[2] == 0 and planner.guide_status() == 0
    assert (planner.guide_field() == model_of(q, T, x0=x1)[0]).all()
    # other walls: one build
    planner.params["wall_segments"] = p["wall_segments"] + np.float32([0.2, -0.1])
    planner.solve()
    assert planner.guide_fields_built == 3
    q["wall_segments"] = planner.params["wall_segments"]
    D, rows, _ = model_of(q, T, x0=x1)
    assert (planner.guide_field() == D).all()
    assert_bits(planner.guide_rows(), rows, "rows behind other walls")
    # another grid: one build
    planner.params["guide"] = dict(p["guide"], origin=(-0.05, 0.0))
    planner.solve()
    assert planner.guide_fields_built == 4
    # the key has gone: the static goal again
    planner.params.pop("guide")
    planner.solve()
    assert "goal_rows" not in planner.last_rollout_kernel()
    with pytest.raises(ValueError):
        planner.guide_rows()


def test_graph_replay_needs_no_new_capture_and_equals_the_direct_loop():
    """A batch, whose starts are read from device memory (the start of a single-problem handle is a launch argument, and a
    new one is a new capture with or without the guide)."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B = 2
    p = loop_task(num_opt=5)
    x0s = np.float32([[0.15, 0.15, 0.8], [2.9, 0.2, 2.0]])
    goals = np.float32([[2.9, 3.1], [0.2, 2.2]])
    direct, graphed = MPPI_Batch(cfg_of(N, T, True), B), MPPI_Batch(cfg_of(N, T, True), B)
    for planner in (direct, graphed):
        planner.setup(p, x0s, goals)
    graphed.set_graph_replay(True, 2)
    x, used, captures = x0s.copy(), None, None
    for step in range(4):
        a_, b_ = direct.solve(), graphed.solve()
        np.testing.assert_array_equal(a_, b_)
        used, x = x, x + np.float32([0.06, 0.05, 0.02])
        for planner in (direct, graphed):
            planner.shift_and_update_on_device(x, num_shifts=1)
        if step == 0:
            captures = graphed.graph_stats()["captures"]
            assert captures >= 1, graphed.graph_stats()
    stats = graphed.graph_stats()
    assert stats["captures"] == captures and stats["replays"] >= 4, "a refresh forced a new capture: %s after %d" % (stats, captures)
    assert graphed.guide_fields_built == 1
    for b in range(B):  # (used: the starts of the last solve)
        assert model_of(p, T, used[b], goals[b])[2] == 0, "bad input: problem %d has no carrots" % b
        assert_bits(graphed.guide_rows()[b], model_of(p, T, used[b], goals[b])[1], "problem %d: rows of the last solve" % b)


# ---------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_as_it_was():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Numba
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    lib = _lib.load()
    p = loop_task()
    planner = MPPI_Numba(cfg_of(N, T, True))
    planner.setup(p)
    planner.solve()
    kernel, rows = planner.last_rollout_kernel(), planner.guide_rows()
    good = dict(x_min=0.0, y_min=0.0, res=0.1, nx=31, ny=33, inflate=0.0708, lead=0.6, pace=0.1)

    def set_guide(handle, **changes):
        a = dict(good, **changes)
        return lib.mppi_planner_set_guide(handle, 1, a["x_min"], a["y_min"], a["res"], a["nx"], a["ny"], a["inflate"], a["lead"], a["pace"])

    bad = [(dict(x_min=np.nan), "finite"), (dict(res=np.inf), "finite"), (dict(lead=-np.inf), "finite"), (dict(res=0.0), "resolution"),
           (dict(res=-0.1), "resolution"), (dict(nx=0), "cells"), (dict(ny=-3), "cells"), (dict(nx=193, ny=192), "cells"),
           (dict(inflate=0.0707), "inflate"), (dict(inflate=-1.0), "inflate"), (dict(lead=-0.1), "lead"), (dict(pace=-0.1), "pace"),
           (dict(res=1e-6, inflate=1e-6, pace=1e3), "2^31"), (dict(res=1e-6, inflate=1e-6, lead=3e38), "2^31")]
    for changes, word in bad:
        assert set_guide(planner._handle, **changes) == ERR_INVALID, changes
        assert word in lib.mppi_last_error().decode(), (changes, lib.mppi_last_error().decode())
    assert set_guide(planner._handle) == 0  # (what it holds: nothing happens)
    track = np.ascontiguousarray(np.float32([[1.0, 1.0], [2.0, 2.0]]))
    assert lib.mppi_planner_set_goal_tracks(planner._handle, 1, 2, _lib.ptr(track, C.c_float)) == ERR_INVALID
    assert "guide" in lib.mppi_last_error().decode()
    planner.solve()
    assert planner.last_rollout_kernel() == kernel and planner.guide_fields_built == 1
    assert_bits(planner.guide_rows(), rows, "the rows after the refusals")
    # the key beside a goal track, a bad shape, no xgoal: ValueError, and the handle goes on
    for broken in (dict(p, goal_track=track), dict(p, guide=dict(p["guide"], shape=(33,))), dict(p, guide=dict(p["guide"], shape=(200, 200))),
                   {k: v for k, v in p.items() if k != "xgoal"}):
        planner.set_params(broken)
        with pytest.raises(ValueError):
            planner.solve()
    planner.set_params(dict(p, guide=dict(p["guide"], inflate=0.05)))  # (the library's refusal through the mirror)
    with pytest.raises(_lib.MppiError) as err:
        planner.solve()
    assert err.value.code == ERR_INVALID and "inflate" in str(err.value)
    planner.set_params(p)
    planner.solve()
    assert planner.last_rollout_kernel() == kernel
    # goal tracks held: the guide is refused, the tracks stay
    tracked = MPPI_Numba(cfg_of(N, T, False))
    tracked.setup({k: v for k, v in make_params(0.1, 1.0).items() if k != "xgoal"} | {"goal_track": track})
    tracked.solve()
    assert set_guide(tracked._handle) == ERR_INVALID and "goal tracks" in lib.mppi_last_error().decode()
    tracked.solve()
    assert tracked.last_rollout_kernel().endswith(" goal_rows=2")
    # a sharded handle
    cfg = _lib.PlannerCfg(device=0, mode=_lib.MODE_BAREBONE, num_control_rollouts=N, num_steps=T, num_grid_samples=1,
                          num_vis_state_rollouts=1, rng=_lib.RNG_PHILOX, math=_lib.MATH_EXACT, rank=0, world_size=2, num_instances=1, seed=1)
    handle = C.c_void_p()
    _lib.call("mppi_planner_create", C.byref(cfg), C.byref(handle))
    try:
        assert set_guide(handle) == ERR_INVALID and "unsharded" in lib.mppi_last_error().decode()
    finally:
        lib.mppi_planner_destroy(handle)
    # a map mode has no guide
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    assert set_guide(mapped._handle) == ERR_INVALID and "barebone" in lib.mppi_last_error().decode()
    assert np.isfinite(mapped.solve()).all()


# ---------------------------------------------------------------------- the room
def pocket():
    """A U-shaped pocket, open to the left, with the goal behind its closed end and the robot inside, facing the closed end."""
    from mppi_numba_amd.barebone import guide_grid, polyline_walls
    seg = polyline_walls([(-1.5, 1.0), (1.5, 1.0), (1.5, -1.0), (-1.5, -1.0)])
    hw = np.float32(0.05)
    p = make_params(0.1, 1.0, num_opt=2)
    p["x0"], p["xgoal"] = np.array([0.5, 0.0, 0.0]), np.array([3.2, 0.0])
    p["goal_tolerance"] = 0.3
    p["wall_segments"], p["wall_halfwidth"] = seg, hw
    return p, seg, hw, guide_grid(seg, 0.1, margin=2.0)


def test_the_robot_leaves_the_pocket_and_arrives():
    from mppi_numba_amd.barebone import MPPI_Numba
    p, seg, hw, (origin, shape) = pocket()
    guided = dict(p, guide=guide_of(origin, 0.1, shape, inflate=0.3, lead=0.45, pace=0.15))
    n, t, max_steps = 1024, 30, 250
    # the model's carrot path exists, and it leaves the pocket by its mouth: far longer than the straight line
    grid = model.Grid(origin, 0.1, shape, 0.3)
    D, rows, status = model_of(guided, t)
    c0 = (int(model.cell_of(0.0, grid.y_min, grid.res, grid.ny)), int(model.cell_of(0.5, grid.x_min, grid.res, grid.nx)))
    assert status == 0 and D[c0] < model.UNREACHED and D[c0] > 12 * 60, "bad input: %d units from the start" % D[c0]
    assert rows[1][0] < 0.5, "bad input: the first carrot does not lead back to the mouth"
    outcome = {}
    for name, params in (("guide", guided), ("no guide", p)):
        planner = MPPI_Numba(cfg_of(n, t, True, seed=5))
        planner.setup(params)
        xhist, _, steps = planner.closed_loop(max_steps)
        path = xhist[:steps + 1, :2].astype(np.float32)
        hits = hit(path[:-1, None], path[1:, None], seg[None, :, 0], seg[None, :, 1], hw).any(axis=1)
        gap = float(np.hypot(*(xhist[steps, :2] - p["xgoal"])))
        outcome[name] = (steps, gap, int(hits.sum()))
        print("the pocket, %s: %d steps, %.2f m from the goal at the end, %d steps hit a wall" % ((name,) + outcome[name]))
    steps, gap, hits = outcome["guide"]
    assert steps < max_steps and gap < 0.3 + 1e-3, "no arrival within %d steps: %.2f m from the goal" % (max_steps, gap)
    assert hits == 0, "%d steps of the executed path hit a wall" % hits
