"""A fleet of bodies: MPPI_Batch.set_fleet_bodies, mppi_planner_set_fleet_bodies -- fleet mode for robots that are up to
eight discs attached to their pose.  At the head of every call that starts iterations the device rebuilds, for every
problem, a wall set from the OTHER problems' plans and headings (k_fleet_plans<., true>, k_fleet_body_centres,
k_fleet_body_walls), and the footprint forms of k_rollout_barebone_crowd count one hit per robot, however many of its body
discs' walls are hit (crowd_fold.h).  Walls and costs are compared bit for bit with tests/fleet_body_model.py on the inputs
of tests/fleet_body_cases.py, which tests/test_fleet_body_model.py checks on the CPU.  The model's states are the exact
ones, so the comparisons with it run in exact math; in fast math the statements made are the equalities between handles."""
import ctypes as C
import gc

import numpy as np
import pytest

import fleet_body_cases as cases
import fleet_body_model as M
import fleet_model
import footprint_model
from test_gpu_barebone_batch import ERR_INVALID, make_params
from test_gpu_barebone_crowd import cfg_of, shape_of
from test_gpu_barebone_fleet import ROOM, ROOM_HW, _euler, fleet_ending, ring
from test_gpu_barebone_tracks import rollout_with, track_params
from test_gpu_barebone_walls import assert_bits, wall_params

pytestmark = pytest.mark.gpu

DT = cases.DT
N = cases.N


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


def ending(B, F, W, t):
    """How the description of a launch in a fleet of bodies ends (ahead of " goal_rows=", " samples=" where they apply)."""
    return " walls=%d wall_rows=%d fleet=%d" % ((B - 1) * M.group_size(F) + W, t, B), " footprint=%d" % F


def fleet_of(case, n=N, math="exact", t=None, seed=3, goal_tracks=None, params=None):
    from mppi_numba_amd.barebone import MPPI_Batch
    B = len(case["x0s"])
    batch = MPPI_Batch(cfg_of(n, t or case["us"].shape[1], True, math=math, seed=seed), B)
    batch.setup(params or case["params"], case["x0s"], case["goals"], goal_tracks=goal_tracks)
    batch.set_fleet_bodies(case["footprint"], case["margin"])
    return batch


# ---- 1. the walls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.WALL_CASES, ids=str)
def test_walls_equal_the_model(case):
    """Random start headings, random controls with entries outside vrange / wrange.  F = 1, 3, 8: one, four and eight slots a
    robot; 66 robots: more than one tile of slots and more than a block of the scatter; T = 37 is no multiple of the eight
    steps k_fleet_plans walks at a time; T = 70: the second block of 64 steps of the plan walk, and the final heading behind
    it."""
    B, F, t, wscale = case
    held = cases.wall_case(*case)
    batch = fleet_of(held)
    rows, margin = batch.fleet_bodies
    assert margin == held["margin"] and (rows == held["footprint"]).all()
    np.testing.assert_array_equal(batch.footprint, held["footprint"])
    seg, hw, others = batch.fleet_body_walls()
    assert seg.shape == (B, B - 1, F, t, 2, 2) and (seg == np.float32(1e18)).all()  # (before the first refresh: nobody's walls)
    batch.set_u(held["us"])
    batch.refresh_fleet()
    seg, hw, others = batch.fleet_body_walls()
    np.testing.assert_array_equal(others, fleet_model.others(B))
    assert_bits(hw, held["hw"], "half-widths")
    assert_bits(seg, held["walls"], "%d robots of %d discs, %d steps: the walls vs the model" % (B, F, t))


# ---- 2. the costs --------------------------------------------------------------------------------------------------------
def check_costs(batch, held, kernel_tail=""):
    B, n, t = len(held["x0s"]), held["noise"].shape[1], held["us"].shape[1]
    F, W, model = len(held["footprint"]), held["W"], held["model"]
    cases.the_input_means_something(model)
    costs, _, _, kernel = rollout_with(batch, held["us"], held["noise"].reshape(B * n, t, 2))
    shape_of(kernel)
    fleet, foot = ending(B, F, W, t)
    assert fleet in kernel and kernel.endswith(kernel_tail + foot) and "exact=1" in kernel and "problems=%d" % B in kernel, kernel
    for b in range(B):
        assert_bits(costs[b], model["costs"][b], "robot %d of %d, %d body discs, %d room walls vs the model" % (b, B, F, W))
    return kernel


@pytest.mark.parametrize("case", cases.COST_CASES, ids=str)
def test_costs_equal_the_model(case):
    """(B = 3, F = 3, W = 2): 8 grouped slots, then singles in one tile.  (10, 8, 3): 72 grouped slots, the groups span two
    tiles.  (18, 3, 2): 68 grouped slots, a tile boundary at a group boundary and the statics behind.  n = 64 a problem,
    T = 12 and 37, the heading by rotation (wscale 1.0) and by the full sincos (1.5).  On the model's counts at least a tenth
    of every reader's rollouts hit some robot, at least a tenth hit none, and counting per robot gives strictly fewer hits
    than counting per slot: a kernel that counted per slot, or missed hits, could not pass."""
    B, F, W, t, wscale = case
    held = cases.cost_case(*case)
    params = wall_params(held["params"], ROOM[:W], ROOM_HW[:W])
    kernel = check_costs(fleet_of(held, params=params), held)
    assert ("rotation=1" in kernel) == (wscale == 1.0), kernel


@pytest.mark.parametrize("kind", cases.EXTRA_CASES)
def test_costs_with_disc_tracks_a_goal_track_and_disc_samples(kind):
    """(3, 3, 2), T = 37 with 70 shared disc tracks read at offset 5 (the fleet rows ignore it), with a goal track per
    problem, and with three disc samples at alpha = 0.5 (the walls are counted once, for every sample)."""
    held = cases.extra_case(kind)
    W, t = held["W"], held["us"].shape[1]
    params = wall_params(held["params"], ROOM[:W], ROOM_HW[:W])
    if kind == "disc_tracks":
        batch = fleet_of(held, params=track_params(params, held["tracks"], held["rad"]))
        batch.move_mppi_task_vars_to_device()  # (hands the disc tracks over: offset 0)
        batch.set_track_offset(cases.TRACK_OFFSET)
        kernel = check_costs(batch, held)
        assert "tracks=%d" % (t + 6) in kernel, kernel
        np.testing.assert_array_equal(batch.track_offset, np.full(3, cases.TRACK_OFFSET))
    elif kind == "goal_track":
        check_costs(fleet_of(held, params=params, goal_tracks=held["goal_tracks"]), held, " goal_rows=20")
    else:
        params = dict(params, obstacle_track_samples=held["samples"], obstacle_radius=held["rad"], cvar_alpha=cases.ALPHA)
        check_costs(fleet_of(held, params=params), held, " samples=3 numel=2")


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("t,W", [(12, 0), (37, 3)])
def test_a_one_disc_body_is_the_disc_fleet(math, t, W):
    """Body (0, 0, rho), rho and margin dyadic: the costs of set_fleet(rho, margin) on the same inputs, bit for bit -- and
    the same again with the row given three and eight times, where the others' walls fill four and eight slots a robot
    that must count once.  In fast math the states are the fast ones in every handle: the formula is the same."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n = 3, 128
    rho, margin = cases.DYADIC
    x0s, goals, us, noise = ring(B, n, t, 7 * B + t)
    params = make_params(DT, 1.0)
    room_hw = np.float32([0.0625, 0.0625, 0.125])  # (dyadic as well: h + rho is exact in float32)
    if W:
        params = wall_params(params, ROOM[:W], room_hw[:W] + np.float32(rho))  # (the disc fleet's reader is a point to them)
    flat = noise.reshape(B * n, t, 2)
    discs = MPPI_Batch(cfg_of(n, t, True, math=math), B)
    discs.setup(params, x0s, goals)
    discs.set_fleet(rho, margin)
    want, _, _, kernel = rollout_with(discs, us, flat)
    assert kernel.endswith(fleet_ending(B, W, t)), kernel
    loose = MPPI_Batch(cfg_of(n, t, True, math=math), B)
    loose.setup(params, x0s, goals)
    assert (rollout_with(loose, us, flat)[0] != want).any(), "bad input: the fleet changes no cost"
    if W:
        params = wall_params(params, ROOM[:W], room_hw[:W])  # (the body adds rho itself)
    for copies in (1, 3, 8):
        body = np.float32([[0.0, 0.0, rho]] * copies)
        batch = MPPI_Batch(cfg_of(n, t, True, math=math), B)
        batch.setup(params, x0s, goals)
        batch.set_fleet_bodies(body, margin)
        got, _, _, kernel = rollout_with(batch, us, flat)
        fleet, foot = ending(B, copies, W, t)
        assert kernel.endswith(fleet + foot) and "exact=%d" % (math == "exact") in kernel, kernel
        assert_bits(got, want, "%s math, the row %d times vs the disc fleet" % (math, copies))


# ---- 3. refresh and loop -------------------------------------------------------------------------------------------------
def loop_case(n=128, t=20, num_opt=2):
    B = 3
    x0s, _, _, _ = ring(B, n, t, 11, radius=0.8)
    goals = (-8.0 * x0s[:, :2]).astype(np.float32)  # out of reach: 0.2 m a step at the most
    return dict(params=make_params(DT, 1.0, num_opt=num_opt), x0s=x0s, goals=goals, footprint=cases.body(3), margin=0.05,
                us=np.zeros((B, t, 2), np.float32))


def test_the_refresh_follows_the_handle():
    """The first solve starts from zero controls: every plan stands at its start pose.  After the solve and
    shift_and_update the next rollout() is given walls made of the new controls and start states -- set_u and
    set_instances --, and its costs are the model's on them; set_fleet(None) gives back the kernel and the bits of a
    handle that never had a fleet."""
    from mppi_numba_amd.barebone import MPPI_Batch, body_discs
    B, n, t = 3, 128, 37
    held = loop_case(n, t, num_opt=1)
    x0s, goals, params, body = held["x0s"], held["goals"], held["params"], held["footprint"]
    noise = np.random.default_rng(5).normal(0, 1.0, (B, n, t, 2)).astype(np.float32)
    batch = fleet_of(held, n, seed=4)
    useqs = batch.solve()
    seg, _, others = batch.fleet_body_walls()
    for a in range(B):
        for o, b in enumerate(others[a]):
            stand = body_discs(x0s[b], body)
            assert_bits(seg[a, o], np.broadcast_to(stand[:, None, None, :], (3, t, 2, 2)).copy(), "first solve: robot %d stands" % b)
    fleet, foot = ending(B, 3, 0, t)
    assert batch.last_rollout_kernel().endswith(fleet + foot), batch.last_rollout_kernel()
    x = np.stack([_euler(x0s[b].astype(np.float64), useqs[b, 0], DT) for b in range(B)])
    batch.shift_and_update(x, useqs, num_shifts=1)
    shifted = useqs.copy()
    shifted[:, :-1] = useqs[:, 1:]
    new_x0s = x.astype(np.float32)
    flat = noise.reshape(B * n, t, 2)
    batch.set_noise(flat)
    batch.rollout()
    costs = batch.costs_d.copy_to_host()
    seg, _, _ = batch.fleet_body_walls()
    want = M.body_walls(params, new_x0s, shifted, body)
    assert (want != M.body_walls(params, x0s, shifted, body)).any() and (want != M.body_walls(params, new_x0s, useqs, body)).any()
    assert_bits(seg, want, "the walls after solve and shift_and_update vs the model")
    model = cases.model_of(params, new_x0s, goals, shifted, noise, body, 0.05, 0)
    assert model["hit_some"].any() and model["grouped"].sum() < model["per_slot"].sum(), "bad input: nothing is hit"
    for b in range(B):
        assert_bits(costs[b], model["costs"][b], "robot %d after solve and shift_and_update vs the model" % b)
    batch.set_fleet(None)
    assert batch.fleet_bodies is None and batch.fleet is None and batch.footprint is None
    got, _, _, kernel = rollout_with(batch, shifted, flat)
    never = MPPI_Batch(cfg_of(n, t, True, seed=4), B)
    never.setup(params, new_x0s, goals)
    plain, _, _, plain_kernel = rollout_with(never, shifted, flat)
    assert "fleet" not in kernel and "footprint" not in kernel and kernel == plain_kernel, (kernel, plain_kernel)
    assert_bits(got, plain, "fleet off vs a handle that never had one")
    assert (got != costs).any()


def test_closed_loop_equals_the_host_loop():
    """Two batches with the same seed: the loop on the device, and solve, float64 Euler step and shift_and_update from the
    host.  The goals are out of reach, so nobody finishes; xhist, uhist and the steps, bit for bit."""
    B, n, t, max_steps = 3, 128, 20, 6
    held = loop_case(n, t)
    host, dev = fleet_of(held, n, seed=6), fleet_of(held, n, seed=6)
    from mppi_numba_amd.barebone import MPPI_Batch
    loose = MPPI_Batch(cfg_of(n, t, True, seed=6), B)
    loose.setup(held["params"], held["x0s"], held["goals"])
    x = held["x0s"].astype(np.float64)
    want_x, want_u = np.full((B, max_steps + 1, 3), np.nan), np.full((B, max_steps, 2), np.nan, np.float32)
    want_x[:, 0] = x
    for step in range(max_steps):
        useqs = host.solve()
        for b in range(B):
            want_u[b, step] = useqs[b, 0]
            x[b] = _euler(x[b], useqs[b, 0], DT)
            want_x[b, step + 1] = x[b]
        host.shift_and_update(x, useqs, num_shifts=1)
    kernel = host.last_rollout_kernel()
    fleet, foot = ending(B, 3, 0, t)
    assert kernel.endswith(fleet + foot), kernel
    got_x, got_u, got_steps = dev.closed_loop(max_steps)
    assert dev.last_rollout_kernel() == kernel
    np.testing.assert_array_equal(got_steps, np.full(B, max_steps))
    np.testing.assert_array_equal(got_u.view(np.int32), want_u.view(np.int32))
    np.testing.assert_array_equal(got_x.view(np.int64), want_x.view(np.int64))
    _, loose_u, _ = loose.closed_loop(max_steps)
    assert (loose_u != got_u).any(), "bad input: the fleet changes no control of the loop"


def test_a_robot_at_its_goal_is_parked_with_its_heading():
    """Robot 2 starts 0.58 m from its goal (tolerance 0.5 m) and arrives early.  From then on every other reader's rows for
    it are the degenerate segments at the body centres of its final float32 pose, heading included; the others' rows are the
    model's on the controls and start states the last control step began with -- those of a twin loop, one step shorter."""
    from mppi_numba_amd.barebone import body_discs
    B, n, t, max_steps = 3, 128, 20, 6
    held = loop_case(n, t)
    x0s = held["x0s"]
    goals = held["goals"].copy()
    goals[2] = x0s[2, :2] + 0.58 * np.float32([np.cos(x0s[2, 2]), np.sin(x0s[2, 2])])
    held = dict(held, goals=goals)
    dev, twin = fleet_of(held, n, seed=6), fleet_of(held, n, seed=6)
    xhist, _, steps = dev.closed_loop(max_steps)
    print("parked: steps", steps)
    assert steps[2] < max_steps - 1 and (steps[:2] == max_steps).all(), "bad input: robot 2 does not arrive early (%s)" % steps
    seg, _, others = dev.fleet_body_walls()
    _, _, twin_steps = twin.closed_loop(max_steps - 1)
    assert twin_steps[2] == steps[2]
    before_u = twin.u_cur_d.copy_to_host()
    np.testing.assert_array_equal(twin.x0s[:2], xhist[:2, max_steps - 1].astype(np.float32))
    want = M.body_walls(held["params"], twin.x0s, before_u, held["footprint"], parked=np.array([False, False, True]))
    final = xhist[2, steps[2]].astype(np.float32)
    assert final[2] != x0s[2, 2] or steps[2] == 0
    stand = body_discs(final, held["footprint"])
    for a in (0, 1):
        o = list(others[a]).index(2)
        assert_bits(seg[a, o], np.broadcast_to(stand[:, None, None, :], (3, t, 2, 2)).copy(), "reader %d: the parked robot's rows" % a)
    assert (want[2, :, :, :, 0] != want[2, :, :, :, 1]).any()
    assert_bits(seg, want, "the rows of the last control step vs the model")


def test_solve_under_graph_replay():
    """A direct loop and a replayed one in step, equal at every solve over four control steps.  The refresh writes into
    arrays that stay where they are: after the first control step nothing is captured again."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t = 3, 128, 20
    held = loop_case(n, t, num_opt=5)
    direct, graphed = fleet_of(held, n), fleet_of(held, n)
    loose = MPPI_Batch(cfg_of(n, t, True), B)
    loose.setup(held["params"], held["x0s"], held["goals"])
    graphed.set_graph_replay(True, 2)
    x, captures, differs = held["x0s"].astype(np.float64), None, False
    for step in range(4):
        a_, b_, c_ = direct.solve(), graphed.solve(), loose.solve()
        np.testing.assert_array_equal(a_, b_)
        differs = differs or not np.array_equal(a_, c_)
        x = np.stack([_euler(x[b], a_[b, 0], DT) for b in range(B)])
        for planner in (direct, graphed, loose):
            planner.shift_and_update_on_device(x, num_shifts=1)
        if step == 0:
            captures = graphed.graph_stats()["captures"]
            assert captures >= 1, graphed.graph_stats()
    assert differs, "bad input: the fleet changes no solve"
    fleet, foot = ending(B, 3, 0, t)
    assert graphed.last_rollout_kernel().endswith(fleet + foot), graphed.last_rollout_kernel()
    stats = graphed.graph_stats()
    assert stats["captures"] == captures, "a refresh forced a new capture: %s after %d" % (stats, captures)
    assert stats["replays"] >= 6, stats
    assert_bits(graphed.fleet_body_walls()[0], direct.fleet_body_walls()[0], "the walls of the last refresh")


# ---- 4. modes and errors -------------------------------------------------------------------------------------------------
def test_mode_and_error_handling():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba, constant_velocity_walls
    lib = _lib.load()
    B, n, t = 3, 64, 12
    x0s, goals, us, noise = ring(B, n, t, 3)
    flat = noise.reshape(B * n, t, 2)
    params = make_params(DT, 1.0)
    body = cases.body(3)
    half = np.full((B, B - 1), 0.5, np.float32)

    def raw(planner, count, rows, margin=0.05):
        rows = np.ascontiguousarray(rows, np.float32)
        return lib.mppi_planner_set_fleet_bodies(planner._handle, count, _lib.ptr(rows, C.c_float), len(rows), C.c_double(margin))

    def refused(planner, count, rows, word, margin=0.05):
        assert raw(planner, count, rows, margin) == ERR_INVALID and word in lib.mppi_last_error().decode(), lib.mppi_last_error().decode()

    single = MPPI_Numba(cfg_of(n, t, True))  # not batched
    single.setup(params)
    refused(single, 1, body, "batched")
    one = MPPI_Batch(cfg_of(n, t, True), 1)  # B < 2
    one.setup(params)
    with pytest.raises(_lib.MppiError) as err:
        one.set_fleet_bodies(body)
    assert err.value.code == ERR_INVALID and "at least two" in str(err.value), str(err.value)
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)  # not barebone
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    refused(mapped, 1, body, "barebone")
    batch = MPPI_Batch(cfg_of(n, t, False), B)  # not in crowd mode
    batch.setup(params, x0s, goals)
    with pytest.raises(_lib.MppiError) as err:
        batch.set_fleet_bodies(body)
    assert err.value.code == ERR_INVALID and "crowd" in str(err.value), str(err.value)
    assert batch.fleet_bodies is None
    batch.set_crowd(True)
    plain_costs, _, _, plain_kernel = rollout_with(batch, us, flat)
    refused(batch, 2, body, "num_instances")  # count is 0 or B
    refused(batch, B, np.zeros((9, 3)), "9")  # 1 .. 8 discs
    assert lib.mppi_planner_set_fleet_bodies(batch._handle, B, None, 0, C.c_double(0.0)) == ERR_INVALID
    negative = body.copy()
    negative[1, 2] = -0.1
    refused(batch, B, negative, "negative")
    broken = body.copy()
    broken[2, 0] = np.nan
    refused(batch, B, broken, "finite")
    refused(batch, B, body, "margin", margin=np.inf)
    refused(batch, B, body, "half-width", margin=-0.3)  # rho + margin < 0
    for bad in (np.zeros((9, 3)), np.zeros((0, 3)), np.zeros((3, 2)), negative, broken):
        with pytest.raises(ValueError):
            batch.set_fleet_bodies(bad)
    with pytest.raises(ValueError):
        batch.set_fleet_bodies(body, margin=np.nan)
    with pytest.raises(ValueError):
        batch.fleet_body_walls()
    count, margin = C.c_int(-1), C.c_double(-1.0)
    _lib.call("mppi_planner_get_fleet_bodies", batch._handle, C.byref(count), C.byref(margin))
    assert count.value == 0 and batch.footprint is None
    # a footprint held through set_footprint, per-problem wall sets: refused, and the handle behaves as before
    batch.set_params(dict(params, footprint=body, x0=x0s[0], xgoal=goals[0]))
    with pytest.raises(ValueError) as verr:
        batch.set_fleet_bodies(body)
    assert "footprint" in str(verr.value)
    batch.move_mppi_task_vars_to_device()
    refused(batch, B, body, "footprint")
    batch.set_params(dict(params, x0=x0s[0], xgoal=goals[0]))
    batch.move_mppi_task_vars_to_device()
    wsets = [(constant_velocity_walls(ROOM, np.zeros((3, 2)), DT, 5, at=0.0), ROOM_HW)] * B
    batch.set_wall_sets(wsets)
    with pytest.raises(ValueError):
        batch.set_fleet_bodies(body)
    refused(batch, B, body, "wall")
    batch.set_wall_sets(None)
    got, _, _, kernel = rollout_with(batch, us, flat)
    assert kernel == plain_kernel
    assert_bits(got, plain_costs, "after the refused calls")
    # the fleet of bodies on
    batch.set_fleet_bodies(body, 0.05)
    _lib.call("mppi_planner_get_fleet_bodies", batch._handle, C.byref(count), C.byref(margin))
    on = C.c_int(-1)
    _lib.call("mppi_planner_get_fleet", batch._handle, C.byref(on))
    assert count.value == 3 and margin.value == 0.05 and on.value == B
    np.testing.assert_array_equal(batch.footprint, body)
    assert raw(batch, B, body, 0.05) == 0  # (the same arguments again: a no-op)
    _, _, _, kernel = rollout_with(batch, us, flat)
    fleet, foot = ending(B, 3, 0, t)
    assert kernel.endswith(fleet + foot), kernel
    with pytest.raises(ValueError):
        batch.fleet_walls()
    seg = np.empty((B, B - 1, t, 2, 2), np.float32)
    assert lib.mppi_planner_get_fleet_walls(batch._handle, _lib.ptr(seg, C.c_float)) == ERR_INVALID
    assert "mppi_planner_get_fleet_body_walls" in lib.mppi_last_error().decode()
    with pytest.raises(ValueError):  # the disc fleet: through off
        batch.set_fleet(0.25)
    assert lib.mppi_planner_set_fleet(batch._handle, B, _lib.ptr(half, C.c_float)) == ERR_INVALID
    both = lib.mppi_last_error().decode()
    assert "mppi_planner_set_fleet_bodies" in both and "mppi_planner_set_fleet:" in both, both
    rows = np.ascontiguousarray(body)
    assert lib.mppi_planner_set_footprint(batch._handle, _lib.ptr(rows, C.c_float), 3) == ERR_INVALID  # a footprint, its clear included
    assert "fleet" in lib.mppi_last_error().decode()
    assert lib.mppi_planner_set_footprint(batch._handle, None, 0) == ERR_INVALID and "fleet" in lib.mppi_last_error().decode()
    batch.set_params(dict(params, footprint=body, x0=x0s[0], xgoal=goals[0]))
    with pytest.raises(ValueError) as verr:
        batch.solve()
    assert "fleet" in str(verr.value)
    batch.set_params(dict(params, x0=x0s[0], xgoal=goals[0]))
    with pytest.raises(ValueError):
        batch.set_wall_sets(wsets)
    tracked = dict(params, x0=x0s[0], xgoal=goals[0])
    tracked["wall_tracks"], tracked["wall_halfwidth"] = wsets[0]
    batch.set_params(tracked)
    with pytest.raises(ValueError):
        batch.solve()
    batch.set_params(dict(params, x0=x0s[0], xgoal=goals[0]))
    with pytest.raises(_lib.MppiError) as err:
        batch.set_crowd(False)
    assert err.value.code == ERR_INVALID and "fleet" in str(err.value), str(err.value)
    np.testing.assert_array_equal(batch.footprint, body)  # (refused calls: the fleet is as it was)
    # static walls set while the fleet is on: the storage is rebuilt with them
    batch.set_params(dict(wall_params(params, ROOM, ROOM_HW), x0=x0s[0], xgoal=goals[0]))
    with_room, _, _, kernel = rollout_with(batch, us, flat)
    fleet, foot = ending(B, 3, 3, t)
    assert kernel.endswith(fleet + foot), kernel
    model = cases.model_of(params, x0s, goals, us, noise, body, 0.05, 3)
    for b in range(B):
        assert_bits(with_room[b], model["costs"][b], "robot %d with the room vs the model" % b)
    batch.set_params(dict(params, x0=x0s[0], xgoal=goals[0]))
    # off restores the kernel; the disc fleet and back go through off
    batch.set_fleet(None)
    assert batch.fleet_bodies is None and batch.footprint is None
    got, _, _, kernel = rollout_with(batch, us, flat)
    assert kernel == plain_kernel
    assert_bits(got, plain_costs, "the fleet of bodies off")
    batch.set_fleet(0.25)
    with pytest.raises(ValueError):
        batch.set_fleet_bodies(body)
    refused(batch, B, body, "mppi_planner_set_fleet_bodies")
    _, _, _, kernel = rollout_with(batch, us, flat)
    assert kernel.endswith(fleet_ending(B, 0, t)), kernel
    batch.set_fleet_bodies(None)
    batch.set_fleet_bodies(body, 0.05)
    _, _, _, kernel = rollout_with(batch, us, flat)
    fleet, foot = ending(B, 3, 0, t)
    assert kernel.endswith(fleet + foot), kernel


# ---- 5. two carts in a corridor ------------------------------------------------------------------------------------------
from fleet_body_cases import CART, CART_MARGIN, CORRIDOR, LOOP_STEPS, WALL_HW  # noqa: E402


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_carts_meet_in_a_corridor(seed):
    """Two carts 1.0 m x 0.4 m (rectangle_footprint(0.5, 0.5, 0.4): three discs) meet head-on in a corridor 1.8 m wide, as
    ONE batch of two in closed_loop with set_fleet_bodies(margin 0.05 m).  Both reach their goals within 120 control steps,
    and the float64 clearance of each cart's rectangle from the other's four edges and from the corridor walls is positive
    at every control step.  Corridor width 1.8 m and max_steps 120 were fixed on the first run on the MI355X, inside the
    bracket test_fleet_body_model.test_two_discs_cannot_pass_in_the_corridor states (1.19 m .. 2.26 m); that run, seeds
    1 / 2 / 3: both carts at their goals after 31 and 31 / 32 and 32 / 40 and 34 control steps, smallest clearance 0.1144 /
    0.0580 / 0.1874 m."""
    from mppi_numba_amd.barebone import Config, MPPI_Batch, rectangle_footprint
    T, dt = 30, 0.1
    starts, goals = np.array([[0.0, 0.0, 0.0], [6.0, 0.0, np.pi]]), np.array([[6.0, 0.0], [0.0, 0.0]])
    cfg = Config(T=(T + 0.5) * dt, dt=dt, num_control_rollouts=1024, num_vis_state_rollouts=4, seed=seed,
                 enforce_recommended_limits=False, crowd=True)
    batch = MPPI_Batch(cfg, 2)
    batch.setup(dict(dt=dt, x0=starts[0].copy(), xgoal=goals[0], goal_tolerance=0.3, dist_weight=10, lambda_weight=1.0,
                     num_opt=2, u_std=np.array([1.0, 1.0]), vrange=np.array([0.0, 2.0]), wrange=np.array([-np.pi, np.pi]),
                     obs_penalty=1e6, wall_segments=CORRIDOR, wall_halfwidth=np.float32(WALL_HW)), starts, goals)
    batch.set_fleet_bodies(rectangle_footprint(*CART), CART_MARGIN)
    xhist, _, steps = batch.closed_loop(LOOP_STEPS)
    fleet, foot = ending(2, 3, 2, T)
    assert batch.last_rollout_kernel().endswith(fleet + foot), batch.last_rollout_kernel()
    front, rear, width = CART
    corners = np.array([[front, width / 2], [-rear, width / 2], [-rear, -width / 2], [front, -width / 2]])
    clearance = np.inf
    for step in range(int(steps.max()) + 1):
        pose = [xhist[r, min(step, steps[r])] for r in range(2)]  # (a cart at its goal stands)
        for r in range(2):
            o = pose[1 - r]
            rot = np.array([[np.cos(o[2]), -np.sin(o[2])], [np.sin(o[2]), np.cos(o[2])]])
            world = o[:2] + corners @ rot.T
            edges = np.stack([world, np.roll(world, -1, axis=0)], 1)
            clearance = min(clearance, footprint_model.rectangle_clearance(pose[r][None], front, rear, width,
                                                                           np.concatenate([edges, CORRIDOR.astype(np.float64)]))[0])
    ends = [np.linalg.norm(xhist[r, steps[r], :2] - goals[r]) for r in range(2)]
    print("seed %d: steps %s, ends %.3f / %.3f m from the goals, smallest clearance %.4f m" % (seed, steps, ends[0], ends[1], clearance))
    assert (steps < LOOP_STEPS).all() and max(ends) <= np.float32(0.3), "a cart does not reach its goal within %d steps: %s" % (LOOP_STEPS, steps)
    assert clearance > 0.0, "the carts touched each other or a wall"
