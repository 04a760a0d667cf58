"""Fleet mode of a batched barebone handle in crowd mode: MPPI_Batch.set_fleet, mppi_planner_set_fleet.  At the head of
every call that starts iterations the device rebuilds, for every problem, a wall set from the OTHER problems' current plans
(k_fleet_plans, k_fleet_walls) and k_rollout_barebone_crowd's CrowdWallTracks form reads it from "now".  Every comparison of
walls and costs here is bit for bit with tests/fleet_model.py (which tests/test_fleet_model.py pins on the CPU); the two
control loops are compared with each other the way test_gpu_barebone_goal_tracks compares them."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import fleet_model
from test_gpu_barebone_batch import ERR_INVALID, make_params, oracle_params, problem_params
from test_gpu_barebone_crowd import cfg_of, shape_of
from test_gpu_barebone_tracks import rollout_with, track_params
from test_gpu_barebone_walls import assert_bits, wall_params, without_walls
from crowd_model import hit_counts

pytestmark = pytest.mark.gpu

DT = 0.1
ROOM = np.float32([[[-4.0, -4.0], [4.0, -4.0]], [[4.0, -4.0], [4.0, 4.0]], [[-0.6, 0.9], [0.9, -0.6]]])  # two sides, one wall inside
ROOM_HW = np.float32([0.05, 0.05, 0.1])


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


@functools.lru_cache(maxsize=None)
def ring(B, n, t, seed, aimed=True, radius=None):
    """B robots on a ring, bound for the far side through the centre, where their plans meet (1.5 m for up to three robots:
    about twelve steps away; 3 m for more, where the neighbours stand 0.29 m apart -- nearer than any half-width used).
    radius: another ring -- 0.5 m puts three robots 0.87 m apart, so that plans of a few steps already meet.
    aimed: they face the centre, give or take 0.3 rad; else the start headings are random.  Controls per robot as
    test_gpu_barebone_crowd.inputs draws them, a few entries outside vrange / wrange so that the clip takes part; noise
    (B, n, t, 2).  Shared by the cases, never changed."""
    rng = np.random.default_rng(seed)
    radius = radius or (1.5 if B <= 3 else 3.0)
    angle = 0.3 + np.arange(B) * (2 * np.pi / B)
    where = radius * np.stack([np.cos(angle), np.sin(angle)], 1)
    heading = angle + np.pi + rng.uniform(-0.3, 0.3, B) if aimed else rng.uniform(-np.pi, np.pi, B)
    x0s = np.concatenate([where, heading[:, None]], 1).astype(np.float32)
    goals = (-where).astype(np.float32)
    us = np.stack([rng.uniform(0.8, 1.8, (B, t)), rng.uniform(-0.2, 0.2, (B, t))], 2).astype(np.float32)
    us[:, 3, 1], us[:, 4, 0], us[:, 7, 0], us[0, 9, 1] = 40.0, -1.0, 5.0, -40.0
    noise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    for a in (x0s, goals, us, noise):
        a.setflags(write=False)
    return x0s, goals, us, noise


def fleet_ending(B, W, t):
    return " walls=%d wall_rows=%d fleet=%d" % (B - 1 + W, t, B)


def model_costs(params, x0s, goals, us, noise, hw, W, discs=None, rad=None, offset=0, goal_tracks=None):
    """(B, n) model costs; asserts on the way that the input means something: some (rollout, step) pair hits a fleet wall,
    and some problem's costs differ from those without the fleet."""
    B = len(x0s)
    walls = fleet_model.fleet_walls(params, x0s, us)
    out, hit_any, differs = [], False, False
    for b in range(B):
        track = None if goal_tracks is None else goal_tracks[b]
        pb = oracle_params(problem_params(params, x0s[b], goals[b] if track is None else track[0]))
        wt, h = fleet_model.reader_walls(walls[b], hw[b], ROOM[:W], ROOM_HW[:W])
        st = hit_counts(pb, np.zeros((0, 1, 2), np.float32), np.zeros(0, np.float32), noise[b], us[b])[1]
        hit_any = hit_any or bool(fleet_model.fleet_hits(st, wt[:B - 1], h[:B - 1]).any())
        costs = fleet_model.fleet_costs(pb, wt, h, noise[b], us[b], discs, rad, offset, track)
        differs = differs or bool((costs != fleet_model.fleet_costs(pb, wt[B - 1:], h[B - 1:], noise[b], us[b], discs, rad, offset, track)).any())
        out.append(costs)
    assert hit_any, "bad input: no (rollout, step) pair hits a fleet wall"
    assert differs, "bad input: the fleet changes no problem's costs"
    return np.stack(out)


@pytest.mark.parametrize("B,t,wscale", [(B, t, wscale) for B in (2, 3, 66) for t in (12, 37) for wscale in (1.0, 1.5)])
def test_walls_equal_the_model(B, t, wscale):
    """Random start headings, random controls with entries outside vrange / wrange.  66 robots: 65 walls a reader, more than
    one tile of the crowd kernel's and more than a wave of k_fleet_plans' lanes; T = 37 is no multiple of the eight steps
    k_fleet_plans walks at a time, T = 12 fewer than a wave's 64."""
    from mppi_numba_amd.barebone import MPPI_Batch
    x0s, goals, us, _ = ring(B, 64, t, 100 * B + t, aimed=False)
    params = make_params(DT, wscale)
    radii = np.random.default_rng(B).uniform(0.1, 0.4, B)
    batch = MPPI_Batch(cfg_of(64, t, True), B)
    batch.setup(params, x0s, goals)
    assert batch.fleet is None
    batch.set_fleet(radii, margin=0.05)
    assert batch.fleet[1] == 0.05 and (batch.fleet[0] == radii.astype(np.float32)).all()
    seg, hw, others = batch.fleet_walls()
    assert seg.shape == (B, B - 1, t, 2, 2) and (seg == np.float32(1e18)).all()  # (before the first refresh: nobody's walls)
    batch.set_u(us)
    batch.refresh_fleet()
    seg, hw, others = batch.fleet_walls()
    np.testing.assert_array_equal(others, fleet_model.others(B))
    assert_bits(hw, fleet_model.halfwidths(radii, 0.05, B), "half-widths")
    want = fleet_model.fleet_walls(params, x0s, us)
    assert (want[:, :, :, 0] != want[:, :, :, 1]).any()
    assert_bits(seg, want, "%d robots, %d steps: the walls vs the model" % (B, t))


COST_CASES = [(3, 128, 37, W, discs, wscale, False) for W, wscale in ((0, 1.0), (3, 1.5)) for discs in (None, 0, 5)]
COST_CASES += [(3, 128, 37, 3, 5, 1.0, True), (66, 64, 12, 0, None, 1.0, False)]


@pytest.mark.parametrize("B,n,t,W,discs,wscale,goal", COST_CASES)
def test_costs_equal_the_model(B, n, t, W, discs, wscale, goal):
    """B = 3, N = 128 (two tiles a problem), T = 37: more than one chunk and no multiple of the counters.  discs: None, or 70
    shared disc tracks read at that offset -- the fleet rows ignore it.  goal: a goal track per problem on top.  66 robots:
    65 fleet walls cross the tile of 64 walls."""
    from mppi_numba_amd.barebone import MPPI_Batch, constant_velocity_tracks
    x0s, goals, us, noise = ring(B, n, t, 7 * B + t)
    rng = np.random.default_rng(W + 17)
    params = make_params(DT, wscale)
    if W:
        params = wall_params(params, ROOM[:W], ROOM_HW[:W])
    tracks = rad = None
    if discs is not None:
        tracks = constant_velocity_tracks(rng.uniform(-1.5, 1.5, (70, 2)), rng.normal(0, 0.4, (70, 2)), DT, t + 6)
        rad = rng.uniform(0.1, 0.3, 70).astype(np.float32)
        params = track_params(params, tracks, rad)
    gtracks = None
    if goal:
        gtracks = [constant_velocity_tracks(goals[b][None], rng.normal(0, 0.5, (1, 2)), DT, 20)[0] for b in range(B)]
    radii, margin = np.linspace(0.2, 0.3, B), 0.02
    hw = fleet_model.halfwidths(radii, margin, B)
    plain = without_walls({k: v for k, v in params.items() if not k.startswith("obstacle_")})
    model = model_costs(plain, x0s, goals, us, noise, hw, W, tracks, rad, discs or 0, gtracks)
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(params, x0s, goals, goal_tracks=gtracks)
    batch.set_fleet(radii, margin)
    batch.move_mppi_task_vars_to_device()  # (hands the disc tracks over: offset 0)
    if discs:
        batch.set_track_offset(discs)
    costs, _, _, kernel = rollout_with(batch, us, noise.reshape(B * n, t, 2))
    shape_of(kernel)
    if goal:
        assert fleet_ending(B, W, t) + " goal_rows=20" in kernel and kernel.endswith(" goal_rows=20"), kernel
    else:
        assert kernel.endswith(fleet_ending(B, W, t)), kernel
    assert ("rotation=1" in kernel) == (wscale == 1.0) and "exact=1" in kernel and "problems=%d" % B in kernel, kernel
    assert ("tracks=%d" % (t + 6) in kernel) == (discs is not None), kernel
    np.testing.assert_array_equal(batch.track_offset, np.full(B, discs or 0))  # (the fleet neither resets nor advances it)
    for b in range(B):
        assert_bits(costs[b], model[b], "robot %d of %d, %d room walls, discs at %s vs the model" % (b, B, W, discs))


def _euler(x, u0, dt):
    """barebone_mppi_numba.ipynb cell 7 in float64 (see test_gpu_barebone_batch._notebook_loop)."""
    u = u0.astype(np.float64)
    return np.array([x[0] + dt * np.cos(x[2]) * u[0], x[1] + dt * np.sin(x[2]) * u[0], x[2] + dt * u[1]])


def test_the_refresh_follows_the_handle():
    """The first solve starts from zero controls: every plan stands at its start.  After the solve and shift_and_update the
    next rollout() is given walls made of the new controls and start states; set_fleet(None) gives back the bits of a
    handle that never had a fleet."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t = 3, 128, 37
    x0s, _, us, noise = ring(B, n, t, 5, radius=0.5)
    goals = (-8.0 * x0s[:, :2]).astype(np.float32)
    params = make_params(DT, 1.0)
    hw = fleet_model.halfwidths(0.25, 0.1, B)
    batch = MPPI_Batch(cfg_of(n, t, True, seed=4), B)
    batch.setup(params, x0s, goals)
    batch.set_fleet(0.25, margin=0.1)
    useqs = batch.solve()
    seg, _, others = batch.fleet_walls()
    for a in range(B):
        for k, b in enumerate(others[a]):
            assert_bits(seg[a, k], np.broadcast_to(x0s[b, :2], (t, 2, 2)).copy(), "first solve: robot %d stands" % b)
    assert batch.last_rollout_kernel().endswith(fleet_ending(B, 0, t)), batch.last_rollout_kernel()
    x = np.stack([_euler(x0s[b].astype(np.float64), useqs[b, 0], DT) for b in range(B)])
    batch.shift_and_update(x, useqs, num_shifts=1)
    shifted = useqs.copy()
    shifted[:, :-1] = useqs[:, 1:]
    new_x0s = x.astype(np.float32)
    flat = noise.reshape(B * n, t, 2)
    batch.set_noise(flat)
    batch.rollout()
    costs = batch.costs_d.copy_to_host()
    assert_bits(batch.u_cur_d.copy_to_host(), shifted, "the controls the refresh saw")
    seg, _, _ = batch.fleet_walls()
    want = fleet_model.fleet_walls(params, new_x0s, shifted)
    assert (want != fleet_model.fleet_walls(params, x0s, shifted)).any() and (want != fleet_model.fleet_walls(params, new_x0s, us)).any()
    assert_bits(seg, want, "the walls after solve and shift_and_update vs the model")
    model = model_costs(params, new_x0s, goals, shifted, noise, hw, 0)
    for b in range(B):
        assert_bits(costs[b], model[b], "robot %d after solve and shift_and_update vs the model" % b)
    np.testing.assert_array_equal(batch.track_offset, np.zeros(B))
    # off again: a handle that never had a fleet
    batch.set_fleet(None)
    assert batch.fleet is None
    got, _, _, kernel = rollout_with(batch, shifted, flat)
    never = MPPI_Batch(cfg_of(n, t, True, seed=4), B)
    never.setup(params, new_x0s, goals)
    plain, _, _, plain_kernel = rollout_with(never, shifted, flat)
    assert "fleet" not in kernel and kernel == plain_kernel, (kernel, plain_kernel)
    assert_bits(got, plain, "fleet off vs a handle that never had one")
    assert (got != costs).any()


@pytest.mark.parametrize("goal_track", [False, True])
def test_closed_loop_equals_the_host_loop(goal_track):
    """Two batches with the same seed: the loop on the device, and solve, float64 Euler step and shift_and_update from the
    host.  The goals are out of reach, so nobody finishes; xhist, uhist, the steps and the track offsets, bit for bit.  With
    a shared goal track of T + 6 rows the offsets advance -- and the fleet rows stay counted from "now"."""
    from mppi_numba_amd.barebone import MPPI_Batch, constant_velocity_tracks
    B, n, t, max_steps = 3, 128, 20, 6
    x0s, _, _, _ = ring(B, n, t, 11, radius=0.5)
    goals = (-8.0 * x0s[:, :2]).astype(np.float32)  # 4.5 m away: 0.2 m a step at the most
    params = make_params(DT, 1.0, num_opt=2)
    if goal_track:
        params = {k: v for k, v in params.items() if k != "xgoal"}
        params["goal_track"] = constant_velocity_tracks([[9.0, 9.0]], [[0.5, -0.5]], DT, t + 6)[0]
    host, dev, loose = (MPPI_Batch(cfg_of(n, t, True, seed=6), B) for _ in range(3))
    for planner in (host, dev, loose):
        planner.setup(params, x0s, goals)
    for planner in (host, dev):
        planner.set_fleet(0.25, margin=0.05)
    x = x0s.astype(np.float64)
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
    assert fleet_ending(B, 0, t) in kernel and kernel.endswith(" goal_rows=%d" % (t + 6) if goal_track else fleet_ending(B, 0, t)), kernel
    got_x, got_u, got_steps = dev.closed_loop(max_steps)
    assert dev.last_rollout_kernel() == kernel
    np.testing.assert_array_equal(got_steps, np.full(B, max_steps))
    np.testing.assert_array_equal(dev.track_offset, host.track_offset)
    np.testing.assert_array_equal(dev.track_offset, np.full(B, max_steps if goal_track else 0))
    np.testing.assert_array_equal(got_u.view(np.int32), want_u.view(np.int32))
    np.testing.assert_array_equal(got_x.view(np.int64), want_x.view(np.int64))
    _, loose_u, _ = loose.closed_loop(max_steps)
    assert (loose_u != got_u).any(), "bad input: the fleet changes no control of the loop"


def test_a_robot_at_its_goal_is_parked():
    """Robot 2 starts 0.58 m from its goal (tolerance 0.5 m, up to 0.2 m a step) and arrives early.  From then on every
    other reader's rows for it are the degenerate segment at its final float32 position; the others' rows are the model's on
    the controls and start states the last control step began with -- those of a twin loop, same seed, one step shorter."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t, max_steps = 3, 128, 20, 6
    x0s, _, _, _ = ring(B, n, t, 11, radius=0.5)
    goals = (-8.0 * x0s[:, :2]).astype(np.float32)
    goals[2] = x0s[2, :2] + 0.58 * np.float32([np.cos(x0s[2, 2]), np.sin(x0s[2, 2])])
    params = make_params(DT, 1.0, num_opt=2)
    dev, twin = (MPPI_Batch(cfg_of(n, t, True, seed=6), B) for _ in range(2))
    for planner in (dev, twin):
        planner.setup(params, x0s, goals)
        planner.set_fleet(0.25, margin=0.05)
    xhist, _, steps = dev.closed_loop(max_steps)
    print("parked: steps", steps)
    assert steps[2] < max_steps - 1 and (steps[:2] == max_steps).all(), "bad input: robot 2 does not arrive early (%s)" % steps
    seg, _, others = dev.fleet_walls()
    _, _, twin_steps = twin.closed_loop(max_steps - 1)
    assert twin_steps[2] == steps[2]
    before_u = twin.u_cur_d.copy_to_host()
    np.testing.assert_array_equal(twin.x0s[:2], xhist[:2, max_steps - 1].astype(np.float32))
    want = fleet_model.fleet_walls(params, twin.x0s, before_u, parked=np.array([False, False, True]))
    final = xhist[2, steps[2], :2].astype(np.float32)
    for a in (0, 1):
        k = list(others[a]).index(2)
        assert_bits(seg[a, k], np.broadcast_to(final, (t, 2, 2)).copy(), "reader %d: the parked robot's rows" % a)
    assert (want[2, :, :, 0] != want[2, :, :, 1]).any()
    assert_bits(seg, want, "the rows of the last control step vs the model")


def test_solve_under_graph_replay():
    """A direct loop and a replayed one in step, equal at every solve over four control steps.  The refresh writes into
    arrays that stay where they are: after the first control step nothing is captured again."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t = 3, 128, 20
    x0s, _, _, _ = ring(B, n, t, 11, radius=0.5)
    goals = (-8.0 * x0s[:, :2]).astype(np.float32)
    params = make_params(DT, 1.0, num_opt=5)
    direct, graphed, loose = (MPPI_Batch(cfg_of(n, t, True), B) for _ in range(3))
    for planner in (direct, graphed, loose):
        planner.setup(params, x0s, goals)
    for planner in (direct, graphed):
        planner.set_fleet(0.25, margin=0.05)
    graphed.set_graph_replay(True, 2)
    x, captures, differs = x0s.astype(np.float64), None, False
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
    assert graphed.last_rollout_kernel().endswith(fleet_ending(B, 0, t)), graphed.last_rollout_kernel()
    stats = graphed.graph_stats()
    assert stats["captures"] == captures, "a refresh forced a new capture: %s after %d" % (stats, captures)
    assert stats["replays"] >= 6, stats
    assert_bits(graphed.fleet_walls()[0], direct.fleet_walls()[0], "the walls of the last refresh")


def test_mode_and_error_handling():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba, constant_velocity_walls
    B, n, t = 3, 64, 12
    x0s, goals, us, noise = ring(B, n, t, 3)
    params = make_params(DT, 1.0)
    half = np.full((B, B - 1), 0.5, np.float32)

    def refused(handle, count, hw, word):
        with pytest.raises(_lib.MppiError) as err:
            _lib.call("mppi_planner_set_fleet", handle, count, None if hw is None else _lib.ptr(hw, C.c_float))
        assert err.value.code == ERR_INVALID and word in str(err.value), str(err.value)

    single = MPPI_Numba(cfg_of(n, t, True))  # not batched
    single.setup(params)
    refused(single._handle, 1, half, "batched")
    one = MPPI_Batch(cfg_of(n, t, True), 1)  # B < 2
    one.setup(params)
    with pytest.raises(_lib.MppiError) as err:
        one.set_fleet(0.25)
    assert err.value.code == ERR_INVALID and "at least two" in str(err.value), str(err.value)
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)  # not barebone
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    refused(mapped._handle, 1, half, "barebone")
    batch = MPPI_Batch(cfg_of(n, t, False), B)  # not in crowd mode
    batch.setup(params, x0s, goals)
    with pytest.raises(_lib.MppiError) as err:
        batch.set_fleet(0.25)
    assert err.value.code == ERR_INVALID and "crowd" in str(err.value), str(err.value)
    assert batch.fleet is None
    batch.set_crowd(True)
    refused(batch._handle, 2, half, "num_instances")  # count is 0 or B
    bad = half.copy()
    bad[1, 0] = -0.1
    refused(batch._handle, B, bad, "half-width")
    with pytest.raises(ValueError):
        batch.set_fleet([0.2, np.nan, 0.2])
    with pytest.raises(ValueError):
        batch.fleet_walls()
    on = C.c_int(-1)
    _lib.call("mppi_planner_get_fleet", batch._handle, C.byref(on))
    assert on.value == 0
    with pytest.raises(_lib.MppiError):
        _lib.call("mppi_planner_fleet_refresh", batch._handle)
    # per-problem wall sets held: the fleet is refused, and the handle behaves as before
    wsets = [(constant_velocity_walls(ROOM, np.zeros((3, 2)), DT, 5, at=0.0), ROOM_HW)] * B
    batch.set_wall_sets(wsets)
    with pytest.raises(ValueError):
        batch.set_fleet(0.25)
    refused(batch._handle, B, half, "wall")
    held, _, _, kernel = rollout_with(batch, us, noise.reshape(B * n, t, 2))
    assert kernel.endswith(" walls=3 wall_rows=5"), kernel
    other = MPPI_Batch(cfg_of(n, t, True), B)
    other.setup(params, x0s, goals, wall_sets=wsets)
    want, _, _, _ = rollout_with(other, us, noise.reshape(B * n, t, 2))
    assert_bits(held, want, "user wall tracks after a refused set_fleet")
    batch.set_wall_sets(None)
    # the fleet on: one owner of the per-problem sets, and crowd mode is held
    batch.set_fleet(0.25)
    _lib.call("mppi_planner_get_fleet", batch._handle, C.byref(on))
    assert on.value == B
    with pytest.raises(ValueError):
        batch.set_wall_sets(wsets)
    counts = np.full(B, 3, np.int32)
    segs = np.ascontiguousarray(np.concatenate([w[0] for w in wsets]).reshape(-1, 4))
    hws = np.ascontiguousarray(np.concatenate([w[1] for w in wsets]))
    with pytest.raises(_lib.MppiError) as err:
        _lib.call("mppi_planner_set_wall_tracks", batch._handle, B, _lib.ptr(counts, C.c_int), 5, _lib.ptr(segs, C.c_float),
                  _lib.ptr(hws, C.c_float))
    assert err.value.code == ERR_INVALID and "fleet" in str(err.value), str(err.value)
    with pytest.raises(_lib.MppiError) as err:
        batch.set_crowd(False)
    assert err.value.code == ERR_INVALID and "fleet" in str(err.value), str(err.value)
    assert batch.crowd
    tracked = dict(params)
    tracked["wall_tracks"], tracked["wall_halfwidth"] = wsets[0]
    batch.set_params(dict(tracked, x0=x0s[0], xgoal=goals[0]))
    with pytest.raises(ValueError):
        batch.solve()
    batch.set_params(dict(params, x0=x0s[0], xgoal=goals[0]))
    got, _, _, kernel = rollout_with(batch, us, noise.reshape(B * n, t, 2))  # (refused calls: the fleet is as it was)
    assert kernel.endswith(fleet_ending(B, 0, t)), kernel
    model = model_costs(params, x0s, goals, us, noise, half, 0)
    for b in range(B):
        assert_bits(got[b], model[b], "robot %d after the refused calls vs the model" % b)
    # static walls set while the fleet is on: the storage is rebuilt with them
    batch.set_params(dict(wall_params(params, ROOM, ROOM_HW), x0=x0s[0], xgoal=goals[0]))
    got, _, _, kernel = rollout_with(batch, us, noise.reshape(B * n, t, 2))
    assert kernel.endswith(fleet_ending(B, 3, t)), kernel
    model = model_costs(params, x0s, goals, us, noise, half, 3)
    for b in range(B):
        assert_bits(got[b], model[b], "robot %d with the room vs the model" % b)
    batch.set_fleet(None)
    _, _, _, kernel = rollout_with(batch, us, noise.reshape(B * n, t, 2))
    assert kernel.endswith(" walls=3"), kernel


def _corridor_fleet(seed, fleet):
    """The corridor of test_gpu_barebone_wall_tracks.test_two_robots_meet_in_a_corridor -- two robots of radius 0.25 m meet
    head-on in a corridor 2.4 m wide and would swap places -- as ONE batch of two in closed_loop: both plan at once, each
    against the other's plan of the previous control step, where that test plans in turn.  Returns the smallest true
    clearance of the executed motion (both move linearly within a control step: 16 samples per step) and the steps."""
    from mppi_numba_amd.barebone import Config, MPPI_Batch
    T, dt, max_steps, reach = 30, 0.1, 90, 0.5
    corridor = np.float32([[[-2.0, 1.2], [8.0, 1.2]], [[-2.0, -1.2], [8.0, -1.2]]])
    starts, goals = np.array([[0.0, 0.0, 0.0], [6.0, 0.0, np.pi]]), np.array([[6.0, 0.0], [0.0, 0.0]])
    cfg = Config(T=(T + 0.5) * dt, dt=dt, num_control_rollouts=1024, num_vis_state_rollouts=4, seed=seed,
                 enforce_recommended_limits=False, crowd=True)
    batch = MPPI_Batch(cfg, 2)
    batch.setup(dict(dt=dt, x0=starts[0].copy(), xgoal=goals[0], goal_tolerance=0.3, dist_weight=10, lambda_weight=1.0,
                     num_opt=2, u_std=np.array([1.0, 1.0]), vrange=np.array([0.0, 2.0]), wrange=np.array([-np.pi, np.pi]),
                     obs_penalty=1e6, wall_segments=corridor, wall_halfwidth=np.float32(0.05)), starts, goals)
    if fleet:
        batch.set_fleet(0.25)
    xhist, _, steps = batch.closed_loop(max_steps)
    kernel = batch.last_rollout_kernel()
    assert kernel.endswith(fleet_ending(2, 2, T) if fleet else " walls=2"), kernel
    clearance = np.inf
    s = np.linspace(0.0, 1.0, 16)[:, None]
    for step in range(int(steps.max())):
        a = [xhist[r, min(step, steps[r]), :2] for r in range(2)]      # (a robot at its goal stands)
        b = [xhist[r, min(step + 1, steps[r]), :2] for r in range(2)]
        gap = (a[0] + s * (b[0] - a[0])) - (a[1] + s * (b[1] - a[1]))
        clearance = min(clearance, np.linalg.norm(gap, axis=1).min() - reach)
    return clearance, steps


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_robots_meet_in_a_corridor_planning_at_once(seed):
    """The parameters are those of the in-turn test, written down once and not tuned.  The run with the fleet off drives
    through the other robot (negative clearance: the input means something); the fleet keeps the executed motion apart.  (On
    the MI355X, with these first parameters, seeds 1 / 2 / 3: smallest clearance with the fleet 0.110 / 0.022 / 0.126 m in 30
    to 33 control steps, with the fleet off -0.472 / -0.086 / -0.263 m -- so >= 0 held at once and is asserted.)"""
    clear_fleet, steps_fleet = _corridor_fleet(seed, True)
    clear_loose, steps_loose = _corridor_fleet(seed, False)
    print("seed %d: fleet: smallest clearance %.4f m, steps %s; fleet off: %.4f m, steps %s"
          % (seed, clear_fleet, steps_fleet, clear_loose, steps_loose))
    assert clear_loose < 0.0, "bad input: without the fleet the robots do not touch"
    assert clear_fleet > clear_loose
    assert clear_fleet >= 0.0, "the robots that avoid each other's plans touched"
