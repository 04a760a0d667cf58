"""Discs that move in the barebone planner: params['obstacle_tracks'] (K, L, 2) / track sets of barebone.MPPI_Batch, row j
a disc's centre at time j*dt from "now" = row `track_offset`; the state after step t is tested against row
min(track_offset + t + 1, L - 1).

The reference planner has no moving obstacles.  The oracle for them is two-fold: tracks that do not move must give the
bits of the static discs (and so of oracle.rollout_barebone), and tracks that move must give the bits of the numpy cost
model of tests/track_model.py, which itself equals the oracle bit for bit on constant tracks (tests/test_track_model.py).
All comparisons are bit for bit unless a tolerance is named."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_barebone_batch import (ERR_INVALID, _notebook_loop, assert_bits, make_cfg, make_params, oracle_params,
                                     problem_params, problems, random_discs, run_batch)
from track_model import track_costs

pytestmark = pytest.mark.gpu

# the shape table of test_gpu_barebone_batch.test_batch_matches_single_handles_and_oracle
SHAPES = [
    (2, 64, 30, 0, 1.0),      # rotation (pi * 0.1 <= 0.36), no discs
    (5, 1024, 50, 2, 1.0),    # the notebook's shape per problem: KD = 2 form
    (64, 64, 50, 3, 1.0),     # KD = 4 form, many problems
    (5, 64, 30, 7, 1.0),      # run-time disc loop
    (2, 1024, 30, 2, 1.5),    # full sincos (1.5 pi * 0.1 > 0.36)
    (64, 1024, 50, 2, 1.0),   # 1024 workgroups
    (5, 64, 50, 3, 2.0),      # full sincos with discs
]
OBS_PENALTY = 1e6  # make_params


def cfg_of(n, t, math="exact", seed=3):
    cfg = make_cfg(n, t, seed=seed)
    cfg.math = math
    return cfg


def form_of(n_discs, rotation):
    return "discs=loop" if not rotation or n_discs > 4 else ("discs<=2" if n_discs <= 2 else "discs<=4")


def track_params(params, tracks, radii):
    p = dict(params)
    p.pop("obstacle_positions", None)
    p["obstacle_tracks"], p["obstacle_radius"] = tracks, radii
    return p


def moving_tracks(rng, pos, dt, rows):
    """Discs that keep a velocity of about 0.6 m/s in a random direction."""
    from mppi_numba_amd.barebone import constant_velocity_tracks
    heading = rng.uniform(-np.pi, np.pi, len(pos))
    speed = rng.uniform(0.4, 0.8, len(pos))
    return constant_velocity_tracks(pos, np.stack([speed * np.cos(heading), speed * np.sin(heading)], axis=1), dt, rows)


def rollout_with(planner, u_in, noise):
    planner.set_u(u_in)
    planner.set_noise(noise)
    planner.rollout()
    costs = planner.costs_d.copy_to_host()
    kernel = planner.last_rollout_kernel()
    planner.update()
    return costs, planner.u_cur_d.copy_to_host(), planner.weights_d.copy_to_host(), kernel


def static_case(B, n, t, n_discs, wscale, math):
    """The static-disc batch of a row of the table after run_batch: what the track handles are compared with."""
    from mppi_numba_amd.barebone import MPPI_Batch
    rng = np.random.default_rng(B * 1000 + n + t + n_discs)
    cfg = cfg_of(n, t, math)
    x0s, goals = problems(rng, B)
    pos, rad = random_discs(rng, n_discs, x0s[0], goals[0]) if n_discs else (np.zeros((0, 2), np.float32), np.zeros(0, np.float32))
    params = make_params(cfg.dt, wscale, (pos, rad) if n_discs else None)
    batch = MPPI_Batch(cfg, B)
    batch.setup(params, x0s, goals)
    u_in, noise, costs, kernel, u_out, weights = run_batch(batch, rng)
    assert "tracks" not in kernel, kernel
    return rng, cfg, x0s, goals, pos, rad, params, u_in, noise, costs, u_out, weights


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("B,n,t,n_discs,wscale", SHAPES)
def test_constant_tracks_equal_static_discs(B, n, t, n_discs, wscale, math):
    """The only statement made about fast math: the track form is the same code on the same operands."""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    rng, cfg, x0s, goals, pos, rad, params, u_in, noise, costs, u_out, weights = static_case(B, n, t, n_discs, wscale, math)
    L = t + 1 if n_discs != 3 else 1
    tparams = track_params(params, np.repeat(pos[:, None], L, 1), rad)
    rotation = math == "exact" and wscale == 1.0
    batch = MPPI_Batch(cfg_of(n, t, math), B)
    batch.setup(tparams, x0s, goals)
    got, got_u, got_w, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    assert "tracks=%d" % L in kernel and "problems=%d" % B in kernel and form_of(n_discs, rotation) in kernel, kernel
    assert ("rotation=1" in kernel) == rotation and ("exact=1" in kernel) == (math == "exact"), kernel
    assert_bits(got, costs, "batch costs, constant tracks vs static discs")
    assert_bits(got_w, weights, "batch weights")
    assert_bits(got_u, u_out, "batch u")
    single = MPPI_Numba(cfg_of(n, t, math))
    for b in range(B):
        single.set_params(problem_params(tparams, x0s[b], goals[b]))
        want, want_u, want_w, kernel = rollout_with(single, u_in[b], noise[b])
        assert "tracks=%d" % L in kernel and "problems" not in kernel and form_of(n_discs, rotation) in kernel, kernel
        assert_bits(want, costs[b], "problem %d: single handle with constant tracks vs static batch" % b)
        assert_bits(want_u, u_out[b], "problem %d u" % b)
        assert_bits(want_w, weights[b], "problem %d weights" % b)
        if math == "exact":
            ref = O.rollout_barebone(oracle_params(problem_params(params, x0s[b], goals[b])), pos, rad, noise[b], u_in[b])
            assert_bits(got[b], ref, "problem %d costs vs oracle" % b)


def turning_tracks(pos, dt, rows):
    """Hand-made, not linear: disc 0 drives a quarter circle of radius 1.5 m at 0.6 m/s, then stands; disc 1 goes back and
    forth along x."""
    j = np.arange(rows) * dt
    angle = np.minimum(0.6 * j / 1.5, np.pi / 2)
    tr = np.repeat(np.asarray(pos, np.float64)[:, None], rows, 1)
    tr[0, :, 0] += 1.5 * np.sin(angle)
    tr[0, :, 1] -= 1.5 * (1.0 - np.cos(angle))
    tr[1, :, 0] += 0.8 * np.sin(2.0 * j)
    return tr.astype(np.float32)


@pytest.mark.parametrize("B,n,t,n_discs,wscale,kind", [row + ("velocity",) for row in SHAPES] + [(5, 1024, 50, 2, 1.0, "turning")])
def test_moving_tracks_equal_the_model(B, n, t, n_discs, wscale, kind):
    """Exact math.  Before anything is compared with the model the case must show that moving matters: at least 10 % of
    its rollouts' costs differ from the static-disc costs at row 0 and some exceed obs_penalty -- a case where that fails
    is a bad input, not a pass.  (The table's row without discs has nothing that can move: it checks the empty track set
    against the model and the static costs only.)"""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    rng, cfg, x0s, goals, pos, rad, params, u_in, noise, costs, _, _ = static_case(B, n, t, n_discs, wscale, "exact")
    L = t + 1
    tracks = turning_tracks(pos, cfg.dt, L) if kind == "turning" else moving_tracks(rng, pos, cfg.dt, L)
    assert tracks.shape == (n_discs, L, 2) and (tracks[:, 0] == pos).all()
    tparams = track_params(params, tracks, rad)
    batch = MPPI_Batch(cfg_of(n, t), B)
    batch.setup(tparams, x0s, goals)
    got, got_u, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    assert "tracks=%d" % L in kernel and "problems=%d" % B in kernel and form_of(n_discs, wscale == 1.0) in kernel, kernel
    changed = float((got != costs).mean())
    print("moving tracks: %.1f %% of %d costs differ from the static discs at row 0; %d above obs_penalty"
          % (100 * changed, got.size, int((got > OBS_PENALTY).sum())))
    if n_discs:
        assert changed >= 0.10, "bad input: only %.1f %% of the costs differ from the static discs" % (100 * changed)
        assert (got > OBS_PENALTY).any(), "bad input: no rollout is inside a disc"
    else:
        assert changed == 0.0
    single = MPPI_Numba(cfg_of(n, t))
    for b in range(B):
        pb = problem_params(tparams, x0s[b], goals[b])
        model = track_costs(oracle_params(pb), tracks, rad, noise[b], u_in[b])
        assert_bits(got[b], model, "problem %d of the batch vs the model" % b)
        single.set_params(pb)
        want, want_u, _, kernel = rollout_with(single, u_in[b], noise[b])
        assert "tracks=%d" % L in kernel and "problems" not in kernel, kernel
        assert_bits(want, model, "problem %d, single handle vs the model" % b)
        assert_bits(got_u[b], want_u, "problem %d u, batch vs single handle" % b)


def test_offset_and_clamp():
    from mppi_numba_amd.barebone import MPPI_Numba
    rng = np.random.default_rng(11)
    n, t = 1024, 50
    cfg = cfg_of(n, t)
    x0, goal = np.float32([0.0, 0.0, np.pi / 4]), np.float32([7.0, 5.0])
    pos, rad = random_discs(rng, 3, x0, goal)
    L = t + 1
    tracks = moving_tracks(rng, pos, cfg.dt, L)
    params = make_params(cfg.dt, 1.0)
    u_in = np.stack([rng.uniform(0.5, 1.8, t), rng.uniform(-0.5, 0.5, t)], 1).astype(np.float32)
    noise = rng.normal(0, 1, (n, t, 2)).astype(np.float32)
    op = oracle_params(params)
    planner = MPPI_Numba(cfg)

    def costs_of(tr, offset):
        planner.set_params(track_params(params, tr, rad))
        planner.move_mppi_task_vars_to_device()  # (hands the tracks over: new tracks put the offset back to 0)
        planner.set_track_offset(offset)
        assert planner.track_offset == offset
        planner.set_u(u_in)
        planner.set_noise(noise)
        planner.rollout()
        return planner.costs_d.copy_to_host()

    base = costs_of(tracks, 0)
    assert_bits(base, track_costs(op, tracks, rad, noise, u_in), "offset 0 vs the model")
    for s in (1, 5, 23):
        shifted = costs_of(tracks, s)
        assert (shifted != base).any()
        assert_bits(shifted, track_costs(op, tracks, rad, noise, u_in, offset=s), "offset %d vs the model" % s)
        assert_bits(shifted, costs_of(np.ascontiguousarray(tracks[:, s:]), 0), "offset %d vs sliced tracks" % s)
    last = O.rollout_barebone(op, tracks[:, -1], rad, noise, u_in)
    for s in (L - 1, L + 7):
        assert_bits(costs_of(tracks, s), last, "offset %d: static discs at the last row (oracle)" % s)
    first = O.rollout_barebone(op, tracks[:, 0], rad, noise, u_in)
    for s in (0, 9):
        assert_bits(costs_of(np.ascontiguousarray(tracks[:, :1]), s), first, "L = 1, offset %d" % s)
        assert "tracks=1" in planner.last_rollout_kernel()
    # new tracks put the offset back to 0; reset() too
    planner.set_params(track_params(params, tracks, rad))
    planner.rollout()
    assert planner.track_offset == 0 and "tracks=%d" % L in planner.last_rollout_kernel()
    planner.set_track_offset(4)
    planner.reset()
    assert planner.track_offset == 0


@pytest.mark.parametrize("counts,form", [
    ([2, 0, 1, 2, 0], "discs<=2"),
    ([4, 0, 2, 3, 1], "discs<=4"),
    ([33, 0, 5, 2, 17], "discs=loop"),
])
def test_per_problem_track_sets_and_offsets(counts, form):
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    B, n, t = len(counts), 128, 30
    L = t + 1
    rng = np.random.default_rng(sum(counts))
    cfg = cfg_of(n, t)
    x0s, goals = problems(rng, B)
    shared = random_discs(rng, 2, x0s[0], goals[0])
    params = make_params(cfg.dt, 1.0, shared)
    static_sets = [random_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate(counts)]
    sets = [(moving_tracks(rng, pos, cfg.dt, L), rad) for pos, rad in static_sets]
    offsets = np.array([0, 3, 7, 12, 40], dtype=np.int32)
    batch = MPPI_Batch(cfg, B)
    batch.setup(params, x0s, goals, obstacle_sets=sets)
    u_in, noise, _, _, _, _ = run_batch(batch, rng)
    batch.set_track_offset(offsets)
    np.testing.assert_array_equal(batch.track_offset, offsets)
    costs, u_out, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    assert form in kernel and "tracks=%d" % L in kernel and "problems=%d" % B in kernel and "rotation=1" in kernel, kernel
    single = MPPI_Numba(cfg_of(n, t))
    bare = dict(params)
    bare.pop("obstacle_positions"), bare.pop("obstacle_radius")
    for b in range(B):
        pb = track_params(problem_params(bare, x0s[b], goals[b]), sets[b][0], sets[b][1])
        single.set_params(pb)
        single.move_mppi_task_vars_to_device()  # (hands the set over: offset 0)
        single.set_track_offset(int(offsets[b]))
        want, want_u, _, _ = rollout_with(single, u_in[b], noise[b])
        assert_bits(costs[b], want, "problem %d (%d tracks, offset %d) vs single handle" % (b, counts[b], offsets[b]))
        assert_bits(u_out[b], want_u, "problem %d u vs single handle" % b)
        assert_bits(costs[b], track_costs(oracle_params(pb), sets[b][0], sets[b][1], noise[b], u_in[b], offset=int(offsets[b])),
                    "problem %d vs the model" % b)
    if counts[0] >= 4:
        assert (costs[0] > 1e5).any(), "some rollouts of the problem with the most discs must hit one"
    # the same sets again: no change, the offsets stay
    batch.set_obstacle_sets(sets)
    np.testing.assert_array_equal(batch.track_offset, offsets)
    again, _, _, _ = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    assert_bits(again, costs, "same sets again")
    # back to the shared static set
    batch.set_obstacle_sets(None)
    back, _, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    assert "tracks" not in kernel and "discs<=2" in kernel and "own_discs" not in kernel, kernel
    for b in range(B):
        p = problem_params(params, x0s[b], goals[b])
        assert_bits(back[b], O.rollout_barebone(oracle_params(p), shared[0], shared[1], noise[b], u_in[b]),
                    "problem %d, shared static set again" % b)


def loop_tracks(dt, rows):
    """The notebook's two discs (cell 5), drifting."""
    from mppi_numba_amd.barebone import constant_velocity_tracks
    return constant_velocity_tracks([[5, 4.5], [2, 1]], [[-0.15, 0.1], [0.1, 0.15]], dt, rows), np.array([1.5, 1.0])


@pytest.mark.parametrize("max_steps", [60, 20])
def test_closed_loop_equals_the_notebook_loop_with_tracks(max_steps):
    """As test_gpu_barebone_batch.test_closed_loop_equals_the_notebook_loop, same tolerances; the host loop advances the
    track offset in shift_and_update, the device loop in its step kernel."""
    from mppi_numba_amd.barebone import MPPI_Numba
    cfg = make_cfg(1000, 50, seed=1)
    tracks, rad = loop_tracks(cfg.dt, 40)  # (shorter than the loop plus horizon: the clamp takes part)
    params = track_params(make_params(cfg.dt, 1.0), tracks, rad)
    host = MPPI_Numba(cfg)
    host.setup(params)
    want_x, want_u, want_steps = _notebook_loop(host, cfg, params["x0"], params["xgoal"], params["goal_tolerance"], max_steps)
    assert "tracks=40" in host.last_rollout_kernel()
    assert (want_steps < max_steps) == (max_steps == 60)
    assert host.track_offset == want_steps
    dev = MPPI_Numba(make_cfg(1000, 50, seed=1))
    dev.setup(params)
    got_x, got_u, got_steps = dev.closed_loop(max_steps)
    assert "tracks=40" in dev.last_rollout_kernel()
    assert got_steps == want_steps
    assert dev.track_offset == got_steps
    ran = want_steps
    np.testing.assert_array_equal(np.isnan(got_x), np.isnan(want_x))
    np.testing.assert_allclose(got_u[:ran], want_u[:ran], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_x[:ran + 1], want_x[:ran + 1], rtol=0, atol=1e-5)
    if ran == max_steps:
        np.testing.assert_allclose(dev.solve(), host.solve(), rtol=0, atol=2e-5)


def test_closed_loop_of_a_batch_advances_each_running_problem():
    from mppi_numba_amd.barebone import MPPI_Batch
    B, max_steps = 3, 40
    rng = np.random.default_rng(21)
    cfg = make_cfg(256, 30)
    x0s, goals = problems(rng, B)
    sets = [(moving_tracks(rng, pos, cfg.dt, 45), rad)
            for pos, rad in (random_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate((1, 0, 6)))]
    batch = MPPI_Batch(cfg, B)
    batch.setup(make_params(cfg.dt, 1.0), x0s, goals, obstacle_sets=sets)
    before = np.array([2, 0, 5], dtype=np.int32)
    batch.set_track_offset(before)
    xhist, uhist, steps = batch.closed_loop(max_steps)
    assert "tracks=45" in batch.last_rollout_kernel()
    np.testing.assert_array_equal(batch.track_offset, before + steps)
    assert steps[-1] < max_steps and steps.max() > steps[-1]  # the goal within reach is reached early: it stopped advancing
    for b in range(B):
        k = int(steps[b])
        assert np.isnan(xhist[b, k + 1:]).all() and np.isfinite(xhist[b, :k + 1]).all()


def test_graph_replay_with_tracks():
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t = 4, 128, 30
    rng = np.random.default_rng(9)
    x0s, goals = problems(rng, B)
    static_sets = [random_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate((2, 0, 3, 1))]
    track_sets = [(moving_tracks(rng, pos, 0.1, t + 1), rad) for pos, rad in static_sets]
    params = make_params(0.1, 1.0, num_opt=5)
    stats = {}
    for kind, sets in (("static", static_sets), ("tracks", track_sets)):
        direct, graphed = MPPI_Batch(make_cfg(n, t), B), MPPI_Batch(make_cfg(n, t), B)
        for planner in (direct, graphed):
            planner.setup(params, x0s, goals, obstacle_sets=sets)
        graphed.set_graph_replay(True, 2)
        x = x0s.copy()
        for step in range(4):
            np.testing.assert_array_equal(direct.solve(), graphed.solve())
            x = x + np.float32([0.05, 0.04, 0.01])
            for planner in (direct, graphed):
                planner.shift_and_update_on_device(x, num_shifts=1)
        assert ("tracks=%d" % (t + 1) in graphed.last_rollout_kernel()) == (kind == "tracks")
        if kind == "tracks":
            np.testing.assert_array_equal(graphed.track_offset, np.full(B, 4))
        stats[kind] = graphed.graph_stats()
    assert stats["tracks"]["replays"] >= 6, stats
    assert stats["tracks"]["replays"] == stats["static"]["replays"], stats
    assert stats["tracks"]["captures"] <= stats["static"]["captures"], stats


def test_errors():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    cfg = make_cfg(128, 30)
    rng = np.random.default_rng(1)
    x0s, goals = problems(rng, 3)
    batch = MPPI_Batch(cfg, 3)
    batch.setup(make_params(cfg.dt, 1.0), x0s, goals)
    lib = _lib.load()

    def rc_of(handle, count, counts, rows, tracks, rad):
        c = np.ascontiguousarray(counts, dtype=np.int32)
        t_ = np.ascontiguousarray(tracks, dtype=np.float32).reshape(-1, 2)
        r_ = np.ascontiguousarray(rad, dtype=np.float32).reshape(-1)
        rc = lib.mppi_planner_set_disc_tracks(handle, count, _lib.ptr(c, C.c_int), rows, _lib.ptr(t_, C.c_float),
                                              _lib.ptr(r_, C.c_float))
        return rc, lib.mppi_last_error().decode()

    rc, msg = rc_of(batch._handle, 2, [1, 1], 4, np.zeros((2, 4, 2)), np.ones(2))
    assert rc == ERR_INVALID and "num_instances" in msg, msg
    rc, msg = rc_of(batch._handle, 3, [1, -1, 1], 4, np.zeros((1, 4, 2)), np.ones(1))
    assert rc == ERR_INVALID and "negative" in msg, msg
    rc, msg = rc_of(batch._handle, 3, [1, 1, 1], 0, np.zeros((3, 1, 2)), np.ones(3))
    assert rc == ERR_INVALID and "row" in msg, msg
    off = np.array([0, -1, 0], dtype=np.int32)
    assert lib.mppi_planner_set_track_offsets(batch._handle, 3, _lib.ptr(off, C.c_int)) == ERR_INVALID
    assert lib.mppi_planner_set_track_offsets(batch._handle, 2, _lib.ptr(off, C.c_int)) == ERR_INVALID
    big = 140  # 16 * 30 + 16 * 30 * 140 > 64 KiB
    rc, msg = rc_of(batch._handle, 3, [1, big, 0], 2, np.zeros((big + 1, 2, 2)), np.ones(big + 1))
    assert rc == ERR_INVALID and "LDS" in msg, msg
    assert np.isfinite(batch.solve()).all() and "tracks" not in batch.last_rollout_kernel()  # the handle is unharmed
    # ... through the Python layer, with tracks already set: they stay
    pos, rad = random_discs(rng, 2, x0s[0], goals[0])
    good = track_params(make_params(cfg.dt, 1.0), np.repeat(pos[:, None], 5, 1), rad)
    single = MPPI_Numba(cfg)
    single.setup(good)
    u_good = single.solve()
    assert "tracks=5" in single.last_rollout_kernel()
    single.set_params(track_params(good, np.zeros((big, 3, 2)), np.ones(big)))
    with pytest.raises(_lib.MppiError) as err:
        single.solve()
    assert err.value.code == ERR_INVALID and "LDS" in str(err.value)
    single.set_params(good)
    assert np.isfinite(single.solve()).all() and "tracks=5" in single.last_rollout_kernel() and u_good.shape == (30, 2)
    # the largest set that fits runs (the size checked is the size launched): 16 * 30 * (1 + 135) = 65280 bytes
    fits = 135
    single.set_params(track_params(good, np.full((fits, 3, 2), 50.0), np.ones(fits)))
    assert np.isfinite(single.solve()).all() and "discs=loop tracks=3" in single.last_rollout_kernel()
    # shapes the Python layer refuses
    for bad in (track_params(good, np.zeros((2, 0, 2)), rad),      # L = 0
                track_params(good, np.zeros((3, 4, 2)), rad),      # three tracks, two radii
                track_params(good, np.zeros((2, 4)), rad)):        # not (K, L, 2)
        single.set_params(bad)
        with pytest.raises(ValueError):
            single.solve()
    both = dict(good)
    both["obstacle_positions"] = pos
    single.set_params(both)
    with pytest.raises(ValueError, match="both"):
        single.solve()
    with pytest.raises(ValueError, match="mix"):
        batch.set_obstacle_sets([(np.zeros((1, 4, 2)), np.ones(1)), (np.zeros((1, 2)), np.ones(1)), (np.zeros((0, 4, 2)), np.ones(0))])
    with pytest.raises(ValueError, match="rows"):
        batch.set_obstacle_sets([(np.zeros((1, 4, 2)), np.ones(1)), (np.zeros((1, 5, 2)), np.ones(1)), (np.zeros((0, 4, 2)), np.ones(0))])
    assert np.isfinite(batch.solve()).all()
    # tracks in a map mode
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    planner = MapPlanner(mcfg)
    planner.setup(mparams, lin, ang)
    rc, msg = rc_of(planner._handle, 1, [1], 4, np.zeros((1, 4, 2)), np.ones(1))
    assert rc == ERR_INVALID and "barebone" in msg, msg
    zero = np.zeros(1, dtype=np.int32)
    assert lib.mppi_planner_set_track_offsets(planner._handle, 1, _lib.ptr(zero, C.c_int)) == ERR_INVALID
    assert lib.mppi_planner_get_track_offsets(planner._handle, 1, _lib.ptr(zero, C.c_int)) == ERR_INVALID


def _clearance(xhist, steps, track, radius):
    """True clearance |x_robot(i) - c(i)| - r at every control step i the loop has run."""
    centres = track[0, :steps + 1].astype(np.float64)
    return np.linalg.norm(xhist[:steps + 1, :2] - centres, axis=1) - radius


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_disc_that_crosses_the_path(seed):
    """One scenario: the robot drives from (0, 0) along y = 0 to (6, 0); a disc of radius 1.5 m starts at (3, -4) and
    crosses that line at 1.5 m/s.  Planner A is given the disc's true track and runs closed_loop; planner B runs the
    notebook's host loop and is given, before every solve, the disc standing at its present place.  A never enters the
    disc, B does (on the MI355X, seeds 1 / 2 / 3: smallest clearance of A 0.008 / 0.068 / 0.008 m, of B -0.19 / -0.17 /
    -0.36 m; A takes 44 control steps, B 30 - 32)."""
    from mppi_numba_amd.barebone import Config, MPPI_Numba, constant_velocity_tracks
    T, dt, max_steps, radius = 50, 0.1, 70, 1.5

    def cfg():
        return Config(T=(T + 0.5) * dt, dt=dt, num_control_rollouts=1024, num_vis_state_rollouts=4, seed=seed,
                      enforce_recommended_limits=False)

    base = dict(dt=dt, x0=np.array([0.0, 0.0, 0.0]), xgoal=np.array([6.0, 0.0]), goal_tolerance=0.3, dist_weight=10,
                lambda_weight=1.0, num_opt=2, u_std=np.array([1.0, 1.0]), vrange=np.array([0.0, 2.0]),
                wrange=np.array([-np.pi, np.pi]), obs_penalty=1e6)
    track = constant_velocity_tracks([[3.0, -4.0]], [[0.0, 1.5]], dt, max_steps + T + 1)
    a = MPPI_Numba(cfg())
    a.setup(dict(base, obstacle_tracks=track, obstacle_radius=np.array([radius])))
    xa, _, steps_a = a.closed_loop(max_steps)
    assert "tracks=%d" % track.shape[1] in a.last_rollout_kernel() and a.track_offset == steps_a
    b = MPPI_Numba(cfg())
    b.setup(dict(base, obstacle_positions=track[:, 0], obstacle_radius=np.array([radius])))
    xb = np.full((max_steps + 1, 3), np.nan)
    xb[0] = base["x0"]
    steps_b = max_steps
    for t in range(max_steps):
        b.params["obstacle_positions"] = track[:, t]  # where the disc is now, as if it stood there
        useq = b.solve()
        u = useq[0].astype(np.float64)
        xb[t + 1] = xb[t] + dt * np.array([np.cos(xb[t, 2]) * u[0], np.sin(xb[t, 2]) * u[0], u[1]])
        b.shift_and_update(xb[t + 1], useq, num_shifts=1)
        if np.linalg.norm(xb[t + 1, :2] - base["xgoal"]) <= base["goal_tolerance"]:
            steps_b = t + 1
            break
    assert "tracks" not in b.last_rollout_kernel()
    clear_a, clear_b = _clearance(xa, steps_a, track, radius), _clearance(xb, steps_b, track, radius)
    print("seed %d: A %d steps, smallest clearance %.4f m; B %d steps, smallest clearance %.4f m"
          % (seed, steps_a, clear_a.min(), steps_b, clear_b.min()))
    assert steps_a < max_steps and steps_b < max_steps, "both reach the goal"
    assert clear_a.min() >= 0.0, "the planner that knows the track entered the disc"
    assert clear_b.min() < 0.0, "the planner that takes the disc to stand still did not enter it: the scenario shows nothing"
