"""Crowd mode of the barebone planner (Config(crowd=True) / set_crowd): disc sets that do not fit the 64 KiB of LDS of the
default forms, and k_rollout_barebone_crowd, which counts every step's hits in parallel and then adds obs_cost once per
hit.  The mode changes no result: every comparison here is bit for bit -- with the C oracle (static discs), with the numpy
models (tests/track_model.py, one addition per disc; tests/crowd_model.py, the kernel's own order; equal to each other by
tests/test_crowd_model.py) and with the default forms on the same inputs where those run."""
import ctypes as C
import re

import numpy as np
import pytest

from crowd_model import crowd_costs, crowd_discs, hit_counts
from oracle import oracle as O
from test_gpu_barebone_batch import (ERR_INVALID, assert_bits, make_cfg, make_params, oracle_params, problem_params, problems,
                                     random_discs)
from test_gpu_barebone_tracks import moving_tracks, rollout_with, track_params
from track_model import reached_goal, track_costs

pytestmark = pytest.mark.gpu

OBS_PENALTY = 1e6  # make_params


def cfg_of(n, t, crowd, math="exact", seed=3):
    cfg = make_cfg(n, t, seed=seed)
    cfg.math, cfg.crowd = math, crowd
    return cfg


def shape_of(kernel):
    """(W, C) of a crowd launch, from its description."""
    found = re.search(r"^k_rollout_barebone_crowd exact=[01] rotation=[01] waves=(\d+) chunk=(\d+)", kernel)
    assert found, kernel
    return int(found.group(1)), int(found.group(2))


def inputs(rng, n, t):
    u = np.stack([rng.uniform(0.8, 1.8, t), rng.uniform(-0.2, 0.2, t)], 1).astype(np.float32)
    return u, rng.normal(0, 0.5, (n, t, 2)).astype(np.float32)


@pytest.mark.parametrize("K", [5, 64, 65, 300, 4100])
def test_static_discs_equal_the_oracle(K):
    """n = 200: the last tile is partial.  4100 discs are what test_gpu_barebone_oracle names as too many for the LDS."""
    from mppi_numba_amd.barebone import MPPI_Numba
    n, t = 200, 30
    rng = np.random.default_rng(K)
    params = make_params(0.1, 1.0)
    near = min(K, 300)
    pos, rad = crowd_discs(rng, near, params["x0"], params["xgoal"])
    if K > near:  # most of them far away, a handful (above) on the path
        pos = np.concatenate([pos, rng.uniform(50, 90, (K - near, 2)).astype(np.float32)])
        rad = np.concatenate([rad, rng.uniform(0.2, 0.8, K - near).astype(np.float32)])
        order = rng.permutation(K)
        pos, rad = np.ascontiguousarray(pos[order]), np.ascontiguousarray(rad[order])
    params["obstacle_positions"], params["obstacle_radius"] = pos, rad
    u_in, noise = inputs(rng, n, t)
    planner = MPPI_Numba(cfg_of(n, t, True))
    assert planner.crowd
    planner.set_params(params)
    got, _, _, kernel = rollout_with(planner, u_in, noise)
    W, chunk = shape_of(kernel)
    assert "rotation=1" in kernel and "exact=1" in kernel and "tracks" not in kernel and "problems" not in kernel, kernel
    assert W >= 3 and 1 <= chunk <= 16
    want = O.rollout_barebone(oracle_params(params), pos, rad, noise, u_in)
    assert (want > OBS_PENALTY).any() and (want > 2 * OBS_PENALTY).any(), "bad input: no rollout is inside two discs"
    assert_bits(got, want, "%d static discs vs the oracle" % K)


def on_off_cases():
    for math in ("exact", "fast"):
        for K in (5, 64):
            for kind in ("static", "tracks"):
                for t in (30, 37, 100):
                    if kind == "tracks" and 16 * t * (1 + K) > 64 * 1024:
                        continue  # (64 tracks at 100 steps: crowd off cannot launch them -- test_tracks_beyond_the_limit)
                    for wscale in (1.0, 1.5):
                        yield math, K, kind, t, wscale


@pytest.mark.parametrize("math,K,kind,t,wscale", list(on_off_cases()))
def test_crowd_on_equals_crowd_off(math, K, kind, t, wscale):
    """The same operations on the same operands -- for fast math the only statement made."""
    from mppi_numba_amd.barebone import MPPI_Numba
    n = 128
    rng = np.random.default_rng(1000 * t + K)
    params = make_params(0.1, wscale)
    pos, rad = crowd_discs(rng, K, params["x0"], params["xgoal"])
    if kind == "tracks":
        params = track_params(params, moving_tracks(rng, pos, 0.1, t + 1), rad)
    else:
        params["obstacle_positions"], params["obstacle_radius"] = pos, rad
    u_in, noise = inputs(rng, n, t)
    results = {}
    for crowd in (False, True):
        planner = MPPI_Numba(cfg_of(n, t, crowd, math))
        planner.set_params(params)
        results[crowd] = rollout_with(planner, u_in, noise)
    kernel_off, kernel_on = results[False][3], results[True][3]
    # (the default loop form: the single static launch names no disc form, the others say "discs=loop")
    assert kernel_off.startswith("k_rollout_barebone exact") and "discs<=" not in kernel_off, kernel_off
    assert ("discs=loop" in kernel_off) == (kind == "tracks"), kernel_off
    W, chunk = shape_of(kernel_on)
    assert t > chunk, "the horizon must span more than one chunk (%s)" % kernel_on
    assert t % W != 0, "the horizon must not be a multiple of the waves (%s)" % kernel_on
    rotation = math == "exact" and wscale == 1.0
    assert ("rotation=1" in kernel_on) == rotation and ("exact=1" in kernel_on) == (math == "exact"), kernel_on
    assert ("tracks=%d" % (t + 1) in kernel_on) == (kind == "tracks"), kernel_on
    assert (results[False][0] > OBS_PENALTY).any(), "bad input: no rollout is inside a disc"
    for i, what in enumerate(("costs", "u after update()", "weights")):
        assert_bits(results[True][i], results[False][i], "%s, crowd on vs off" % what)


@pytest.mark.parametrize("n,t,K", [(128, 50, 100), (64, 100, 64)])
def test_tracks_beyond_the_limit(n, t, K):
    """100 pedestrians at T = 50 and a 64-robot fleet's worth of tracks at T = 100: neither fits the default forms."""
    from mppi_numba_amd.barebone import MPPI_Numba, constant_velocity_tracks
    assert 16 * t * (1 + K) > 64 * 1024
    rng = np.random.default_rng(n + t + K)
    params = make_params(0.1, 1.0)
    params["xgoal"] = np.array([2.2, 2.2])  # within reach of the horizon
    pos, rad = crowd_discs(rng, K, params["x0"], params["xgoal"])
    L = t + 1
    tracks = constant_velocity_tracks(pos, rng.normal(0, 0.3, (K, 2)), 0.1, L)
    tparams = track_params(params, tracks, rad)
    u_in, noise = inputs(rng, n, t)
    p = oracle_params(tparams)
    # the input must mean something (checked with the model, before anything is compared)
    counts, _ = hit_counts(p, tracks, rad, noise, u_in)
    model = crowd_costs(p, tracks, rad, noise, u_in)
    early = reached_goal(p, noise[:, :t - 1], u_in[:t - 1])
    assert (counts >= 2).any(), "bad input: no (rollout, step) pair is inside two discs"
    assert (model > OBS_PENALTY).any(), "bad input: no rollout costs more than obs_penalty"
    assert early.mean() >= 0.10, "bad input: only %.1f %% of the rollouts reach the goal early" % (100 * early.mean())
    planner = MPPI_Numba(cfg_of(n, t, True))
    planner.set_params(tparams)
    for offset in (0, 13, L + 5):
        planner.move_mppi_task_vars_to_device()  # (hands the tracks over the first time: offset 0)
        planner.set_track_offset(offset)
        got, _, _, kernel = rollout_with(planner, u_in, noise)
        shape_of(kernel)
        assert "tracks=%d" % L in kernel and "rotation=1" in kernel, kernel
        assert_bits(got, crowd_costs(p, tracks, rad, noise, u_in, offset=offset), "offset %d vs the crowd model" % offset)
        assert_bits(got, track_costs(p, tracks, rad, noise, u_in, offset=offset), "offset %d vs the track model" % offset)
    last = O.rollout_barebone(p, tracks[:, -1], rad, noise, u_in)
    assert_bits(got, last, "an offset past the end: static discs at the last row (oracle)")


@pytest.mark.parametrize("kind", ["static", "tracks"])
def test_batch_with_per_problem_sets(kind):
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    counts = [0, 3, 90, 200, 1]
    B, n, t, L = len(counts), 64, 30, 31
    rng = np.random.default_rng(7 + (kind == "tracks"))
    x0s, goals = problems(rng, B)
    params = make_params(0.1, 1.0)
    static_sets = [crowd_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate(counts)]
    track_sets = [(moving_tracks(rng, pos, 0.1, L), rad) for pos, rad in static_sets]
    sets = static_sets if kind == "static" else track_sets
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(params, x0s, goals, obstacle_sets=sets)
    u_in = np.stack([inputs(rng, n, t)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    offsets = np.array([0, 3, 7, 12, 40], dtype=np.int32) if kind == "tracks" else np.zeros(B, np.int32)
    if kind == "tracks":
        batch.set_track_offset(offsets)
    costs, u_out, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    shape_of(kernel)
    assert "problems=%d" % B in kernel and ("tracks=%d" % L in kernel) == (kind == "tracks") and "rotation=1" in kernel, kernel
    assert (costs[3] > 2 * OBS_PENALTY).any(), "bad input: no rollout of the largest problem is inside two discs"
    single = MPPI_Numba(cfg_of(n, t, True))
    for b in range(B):
        if kind == "tracks":
            pb = track_params(problem_params(params, x0s[b], goals[b]), sets[b][0], sets[b][1])
        else:
            pb = problem_params(params, x0s[b], goals[b], sets[b])
        single.set_params(pb)
        single.move_mppi_task_vars_to_device()
        single.set_track_offset(int(offsets[b]))
        want, want_u, _, single_kernel = rollout_with(single, u_in[b], noise[b])
        assert single_kernel.startswith("k_rollout_barebone_crowd") == (counts[b] >= 5), single_kernel
        assert_bits(costs[b], want, "problem %d (%d discs) vs a single crowd handle" % (b, counts[b]))
        assert_bits(u_out[b], want_u, "problem %d u vs a single crowd handle" % b)
        tr = track_sets[b][0] if kind == "tracks" else np.repeat(static_sets[b][0][:, None], 1, 1)
        model = crowd_costs(oracle_params(pb), tr, sets[b][1], noise[b], u_in[b], offset=int(offsets[b]))
        assert_bits(costs[b], model, "problem %d vs the model" % b)


def test_fleet_of_64():
    """Every robot avoids the straight-line tracks of the 63 others: 63 moving discs per problem at T = 50."""
    from mppi_numba_amd.barebone import MPPI_Batch, constant_velocity_tracks
    B, n, t = 64, 64, 50
    L = t + 1
    rng = np.random.default_rng(64)
    angle = np.arange(B) * (2 * np.pi / B)
    ring = 3.0 * np.stack([np.cos(angle), np.sin(angle)], 1)
    x0s = np.concatenate([ring, (angle + np.pi)[:, None]], 1).astype(np.float32)  # facing the centre
    goals = (-ring).astype(np.float32)                                             # ... and bound for the far side
    robot_tracks = constant_velocity_tracks(ring, -ring / 3.0, 0.1, L)             # 2 m/s... towards the goal: 1 m/s per 3 m
    sets = [(np.ascontiguousarray(np.delete(robot_tracks, b, axis=0)), np.full(B - 1, 0.35, np.float32)) for b in range(B)]
    params = make_params(0.1, 1.0)
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(params, x0s, goals, obstacle_sets=sets)
    u_in = np.stack([inputs(rng, n, t)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    costs, _, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    shape_of(kernel)
    assert "problems=64" in kernel and "tracks=%d" % L in kernel, kernel
    assert (costs > 2 * OBS_PENALTY).any(), "bad input: no robot's rollout is inside two others at once"
    for b in range(B):
        pb = oracle_params(problem_params(params, x0s[b], goals[b]))
        assert_bits(costs[b], crowd_costs(pb, sets[b][0], sets[b][1], noise[b], u_in[b]), "robot %d vs the model" % b)


def loop_sets(rng, x0s, goals, rows):
    return [(moving_tracks(rng, pos, 0.1, rows), rad) for pos, rad in (crowd_discs(rng, 7, x0s[b], goals[b]) for b in range(len(x0s)))]


def test_solve_is_the_same_with_crowd_on_and_off():
    from mppi_numba_amd.barebone import MPPI_Numba
    n, t = 1024, 50
    rng = np.random.default_rng(5)
    params = make_params(0.1, 1.0, num_opt=2)
    pos, rad = crowd_discs(rng, 7, params["x0"], params["xgoal"])
    tparams = track_params(params, moving_tracks(rng, pos, 0.1, t + 1), rad)
    got = {}
    for crowd in (False, True):
        planner = MPPI_Numba(cfg_of(n, t, crowd, seed=11))
        planner.setup(tparams)
        got[crowd] = planner.solve()
        assert planner.last_rollout_kernel().startswith("k_rollout_barebone_crowd") == crowd
        assert planner.get_state_rollout().shape == (4, t + 1, 3)
    np.testing.assert_array_equal(got[True], got[False])


def test_closed_loop_of_a_batch_is_the_same_with_crowd_on_and_off():
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t = 3, 64, 30
    rng = np.random.default_rng(31)
    x0s, goals = problems(rng, B)
    sets = loop_sets(rng, x0s, goals, 36)
    got = {}
    for crowd in (False, True):
        batch = MPPI_Batch(cfg_of(n, t, crowd, seed=2), B)
        batch.setup(make_params(0.1, 1.0), x0s, goals, obstacle_sets=sets)
        batch.set_track_offset(np.array([2, 0, 5], dtype=np.int32))
        xhist, uhist, steps = batch.closed_loop(10)
        assert batch.last_rollout_kernel().startswith("k_rollout_barebone_crowd") == crowd
        got[crowd] = (xhist, uhist, steps, batch.track_offset)
    for a, b in zip(got[True], got[False]):
        np.testing.assert_array_equal(a, b)
    assert (got[True][3] == np.array([2, 0, 5]) + got[True][2]).all()


def test_graph_replay_equals_the_direct_loop():
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t = 4, 128, 30
    rng = np.random.default_rng(9)
    x0s, goals = problems(rng, B)
    sets = loop_sets(rng, x0s, goals, t + 1)
    params = make_params(0.1, 1.0, num_opt=5)
    direct, graphed = MPPI_Batch(cfg_of(n, t, True), B), MPPI_Batch(cfg_of(n, t, True), B)
    for planner in (direct, graphed):
        planner.setup(params, x0s, goals, obstacle_sets=sets)
    graphed.set_graph_replay(True, 2)
    x = x0s.copy()
    for step in range(4):
        np.testing.assert_array_equal(direct.solve(), graphed.solve())
        x = x + np.float32([0.05, 0.04, 0.01])
        for planner in (direct, graphed):
            planner.shift_and_update_on_device(x, num_shifts=1)
    shape_of(graphed.last_rollout_kernel())
    np.testing.assert_array_equal(graphed.track_offset, np.full(B, 4))
    assert graphed.graph_stats()["replays"] >= 6, graphed.graph_stats()


def test_mode_handling():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Numba
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    n, t, big = 128, 30, 140  # 16 * 30 + 16 * 30 * 140 > 64 KiB: the oversize set of test_gpu_barebone_tracks.test_errors
    rng = np.random.default_rng(1)
    base = make_params(0.1, 1.0)
    pos, rad = random_discs(rng, 2, base["x0"], base["xgoal"])
    good = track_params(base, np.repeat(pos[:, None], 5, 1), rad)
    oversize = track_params(base, np.zeros((big, 3, 2)), np.ones(big))
    planner = MPPI_Numba(cfg_of(n, t, False))
    assert not planner.crowd
    planner.setup(good)
    assert np.isfinite(planner.solve()).all() and "tracks=5" in planner.last_rollout_kernel()
    planner.set_params(oversize)
    with pytest.raises(_lib.MppiError) as err:  # crowd off: as before
        planner.solve()
    assert err.value.code == ERR_INVALID and "LDS" in str(err.value)
    planner.set_crowd(True)
    assert planner.crowd
    assert np.isfinite(planner.solve()).all()  # crowd on: the same set solves
    kernel = planner.last_rollout_kernel()
    shape_of(kernel)
    assert "tracks=3" in kernel, kernel
    with pytest.raises(_lib.MppiError) as err:  # ... and holds the handle in crowd mode
        planner.set_crowd(False)
    assert err.value.code == ERR_INVALID and "tracks" in str(err.value) and "LDS" in str(err.value), str(err.value)
    assert planner.crowd
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == kernel
    planner.set_params(good)  # a set the default forms can launch: crowd mode can go
    assert np.isfinite(planner.solve()).all() and "k_rollout_barebone exact" in planner.last_rollout_kernel()  # (2 discs: KD form)
    planner.set_crowd(False)
    assert not planner.crowd
    assert np.isfinite(planner.solve()).all() and "discs<=2 tracks=5" in planner.last_rollout_kernel()
    # a map mode has no crowd mode
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    lib = _lib.load()
    assert lib.mppi_planner_set_crowd(mapped._handle, 1) == ERR_INVALID
    assert "barebone" in lib.mppi_last_error().decode()
    on = C.c_int(0)
    assert lib.mppi_planner_get_crowd(mapped._handle, C.byref(on)) == ERR_INVALID
