"""Disc samples of the barebone planner (params['obstacle_track_samples'], crowd mode): S sampled futures of the moving
discs, the rollout's cost the CVaR tail over its S costs.  Every comparison is bit for bit: the per-sample costs with the
plain crowd launch given one sample as its tracks (both math modes), the costs with tests/disc_samples_model.py (exact math).

Shapes, unless a test says otherwise: n = 200 (the last tile is partial), T = 37 (more than one chunk, no multiple of the
waves: asserted from the launch's description)."""
import functools
import gc

import numpy as np
import pytest

import disc_samples_model as M
import fleet_model
from crowd_model import crowd_discs
from test_gpu_barebone_batch import (ERR_INVALID, assert_bits, check_update_vs_oracle, make_params, oracle_params, problem_params,
                                     problems)
from test_gpu_barebone_crowd import cfg_of, inputs, shape_of
from test_gpu_barebone_fleet import ROOM, ROOM_HW, fleet_ending, ring
from test_gpu_barebone_goal_tracks import crossing_goal, goal_params
from test_gpu_barebone_tracks import moving_tracks, rollout_with, track_params
from test_gpu_barebone_wall_tracks import moving_building, track_wall_params
from test_gpu_barebone_walls import N, building, task, wall_params, without_walls

pytestmark = pytest.mark.gpu

T = 37
DT = 0.1


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


@functools.lru_cache(maxsize=None)
def sample_set(K, S, rows=T + 1, x0=(0.0, 0.0, np.pi / 4), goal=(2.2, 2.2)):
    """(S, K, rows, 2) samples and (K,) radii: moving_tracks of crowd_discs, and per sample an offset per disc of about half
    a metre -- as large as the discs -- so that the samples disagree."""
    rng = np.random.default_rng(1000 * K + S)
    pos, rad = crowd_discs(rng, K, np.array(x0), np.array(goal))
    tracks = moving_tracks(rng, pos, DT, rows)
    off = rng.normal(0, 0.5, (S, K, 1, 2))
    smp = (tracks[None].astype(np.float64) + off).astype(np.float32)
    smp.setflags(write=False)
    rad.setflags(write=False)
    return smp, rad


def sample_params(params, smp, rad, alpha=None):
    p = {k: v for k, v in params.items() if k not in ("obstacle_positions", "obstacle_tracks")}
    p["obstacle_track_samples"], p["obstacle_radius"] = smp, rad
    if alpha is not None:
        p["cvar_alpha"] = alpha
    return p


def the_samples_discriminate(per, alpha=None):
    """Asserted before anything is compared.  per: (n, S) per-sample costs.  (numel == S: the sorted and the unsorted tree
    add the same S values, which for S = 2 cannot differ; the third statement is made where numel < S.)"""
    S = per.shape[1]
    if S > 1:
        assert (np.ptp(per, axis=1) > 0).any(), "bad input: every rollout costs the same under every sample"
        assert (np.diff(per, axis=1) > 0).any(), "bad input: the descending order is the sample order for every rollout"
    if alpha is not None and alpha < 1 and M.cvar_numel(S, alpha) < S:
        assert (M.cvar_tail(per, alpha) != M.cvar_tail(per, 1.0)).any(), "bad input: the CVaR is the mean for every rollout"


def check_shape(kernel, S, alpha, rows):
    W, chunk = shape_of(kernel)
    assert T > chunk, "the horizon must span more than one chunk (%s)" % kernel
    assert T % W != 0, "the horizon must not be a multiple of the waves (%s)" % kernel
    assert " tracks=%d" % rows in kernel, kernel
    assert kernel.endswith(" samples=%d numel=%d" % (S, M.cvar_numel(S, alpha))), kernel


def sampled_rollout(planner, u_in, noise):
    planner.record_sample_costs()
    costs, u, w, kernel = rollout_with(planner, u_in, noise)
    return costs, planner.sample_costs(), u, kernel


# ---- 1. per-sample costs against the plain crowd launch ----------------------------------------------------------------
@pytest.mark.parametrize("K,S,math,wscale", [(K, S, math, wscale) for K in (5, 70) for S in (1, 3, 16) for math in ("exact", "fast")
                                             for wscale in (1.0, 1.5)])
def test_per_sample_costs_equal_the_plain_launch(K, S, math, wscale):
    """sample_costs()[:, s] is what a second handle gives with obstacle_tracks = samples[s] -- for fast math the only
    statement made.  S = 1: the costs themselves are the plain launch's, at any alpha."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(T, wscale)
    smp, rad = sample_set(K, S)
    planner, plain = MPPI_Numba(cfg_of(N, T, True, math)), MPPI_Numba(cfg_of(N, T, True, math))
    planner.set_params(sample_params(params, smp, rad, 0.5))
    costs, per, _, kernel = sampled_rollout(planner, u_in, noise)
    check_shape(kernel, S, 0.5, T + 1)
    assert ("rotation=1" in kernel) == (math == "exact" and wscale == 1.0) and ("exact=1" in kernel) == (math == "exact"), kernel
    assert per.shape == (N, S)
    want = []
    for s in range(S):
        plain.set_params(track_params(params, smp[s], rad))
        got, _, _, plain_kernel = rollout_with(plain, u_in, noise)
        assert plain_kernel.startswith("k_rollout_barebone_crowd") and "samples" not in plain_kernel, plain_kernel
        want.append(got)
    want = np.stack(want, axis=1)
    assert (want > 1e6).any(), "bad input: no rollout is inside a disc"
    the_samples_discriminate(want, 0.5)
    assert_bits(per, want, "%d discs, %d samples, %s math: per-sample costs vs the plain launch" % (K, S, math))
    assert_bits(costs, M.cvar_tail(want, 0.5), "the tail over the plain launch's costs")
    if S == 1:
        assert_bits(costs, want[:, 0], "one sample is the plain track set")


# ---- 2. costs against the model ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_per_sample(K, S, offset=0, rows=T + 1, wscale=1.0):
    params, u_in, noise = task(T, wscale)
    smp, rad = sample_set(K, S, rows)
    per = M.sample_costs(oracle_params(params), smp, rad, noise, u_in, offset=offset)
    per.setflags(write=False)
    return per


ALPHAS = (1.0, 0.99, 0.5, 0.34, 1 / 16, 1e-3)


@pytest.mark.parametrize("S,alpha", [(S, alpha) for S in (2, 3, 5, 16) for alpha in ALPHAS])
def test_costs_equal_the_model(S, alpha):
    """numel 1 (alpha <= 1 / S), odd (S = 5 at 0.5: 3; S = 3 at 0.99), equal to S with a sort (0.99) and without (1.0)."""
    from mppi_numba_amd.barebone import MPPI_Numba
    K = 70
    params, u_in, noise = task(T, 1.0)
    smp, rad = sample_set(K, S)
    per = model_per_sample(K, S)
    the_samples_discriminate(per, alpha)
    planner = MPPI_Numba(cfg_of(N, T, True))
    planner.set_params(sample_params(params, smp, rad, alpha))
    costs, got_per, _, kernel = sampled_rollout(planner, u_in, noise)
    check_shape(kernel, S, alpha, T + 1)
    assert_bits(got_per, per, "per-sample costs vs the model")
    assert_bits(costs, M.cvar_tail(per, alpha), "%d samples, alpha %g vs the model" % (S, alpha))


def test_numel_cases_are_covered():
    numels = {(S, a): M.cvar_numel(S, a) for S in (2, 3, 5, 16) for a in ALPHAS}
    assert 1 in numels.values() and any(v % 2 == 1 and v > 1 for v in numels.values())
    assert numels[(16, 0.99)] == 16 and numels[(16, 1.0)] == 16 and numels[(5, 0.5)] == 3


@pytest.mark.parametrize("offset,rows", [(5, T + 1), (0, 20), (5, 20)])  # an offset; a track shorter than the horizon (clamp)
def test_offset_and_clamp(offset, rows):
    from mppi_numba_amd.barebone import MPPI_Numba
    K, S, alpha = 70, 3, 0.5
    params, u_in, noise = task(T, 1.0)
    smp, rad = sample_set(K, S, rows)
    per = model_per_sample(K, S, offset, rows)
    the_samples_discriminate(per, alpha)
    assert (per != model_per_sample(K, S, 0, T + 1)).any(), "bad input: the offset / the clamp changes nothing"
    planner = MPPI_Numba(cfg_of(N, T, True))
    planner.set_params(sample_params(params, smp, rad, alpha))
    planner.move_mppi_task_vars_to_device()  # (hands the samples over: offset 0)
    assert planner.track_offset == 0
    planner.set_track_offset(offset)
    costs, got_per, _, kernel = sampled_rollout(planner, u_in, noise)
    check_shape(kernel, S, alpha, rows)
    assert_bits(got_per, per, "per-sample costs vs the model")
    assert_bits(costs, M.cvar_tail(per, alpha), "offset %d, %d rows vs the model" % (offset, rows))


# ---- 3. composition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["walls", "wall_tracks", "goal_track", "all_at_an_offset"])
def test_composition_equals_the_model(what):
    """S = 3, alpha = 0.5, 70 discs; 70 static walls (launched as wall tracks of one row), 70 wall tracks, a goal track, and
    wall tracks with a goal track at track_offset = 5."""
    from mppi_numba_amd.barebone import MPPI_Numba
    K, S, alpha, W = 70, 3, 0.5, 70
    params, u_in, noise = task(T, 1.0)
    smp, rad = sample_set(K, S)
    full, kw, offset = sample_params(params, smp, rad, alpha), {}, 0
    if what == "walls":
        seg, hw = building(W)
        full, kw = wall_params(full, seg, hw), dict(wall_segments=seg, halfwidths=hw)
    if what in ("wall_tracks", "all_at_an_offset"):
        wtracks, hw = moving_building(W, T + 6)
        full, kw = track_wall_params(full, wtracks, hw), dict(wall_tracks=wtracks, halfwidths=hw)
    plain = oracle_params(without_walls(params))
    if what in ("goal_track", "all_at_an_offset"):
        goal = crossing_goal(T, T + 4)
        full, kw["goal_track"] = goal_params(full, goal), goal
        plain = oracle_params(dict(without_walls(params), xgoal=goal[0]))
    if what == "all_at_an_offset":
        offset = 5
    per = M.sample_costs(plain, smp, rad, noise, u_in, offset=offset, **kw)
    bare = M.sample_costs(oracle_params(without_walls(params)), smp, rad, noise, u_in, offset=offset)
    the_samples_discriminate(per, alpha)
    assert (per != bare).any(), "bad input: the walls / the goal track change nothing"
    planner = MPPI_Numba(cfg_of(N, T, True))
    planner.set_params(full)
    planner.move_mppi_task_vars_to_device()
    planner.set_track_offset(offset)
    costs, got_per, _, kernel = sampled_rollout(planner, u_in, noise)
    W_, chunk = shape_of(kernel)
    assert T > chunk and T % W_ != 0 and kernel.endswith(" samples=3 numel=2"), kernel
    assert (" walls=%d" % W in kernel) == (what != "goal_track") and (" goal_rows=" in kernel) == ("goal_track" in kw), kernel
    assert_bits(got_per, per, "%s: per-sample costs vs the model" % what)
    assert_bits(costs, M.cvar_tail(per, alpha), "%s: costs vs the model" % what)


def test_fleet_in_a_room_past_sampled_discs():
    """B = 3 robots, n = 64 each, the room's wall_segments behind the others in every robot's set, S = 3 samples of 20 discs."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, S, alpha, Wr = 3, 64, 3, 0.5, len(ROOM)
    x0s, goals, us, noise = ring(B, n, T, 7 * B + T)
    smp, rad = sample_set(20, S, T + 1, (0.0, 0.0, 0.0), (0.3, 0.3))  # (around the centre, where the plans meet)
    params = make_params(DT, 1.0)
    radii, margin = np.linspace(0.2, 0.3, B), 0.02
    hw = fleet_model.halfwidths(radii, margin, B)
    walls = fleet_model.fleet_walls(params, x0s, us)
    batch = MPPI_Batch(cfg_of(n, T, True), B)
    batch.setup(sample_params(wall_params(params, ROOM, ROOM_HW), smp, rad, alpha), x0s, goals)
    batch.set_fleet(radii, margin)
    batch.record_sample_costs()
    costs, _, _, kernel = rollout_with(batch, us, noise.reshape(B * n, T, 2))
    got_per = batch.sample_costs()
    assert got_per.shape == (B, n, S)
    shape_of(kernel)
    assert kernel.endswith(fleet_ending(B, Wr, T) + " samples=3 numel=2") and "problems=3" in kernel, kernel
    differs = False
    for b in range(B):
        pb = oracle_params(problem_params(params, x0s[b], goals[b]))
        wt, h = fleet_model.reader_walls(walls[b], hw[b], ROOM, ROOM_HW)
        per = M.sample_costs(pb, smp, rad, noise[b], us[b], wall_tracks=wt, halfwidths=h, wall_offset=0)
        differs = differs or bool((per != M.sample_costs(pb, smp, rad, noise[b], us[b])).any())
        the_samples_discriminate(per, alpha)
        assert_bits(got_per[b], per, "robot %d: per-sample costs vs the model" % b)
        assert_bits(costs[b], M.cvar_tail(per, alpha), "robot %d: costs vs the model" % b)
    assert differs, "bad input: the fleet and the room change no robot's costs"


# ---- 4. batch ----------------------------------------------------------------------------------------------------------------
def test_batch_shares_the_sample_set():
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    B, n, S, alpha = 3, 128, 3, 0.5
    rng = np.random.default_rng(41)
    x0s, goals = problems(rng, B)
    smp, rad = sample_set(70, S, T + 1, tuple(x0s[0]), tuple(goals[0]))
    params = sample_params(make_params(DT, 1.0), smp, rad, alpha)
    u_in = np.stack([inputs(rng, n, T)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, T, 2)).astype(np.float32)
    batch = MPPI_Batch(cfg_of(n, T, True), B)
    batch.setup(params, x0s, goals)
    batch.record_sample_costs()  # (hands the samples over: offset 0)
    batch.set_track_offset(np.array([0, 2, 7], dtype=np.int32))
    costs, u_out, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, T, 2))
    per = batch.sample_costs()
    np.testing.assert_array_equal(batch.track_offset, [0, 2, 7])
    shape_of(kernel)
    assert "problems=3" in kernel and kernel.endswith(" samples=3 numel=2"), kernel
    single = MPPI_Numba(cfg_of(n, T, True))
    for b, offset in enumerate((0, 2, 7)):
        single.set_params(problem_params(params, x0s[b], goals[b]))
        single.move_mppi_task_vars_to_device()
        single.set_track_offset(offset)
        want, want_per, want_u, _ = sampled_rollout(single, u_in[b], noise[b])
        if b == 0:
            the_samples_discriminate(want_per, alpha)
        assert_bits(per[b], want_per, "problem %d: per-sample costs vs a single handle" % b)
        assert_bits(costs[b], want, "problem %d: costs vs a single handle" % b)
        assert_bits(u_out[b], want_u, "problem %d: u vs a single handle" % b)


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------
def test_solve_equals_the_update_on_the_models_costs():
    """Two handles with one seed: solve() on the one; noise, rollout and update stage by stage on the other, whose noise the
    model takes."""
    from mppi_numba_amd.barebone import MPPI_Numba
    from oracle import oracle as O
    K, S, alpha = 20, 3, 0.5
    params, _, _ = task(T, 1.0)
    smp, rad = sample_set(K, S)
    full = sample_params(params, smp, rad, alpha)
    solver, staged = MPPI_Numba(cfg_of(N, T, True, seed=9)), MPPI_Numba(cfg_of(N, T, True, seed=9))
    solver.setup(full)
    staged.setup(full)
    useq = solver.solve()
    assert solver.last_rollout_kernel().endswith(" samples=3 numel=2")
    staged.sample_noise()
    noise, u_in = staged.noise_samples_d.copy_to_host(), staged.u_cur_d.copy_to_host()
    per = M.sample_costs(oracle_params(params), smp, rad, noise, u_in)
    the_samples_discriminate(per, alpha)
    model = M.cvar_tail(per, alpha)
    staged.rollout()
    assert_bits(staged.costs_d.copy_to_host(), model, "the staged rollout vs the model")
    staged.update()
    check_update_vs_oracle(params, model, noise, u_in, staged.u_cur_d.copy_to_host())
    check_update_vs_oracle(params, model, noise, u_in, useq)


def _euler(x, u0, dt):
    """barebone_mppi_numba.ipynb cell 7 in float64 (see test_gpu_barebone_batch._notebook_loop)."""
    u = u0.astype(np.float64)
    return np.array([x[0] + dt * np.cos(x[2]) * u[0], x[1] + dt * np.sin(x[2]) * u[0], x[2] + dt * u[1]])


def test_closed_loop_equals_the_host_loop():
    from mppi_numba_amd.barebone import MPPI_Numba
    n, steps, S, alpha = 256, 6, 3, 0.5
    params = make_params(DT, 1.0)  # (the goal is out of reach of six steps)
    smp, rad = sample_set(20, S, T + 7, tuple(params["x0"]), tuple(params["xgoal"]))
    full = sample_params(params, smp, rad, alpha)
    host, dev = (MPPI_Numba(cfg_of(n, T, True, seed=5)) for _ in range(2))
    for planner in (host, dev):
        planner.setup(full)
    x = np.asarray(params["x0"], np.float64)
    want_x, want_u = np.full((steps + 1, 3), np.nan), np.full((steps, 2), np.nan, np.float32)
    want_x[0] = x
    for step in range(steps):
        useq = host.solve()
        want_u[step] = useq[0]
        x = _euler(x, useq[0], DT)
        want_x[step + 1] = x
        host.shift_and_update(x, useq, num_shifts=1)
        assert host.track_offset == step + 1
    assert host.last_rollout_kernel().endswith(" samples=3 numel=2")
    got_x, got_u, got_steps = dev.closed_loop(steps)
    assert got_steps == steps and dev.track_offset == steps
    np.testing.assert_array_equal(got_u.view(np.int32), want_u.view(np.int32))
    np.testing.assert_array_equal(got_x.view(np.int64), want_x.view(np.int64))


# ---- 6. graph replay -----------------------------------------------------------------------------------------------------------
def test_graph_replay_and_a_changed_sample_set():
    from mppi_numba_amd.barebone import MPPI_Numba
    K, S, alpha = 20, 3, 0.5
    params, _, _ = task(T, 1.0)
    params = dict(params, num_opt=4)
    smp, rad = sample_set(K, S)
    direct, graphed = MPPI_Numba(cfg_of(N, T, True, seed=4)), MPPI_Numba(cfg_of(N, T, True, seed=4))
    for planner in (direct, graphed):
        planner.setup(sample_params(params, smp, rad, alpha))
    graphed.set_graph_replay(True, 2)
    for _ in range(2):
        np.testing.assert_array_equal(direct.solve(), graphed.solve())
    stats = graphed.graph_stats()
    assert stats["captures"] >= 1 and stats["replays"] >= 2, stats
    captures = stats["captures"]
    for planner in (direct, graphed):  # the same set, as new objects: nothing changes
        planner.params["obstacle_track_samples"], planner.params["obstacle_radius"] = smp.copy(), rad.copy()
    np.testing.assert_array_equal(direct.solve(), graphed.solve())
    assert graphed.graph_stats()["captures"] == captures, "the same samples again: no new capture"
    moved = (smp + np.float32([0.3, -0.2])).astype(np.float32)
    for planner in (direct, graphed):
        planner.params["obstacle_track_samples"] = moved
    np.testing.assert_array_equal(direct.solve(), graphed.solve())
    assert graphed.graph_stats()["captures"] == captures + 1, "a changed sample set: one more capture"
    np.testing.assert_array_equal(direct.solve(), graphed.solve())
    assert graphed.graph_stats()["captures"] == captures + 1
    assert graphed.last_rollout_kernel().endswith(" samples=3 numel=2")


# ---- 7. refusals and state -------------------------------------------------------------------------------------------------------
def test_refusals_and_state():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    K, S = 20, 3
    params, u_in, noise = task(T, 1.0)
    smp, rad = sample_set(K, S)
    full = sample_params(params, smp, rad, 0.5)
    # crowd mode off
    off = MPPI_Numba(cfg_of(N, T, False))
    off.set_params(full)
    with pytest.raises(_lib.MppiError) as err:
        off.rollout()
    assert err.value.code == ERR_INVALID and "crowd" in str(err.value), str(err.value)
    # held: crowd mode stays on
    planner = MPPI_Numba(cfg_of(N, T, True))
    planner.set_params(full)
    held_costs = rollout_with(planner, u_in, noise)[0]
    with pytest.raises(_lib.MppiError) as err:
        planner.set_crowd(False)
    assert err.value.code == ERR_INVALID and "samples" in str(err.value) and planner.crowd, str(err.value)
    # 17 samples; two disc keys at once; cvar_alpha outside (0, 1]
    bad = [sample_params(params, np.repeat(smp[:1], 17, axis=0), rad),
           dict(full, obstacle_tracks=smp[0]), dict(full, obstacle_positions=smp[0, :, 0]),
           dict(track_params(params, smp[0], rad), obstacle_positions=smp[0, :, 0]),
           dict(full, cvar_alpha=0.0), dict(full, cvar_alpha=1.5), sample_params(params, smp[0], rad)]
    for p in bad:
        fresh = MPPI_Numba(cfg_of(N, T, True))
        fresh.set_params(p)
        with pytest.raises(ValueError):
            fresh.rollout()
    # ... and the library's own refusals
    lib = _lib.load()
    flat = np.ascontiguousarray(np.repeat(smp[:1], 17, axis=0))
    import ctypes as C
    assert lib.mppi_planner_set_disc_track_samples(planner._handle, 17, K, T + 1, _lib.ptr(flat, C.c_float), _lib.ptr(rad, C.c_float)) == ERR_INVALID
    assert "17" in lib.mppi_last_error().decode()
    assert lib.mppi_planner_set_disc_track_samples(planner._handle, 3, K, 0, _lib.ptr(flat, C.c_float), _lib.ptr(rad, C.c_float)) == ERR_INVALID
    neg = np.ascontiguousarray(-np.asarray(rad))
    assert lib.mppi_planner_set_disc_track_samples(planner._handle, 3, K, T + 1, _lib.ptr(flat, C.c_float), _lib.ptr(neg, C.c_float)) == ERR_INVALID
    assert "radius" in lib.mppi_last_error().decode()
    counts = np.array([K], dtype=np.int32)
    one = np.ascontiguousarray(smp[0])
    assert lib.mppi_planner_set_disc_tracks(planner._handle, 1, _lib.ptr(counts, C.c_int), T + 1, _lib.ptr(one, C.c_float),
                                            _lib.ptr(rad, C.c_float)) == ERR_INVALID
    assert "samples" in lib.mppi_last_error().decode()
    assert_bits(rollout_with(planner, u_in, noise)[0], held_costs, "the refusals left the handle as it was")
    # a batch: per-problem sets and samples exclude each other, both ways
    B, n = 2, 64
    rng = np.random.default_rng(3)
    x0s, goals = problems(rng, B)
    sets = [crowd_discs(rng, 6, x0s[b], goals[b]) for b in range(B)]
    batch = MPPI_Batch(cfg_of(n, T, True), B)
    batch.setup(full, x0s, goals)
    batch.rollout()
    with pytest.raises(ValueError):
        batch.set_obstacle_sets(sets)
    own = np.array([6, 6], dtype=np.int32)
    pos = np.ascontiguousarray(np.concatenate([s[0] for s in sets]))
    rr = np.ascontiguousarray(np.concatenate([s[1] for s in sets]))
    assert lib.mppi_planner_set_instance_disc_obstacles(batch._handle, B, _lib.ptr(own, C.c_int), _lib.ptr(pos, C.c_float),
                                                        _lib.ptr(rr, C.c_float)) == ERR_INVALID
    assert "samples" in lib.mppi_last_error().decode()
    other = MPPI_Batch(cfg_of(n, T, True), B)
    other.setup(without_samples(full), x0s, goals, obstacle_sets=sets)
    other.rollout()
    other.set_params(dict(full, x0=other.params["x0"], xgoal=other.params["xgoal"]))
    with pytest.raises(ValueError):
        other.rollout()
    assert lib.mppi_planner_set_disc_track_samples(other._handle, 3, K, T + 1, _lib.ptr(np.ascontiguousarray(smp), C.c_float),
                                                   _lib.ptr(rad, C.c_float)) == ERR_INVALID
    assert "per-problem" in lib.mppi_last_error().decode()


def without_samples(params):
    return {k: v for k, v in params.items() if k not in ("obstacle_track_samples", "obstacle_radius", "cvar_alpha")}


def test_dropping_the_key_restores_the_static_discs():
    from mppi_numba_amd.barebone import MPPI_Numba
    K, S = 20, 3
    params, u_in, noise = task(T, 1.0)
    smp, rad = sample_set(K, S)
    static = dict(params, obstacle_positions=np.ascontiguousarray(smp[1, :, 3]), obstacle_radius=rad)
    planner = MPPI_Numba(cfg_of(N, T, True))
    planner.set_params(static)
    before, _, _, kernel = rollout_with(planner, u_in, noise)
    assert (before > 1e6).any() and "samples" not in kernel
    planner.set_params(sample_params(params, smp, rad, 0.5))
    planner.move_mppi_task_vars_to_device()
    planner.set_track_offset(4)
    sampled, _, _, kernel = rollout_with(planner, u_in, noise)
    assert kernel.endswith(" samples=3 numel=2") and (sampled != before).any()
    planner.shift_and_update(np.asarray(params["x0"]), u_in)  # (samples count as tracks: "now" advances)
    assert planner.track_offset == 5
    planner.set_params(static)
    after, _, _, kernel = rollout_with(planner, u_in, noise)
    assert "samples" not in kernel and planner.track_offset == 0
    assert_bits(after, before, "the static discs again")
    with pytest.raises(ValueError):
        planner.sample_costs()


@pytest.mark.parametrize("crowd,K", [(True, 20), (False, 3)])
def test_cvar_alpha_alone_changes_nothing(crowd, K):
    """Without a sample set nothing reads cvar_alpha: a plain crowd launch and a default-family launch keep their bits."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(T, 1.0)
    smp, rad = sample_set(K, 1)
    tparams = track_params(params, smp[0], rad)
    planner = MPPI_Numba(cfg_of(N, T, crowd))
    planner.set_params(tparams)
    want, want_u, want_w, kernel = rollout_with(planner, u_in, noise)
    assert kernel.startswith("k_rollout_barebone_crowd") == crowd, kernel
    planner.set_params(dict(tparams, cvar_alpha=0.3))
    got, got_u, got_w, again = rollout_with(planner, u_in, noise)
    assert again == kernel
    assert_bits(got, want, "costs")
    assert_bits(got_u, want_u, "u")
    assert_bits(got_w, want_w, "weights")
