"""The middle of k_rollout_scan_exact (rollout_scan_exact_kernel.h): heading increments -> theta walk -> B (sin / cos,
position increments) -> x | y walk, and the control-cost terms a chunk wave forms from the noise it keeps.  Written for
a change to when a chunk wave forms those terms and at which priority it runs B (profiles/HISTORY.md, "C2 rollout:
position increments ahead of the position walk"); the file passes unchanged on the kernel before that change.

The checker is the oracle throughout (oracle.rollout_det, oracle.update_useq): every cost BIT FOR BIT, u within 1e-5 of
the control range; the kernel is asserted by name (mppi_planner_describe_last_rollout).

  1  stage-level rollouts (noise and u through the C ABI): 1, 2, 3 groups of 8 steps, groups 9 - 12 present and absent,
     last groups of 1, 4 and 8 valid steps; a full tile, a ragged one, three tiles
  2  the same shapes with the noise generated in the kernel (the one-launch loop), against a staged twin over stored
     noise and against the oracle, lambda = 50: the control-cost terms are a visible share of every cost, so terms
     formed from another step's or another rollout's noise (a wrong swizzle column) show in the costs
  3  headings that move: the noise's w scaled x4 in every other group and the turn-rate limit doubled, so that B takes
     the full sin / cos evaluation (|delta theta| > 0.36) in some groups and the rotation in others within one tile
  4  three iterations of the one-launch loop against the stage-level sequence, with an update launch between the
     rollout launches (N = 70) and with the update folded into the next rollout launch (N = 200, 800)
  5  the speed-map form; a failed vote on both re-run paths with a launch whose vote holds behind it; the direct form
  6  the same launch twice: the same bits"""
import numpy as np
import pytest

from mppi_numba_amd import _lib
from oracle import oracle as O
from test_gpu_scan_tail import (a_launch_whose_vote_holds, build, cell_of, folded_iteration_vs_oracle, grids, inputs,
                                oracle_run, run_costs, same_bits, span)

pytestmark = pytest.mark.gpu
f32 = np.float32

HORIZONS = [8, 9, 16, 17, 24, 96, 100, 104]
ROLLOUTS = [32, 40, 70]


def speculative(name):
    return name.startswith("k_rollout_scan_exact") and "direct=1" not in name


def u_of_update(params, want, noise, u):
    return O.update_useq(params["lambda_weight"], want, noise, params["vrange"], params["wrange"], u)[1]


def du_over_range(planner, params, u_ref):
    return float((np.abs(planner.u_cur_d.copy_to_host() - u_ref) / span(params)).max())


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n", ROLLOUTS)
@pytest.mark.parametrize("t", HORIZONS)
def test_stage_level_rollout(n, t):
    w, cfg, lin, ang, planner, params = build("c2", n, t)
    planner.solve()   # (grids sampled)
    g = grids(w, lin, ang)
    noise, u = inputs(n, t, 100 + t)
    want = oracle_run(params, lin, ang, g, noise, u)
    got, name = run_costs(planner, noise, u)
    assert speculative(name) and "noise=read" in name, name
    assert same_bits(got, want), int((got != want).sum())
    planner.update()
    du = du_over_range(planner, params, u_of_update(params, want, noise, u))
    assert du <= 1e-5, du


# ---------------------------------------------------------------------------------------------------------------- 2
LAMBDA = 50.0


@pytest.mark.parametrize("n", ROLLOUTS)
@pytest.mark.parametrize("t", HORIZONS)
def test_noise_generated_in_the_kernel(n, t):
    w, cfg, lin, ang, loop, params = build("c2", n, t, lambda_weight=LAMBDA)
    _, _, _, _, twin, _ = build("c2", n, t, lambda_weight=LAMBDA)
    for planner in (loop, twin):
        planner.solve()
    u_in = loop.u_cur_d.copy_to_host()
    assert same_bits(u_in, twin.u_cur_d.copy_to_host())
    loop.iterate_async(1)
    loop.synchronize()
    name = loop.last_rollout_kernel()
    assert speculative(name) and "noise=in-kernel" in name, name
    twin.sample_noise()
    twin.rollout()
    assert speculative(twin.last_rollout_kernel()) and "noise=read" in twin.last_rollout_kernel()
    twin.update()
    noise = loop.noise_samples_d.copy_to_host()   # (regenerated from the counters of the launch)
    assert same_bits(noise, twin.noise_samples_d.copy_to_host())
    costs = loop.costs_d.copy_to_host()
    assert same_bits(costs, twin.costs_d.copy_to_host()), int((costs != twin.costs_d.copy_to_host()).sum())
    g = grids(w, lin, ang)
    want = oracle_run(params, lin, ang, g, noise, u_in)
    # the control-cost terms count: with the terms of lambda = 1 nearly every cost would be another float32
    other = oracle_run(dict(params, lambda_weight=1.0), lin, ang, g, noise, u_in)
    assert (other != want).mean() > 0.9, float((other != want).mean())
    assert same_bits(costs, want), int((costs != want).sum())
    u_ref = u_of_update(params, want, noise, u_in)
    assert du_over_range(loop, params, u_ref) <= 1e-5
    assert du_over_range(twin, params, u_ref) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("n,t", [(32, 24), (70, 100), (40, 17)])
def test_headings_that_move(n, t):
    wide = np.array([-2.0 * np.pi, 2.0 * np.pi])
    w, cfg, lin, ang, planner, params = build("c2", n, t, wrange=wide)
    planner.solve()
    g = grids(w, lin, ang)
    noise, u = inputs(n, t, 300 + t)
    group = np.arange(t) // 8
    noise[:, :, 1] *= np.where(group % 2 == 1, 4.0, 0.2).astype(f32)[None, :]
    # the oracle's side of "both branches": the heading increment of step s is dt * w_s * traction, traction <= 1 on
    # this map (1 in the start cell); B compares headings s and s + 1 for s = 4 k .. 4 k + 2, a whole wave at a time
    # (one tile; the upper 32 lanes hold the group's second four steps)
    wc = np.clip(u[None, :, 1] + noise[:, :, 1], wide[0], wide[1]).astype(np.float64) * params["dt"]
    compared = (np.arange(t) % 4) != 3
    for tile in range((n + 31) // 32):
        big = (np.abs(wc[32 * tile: 32 * tile + 32]) > 0.37).any(axis=0)
        small = (np.abs(wc[32 * tile: 32 * tile + 32]) < 0.35).all(axis=0)
        per_group_big = [bool((big & compared)[group == k].any()) for k in range(group.max() + 1)]
        per_group_small = [bool((small | ~compared)[group == k].all()) for k in range(group.max() + 1)]
        assert any(per_group_big) and any(per_group_small), (tile, per_group_big, per_group_small)
    want = oracle_run(params, lin, ang, g, noise, u)
    got, name = run_costs(planner, noise, u)
    assert speculative(name), name
    assert same_bits(got, want), int((got != want).sum())
    planner.update()
    assert du_over_range(planner, params, u_of_update(params, want, noise, u)) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n,t", [(70, 17), (70, 100), (200, 17), (800, 100)])
def test_three_folded_iterations_against_the_stage_level_sequence(n, t):
    """(a launch combines the previous launch's tile packets itself when 4 * tiles >= T -- update_plan.h,
    tiles_can_reduce: at N = 70 an update launch runs between the rollout launches, at N = 200 / 800 none does)"""
    w, cfg, lin, ang, loop, params = build("c2", n, t)
    _, _, _, _, staged, _ = build("c2", n, t)
    for planner in (loop, staged):
        planner.solve()
    loop.iterate_async(3)
    loop.synchronize()
    name = loop.last_rollout_kernel()
    assert speculative(name) and "noise=in-kernel" in name, name
    assert ("reduces_tiles=1" in name) == (4 * ((n + 31) // 32) >= t), name
    g = grids(w, lin, ang)
    for _ in range(3):
        u_in = staged.u_cur_d.copy_to_host()
        staged.sample_noise()
        staged.rollout()
        assert speculative(staged.last_rollout_kernel())
        noise = staged.noise_samples_d.copy_to_host()
        want = oracle_run(params, lin, ang, g, noise, u_in)
        assert same_bits(staged.costs_d.copy_to_host(), want)
        staged.update()
        assert du_over_range(staged, params, u_of_update(params, want, noise, u_in)) <= 1e-5
    assert same_bits(loop.noise_samples_d.copy_to_host(), noise)
    assert same_bits(loop.costs_d.copy_to_host(), want), int((loop.costs_d.copy_to_host() != want).sum())
    assert du_over_range(loop, params, staged.u_cur_d.copy_to_host()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("t", [17, 100])
def test_speed_map_form(t):
    n = 64
    w, cfg, lin, ang, planner, params = build("c2m", n, t, lambda_weight=LAMBDA)
    planner.solve()
    g = grids(w, lin, ang)
    noise, u = inputs(n, t, 500 + t)
    want = oracle_run(params, lin, ang, g, noise, u)
    got, name = run_costs(planner, noise, u)
    assert name.startswith("k_rollout_scan_exact speed_map"), name
    assert same_bits(got, want), int((got != want).sum())
    planner.update()
    assert du_over_range(planner, params, u_of_update(params, want, noise, u)) <= 1e-5
    name = folded_iteration_vs_oracle(planner, w, params, lin, ang, g)   # (noise in the kernel)
    assert name.startswith("k_rollout_scan_exact speed_map"), name


def test_failed_vote_reexecuted_by_the_workgroup_then_a_vote_that_holds():
    n, t = 64, 100
    w, cfg, lin, ang, planner, params = build("c2s", n, t)
    planner.set_debug_flags(_lib.DEBUG_KEEP_SPECULATING)
    lin.sample_grids()
    ang.sample_grids()
    g = grids(w, lin, ang)
    noise, u = inputs(n, t, 600)
    want = oracle_run(params, lin, ang, g, noise, u)
    cx, cy = cell_of(params, lin, ang, g["lin"][0], params["x0"][0], params["x0"][1])
    flat = dict(g, lin=np.full_like(g["lin"], g["lin"][0][cy, cx]), ang=np.full_like(g["ang"], g["ang"][0][cy, cx]))
    moved = oracle_run(params, lin, ang, flat, noise, u) != want
    assert moved[:32].any() and moved[32:].any(), "both tiles must leave the start cell's traction"
    got, name = run_costs(planner, noise, u)
    assert speculative(name) and "failed_tiles=pipelined" in name, name
    assert same_bits(got, want), int((got != want).sum())
    planner.update()
    assert speculative(folded_iteration_vs_oracle(planner, w, params, lin, ang, g))
    a_launch_whose_vote_holds(planner, w, params, lin, ang, g, n, t)


def test_failed_vote_rerun_by_the_cost_wave_alone_then_a_vote_that_holds():
    """the c2s map's tractions injected into the speed-map form (no window of 32-bit cells: the cost wave re-runs alone)"""
    n, t = 64, 100
    w, cfg, lin, ang, planner, params = build("c2m", n, t)
    planner.set_debug_flags(_lib.DEBUG_KEEP_SPECULATING)
    planner.solve()
    g = grids(w, lin, ang)
    rows, cols = g["obs"].shape
    nominal = g["lin"][:, :rows, :cols].copy()
    patchy = nominal.copy()
    patchy[:, 2:rows - 2, 2:cols - 2] = np.random.default_rng(6).integers(40, 101, size=(nominal.shape[0], rows - 4, cols - 4)).astype(np.int8)
    lin.set_sampled_grids(patchy)
    ang.set_sampled_grids(patchy)
    g_patchy = dict(g, lin=patchy, ang=patchy)
    noise, u = inputs(n, t, 601)
    want = oracle_run(params, lin, ang, g_patchy, noise, u)
    moved = oracle_run(params, lin, ang, dict(g, lin=nominal, ang=nominal), noise, u) != want
    assert moved[:32].any() and moved[32:].any()
    got, name = run_costs(planner, noise, u)
    assert name.startswith("k_rollout_scan_exact speed_map") and "failed_tiles=one_wave" in name, name
    assert same_bits(got, want), int((got != want).sum())
    planner.update()
    folded_iteration_vs_oracle(planner, w, params, lin, ang, g_patchy)
    lin.set_sampled_grids(nominal)
    ang.set_sampled_grids(nominal)
    a_launch_whose_vote_holds(planner, w, params, lin, ang, dict(g, lin=nominal, ang=nominal), n, t)


def test_direct_form():
    n, t = 64, 100
    w, cfg, lin, ang, planner, params = build("c2s", n, t, lambda_weight=LAMBDA)
    planner.solve()
    g = grids(w, lin, ang)
    noise, u = inputs(n, t, 700)
    want = oracle_run(params, lin, ang, g, noise, u)
    # (two tiles near the start: the planner leaves the speculative form once it has seen their votes fail on these
    #  controls -- review_speculation, at a wait of the host)
    for _ in range(3):
        got, name = run_costs(planner, noise, u)
        assert same_bits(got, want), (name, int((got != want).sum()))
        planner.synchronize()
        if "direct=1" in name:
            break
    assert name.startswith("k_rollout_scan_exact") and "direct=1" in name, name
    assert same_bits(got, want), int((got != want).sum())
    name = folded_iteration_vs_oracle(planner, w, params, lin, ang, g)
    assert "direct=1" in name, name


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("n,t", [(70, 100), (40, 17)])
def test_the_same_launch_twice(n, t):
    w, cfg, lin, ang, planner, params = build("c2", n, t, lambda_weight=LAMBDA)
    planner.solve()
    noise, u = inputs(n, t, 800 + t)
    first, name = run_costs(planner, noise, u)
    second, _ = run_costs(planner, noise, u)
    assert speculative(name), name
    assert same_bits(first, second)
    loops = []
    for _ in range(2):
        _, _, _, _, p, _ = build("c2", n, t, lambda_weight=LAMBDA)
        p.solve()
        p.iterate_async(3)
        p.synchronize()
        loops.append((p.u_cur_d.copy_to_host(), p.costs_d.copy_to_host()))
    assert same_bits(loops[0][0], loops[1][0]) and same_bits(loops[0][1], loops[1][1])
