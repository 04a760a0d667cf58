"""The tail of k_rollout_scan_exact (rollout_scan_exact_kernel.h) behind the last group of the stage-cost walk: the
cost wave asks for what the tail starts with (the vote, the events, the terminal cost, the control-cost flags and the
first terms) while it still walks the last group; then the T control-cost additions, the weights, the hand-over to
phase F and the tile sums.  Written for a change of four parts to that stretch, of which the look ahead was kept
(profiles/HISTORY.md, "C2 rollout tail: what the control-cost walk starts with ..."); the cases cover what the other
three would have touched as well -- last groups with padded steps, the vote's verdict on every path, tiles with any
number of weighted rollouts -- and pass on the kernel before the change.

The checker is the oracle throughout (oracle.rollout_det, oracle.update_useq); at these sizes no rollout may be left
out: every cost BIT FOR BIT.

  1  costs of a stage-level rollout (noise and u through the C ABI): last groups with 4, 1, 8, 1, 4 valid steps and a
     single group, a ragged last tile, horizons on both sides of phase F's 64-lane split; obstacle / unknown penalties
     in the last group where the oracle's side says so
  2  u after one-launch iterations, lambda from one non-zero weight per tile to all 32; the loop with the fold against
     the loop with an update launch per iteration
  3  a failed vote on both re-run paths (re-execution by the workgroup; the cost wave alone), and a launch whose vote
     holds on the same handle behind each
  4  the direct form at C2's N and the speed-map form
  5  graph replay, 6 repeatability"""
import contextlib

import numpy as np
import pytest

import bench
from mppi_numba_amd import _lib
from oracle import oracle as O
from scan_model import _cell_index
from stage_walk_model import stage_records
from test_gpu_scale import oracle_params

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


@contextlib.contextmanager
def workload_with(workload, t, **params):
    saved_w, saved_make = dict(bench.WORKLOADS[workload]), bench.make_params
    bench.WORKLOADS[workload] = dict(saved_w, t=t)
    bench.make_params = lambda name: dict(saved_make(name), **params)
    try:
        yield
    finally:
        bench.WORKLOADS[workload], bench.make_params = saved_w, saved_make


def build(workload, n, t, **params):
    with workload_with(workload, t, **params):
        return bench.build_planner(workload, n)


def span(params):
    return np.array([params["vrange"][1] - params["vrange"][0], params["wrange"][1] - params["wrange"][0]])


def grids(w, lin, ang):
    return dict(lin=lin.sample_grid_batch_d.copy_to_host(), ang=ang.sample_grid_batch_d.copy_to_host(),
                obs=lin.obstacle_map_d.copy_to_host(), unk=lin.unknown_map_d.copy_to_host(),
                risk=lin.risk_traction_map_d.copy_to_host() if w.get("speed_map") else None)


def oracle_run(params, lin, ang, g, noise, u):
    return O.rollout_det(oracle_params(params, lin, ang), g["lin"], g["ang"], g["obs"], g["unk"], noise, u, risk=g["risk"])


def inputs(n, t, seed, scale=1.0, u_zero=False):
    rng = np.random.default_rng(seed)
    noise = (rng.normal(0.0, 1.0, (n, t, 2)) * np.array([2.0, 3.0]) * scale).astype(f32)
    u = np.stack([rng.uniform(1.0, 2.5, t), rng.uniform(-1.0, 1.0, t)], axis=1).astype(f32)
    return noise, (np.zeros_like(u) if u_zero else u)


def run_costs(planner, noise, u):
    planner.set_noise(noise)
    planner.set_u(u)
    planner.rollout()
    return planner.costs_d.copy_to_host(), planner.last_rollout_kernel()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def last_group_penalties(params, lin, ang, g, noise, u):
    """rollouts that pay an obstacle or unknown penalty in a step of the horizon's last group of 8 (the oracle's side)"""
    rec = stage_records(oracle_params(params, lin, ang), g["lin"], g["ang"], g["obs"], g["unk"], noise, u, risk=g["risk"])
    t = noise.shape[1]
    first = 8 * ((t - 1) // 8)
    return int((rec["active"][:, first:] & ((rec["po"][:, first:] != 0) | (rec["pu"][:, first:] != 0))).any(axis=1).sum())


# ---------------------------------------------------------------------------------------------------------------- 1
# (n, t, seed, a penalty in the last group?)  C2's maps flag 2 % of the cells as obstacles and 2 % as unknown
STAGE_CASES = [(32, 100, 1, True), (40, 17, 2, None), (64, 104, 3, True), (64, 97, 4, True), (32, 4, 5, None),
               (200, 65, 6, True), (200, 64, 7, True)]


@pytest.mark.parametrize("n,t,seed,pen", STAGE_CASES)
def test_costs_of_a_stage_level_rollout(n, t, seed, pen):
    w, cfg, lin, ang, planner, params = build("c2", n, t)
    planner.solve()   # (grids sampled)
    g = grids(w, lin, ang)
    noise, u = inputs(n, t, seed)
    want = oracle_run(params, lin, ang, g, noise, u)
    paying = last_group_penalties(params, lin, ang, g, noise, u)
    got, name = run_costs(planner, noise, u)
    print("\nN=%d T=%d: %d valid steps in the last group, %d rollouts pay a penalty there, %d costs differ, %s" % (
        n, t, t - 8 * ((t - 1) // 8), paying, int((got != want).sum()), name))
    assert name.startswith("k_rollout_scan_exact") and "direct=1" not in name, name
    if pen:
        assert paying > 0
    assert same_bits(got, want), int((got != want).sum())


# ---------------------------------------------------------------------------------------------------------------- 2
def tile_weights(costs, lam, tile=32):
    pad = (-costs.size) % tile
    c = np.concatenate([costs, np.full(pad, np.inf, f32)]).reshape(-1, tile)
    return np.exp(-(c - c.min(axis=1, keepdims=True)).astype(f64) / lam).astype(f32)


@pytest.mark.parametrize("n,t", [(200, 100), (40, 17)])
@pytest.mark.parametrize("lam", [0.5, 1.0, 64.0, 1e4, 1e6])
def test_u_after_one_launch_iterations(n, t, lam):
    """iterate_async(k): the last launch of the call rolls out on the u that k - 1 iterations leave (a twin handle's,
    the same bits: tests/test_gpu_reduce_fold.py) and on the noise of its own Philox block; its tile packets (phase F)
    are all the update sees of that noise."""
    for k in (2, 5):
        w, cfg, lin, ang, loop, params = build("c2", n, t, lambda_weight=lam)
        _, _, _, _, twin, _ = build("c2", n, t, lambda_weight=lam)
        for planner in (loop, twin):
            planner.solve()
        twin.iterate_async(k - 1)
        twin.synchronize()
        u_in = twin.u_cur_d.copy_to_host()
        loop.iterate_async(k)
        loop.synchronize()
        name = loop.last_rollout_kernel()
        assert name.startswith("k_rollout_scan_exact"), name
        noise = loop.noise_samples_d.copy_to_host()   # (regenerated from the counters of the last launch)
        costs = loop.costs_d.copy_to_host()
        want = oracle_run(params, lin, ang, grids(w, lin, ang), noise, u_in)
        assert same_bits(costs, want), (k, int((costs != want).sum()))
        _, u_ref, _ = O.update_useq(params["lambda_weight"], want, noise, params["vrange"], params["wrange"], u_in)
        du = float((np.abs(loop.u_cur_d.copy_to_host() - u_ref) / span(params)).max())
        counts = (tile_weights(costs, lam) != 0.0).sum(axis=1)
        print("\nN=%d T=%d lambda %g k=%d: non-zero weights per tile %s, du / range %.2e" % (n, t, lam, k, counts, du))
        assert du <= 1e-5, (k, du)


@pytest.mark.parametrize("n,t", [(40, 17), (200, 65), (64, 97)])
def test_loop_with_the_fold_equals_the_loop_with_update_launches(n, t):
    _, _, _, _, folded, params = build("c2", n, t)
    _, _, _, _, plain, _ = build("c2", n, t)
    plain.set_debug_flags(_lib.DEBUG_NO_REDUCE_FOLD)
    for planner in (folded, plain):
        planner.solve()
    for k in (1, 2, 5, 8):
        for planner in (folded, plain):
            planner.iterate_async(k)
            planner.synchronize()
        assert folded.last_rollout_kernel().startswith("k_rollout_scan_exact"), folded.last_rollout_kernel()
        assert "reduces_tiles" not in plain.last_rollout_kernel()
        assert same_bits(folded.u_cur_d.copy_to_host(), plain.u_cur_d.copy_to_host()), k
        assert same_bits(folded.costs_d.copy_to_host(), plain.costs_d.copy_to_host()), k


# ---------------------------------------------------------------------------------------------------------------- 3
def folded_iteration_vs_oracle(planner, w, params, lin, ang, g):
    """one iterate_async(1): costs of its launch against the oracle (bits), its u against the oracle's update"""
    u_in = planner.u_cur_d.copy_to_host()
    planner.iterate_async(1)
    planner.synchronize()
    name = planner.last_rollout_kernel()
    noise = planner.noise_samples_d.copy_to_host()
    costs = planner.costs_d.copy_to_host()
    want = oracle_run(params, lin, ang, g, noise, u_in)
    assert same_bits(costs, want), (name, int((costs != want).sum()))
    _, u_ref, _ = O.update_useq(params["lambda_weight"], want, noise, params["vrange"], params["wrange"], u_in)
    du = float((np.abs(planner.u_cur_d.copy_to_host() - u_ref) / span(params)).max())
    assert du <= 1e-5, (name, du)
    return name


def cell_of(params, lin, ang, grid, x, y):
    p = oracle_params(params, lin, ang)
    return (int(_cell_index(np.array([x], f32), f32(p.xlo), f32(p.res), grid.shape[1])[0]),
            int(_cell_index(np.array([y], f32), f32(p.ylo), f32(p.res), grid.shape[0])[0]))


def uniform_around_start(params, lin, ang, g, reach):
    """every cell within `reach` metres of the start carries the start cell's traction: a vote there must hold"""
    x0, y0 = float(params["x0"][0]), float(params["x0"][1])
    ok = True
    for grid in (g["lin"][0], g["ang"][0]):
        (xa, ya), (xs, ys), (xb, yb) = (cell_of(params, lin, ang, grid, x0 + d, y0 + d) for d in (-reach, 0.0, reach))
        ok = ok and bool((grid[ya:yb + 1, xa:xb + 1] == grid[ys, xs]).all())
    return ok


def a_launch_whose_vote_holds(planner, w, params, lin, ang, g, n, t):
    """zero controls and a noise that moves nobody further than 0.5 m in the horizon (traction <= 1): every visited cell
    carries the start cell's traction"""
    assert uniform_around_start(params, lin, ang, g, 0.75)
    noise, u = inputs(n, t, 11, scale=0.02, u_zero=True)
    assert float(np.clip(noise[:, :, 0], 0.0, None).sum(axis=1).max()) * params["dt"] < 0.5
    got, name = run_costs(planner, noise, u)
    assert name.startswith("k_rollout_scan_exact") and "direct=1" not in name, name
    want = oracle_run(params, lin, ang, g, noise, u)
    assert same_bits(got, want), int((got != want).sum())


def test_a_failed_vote_reexecuted_by_the_workgroup_then_a_vote_that_holds():
    n, t = 64, 100
    w, cfg, lin, ang, planner, params = build("c2s", n, t)
    planner.set_debug_flags(_lib.DEBUG_KEEP_SPECULATING)
    lin.sample_grids()
    ang.sample_grids()
    g = grids(w, lin, ang)
    noise, u = inputs(n, t, 8)
    want = oracle_run(params, lin, ang, g, noise, u)
    # the oracle's side of "the vote fails": with the start cell's traction everywhere the costs would be others
    cx, cy = cell_of(params, lin, ang, g["lin"][0], params["x0"][0], params["x0"][1])
    flat = dict(g, lin=np.full_like(g["lin"], g["lin"][0][cy, cx]), ang=np.full_like(g["ang"], g["ang"][0][cy, cx]))
    moved = oracle_run(params, lin, ang, flat, noise, u) != want
    assert moved[:32].any() and moved[32:].any(), "both tiles must leave the start cell's traction"
    got, name = run_costs(planner, noise, u)   # (the handle's first launch: speculative, the window fits)
    assert name.startswith("k_rollout_scan_exact") and "failed_tiles=pipelined" in name and "direct=1" not in name, name
    assert same_bits(got, want), int((got != want).sum())
    planner.update()
    name = folded_iteration_vs_oracle(planner, w, params, lin, ang, g)
    assert name.startswith("k_rollout_scan_exact") and "direct=1" not in name, name
    a_launch_whose_vote_holds(planner, w, params, lin, ang, g, n, t)


def test_a_failed_vote_rerun_by_the_cost_wave_alone_then_a_vote_that_holds():
    """speed-map mode, traction that changes from cell to cell injected through the C API (tests/test_gpu_speedmap_scan.py)"""
    n, t = 64, 100
    w, cfg, lin, ang, planner, params = build("c2m", n, t)
    planner.set_debug_flags(_lib.DEBUG_KEEP_SPECULATING)
    planner.solve()
    g = grids(w, lin, ang)
    rows, cols = g["obs"].shape
    nominal = g["lin"][:, :rows, :cols].copy()
    noisy = nominal.copy()
    noisy[:, 2:rows - 2, 2:cols - 2] = np.random.default_rng(5).integers(40, 101, size=(nominal.shape[0], rows - 4, cols - 4)).astype(np.int8)
    lin.set_sampled_grids(noisy)
    ang.set_sampled_grids(noisy)
    g_noisy = dict(g, lin=noisy, ang=noisy)
    noise, u = inputs(n, t, 9)
    want = oracle_run(params, lin, ang, g_noisy, noise, u)
    moved = oracle_run(params, lin, ang, dict(g, lin=nominal, ang=nominal), noise, u) != want
    assert moved[:32].any() and moved[32:].any(), "both tiles must meet another traction than the start cell's"
    got, name = run_costs(planner, noise, u)
    assert name.startswith("k_rollout_scan_exact speed_map"), name
    assert same_bits(got, want), int((got != want).sum())
    planner.update()
    name = folded_iteration_vs_oracle(planner, w, params, lin, ang, g_noisy)
    assert name.startswith("k_rollout_scan_exact speed_map"), name
    # the nominal grids again: every vote holds
    lin.set_sampled_grids(nominal)
    ang.set_sampled_grids(nominal)
    a_launch_whose_vote_holds(planner, w, params, lin, ang, dict(g, lin=nominal, ang=nominal), n, t)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("workload,n,t", [("c2s", 8192, 100), ("c2m", 64, 100)])
def test_costs_of_the_direct_and_of_the_speed_map_form(workload, n, t):
    w, cfg, lin, ang, planner, params = build(workload, n, t)
    planner.solve()   # (c2s: the planner has seen the failed votes and launches the direct form)
    g = grids(w, lin, ang)
    noise, u = inputs(n, t, 10)
    got, name = run_costs(planner, noise, u)
    assert name.startswith("k_rollout_scan_exact"), name
    assert ("speed_map" in name) == (workload == "c2m") and ("direct=1" in name) == (workload == "c2s"), name
    want = oracle_run(params, lin, ang, g, noise, u)
    assert same_bits(got, want), int((got != want).sum())


# ---------------------------------------------------------------------------------------------------------------- 5, 6
def run(planner, iterations, calls=1):
    for _ in range(calls):
        planner.iterate_async(iterations)
        planner.synchronize()
    return planner.u_cur_d.copy_to_host(), planner.costs_d.copy_to_host()


def test_graph_replay_of_the_loop_has_the_bits_of_direct_launches():
    _, _, _, _, direct, _ = build("c2", 40, 17)
    _, _, _, _, graphed, _ = build("c2", 40, 17)
    graphed.set_graph_replay(True, iterations_per_graph=2)
    for planner in (direct, graphed):
        planner.solve()
    for chunk in (2, 8, 4):
        u_d, c_d = run(direct, chunk)
        u_g, c_g = run(graphed, chunk)
        assert same_bits(u_d, u_g) and same_bits(c_d, c_g), chunk


def test_the_loop_is_repeatable():
    got = []
    for _ in range(3):
        _, _, _, _, planner, _ = build("c2", 200, 100)
        planner.solve()
        got.append(run(planner, 7, calls=3))
    for u, c in got[1:]:
        assert same_bits(u, got[0][0]) and same_bits(c, got[0][1])
