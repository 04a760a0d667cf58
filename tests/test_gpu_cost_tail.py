"""The tail of k_rollout_scan_exact (rollout_scan_exact_kernel.h): the T control-cost additions behind the terminal
cost, and phase F, the tile's share of the update, which now skips the rollouts whose weight is exactly +0.0f.

Costs: against oracle.rollout_det, BIT FOR BIT, on inputs that drive the additions over what the integer form of
tests/cost_tail_segmented_model.py has to treat specially -- binade crossings up and down (at 4096 and 8192 where the
costs can be put there: with C2's obstacle penalty of 1e5 per step most rollouts of a long horizon cost more whatever
dist_weight is, and the edge is then the next power of two above them; an edge is an edge), exact ties, costs that stay
below 1 and turn negative -- each input proved by that model to be what it is called (round counts); the plain, the
speed-map and the direct form of the kernel (the direct form at C2's own N: the planner launches it once it has seen a
launch's failed votes).  Noise and u go in through the C ABI.

Phase F: one-launch iterations whose tiles hold a single non-zero weight (lambda <= 1, costs far apart) and none
at all that is zero (a large lambda), u against the oracle's update within 1e-5 of the control range; and the loop with
the fold against the loop with an update launch per iteration, the same bits."""
import contextlib

import numpy as np
import pytest

import bench
from cost_tail_segmented_model import can_start_round, segmented, walk
from mppi_numba_amd import _lib
from oracle import oracle as O
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


def oracle_run(w, params, lin, ang, noise, u):
    p = oracle_params(params, lin, ang)
    return O.rollout_det(p, lin.sample_grid_batch_d.copy_to_host(), ang.sample_grid_batch_d.copy_to_host(),
                         lin.obstacle_map_d.copy_to_host(), lin.unknown_map_d.copy_to_host(), noise, u,
                         risk=lin.risk_traction_map_d.copy_to_host() if w.get("speed_map") else None)


def control_terms(params, noise, u):
    """a[n, t] as the oracle forms it (control_cost_term: float64 quotients, products, sum, times float32 lambda)"""
    s = np.asarray(params["u_std"], f64).astype(f32).astype(f64) ** 2
    uo = u.astype(f64) / s[None, :]
    return f64(f32(params["lambda_weight"])) * (uo[None, :, 0] * noise[:, :, 0].astype(f64) + uo[None, :, 1] * noise[:, :, 1].astype(f64))


def inputs(n, t, seed, quantum=None):
    rng = np.random.default_rng(seed)
    noise = (rng.normal(0.0, 1.0, (n, t, 2)) * np.array([2.0, 3.0])).astype(f32)
    u = np.stack([rng.uniform(1.0, 2.5, t), rng.uniform(-1.0, 1.0, t)], axis=1).astype(f32)
    if quantum is not None:
        noise = (np.rint(noise / quantum) * quantum).astype(f32)
        u = (np.rint(u / 0.125) * 0.125).astype(f32)
    return noise, u


def tail_of(w, params, lin, ang, noise, u):
    """(cost after the terminal cost, control-cost terms), proved: walking the terms from that cost gives the oracle's bits"""
    c_term = oracle_run(w, dict(params, lambda_weight=0.0), lin, ang, noise, u)   # (terms of +-0.0 leave a cost >= +0 as it is)
    a = control_terms(params, noise, u)
    want = oracle_run(w, params, lin, ang, noise, u)
    assert np.array_equal(walk(c_term, a).view(np.uint32), want.view(np.uint32))
    return c_term, a, want


def run_costs(planner, noise, u):
    planner.set_noise(noise)
    planner.set_u(u)
    planner.rollout()
    return planner.costs_d.copy_to_host(), planner.last_rollout_kernel()


def binades_visited(c_term, a):
    c = c_term.astype(f32).copy()
    seen = [np.frexp(c)[1]]
    for t in range(a.shape[1]):
        c = (c.astype(f64) + a[:, t]).astype(f32)
        seen.append(np.frexp(c)[1])
    return np.stack(seen, axis=1)   # [n, T + 1]: exponent e with c in [2^(e-1), 2^e)


def dist_weight_for(w, params, lin, ang, noise, u, edge):
    """(dist_weight, edge): the dist_weight (a float32 value) that puts the median cost after the terminal cost on a
    binade edge -- `edge`, or where the costs lie above it whatever the weight (the terminal cost and, in speed-map
    mode, the time charged per step do not scale with it) the next power of two above them.  Costs grow with it."""
    c_at = lambda dw: oracle_run(w, dict(params, dist_weight=dw, lambda_weight=0.0), lin, ang, noise, u)
    floor = float(np.median(c_at(0.0)))
    if floor >= 0.9 * edge:
        edge = float(2.0 ** (np.floor(np.log2(floor / 0.9)) + 1))
    lo, hi = 0.0, 4096.0
    for _ in range(48):
        mid = float(f32(0.5 * (lo + hi)))
        lo, hi = (mid, hi) if np.median(c_at(mid)) < edge else (lo, mid)
    return float(f32(hi)), edge


def lambda_for(params, noise, u, c_term):
    """the power of two that makes the T terms wander about as far as the costs are spread: many rollouts reach the edge"""
    unit = control_terms(dict(params, lambda_weight=1.0), noise, u)
    spread = float(np.subtract(*np.percentile(c_term.astype(f64), [75, 25])))
    return float(2.0 ** np.clip(np.rint(np.log2(max(spread, 1.0) / (unit.std() * np.sqrt(unit.shape[1])))) + 1, 0, 30))


@pytest.mark.parametrize("workload,n,t,edge", [("c2", 32, 100, 4096.0), ("c2", 64, 104, 8192.0), ("c2", 64, 9, 8192.0),
                                               ("c2", 32, 4, 4096.0), ("c2m", 64, 100, 8192.0), ("c2s", 8192, 100, 4096.0)])
def test_costs_that_cross_a_binade_edge_up_and_down(workload, n, t, edge):
    # (the terminal cost, distance / v_post_rollout, does not scale with dist_weight: it has to leave room below the edge)
    w, cfg, lin, ang, planner, params = build(workload, n, t, v_post_rollout=0.05 if edge == 4096.0 else 0.01)
    planner.solve()   # (grids sampled; c2s: the planner has seen the failed votes and launches the direct form)
    noise, u = inputs(n, t, seed=t + n)
    dw, edge = dist_weight_for(w, params, lin, ang, noise, u, edge)
    params = dict(params, dist_weight=dw)
    c_plain = oracle_run(w, dict(params, lambda_weight=0.0), lin, ang, noise, u)
    params = dict(params, lambda_weight=lambda_for(params, noise, u, c_plain))
    planner.set_params(params)
    c_term, a, want = tail_of(w, params, lin, ang, noise, u)
    # the input is what it is called: both sides of the edge at the start, crossings in both directions, >= 2 rounds
    e = binades_visited(c_term, a)
    e_edge = int(np.log2(edge)) + 1
    assert (c_term < edge).sum() >= n // 4 and (c_term >= edge).sum() >= n // 4
    up = ((e[:, :-1] < e_edge) & (e[:, 1:] >= e_edge)).any(axis=1)
    down = ((e[:, :-1] >= e_edge) & (e[:, 1:] < e_edge)).any(axis=1)
    assert up.sum() >= 2 and down.sum() >= 2, (int(up.sum()), int(down.sum()))
    got_model, rounds = segmented(c_term, a)
    assert np.array_equal(got_model.view(np.uint32), want.view(np.uint32))
    if t > 4:
        assert (rounds >= 2).sum() >= 2, rounds
    got, name = run_costs(planner, noise, u)
    print("\n%s N=%d T=%d edge %g: dist_weight %.6f, lambda %g, up %d down %d, most rounds %d, %s" % (
        workload, n, t, edge, dw, params["lambda_weight"], up.sum(), down.sum(), rounds.max(), name))
    assert name.startswith("k_rollout_scan_exact"), name
    assert ("speed_map" in name) == (workload == "c2m") and ("direct=1" in name) == (workload == "c2s"), name
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())


@pytest.mark.parametrize("n,t", [(64, 100), (32, 9)])
def test_costs_whose_terms_are_exact_ties(n, t):
    """lambda = 1, sigma^2 = 4 and 16, u in eighths, noise in 64ths: every term is a multiple of 2^-13 -- a quarter of an
    ulp of a cost in [4096, 8192), an eighth in the binade above: odd multiples of half an ulp, exact ties of the float32
    store, are common."""
    w, cfg, lin, ang, planner, params = build("c2", n, t, lambda_weight=1.0, u_std=np.array([2.0, 4.0]), v_post_rollout=0.02)
    planner.solve()
    noise, u = inputs(n, t, seed=3 * t, quantum=2.0 ** -6)
    params = dict(params, dist_weight=dist_weight_for(w, params, lin, ang, noise, u, 4096.0)[0])
    planner.set_params(params)
    c_term, a, want = tail_of(w, params, lin, ang, noise, u)
    assert np.array_equal(a, np.rint(a * 2.0 ** 13) * 2.0 ** -13)
    half_ulp = np.ldexp(1.0, binades_visited(c_term, a)[:, :-1] - 1 - 24)      # of the cost each term is added to
    halves = a / half_ulp
    ties = (halves == np.rint(halves)) & (np.rint(halves) % 2 != 0)
    got_model, rounds = segmented(c_term, a)
    assert np.array_equal(got_model.view(np.uint32), want.view(np.uint32))
    print("\nN=%d T=%d: rollouts with a tie %d, with >= 2 rounds %d" % (n, t, ties.any(axis=1).sum(), (rounds >= 2).sum()))
    assert ties.any(axis=1).sum() >= 3
    if t > 4:
        assert (rounds >= 2).sum() >= 3
    got, name = run_costs(planner, noise, u)
    assert name.startswith("k_rollout_scan_exact"), name
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())


@pytest.mark.parametrize("n,t", [(64, 9), (32, 4)])
def test_costs_that_stay_below_one_and_turn_negative(n, t):
    """Stage and terminal costs of thousandths, control-cost terms of order 1: the running cost is below 1, passes
    through zero and below -- the model's walk rule (no round starts from such a cost)."""
    w, cfg, lin, ang, planner, params = build("c2", n, t, dist_weight=1e-4, v_post_rollout=1e4)
    planner.solve()
    noise, u = inputs(n, t, seed=5 * t)
    c_term, a, want = tail_of(w, params, lin, ang, noise, u)
    assert (c_term < 1.0).all() and (c_term > 0.0).all()
    running = np.stack([walk(c_term, a[:, :k]) for k in range(t + 1)], axis=1)
    assert (~can_start_round(running)).any(axis=1).sum() >= n // 4      # (negative on the way)
    assert np.array_equal(segmented(c_term, a)[0].view(np.uint32), want.view(np.uint32))
    got, name = run_costs(planner, noise, u)
    assert name.startswith("k_rollout_scan_exact"), name
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())


def tile_weights(costs, lam, tile=32):
    c = costs.reshape(-1, tile)
    return np.exp(-(c - c.min(axis=1, keepdims=True)).astype(f64) / lam).astype(f32)


@pytest.mark.parametrize("workload,n,t,lam", [("c2", 64, 100, 1.0), ("c2", 64, 100, 1e5), ("c2", 32, 9, 2.0 ** -10), ("c2", 64, 104, 1e5),
                                              ("c2m", 64, 100, 1.0), ("c2s", 64, 100, 2.0 ** -10)])
def test_update_sums_of_tiles_with_one_and_with_no_zero_weight(workload, n, t, lam):
    """One-launch iterations: the tile packets of the rollout launch (phase F) are all the update sees of the noise."""
    w, cfg, lin, ang, planner, params = build(workload, n, t, lambda_weight=lam)
    planner.solve()
    planner.iterate_async(2)   # (c2s: direct form from here on)
    planner.synchronize()
    u_in = planner.u_cur_d.copy_to_host()
    planner.iterate_async(1)
    planner.synchronize()
    name = planner.last_rollout_kernel()
    assert name.startswith("k_rollout_scan_exact"), name
    noise = planner.noise_samples_d.copy_to_host()   # (regenerated from the counters of the last launch)
    costs = planner.costs_d.copy_to_host()
    want = oracle_run(w, params, lin, ang, noise, u_in)
    assert np.array_equal(costs.view(np.uint32), want.view(np.uint32))
    wt = tile_weights(costs, lam)
    if lam <= 1.0:
        assert ((wt != 0.0).sum(axis=1) == 1).any(), (wt != 0.0).sum(axis=1)   # a tile where every weight but one is zero
    else:
        assert (wt != 0.0).all()                                                 # tiles where none is
    _, u_ref, _ = O.update_useq(params["lambda_weight"], want, noise, params["vrange"], params["wrange"], u_in)
    du = float((np.abs(planner.u_cur_d.copy_to_host() - u_ref) / span(params)).max())
    print("\n%s N=%d T=%d lambda %g: non-zero weights per tile %s, du / range %.2e" % (workload, n, t, lam, (wt != 0.0).sum(axis=1), du))
    assert du <= 1e-5, du


@pytest.mark.parametrize("n,t", [(64, 8), (64, 100)])
def test_loop_of_four_iterations_with_the_fold_equals_the_loop_with_update_launches(n, t):
    _, _, _, _, folded, params = build("c2", n, t)
    _, _, _, _, plain, _ = build("c2", n, t)
    plain.set_debug_flags(_lib.DEBUG_NO_REDUCE_FOLD)
    for planner in (folded, plain):
        planner.solve()
        planner.iterate_async(4)
        planner.synchronize()
    name = folded.last_rollout_kernel()
    assert name.startswith("k_rollout_scan_exact") and ("reduces_tiles=1" in name) == (4 * (n // 32) >= t), name
    assert "reduces_tiles" not in plain.last_rollout_kernel()
    assert np.array_equal(folded.u_cur_d.copy_to_host().view(np.uint32), plain.u_cur_d.copy_to_host().view(np.uint32))
    assert np.array_equal(folded.costs_d.copy_to_host().view(np.uint32), plain.costs_d.copy_to_host().view(np.uint32))
