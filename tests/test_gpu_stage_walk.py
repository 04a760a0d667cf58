"""The stage-cost walk of k_rollout_scan_exact (rollout_scan_exact_kernel.h, wave 1) and the records it consumes.

A chunk wave tells the walk with the value it raises on c_done whether its group of 8 steps holds a penalty (the walk
adds stage cost, obstacle and unknown penalty per step, the reference's order) or none (the stage costs alone); the
records lie in LDS as four planes per chunk of 4 steps (stage costs 0-1, 2-3, obstacle, unknown), one 16-byte vector
per rollout in each.  Costs against
oracle.rollout_det, BIT FOR BIT on every rollout, on maps made for each kind of group: (a) nothing flagged, (b)
obstacles only, (c) unknown cells only, (d) one mask for both, (e) disjoint masks -- both penalties in a group, never in
one step: where a walk could add po + pu as ONE addend exactly, one of them being +0.0f -- (f) as (d) with cells of zero
traction next to the start, where stopped rollouts go on paying both penalties through the same records.  Every case
proves on the CPU that it is what it is called (tests/stage_walk_model.py, itself proved against the oracle on the
very input).

Whether adding po + pu as one float32 addend can be told from the reference's two additions depends on the penalties:
with C2's 1e5 and 1e2 it cannot on these costs (both are multiples of the cost's ulp up to 2^24, so the only way to
differ is a binade edge between c + 1e5 and c + 1e5 + 1e2, and k * 100100 plus at most T stage costs never lies within
100 above a power of two for k <= 104) -- a walk that merged everywhere would pass (d) unseen.  So (d) runs twice: with
C2's penalties, and ("d3") with an unknown penalty of 1/3, where the merged sum rounds differently on many rollouts;
there the test asserts that such a merge changes bits.  (A walk that merges where that is exact was built and measured:
profiles/HISTORY.md, "C2 rollout: the stage-cost walk"; these tests are what it passed.)

Then one loop of 6 one-launch iterations on map (d) at C2's N against the loop with an update launch per iteration."""
import contextlib

import numpy as np
import pytest

import bench
from mppi_numba_amd import _lib
from oracle import oracle as O
from stage_walk_model import control_terms, stage_records, walk
from test_gpu_scale import oracle_params

pytestmark = pytest.mark.gpu
f32 = np.float32
DENSITY = 0.3
ZERO_COLS = 2          # (f): columns of zero traction at the map's left edge, x < 0.5 m
START_F = np.array([1.0, 30.0, np.pi])   # 1 m from that edge, heading for it


def masks(kind, rows=256, cols=256):
    q = np.random.default_rng(ord(kind[0])).random((rows, cols))
    none, some = np.zeros((rows, cols), np.int8), (q < DENSITY).astype(np.int8)
    if kind == "a":
        return none, none
    if kind == "b":
        return some, none
    if kind == "c":
        return none, some
    if kind == "e":
        return some, ((q >= DENSITY) & (q < 2 * DENSITY)).astype(np.int8)
    if kind == "f":
        some[:, :ZERO_COLS] = 1   # (wherever a rollout stops, it stands on both flags)
    return some, some.copy()   # d, d3, f


@contextlib.contextmanager
def world_of(kind, t, **params):
    """bench.build_planner's world with this test's masks (f: and its columns of zero traction), horizon and parameters"""
    saved = bench.synthetic_world, bench.make_params, dict(bench.WORKLOADS)

    def world(workload, rng):
        pmf, _, _, tdm_dict = saved[0](workload, rng)
        obstacle, unknown = masks(kind)
        if kind == "f":
            pmf = pmf.copy()
            pmf[:, :, :ZERO_COLS] = 0
            pmf[0, :, :ZERO_COLS] = 100
        return pmf, obstacle, unknown, tdm_dict

    bench.synthetic_world = world
    bench.make_params = lambda name: dict(saved[1](name), **params)
    for name in ("c2", "c2m"):
        bench.WORKLOADS[name] = dict(saved[2][name], t=t)
    try:
        yield
    finally:
        bench.synthetic_world, bench.make_params = saved[:2]
        bench.WORKLOADS.update(saved[2])


def params_of(kind):
    extra = {}
    if kind == "d3":
        extra["unknown_penalty"] = 1.0 / 3.0
    if kind == "f":
        extra["x0"] = START_F
    return extra


def build(workload, kind, n, t):
    with world_of(kind, t, **params_of(kind)):
        return bench.build_planner(workload, n)


def inputs(n, t):
    rng = np.random.default_rng(1000 * t + n)
    noise = (rng.normal(0.0, 1.0, (n, t, 2)) * np.array([2.0, 3.0])).astype(f32)
    u = np.stack([rng.uniform(1.0, 2.5, t), rng.uniform(-1.0, 1.0, t)], axis=1).astype(f32)
    return noise, u


def check_case(kind, rec, want, terms):
    """the case is what it is called; returns a line for the log"""
    same_bits = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert same_bits(walk(rec, terms), want), "the model does not restate the oracle on this input"
    o, q = (rec["po"] != 0) & rec["active"], (rec["pu"] != 0) & rec["active"]
    both, either = int((o & q).sum()), int((o | q).sum())
    standing_both = int((o & q & rec["still"]).sum())
    differs = int((walk(rec, terms, merged=True) != want).sum())
    if kind == "a":
        assert either == 0
    elif kind == "b":
        assert o.sum() > 0 and q.sum() == 0
    elif kind == "c":
        assert q.sum() > 0 and o.sum() == 0
    elif kind == "e":
        assert o.sum() > 0 and q.sum() > 0 and both == 0
        assert differs == 0       # (one addend is +0.0f in every step: the merged walk is exact)
    else:
        assert both > 0
    if kind == "d3":
        assert differs > 0        # a walk that merged where both penalties fall in one step would not pass
    if kind == "f":
        assert standing_both > 0  # stopped rollouts that go on paying both penalties where they stand
    return "steps with a penalty %d, with both %d (standing %d), rollouts a merged walk gets wrong %d" % (
        either, both, standing_both, differs)


T_ALL, N_ALL = (8, 9, 16, 100, 104), (32, 33, 64)
CASES = [("c2", kind, N_ALL[(i + j) % 3], t) for i, kind in enumerate(("a", "b", "c", "d", "d3", "e", "f")) for j, t in enumerate(T_ALL)]
# the speed-map form shares the walk: both kinds of group at every horizon, the one-penalty maps at C2's
CASES += [("c2m", kind, N_ALL[(i + j + 1) % 3], t) for i, kind in enumerate(("d3", "e")) for j, t in enumerate(T_ALL)]
CASES += [("c2m", kind, n, 100) for kind, n in (("a", 33), ("b", 64), ("c", 32), ("d", 33))]


@pytest.mark.parametrize("workload,kind,n,t", CASES)
def test_costs_have_the_bits_of_the_oracle(workload, kind, n, t):
    w, cfg, lin, ang, planner, params = build(workload, kind, n, t)
    planner.solve()   # (grids sampled)
    noise, u = inputs(n, t)
    p = oracle_params(params, lin, ang)
    grids = (lin.sample_grid_batch_d.copy_to_host(), ang.sample_grid_batch_d.copy_to_host(),
             lin.obstacle_map_d.copy_to_host(), lin.unknown_map_d.copy_to_host())
    risk = lin.risk_traction_map_d.copy_to_host().reshape(grids[2].shape) if w.get("speed_map") else None
    want = O.rollout_det(p, *grids, noise, u, risk=risk)
    said = check_case(kind, stage_records(p, *grids, noise, u, risk=risk), want, control_terms(p, noise, u))
    planner.set_noise(noise)
    planner.set_u(u)
    planner.rollout()
    got, name = planner.costs_d.copy_to_host(), planner.last_rollout_kernel()
    print("\n%s (%s) N=%d T=%d: %s; %s" % (workload, kind, n, t, said, name))
    assert name.startswith("k_rollout_scan_exact") and "direct=1" not in name, name
    assert ("speed_map" in name) == (workload == "c2m"), name
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())


def test_loop_of_six_iterations_with_the_fold_equals_the_loop_with_update_launches():
    _, _, _, _, folded, _ = build("c2", "d", 8192, 100)
    _, _, _, _, plain, _ = build("c2", "d", 8192, 100)
    plain.set_debug_flags(_lib.DEBUG_NO_REDUCE_FOLD)
    for planner in (folded, plain):
        planner.solve()
        planner.iterate_async(6)
        planner.synchronize()
    name = folded.last_rollout_kernel()
    assert name.startswith("k_rollout_scan_exact") and "direct=1" not in name and "reduces_tiles=1" in name, name
    assert "reduces_tiles" not in plain.last_rollout_kernel()
    assert np.array_equal(folded.u_cur_d.copy_to_host().view(np.uint32), plain.u_cur_d.copy_to_host().view(np.uint32))
    assert np.array_equal(folded.costs_d.copy_to_host().view(np.uint32), plain.costs_d.copy_to_host().view(np.uint32))
