"""Wall obstacles of the barebone planner in crowd mode (params['wall_segments'] / ['wall_halfwidth'],
mppi_planner_set_walls): thick segments tested against the SEGMENT a step covers, so that no step jumps a thin wall.
k_rollout_barebone_crowd<..., WALLS> counts the wall hits of a step beside its disc hits; every comparison of costs here is
bit for bit with tests/wall_model.py (whose arithmetic tests/test_wall_model.py checks on the CPU)."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_barebone_batch import ERR_INVALID, assert_bits, make_params, oracle_params, problem_params, problems
from test_gpu_barebone_crowd import cfg_of, inputs, shape_of
from test_gpu_barebone_tracks import moving_tracks, rollout_with, track_params
from crowd_model import crowd_discs, hit_counts
from wall_model import active_steps, chain, hit, pure_crossing, wall_costs, wall_hits_of_states

pytestmark = pytest.mark.gpu

OBS_PENALTY = 1e6  # make_params
N = 200            # the last tile is partial
GOAL = np.array([2.2, 2.2])  # within reach of both horizons (x0 = (0, 0, pi / 4): 3.1 m along the diagonal)
DIAG, SIDE = np.array([1.0, 1.0]) / np.sqrt(2.0), np.array([-1.0, 1.0]) / np.sqrt(2.0)


def building(count):
    """`count` walls for the task of make_params with GOAL.  In this order:
      0  thin (h = 0.01), across the diagonal 0.8 m from the start: steps are up to 0.18 m long, so it is jumped;
      1  thin, across the diagonal 0.3 m BEHIND the goal: a rollout that reaches the goal (tolerance 0.5) goes on and
         crosses it after the freeze;
      2, 3  thick (h = 0.25), crossing each other on the diagonal 1.6 m from the start: two hits at one step, and a
         rollout stays inside for several steps;
      the rest: short walls scattered over the scene, half-widths 0 .. 0.1 (every fourth one exactly 0)."""
    rng = np.random.default_rng(99)
    seg = np.empty((count, 2, 2))
    hw = np.empty(count)
    fixed = [(0.8 * DIAG - 3 * SIDE, 0.8 * DIAG + 3 * SIDE, 0.01),
             (GOAL + 0.3 * DIAG - 3 * SIDE, GOAL + 0.3 * DIAG + 3 * SIDE, 0.01),
             (1.6 * DIAG - DIAG - 0.5 * SIDE, 1.6 * DIAG + DIAG + 0.5 * SIDE, 0.25),
             (1.6 * DIAG - 1.5 * SIDE, 1.6 * DIAG + 1.5 * SIDE, 0.25)]
    for k in range(count):
        if k < len(fixed):
            seg[k, 0], seg[k, 1], hw[k] = fixed[k]
        else:
            a = rng.uniform(-1.0, 4.0, 2)
            seg[k, 0], seg[k, 1] = a, a + rng.uniform(-0.6, 0.6, 2)
            hw[k] = 0.0 if k % 4 == 0 else rng.uniform(0.0, 0.1)
    return seg.astype(np.float32), hw.astype(np.float32)


def wall_params(params, seg, hw):
    p = dict(params)
    p["wall_segments"], p["wall_halfwidth"] = seg, hw
    return p


def without_walls(params):
    return {k: v for k, v in params.items() if not k.startswith("wall_")}


@functools.lru_cache(maxsize=None)
def task(t, wscale):
    """Controls and noise of a (horizon, rotation on / off) pair: shared by the cases, never changed."""
    rng = np.random.default_rng(100 * t + int(10 * wscale))
    params = make_params(0.1, wscale)
    params["xgoal"] = GOAL.copy()
    params["vrange"] = np.array([0.0, 1.8])  # steps of up to 0.18 m
    u_in, noise = inputs(rng, N, t)
    u_in.setflags(write=False)
    noise.setflags(write=False)
    return params, u_in, noise


def discs_of(K, kind, t, params):
    rng = np.random.default_rng(K + 7)
    pos, rad = crowd_discs(rng, K, params["x0"], params["xgoal"])
    if kind == "tracks":
        return moving_tracks(rng, pos, 0.1, t + 1), rad
    return pos, rad


def the_input_means_something(p, tracks, rad, seg, hw, noise, u_in, offset=0):
    """Asserted with the model before anything is compared.  One wall cannot be hit twice at a step and the scene's fixed
    walls are its first four: the four statements are made from four walls on, the jumped wall always."""
    W = len(seg)
    disc_counts, st = hit_counts(p, tracks, rad, noise, u_in, offset)
    P, Q = st[:, :-1, :2], st[:, 1:, :2]
    assert hw[0] == np.float32(0.01) and np.linalg.norm((Q - P).astype(np.float64), axis=-1).max() <= 0.18 + 1e-6
    assert pure_crossing(P, Q, seg[0, 0], seg[0, 1], hw[0]).any(), "bad input: no step jumps the thin wall (neither end within h of it)"
    walls = wall_hits_of_states(st, seg, hw)
    model = chain(p, disc_counts + walls, st, noise, u_in)  # (= wall_costs(p, tracks, rad, seg, hw, noise, u_in, offset))
    if W >= 4:
        assert (walls >= 2).any(), "bad input: no (rollout, step) pair has two wall hits"
        frozen = ~active_steps(p, st)
        assert (frozen & (walls > 0)).any(), "bad input: no rollout hits a wall after it has reached the goal"
        assert (model > 2 * OBS_PENALTY).any(), "bad input: no rollout costs more than 2 x obs_penalty"
    return model


CASES = [(W, K, kind, t, wscale) for W in (1, 64, 65, 130) for K in (0, 3, 70) for kind in ("static", "tracks")
         for t, wscale in ((30, 1.0), (37, 1.5), (37, 1.0), (30, 1.5))]


@pytest.mark.parametrize("W,K,kind,t,wscale", CASES)
def test_costs_equal_the_model(W, K, kind, t, wscale):
    """Exact math, rotation on (wscale 1.0) and off (1.5); T = 30 and 37: more than one chunk, no multiple of the waves."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, wscale)
    seg, hw = building(W)
    where, rad = discs_of(K, kind, t, params)
    if kind == "tracks":
        tracks, full = where, wall_params(track_params(params, where, rad), seg, hw)
    else:
        tracks, full = where[:, None, :], wall_params(problem_params(params, params["x0"], params["xgoal"], (where, rad)), seg, hw)
    full["x0"], full["xgoal"] = params["x0"], params["xgoal"]
    p = oracle_params(without_walls(params))
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.set_params(full)
    for offset in ((0, 5) if kind == "tracks" else (0,)):
        model = the_input_means_something(p, tracks, rad, seg, hw, noise, u_in, offset)
        planner.move_mppi_task_vars_to_device()  # (hands the tracks over the first time: offset 0)
        planner.set_track_offset(offset)
        got, _, _, kernel = rollout_with(planner, u_in, noise)
        chunk = shape_of(kernel)[1]
        assert t > chunk, kernel
        assert kernel.endswith(" walls=%d" % W), kernel
        assert ("rotation=1" in kernel) == (wscale == 1.0) and "exact=1" in kernel, kernel
        assert ("tracks=%d" % (t + 1) in kernel) == (kind == "tracks"), kernel
        assert_bits(got, model, "%d walls, %d discs (%s, offset %d) vs the model" % (W, K, kind, offset))


@pytest.mark.parametrize("W,K,kind,t", [(65, 3, "static", 37), (130, 70, "tracks", 30), (1, 0, "static", 30)])
def test_fast_math_adds_the_wall_hits(W, K, kind, t):
    """math="fast" rolls its states out in float32 (sincosf, fmaf); the handle reports no such states at stage level --
    get_state_rollout is the float64 form -- so this is the second of the two statements: a launch with the walls and a
    launch without differ by the model's wall hits (of the steps before the freeze) times obs_cost.

    The model's hits are taken on the exact states.  A fast state is within 37 steps x (half an ulp of a coordinate < 8 m
    plus the sincosf error of a step < 0.2 m) < 2e-5 m of the exact one, and the distance between two segments moves by no
    more than their endpoints do: a rollout whose wall verdicts all stay the same for half-widths 1e-4 m smaller and larger
    (a wall of half-width 0: no endpoint of the step or of the wall within 1e-4 m of the other segment),
    and whose goal tests are all 1e-4 m clear of the tolerance (five times the bound), has the same hits in both; the statement is made for those
    (most: asserted).  Every other rollout is held to a range: at the least the hits that stay with every half-width 1e-4 m
    smaller and the freeze as early as the goal tests allow, at the most those with every half-width 1e-4 m larger and the
    freeze as late as they allow.  Both costs are chains of at most 2T + 2 + hits float32-rounded additions of running values no larger
    than the cost with walls, each rounding at most half an ulp of that cost: the difference of the two chains is within
    (2T + 2 + hits) ulps of hits x obs_cost (hits: the walls' and the discs', the width of the range added)."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, 1.0)
    seg, hw = building(W)
    where, rad = discs_of(K, kind, t, params)
    if kind == "tracks":
        tracks, base = where, track_params(params, where, rad)
    else:
        tracks, base = where[:, None, :], problem_params(params, params["x0"], params["xgoal"], (where, rad))
    base["x0"], base["xgoal"] = params["x0"], params["xgoal"]
    p = oracle_params(without_walls(params))
    the_input_means_something(p, tracks, rad, seg, hw, noise, u_in)
    planner = MPPI_Numba(cfg_of(N, t, True, math="fast"))
    planner.set_params(base)
    absent, _, _, kernel_absent = rollout_with(planner, u_in, noise)
    planner.set_params(wall_params(base, seg, hw))
    present, _, _, kernel = rollout_with(planner, u_in, noise)
    assert "walls" not in kernel_absent and kernel.endswith(" walls=%d" % W) and "exact=0" in kernel, (kernel_absent, kernel)
    shape_of(kernel)
    disc_counts, st = hit_counts(p, tracks, rad, noise, u_in)
    walls = wall_hits_of_states(st, seg, hw)
    margin = np.float32(1e-4)
    thick = hw > 0
    fewest, most = np.zeros_like(walls), wall_hits_of_states(st, seg, hw + margin)  # per step, whatever the fast states are
    if thick.any():
        fewest += wall_hits_of_states(st, seg[thick], np.maximum(hw[thick] - margin, 0))
    if (~thick).any():  # half-width 0: segments that meet stop meeting only by way of an endpoint of one ON the other
        P, Q = st[:, :-1, None, :2], st[:, 1:, None, :2]
        A, B = seg[None, None, ~thick, 0], seg[None, None, ~thick, 1]
        touching = hit(P, P, A, B, margin) | hit(Q, Q, A, B, margin) | hit(P, Q, A, A, margin) | hit(P, Q, B, B, margin)
        fewest += (hit(P, Q, A, B, hw[~thick]) & ~touching).sum(axis=2)
    assert (fewest <= walls).all() and (walls <= most).all()
    # the freeze: the earliest and the latest step at which the fast states can have reached the goal
    tol = float(np.float32(params["goal_tolerance"]))
    goal_d = np.linalg.norm(st[:, 1:, :2].astype(np.float64) - np.float32(params["xgoal"]).astype(np.float64), axis=2)
    surely, maybe = goal_d <= tol - 1e-4, goal_d <= tol + 1e-4
    active_least = (np.cumsum(maybe, axis=1) - maybe) == 0    # frozen as early as can be
    active_most = (np.cumsum(surely, axis=1) - surely) == 0   # ... as late as can be
    active = active_steps(p, st)
    want_hits = (walls * active).sum(axis=1)
    lowest, highest = (fewest * active_least).sum(axis=1), (most * active_most).sum(axis=1)
    steady = lowest == highest
    assert (lowest <= want_hits).all() and (want_hits <= highest).all()
    assert steady.mean() >= 0.8, "bad input: only %.0f %% of the rollouts are clear of every boundary" % (100 * steady.mean())
    assert (want_hits[steady] > 0).any()
    diff = present.astype(np.float64) - absent.astype(np.float64)
    got_hits = np.rint(diff / OBS_PENALTY).astype(np.int64)
    print("fast math: %d of %d rollouts steady, wall hits up to %d, widest range %d" % (steady.sum(), N, want_hits.max(), (highest - lowest).max()))
    assert (got_hits[steady] == want_hits[steady]).all(), "%d rollouts differ in their hits" % (got_hits[steady] != want_hits[steady]).sum()
    assert ((lowest <= got_hits) & (got_hits <= highest)).all(), "rollouts %s are outside their range of hits" % np.nonzero((got_hits < lowest) | (got_hits > highest))[0]
    ops = 2 * t + 2 + got_hits + disc_counts.sum(axis=1) + (highest - lowest)
    bound = ops * np.spacing(present).astype(np.float64)
    assert (np.abs(diff - got_hits * OBS_PENALTY) <= bound).all()


def test_batch_with_shared_walls():
    """n = 64 per problem, not 200: a batched handle takes whole tiles only (mppi_planner_create refuses a per-problem
    rollout count that is not a multiple of 64), so a batch has no partial last tile; the single handles above have one."""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    counts = [0, 3, 90]
    B, n, t = len(counts), 64, 30
    rng = np.random.default_rng(17)
    x0s, goals = problems(rng, B)
    params = make_params(0.1, 1.0)
    sets = [crowd_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate(counts)]
    a = rng.uniform(-2.0, 5.0, (40, 2))
    seg = np.stack([a, a + rng.uniform(-1.5, 1.5, (40, 2))], axis=1).astype(np.float32)
    hw = rng.uniform(0.0, 0.2, 40).astype(np.float32)
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(wall_params(params, seg, hw), x0s, goals, obstacle_sets=sets)
    u_in = np.stack([inputs(rng, n, t)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    costs, u_out, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    shape_of(kernel)
    assert "problems=%d" % B in kernel and kernel.endswith(" walls=40"), kernel
    single = MPPI_Numba(cfg_of(n, t, True))
    for b in range(B):
        pb = problem_params(params, x0s[b], goals[b], sets[b])
        single.set_params(wall_params(pb, seg, hw))
        want, want_u, _, single_kernel = rollout_with(single, u_in[b], noise[b])
        assert single_kernel.startswith("k_rollout_barebone_crowd") and single_kernel.endswith(" walls=40"), single_kernel
        assert_bits(costs[b], want, "problem %d (%d discs) vs a single crowd handle" % (b, counts[b]))
        assert_bits(u_out[b], want_u, "problem %d u vs a single crowd handle" % b)
        p = oracle_params(pb)
        tracks = sets[b][0][:, None, :]
        _, st = hit_counts(p, tracks, sets[b][1], noise[b], u_in[b])
        assert (wall_hits_of_states(st, seg, hw) > 0).any(), "bad input: problem %d hits no wall" % b
        assert_bits(costs[b], wall_costs(p, tracks, sets[b][1], seg, hw, noise[b], u_in[b]), "problem %d vs the model" % b)


def test_solve_under_graph_replay_and_wall_changes():
    """shift_and_update_on_device is the batch's: n = 128 per problem, whole tiles as a batched handle requires."""
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t = 4, 128, 30
    rng = np.random.default_rng(9)
    x0s, goals = problems(rng, B)
    a = rng.uniform(-1.0, 4.0, (70, 2))
    seg = np.stack([a, a + rng.uniform(-1.0, 1.0, (70, 2))], axis=1).astype(np.float32)
    hw = rng.uniform(0.0, 0.15, 70).astype(np.float32)
    params = wall_params(make_params(0.1, 1.0, num_opt=5), seg, hw)
    direct, graphed, kept = (MPPI_Batch(cfg_of(n, t, True), B) for _ in range(3))
    for planner in (direct, graphed, kept):
        planner.setup(params, x0s, goals)
    graphed.set_graph_replay(True, 2)
    x = x0s.copy()

    def step_all():
        nonlocal x
        out = [planner.solve() for planner in (direct, graphed, kept)]
        x = x + np.float32([0.05, 0.04, 0.01])
        for planner in (direct, graphed, kept):
            planner.shift_and_update_on_device(x, num_shifts=1)
        return out

    for _ in range(4):
        a_, b_, c_ = step_all()
        np.testing.assert_array_equal(a_, b_)
        np.testing.assert_array_equal(a_, c_)
    kernel = graphed.last_rollout_kernel()
    assert kernel.startswith("k_rollout_barebone_crowd") and kernel.endswith(" walls=70"), kernel
    assert graphed.graph_stats()["replays"] >= 6, graphed.graph_stats()
    # the same arrays handed over again -- as new objects through the params, and straight to the library: nothing changes
    captures = graphed.graph_stats()["captures"]
    for planner in (direct, graphed):
        planner.params["wall_segments"], planner.params["wall_halfwidth"] = seg.copy(), hw.copy()
        flat = np.ascontiguousarray(seg.reshape(-1, 4))
        _lib.call("mppi_planner_set_walls", planner._handle, _lib.ptr(flat, C.c_float), _lib.ptr(hw, C.c_float), len(hw))
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    np.testing.assert_array_equal(a_, c_)
    assert graphed.graph_stats()["captures"] == captures, "the same walls again: no new capture"
    # other walls: another result, the same under replay and in the direct loop
    moved = seg + np.float32([0.3, -0.2])
    for planner in (direct, graphed):
        planner.params["wall_segments"] = moved
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    assert not np.array_equal(a_, c_), "other walls, the same controls"
    assert graphed.graph_stats()["captures"] > captures
    a_, b_, _ = step_all()
    np.testing.assert_array_equal(a_, b_)


def test_closed_loop_goes_round_the_wall():
    """A wall across the straight line from start to goal, 3 m long to one side and 0.8 m to the other.  The executed path:
    without walls it hits the wall (the model's `hit` on consecutive states), with walls it does not."""
    from mppi_numba_amd.barebone import MPPI_Numba
    n, t = 1024, 30
    centre = 2.0 * DIAG
    seg = np.float32([[centre - 3.0 * SIDE, centre + 0.8 * SIDE]])
    hw = np.float32([0.15])
    params = make_params(0.1, 1.0, num_opt=2)
    params["xgoal"] = np.array([3.0, 3.0])
    paths = {}
    for walls in (False, True):
        planner = MPPI_Numba(cfg_of(n, t, True, seed=5))
        planner.setup(wall_params(params, seg, hw) if walls else params)
        xhist, _, steps = planner.closed_loop(80)
        assert planner.last_rollout_kernel().endswith(" walls=1") == walls
        assert steps >= 1 and np.isfinite(xhist[:steps + 1]).all()
        path = xhist[:steps + 1, :2].astype(np.float32)
        paths[walls] = hit(path[:-1], path[1:], seg[:, 0], seg[:, 1], hw)
        print("closed loop, walls %d: %d steps, %d of them hit the wall" % (walls, steps, paths[walls].sum()))
    assert paths[False].any(), "bad input: the path without walls does not meet the wall"
    assert not paths[True].any(), "the executed path hits the wall at steps %s" % np.nonzero(paths[True])[0]


def test_mode_handling():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Numba
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    n, t = 128, 30
    seg, hw = building(6)
    params = make_params(0.1, 1.0)
    planner = MPPI_Numba(cfg_of(n, t, False))
    planner.setup(params)
    assert np.isfinite(planner.solve()).all()
    plain = planner.last_rollout_kernel()
    assert plain.startswith("k_rollout_barebone exact"), plain
    planner.set_params(wall_params(params, seg, hw))
    with pytest.raises(_lib.MppiError) as err:  # no crowd mode: no walls
        planner.solve()
    assert err.value.code == ERR_INVALID and "crowd" in str(err.value), str(err.value)
    planner.set_crowd(True)
    assert np.isfinite(planner.solve()).all()
    kernel = planner.last_rollout_kernel()
    shape_of(kernel)
    assert kernel.endswith(" walls=6"), kernel
    with pytest.raises(_lib.MppiError) as err:  # the walls hold the handle in crowd mode
        planner.set_crowd(False)
    assert err.value.code == ERR_INVALID and "walls" in str(err.value), str(err.value)
    assert planner.crowd
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == kernel
    bad = hw.copy()
    bad[2] = -0.1
    planner.set_params(wall_params(params, seg, bad))
    with pytest.raises(_lib.MppiError) as err:
        planner.solve()
    assert err.value.code == ERR_INVALID and "half-width" in str(err.value), str(err.value)
    for value in (np.nan, np.inf):
        broken = seg.copy()
        broken[1, 0, 1] = value
        planner.set_params(wall_params(params, broken, hw))
        with pytest.raises(_lib.MppiError) as err:
            planner.solve()
        assert err.value.code == ERR_INVALID and "finite" in str(err.value), str(err.value)
    assert planner.last_rollout_kernel() == kernel  # (refused: the handle keeps the walls it had)
    planner.set_params(params)  # the keys have gone: count = 0 clears the walls ...
    assert np.isfinite(planner.solve()).all()
    assert planner.last_rollout_kernel() == plain  # ... and the launch is the one without walls again (no discs: default form)
    planner.set_crowd(False)  # ... and crowd mode can go
    assert not planner.crowd
    # a map mode has no walls
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    lib = _lib.load()
    flat = np.ascontiguousarray(seg.reshape(-1, 4))
    assert lib.mppi_planner_set_walls(mapped._handle, _lib.ptr(flat, C.c_float), _lib.ptr(hw, C.c_float), len(hw)) == ERR_INVALID
    assert "barebone" in lib.mppi_last_error().decode()
