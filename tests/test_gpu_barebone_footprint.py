"""A body footprint for the barebone planner in crowd mode (params['footprint'], mppi_planner_set_footprint): the robot as up
to eight discs rigidly attached to its pose, so that the heading counts in the hit tests.  The footprint forms of
k_rollout_barebone_crowd count, per step, the obstacles ANY body disc touches; every comparison of costs with
tests/footprint_model.py is bit for bit (tests/test_footprint_model.py shows on the CPU that these inputs allow it: no centre
is within 1e-15 of sine and cosine of a rounding boundary)."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import disc_samples_model
import footprint_model as fm
from test_footprint_model import EIGHT, dyadic
from test_gpu_barebone_batch import ERR_INVALID, assert_bits, make_params, oracle_params, problem_params, problems
from test_gpu_barebone_crowd import cfg_of, inputs, shape_of
from test_gpu_barebone_disc_samples import sample_params, sample_set, sampled_rollout
from test_gpu_barebone_goal_tracks import crossing_goal, goal_params
from test_gpu_barebone_tracks import moving_tracks, rollout_with, track_params
from test_gpu_barebone_wall_tracks import moving_building, track_wall_params
from test_gpu_barebone_walls import N, building, discs_of, task, wall_params, without_walls
from crowd_model import crowd_discs
from wall_model import states, wall_costs

pytestmark = pytest.mark.gpu

FOOTPRINTS = {1: EIGHT[5:6], 3: EIGHT[[0, 5, 6]], 8: EIGHT}  # (F = 1: one disc off the axis, so that the heading counts)
TASKS = ((30, 1.0), (37, 1.5))  # more than one chunk, not a multiple of the counters; rotation on, off


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


def body_params(params, footprint):
    p = dict(params)
    p["footprint"] = footprint
    return p


def without_body(params):
    return {k: v for k, v in params.items() if k != "footprint"}


def scene_params(params, K, W, kind, t):
    """params with K discs (static, or tracks of t + 1 rows) and W static walls; plus the model's view of them."""
    where, rad = discs_of(K, kind, t, params)
    if kind == "tracks":
        tracks, full = where, track_params(params, where, rad)
    else:
        tracks, full = where[:, None, :], problem_params(params, params["x0"], params["xgoal"], (where, rad))
    full["x0"], full["xgoal"] = params["x0"], params["xgoal"]
    seg = hw = None
    if W:
        seg, hw = building(W)
        full = wall_params(full, seg, hw)
    return full, tracks, rad, seg, hw


def check_kernel(kernel, F, t, wscale, exact=True):
    chunk = shape_of(kernel)[1]
    assert t > chunk, kernel
    assert kernel.endswith(" footprint=%d" % F), kernel
    assert ("rotation=1" in kernel) == (exact and wscale == 1.0) and ("exact=%d" % exact) in kernel, kernel


# ---- 1. costs against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,K,W,t,wscale", [(F, K, W, t, wscale) for F in (1, 3, 8) for K in (0, 3, 70) for W in (0, 1, 65)
                                            for t, wscale in TASKS])
def test_costs_equal_the_model(F, K, W, t, wscale):
    """Static discs, then tracks at offsets 0 and 5, on one handle.  K = 70: two disc tiles; W = 65: two wall tiles."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, wscale)
    p = oracle_params(without_walls(params))
    fp = FOOTPRINTS[F]
    planner = MPPI_Numba(cfg_of(N, t, True))
    differs = False
    for kind in ("static", "tracks"):
        full, tracks, rad, seg, hw = scene_params(params, K, W, kind, t)
        planner.set_params(body_params(full, fp))
        for offset in ((0, 5) if kind == "tracks" else (0,)):
            model = fm.costs(p, fp, tracks, rad, seg, hw, noise, u_in, offset)
            planner.move_mppi_task_vars_to_device()  # (hands the tracks over the first time: offset 0)
            planner.set_track_offset(offset)
            got, _, _, kernel = rollout_with(planner, u_in, noise)
            check_kernel(kernel, F, t, wscale)
            assert ("tracks=%d" % (t + 1) in kernel) == (kind == "tracks"), kernel
            assert (" walls=%d" % W in kernel) == (W > 0), kernel
            assert_bits(got, model, "F = %d, %d discs (%s, offset %d), %d walls vs the model" % (F, K, kind, offset, W))
            if K or W:
                point = wall_costs(p, tracks, rad, seg if W else np.zeros((0, 2, 2), np.float32), hw if W else np.zeros(0, np.float32),
                                   noise, u_in, offset)
                differs = differs or (point.view(np.int32) != model.view(np.int32)).any()
    assert differs == bool(K or W), "bad input: the body costs what the reference point costs"


@pytest.mark.parametrize("t,wscale", TASKS)
def test_wall_tracks_equal_the_model(t, wscale):
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, wscale)
    p = oracle_params(without_walls(params))
    where, rad = discs_of(70, "tracks", t, params)
    wtracks, hw = moving_building(65, t + 1)
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.set_params(body_params(track_wall_params(track_params(params, where, rad), wtracks, hw), EIGHT))
    for offset in (0, 5):
        model = fm.costs(p, EIGHT, where, rad, wtracks, hw, noise, u_in, offset)
        assert (model != fm.costs(p, EIGHT, where, rad, wtracks[:, 0], hw, noise, u_in, offset)).any(), "bad input: the rows cannot be told apart"
        planner.move_mppi_task_vars_to_device()
        planner.set_track_offset(offset)
        got, _, _, kernel = rollout_with(planner, u_in, noise)
        check_kernel(kernel, 8, t, wscale)
        assert " walls=65 wall_rows=%d" % (t + 1) in kernel, kernel
        assert_bits(got, model, "wall tracks at offset %d vs the model" % offset)


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("W", [0, 65])
def test_disc_samples_equal_the_model(alpha, W):
    """S = 3 samples of 70 discs: each sample's count is the body's against that sample's discs, the walls counted once."""
    from mppi_numba_amd.barebone import MPPI_Numba
    t, S = 37, 3
    params, u_in, noise = task(t, 1.0)
    p = oracle_params(without_walls(params))
    smp, rad = sample_set(70, S)
    seg, hw = building(W) if W else (None, None)
    per = fm.sample_costs(p, EIGHT, smp, rad, seg, hw, noise, u_in)
    assert (np.ptp(per, axis=1) > 0).any(), "bad input: every rollout costs the same under every sample"
    full = sample_params(params, smp, rad, alpha)
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.set_params(body_params(wall_params(full, seg, hw) if W else full, EIGHT))
    costs, got_per, _, kernel = sampled_rollout(planner, u_in, noise)
    check_kernel(kernel, 8, t, 1.0)
    assert " samples=%d numel=%d footprint=8" % (S, disc_samples_model.cvar_numel(S, alpha)) in kernel, kernel
    assert_bits(got_per, per, "per-sample costs vs the model")
    assert_bits(costs, disc_samples_model.cvar_tail(per, alpha), "the tail over the model's costs")


def test_a_goal_track_beside_the_footprint():
    from mppi_numba_amd.barebone import MPPI_Numba
    t, wscale = 37, 1.0
    params, u_in, noise = task(t, wscale)
    track = crossing_goal(t, t + 1)
    p = oracle_params(dict(without_walls(params), xgoal=track[0]))
    fp = FOOTPRINTS[3]
    full, tracks, rad, seg, hw = scene_params(params, 3, 1, "static", t)
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.set_params(body_params(goal_params(full, track), fp))
    got, _, _, kernel = rollout_with(planner, u_in, noise)
    check_kernel(kernel, 3, t, wscale)
    assert " goal_rows=%d" % (t + 1) in kernel, kernel
    model = fm.costs(p, fp, tracks, rad, seg, hw, noise, u_in, goal_track=track)
    assert (model != fm.costs(p, fp, tracks, rad, seg, hw, noise, u_in, goal_track=track[:1])).any(), "bad input: the goal's rows cannot be told apart"
    assert_bits(got, model, "a goal track beside the footprint vs the model")


# ---- 2. the three equalities, handle against handle ----------------------------------------------------------------------
@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("t,wscale", TASKS)
def test_the_equalities_of_the_definition(math, t, wscale):
    """[[0, 0, 0]] is the point launch; [[0, 0, rho]] is the point launch with radii r + rho and half-widths h + rho (dyadic
    values: the float32 sums are exact); a row repeated is the row once.  In fast math the states are the fast ones in both
    handles: the formula is the same."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, wscale)
    full, tracks, rad, seg, hw = scene_params(params, 70, 65, "static", t)
    rad, hw, rho = dyadic(rad), dyadic(hw), np.float32(5.0 / 64)
    full["obstacle_radius"], full["wall_halfwidth"] = rad, hw
    body, point = MPPI_Numba(cfg_of(N, t, True, math)), MPPI_Numba(cfg_of(N, t, True, math))
    exact = math == "exact"

    def run(planner, p):
        planner.set_params(p)
        return rollout_with(planner, u_in, noise)

    want, want_u, _, point_kernel = run(point, full)
    assert "footprint" not in point_kernel and point_kernel.endswith(" walls=65"), point_kernel
    got, got_u, _, kernel = run(body, body_params(full, [[0, 0, 0]]))
    check_kernel(kernel, 1, t, wscale, exact)
    assert_bits(got, want, "%s math: [[0, 0, 0]] vs the point launch" % math)
    assert_bits(got_u, want_u, "... and the update")
    larger = dict(full)
    larger["obstacle_radius"], larger["wall_halfwidth"] = rad + rho, hw + rho
    want_rho = run(point, larger)[0]
    assert (want_rho != want).any(), "bad input: rho changes nothing"
    assert_bits(run(body, body_params(full, [[0, 0, rho]]))[0], want_rho, "%s math: [[0, 0, rho]] vs the point launch with larger obstacles" % math)
    once, _, _, kernel = run(body, body_params(full, EIGHT[[0, 5]]))
    check_kernel(kernel, 2, t, wscale, exact)
    assert (once != want).any(), "bad input: the body costs what the point costs"
    twice, _, _, kernel = run(body, body_params(full, EIGHT[[0, 5, 0, 0, 5]]))
    check_kernel(kernel, 5, t, wscale, exact)
    assert_bits(twice, once, "%s math: a row repeated vs the row once" % math)
    if exact:
        p = oracle_params(without_walls(params))
        assert_bits(once, fm.costs(p, EIGHT[[0, 5]], tracks, rad, seg, hw, noise, u_in), "two rows vs the model")


# ---- 3. a batch ----------------------------------------------------------------------------------------------------------
def test_batch_with_per_problem_discs_and_walls():
    """B = 3 problems of n = 64 (a batched handle takes whole tiles), each with its own disc set and wall set, one footprint:
    problem b equals a single planner bit for bit, and the model."""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    counts, wcounts = [0, 3, 90], [70, 0, 5]
    B, n, t = len(counts), 64, 30
    rng = np.random.default_rng(23)
    x0s, goals = problems(rng, B)
    params = make_params(0.1, 1.0)
    sets = [crowd_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate(counts)]
    wall_sets = []
    for b, w in enumerate(wcounts):
        a = x0s[b, :2] + rng.uniform(-1.0, 4.0, (w, 2))
        wall_sets.append((np.stack([a, a + rng.uniform(-1.5, 1.5, (w, 2))], axis=1).astype(np.float32).reshape(w, 2, 2),
                          rng.uniform(0.0, 0.2, w).astype(np.float32)))
    fp = FOOTPRINTS[3]
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(body_params(params, fp), x0s, goals, obstacle_sets=sets, wall_sets=wall_sets)
    u_in = np.stack([inputs(rng, n, t)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    costs, u_out, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    shape_of(kernel)
    assert "problems=%d" % B in kernel and kernel.endswith(" footprint=3"), kernel
    single = MPPI_Numba(cfg_of(n, t, True))
    for b in range(B):
        pb = problem_params(params, x0s[b], goals[b], sets[b])
        seg, hw = wall_sets[b]
        single.set_params(body_params(wall_params(pb, seg, hw) if len(hw) else pb, fp))
        want, want_u, _, single_kernel = rollout_with(single, u_in[b], noise[b])
        assert single_kernel.endswith(" footprint=3") and "problems" not in single_kernel, single_kernel
        assert_bits(costs[b], want, "problem %d (%d discs, %d walls) vs a single handle" % (b, counts[b], wcounts[b]))
        assert_bits(u_out[b], want_u, "problem %d u vs a single handle" % b)
        model = fm.costs(oracle_params(pb), fp, sets[b][0][:, None, :], sets[b][1], seg if len(hw) else None, hw, noise[b], u_in[b])
        assert_bits(costs[b], model, "problem %d vs the model" % b)


# ---- 4. the key comes and goes -------------------------------------------------------------------------------------------
def test_clearing_the_key_restores_the_point_launch():
    from mppi_numba_amd.barebone import MPPI_Numba
    t, wscale = 37, 1.0
    params, u_in, noise = task(t, wscale)
    full = scene_params(params, 70, 65, "static", t)[0]
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.set_params(full)
    before, before_u, _, before_kernel = rollout_with(planner, u_in, noise)
    assert planner.footprint is None
    planner.set_params(body_params(full, EIGHT))
    held, _, _, kernel = rollout_with(planner, u_in, noise)
    check_kernel(kernel, 8, t, wscale)
    np.testing.assert_array_equal(planner.footprint, EIGHT)
    assert (held != before).any()
    planner.set_params(full)
    after, after_u, _, after_kernel = rollout_with(planner, u_in, noise)
    assert after_kernel == before_kernel and "footprint" not in after_kernel, (before_kernel, after_kernel)
    assert planner.footprint is None
    assert_bits(after, before, "the key has gone: the point launch's costs")
    assert_bits(after_u, before_u, "... and its update")
    # no discs, no walls: a footprint still launches the crowd kernel; without it the default form is back
    bare = MPPI_Numba(cfg_of(N, t, True))
    bare.set_params(body_params(params, EIGHT[:3]))
    alone, _, _, kernel = rollout_with(bare, u_in, noise)
    check_kernel(kernel, 3, t, wscale)
    bare.set_params(params)
    plain, _, _, plain_kernel = rollout_with(bare, u_in, noise)
    assert plain_kernel.startswith("k_rollout_barebone exact"), plain_kernel
    assert_bits(alone, plain, "nothing to hit: the costs of the default form")


def test_error_paths():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    n, t = 128, 30
    params = make_params(0.1, 1.0)
    lib = _lib.load()

    def raw(planner, rows):
        rows = np.ascontiguousarray(rows, np.float32)
        return lib.mppi_planner_set_footprint(planner._handle, _lib.ptr(rows, C.c_float), len(rows))

    planner = MPPI_Numba(cfg_of(n, t, False))
    planner.setup(params)
    assert np.isfinite(planner.solve()).all()
    plain = planner.last_rollout_kernel()
    planner.set_params(body_params(params, EIGHT[:3]))
    with pytest.raises(_lib.MppiError) as err:  # no crowd mode: no footprint
        planner.solve()
    assert err.value.code == ERR_INVALID and "crowd" in str(err.value), str(err.value)
    assert planner.footprint is None
    planner.set_crowd(True)
    assert np.isfinite(planner.solve()).all()
    kernel = planner.last_rollout_kernel()
    assert kernel.startswith("k_rollout_barebone_crowd") and kernel.endswith(" footprint=3"), kernel
    with pytest.raises(_lib.MppiError) as err:  # the footprint holds the handle in crowd mode
        planner.set_crowd(False)
    assert err.value.code == ERR_INVALID and "footprint" in str(err.value), str(err.value)
    assert planner.crowd
    for bad in (np.zeros((9, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((3, 2), np.float32), np.zeros(3, np.float32)):
        planner.set_params(body_params(params, bad))
        with pytest.raises(ValueError):  # F = 9, F = 0, a wrong shape
            planner.solve()
    assert raw(planner, np.zeros((9, 3))) == ERR_INVALID and "9" in lib.mppi_last_error().decode()
    negative = EIGHT[:3].copy()
    negative[1, 2] = -0.1
    planner.set_params(body_params(params, negative))
    with pytest.raises(_lib.MppiError) as err:
        planner.solve()
    assert err.value.code == ERR_INVALID and "negative" in str(err.value), str(err.value)
    for value in (np.nan, np.inf):
        broken = EIGHT[:3].copy()
        broken[2, 0] = value
        planner.set_params(body_params(params, broken))
        with pytest.raises(_lib.MppiError) as err:
            planner.solve()
        assert err.value.code == ERR_INVALID and "finite" in str(err.value), str(err.value)
    np.testing.assert_array_equal(planner.footprint, EIGHT[:3])  # (refused: the handle keeps what it had)
    planner.set_params(params)  # the key has gone ...
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == plain
    planner.set_crowd(False)  # ... and crowd mode can go
    # the fleet, both ways: in Python and at the C ABI
    B = 2
    rng = np.random.default_rng(5)
    x0s, goals = problems(rng, B)
    batch = MPPI_Batch(cfg_of(64, t, True), B)
    batch.setup(body_params(params, EIGHT[:3]), x0s, goals)
    assert np.isfinite(batch.solve()).all() and batch.last_rollout_kernel().endswith(" footprint=3")
    with pytest.raises(ValueError) as verr:
        batch.set_fleet(0.2, 0.05)
    assert "footprint" in str(verr.value)
    half = np.full((B, B - 1), 0.45, np.float32)
    assert lib.mppi_planner_set_fleet(batch._handle, B, _lib.ptr(half, C.c_float)) == ERR_INVALID
    assert "footprint" in lib.mppi_last_error().decode()
    assert batch.fleet is None
    batch.set_params(without_body(batch.params))
    batch.set_fleet(0.2, 0.05)
    assert np.isfinite(batch.solve()).all() and "fleet=%d" % B in batch.last_rollout_kernel()
    batch.set_params(body_params(batch.params, EIGHT[:3]))
    with pytest.raises(ValueError) as verr:
        batch.solve()
    assert "fleet" in str(verr.value)
    assert raw(batch, EIGHT[:3]) == ERR_INVALID and "fleet" in lib.mppi_last_error().decode()
    assert batch.footprint is None
    # a map mode has no footprint
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    assert raw(mapped, EIGHT[:3]) == ERR_INVALID and "barebone" in lib.mppi_last_error().decode()


# ---- 5. graph replay -----------------------------------------------------------------------------------------------------
def test_graph_replay_and_a_changed_footprint():
    """The footprint's rows are by-value arguments of the captured launches: a changed footprint must not replay them."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t = 4, 128, 30
    rng = np.random.default_rng(9)
    x0s, goals = problems(rng, B)
    a = rng.uniform(-1.0, 4.0, (70, 2))
    seg = np.stack([a, a + rng.uniform(-1.0, 1.0, (70, 2))], axis=1).astype(np.float32)
    hw = rng.uniform(0.0, 0.15, 70).astype(np.float32)
    params = body_params(wall_params(make_params(0.1, 1.0, num_opt=5), seg, hw), EIGHT[:3])
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

    for _ in range(3):
        a_, b_, c_ = step_all()
        np.testing.assert_array_equal(a_, b_)
        np.testing.assert_array_equal(a_, c_)
    kernel = graphed.last_rollout_kernel()
    assert kernel.startswith("k_rollout_barebone_crowd") and kernel.endswith(" walls=70 footprint=3"), kernel
    assert graphed.graph_stats()["replays"] >= 4, graphed.graph_stats()
    captures = graphed.graph_stats()["captures"]
    for planner in (direct, graphed):  # the same rows as a new object: nothing changes
        planner.params["footprint"] = EIGHT[:3].copy()
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    np.testing.assert_array_equal(a_, c_)
    assert graphed.graph_stats()["captures"] == captures, "the same footprint again: no new capture"
    wider = EIGHT[:3].copy()  # the same count, other rows: only the by-value argument differs
    wider[:, 2] += np.float32(0.2)
    wider[1, 1] = np.float32(-0.4)
    for planner in (direct, graphed):
        planner.params["footprint"] = wider
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    assert not np.array_equal(a_, c_), "another footprint, the same controls"
    assert graphed.graph_stats()["captures"] > captures
    a_, b_, _ = step_all()
    np.testing.assert_array_equal(a_, b_)


# ---- 6. the doorway ------------------------------------------------------------------------------------------------------
CART = (0.5, 0.5, 0.4)      # front, rear, width: 1.0 m long, 0.4 m wide; circumscribed radius 0.54 m
GAP = 0.7
DOOR_X = 1.5
DOOR = np.float32([[[DOOR_X, -3.0], [DOOR_X, -GAP / 2]], [[DOOR_X, GAP / 2], [DOOR_X, 3.0]]])  # a wall across the way, half-width 0


def doorway_params(num_opt=1):
    params = make_params(0.1, 1.0, num_opt=num_opt)
    params["x0"], params["xgoal"] = np.array([0.0, 0.0, 0.0]), np.array([3.5, 0.0])
    params["vrange"] = np.array([0.0, 1.8])
    return wall_params(params, DOOR, np.float32(0.0))


@functools.lru_cache(maxsize=None)
def doorway_inputs():
    rng = np.random.default_rng(77)
    t = 30
    u = np.stack([np.full(t, 1.2), np.zeros(t)], 1).astype(np.float32)
    noise = np.stack([rng.normal(0, 0.3, (N, t)), rng.normal(0, 0.6, (N, t))], axis=2).astype(np.float32)
    return t, u, noise


def test_the_doorway_at_rollout_level():
    """With the model: every rollout whose reference point passes the gap is hit when the robot is its circumscribed disc
    (the single row (0, 0, 0.54)), and some pass unhit as the cart -- the launch gives the model's bits for both."""
    from mppi_numba_amd.barebone import MPPI_Numba, rectangle_footprint
    t, u_in, noise = doorway_inputs()
    params = doorway_params()
    cart = rectangle_footprint(*CART)
    assert cart.shape == (3, 3)
    disc = np.float32([[0.0, 0.0, 0.54]])
    p = oracle_params(without_walls(params))
    st = states(p, noise, u_in)
    none, no_r = np.zeros((0, 1, 2), np.float32), np.zeros(0, np.float32)
    before, after = st[:, :-1, 0] < DOOR_X, st[:, 1:, 0] >= DOOR_X
    inside = np.abs(st[:, :-1, 1]) < GAP / 2 - 0.02
    point_hits = fm.footprint_hits(st, [[0, 0, 0]], none, no_r, DOOR, 0.0)[1].sum(axis=1)
    passes = (before & after & inside).any(axis=1) & (point_hits == 0)  # the reference point goes through the gap
    hits_disc = fm.footprint_hits(st, disc, none, no_r, DOOR, 0.0)[1].sum(axis=1)
    hits_cart = fm.footprint_hits(st, cart, none, no_r, DOOR, 0.0)[1].sum(axis=1)
    print("doorway: %d of %d rollouts pass the gap; as a disc %d of them are hit, as the cart %d" % (
        passes.sum(), N, (hits_disc[passes] > 0).sum(), (hits_cart[passes] > 0).sum()))
    assert passes.sum() >= 10, "bad input: hardly a rollout passes the gap"
    assert (hits_disc[passes] > 0).all(), "a rollout passes a 0.7 m gap as a disc of radius 0.54 m"
    assert (hits_cart[passes] == 0).any(), "no rollout passes the gap unhit as the cart"
    planner = MPPI_Numba(cfg_of(N, t, True))
    for fp in (disc, cart):
        planner.set_params(body_params(params, fp))
        got, _, _, kernel = rollout_with(planner, u_in, noise)
        assert kernel.endswith(" walls=2 footprint=%d" % len(fp)), kernel
        assert_bits(got, fm.costs(p, fp, none, no_r, DOOR, 0.0, noise, u_in), "the doorway, F = %d, vs the model" % len(fp))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_closed_loop_through_the_doorway(seed):
    """The cart reaches the goal behind the doorway, and the rectangle's true float64 clearance from the wall along the
    executed states is not negative."""
    from mppi_numba_amd.barebone import MPPI_Numba, rectangle_footprint
    n, t = 1024, 30
    params = body_params(doorway_params(num_opt=2), rectangle_footprint(*CART))
    planner = MPPI_Numba(cfg_of(n, t, True, seed=seed))
    planner.setup(params)
    xhist, _, steps = planner.closed_loop(120)
    assert planner.last_rollout_kernel().endswith(" walls=2 footprint=3")
    path = xhist[:steps + 1]
    assert np.isfinite(path).all()
    clearance = fm.rectangle_clearance(path, *CART, DOOR)
    print("closed loop through the doorway, seed %d: %d steps, ends %.3f m from the goal, clearance %.4f m (at step %d, x = %.3f)" % (
        seed, steps, np.linalg.norm(path[-1, :2] - params["xgoal"]), clearance.min(), clearance.argmin(), path[clearance.argmin(), 0]))
    assert np.linalg.norm(path[-1, :2] - params["xgoal"]) <= params["goal_tolerance"], "the goal is not reached"
    assert path[0, 0] < DOOR_X < path[-1, 0]
    assert clearance.min() >= 0.0, "the rectangle meets the wall at step %d" % clearance.argmin()
