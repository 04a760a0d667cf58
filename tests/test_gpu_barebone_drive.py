"""Car-like steering in the barebone planner (params['drive'] = 'car', mppi_planner_set_drive): the second control is the
path curvature kappa and a step turns by dt * fl(v * kappa).  Everything downstream of the pose is untouched, so the suite's
cost models serve as they stand: they take their states from oracle.state_rollout_barebone, looked up on the module when
they are called, and the `car` fixture puts tests/car_model.py's state_rollout there (equal to the oracle bit for bit with
car=False: tests/test_car_model.py).  Costs are compared to the bit, in exact math.

The standard task (dt = 0.1, vrange (0, 2), wrange +-pi * wscale) bounds the heading increment of a car by 0.628 rad at
wscale 1.0 -- no (cos, sin) by rotation, which the unicycle has there at 0.314 -- and by 0.314 rad at wscale 0.5: the tests
stand on both sides of the host's 0.36 rad."""
import ctypes as C
import gc

import numpy as np
import pytest

import car_model
import clearance_model
import fleet_body_model
import fleet_model
import footprint_model
import occupancy_model
from crowd_model import crowd_costs, crowd_discs, hit_counts
from oracle import oracle as O
from test_gpu_barebone_batch import ERR_INVALID, assert_bits, make_cfg, make_params, oracle_params, problem_params, problems
from test_gpu_barebone_crowd import cfg_of, inputs, shape_of
from test_gpu_barebone_tracks import rollout_with
from track_model import track_costs

pytestmark = pytest.mark.gpu

DT = 0.1
SHAPES = [(63, 7), (64, 8), (65, 9), (130, 17), (128, 30)]  # below, at, above a tile; below, at, past the eight-step batch, and a tail
WSCALES = [1.0, 0.5]  # dt * max|v| * max|kappa| = 0.628 (no rotation) and 0.314 (rotation)


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


@pytest.fixture
def car(monkeypatch):
    """The models' states are the car's from here on (until the test ends)."""
    monkeypatch.setattr(O, "state_rollout_barebone", car_model.state_rollout)


def car_params(params):
    return dict(params, drive="car")


def scene(n, t, K, wscale, goal=None):
    """The standard task with K discs of crowd_model.crowd_discs, the first three on top of each other; at a horizon too
    short to reach them where crowd_discs puts them (T < 30) they lie 0.14 * T m ahead of the start -- within 0.15 * T m --,
    along its heading.  Controls and noise of test_gpu_barebone_crowd.inputs, seed n * 100 + t, with three entries outside
    vrange / wrange so that both clips take part: a step at rest, a step at either end of the curvature range."""
    rng = np.random.default_rng(n * 100 + t)
    params = make_params(DT, wscale)
    if goal is not None:
        params["xgoal"] = np.asarray(goal, np.float64)
    pos, rad = crowd_discs(rng, K, params["x0"], params["xgoal"])
    if t < 30:
        m = min(3, K)
        th0 = params["x0"][2]
        pos[:m] = (params["x0"][:2] + 0.14 * t * np.array([np.cos(th0), np.sin(th0)]) + rng.normal(0, 0.05, (m, 2))).astype(np.float32)
    params["obstacle_positions"], params["obstacle_radius"] = pos, rad
    u_in, noise = inputs(rng, n, t)
    u_in[0, 0], u_in[1, 1], u_in[2, 1] = -3.0, 40.0, -40.0
    return params, pos, rad, u_in, noise


def the_input_means_something(p, pos, rad, noise, u_in):
    """Asserted on the model's (car) states before anything is compared."""
    counts, st = hit_counts(p, pos[:, None], rad, noise, u_in)
    hit, twice = int((counts > 0).any(axis=1).sum()), int((counts >= 2).any(axis=1).sum())
    print("rollouts with a hit: %d, inside two discs at one step: %d of %d" % (hit, twice, len(noise)))
    assert hit >= 1, "bad input: no rollout is inside a disc"
    assert twice >= 1, "bad input: no rollout is inside two discs at one step"
    return st


def check_name(kernel, wscale, family, exact=True):
    assert kernel.startswith(family), kernel
    assert ("rotation=%d" % (1 if exact and wscale == 0.5 else 0)) in kernel and ("exact=%d" % exact) in kernel, kernel
    assert kernel.endswith(" drive=car") and kernel.count("drive") == 1, kernel


# ---- 1. the default family --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("wscale", WSCALES)
@pytest.mark.parametrize("n,t", SHAPES)
def test_default_family_costs_equal_the_model(car, n, t, wscale, K):
    """K = 2, 3, 5: the discs<=2, discs<=4 and loop forms under rotation."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, pos, rad, u_in, noise = scene(n, t, K, wscale)
    p = oracle_params(params)
    the_input_means_something(p, pos, rad, noise, u_in)
    model = track_costs(p, pos[:, None], rad, noise, u_in)
    planner = MPPI_Numba(cfg_of(n, t, False))
    planner.set_params(car_params(params))
    got, _, _, kernel = rollout_with(planner, u_in, noise)
    check_name(kernel, wscale, "k_rollout_barebone exact")
    assert planner.drive == "car"
    assert_bits(got, model, "(%d, %d), %d discs, wscale %.1f vs the track model on car states" % (n, t, K, wscale))


# ---- 2. the crowd family ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wscale", WSCALES)
@pytest.mark.parametrize("n,t", [(130, 17), (128, 30), (128, 37)])
def test_crowd_family_costs_equal_the_model(car, n, t, wscale):
    from mppi_numba_amd.barebone import MPPI_Numba
    params, pos, rad, u_in, noise = scene(n, t, 7, wscale)
    p = oracle_params(params)
    the_input_means_something(p, pos, rad, noise, u_in)
    model = crowd_costs(p, pos[:, None], rad, noise, u_in)
    planner = MPPI_Numba(cfg_of(n, t, True))
    planner.set_params(car_params(params))
    got, _, _, kernel = rollout_with(planner, u_in, noise)
    shape_of(kernel)
    check_name(kernel, wscale, "k_rollout_barebone_crowd")
    assert_bits(got, model, "(%d, %d), 7 discs, wscale %.1f vs the crowd model on car states" % (n, t, wscale))


GOAL = (2.2, 2.2)  # (within reach of the horizon: the goal test and the freeze take part)


@pytest.mark.parametrize("kind", ["walls+footprint", "rings", "occupancy"])
def test_crowd_forms_equal_their_models(car, kind):
    """(128, 30), 7 discs and: five walls under a body of three discs; two clearance rings; an occupancy grid tested at two
    points a step."""
    from mppi_numba_amd.barebone import MPPI_Numba
    from clearance_cases import RINGS
    from occupancy_cases import grid_over, occupancy_params
    from test_footprint_model import EIGHT
    from test_gpu_barebone_walls import building
    n, t, wscale = 128, 30, 0.5
    params, pos, rad, u_in, noise = scene(n, t, 7, wscale, GOAL)
    params["vrange"] = np.array([0.0, 1.8])  # (steps of up to 0.18 m: the thin wall of building() is jumped)
    p = oracle_params(params)
    st = the_input_means_something(p, pos, rad, noise, u_in)
    tracks = pos[:, None]
    if kind == "walls+footprint":
        fp = EIGHT[[0, 5, 6]]
        seg, hw = building(5)
        full = dict(params, wall_segments=seg, wall_halfwidth=hw, footprint=fp)
        discs, walls = footprint_model.footprint_hits(st, fp, tracks, rad, seg, hw)
        assert (walls > 0).any() and (discs > 0).any(), "bad input: the body touches no wall (or no disc)"
        model = footprint_model.costs(p, fp, tracks, rad, seg, hw, noise, u_in)
        ending = " walls=5 footprint=3 drive=car"
    elif kind == "rings":
        rings = RINGS[2]
        full = dict(params, clearance_rings=rings)
        near = clearance_model.ring_counts(st, rings, tracks, rad, None, None)
        assert (near > 0).any(), "bad input: no step is near at a ring"
        model = clearance_model.costs(p, rings, tracks, rad, None, None, noise, u_in)
        ending = " rings=2 drive=car"
    else:
        grid = grid_over(st, 23, inflate=0.25, substeps=2)
        full = occupancy_params(params, grid)
        bits, inside = occupancy_model.level_bits(grid, st, [0.0], None)
        assert bits[0].any() and not bits[0].all() and inside.any(), "bad input: the grid is hit nowhere (or everywhere)"
        model = occupancy_model.costs(p, grid, None, tracks, rad, None, None, noise, u_in)
        ending = " grid=%dx%d drive=car" % (grid.nx, grid.ny)
    planner = MPPI_Numba(cfg_of(n, t, True))
    planner.set_params(car_params(full))
    got, _, _, kernel = rollout_with(planner, u_in, noise)
    shape_of(kernel)
    check_name(kernel, wscale, "k_rollout_barebone_crowd")
    assert kernel.endswith(ending), kernel
    assert_bits(got, model, "%s vs its model on car states" % kind)


# ---- 3. crowd on equals crowd off -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("wscale", WSCALES)
def test_crowd_on_equals_crowd_off(math, wscale):
    """The same operations on the same operands -- for fast math the only statement made."""
    from mppi_numba_amd.barebone import MPPI_Numba
    n, t = 128, 30
    params, pos, rad, u_in, noise = scene(n, t, 7, wscale)
    results = {}
    for crowd in (False, True):
        planner = MPPI_Numba(cfg_of(n, t, crowd, math))
        planner.set_params(car_params(params))
        results[crowd] = rollout_with(planner, u_in, noise)
    check_name(results[False][3], wscale, "k_rollout_barebone exact", math == "exact")
    check_name(results[True][3], wscale, "k_rollout_barebone_crowd", math == "exact")
    assert (results[False][0] > 2e6).any(), "bad input: no rollout is inside two discs"  # (obs_penalty 1e6)
    plain = MPPI_Numba(cfg_of(n, t, True, math))
    plain.set_params(params)
    assert (rollout_with(plain, u_in, noise)[0] != results[True][0]).any(), "bad input: the car costs what the unicycle costs"
    for i, what in enumerate(("costs", "u after update()", "weights")):
        assert_bits(results[True][i], results[False][i], "%s, crowd on vs off (%s math)" % (what, math))


# ---- 4. a batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crowd", [False, True])
def test_a_batch_equals_single_car_planners(car, crowd):
    """B = 3 with per-problem starts and goals, a goal track on problem 1 (the others' tracks repeat their goals)."""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    from goal_track_model import goal_track_costs
    from test_gpu_barebone_goal_tracks import goal_params, problem_goal
    B, n, t, L = 3, 64, 30, 9
    rng = np.random.default_rng(41 + crowd)
    x0s, goals = problems(rng, B)
    pos, rad = crowd_discs(rng, 7 if crowd else 2, x0s[0], goals[0])
    params = car_params(make_params(DT, 0.5, (pos, rad)))
    gtracks = [np.repeat(goals[b][None], L, 0) for b in range(B)]
    gtracks[1] = problem_goal(rng, x0s[1], goals[1], L)
    u_in = np.stack([inputs(rng, n, t)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    batch = MPPI_Batch(cfg_of(n, t, crowd), B)
    batch.setup(params, x0s, goals, goal_tracks=gtracks)
    costs, u_out, weights, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    check_name(kernel, 0.5, "k_rollout_barebone_crowd" if crowd else "k_rollout_barebone exact")
    assert "problems=%d" % B in kernel and " goal_rows=%d" % L in kernel, kernel
    assert batch.drive == "car"
    single = MPPI_Numba(cfg_of(n, t, crowd))
    for b in range(B):
        pb = problem_params(params, x0s[b], goals[b])
        single.set_params(goal_params(pb, gtracks[b]))
        want, want_u, want_w, single_kernel = rollout_with(single, u_in[b], noise[b])
        assert "problems" not in single_kernel and single_kernel.endswith(" drive=car"), single_kernel
        assert_bits(costs[b], want, "problem %d vs a single car planner" % b)
        assert_bits(u_out[b], want_u, "problem %d u vs a single car planner" % b)
        assert_bits(weights[b], want_w, "problem %d weights vs a single car planner" % b)
        model = goal_track_costs(oracle_params(pb), gtracks[b], noise[b], u_in[b], 0, pos[:, None], rad)
        assert_bits(costs[b], model, "problem %d vs the goal-track model on car states" % b)


# ---- 5. the visualisation rollouts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wscale", WSCALES)
def test_state_rollouts_equal_the_model(wscale):
    """Row 0 is u_cur unclipped -- entries outside both ranges --, w = fl(v * kappa) there as well."""
    from mppi_numba_amd.barebone import MPPI_Numba
    n, t, v = 128, 30, 8
    rng = np.random.default_rng(5)
    params = car_params(make_params(DT, wscale))
    planner = MPPI_Numba(make_cfg(n, t, v=v))
    planner.setup(params)
    planner.solve()
    u_cur = inputs(rng, n, t)[0]
    u_cur[3], u_cur[4], u_cur[7] = (1.5, 40.0), (-1.0, 0.3), (5.0, -4.0)
    planner.set_u(u_cur)
    noise = planner.noise_samples_d.copy_to_host()
    u_prev, u_now = planner.u_prev_d.copy_to_host(), planner.u_cur_d.copy_to_host()
    assert_bits(u_now, u_cur, "the controls set")
    got = planner.get_state_rollout()
    assert got.shape == (v, t + 1, 3)
    p = oracle_params(params)
    want = car_model.state_rollout(p, noise, u_prev, u_now, v)
    unicycle = O.state_rollout_barebone(p, noise, u_prev, u_now, v)
    assert (want[0] != unicycle[0]).any() and (want[1:] != unicycle[1:]).any(), "bad input: car and unicycle cannot be told apart"
    clipped = car_model.state_rollout(p, np.concatenate([noise[:1] * 0, noise]), u_now, u_now, v + 1)[1]
    assert (want[0] != clipped).any(), "bad input: row 0 is the same clipped or not"
    assert_bits(got, want, "state rollouts vs the car model")


# ---- 6. the fleets ----------------------------------------------------------------------------------------------------------
def fleet_scene(t):
    from test_gpu_barebone_fleet import ring
    x0s, goals, us, noise = ring(3, 64, t, 11, aimed=False, radius=0.5)
    return x0s, goals, us, noise.reshape(3 * 64, t, 2)


@pytest.mark.parametrize("wscale", WSCALES)
def test_fleet_walls_equal_the_model(car, wscale):
    """Random start headings, controls with entries outside vrange / wrange.  The refresh at the head of the one solve()
    reads the controls set; the walls behind it are the model's on car plans."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, t = 3, 37
    x0s, goals, us, noise = fleet_scene(t)
    params = car_params(make_params(DT, wscale))
    batch = MPPI_Batch(cfg_of(64, t, True), B)
    batch.setup(params, x0s, goals)
    batch.set_fleet(0.25, margin=0.05)
    batch.set_u(us)
    batch.solve()
    seg, hw, others = batch.fleet_walls()
    kernel = batch.last_rollout_kernel()
    check_name(kernel, wscale, "k_rollout_barebone_crowd")
    assert " fleet=%d" % B in kernel, kernel
    want = fleet_model.fleet_walls(params, x0s, us)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(O, "state_rollout_barebone", lambda *a: car_model.state_rollout(*a, car=False))
        assert (want != fleet_model.fleet_walls(params, x0s, us)).any(), "bad input: the car's plans are the unicycle's"
    assert_bits(hw, fleet_model.halfwidths(0.25, 0.05, B), "half-widths")
    assert_bits(seg, want, "the fleet's walls vs the model on car plans")
    # ... and the costs of a rollout launch over them
    costs, _, _, _ = rollout_with(batch, us, noise)
    for b in range(B):
        pb = oracle_params(problem_params(params, x0s[b], goals[b]))
        model = fleet_model.fleet_costs(pb, want[b], hw[b], noise.reshape(B, 64, t, 2)[b], us[b])
        assert_bits(costs[b], model, "robot %d vs the fleet model on car states" % b)


@pytest.mark.parametrize("wscale", WSCALES)
def test_fleet_body_walls_equal_the_model(car, wscale):
    from mppi_numba_amd.barebone import MPPI_Batch
    from test_footprint_model import EIGHT
    B, t = 3, 37
    body = EIGHT[[0, 5, 6]]
    x0s, goals, us, _ = fleet_scene(t)
    params = car_params(make_params(DT, wscale))
    batch = MPPI_Batch(cfg_of(64, t, True), B)
    batch.setup(params, x0s, goals)
    batch.set_fleet_bodies(body, margin=0.05)
    batch.set_u(us)
    batch.solve()
    seg, hw, others = batch.fleet_body_walls()
    kernel = batch.last_rollout_kernel()
    check_name(kernel, wscale, "k_rollout_barebone_crowd")
    assert " fleet=%d" % B in kernel and " footprint=3" in kernel, kernel
    want = fleet_body_model.body_walls(params, x0s, us, body)
    assert seg.shape == want.shape == (B, B - 1, 3, t, 2, 2)
    assert_bits(hw, fleet_body_model.halfwidths(body, 0.05), "half-widths")
    assert_bits(seg, want, "the body fleet's walls vs the model on car plans")


# ---- 7. the closed loop -----------------------------------------------------------------------------------------------------
def _car_loop(planner, dt, x0, xgoal, tol, max_steps):
    """test_gpu_barebone_batch._notebook_loop with the car's heading: th += dt * v * kappa, in float64."""
    xhist = np.zeros((max_steps + 1, 3)) * np.nan
    uhist = np.zeros((max_steps, 2), dtype=np.float32) * np.nan
    xhist[0] = x0
    steps = max_steps
    for t in range(max_steps):
        useq = planner.solve()
        uhist[t] = useq[0]
        u_curr = useq[0].astype(np.float64)
        xhist[t + 1, 0] = xhist[t, 0] + dt * np.cos(xhist[t, 2]) * u_curr[0]
        xhist[t + 1, 1] = xhist[t, 1] + dt * np.sin(xhist[t, 2]) * u_curr[0]
        xhist[t + 1, 2] = xhist[t, 2] + dt * u_curr[0] * u_curr[1]
        planner.shift_and_update(xhist[t + 1], useq, num_shifts=1)
        if np.linalg.norm(xhist[t + 1, :2] - xgoal) <= tol:
            steps = t + 1
            break
    return xhist, uhist, steps


@pytest.mark.parametrize("wscale", WSCALES)
def test_closed_loop_equals_the_host_loop(wscale):
    """The tolerances of test_gpu_barebone_batch.test_closed_loop_equals_the_notebook_loop."""
    from mppi_numba_amd.barebone import MPPI_Numba
    max_steps = 20
    cfg = make_cfg(1000, 50, seed=1)
    params = car_params(make_params(cfg.dt, wscale, (np.array([[5, 4.5], [2, 1]]), np.array([1.5, 1.0]))))
    host = MPPI_Numba(cfg)
    host.setup(params)
    want_x, want_u, want_steps = _car_loop(host, cfg.dt, params["x0"], params["xgoal"], params["goal_tolerance"], max_steps)
    assert want_steps == max_steps
    unicycle = want_x[:-1, 2] + cfg.dt * want_u[:, 1].astype(np.float64)
    assert np.abs(unicycle - want_x[1:, 2]).max() > 1e-3, "bad input: the unicycle's world would turn the same way"
    dev = MPPI_Numba(make_cfg(1000, 50, seed=1))
    dev.setup(params)
    got_x, got_u, got_steps = dev.closed_loop(max_steps)
    check_name(dev.last_rollout_kernel(), wscale, "k_rollout_barebone exact")
    assert got_steps == want_steps
    np.testing.assert_allclose(got_u, want_u, rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_x, want_x, rtol=0, atol=1e-5)
    np.testing.assert_allclose(dev.params["x0"], got_x[max_steps])
    np.testing.assert_allclose(dev.solve(), host.solve(), rtol=0, atol=2e-5)


def test_graph_replay_gives_the_direct_loops_bits():
    """Five iterations a solve.  A new anchor and new cells of the same shape need no new capture in car mode either; a
    change of the drive needs one."""
    from mppi_numba_amd.barebone import MPPI_Numba
    from occupancy_cases import scatter
    n, t = 128, 18
    occ = dict(origin=(-1.0, -1.0), resolution=0.1, cells=scatter(31, (60, 60), 0.03), inflate=0.2, substeps=2)
    params = car_params(dict(make_params(DT, 0.5, num_opt=5), accel_limits=np.array([3.0, 4.0]), occupancy=occ))
    direct, graph = MPPI_Numba(cfg_of(n, t, True)), MPPI_Numba(cfg_of(n, t, True))
    graph.set_graph_replay(True)
    for planner in (direct, graph):
        planner.setup(params)
        planner.set_applied_control([0.5, 0.1])
    for call in range(3):
        assert_bits(graph.solve(), direct.solve(), "solve %d" % call)
    check_name(graph.last_rollout_kernel(), 0.5, "k_rollout_barebone_crowd")
    stats = graph.graph_stats()
    assert stats["captures"] >= 1 and stats["replays"] >= 3, stats
    for planner in (direct, graph):
        planner.set_applied_control([0.2, 0.9])
    assert_bits(graph.solve(), direct.solve(), "a new anchor")
    assert graph.graph_stats()["captures"] == stats["captures"], "a new anchor forced a new capture"
    for planner in (direct, graph):
        planner.params["occupancy"] = dict(occ, cells=scatter(32, (60, 60), 0.2))
    assert_bits(graph.solve(), direct.solve(), "new cells")
    assert graph.graph_stats()["captures"] == stats["captures"], "new cells of the same shape forced a new capture"
    for planner in (direct, graph):
        planner.params["drive"] = "car"
    assert_bits(graph.solve(), direct.solve(), "the same drive again")
    assert graph.graph_stats()["captures"] == stats["captures"], "the same drive again forced a new capture"
    for planner in (direct, graph):
        del planner.params["drive"]
    assert_bits(graph.solve(), direct.solve(), "the unicycle")
    assert "drive" not in graph.last_rollout_kernel()
    assert graph.graph_stats()["captures"] > stats["captures"], "another drive, the same captured launches"


# ---- 8. off is off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wscale", [1.0, 1.5])
@pytest.mark.parametrize("crowd", [False, True])
def test_without_the_key_every_bit_and_every_name_is_as_before(crowd, wscale):
    """The key absent, 'unicycle', and 'car' set and then removed: the C oracle's costs, and one kernel name."""
    from mppi_numba_amd.barebone import MPPI_Numba
    n, t = 130, 17
    params, pos, rad, u_in, noise = scene(n, t, 7 if crowd else 2, wscale)
    want = O.rollout_barebone(oracle_params(params), pos, rad, noise, u_in)
    names = set()
    for how in ("absent", "unicycle", "car, then removed"):
        planner = MPPI_Numba(cfg_of(n, t, crowd))
        if how == "car, then removed":
            planner.set_params(car_params(params))
            got, _, _, kernel = rollout_with(planner, u_in, noise)
            assert kernel.endswith(" drive=car") and (got != want).any(), kernel
        planner.set_params(dict(params, drive="unicycle") if how == "unicycle" else params)
        got, _, _, kernel = rollout_with(planner, u_in, noise)
        assert planner.drive == "unicycle"
        assert "drive" not in kernel and ("rotation=1" in kernel) == (wscale == 1.0), kernel
        names.add(kernel)
        assert_bits(got, want, "the key %s vs the oracle" % how)
    assert len(names) == 1, names


def test_a_new_anchor_or_new_cells_need_no_new_capture_without_the_key():
    from mppi_numba_amd.barebone import MPPI_Numba
    from occupancy_cases import scatter
    n, t = 128, 18
    occ = dict(origin=(-1.0, -1.0), resolution=0.1, cells=scatter(31, (60, 60), 0.03), inflate=0.2, substeps=2)
    params = dict(make_params(DT, 1.0, num_opt=5), accel_limits=np.array([3.0, 4.0]), occupancy=occ)
    never, graph = MPPI_Numba(cfg_of(n, t, True)), MPPI_Numba(cfg_of(n, t, True))
    graph.set_graph_replay(True)
    never.setup(params)
    graph.setup(dict(params, drive="unicycle"))
    for call in range(3):
        assert_bits(graph.solve(), never.solve(), "solve %d" % call)
    captures = graph.graph_stats()["captures"]
    for planner in (never, graph):
        planner.set_applied_control([0.2, 0.9])
        planner.params["occupancy"] = dict(occ, cells=scatter(32, (60, 60), 0.2))
    assert_bits(graph.solve(), never.solve(), "a new anchor and new cells")
    assert graph.graph_stats()["captures"] == captures
    assert "drive" not in graph.last_rollout_kernel() and graph.last_rollout_kernel() == never.last_rollout_kernel()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Numba
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    from test_gpu_batch import make_world
    lib = _lib.load()
    # a map mode has no drive
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    before = mapped.solve()
    assert lib.mppi_planner_set_drive(mapped._handle, 1) == ERR_INVALID
    assert "barebone" in lib.mppi_last_error().decode()
    drive = C.c_int(7)
    assert lib.mppi_planner_get_drive(mapped._handle, C.byref(drive)) == ERR_INVALID and drive.value == 7
    assert np.isfinite(before).all() and np.isfinite(mapped.solve()).all()
    # a value that is no drive
    n, t = 130, 17
    params, pos, rad, u_in, noise = scene(n, t, 2, 0.5)
    planner, twin = MPPI_Numba(cfg_of(n, t, False)), MPPI_Numba(cfg_of(n, t, False))
    for p in (planner, twin):
        p.set_params(car_params(params))
    want = rollout_with(twin, u_in, noise)
    got = rollout_with(planner, u_in, noise)
    for bad in (2, -1, 1 << 20):
        assert lib.mppi_planner_set_drive(planner._handle, bad) == ERR_INVALID
        assert "MPPI_DRIVE" in lib.mppi_last_error().decode()
        assert planner.drive == "car"
    again = rollout_with(planner, u_in, noise)
    assert again[3] == want[3] and again[3].endswith(" drive=car")
    for i, what in enumerate(("costs", "u", "weights")):
        assert_bits(got[i], want[i], what)
        assert_bits(again[i], want[i], "%s after the refusals" % what)
    planner.set_params(dict(params, drive="tank"))
    with pytest.raises(ValueError, match="drive"):
        planner.solve()
    assert planner.drive == "car"
    assert lib.mppi_planner_get_drive(planner._handle, None) == ERR_INVALID


# ---- 10. behaviour ----------------------------------------------------------------------------------------------------------
def test_a_car_does_not_turn_on_the_spot():
    """Start facing away from the goal, v in (0, 2), kappa in +-1: at every executed step |dth| <= kappa_max * ds + 1e-5, ds
    the distance moved -- the float64 world step turns by dt * v * kappa and moves by dt * v (times a unit vector whose
    float64 norm is 1 to 1e-16), and |kappa| <= 1 after the update's clip.  The unicycle on the same task spins where it
    stands at the first steps."""
    from mppi_numba_amd.barebone import MPPI_Numba
    max_steps, kappa_max = 40, 1.0
    task = dict(make_params(DT, 1.0, num_opt=2), x0=np.array([0.0, 0.0, np.pi]), xgoal=np.array([6.0, 0.5]),
                wrange=np.array([-kappa_max, kappa_max]))

    def excess(params):
        planner = MPPI_Numba(make_cfg(1024, 30, seed=2))
        planner.setup(params)
        xhist, uhist, steps = planner.closed_loop(max_steps)
        x = xhist[:steps + 1]
        assert np.isfinite(x).all() and steps >= 10
        ds = np.linalg.norm(np.diff(x[:, :2], axis=0), axis=1)
        dth = np.abs(np.diff(x[:, 2]))
        return dth - kappa_max * ds, planner.last_rollout_kernel()

    over, kernel = excess(car_params(task))
    print("car: largest |dth| - kappa_max * ds = %.3g" % over.max())
    assert kernel.endswith(" drive=car"), kernel
    assert (over <= 1e-5).all(), "the car turned by more than kappa_max * ds at steps %s" % np.nonzero(over > 1e-5)[0]
    spin, kernel = excess(task)
    assert "drive" not in kernel
    assert (spin[:5] > 1e-2).any(), "bad input: the unicycle does not spin at the first steps (%s)" % spin[:5]
