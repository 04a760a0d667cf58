"""Time-correlated control noise in the barebone planner (params['noise_smoothing'], mppi_planner_set_noise_smoothing):
every generated block is the AR(1) filter of the white block a twin handle -- same seed, no smoothing -- draws at the same
Philox epoch, bit for bit (tests/noise_smoothing_model.py is the recurrence in numpy float32); the iteration loop, graph
replay and closed_loop consume that block and no other; off is off to the bit."""
import ctypes as C

import numpy as np
import pytest

import noise_smoothing_model as model
from test_gpu_barebone_batch import _notebook_loop, assert_bits, make_cfg, make_params, problems
from test_gpu_barebone_walls import wall_params
from test_noise_plan import BAREBONE, IN_LINE, choose, held  # noqa: F401  (choose: the fixture that compiles noise_plan.h)

pytestmark = pytest.mark.gpu

NOTEBOOK_DISCS = (np.array([[5.0, 4.5], [2.0, 1.0]]), np.array([1.5, 1.0]))  # barebone_mppi_numba.ipynb cell 5

# csrc/rng_kernels.h: kSmoothChunk = 128 steps of a tile are in LDS at once -- (70, 129) and (64, 257) are one step past a
# chunk and one past two.  Below, at and above a tile of 64 rollouts; odd horizons whose last Philox block stores one step.
SHAPES = [(63, 1), (64, 2), (65, 7), (130, 17), (200, 33), (70, 129), (64, 257)]
BETAS = [(0.9, 0.5), (0.0, 0.7), (0.999, 0.0)]

# The routes noise_choose (csrc/noise_plan.h) has for kLaunchBarebone, and the smallest shapes that reach them on 256 CUs:
# in line below 4M rollout-steps (update_plan.h: update_noise_is_long); ahead on the second stream beside the rollout from
# 4M on while a CU holds at most kSideStreamMaxWaves = 8 tiles (N <= 8 * 256 * 64 = 131072); ahead beside the update from
# 2049 tiles on.
ROUTE_SHAPES = {"in_line": (128, 18), "second_stream": (125056, 32), "beside_update": (131136, 31)}


def cfg_of(n, t, seed=3, math="exact", crowd=False, rng="philox"):
    cfg = make_cfg(n, t, seed=seed)
    cfg.math, cfg.crowd, cfg.rng = math, crowd, rng
    return cfg


def task(num_opt=1, discs=NOTEBOOK_DISCS, **more):
    return dict(make_params(0.1, 1.0, discs, num_opt=num_opt), **more)


def planner_of(cfg, params):
    from mppi_numba_amd.barebone import MPPI_Numba
    p = MPPI_Numba(cfg)
    p.setup(params)
    return p


def draw(planner, n, t):
    planner.sample_noise()
    return planner.noise_samples_d.copy_to_host().reshape(n, t, 2)


def check_block(got, white, beta, what):
    """got is the model of white, bit for bit; a component with beta = 0 is the twin's outright."""
    assert_bits(got, model.smooth(white, beta), what)
    for c in range(2):
        if beta[c] == 0.0:
            np.testing.assert_array_equal(got[..., c], white[..., c], err_msg=what)
        elif got.shape[1] > 1:
            assert (got[:, 1:, c] != white[:, 1:, c]).any(), what + ": component %d is not filtered" % c


# ---- 1. the generator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("n,t", SHAPES)
def test_every_block_is_the_filter_of_the_twins_block(n, t, math):
    twin = planner_of(cfg_of(n, t, math=math), task())
    white = [draw(twin, n, t) for _ in range(3)]  # epochs 0, 1, 2
    assert twin.noise_smoothing is None
    assert (white[0] != white[1]).any()
    for beta in BETAS:
        smooth = planner_of(cfg_of(n, t, math=math), task(noise_smoothing=np.array(beta)))
        for epoch in range(3):
            check_block(draw(smooth, n, t), white[epoch], beta, "N %d T %d beta %s epoch %d" % (n, t, beta, epoch))
        np.testing.assert_array_equal(smooth.noise_smoothing, np.array(beta, dtype=np.float32))


def batch_of(cfg, B, params, seed=5):
    from mppi_numba_amd.barebone import MPPI_Batch
    x0s, goals = problems(np.random.default_rng(seed), B)
    batch = MPPI_Batch(cfg, B)
    batch.setup(params, x0s, goals)
    return batch


def test_every_block_of_a_batch_is_the_filter_of_the_twins_block():
    B, n, t = 3, 64, 17
    twin = batch_of(cfg_of(n, t), B, task())
    smooth = batch_of(cfg_of(n, t), B, task(noise_smoothing=0.8))
    for epoch in range(3):
        check_block(draw(smooth, B * n, t), draw(twin, B * n, t), (0.8, 0.8), "batch, epoch %d" % epoch)


# ---- 2. off is off ---------------------------------------------------------------------------------------------------
def test_zero_and_cleared_coefficients_are_the_white_generator():
    n, t = 130, 17
    params = task(num_opt=2)
    never = planner_of(cfg_of(n, t), params)
    zero = planner_of(cfg_of(n, t), dict(params, noise_smoothing=(0.0, 0.0)))
    cleared = planner_of(cfg_of(n, t), dict(params, noise_smoothing=0.9))
    cleared.move_mppi_task_vars_to_device()  # (handed over ...)
    np.testing.assert_array_equal(cleared.noise_smoothing, np.float32([0.9, 0.9]))
    cleared.set_params(params)               # (... and the key gone again)
    for call in range(2):
        want_u = never.solve()
        want_c = never.costs_d.copy_to_host()
        for other, name in ((zero, "set to (0, 0)"), (cleared, "set and cleared")):
            assert_bits(other.solve(), want_u, "u, %s, solve %d" % (name, call))
            assert_bits(other.costs_d.copy_to_host(), want_c, "costs, %s, solve %d" % (name, call))
            assert other.noise_smoothing is None


# ---- 3. the loop consumes what the generator made --------------------------------------------------------------------
def crowd_scene():
    rng = np.random.default_rng(11)
    pos = rng.uniform(0.5, 6.5, (7, 2)).astype(np.float32)
    rad = rng.uniform(0.2, 0.6, 7).astype(np.float32)
    a = rng.uniform(0.0, 7.0, (10, 1, 2))
    seg = np.concatenate([a, a + rng.normal(0, 0.8, (10, 1, 2))], axis=1).astype(np.float32)
    return wall_params(task(discs=(pos, rad)), seg, 0.05)


def stage_level_twin(make, params, beta, iterations):
    """Twin A draws the white blocks; twin B is driven through set_noise(model(...)), rollout(), update(): its costs and u
    after every iteration."""
    drawer, driven = make(params), make(params)
    n, t = drawer.num_instances * drawer.num_control_rollouts, drawer.num_steps
    out = []
    for _ in range(iterations):
        driven.set_noise(model.smooth(draw(drawer, n, t), beta))
        driven.rollout()
        costs = driven.costs_d.copy_to_host()
        driven.update()
        out.append((costs, driven.u_cur_d.copy_to_host()))
    return out


@pytest.mark.parametrize("family", ["default", "crowd", "batch"])
def test_the_loop_consumes_the_filtered_blocks(family):
    beta = (0.9, 0.6)
    if family == "default":
        params, make = task(), lambda p: planner_of(cfg_of(128, 18), p)
    elif family == "crowd":
        params, make = crowd_scene(), lambda p: planner_of(cfg_of(64, 18, crowd=True), p)
    else:
        params, make = task(), lambda p: batch_of(cfg_of(64, 18), 3, p)
    want = stage_level_twin(make, params, beta, 3)
    on = dict(params, noise_smoothing=np.array(beta))
    # one iteration per solve(): costs and u after every iteration
    stepwise = make(on)
    for k in range(3):
        u = stepwise.solve()
        assert_bits(stepwise.costs_d.copy_to_host(), want[k][0], "%s: costs after iteration %d" % (family, k))
        assert_bits(u, want[k][1], "%s: u after iteration %d" % (family, k))
    if family == "crowd":
        assert stepwise.last_rollout_kernel().startswith("k_rollout_barebone_crowd"), stepwise.last_rollout_kernel()
    # ... and the three iterations of one solve()
    loop = make(dict(on, num_opt=3))
    u = loop.solve()
    assert_bits(loop.costs_d.copy_to_host(), want[2][0], "%s: costs of solve(num_opt = 3)" % family)
    assert_bits(u, want[2][1], "%s: u of solve(num_opt = 3)" % family)
    # (the white loop is another: the twin is not passed by accident)
    assert (make(dict(params, num_opt=3)).solve() != u).any()


def test_the_route_shapes_reach_their_routes(choose):  # noqa: F811
    """noise_plan.h compiled on the host: the shapes of ROUTE_SHAPES take the three routes a barebone launch has, on the
    device's own CU count (the loop of a solve(): noise wanted ahead, none there yet | taken from ahead)."""
    from mppi_numba_amd import _lib
    cus = _lib.device_props(0).compute_units

    def can_host(n, t):  # update_plan.h, update_noise_beside: the update launch hosts a generator from 4M rollout-steps on
        return int(n * t >= 4 * 1000 * 1000)
    states, names = [], []
    for name, (n, t) in ROUTE_SHAPES.items():
        for have in ((0,) if name == "in_line" else (0, 1)):  # (in line: nothing is ever there ahead)
            states.append(held(launch=BAREBONE, n_local=n, T=t, num_cus=cus, workgroups=(n + 63) // 64, have_noise=have,
                               noise_on_side_stream=int(have and name == "second_stream"), update_can_host=can_host(n, t)))
            names.append(name)
    for name, state, c in zip(names, states, choose(states)):
        assert c["extra_blocks"] == 0, name
        assert c["beside_rollout"] == int(name == "second_stream"), (name, state, c)
        assert c["beside_update"] == int(name == "beside_update"), (name, state, c)
        if name == "in_line":
            assert c["source"] == IN_LINE and not c["have_noise"], (name, c)
        else:
            assert c["have_noise"] == 1, (name, c)
    # one tile, one step fewer: the next route down
    n, t = ROUTE_SHAPES["second_stream"]
    fewer = choose([held(launch=BAREBONE, n_local=n - 64, T=t, num_cus=cus, workgroups=n // 64 - 1, update_can_host=can_host(n - 64, t))])[0]
    assert not fewer["beside_rollout"] and not fewer["beside_update"]
    n, t = ROUTE_SHAPES["beside_update"]
    fewer = choose([held(launch=BAREBONE, n_local=n - 64, T=t, num_cus=cus, workgroups=n // 64 - 1, update_can_host=can_host(n - 64, t))])[0]
    assert fewer["beside_rollout"] and not fewer["beside_update"]


@pytest.mark.parametrize("route", ["second_stream", "beside_update"])
def test_a_generator_that_runs_ahead_is_filtered_too(route):
    """N * T >= 4M: the blocks of the second and third iteration are generated ahead, beside the first and second.  The
    block the third iteration consumed against the model of the twin's third block, on a strided sample of 64 tiles; and the
    block left primed for the next call, handed out by sample_noise(), against the twin's fourth."""
    n, t = ROUTE_SHAPES[route]
    beta = (0.9, 0.5)
    params = task(num_opt=3, discs=None)
    twin = planner_of(cfg_of(n, t), params)
    white = [draw(twin, n, t) for _ in range(4)]
    loop = planner_of(cfg_of(n, t), dict(params, noise_smoothing=np.array(beta)))
    u = loop.solve()
    assert np.isfinite(u).all()
    tiles = n // 64
    rows = (np.arange(0, tiles, max(1, tiles // 64))[:64, None] * 64 + np.arange(64)[None, :]).ravel()
    rows = np.concatenate([rows, np.arange(n - 64, n)])  # (and the last tile)
    got = loop.noise_samples_d.copy_to_host().reshape(n, t, 2)
    check_block(got[rows], white[2][rows], beta, "%s: the third iteration's block" % route)
    ahead = draw(loop, n, t)
    check_block(ahead[rows], white[3][rows], beta, "%s: the block generated beside the last iteration" % route)


# ---- 4. a change in mid-life -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t", [(130, 17), ROUTE_SHAPES["second_stream"]])
def test_a_change_applies_to_the_block_that_is_already_there(n, t):
    """After solve() the large shape holds the next block primed; the new coefficients replace it, same epoch."""
    params = task(discs=None)
    changed, other = planner_of(cfg_of(n, t), params), planner_of(cfg_of(n, t), params)
    assert_bits(changed.solve(), other.solve(), "the same handles")
    changed.set_params(dict(params, noise_smoothing=0.8))
    got, white = draw(changed, n, t), draw(other, n, t)
    rows = np.arange(0, n, max(1, n // 4096))
    check_block(got[rows], white[rows], (0.8, 0.8), "the block after the change")
    # the same values again, past the key cache: a comparison, nothing dropped
    from mppi_numba_amd import _lib
    captures, same = changed.graph_stats()["captures"], np.float32([0.8, 0.8])
    _lib.call("mppi_planner_set_noise_smoothing", changed._handle, _lib.ptr(same, C.c_float))
    assert changed.graph_stats()["captures"] == captures
    np.testing.assert_array_equal(changed.noise_smoothing, same)
    # ... and back, in front of a loop
    changed.set_params(params)
    assert_bits(changed.solve(), other.solve(), "cleared again")


# ---- 5. graph replay -------------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_direct_loops_bits():
    from mppi_numba_amd import _lib
    n, t = 128, 18
    params = task(num_opt=5, noise_smoothing=0.9)
    direct, graph = planner_of(cfg_of(n, t), params), planner_of(cfg_of(n, t), params)
    graph.set_graph_replay(True)
    for call in range(3):
        assert_bits(graph.solve(), direct.solve(), "solve %d" % call)
    stats = graph.graph_stats()
    assert stats["captures"] >= 1 and stats["replays"] >= 3, stats
    # the same values again, past the key cache: nothing is dropped
    same = np.float32([0.9, 0.9])
    _lib.call("mppi_planner_set_noise_smoothing", graph._handle, _lib.ptr(same, C.c_float))
    assert_bits(graph.solve(), direct.solve(), "the same values again")
    assert graph.graph_stats()["captures"] == stats["captures"]
    # a changed coefficient: one more capture, the direct loop's bits
    for p in (graph, direct):
        p.set_params(dict(params, noise_smoothing=(0.9, 0.3)))
    assert_bits(graph.solve(), direct.solve(), "a changed coefficient")
    assert graph.graph_stats()["captures"] == stats["captures"] + 1
    assert_bits(graph.solve(), direct.solve(), "... and the solve after it")
    assert graph.graph_stats()["captures"] == stats["captures"] + 1


# ---- 6. closed_loop --------------------------------------------------------------------------------------------------
def test_closed_loop_equals_the_host_driven_loop():
    """As test_gpu_barebone_batch.test_closed_loop_equals_the_notebook_loop compares them, same tolerances."""
    max_steps = 10
    params = task(num_opt=1, noise_smoothing=0.9)
    host = planner_of(cfg_of(256, 30, seed=1), params)
    want_x, want_u, want_steps = _notebook_loop(host, host.cfg, params["x0"], params["xgoal"], params["goal_tolerance"], max_steps)
    assert want_steps == max_steps
    dev = planner_of(cfg_of(256, 30, seed=1), params)
    got_x, got_u, got_steps = dev.closed_loop(max_steps)
    assert got_steps == want_steps
    np.testing.assert_allclose(got_u, want_u, rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_x, want_x, rtol=0, atol=1e-5)
    white = planner_of(cfg_of(256, 30, seed=1), task(num_opt=1))
    _, white_u, _ = white.closed_loop(max_steps)
    assert np.abs(white_u - got_u).max() > 1e-3, "the device loop drew the white noise"


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    n, t = 130, 17
    params = task(noise_smoothing=(0.5, 0.25))
    planner, twin = planner_of(cfg_of(n, t), params), planner_of(cfg_of(n, t), params)
    assert_bits(planner.solve(), twin.solve(), "before")
    for bad in (1.0, -0.1, np.nan, np.float32(1 - 2.0 ** -25), (0.5, 1.0), (np.inf, 0.0)):
        planner.set_params(dict(params, noise_smoothing=bad))
        with pytest.raises(_lib.MppiError, match=r"\[0, 1\)"):
            planner.solve()
        np.testing.assert_array_equal(planner.noise_smoothing, np.float32([0.5, 0.25]))
    for shape in ((3,), (1,), (2, 2)):
        planner.set_params(dict(params, noise_smoothing=np.full(shape, 0.5)))
        with pytest.raises(ValueError, match="noise_smoothing"):
            planner.solve()
    planner.set_params(params)
    np.testing.assert_array_equal(planner.noise_smoothing, np.float32([0.5, 0.25]))
    assert_bits(planner.solve(), twin.solve(), "the solve after the refusals")
    # the generator that exists for parity with the reference
    xoro = planner_of(cfg_of(n, t, rng="xoroshiro"), params)
    with pytest.raises(_lib.MppiError, match="Philox"):
        xoro.solve()
    assert xoro.noise_smoothing is None
    xoro.set_params(task())
    assert np.isfinite(xoro.solve()).all()
    # a map mode
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    beta = np.float32([0.5, 0.5])
    with pytest.raises(_lib.MppiError, match="barebone"):
        _lib.call("mppi_planner_set_noise_smoothing", mapped._handle, _lib.ptr(beta, C.c_float))
    with pytest.raises(_lib.MppiError, match="barebone"):
        _lib.call("mppi_planner_set_noise_smoothing", mapped._handle, None)


# ---- 8. what it is for -----------------------------------------------------------------------------------------------
def test_the_returned_controls_are_smoother():
    """The notebook's problem, zero controls, one iteration, the same seed: sum_t |u[t+1] - u[t]|^2 of the returned
    sequence.  (Under near-equal weights theory says a ratio of about 1 - beta = 0.1; measured on the MI355X: 132.447
    white, 13.1674 smoothed, ratio 0.0994 -- profiles/HISTORY.md, "Barebone noise smoothing".)"""
    rough = {}
    for name, extra in (("white", {}), ("smooth", dict(noise_smoothing=0.9))):
        planner = planner_of(cfg_of(1024, 50, seed=1), task(num_opt=1, **extra))
        rough[name] = model.roughness(planner.solve())
    print("roughness white %.6g  beta 0.9 %.6g  ratio %.4f" % (rough["white"], rough["smooth"], rough["smooth"] / rough["white"]))
    assert rough["smooth"] < rough["white"]
