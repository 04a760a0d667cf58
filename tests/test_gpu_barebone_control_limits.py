"""Acceleration limits on the sampled controls in the barebone planner (params['accel_limits'],
mppi_planner_set_control_limits): every block an iteration consumes is the projection of the block a twin handle -- same
seed, no limits -- draws at the same epoch, bit for bit (tests/control_limits_model.py is the recurrence in numpy float32);
the iteration loop, graph replay and closed_loop consume that block and no other; what solve() returns is feasible within
tol = 2^-20 * (M + d) from the applied control; off is off to the bit."""
import ctypes as C

import numpy as np
import pytest

import control_limits_model as model
import noise_smoothing_model as smoothing
from test_gpu_barebone_batch import _notebook_loop, assert_bits
from test_gpu_barebone_noise_smoothing import ROUTE_SHAPES, batch_of, cfg_of, crowd_scene, draw, planner_of, task

pytestmark = pytest.mark.gpu

# Below, at and above a tile of 64 rollouts; horizons below, at and one past the eight steps whose targets k_noise_limit
# forms ahead of the chain (csrc/rng_kernels.h: kLimitAhead), T = 1, one past a register set of kLimitBatch = 32 steps; then
# the horizons at which the kernel fetches a set again: the two sets hold 64 steps, (65, 65) is one past them, (70, 129) one
# past four.
SHAPES = [(63, 1), (64, 2), (65, 7), (64, 8), (64, 9), (130, 17), (200, 33), (64, 64), (65, 65), (70, 129)]
ACCEL = (1.0, 2.0)
ANCHOR = np.float32([0.7, -0.4])
DT = 0.1


def ranges(params):
    return tuple(params["vrange"]), tuple(params["wrange"])


def random_u(rng, t, params, lead=()):
    """A control sequence inside the box, float32."""
    (vlo, vhi), (wlo, whi) = ranges(params)
    return np.stack([rng.uniform(vlo, vhi, lead + (t,)), rng.uniform(wlo, whi, lead + (t,))], axis=-1).astype(np.float32)


def limited(params, accel=ACCEL):
    return dict(params, accel_limits=np.array(accel))


def want_block(white, u, anchor, params, accel=ACCEL):
    return model.limit(white, u, anchor, *ranges(params), accel, params["dt"])


def check_limited(got, white, u, anchor, params, what, accel=ACCEL):
    assert_bits(got, want_block(white, u, anchor, params, accel), what)
    if got.shape[1] > 1:
        assert (got != white).any(), what + ": the block is not limited"


# ---- 1. the block against the model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("n,t", SHAPES)
def test_every_block_is_the_projection_of_the_twins_block(n, t, math):
    params = task()
    twin = planner_of(cfg_of(n, t, math=math), params)
    lim = planner_of(cfg_of(n, t, math=math), limited(params))
    rng = np.random.default_rng(n * 100 + t)
    for epoch in range(2):
        u = random_u(rng, t, params)
        lim.set_u(u)
        lim.set_applied_control(ANCHOR)
        check_limited(draw(lim, n, t), draw(twin, n, t), u, ANCHOR, params, "N %d T %d %s epoch %d" % (n, t, math, epoch))
    np.testing.assert_array_equal(lim.accel_limits, np.float32(ACCEL))
    np.testing.assert_array_equal(lim.applied_control, ANCHOR)
    assert twin.accel_limits is None


@pytest.mark.parametrize("how", ["xoroshiro", "smoothing", "one_component"])
def test_the_pass_is_behind_whatever_generated_the_block(how):
    n, t = 130, 17
    params = task(noise_smoothing=np.array([0.9, 0.5])) if how == "smoothing" else task()
    rng_kind = "xoroshiro" if how == "xoroshiro" else "philox"
    accel = (np.inf, 2.0) if how == "one_component" else ACCEL
    twin = planner_of(cfg_of(n, t, rng=rng_kind), params)
    lim = planner_of(cfg_of(n, t, rng=rng_kind), limited(params, accel))
    u = random_u(np.random.default_rng(4), t, params)
    lim.set_u(u)
    lim.set_applied_control(ANCHOR)
    block = draw(twin, n, t)  # (smoothing: the twin's block is the filtered one)
    got = draw(lim, n, t)
    check_limited(got, block, u, ANCHOR, params, how, accel)
    if how == "smoothing":
        white = draw(planner_of(cfg_of(n, t), task()), n, t)
        assert_bits(block, smoothing.smooth(white, (0.9, 0.5)), "the twin's block is the filter of the white one")
    if how == "one_component":
        assert_bits(got[..., 0], block[..., 0], "the component without a limit stays as drawn")


def hand_made_block(rng, n, t, u, params):
    """Rows that drive every branch: the box binding, the rate binding both ways, nothing binding, sums that cancel,
    denormal noise."""
    block = rng.normal(0, 1, (n, t, 2)).astype(np.float32)
    block[0::6] *= np.float32(8.0)      # far outside the box
    block[1::6] *= np.float32(1e-3)     # next to u: nothing binds once the chain has caught up
    block[2::6] = -u[None]              # u + e cancels
    block[3::6] *= np.float32(1e-40)    # denormal
    block[4::6] = np.abs(block[4::6])   # upwards only
    return block


def test_the_stage_hook_limits_the_block_that_was_set():
    n, t = 130, 17
    params = task()
    lim = planner_of(cfg_of(n, t), limited(params))
    rng = np.random.default_rng(6)
    u = random_u(rng, t, params)
    block = hand_made_block(rng, n, t, u, params)
    lim.set_u(u)
    lim.set_applied_control(ANCHOR)
    lim.set_noise(block)
    assert_bits(lim.noise_samples_d.copy_to_host().reshape(n, t, 2), block, "set_noise stores what it is given")
    lim.limit_noise()
    got = lim.noise_samples_d.copy_to_host().reshape(n, t, 2)
    check_limited(got, block, u, ANCHOR, params, "the hand-made block")
    # the block reaches the branches: box, rate up, rate down, nothing
    raw = model.applied(block, u, *ranges(params))
    path = model.applied(got, u, *ranges(params))
    (vlo, vhi), _ = ranges(params)
    assert ((block[..., 0] + u[None, :, 0] > vhi) | (block[..., 0] + u[None, :, 0] < vlo)).any()
    assert (path > raw).any() and (path < raw).any() and (path == raw).any()


def test_every_block_of_a_batch_is_limited_next_to_its_own_u_and_anchor():
    B, n, t = 3, 64, 17
    params = task()
    twin = batch_of(cfg_of(n, t), B, params)
    lim = batch_of(cfg_of(n, t), B, limited(params))
    rng = np.random.default_rng(8)
    u = random_u(rng, t, params, (B,))
    anchors = np.float32([[0.7, -0.4], [0.0, 1.5], [1.9, -3.0]])
    lim.set_u(u)
    lim.set_applied_control(anchors)
    white = draw(twin, B * n, t).reshape(B, n, t, 2)
    got = draw(lim, B * n, t).reshape(B, n, t, 2)
    for b in range(B):
        check_limited(got[b], white[b], u[b], anchors[b], params, "problem %d" % b)
    np.testing.assert_array_equal(lim.applied_control, anchors)
    lim.set_applied_control(ANCHOR)  # (one row: every problem's)
    np.testing.assert_array_equal(lim.applied_control, np.tile(ANCHOR, (B, 1)))


# ---- 2. off is off ---------------------------------------------------------------------------------------------------
def test_no_key_infinite_limits_and_cleared_limits_are_the_unlimited_loop():
    n, t = 130, 17
    params = task(num_opt=2)
    never = planner_of(cfg_of(n, t), params)
    infinite = planner_of(cfg_of(n, t), limited(params, (np.inf, np.inf)))
    cleared = planner_of(cfg_of(n, t), limited(params))
    cleared.move_mppi_task_vars_to_device()  # (handed over ...)
    np.testing.assert_array_equal(cleared.accel_limits, np.float32(ACCEL))
    cleared.set_params(params)               # (... and the key gone again)
    for other in (infinite, cleared):
        other.set_applied_control(ANCHOR)    # (stored whether or not limits are held; nobody reads it)
    for call in range(2):
        want_u = never.solve()
        want_c = never.costs_d.copy_to_host()
        for other, name in ((infinite, "(inf, inf)"), (cleared, "set and cleared")):
            assert_bits(other.solve(), want_u, "u, %s, solve %d" % (name, call))
            assert_bits(other.costs_d.copy_to_host(), want_c, "costs, %s, solve %d" % (name, call))
    assert cleared.accel_limits is None and never.accel_limits is None
    np.testing.assert_array_equal(infinite.accel_limits, np.float32([np.inf, np.inf]))


# ---- 3. the loop consumes the limited block ------------------------------------------------------------------------------
def stage_level_twin(make, params, anchors, iterations):
    """Twin A draws the unlimited blocks; twin B is driven through set_noise(model.limit(block_k, u_k, anchor)), rollout(),
    update(): its costs and u after every iteration."""
    drawer, driven = make(params), make(params)
    B, n, t = drawer.num_instances, drawer.num_control_rollouts, drawer.num_steps
    anchors = np.broadcast_to(anchors, (B, 2))
    out = []
    for _ in range(iterations):
        u = driven.u_cur_d.copy_to_host().reshape(B, t, 2)
        white = draw(drawer, B * n, t).reshape(B, n, t, 2)
        driven.set_noise(np.concatenate([want_block(white[b], u[b], anchors[b], params) for b in range(B)]))
        driven.rollout()
        costs = driven.costs_d.copy_to_host()
        driven.update()
        out.append((costs, driven.u_cur_d.copy_to_host()))
    return out


@pytest.mark.parametrize("family", ["default", "crowd", "batch"])
def test_the_loop_consumes_the_limited_blocks(family):
    anchors = ANCHOR
    if family == "default":
        params, make = task(), lambda p: planner_of(cfg_of(128, 18), p)
    elif family == "crowd":
        params, make = crowd_scene(), lambda p: planner_of(cfg_of(64, 18, crowd=True), p)
    else:
        params, make = task(), lambda p: batch_of(cfg_of(64, 18), 3, p)
        anchors = np.float32([[0.7, -0.4], [0.0, 1.5], [1.9, -3.0]])
    want = stage_level_twin(make, params, anchors, 3)
    on = limited(params)
    stepwise = make(on)
    stepwise.set_applied_control(anchors)
    for k in range(3):
        u = stepwise.solve()
        assert_bits(stepwise.costs_d.copy_to_host(), want[k][0], "%s: costs after iteration %d" % (family, k))
        assert_bits(u, want[k][1], "%s: u after iteration %d" % (family, k))
    if family == "crowd":
        assert stepwise.last_rollout_kernel().startswith("k_rollout_barebone_crowd"), stepwise.last_rollout_kernel()
    loop = make(dict(on, num_opt=3))
    loop.set_applied_control(anchors)
    u = loop.solve()
    assert_bits(loop.costs_d.copy_to_host(), want[2][0], "%s: costs of solve(num_opt = 3)" % family)
    assert_bits(u, want[2][1], "%s: u of solve(num_opt = 3)" % family)
    # (the unlimited loop is another: the twin is not passed by accident)
    assert (make(dict(params, num_opt=3)).solve() != u).any()


# ---- 4. blocks produced ahead ------------------------------------------------------------------------------------------
def test_a_block_produced_ahead_is_limited_before_it_is_consumed():
    """N * T >= 4M: the blocks of the second and third iteration are generated ahead on the second stream, unlimited; the
    main stream waits for the generator, then limits.  The block the third iteration consumed against the model of the
    twin's third block next to the u the second update left, on a strided sample of 64 tiles and the last."""
    n, t = ROUTE_SHAPES["second_stream"]
    params = task(num_opt=3, discs=None)
    twin = planner_of(cfg_of(n, t), params)
    white = [draw(twin, n, t) for _ in range(3)]
    two = planner_of(cfg_of(n, t), limited(dict(params, num_opt=2)))
    two.set_applied_control(ANCHOR)
    u_two = two.solve()
    loop = planner_of(cfg_of(n, t), limited(params))
    loop.set_applied_control(ANCHOR)
    u = loop.solve()
    assert np.isfinite(u).all()
    tiles = n // 64
    rows = (np.arange(0, tiles, max(1, tiles // 64))[:64, None] * 64 + np.arange(64)[None, :]).ravel()
    rows = np.concatenate([rows, np.arange(n - 64, n)])
    got = loop.noise_samples_d.copy_to_host().reshape(n, t, 2)
    check_limited(got[rows], white[2][rows], u_two, ANCHOR, params, "the third iteration's block")


# ---- 5. what it is for -------------------------------------------------------------------------------------------------
def test_the_returned_controls_are_feasible_from_the_applied_control():
    """The notebook's problem.  After each of three solve() + shift_and_update steps the returned sequence is feasible
    within tol from the control applied last; the same run without the key is not."""
    n, t = 1024, 50
    params = task(num_opt=1)
    vr, wr = ranges(params)
    tol, d = model.tolerance(vr, wr, ACCEL, DT), model.step_size(ACCEL, DT).astype(np.float64)
    worst = {}
    for name, p in (("limited", limited(params)), ("unlimited", params)):
        planner = planner_of(cfg_of(n, t, seed=1), p)
        x = np.array(params["x0"], dtype=np.float64)
        anchor = np.zeros(2, dtype=np.float32)
        worst[name] = []
        for step in range(3):
            u = planner.solve()
            if name == "limited":
                np.testing.assert_array_equal(planner.applied_control, anchor)
                excess = model.excess(u, anchor, vr, wr, ACCEL, DT)
                print("step %d: excess %s  tol %s" % (step, excess, tol))
                assert (excess <= tol).all(), (step, excess, tol)
            worst[name].append(model.largest_step(u, anchor))
            x = x + DT * np.array([np.cos(x[2]) * u[0, 0], np.sin(x[2]) * u[0, 0], u[0, 1]], dtype=np.float64)
            planner.shift_and_update(x, u, num_shifts=1)
            anchor = u[0].copy()
    print("largest steps: limited %s  unlimited %s  d %s" % (np.max(worst["limited"], axis=0), np.max(worst["unlimited"], axis=0), d))
    assert (np.max(worst["unlimited"], axis=0) > d).all(), "the unlimited run is feasible too: the test shows nothing"


# ---- 6. closed_loop ------------------------------------------------------------------------------------------------------
def test_closed_loop_equals_the_host_driven_loop_and_is_feasible():
    """As test_gpu_barebone_batch.test_closed_loop_equals_the_notebook_loop compares them, same tolerances."""
    max_steps = 10
    params = limited(task(num_opt=1))
    vr, wr = ranges(params)
    host = planner_of(cfg_of(256, 30, seed=1), params)
    want_x, want_u, want_steps = _notebook_loop(host, host.cfg, params["x0"], params["xgoal"], params["goal_tolerance"], max_steps)
    assert want_steps == max_steps
    dev = planner_of(cfg_of(256, 30, seed=1), params)
    got_x, got_u, got_steps = dev.closed_loop(max_steps)
    assert got_steps == want_steps
    np.testing.assert_allclose(got_u, want_u, rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_x, want_x, rtol=0, atol=1e-5)
    tol = model.tolerance(vr, wr, ACCEL, DT)
    excess = model.excess(got_u, np.zeros(2), vr, wr, ACCEL, DT)
    print("uhist: excess %s  tol %s" % (excess, tol))
    assert (excess <= tol).all(), (excess, tol)
    assert_bits(dev.applied_control, got_u[-1], "the anchor is the last applied row")
    assert_bits(host.applied_control, want_u[-1], "the host-driven loop's likewise")
    unlimited = planner_of(cfg_of(256, 30, seed=1), task(num_opt=1))
    _, white_u, _ = unlimited.closed_loop(max_steps)
    assert (model.excess(white_u, np.zeros(2), vr, wr, ACCEL, DT) > 100 * tol).any(), "the unlimited loop is feasible too"
    assert_bits(unlimited.applied_control, np.zeros(2, dtype=np.float32), "without limits the loop leaves the anchor alone")


def test_closed_loop_of_a_batch_equals_the_host_driven_loop_and_is_feasible():
    B, max_steps = 2, 8
    params = limited(task(num_opt=1))
    vr, wr = ranges(params)
    x0s = np.float32([[0.0, 0.0, np.pi / 4], [1.0, -0.5, 0.3]])
    goals = np.float32([[7.0, 5.0], [6.0, 6.0]])  # (out of reach of eight steps: no problem arrives)

    def make():
        from mppi_numba_amd.barebone import MPPI_Batch
        batch = MPPI_Batch(cfg_of(256, 30, seed=1), B)
        batch.setup(params, x0s, goals)
        return batch
    host = make()
    x = x0s.astype(np.float64)
    want_u = np.zeros((B, max_steps, 2), dtype=np.float32)
    want_x = np.zeros((B, max_steps + 1, 3))
    want_x[:, 0] = x
    for step in range(max_steps):
        useqs = host.solve()
        u0 = useqs[:, 0].astype(np.float64)
        x = x + DT * np.stack([np.cos(x[:, 2]) * u0[:, 0], np.sin(x[:, 2]) * u0[:, 0], u0[:, 1]], axis=1)
        want_u[:, step], want_x[:, step + 1] = useqs[:, 0], x
        host.shift_and_update(x, useqs, num_shifts=1)
    dev = make()
    got_x, got_u, steps = dev.closed_loop(max_steps)
    assert (steps == max_steps).all()
    np.testing.assert_allclose(got_u, want_u, rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_x, want_x, rtol=0, atol=1e-5)
    tol = model.tolerance(vr, wr, ACCEL, DT)
    for b in range(B):
        excess = model.excess(got_u[b], np.zeros(2), vr, wr, ACCEL, DT)
        assert (excess <= tol).all(), (b, excess, tol)
    assert_bits(dev.applied_control, got_u[:, -1], "the anchors are the last applied rows")
    assert (got_u[0, -1] != got_u[1, -1]).any()


# ---- 7. graph replay -----------------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_direct_loops_bits():
    n, t = 128, 18
    params = limited(task(num_opt=5))
    direct, graph = planner_of(cfg_of(n, t), params), planner_of(cfg_of(n, t), params)
    graph.set_graph_replay(True)
    for p in (direct, graph):
        p.set_applied_control(ANCHOR)
    for call in range(3):
        assert_bits(graph.solve(), direct.solve(), "solve %d" % call)
    stats = graph.graph_stats()
    assert stats["captures"] >= 1 and stats["replays"] >= 3, stats
    # a new anchor: device memory the captured launch reads at replay -- no capture
    for p in (direct, graph):
        p.set_applied_control([0.2, 0.9])
    assert_bits(graph.solve(), direct.solve(), "a new anchor")
    assert graph.graph_stats()["captures"] == stats["captures"]
    other = planner_of(cfg_of(n, t), params)
    other.set_applied_control(ANCHOR)
    for call in range(4):
        kept = other.solve()
    assert (kept != graph.u_cur_d.copy_to_host()).any(), "the new anchor changed nothing"
    # the same values again, past the key cache: nothing is dropped
    from mppi_numba_amd import _lib
    same = np.float32(ACCEL)
    _lib.call("mppi_planner_set_control_limits", graph._handle, _lib.ptr(same, C.c_float))
    assert_bits(graph.solve(), direct.solve(), "the same values again")
    assert graph.graph_stats()["captures"] == stats["captures"]
    # a changed limit: exactly one more capture, the direct loop's bits
    for p in (graph, direct):
        p.set_params(limited(task(num_opt=5), (1.0, 0.5)))
    assert_bits(graph.solve(), direct.solve(), "a changed limit")
    assert graph.graph_stats()["captures"] == stats["captures"] + 1
    assert_bits(graph.solve(), direct.solve(), "... and the solve after it")
    assert graph.graph_stats()["captures"] == stats["captures"] + 1


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    n, t = 130, 17
    params = limited(task(), (0.5, 2.5))
    planner, twin = planner_of(cfg_of(n, t), params), planner_of(cfg_of(n, t), params)
    for p in (planner, twin):
        p.set_applied_control(ANCHOR)
    assert_bits(planner.solve(), twin.solve(), "before")
    for bad in (0.0, -1.0, np.nan, -np.inf, (0.5, 0.0), (np.nan, np.inf)):
        planner.set_params(limited(task(), bad))
        with pytest.raises(_lib.MppiError, match="control limit"):
            planner.solve()
        np.testing.assert_array_equal(planner.accel_limits, np.float32([0.5, 2.5]))
    for shape in ((3,), (1,), (2, 2)):
        planner.set_params(limited(task(), np.full(shape, 0.5)))
        with pytest.raises(ValueError, match="accel_limits"):
            planner.solve()
    # an anchor that is not finite, or of the wrong shape
    for bad in ((np.nan, 0.0), (0.0, np.inf)):
        with pytest.raises(_lib.MppiError, match="finite"):
            planner.set_applied_control(bad)
    for shape in ((3,), (2, 2), (1, 3)):
        with pytest.raises(ValueError, match="applied control"):
            planner.set_applied_control(np.zeros(shape))
    np.testing.assert_array_equal(planner.applied_control, ANCHOR)
    planner.set_params(params)
    np.testing.assert_array_equal(planner.accel_limits, np.float32([0.5, 2.5]))
    assert_bits(planner.solve(), twin.solve(), "the solve after the refusals")
    # the stage hook without limits
    plain = planner_of(cfg_of(n, t), task())
    with pytest.raises(_lib.MppiError, match="no control limits"):
        plain.limit_noise()
    # a map mode
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    accel = np.float32([1.0, 1.0])
    with pytest.raises(_lib.MppiError, match="barebone"):
        _lib.call("mppi_planner_set_control_limits", mapped._handle, _lib.ptr(accel, C.c_float))
    with pytest.raises(_lib.MppiError, match="barebone"):
        _lib.call("mppi_planner_set_control_limits", mapped._handle, None)
    with pytest.raises(_lib.MppiError, match="barebone"):
        _lib.call("mppi_planner_set_applied_control", mapped._handle, 1, _lib.ptr(accel, C.c_float))
