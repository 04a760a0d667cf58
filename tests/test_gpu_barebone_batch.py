"""Batched barebone planning (barebone.MPPI_Batch): B problems of the disc-obstacle planner of
barebone_mppi_numba.ipynb in one handle, each with its own start, goal and -- optionally -- its own disc set,
plus the notebook's control loop (cell 7) on the device.

The batch is not in the reference, so its oracle is two-fold: every problem must be bit-identical to a
single-problem barebone handle fed the same discs, controls and noise, and its costs must match the C
restatement of the notebook's rollout kernel (oracle/)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID = -1


def make_cfg(n, t, dt=0.1, seed=3, v=4):
    from mppi_numba_amd.barebone import Config
    cfg = Config(T=(t + 0.5) * dt, dt=dt, num_control_rollouts=n, num_vis_state_rollouts=v, seed=seed,
                 enforce_recommended_limits=False)
    assert cfg.num_steps == t and cfg.num_control_rollouts == n
    return cfg


def make_params(dt, wscale, discs=None, num_opt=1):
    """The notebook's cell 5 task; wscale * pi * dt on either side of 0.36 rad picks the heading's rotation or sincos."""
    p = dict(dt=dt, x0=np.array([0.0, 0.0, np.pi / 4]), xgoal=np.array([7.0, 5.0]), goal_tolerance=0.5, dist_weight=10,
             lambda_weight=1.0, num_opt=num_opt, u_std=np.array([1.0, 1.0]), vrange=np.array([0.0, 2.0]),
             wrange=np.array([-np.pi, np.pi]) * wscale, obs_penalty=1e6)
    if discs is not None:
        p["obstacle_positions"], p["obstacle_radius"] = discs
    return p


def problems(rng, count):
    x0s = np.stack([rng.uniform(-1, 1, count), rng.uniform(-1, 1, count), rng.uniform(-np.pi, np.pi, count)],
                   axis=1).astype(np.float32)
    goals = (x0s[:, :2] + rng.uniform(1.0, 6.0, (count, 2))).astype(np.float32)
    goals[-1] = x0s[-1, :2] + 0.8  # one goal within reach of the horizon
    return x0s, goals


def random_discs(rng, count, x0, goal):
    """`count` discs around the segment start -> goal (so that rollouts hit some of them)."""
    s = rng.uniform(0, 1, (count, 1))
    pos = (x0[:2] * (1 - s) + goal * s + rng.normal(0, 0.5, (count, 2))).astype(np.float32)
    rad = rng.uniform(0.2, 0.8, count).astype(np.float32)
    return pos, rad


def oracle_params(params):
    return O.make_params(params, 1.0, [0, 0], [0, 0], [0.0, 1.0], [0.0, 1.0], default_obs_cost=1e3, default_dist_weight=10)


def run_batch(batch, rng):
    """A solve, then per-problem warm starts and fresh noise, one rollout and one update: what the checks compare."""
    useqs = batch.solve()
    assert useqs.shape == (batch.num_instances, batch.num_steps, 2) and np.isfinite(useqs).all()
    u_in = (useqs + rng.normal(0, 0.05, useqs.shape)).astype(np.float32)
    batch.set_u(u_in)
    batch.sample_noise()
    noise = batch.noise_samples_d.copy_to_host().reshape(batch.num_instances, batch.num_control_rollouts, batch.num_steps, 2)
    batch.rollout()
    costs = batch.costs_d.copy_to_host()
    kernel = batch.last_rollout_kernel()
    batch.update()
    return u_in, noise, costs, kernel, batch.u_cur_d.copy_to_host(), batch.weights_d.copy_to_host()


def single_run(single, params, u, noise):
    single.set_params(params)
    single.set_u(u)
    single.set_noise(noise)
    single.rollout()
    costs = single.costs_d.copy_to_host()
    single.update()
    return costs, single.u_cur_d.copy_to_host(), single.weights_d.copy_to_host()


def problem_params(params, x0, goal, discs=None):
    p = dict(params)
    p["x0"], p["xgoal"] = np.asarray(x0, dtype=np.float32), np.asarray(goal, dtype=np.float32)
    if discs is not None:
        p.pop("obstacle_positions", None)
        p.pop("obstacle_radius", None)
        if len(discs[1]):
            p["obstacle_positions"], p["obstacle_radius"] = discs
    return p


def assert_bits(got, want, what):
    assert (got.view(np.int32) == want.view(np.int32)).all(), "%s: %d of %d differ" % (what, (got != want).sum(), got.size)


def check_update_vs_oracle(params, costs, noise, u_in, u_out):
    _, u_ref, _ = O.update_useq(params["lambda_weight"], costs, noise, params["vrange"], params["wrange"], u_in)
    span = np.array([np.ptp(params["vrange"]), np.ptp(params["wrange"])])
    assert (np.abs(u_out - u_ref) / span).max() <= 1e-5


@pytest.mark.parametrize("B,n,t,n_discs,wscale", [
    (2, 64, 30, 0, 1.0),      # rotation (pi * 0.1 <= 0.36), no discs
    (5, 1024, 50, 2, 1.0),    # the notebook's shape per problem: KD = 2 form
    (64, 64, 50, 3, 1.0),     # KD = 4 form, many problems
    (5, 64, 30, 7, 1.0),      # run-time disc loop
    (2, 1024, 30, 2, 1.5),    # full sincos (1.5 pi * 0.1 > 0.36)
    (64, 1024, 50, 2, 1.0),   # 1024 workgroups
    (5, 64, 50, 3, 2.0),      # full sincos with discs
])
def test_batch_matches_single_handles_and_oracle(B, n, t, n_discs, wscale):
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    rng = np.random.default_rng(B * 1000 + n + t + n_discs)
    cfg = make_cfg(n, t)
    x0s, goals = problems(rng, B)
    discs = random_discs(rng, n_discs, x0s[0], goals[0]) if n_discs else None
    params = make_params(cfg.dt, wscale, discs)
    batch = MPPI_Batch(cfg, B)
    batch.setup(params, x0s, goals)
    u_in, noise, costs, kernel, u_out, weights = run_batch(batch, rng)
    assert costs.shape == (B, n) and u_out.shape == (B, t, 2)
    assert kernel.startswith("k_rollout_barebone") and "problems=%d" % B in kernel, kernel
    assert ("rotation=1" in kernel) == (wscale == 1.0), kernel
    assert np.allclose(weights.sum(axis=1), 1.0, atol=1e-5)
    single = MPPI_Numba(cfg)
    for b in range(B):
        p = problem_params(params, x0s[b], goals[b])
        want, want_u, want_w = single_run(single, p, u_in[b], noise[b])
        assert "problems" not in single.last_rollout_kernel()
        assert_bits(costs[b], want, "problem %d costs vs single handle" % b)
        assert_bits(u_out[b], want_u, "problem %d u vs single handle" % b)
        assert_bits(weights[b], want_w, "problem %d weights vs single handle" % b)
        pos, rad = discs if discs is not None else (np.zeros((0, 2), np.float32), np.zeros(0, np.float32))
        ref = O.rollout_barebone(oracle_params(p), pos, rad, noise[b], u_in[b])
        assert_bits(costs[b], ref, "problem %d costs vs oracle" % b)
        check_update_vs_oracle(p, costs[b], noise[b], u_in[b], u_out[b])


@pytest.mark.parametrize("counts,form", [
    ([2, 0, 1, 2, 0], "discs<=2"),
    ([4, 0, 2, 3, 1], "discs<=4"),
    ([33, 0, 5, 2, 17], "discs=loop"),
])
def test_per_problem_disc_sets(counts, form):
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    B, n, t = len(counts), 128, 30
    rng = np.random.default_rng(sum(counts))
    cfg = make_cfg(n, t)
    x0s, goals = problems(rng, B)
    shared = random_discs(rng, 2, x0s[0], goals[0])
    params = make_params(cfg.dt, 1.0, shared)
    sets = [random_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate(counts)]
    batch = MPPI_Batch(cfg, B)
    batch.setup(params, x0s, goals, obstacle_sets=sets)
    u_in, noise, costs, kernel, u_out, _ = run_batch(batch, rng)
    assert form in kernel and "problems=%d" % B in kernel and "rotation=1" in kernel, kernel
    single = MPPI_Numba(cfg)
    for b in range(B):
        p = problem_params(params, x0s[b], goals[b], sets[b])
        want, want_u, _ = single_run(single, p, u_in[b], noise[b])
        assert_bits(costs[b], want, "problem %d (%d discs) vs single handle" % (b, counts[b]))
        assert_bits(u_out[b], want_u, "problem %d u vs single handle" % b)
        assert_bits(costs[b], O.rollout_barebone(oracle_params(p), sets[b][0], sets[b][1], noise[b], u_in[b]),
                    "problem %d vs oracle" % b)
    if counts[0] >= 4:
        assert (costs[0] > 1e5).any(), "some rollouts of the problem with the most discs must hit one"
    # the same sets again: a comparison, no new upload, no change
    batch.set_obstacle_sets(sets)
    batch.set_u(u_in)
    batch.rollout()
    assert_bits(batch.costs_d.copy_to_host(), costs, "same sets again")
    # back to the shared set (count = 0)
    batch.set_obstacle_sets(None)
    batch.set_u(u_in)
    batch.rollout()
    assert "discs<=2" in batch.last_rollout_kernel() and "own_discs" not in batch.last_rollout_kernel()
    back = batch.costs_d.copy_to_host()
    for b in range(B):
        p = problem_params(params, x0s[b], goals[b])
        assert_bits(back[b], O.rollout_barebone(oracle_params(p), shared[0], shared[1], noise[b], u_in[b]),
                    "problem %d, shared set again" % b)


def test_instance_path_with_one_problem_equals_the_classic_path():
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    rng = np.random.default_rng(7)
    cfg = make_cfg(1000, 50)  # the notebook's shape: N not a multiple of 64 is fine for one problem
    params = make_params(cfg.dt, 1.0, (np.array([[5, 4.5], [2, 1]]), np.array([1.5, 1.0])))
    classic = MPPI_Numba(cfg)
    classic.setup(params)
    batch = MPPI_Batch(cfg, 1)
    batch.setup(params)
    u0 = classic.solve()
    np.testing.assert_array_equal(batch.solve(), u0)
    assert "problems=1" in batch.last_rollout_kernel() and "problems" not in classic.last_rollout_kernel()
    u_in = (u0 + rng.normal(0, 0.05, u0.shape)).astype(np.float32)
    for planner in (classic, batch):
        planner.set_u(u_in)
    batch.sample_noise()
    noise = batch.noise_samples_d.copy_to_host()
    classic.set_noise(noise)
    for planner in (classic, batch):
        planner.rollout()
        planner.update()
    assert_bits(batch.costs_d.copy_to_host(), classic.costs_d.copy_to_host(), "costs")
    assert_bits(batch.u_cur_d.copy_to_host(), classic.u_cur_d.copy_to_host(), "u")


def _notebook_loop(planner, cfg, x0, xgoal, tol, max_steps):
    """barebone_mppi_numba.ipynb cell 7, verbatim arithmetic, in float64 as the notebook's NumPy 1 evaluated it (under
    NumPy 2's promotion rules, NEP 50, cfg.dt * u_curr[1] of a float32 u_curr would be rounded to float32)."""
    xhist = np.zeros((max_steps + 1, 3)) * np.nan
    uhist = np.zeros((max_steps, 2), dtype=np.float32) * np.nan
    xhist[0] = x0
    steps = max_steps
    for t in range(max_steps):
        useq = planner.solve()
        uhist[t] = useq[0]
        u_curr = useq[0].astype(np.float64)
        xhist[t + 1, 0] = xhist[t, 0] + cfg.dt * np.cos(xhist[t, 2]) * u_curr[0]
        xhist[t + 1, 1] = xhist[t, 1] + cfg.dt * np.sin(xhist[t, 2]) * u_curr[0]
        xhist[t + 1, 2] = xhist[t, 2] + cfg.dt * u_curr[1]
        planner.shift_and_update(xhist[t + 1], useq, num_shifts=1)
        if np.linalg.norm(xhist[t + 1, :2] - xgoal) <= tol:
            steps = t + 1
            break
    return xhist, uhist, steps


@pytest.mark.parametrize("max_steps", [60, 20])
def test_closed_loop_equals_the_notebook_loop(max_steps):
    """60 steps: the goal is reached on the way (NaN tail).  20 steps: the loop runs to its end, and then the handle is
    where the notebook's loop leaves it -- the same next solve.  (A loop that ends early has run the solves up to the
    host's next look at the goal flags: they advanced the noise generator's counters, see mppi.MPPI_Numba.closed_loop.)"""
    from mppi_numba_amd.barebone import MPPI_Numba
    cfg = make_cfg(1000, 50, seed=1)
    params = make_params(cfg.dt, 1.0, (np.array([[5, 4.5], [2, 1]]), np.array([1.5, 1.0])))
    host = MPPI_Numba(cfg)
    host.setup(params)
    want_x, want_u, want_steps = _notebook_loop(host, cfg, params["x0"], params["xgoal"], params["goal_tolerance"],
                                                max_steps)
    assert (want_steps < max_steps) == (max_steps == 60)
    dev = MPPI_Numba(make_cfg(1000, 50, seed=1))
    dev.setup(params)
    got_x, got_u, got_steps = dev.closed_loop(max_steps)
    assert got_x.shape == (max_steps + 1, 3) and got_u.shape == (max_steps, 2)
    assert got_steps == want_steps
    ran = want_steps
    np.testing.assert_array_equal(np.isnan(got_x), np.isnan(want_x))
    np.testing.assert_allclose(got_u[:ran], want_u[:ran], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_x[:ran + 1], want_x[:ran + 1], rtol=0, atol=1e-5)
    assert np.linalg.norm(got_x[ran, :2] - params["xgoal"]) < np.linalg.norm(params["x0"][:2] - params["xgoal"])
    np.testing.assert_allclose(dev.params["x0"], got_x[ran])
    if ran == max_steps:
        np.testing.assert_allclose(dev.solve(), host.solve(), rtol=0, atol=2e-5)


def test_closed_loop_of_a_batch_with_own_discs():
    from mppi_numba_amd.barebone import MPPI_Batch
    B, max_steps = 3, 40
    rng = np.random.default_rng(21)
    cfg = make_cfg(256, 30)
    x0s, goals = problems(rng, B)
    sets = [random_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate((1, 0, 6))]
    params = make_params(cfg.dt, 1.0)
    batch = MPPI_Batch(cfg, B)
    batch.setup(params, x0s, goals, obstacle_sets=sets)
    xhist, uhist, steps = batch.closed_loop(max_steps)
    assert xhist.shape == (B, max_steps + 1, 3) and uhist.shape == (B, max_steps, 2) and steps.shape == (B,)
    for b in range(B):
        k = int(steps[b])
        x, u = xhist[b], uhist[b].astype(np.float64)
        np.testing.assert_allclose(x[0], x0s[b].astype(np.float64))
        want = np.stack([x[:k, 0] + cfg.dt * np.cos(x[:k, 2]) * u[:k, 0],
                         x[:k, 1] + cfg.dt * np.sin(x[:k, 2]) * u[:k, 0],
                         x[:k, 2] + cfg.dt * u[:k, 1]], axis=1)
        np.testing.assert_allclose(x[1:k + 1], want, rtol=0, atol=1e-12)
        assert np.isnan(x[k + 1:]).all() and np.isnan(uhist[b, k:]).all()
        assert np.linalg.norm(x[k, :2] - goals[b]) < np.linalg.norm(x0s[b, :2] - goals[b]), b
        np.testing.assert_array_equal(batch.x0s[b], x[k].astype(np.float32))
    assert steps[-1] < max_steps  # (the goal within reach is reached)


def test_state_rollouts_per_problem():
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t, v = 4, 128, 30, 8
    rng = np.random.default_rng(5)
    cfg = make_cfg(n, t, v=v)
    x0s, goals = problems(rng, B)
    params = make_params(cfg.dt, 1.0, random_discs(rng, 2, x0s[0], goals[0]))
    batch = MPPI_Batch(cfg, B)
    batch.setup(params, x0s, goals)
    batch.solve()
    noise = batch.noise_samples_d.copy_to_host().reshape(B, n, t, 2)
    u_prev, u_cur = batch.u_prev_d.copy_to_host(), batch.u_cur_d.copy_to_host()
    for b in range(B):
        got = batch.get_state_rollout(b)
        assert got.shape == (v, t + 1, 3)
        np.testing.assert_array_equal(got[:, 0], np.tile(x0s[b], (v, 1)))
        want = O.state_rollout_barebone(oracle_params(problem_params(params, x0s[b], goals[b])), noise[b], u_prev[b],
                                        u_cur[b], v)
        assert_bits(got, want, "problem %d state rollouts" % b)


def test_graph_replay_of_a_batch():
    from mppi_numba_amd.barebone import MPPI_Batch
    B = 4
    rng = np.random.default_rng(9)
    cfg = make_cfg(128, 30)
    x0s, goals = problems(rng, B)
    sets = [random_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate((2, 0, 3, 1))]
    params = make_params(cfg.dt, 1.0, num_opt=5)
    direct, graphed = MPPI_Batch(cfg, B), MPPI_Batch(make_cfg(128, 30), B)
    for planner in (direct, graphed):
        planner.setup(params, x0s, goals, obstacle_sets=sets)
    graphed.set_graph_replay(True, 2)
    for _ in range(3):
        np.testing.assert_array_equal(direct.solve(), graphed.solve())
    stats = graphed.graph_stats()
    assert stats["captures"] >= 1 and stats["replays"] >= 4, stats
    # one problem's discs change: the graph's launches held the old arrays -> recapture
    sets[1] = random_discs(rng, 4, x0s[1], goals[1])
    for planner in (direct, graphed):
        planner.set_obstacle_sets(sets)
    for _ in range(2):
        np.testing.assert_array_equal(direct.solve(), graphed.solve())
    after = graphed.graph_stats()
    assert after["captures"] > stats["captures"] and after["replays"] > stats["replays"], (stats, after)
    assert "discs<=4" in graphed.last_rollout_kernel()


def test_errors():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    cfg = make_cfg(128, 30)
    batch = MPPI_Batch(cfg, 3)
    batch.setup(make_params(cfg.dt, 1.0), *problems(np.random.default_rng(1), 3))
    lib = _lib.load()

    def rc_of(handle, count, counts, pos, rad):
        c = np.ascontiguousarray(counts, dtype=np.int32)
        p_ = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 2)
        r_ = np.ascontiguousarray(rad, dtype=np.float32).reshape(-1)
        rc = lib.mppi_planner_set_instance_disc_obstacles(handle, count, _lib.ptr(c, C.c_int), _lib.ptr(p_, C.c_float),
                                                          _lib.ptr(r_, C.c_float))
        return rc, lib.mppi_last_error().decode()

    rc, msg = rc_of(batch._handle, 2, [1, 1], np.zeros((2, 2)), np.ones(2))
    assert rc == ERR_INVALID and "num_instances" in msg, msg
    rc, msg = rc_of(batch._handle, 3, [1, -1, 1], np.zeros((1, 2)), np.ones(1))
    assert rc == ERR_INVALID and "negative" in msg, msg
    big = 4100  # 16 * 30 + 16 * 4100 > 64 KiB
    rc, msg = rc_of(batch._handle, 3, [1, big, 0], np.zeros((big + 1, 2)), np.ones(big + 1))
    assert rc == ERR_INVALID and "LDS" in msg, msg
    batch.solve()  # the handle is unharmed
    # a barebone batch still needs N to be a multiple of 64
    with pytest.raises(_lib.MppiError) as err:
        MPPI_Batch(make_cfg(100, 30), 2)
    assert err.value.code == ERR_INVALID and "multiple of 64" in str(err.value)
    # discs in a map mode; closed_loop without a world in a map mode
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    planner = MapPlanner(mcfg)
    planner.setup(mparams, lin, ang)
    rc, msg = rc_of(planner._handle, 1, [1], np.zeros((1, 2)), np.ones(1))
    assert rc == ERR_INVALID and "barebone" in msg, msg
    x = np.zeros((1, 3), np.float32)
    g = np.ones((1, 2), np.float32)
    lib.mppi_planner_set_instances(planner._handle, 1, _lib.ptr(x, C.c_float), _lib.ptr(g, C.c_float))
    xh, uh, st = np.zeros((2, 3)), np.zeros((1, 2), np.float32), np.zeros(1, np.int32)
    rc = lib.mppi_planner_closed_loop(planner._handle, lin._handle, ang._handle, None, 1, 0.1, 0.5, None,
                                      _lib.ptr(xh, C.c_double), _lib.ptr(uh, C.c_float), _lib.ptr(st, C.c_int))
    assert rc == ERR_INVALID and "world" in lib.mppi_last_error().decode()
    # a single barebone handle without discs of its own is unaffected
    single = MPPI_Numba(cfg)
    single.setup(make_params(cfg.dt, 1.0))
    assert np.isfinite(single.solve()).all()


@pytest.mark.parametrize("kind", ["static", "tracks"])
def test_a_set_handed_back_gives_the_first_result(kind):
    """A hand-over builds the new device arrays before it frees the old ones (csrc/barebone_api.h, staged upload).  A set
    of 2 discs per problem, one of 5, the first again: the third result is the first one's bit for bit, nothing of the
    set in between is left.  tracks: crowd mode, so that the [row][disc] copy goes the same way."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t, L = 2, 64, 8, 3
    rng = np.random.default_rng(77)
    cfg = make_cfg(n, t)
    cfg.crowd = kind == "tracks"
    x0s, goals = problems(rng, B)
    params = make_params(cfg.dt, 1.0)

    def sets_of(count):
        # (within the 1.6 m the 8 steps can cover, so that rollouts hit them)
        sets = [((x0s[b, :2] + rng.uniform(-1.2, 1.2, (count, 2))).astype(np.float32),
                 rng.uniform(0.3, 0.7, count).astype(np.float32)) for b in range(B)]
        if kind == "static":
            return sets
        return [((pos[:, None, :] + 0.1 * np.arange(L)[None, :, None]).astype(np.float32), rad) for pos, rad in sets]

    small, large = sets_of(2), sets_of(5)
    batch = MPPI_Batch(cfg, B)
    batch.setup(params, x0s, goals, small)
    u_in = rng.normal(0.5, 0.2, (B, t, 2)).astype(np.float32)
    noise = rng.normal(0, 1, (B, n, t, 2)).astype(np.float32)

    def result(sets):
        batch.set_obstacle_sets(sets)
        batch.set_u(u_in)
        batch.set_noise(noise)
        batch.rollout()
        costs, kernel = batch.costs_d.copy_to_host(), batch.last_rollout_kernel()
        batch.update()
        return costs, batch.u_cur_d.copy_to_host(), kernel

    first, between, again = result(small), result(large), result(small)
    tail = " tracks=%d problems=%d" % (L, B) if kind == "tracks" else " own_discs=1 problems=%d" % B
    assert first[2] == "k_rollout_barebone exact=1 rotation=1 discs<=2" + tail, first[2]
    assert between[2].startswith("k_rollout_barebone_crowd" if kind == "tracks" else "k_rollout_barebone exact=1 rotation=1 discs=loop"), between[2]
    assert again[2] == first[2]
    assert (between[0] != first[0]).any(), "bad input: the larger sets change no cost"
    assert_bits(again[0], first[0], "costs with the first sets handed back")
    assert_bits(again[1], first[1], "controls with the first sets handed back")
