"""The map border on the device: rollouts that leave the map, starts on its edge and outside it, in every kernel family.

A cell index that is off the map is CLAMPED to the border cell (deliberate deviations; the clamp is
written out once per kernel).  The worlds of tests/border_cases.py have no zero-traction ring, so the rollouts do leave,
and carry the copy property, so the oracle -- which clamps on the high side and wraps on the low side -- is the clamp's
reference on both (tests/test_border_cases.py holds the inputs to that on the CPU).

One case: solve() once from a start on the map (an outside start: from the nearest point on it -- solve() refuses an
outside start, params["x0"] and the stage-level calls do not), then sample_noise(), the noise and the controls read
back, rollout(), the costs against the oracle, and the kernel family by name.  Exact-math kernels are held bit for bit.

The last test is the planner's own maps (the reference's ring): a start OUTSIDE the ring must take the clamped address
(map_plan.h: map_unclamped_ok looks at the start cell), where the unclamped one would index past the LDS window.
"""
import ctypes as C

import numpy as np
import pytest

import border_cases as BC
from mppi_numba_amd import _lib
from oracle import oracle as O
from scan_exact_model import scan_exact_rollout

pytestmark = pytest.mark.gpu

DET, SPEED, TDM = dict(use_det_dynamics=True), dict(use_nom_dynamics_with_speed_map=True), dict(use_tdm=True)
NO_SPECULATION, NO_SCAN_KERNEL = _lib.DEBUG_NO_SPECULATION, _lib.DEBUG_NO_SCAN_KERNEL
N = 96  # three tiles of 32 rollouts

WORLDS = {}


def the_world(kind, **kw):
    key = (kind,) + tuple(sorted(kw.items()))
    if key not in WORLDS:
        WORLDS[key] = BC.world(kind, **kw)
    return WORLDS[key]


def make(w, mode=DET, n=N, t=BC.T_STEPS, m=1, math="exact", pad_speed=0.0, vis=1):
    """(cfg, lin, ang, planner) over a world; pad_speed = 0: no ring, the map's own dims."""
    from mppi_numba_amd.config import Config
    from mppi_numba_amd.mppi import MPPI_Numba
    from mppi_numba_amd.terrain import TDM_Numba
    pad = int(np.ceil(pad_speed * BC.DT / w["res"]))
    cfg = Config(T=t * BC.DT + 0.05, dt=BC.DT, num_grid_samples=m, num_control_rollouts=n, max_speed_padding=pad_speed,
                 num_vis_state_rollouts=vis, max_map_dim=(w["rows"] + 2 * pad, w["cols"] + 2 * pad), seed=5,
                 enforce_recommended_limits=False, math=math, **mode)
    assert cfg.num_steps == t, cfg.num_steps
    lin, ang = TDM_Numba(cfg), TDM_Numba(cfg)
    speed = mode is SPEED
    lin.set_TDM_from_PMF_grid(w["risk_pmf"] if speed else w["lin_pmf"], w["td"], w["obstacle"], w["unknown"])
    ang.set_TDM_from_PMF_grid(w["ang_pmf"], w["td"], w["obstacle"], w["unknown"])
    assert lin.pad_cells == pad
    return cfg, lin, ang, MPPI_Numba(cfg)


def on_the_map(w, x0):
    """The nearest point of the map's interior (0.4 of a cell inside the border where the start is outside)."""
    out = np.array(x0, dtype=float)
    out[0] = np.clip(out[0], w["xlimits"][0] + 0.4 * w["res"], w["xlimits"][1] - 0.6 * w["res"])
    out[1] = np.clip(out[1], w["ylimits"][0] + 0.4 * w["res"], w["ylimits"][1] - 0.6 * w["res"])
    return out


def layers(lin, ang, speed=False):
    return (lin.sample_grid_batch_d.copy_to_host(), ang.sample_grid_batch_d.copy_to_host(), lin.obstacle_map_d.copy_to_host(),
            lin.unknown_map_d.copy_to_host(), lin.risk_traction_map_d.copy_to_host() if speed else None)


def check_layers(w, got, speed=False, m=1):
    """The device arrived at the world's layers: what tests/test_border_cases.py held on the CPU is what runs here."""
    lin, ang, obs, unk, risk = got
    assert lin.shape == (m, w["rows"], w["cols"])  # the oracle's stride is the map's columns
    for g in range(m):
        assert np.array_equal(lin[g], np.full_like(w["lin"][0], w["nominal_byte"]) if speed else w["lin"][0])
        assert np.array_equal(ang[g], np.full_like(w["ang"][0], w["nominal_byte"]) if speed else w["ang"][0])
    assert np.array_equal(obs, w["obstacle"]) and np.array_equal(unk, w["unknown"])
    if speed:
        assert np.array_equal(risk.reshape(w["rows"], w["cols"]), w["risk"][0])


def oracle_params(params, lin, ang):
    return O.make_params(params, lin.res, lin.padded_xlimits, lin.padded_ylimits, lin.bin_values_bounds_d.copy_to_host(),
                         ang.bin_values_bounds_d.copy_to_host())


def oracle_costs(params, lin, ang, got_layers, noise, u, tdm=False):
    lin_g, ang_g, obs, unk, risk = got_layers
    p = oracle_params(params, lin, ang)
    if tdm:
        return O.rollout_tdm(p, lin_g, ang_g, obs, unk, noise, u)
    return O.rollout_det(p, lin_g, ang_g, obs, unk, noise, u, risk=risk)


def prepared(w, name, mode=DET, flags=0, solve=True, **kw):
    """A planner that has solved once from the named start (from the nearest point on the map where it is outside) and
    now stands at the start itself.  solve=False: the grids drawn by hand and controls that drive ahead -- a planner
    that knows nothing about its map yet."""
    cfg, lin, ang, planner = make(w, mode=mode, **{k: v for k, v in kw.items() if k in ("n", "t", "m", "math", "vis")})
    params = BC.params(w, name, **{k: v for k, v in kw.items() if k in ("vrange", "wrange")})
    x0 = params["x0"].copy()
    if "far_goal" in kw:  # metres ahead
        params["xgoal"] = x0[:2] + kw["far_goal"] * np.array([np.cos(x0[2]), np.sin(x0[2])])
    planner.setup(dict(params, x0=on_the_map(w, x0)), lin, ang)
    if flags:
        planner.set_debug_flags(flags)
    if solve:
        u0 = planner.solve()
        assert u0 is not None and np.isfinite(u0).all()
    else:
        lin.sample_grids()
        ang.sample_grids()
        planner.set_u(np.tile(np.array([1.5, 0.1], dtype=np.float32), (cfg.num_steps, 1)))
    planner.params["x0"] = x0
    return cfg, lin, ang, planner, params


def rolled_out(planner):
    planner.sample_noise()
    noise, u_in = planner.noise_samples_d.copy_to_host(), planner.u_cur_d.copy_to_host()
    planner.rollout()
    return noise, u_in, planner.costs_d.copy_to_host(), planner.last_rollout_kernel()


def assert_bits(got, want, what):
    assert np.isfinite(want).all()
    assert np.array_equal(got, want), "%s: %d of %d costs differ, first at %s" % (
        what, int((got != want).sum()), got.size, np.flatnonzero(got != want)[:4])


def exact_case(family, name, mode=DET, flags=0, tokens=(), absent=(), kind=None, **kw):
    """One exact-math case of a family of tests/border_cases.py: GPU_CASES.  Returns what a test may want to look at."""
    kind = kind or BC.GPU_CASES[family][0]
    w = the_world(kind)
    speed, tdm = mode is SPEED, mode is TDM
    cfg, lin, ang, planner, params = prepared(w, name, mode=mode, flags=flags, **kw)
    got_layers = layers(lin, ang, speed)
    check_layers(w, got_layers, speed, m=kw.get("m", 1))
    noise, u_in, got, kernel = rolled_out(planner)
    print("\n%s from %s: %s" % (family, name, kernel))
    for token in tokens:
        assert token in kernel, (token, kernel)
    for token in absent:
        assert token not in kernel, (token, kernel)
    want = oracle_costs(params, lin, ang, got_layers, noise, u_in, tdm=tdm)
    assert_bits(got, want, "%s %s %s" % (family, name, kernel))
    return dict(w=w, lin=lin, ang=ang, planner=planner, params=params, layers=got_layers, noise=noise, u=u_in, want=want)


# ---- the time-parallel kernel, exact arithmetic ------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [(s, N) for s in BC.GPU_CASES["scan_exact"][1]] + [("corner_hihi", 70)])
def test_scan_exact_speculative(name, n):
    """One traction value everywhere: the vote holds, the walks' lookups (scan_lookup) are what clamps.  n = 70: a ragged
    last tile."""
    exact_case("scan_exact", name, n=n, tokens=["k_rollout_scan_exact tile=32", "pow2res=0"], absent=["speed_map", "direct=1"])


@pytest.mark.parametrize("name", BC.GPU_CASES["scan_exact_reexecuted"][1])
def test_scan_exact_reexecuted_tiles(name):
    """Traction that changes from cell to cell, no debug flag and a planner that has not looked at its map yet: every tile
    fails its vote and is re-executed on the exact schedule inside the kernel (PipeWindow<false>: the clamp)."""
    r = exact_case("scan_exact_reexecuted", name, solve=False, tokens=["k_rollout_scan_exact tile=32", "pow2res=0"],
                   absent=["speed_map", "direct=1"])
    lin_g, ang_g, obs, unk, _ = r["layers"]
    _, failed = scan_exact_rollout(oracle_params(r["params"], r["lin"], r["ang"]), lin_g, ang_g, obs, unk, r["noise"], r["u"])
    assert failed.all()  # (the model of the kernel's vote: every tile of 32 is one that was re-executed)


@pytest.mark.parametrize("name", BC.GPU_CASES["scan_exact_direct"][1])
def test_scan_exact_direct(name):
    exact_case("scan_exact_direct", name, flags=NO_SPECULATION, tokens=["k_rollout_scan_exact tile=32", "pow2res=0", "direct=1"])


@pytest.mark.parametrize("name", BC.GPU_CASES["speed_map"][1])
def test_speed_map_kernels(name):
    """The speed-map forms: k_rollout_scan_exact (map_plan.h: "its lookups all clamp" -- pow2res is its cell arithmetic
    alone, also for an outside start) and, without the time-parallel kernel, k_rollout_fused; the risk layer has the
    copy property like every other."""
    r = exact_case("speed_map", name, mode=SPEED, tokens=["k_rollout_scan_exact speed_map", "pow2res=1"])
    planner = r["planner"]
    planner.set_debug_flags(NO_SCAN_KERNEL)
    planner.rollout()
    assert "k_rollout_fused speed_map" in planner.last_rollout_kernel(), planner.last_rollout_kernel()
    assert_bits(planner.costs_d.copy_to_host(), r["want"], "fused speed_map %s" % name)


# ---- the exact three-wave pipeline -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.GPU_CASES["pipe"][1])
def test_pipe_clipped_by_a_border(name):
    exact_case("pipe", name, flags=NO_SCAN_KERNEL, tokens=["k_rollout_pipe", "pow2res=0"])


def test_pipe_reach_square_inside_the_map_is_the_unclamped_control():
    """The other route to the unclamped address: no ring, but a reach square strictly inside the map.  No exits."""
    exact_case("pipe", "mid", flags=NO_SCAN_KERNEL, tokens=["k_rollout_pipe", "pow2res=1"])


@pytest.mark.parametrize("name", BC.GPU_CASES["pipe_res03"][1])
def test_pipe_resolution_that_is_no_power_of_two(name):
    exact_case("pipe_res03", name, flags=NO_SCAN_KERNEL, tokens=["k_rollout_pipe", "pow2res=0"])


def test_pipe_long_horizon():
    """T = 105: beyond the time-parallel kernel, the pipeline by the plan's own choice."""
    case = BC.PIPE_T105
    exact_case("pipe", case["start"], kind=case["kind"], t=case["t_steps"], vrange=np.array([0.0, case["vmax"]]),
               tokens=["k_rollout_pipe", "pow2res=0"])


# ---- the throughput kernel and the general kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.GPU_CASES["fused"][1])
def test_fused_exact(name):
    """513 tiles of 64 (the last one ragged): beyond two wave triples per CU the plan picks k_rollout_fused by itself
    (tests/test_map_plan.py: c2_32832_fused_lone)."""
    if _lib.device_props(0).compute_units != 256:
        pytest.skip("the shape is the smallest one k_rollout_fused takes on 256 CUs")
    exact_case("fused", name, n=32800, tokens=["k_rollout_fused pow2res=1"], absent=["speed_map", "one pass"])


@pytest.mark.parametrize("name", BC.GPU_CASES["general"][1])
def test_general_kernel_beyond_the_rotations_proof(name):
    """w in [-4, 4]: 0.4 rad per step, no incremental trig -- k_rollout_map on the LDS window."""
    exact_case("general", name, flags=NO_SCAN_KERNEL, wrange=np.array([-4.0, 4.0]), tokens=["k_rollout_map det lds_window"])


@pytest.mark.parametrize("name", BC.GPU_CASES["general"][1])
def test_general_kernel_on_the_global_cells(name):
    """A negative injected byte takes the 16-bit cells away: k_rollout_map on the global 32-bit cells.  The byte sits
    mid-map, outside the copies and off row 0 / column 0, so the copy property stands."""
    w = the_world("cellwise")
    cfg, lin, ang, planner, params = prepared(w, name)
    grid = lin.sample_grid_batch_d.copy_to_host()
    grid[0, 30, 31] = -7
    assert BC.has_copy_property(grid[0])
    lin.set_sampled_grids(grid)
    got_layers = layers(lin, ang)
    assert np.array_equal(got_layers[0], grid)
    noise, u_in, got, kernel = rolled_out(planner)
    assert kernel.startswith("k_rollout_map det global_cells exact=1"), kernel
    assert_bits(got, oracle_costs(params, lin, ang, got_layers, noise, u_in), "global cells %s" % name)


# ---- the CVaR kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m,wide", [(s, 4, False) for s in BC.GPU_CASES["tdm"][1]] + [("corner_hihi", 65, False)] +
                         [(s, 65, True) for s in BC.GPU_CASES["tdm"][1]] + [("corner_hihi", 4, True)])
def test_cvar_kernels(name, m, wide):
    """k_rollout_tdm_fast, and k_rollout_tdm beyond the rotation's proof, over M = 4 and M = 65 traction samples of the
    cell-wise (one-hot) PMFs -- every sample draws the same bytes, so the copy property stands -- against O.rollout_tdm."""
    kw = dict(wrange=np.array([-4.0, 4.0])) if wide else {}
    exact_case("tdm", name, mode=TDM, m=m, tokens=["k_rollout_tdm exact=1" if wide else "k_rollout_tdm_fast pow2res=1"], **kw)


# ---- a batched handle with per-problem windows -------------------------------------------------------------------------
@pytest.mark.parametrize("flags,token", [(0, "k_rollout_scan_exact"), (NO_SCAN_KERNEL, "k_rollout_pipe")])
def test_batch_of_six_problems_around_the_map(flags, token):
    """B = 6: one problem in each corner, one mid-map, one beyond the high corner.  Every problem against the oracle and
    against a single-problem planner, bit for bit."""
    from mppi_numba_amd.batch import MPPI_Batch
    kind, names = BC.GPU_CASES["batch"]
    w = the_world(kind)
    n = 64
    cfg, lin, ang, _ = make(w, n=n)
    tasks = [BC.params(w, name) for name in names]
    x0s = np.stack([p["x0"] for p in tasks]).astype(np.float32)
    goals = np.stack([p["xgoal"] for p in tasks]).astype(np.float32)
    batch = MPPI_Batch(cfg, len(names))
    batch.set_debug_flags(flags)
    batch.setup(tasks[0], lin, ang, np.stack([on_the_map(w, x) for x in x0s]).astype(np.float32), goals)
    assert np.isfinite(batch.solve()).all()
    # (MPPI_Batch.set_instances refuses a start outside the limits; the library takes it, as it takes a robot that a
    #  closed loop has moved there)
    _lib.call("mppi_planner_set_instances", batch._handle, len(names), _lib.ptr(x0s, C.c_float), _lib.ptr(goals, C.c_float))
    got_layers = layers(lin, ang)
    check_layers(w, got_layers)
    noise, u_in, costs, kernel = rolled_out(batch)
    noise, u_in = noise.reshape(len(names), n, cfg.num_steps, 2), u_in.reshape(len(names), cfg.num_steps, 2)
    assert kernel.startswith(token) and "problems=6" in kernel and "pow2res=0" in kernel, kernel
    assert costs.shape == (len(names), n)
    from mppi_numba_amd.mppi import MPPI_Numba
    for b, name in enumerate(names):
        assert_bits(costs[b], oracle_costs(tasks[b], lin, ang, got_layers, noise[b], u_in[b]), "problem %d (%s)" % (b, name))
        single = MPPI_Numba(cfg)
        single.set_debug_flags(flags)
        single.setup(dict(tasks[b], x0=on_the_map(w, x0s[b])), lin, ang)
        single.params["x0"] = x0s[b]
        single.set_u(u_in[b])
        single.set_noise(noise[b])
        single.rollout()
        assert single.last_rollout_kernel().startswith(token), single.last_rollout_kernel()
        assert_bits(costs[b], single.costs_d.copy_to_host(), "problem %d (%s) against a single planner" % (b, name))


# ---- the state rollouts drawn for the operator -------------------------------------------------------------------------
@pytest.mark.parametrize("mode,m", [(DET, 1), (TDM, 4)])
def test_vis_state_rollouts_from_an_edge(mode, m):
    """k_state_rollout: the optimal controls rolled out for plotting -- Config keeps no more of these rows than there are
    sampled maps, so the deterministic mode draws row 0 (O.state_rollout_noise) and the CVaR mode one row per traction
    sample (O.state_rollout_envs).  After a solve() and one more iteration the controls drive over the low x border."""
    kind, (name,) = BC.GPU_CASES["state_rollout"]
    w = the_world(kind)
    cfg, lin, ang, planner, params = prepared(w, name, mode=mode, m=m, vis=m)
    planner.sample_noise()
    planner.rollout()
    planner.update()
    got = planner.get_state_rollout()
    noise = planner.noise_samples_d.copy_to_host()
    u_cur, u_prev = planner.u_cur_d.copy_to_host(), planner.u_prev_d.copy_to_host()
    lin_g, ang_g = lin.sample_grid_batch_d.copy_to_host(), ang.sample_grid_batch_d.copy_to_host()
    p = oracle_params(params, lin, ang)
    want = O.state_rollout_envs(p, lin_g, ang_g, u_cur, m) if mode is TDM else O.state_rollout_noise(p, lin_g, ang_g, noise, u_prev, u_cur, m)
    assert got.shape == want.shape == (m, cfg.num_steps + 1, 3)
    assert (want[:, -1, 0] < w["xlimits"][0] - w["res"]).all(), want[:, -1, 0]  # they leave the map over the low x border
    assert np.array_equal(got, want), np.abs(got - want).max()


# ---- the tolerance mode (math="fast") ------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,token", [(100, "k_rollout_scan "), (129, "k_rollout_fused<one pass>")])
def test_fast_math_at_the_border_and_mid_map(t, token):
    """The project's bar for math="fast" (README, tests/test_gpu_fast_throughput.py): at least 99.9 % of the costs within
    1e-6 relative.  The same world from the high corner, where the rollouts leave over both high borders, and from the
    middle, where v in [0, 2] keeps every rollout on the map (the control).  200 x 208 cells: no rollout from the high
    corner gets to a low border (at most 129 * 0.2 m * 0.85 / 0.25 m = 88 cells), so the oracle is the clamp."""
    w = the_world("nominal", density=0.03, rows=200, cols=208)
    shares = {}
    for name in ("mid", "corner_hihi"):
        cfg, lin, ang, planner, params = prepared(w, name, n=2048, t=t, math="fast", vrange=np.array([0.0, 2.0]), far_goal=60.0)
        got_layers = layers(lin, ang)
        check_layers(w, got_layers)
        noise, u_in, got, kernel = rolled_out(planner)
        assert kernel.startswith(token), kernel
        want = oracle_costs(params, lin, ang, got_layers, noise, u_in)
        rel = np.abs(got - want) / np.maximum(np.abs(want), 30.0)
        shares[name] = float((rel <= 1e-6).mean())
        print("\n%s T=%d from %s: within 1e-6 relative %.5f, bit-identical %.5f, rel quantiles %s" % (
            kernel.split(" ")[0], t, name, shares[name], (got == want).mean(), np.quantile(rel, [0.5, 0.99, 0.999, 1.0])))
        # the case is what it says: from the corner nearly every rollout ends off the map, from the middle none does
        p = oracle_params(params, lin, ang)
        ends = O.state_rollout_noise(p, got_layers[0], got_layers[1], noise, u_in, u_in, 64)[:, -1, :2]
        off = (ends[:, 0] >= w["xlimits"][1]) | (ends[:, 1] >= w["ylimits"][1]) | (ends[:, 0] < w["xlimits"][0]) | (ends[:, 1] < w["ylimits"][0])
        assert off[1:].mean() >= 0.8 if name == "corner_hihi" else not off.any(), (name, off.mean())
    assert shares["mid"] >= 0.999, shares
    assert shares["corner_hihi"] >= 0.999, shares


# ---- the planner's own maps: a start outside the ring ------------------------------------------------------------------
def hole_starts(lin):
    """(x, y, theta) 1 cell and 30 cells beyond each high limit of the padded map, and 1 cell beyond each low limit."""
    (xlo, xhi), (ylo, yhi), res = lin.padded_xlimits, lin.padded_ylimits, lin.res
    xm, ym = 0.5 * (xlo + xhi) + 0.1, 0.5 * (ylo + yhi) + 0.1
    return {"x_high_1": (xhi + 0.4 * res, ym, 0.3), "x_high_30": (xhi + 29.4 * res, ym, 2.0), "y_high_1": (xm, yhi + 0.4 * res, 1.0),
            "y_high_30": (xm, yhi + 29.4 * res, -1.0), "x_low_1": (xlo - 0.6 * res, ym, 3.0), "y_low_1": (xm, ylo - 0.6 * res, -1.5)}


@pytest.mark.parametrize("flags,token", [(0, "k_rollout_scan_exact"), (NO_SPECULATION, "direct=1"), (NO_SCAN_KERNEL, "k_rollout_pipe")])
def test_a_start_outside_the_ring_takes_the_clamped_address(flags, token):
    """The reference's padded map (a ring of 2 zero-traction cells for 5 m/s, cells of 0.25 m), C2's parameters.  From a
    start on the map the address goes unclamped (pow2res=1: the ring stops every rollout).  From a start outside, the
    clamp takes the ring cell -- as the oracle does, high side and low (the ring's masks are 0 and its traction is 0
    all around) -- so the rollout stands still and pays that cell at every step."""
    from mppi_numba_amd.batch import MPPI_Batch
    w = the_world("cellwise")
    cfg, lin, ang, planner = make(w, pad_speed=5.0)
    assert lin.pad_cells == 2
    params = BC.params(w, "mid")
    inside = params["x0"].copy()
    planner.set_debug_flags(flags)
    planner.setup(params, lin, ang)
    assert np.isfinite(planner.solve()).all()
    got_layers = layers(lin, ang)
    assert (got_layers[0][0, :2] == 0).all() and (got_layers[0][0, :, -2:] == 0).all()  # the ring

    def check(x0, pow2res):
        planner.params["x0"] = np.array(x0)
        noise, u_in, got, kernel = rolled_out(planner)
        assert token in kernel and "pow2res=%d" % pow2res in kernel, kernel
        want = oracle_costs(dict(params, x0=np.array(x0)), lin, ang, got_layers, noise, u_in)
        assert_bits(got, want, "%s from %s" % (kernel, x0))
        return want

    check(inside, 1)
    starts = hole_starts(lin)
    for name, x0 in starts.items():
        check(x0, 0)
    check(inside, 1)
    # one problem of a batch outside: the whole handle takes the clamped address
    names = list(starts)
    x0s = np.array([inside] + [starts[k] for k in names], dtype=np.float32)
    goals = np.tile(np.asarray(params["xgoal"], dtype=np.float32), (len(x0s), 1))
    bcfg, _, _, _ = make(w, pad_speed=5.0, n=64)
    batch = MPPI_Batch(bcfg, len(x0s))
    batch.set_debug_flags(flags)
    batch.setup(params, lin, ang, np.tile(x0s[:1], (len(x0s), 1)), goals)
    assert np.isfinite(batch.solve()).all()
    noise, u_in, costs, kernel = rolled_out(batch)
    assert token in kernel and "pow2res=1" in kernel, kernel
    _lib.call("mppi_planner_set_instances", batch._handle, len(x0s), _lib.ptr(x0s, C.c_float), _lib.ptr(goals, C.c_float))
    noise, u_in, costs, kernel = rolled_out(batch)
    assert token in kernel and "pow2res=0" in kernel and "problems=%d" % len(x0s) in kernel, kernel
    noise, u_in = noise.reshape(len(x0s), 64, cfg.num_steps, 2), u_in.reshape(len(x0s), cfg.num_steps, 2)
    for b in range(len(x0s)):
        want = oracle_costs(dict(params, x0=x0s[b]), lin, ang, got_layers, noise[b], u_in[b])
        assert_bits(costs[b], want, "batch problem %d from %s" % (b, x0s[b]))
