"""The CVaR mode's kernel choice and the route from the TDMs to the cell words (csrc/cvar_plan.h: cvar_choose,
cells_choose), on the device: one case per answer of tests/test_cvar_plan.py's tables that a small shape reaches --
N = 64 rollouts, T = 20 steps, a map cut to 70 x 90 cells.

  m8_exact      M = 8: k_rollout_tdm_fast on cells of 0.25 m
  m8_fast       ... math="fast": its <cost f32> form
  res03         cells of 0.3 m: pow2res=0
  wide_w        w in [-4, 4]: 0.4 rad per step are beyond the rotation's proof, k_rollout_tdm
  wide_w_fast   ... math="fast": exact=0
  m65           M = 65: 128 threads, a ragged last wave of samples
  m1            M = 1 in CVaR mode: the single-sample packing, the CVaR kernel all the same

One rollout() per case.  The whole last_rollout_kernel() text is held to a literal recorded from the library as it was
before the choices became functions; with exact math the costs to the bits of the CPU oracle.  (The 64 KiB borders of
the table need samples in the thousands: tests/test_cvar_plan.py alone holds them.)

solve() against the staged path on both sides of the measured border of sampling straight into the cell words (M = 190:
sample, sample, pack; M = 192: k_sample_cellsM_philox), with the assertions of
tests/test_gpu_parity.py::test_sampling_straight_into_cell_words_equals_sample_then_pack.
"""
import numpy as np
import pytest

import bench
from test_gpu_scale import oracle_costs

pytestmark = pytest.mark.gpu

N, T_STEPS, ROWS, COLS = 64, 20, 70, 90

CASES = {
    "m8_exact": dict(m=8),
    "m8_fast": dict(m=8, math="fast"),
    "res03": dict(m=8, res=0.3),
    "wide_w": dict(m=8, wrange=(-4.0, 4.0)),
    "wide_w_fast": dict(m=8, wrange=(-4.0, 4.0), math="fast"),
    "m65": dict(m=65),
    "m1": dict(m=1),
}

# recorded on an MI355X from the library before csrc/cvar_plan.h existed
EXPECTED = {
    "m8_exact": "k_rollout_tdm_fast pow2res=1 noise_blocks=0",
    "m8_fast": "k_rollout_tdm_fast<cost f32> pow2res=1 noise_blocks=0",
    "res03": "k_rollout_tdm_fast pow2res=0 noise_blocks=0",
    "wide_w": "k_rollout_tdm exact=1",
    "wide_w_fast": "k_rollout_tdm exact=0",
    "m65": "k_rollout_tdm_fast pow2res=1 noise_blocks=0",
    "m1": "k_rollout_tdm_fast pow2res=1 noise_blocks=0",
}


def small_world(res=0.25):
    pmf, obstacle, unknown, td = bench.synthetic_world("c3", np.random.default_rng(3))
    pmf, obstacle, unknown = pmf[:, :ROWS, :COLS].copy(), obstacle[:ROWS, :COLS].copy(), unknown[:ROWS, :COLS].copy()
    return pmf, obstacle, unknown, dict(td, xlimits=(0.0, COLS * res), ylimits=(0.0, ROWS * res), res=res)


def build(m, n=N, math="exact", res=0.25, wrange=None, world=None):
    from mppi_numba_amd.config import Config
    from mppi_numba_amd.mppi import MPPI_Numba
    from mppi_numba_amd.terrain import TDM_Numba
    pmf, obstacle, unknown, td = world or small_world(res)
    cfg = Config(T=T_STEPS * 0.1, dt=0.1, num_grid_samples=m, num_control_rollouts=n, max_speed_padding=4.0,
                 num_vis_state_rollouts=1, max_map_dim=(80, 100), seed=9, enforce_recommended_limits=False, math=math,
                 use_tdm=True)
    lin, ang = TDM_Numba(cfg), TDM_Numba(cfg)
    lin.set_TDM_from_PMF_grid(pmf, td, obstacle, unknown)
    ang.set_TDM_from_PMF_grid(pmf[::-1].copy(), td, obstacle, unknown)
    planner = MPPI_Numba(cfg)
    params = bench.make_params("c3")
    params.update(x0=np.array([5.0, 6.0, 0.4]), xgoal=np.array([9.0, 9.0]), alpha_dyn=0.8)
    if wrange is not None:
        params["wrange"] = np.array(wrange)
    planner.setup(params, lin, ang)
    return lin, ang, planner, params


@pytest.mark.parametrize("name", list(CASES))
def test_one_rollout(name):
    opt = CASES[name]
    lin, ang, planner, params = build(**opt)
    lin.sample_grids(params["alpha_dyn"])
    ang.sample_grids(params["alpha_dyn"])
    planner.sample_noise()
    noise, u_in = planner.noise_samples_d.copy_to_host(), planner.u_cur_d.copy_to_host()
    planner.rollout()
    text = planner.last_rollout_kernel()
    print("\n%s: %r" % (name, text))
    assert text == EXPECTED[name]
    got = planner.costs_d.copy_to_host()
    assert got.shape == (N,) and np.isfinite(got).all()
    if opt.get("math", "exact") == "exact":
        # (m=2: oracle.rollout_tdm for one sample too -- the CVaR kernel's cost order is not the deterministic kernel's)
        want = oracle_costs(dict(m=2), params, lin, ang, noise, u_in)
        assert np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("m", [190, 192])
def test_solve_equals_sample_then_pack_on_both_sides_of_the_border(m):
    world = small_world()
    (lin_a, ang_a, fused, _), (lin_b, ang_b, staged, params) = [build(m, n=96, world=world) for _ in range(2)]
    for _ in range(2):  # two solves: the epochs advance alike
        u_fused = fused.solve()
        # the ordinary path by hand: sample both TDMs, then one staged iteration
        lin_b.sample_grids(params["alpha_dyn"])
        ang_b.sample_grids(params["alpha_dyn"])
        staged.sample_noise()
        staged.rollout()
        staged.update()
        assert np.array_equal(fused.costs_d.copy_to_host(), staged.costs_d.copy_to_host())
        assert np.array_equal(u_fused, staged.u_cur_d.copy_to_host())
        assert np.array_equal(lin_a.sample_grid_batch_d.copy_to_host(), lin_b.sample_grid_batch_d.copy_to_host())
        assert np.array_equal(ang_a.sample_grid_batch_d.copy_to_host(), ang_b.sample_grid_batch_d.copy_to_host())
