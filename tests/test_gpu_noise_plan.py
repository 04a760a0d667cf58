"""Where an iteration's noise comes from and who produces the next iteration's (csrc/noise_plan.h: noise_choose), on the
device: one case per route of tests/test_noise_plan.py's table, at the smallest shape that reaches it.

  in_kernel           c2, N = 800, T = 32: k_rollout_scan_exact computes its noise from the Philox counters
  scan_spare_blocks   the same shape, math="fast" with MPPI_DEBUG_SCAN_READ_NOISE: k_rollout_scan reads its noise, the CUs
                      without a tile generate the next iteration's
  pipe_spare_blocks   the same shape with MPPI_DEBUG_NO_SCAN_KERNEL: the spare CUs of k_rollout_pipe
  cvar_appended       c3, N = 256, T = 32, M = 64: workgroups appended to k_rollout_tdm_fast
  beside_rollout      c2, N = 40000, T = 100: the second stream beside the rollout.  N * T >= 4 000 000 from this N on, and
                      k_rollout_fused runs there already (157 workgroups of four waves, no blocks of its own)
  beside_update       c5, 64 problems x 2112 rollouts, T = 32: nine rollout waves per CU, so the second stream beside the update

Loops of 1, 2, 3 and 4 iterations on fresh planners: the last_rollout_kernel() text after a loop of k iterations is that of
the k-th launch, and it names the noise's source and the blocks appended.  The texts are held to literals recorded from the
library as it was before the choice became one function; u and the costs after four iterations to the bits of the same
iterations driven through sample_noise / rollout / update.  For in_kernel, pipe_spare_blocks and cvar_appended
tests/test_gpu_update_plan.py holds exactly that (its cases fold, rows_behind_pipe and tdm), so they are not repeated here.
What a generator that never announces itself does is tests/test_gpu_stream_flags.py's.

Every case also holds, against the stage-level planner: the noise read back after the loop (regenerated from the counters
where the launch never stored it), the block that sample_noise() hands out behind a loop of two iterations (the one
produced ahead, where one was), and a loop interrupted by a set_params that changes u_std (the noise ahead is dropped).
"""
import functools

import numpy as np
import pytest

import bench
from mppi_numba_amd import _lib

pytestmark = pytest.mark.gpu

ITERATIONS = 4

# name -> (workload, rollouts (per problem), steps, options): math, flags, problems (a batched handle), m (traction samples)
CASES = {
    "in_kernel": ("c2", 800, 32, {}),
    "scan_spare_blocks": ("c2", 800, 32, dict(math="fast", flags=_lib.DEBUG_SCAN_READ_NOISE)),
    "pipe_spare_blocks": ("c2", 800, 32, dict(flags=_lib.DEBUG_NO_SCAN_KERNEL)),
    "cvar_appended": ("c3", 256, 32, dict(m=64)),
    "beside_rollout": ("c2", 40000, 100, {}),
    "beside_update": ("c5", 2112, 32, dict(problems=64)),
}

# recorded on an MI355X (256 CUs) from the library before csrc/noise_plan.h existed: the launch of iteration 1, 2, 3, 4
SCAN_READS = "k_rollout_scan tile=32 waves=4 pow2res=1 noise=read lds=40960 noise_blocks=231 problems=0"
EXPECTED = {
    "scan_spare_blocks": [SCAN_READS] + [SCAN_READS + " applies_update=1 reduces_tiles=1"] * (ITERATIONS - 1),
    "beside_rollout": ["k_rollout_fused pow2res=1 waves_per_wg=4 window=142x144 problems=0 noise_kept=56"] * ITERATIONS,
    "beside_update": ["k_rollout_fused pow2res=1 waves_per_wg=11 window=83x96 problems=64 noise_kept=24"] * ITERATIONS,
}


class Case:
    """The TDMs of a case, sampled once, and as many fresh planners on them as asked for."""

    def __init__(self, name):
        workload, n, t, self.opt = CASES[name]
        saved = bench.WORKLOADS[workload]
        bench.WORKLOADS[workload] = dict(saved, t=t, **({"m": self.opt["m"]} if "m" in self.opt else {}))
        try:
            _, self.cfg, self.lin, self.ang, _, self.params = bench.build_planner(workload, n, math=self.opt.get("math", "exact"))
        finally:
            bench.WORKLOADS[workload] = saved
        self.lin.sample_grids(self.params["alpha_dyn"])
        self.ang.sample_grids(self.params["alpha_dyn"])

    def planner(self):
        from mppi_numba_amd.batch import MPPI_Batch
        from mppi_numba_amd.mppi import MPPI_Numba
        problems = self.opt.get("problems", 0)
        if problems:
            planner = MPPI_Batch(self.cfg, problems)
            planner.setup(self.params, self.lin, self.ang, *bench.batch_problems(problems, np.random.default_rng(100)))
        else:
            planner = MPPI_Numba(self.cfg)
            planner.setup(self.params, self.lin, self.ang)
        planner.move_mppi_task_vars_to_device()  # (solve() and the stage-level calls do; the loop expects it done)
        if self.opt.get("flags"):
            planner.set_debug_flags(self.opt["flags"])
        return planner


def widen_u_std(planner):
    planner.params["u_std"] = [1.5 * s for s in planner.params["u_std"]]
    planner.move_mppi_task_vars_to_device()


def state(planner):
    return planner.u_cur_d.copy_to_host(), planner.costs_d.copy_to_host()


@functools.lru_cache(maxsize=None)
def stage_level(name):
    """The reference of a case, computed once: the stage-level planner's u, costs and noise after four iterations, the
    block of its third sample_noise(), and u and costs where u_std changes behind the second iteration."""
    case = Case(name)
    planner, changed = case.planner(), case.planner()
    out = {}
    for k in range(ITERATIONS):
        for p in (planner, changed):
            if p is changed and k == 2:
                widen_u_std(p)
            p.sample_noise()
            if p is planner and k == 2:
                out["third_block"] = p.noise_samples_d.copy_to_host()
            p.rollout()
            p.update()
    out["u"], out["costs"] = state(planner)
    out["noise"] = planner.noise_samples_d.copy_to_host()
    out["changed"] = state(changed)
    for value in out.values():
        for array in value if isinstance(value, tuple) else (value,):
            array.setflags(write=False)
    return case, out


@pytest.mark.parametrize("name", list(EXPECTED))
def test_four_iterations(name):
    case, want = stage_level(name)
    texts = []
    for k in range(1, ITERATIONS + 1):
        planner = case.planner()
        planner.iterate_async(k)
        planner.synchronize()
        texts.append(planner.last_rollout_kernel())
    print("\n%s: %r" % (name, texts))
    # (the texts name noise blocks on spare CUs: the literals are those of 256 CUs)
    if _lib.device_props(0).compute_units == 256:
        assert texts == EXPECTED[name]
    u, costs = state(planner)
    assert np.isfinite(costs).all() and np.abs(u).max() > 0
    assert np.array_equal(u, want["u"]), float(np.abs(u - want["u"]).max())
    assert np.array_equal(costs, want["costs"])


@pytest.mark.parametrize("name", list(CASES))
def test_noise_read_back_after_the_loop(name):
    case, want = stage_level(name)
    planner = case.planner()
    planner.iterate_async(ITERATIONS)
    planner.synchronize()
    noise = planner.noise_samples_d.copy_to_host()
    assert np.abs(noise).max() > 0
    assert np.array_equal(noise, want["noise"])


@pytest.mark.parametrize("name", list(CASES))
def test_sample_noise_behind_a_loop_hands_out_the_next_block(name):
    case, want = stage_level(name)
    planner = case.planner()
    planner.iterate_async(2)
    planner.sample_noise()
    assert np.array_equal(planner.noise_samples_d.copy_to_host(), want["third_block"])


@pytest.mark.parametrize("name", list(CASES))
def test_u_std_changed_between_two_loops(name):
    case, want = stage_level(name)
    planner = case.planner()
    planner.iterate_async(2)
    widen_u_std(planner)
    planner.iterate_async(2)
    planner.synchronize()
    u, costs = state(planner)
    assert np.array_equal(u, want["changed"][0]), float(np.abs(u - want["changed"][0]).max())
    assert np.array_equal(costs, want["changed"][1])
