"""Which update an iteration runs (csrc/update_plan.h: update_choose, next_rollout_takes), on the device.

Each case is one state of tests/test_update_plan.py's table at the smallest shape that reaches it.  It runs a loop of four
iterations and holds
  * the last_rollout_kernel() text of every iteration -- the text after a loop of k iterations is that of the k-th launch;
    it says whether the launch took the previous update over (applies_update / reduces_tiles) -- to literals recorded
    from the library as it was before the choice became one function, and
  * u after the four iterations to the bits of the same iterations driven through the stage-level calls
    (sample_noise, rollout, update), where every update is a launch of its own.

The folds: N = 800, T = 32 (25 tiles of 32 rollouts: 4 * 25 >= 32); refused at N = 256, T = 100 (8 tiles).  Four rows per
workgroup of k_update_rows: 32 problems x 64 steps = 2048 rows.  Two shards whose packets are gathered by hand run their
loop through update_local / update_apply_and_rollout (the rollout launch applies the packets) against update_apply + rollout.
"""
import numpy as np
import pytest

import bench
from mppi_numba_amd import _lib

pytestmark = pytest.mark.gpu

ITERATIONS = 4

# name -> (workload, rollouts (per problem, per shard), steps, options)
#   math, flags, problems (a batched handle), comm (a communicator of one rank), m (traction samples), world (shards)
CASES = {
    "fold": ("c2", 800, 32, {}),
    "fold_fast": ("c2", 800, 32, dict(math="fast")),
    "fold_speed_map": ("c2m", 800, 32, {}),
    "fold_refused": ("c2", 256, 100, {}),
    "no_reduce_fold": ("c2", 800, 32, dict(flags=_lib.DEBUG_NO_REDUCE_FOLD)),
    "rows_behind_pipe": ("c2", 800, 32, dict(flags=_lib.DEBUG_NO_SCAN_KERNEL)),
    "rows_four_per_workgroup": ("c5", 64, 64, dict(problems=32, flags=_lib.DEBUG_NO_SCAN_KERNEL)),
    "combine_batch": ("c5", 64, 64, dict(problems=32)),
    "comm_one_rank": ("c2", 800, 32, dict(comm=True)),
    "tdm": ("c3", 256, 32, dict(m=64)),
    "two_shards_by_hand": ("c2", 400, 32, dict(world=2)),
}

# recorded on an MI355X (256 CUs) from the library before csrc/update_plan.h existed: the launch of iteration 1, 2, 3, 4
def four(text, takes=""):
    """the first launch has nothing to take; `takes`: what the text of the other three says they took"""
    return [text] + [text + takes] * (ITERATIONS - 1)


SCAN_EXACT_800 = "k_rollout_scan_exact tile=32 waves=10 pow2res=1 noise=in-kernel lds=83408 noise_blocks=0 problems=0 failed_tiles=pipelined"
EXPECTED = {
    "fold": four(SCAN_EXACT_800, " applies_update=1 reduces_tiles=1"),
    "fold_fast": four("k_rollout_scan tile=32 waves=4 pow2res=1 noise=in-kernel lds=40960 noise_blocks=0 problems=0",
                      " applies_update=1 reduces_tiles=1"),
    "fold_speed_map": four("k_rollout_scan_exact speed_map tile=32 waves=10 pow2res=1 noise=in-kernel lds=48848 noise_blocks=0 problems=0 "
                           "failed_tiles=one_wave", " applies_update=1 reduces_tiles=1"),
    "fold_refused": four("k_rollout_scan_exact tile=32 waves=16 pow2res=1 noise=in-kernel lds=151952 noise_blocks=0 problems=0 "
                         "failed_tiles=pipelined"),
    "no_reduce_fold": four(SCAN_EXACT_800),
    "rows_behind_pipe": four("k_rollout_pipe chunk=8 pow2res=1 cc_lds=1 triples_per_wg=1 window=60x64@(0,0) lds=51456 noise_blocks=243 "
                             "problems=0"),
    "rows_four_per_workgroup": four("k_rollout_pipe chunk=8 pow2res=1 cc_lds=1 triples_per_wg=1 window=159x168@(0,0) lds=114352 "
                                    "noise_blocks=224 problems=32"),
    "combine_batch": four("k_rollout_scan_exact tile=32 waves=14 pow2res=1 noise=in-kernel lds=94672 noise_blocks=0 problems=32 "
                          "failed_tiles=one_wave"),
    "comm_one_rank": four(SCAN_EXACT_800, " applies_update=1"),
    "tdm": four("k_rollout_tdm_fast pow2res=1 noise_blocks=16"),
    "two_shards_by_hand": four(SCAN_EXACT_800.replace("noise=in-kernel", "noise=read"), " applies_update=1"),
}


class Case:
    """The TDMs of a case, sampled once, and as many fresh planners on them as asked for."""

    def __init__(self, name):
        workload, n, t, opt = CASES[name]
        self.opt, self.world = opt, opt.get("world", 1)
        saved = bench.WORKLOADS[workload]
        bench.WORKLOADS[workload] = dict(saved, t=t, **({"m": opt["m"]} if "m" in opt else {}))
        try:
            _, self.cfg, self.lin, self.ang, _, self.params = bench.build_planner(workload, n, world=self.world, math=opt.get("math", "exact"))
        finally:
            bench.WORKLOADS[workload] = saved
        self.lin.sample_grids(self.params["alpha_dyn"])
        self.ang.sample_grids(self.params["alpha_dyn"])

    def planner(self, rank=0):
        from mppi_numba_amd.batch import MPPI_Batch
        from mppi_numba_amd.mppi import MPPI_Numba, comm_unique_id
        problems = self.opt.get("problems", 0)
        if problems:
            planner = MPPI_Batch(self.cfg, problems)
            planner.setup(self.params, self.lin, self.ang, *bench.batch_problems(problems, np.random.default_rng(100)))
        else:
            planner = MPPI_Numba(self.cfg, rank=rank, world_size=self.world)
            planner.setup(self.params, self.lin, self.ang)
        planner.move_mppi_task_vars_to_device()  # (solve() and the stage-level calls do; the loop expects it done)
        if self.opt.get("flags"):
            planner.set_debug_flags(self.opt["flags"])
        if self.opt.get("comm"):
            planner.comm_init(comm_unique_id())
        return planner

    def loop(self, iterations):
        """(text of the last launch, u, costs) of a fresh planner after a loop of `iterations`"""
        if self.world > 1:
            return self.shards(iterations, fold=True)
        planner = self.planner()
        planner.iterate_async(iterations)
        planner.synchronize()
        return planner.last_rollout_kernel(), planner.u_cur_d.copy_to_host(), planner.costs_d.copy_to_host()

    def stages(self, iterations):
        """... after the same iterations, every stage a call"""
        if self.world > 1:
            return self.shards(iterations, fold=False)
        planner = self.planner()
        for _ in range(iterations):
            planner.sample_noise()
            planner.rollout()
            planner.update()
        return planner.last_rollout_kernel(), planner.u_cur_d.copy_to_host(), planner.costs_d.copy_to_host()

    def shards(self, iterations, fold):
        """Shards of one problem, the packets gathered by hand.  fold: the next rollout launch applies them
        (update_apply_and_rollout), else k_apply (update_apply) and a rollout call."""
        shards = [self.planner(rank) for rank in range(self.world)]
        packets = None
        for k in range(iterations):
            for s in shards:
                s.sample_noise()
                if packets is None:
                    s.rollout()
                elif fold:
                    s.update_apply_and_rollout(packets)
                else:
                    s.update_apply(packets)
                    s.rollout()
            packets = np.stack([s.update_local() for s in shards])
        for s in shards:
            s.update_apply(packets)
        u = [s.u_cur_d.copy_to_host() for s in shards]
        assert all(np.array_equal(u[0], other) for other in u[1:])
        return shards[0].last_rollout_kernel(), u[0], np.concatenate([s.costs_d.copy_to_host() for s in shards])


@pytest.mark.parametrize("name", list(CASES))
def test_four_iterations(name):
    case = Case(name)
    loops = [case.loop(k) for k in range(1, ITERATIONS + 1)]
    texts = [text for text, _, _ in loops]
    print("\n%s: %r" % (name, texts))
    # (the texts name noise blocks on spare CUs: the literals are those of 256 CUs)
    if _lib.device_props(0).compute_units == 256:
        assert texts == EXPECTED[name]
    _, u_loop, costs_loop = loops[-1]
    _, u_stages, costs_stages = case.stages(ITERATIONS)
    assert np.isfinite(costs_loop).all() and np.abs(u_loop).max() > 0
    assert np.array_equal(u_loop, u_stages), float(np.abs(u_loop - u_stages).max())
    assert np.array_equal(costs_loop, costs_stages)
