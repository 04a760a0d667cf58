"""Which rollout kernel a map-mode launch runs, and with what geometry (csrc/map_plan.h: map_choose), on the device.

Each case builds a planner through bench.build_planner, draws the traction grids, calls rollout() once and holds the
WHOLE last_rollout_kernel() string to a literal.  The literals were recorded from the library as it was before the
choice became one function (csrc/map_plan.h), so the test passes on both; tests/test_map_plan.py parses the same
literals on the CPU and holds their fields to the rows of its table.

The cases are the smallest shapes on each side of every border that depends on the 256 CUs of an MI355X: the last scan
launch and the first pipe launch (256 tiles of 32 against 257), one wave triple against two (256 tiles of 64 against
257), two triples against the fused kernel (512 tiles of 64 against 513); the other cases reach one kernel family each
at N = 64.  A batched handle (c5) at 64 and at 256 rollouts per problem: the workgroup's waves divide the tiles per
problem (1 and 4), in the families a batch of 64 problems reaches (scan-exact and pipe by default; fused under
math="fast" without the scan kernel, where the waves show in the text).
"""
import numpy as np
import pytest

import bench
from mppi_numba_amd import _lib

pytestmark = pytest.mark.gpu

NO_SPECULATION, NO_SCAN_KERNEL, SCAN_FULL_TILES = _lib.DEBUG_NO_SPECULATION, _lib.DEBUG_NO_SCAN_KERNEL, _lib.DEBUG_SCAN_FULL_TILES

# (name, workload, rollouts (per problem), math, debug flags, problems (0: a single-problem handle), wrange or None)
CASES = [
    ("c2_64_exact", "c2", 64, "exact", 0, 0, None),
    ("c2_64_fast", "c2", 64, "fast", 0, 0, None),
    ("c2_64_fast_full_tiles", "c2", 64, "fast", SCAN_FULL_TILES, 0, None),
    ("c2_64_exact_direct", "c2", 64, "exact", NO_SPECULATION, 0, None),
    ("c2_64_exact_pipe", "c2", 64, "exact", NO_SCAN_KERNEL, 0, None),
    ("c2_8192_last_scan", "c2", 8192, "exact", 0, 0, None),
    ("c2_8224_first_pipe", "c2", 8224, "exact", 0, 0, None),
    ("c2_16384_one_triple", "c2", 16384, "exact", 0, 0, None),
    ("c2_16448_two_triples", "c2", 16448, "exact", 0, 0, None),
    ("c2_32768_two_triples", "c2", 32768, "exact", 0, 0, None),
    ("c2_32832_fused_lone", "c2", 32832, "exact", 0, 0, None),
    # |dt * w * traction| = 0.4 rad > 0.36: no incremental trig, the general kernel on the LDS window
    ("c2_64_general_windowed", "c2", 64, "exact", NO_SCAN_KERNEL, 0, (-4.0, 4.0)),
    ("c2l_64_pipe", "c2l", 64, "exact", 0, 0, None),
    ("c2m_64_exact", "c2m", 64, "exact", 0, 0, None),
    ("c2m_64_exact_fused", "c2m", 64, "exact", NO_SCAN_KERNEL, 0, None),
    ("c2m_64_fast", "c2m", 64, "fast", 0, 0, None),
    ("c5_64_exact", "c5", 64, "exact", 0, 64, None),
    ("c5_256_exact", "c5", 256, "exact", 0, 64, None),
    ("c5_64_fast_fused", "c5", 64, "fast", NO_SCAN_KERNEL, 64, None),
    ("c5_256_fast_fused", "c5", 256, "fast", NO_SCAN_KERNEL, 64, None),
]

# recorded on an MI355X (256 CUs, 160 KiB of LDS per CU) from the library before csrc/map_plan.h existed
EXPECTED = {
    "c2_64_exact":
        "k_rollout_scan_exact tile=32 waves=16 pow2res=1 noise=read lds=151952 noise_blocks=0 problems=0 failed_tiles=pipelined",
    "c2_64_fast":
        "k_rollout_scan tile=32 waves=13 pow2res=1 noise=read lds=68752 noise_blocks=0 problems=0",
    "c2_64_fast_full_tiles":
        "k_rollout_scan tile=64 waves=13 pow2res=1 noise=read lds=136464 noise_blocks=0 problems=0",
    "c2_64_exact_direct":
        "k_rollout_scan_exact tile=32 waves=16 pow2res=1 noise=read lds=140176 noise_blocks=0 problems=0 direct=1 (exact three-wave schedule, no speculation)",
    "c2_64_exact_pipe":
        "k_rollout_pipe chunk=8 pow2res=1 cc_lds=1 triples_per_wg=1 window=142x144@(0,0) lds=121120 noise_blocks=0 problems=0",
    "c2_8192_last_scan":
        "k_rollout_scan_exact tile=32 waves=16 pow2res=1 noise=read lds=151952 noise_blocks=0 problems=0 failed_tiles=pipelined",
    "c2_8224_first_pipe":
        "k_rollout_pipe chunk=8 pow2res=1 cc_lds=1 triples_per_wg=1 window=142x144@(0,0) lds=121120 noise_blocks=0 problems=0",
    "c2_16384_one_triple":
        "k_rollout_pipe chunk=8 pow2res=1 cc_lds=1 triples_per_wg=1 window=142x144@(0,0) lds=121120 noise_blocks=0 problems=0",
    "c2_16448_two_triples":
        "k_rollout_pipe chunk=8 pow2res=1 cc_lds=0 triples_per_wg=2 window=142x144@(0,0) lds=96544 noise_blocks=0 problems=0",
    "c2_32768_two_triples":
        "k_rollout_pipe chunk=8 pow2res=1 cc_lds=0 triples_per_wg=2 window=142x144@(0,0) lds=96544 noise_blocks=0 problems=0",
    "c2_32832_fused_lone":
        "k_rollout_fused pow2res=1 waves_per_wg=4 window=142x144 problems=0 noise_kept=56",
    "c2_64_general_windowed":
        "k_rollout_map det lds_window exact=1 waves_per_wg=4 window=142x144 problems=0",
    "c2l_64_pipe":
        "k_rollout_pipe chunk=6 pow2res=1 cc_lds=0 triples_per_wg=1 window=260x264@(0,0) lds=162048 noise_blocks=0 problems=0",
    "c2m_64_exact":
        "k_rollout_scan_exact speed_map tile=32 waves=16 pow2res=1 noise=read lds=151952 noise_blocks=0 problems=0 failed_tiles=one_wave",
    "c2m_64_exact_fused":
        "k_rollout_fused speed_map pow2res=1 waves_per_wg=4 window=142x144 problems=0",
    "c2m_64_fast":
        "k_rollout_fused<one pass> speed_map pow2res=1 waves_per_wg=4 window=142x144 problems=0",
    "c5_64_exact":
        "k_rollout_scan_exact tile=32 waves=16 pow2res=1 noise=read lds=151952 noise_blocks=0 problems=64 failed_tiles=one_wave",
    "c5_256_exact":
        "k_rollout_pipe chunk=8 pow2res=1 cc_lds=0 triples_per_wg=1 window=247x256@(0,0) lds=155488 noise_blocks=0 problems=64",
    "c5_64_fast_fused":
        "k_rollout_fused<one pass> pow2res=1 waves_per_wg=1 window=247x256 problems=64 noise_kept=0",
    "c5_256_fast_fused":
        "k_rollout_fused<one pass> pow2res=1 waves_per_wg=4 window=247x256 problems=64 noise_kept=0",
}


def run_case(workload, n, math, flags, problems, wrange):
    """The planner of one case after one rollout()."""
    _, cfg, lin, ang, planner, params = bench.build_planner(workload, n, math=math)
    if problems:
        from mppi_numba_amd.batch import MPPI_Batch
        planner = MPPI_Batch(cfg, problems)
        planner.setup(params, lin, ang, *bench.batch_problems(problems, np.random.default_rng(100)))
    if wrange is not None:
        planner.params["wrange"] = np.array(wrange)
    if flags:
        planner.set_debug_flags(flags)
    lin.sample_grids(params["alpha_dyn"])
    ang.sample_grids(params["alpha_dyn"])
    planner.sample_noise()
    planner.rollout()
    return planner


@pytest.mark.parametrize("name,workload,n,math,flags,problems,wrange", CASES, ids=[c[0] for c in CASES])
def test_last_rollout_text(name, workload, n, math, flags, problems, wrange):
    cus = _lib.device_props(0).compute_units
    if cus != 256:
        pytest.skip("the literals are those of 256 CUs; this device has %d" % cus)
    planner = run_case(workload, n, math, flags, problems, wrange)
    assert planner.last_rollout_kernel() == EXPECTED[name]
    assert np.isfinite(planner.costs_d.copy_to_host()).all()
