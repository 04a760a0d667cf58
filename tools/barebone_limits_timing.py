#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner with acceleration limits (params['accel_limits']) against the same
planner without the key, timed the way `bench.py --workload bb` times solve(): at the notebook's shape (N = 1000, T = 50,
its two discs) on two handles side by side in one process; and the rollout and the update launch in the loop
(mppi_planner_time_kernels).  The pass's own kernel time comes from a `rocprofv3 --kernel-trace --stats` run of this script
(k_noise_limit in the statistics).

    python tools/barebone_limits_timing.py [--accel 1.0 2.0] [--steps 2000] [--warmup 200] [--rounds 3] [--reps 200]

Off and on alternate, `rounds` times each; prints one JSON line with the per-round and median us per solve()."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_solves(planner, steps, warmup):
    for _ in range(warmup):
        planner.solve()
    t0 = time.perf_counter()
    for _ in range(steps):
        planner.solve()
    return 1e6 * (time.perf_counter() - t0) / steps


def kernel_times(planner, reps):
    from mppi_numba_amd import _lib
    roll, upd = C.c_float(0), C.c_float(0)
    _lib.call("mppi_planner_time_kernels", planner._handle, None, None, reps, C.byref(roll), C.byref(upd))
    return {"us_rollout": roll.value, "us_update": upd.value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accel", type=float, nargs=2, default=[1.0, 2.0])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    from mppi_numba_amd.barebone import Config, MPPI_Numba
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    with contextlib.redirect_stdout(io.StringIO()):
        off, on = MPPI_Numba(Config(**cfg_kwargs)), MPPI_Numba(Config(**cfg_kwargs))
        off.setup(params)
        on.setup(dict(params, accel_limits=args.accel))
    us = {"off": [], "on": []}
    for _ in range(args.rounds):
        us["off"].append(time_solves(off, args.steps, args.warmup))
        us["on"].append(time_solves(on, args.steps, args.warmup))
    med = {k: statistics.median(v) for k, v in us.items()}
    out = {"n": cfg_kwargs["num_control_rollouts"], "t": int(cfg_kwargs["T"] / cfg_kwargs["dt"]), "num_opt": int(params["num_opt"]),
           "discs": len(params["obstacle_radius"]), "accel": args.accel,
           "us_per_solve_off": us["off"], "us_per_solve_on": us["on"], "median_off": med["off"], "median_on": med["on"],
           "on_minus_off": med["on"] - med["off"], "kernels_off": kernel_times(off, args.reps),
           "kernels_on": kernel_times(on, args.reps), "rollout_kernel": on.last_rollout_kernel()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
