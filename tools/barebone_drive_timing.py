#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner with car-like steering (params['drive'] = 'car') against the same planner
without the key, timed the way `bench.py --workload bb` times solve(): at the notebook's shape (N = 1000, T = 50, its two
discs) on handles side by side in one process; and the rollout and the update launch in the loop
(mppi_planner_time_kernels).

The car adds one float32 product per step, off the heading chain -- but the host's bound on the heading increment becomes
dt * max|v| * max|kappa|, so with the notebook's ranges (0.628 rad) the car loses the rotation form the unicycle runs
(0.314 rad).  Both are timed: the notebook's wrange, and wrange * `--wscale` (default 0.5: rotation for either drive).

    python tools/barebone_drive_timing.py [--wscale 0.5] [--steps 2000] [--warmup 200] [--rounds 3] [--reps 200]

The handles alternate, `rounds` times each; prints one JSON line with the per-round and median us per solve()."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np

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
    ap.add_argument("--wscale", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    from mppi_numba_amd.barebone import Config, MPPI_Numba
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    narrow = dict(params, wrange=np.asarray(params["wrange"], dtype=np.float64) * args.wscale)
    tasks = {"unicycle": params, "car": dict(params, drive="car"),
             "unicycle_narrow": narrow, "car_narrow": dict(narrow, drive="car")}
    planners = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for name, task in tasks.items():
            planners[name] = MPPI_Numba(Config(**cfg_kwargs))
            planners[name].setup(task)
    us = {name: [] for name in tasks}
    for _ in range(args.rounds):
        for name, planner in planners.items():
            us[name].append(time_solves(planner, args.steps, args.warmup))
    out = {"n": cfg_kwargs["num_control_rollouts"], "t": int(cfg_kwargs["T"] / cfg_kwargs["dt"]), "num_opt": int(params["num_opt"]),
           "discs": len(params["obstacle_radius"]), "wscale": args.wscale, "us_per_solve": us,
           "median": {name: statistics.median(v) for name, v in us.items()},
           "kernels": {name: kernel_times(planner, args.reps) for name, planner in planners.items()},
           "rollout_kernel": {name: planner.last_rollout_kernel() for name, planner in planners.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
