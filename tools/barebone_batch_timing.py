#!/usr/bin/env python3
"""Wall time of one solve() of a barebone batch (barebone.MPPI_Batch) against the single-problem planner of
`bench.py --workload bb`: B problems x N rollouts x T steps, the notebook's task (cell 5) with its two discs shared.

    python tools/barebone_batch_timing.py [--problems 64] [--n 1024] [--t 50] [--steps 200] [--warmup 20]

Prints one JSON line: us per solve() of the batch, of the single problem, and their ratio."""
import argparse
import contextlib
import io
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--t", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from mppi_numba_amd.barebone import Config, MPPI_Batch, MPPI_Numba
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    cfg_kwargs = dict(cfg_kwargs, T=(args.t + 0.5) * cfg_kwargs["dt"], num_control_rollouts=args.n,
                      enforce_recommended_limits=False)
    rng = np.random.default_rng(0)
    x0s = np.tile(np.asarray(params["x0"], dtype=np.float32), (args.problems, 1))
    x0s[:, :2] += rng.uniform(-0.5, 0.5, (args.problems, 2)).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        single = MPPI_Numba(Config(**cfg_kwargs))
        single.setup(params)
        batch = MPPI_Batch(Config(**cfg_kwargs), args.problems)
        batch.setup(params, x0s)
    us_single = time_solves(single, args.steps, args.warmup)
    us_batch = time_solves(batch, args.steps, args.warmup)
    print(json.dumps({"problems": args.problems, "n": args.n, "t": args.t, "discs": len(params["obstacle_radius"]),
                      "us_per_solve_batch": us_batch, "us_per_solve_single": us_single,
                      "batch_over_single": us_batch / us_single,
                      "batch_over_problems_x_single": us_batch / (args.problems * us_single),
                      "rollout_kernel_batch": batch.last_rollout_kernel(),
                      "rollout_kernel_single": single.last_rollout_kernel()}))


if __name__ == "__main__":
    main()
