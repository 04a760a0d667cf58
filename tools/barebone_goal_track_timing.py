#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner with a goal that moves (params['goal_track'], T + 1 rows) beside the
same task with its static goal, timed the way `bench.py --workload bb` times solve(), all handles in one process and taking
turns: at the notebook's shape (N = 1000, T = 50, its two discs) on a single handle, for a batch of 64 problems x 1024
rollouts, and in crowd mode with 70 discs at the notebook's shape.

    python tools/barebone_goal_track_timing.py [--problems 64] [--n 1024] [--crowd-discs 70] [--steps 2000] [--warmup 200]
                                               [--rounds 3]

Static and goal track alternate, `rounds` times each; prints the table for profiles/HISTORY.md and one JSON line with the
per-round and median us per solve().  What to expect, written down before the first run: no more than the disc tracks' own
overhead at the notebook's shape (40.0 against 38.0 us, profiles/HISTORY.md) -- a goal track stages one slot per step where
two moving discs stage two."""
import argparse
import contextlib
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


def alternate(static, moving, steps, warmup, rounds):
    us = {"static": [], "goal_track": []}
    for _ in range(rounds):
        us["static"].append(time_solves(static, steps, warmup))
        us["goal_track"].append(time_solves(moving, steps, warmup))
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"us_per_solve_static": us["static"], "us_per_solve_goal_track": us["goal_track"], "median_static": med["static"],
            "median_goal_track": med["goal_track"], "goal_track_over_static": med["goal_track"] / med["static"],
            "rollout_kernel_static": static.last_rollout_kernel(), "rollout_kernel_goal_track": moving.last_rollout_kernel()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--crowd-discs", type=int, default=70)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from mppi_numba_amd.barebone import Config, MPPI_Batch, MPPI_Numba, constant_velocity_tracks
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    t = int(cfg_kwargs["T"] / cfg_kwargs["dt"])
    rng = np.random.default_rng(0)

    def with_goal_track(p):
        """The same goal, drifting at 0.3 m/s: T + 1 rows."""
        q = {k: v for k, v in p.items() if k != "xgoal"}
        q["goal_track"] = constant_velocity_tracks([p["xgoal"]], [[-0.3, 0.2]], cfg_kwargs["dt"], t + 1)[0]
        return q

    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        static, moving = MPPI_Numba(Config(**cfg_kwargs)), MPPI_Numba(Config(**cfg_kwargs))
        static.setup(params)
        moving.setup(with_goal_track(params))
    out["single"] = dict(alternate(static, moving, args.steps, args.warmup, args.rounds), n=cfg_kwargs["num_control_rollouts"],
                         t=t, discs=len(params["obstacle_radius"]), rows=t + 1)
    bkw = dict(cfg_kwargs, num_control_rollouts=args.n, enforce_recommended_limits=False)
    x0s = np.tile(np.asarray(params["x0"], dtype=np.float32), (args.problems, 1))
    x0s[:, :2] += rng.uniform(-0.5, 0.5, (args.problems, 2)).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        static, moving = MPPI_Batch(Config(**bkw), args.problems), MPPI_Batch(Config(**bkw), args.problems)
        static.setup(params, x0s)
        moving.setup(with_goal_track(params), x0s)
    steps, warmup = max(1, args.steps // 10), max(1, args.warmup // 10)
    out["batch"] = dict(alternate(static, moving, steps, warmup, args.rounds), problems=args.problems, n=args.n, t=t,
                        discs=len(params["obstacle_radius"]), rows=t + 1)
    pos = rng.uniform(1.0, 6.0, (args.crowd_discs, 2))
    rad = rng.uniform(0.1, 0.4, args.crowd_discs)
    cparams = dict(params, obstacle_positions=pos, obstacle_radius=rad)
    with contextlib.redirect_stdout(io.StringIO()):
        static, moving = MPPI_Numba(Config(crowd=True, **cfg_kwargs)), MPPI_Numba(Config(crowd=True, **cfg_kwargs))
        static.setup(cparams)
        moving.setup(with_goal_track(cparams))
    out["crowd"] = dict(alternate(static, moving, args.steps, args.warmup, args.rounds), n=cfg_kwargs["num_control_rollouts"],
                        t=t, discs=args.crowd_discs, rows=t + 1)
    print("| case | static goal, us per solve() | goal track of %d rows | ratio |" % (t + 1))
    print("|---|---|---|---|")
    for name, r in out.items():
        print("| %s | %.1f | %.1f | %.3f |" % (name, r["median_static"], r["median_goal_track"], r["goal_track_over_static"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
