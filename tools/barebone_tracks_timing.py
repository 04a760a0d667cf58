#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner with discs that move (params['obstacle_tracks'], L = T + 1 rows)
against the same discs standing still, timed the way `bench.py --workload bb` times solve(): at the notebook's shape
(N = 1000, T = 50, its two discs) on a single handle, and for a batch of B problems x N rollouts with K discs each.

    python tools/barebone_tracks_timing.py [--problems 64] [--n 1024] [--discs 4] [--steps 2000] [--warmup 200] [--rounds 3]

Static and tracks alternate, `rounds` times each; prints one JSON line with the per-round and median us per solve()."""
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


def alternate(static, tracks, steps, warmup, rounds):
    us = {"static": [], "tracks": []}
    for _ in range(rounds):
        us["static"].append(time_solves(static, steps, warmup))
        us["tracks"].append(time_solves(tracks, steps, warmup))
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"us_per_solve_static": us["static"], "us_per_solve_tracks": us["tracks"], "median_static": med["static"],
            "median_tracks": med["tracks"], "tracks_over_static": med["tracks"] / med["static"],
            "rollout_kernel_static": static.last_rollout_kernel(), "rollout_kernel_tracks": tracks.last_rollout_kernel()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--discs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from mppi_numba_amd.barebone import Config, MPPI_Batch, MPPI_Numba, constant_velocity_tracks
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    t = int(cfg_kwargs["T"] / cfg_kwargs["dt"])
    rng = np.random.default_rng(0)

    def with_tracks(p, pos, rad):
        q = {k: v for k, v in p.items() if k != "obstacle_positions"}
        q["obstacle_tracks"] = constant_velocity_tracks(pos, rng.uniform(-0.6, 0.6, (len(rad), 2)), cfg_kwargs["dt"], t + 1)
        q["obstacle_radius"] = rad
        return q

    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        static, tracks = MPPI_Numba(Config(**cfg_kwargs)), MPPI_Numba(Config(**cfg_kwargs))
        static.setup(params)
        tracks.setup(with_tracks(params, params["obstacle_positions"], params["obstacle_radius"]))
    out["single"] = dict(alternate(static, tracks, args.steps, args.warmup, args.rounds), n=cfg_kwargs["num_control_rollouts"],
                         t=t, discs=len(params["obstacle_radius"]), rows=t + 1)
    bkw = dict(cfg_kwargs, num_control_rollouts=args.n, enforce_recommended_limits=False)
    x0s = np.tile(np.asarray(params["x0"], dtype=np.float32), (args.problems, 1))
    x0s[:, :2] += rng.uniform(-0.5, 0.5, (args.problems, 2)).astype(np.float32)
    pos = rng.uniform(1.0, 6.0, (args.discs, 2))
    rad = rng.uniform(0.3, 1.0, args.discs)
    bparams = dict(params, obstacle_positions=pos, obstacle_radius=rad)
    with contextlib.redirect_stdout(io.StringIO()):
        static, tracks = MPPI_Batch(Config(**bkw), args.problems), MPPI_Batch(Config(**bkw), args.problems)
        static.setup(bparams, x0s)
        tracks.setup(with_tracks(bparams, pos, rad), x0s)
    steps, warmup = max(1, args.steps // 10), max(1, args.warmup // 10)
    out["batch"] = dict(alternate(static, tracks, steps, warmup, args.rounds), problems=args.problems, n=args.n, t=t,
                        discs=args.discs, rows=t + 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
