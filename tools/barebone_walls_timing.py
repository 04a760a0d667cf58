#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner in crowd mode with wall obstacles (params['wall_segments']:
k_rollout_barebone_crowd's WALLS form), timed the way tools/barebone_crowd_timing.py times solve(): at the notebook's
shape (N = 1000, T = 50) with 8 discs on tracks of T + 1 rows, and 0, 4, 16 and 64 walls side by side.

    python tools/barebone_walls_timing.py [--steps 1000] [--warmup 100] [--rounds 3] [--limit 120] [--walls 0 4 16 64]

One child process under a time limit of --limit seconds holds one handle per wall count; the handles take turns, `rounds`
times each, so every count is compared with the others in the same run.  Prints one JSON line and a markdown table; the
spread of a count is (max - min) of its rounds."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DISCS = 8


def scene_walls(rng, count):
    """`count` walls of a building around the notebook's task (start (0, 0), goal (7, 5) in bench.barebone_problem's
    scene): a room outline first, then partitions."""
    from mppi_numba_amd.barebone import polyline_walls
    outline = polyline_walls([[-1.0, -1.0], [8.0, -1.0], [8.0, 6.0], [-1.0, 6.0]], closed=True)
    a = rng.uniform(0.0, 7.0, (max(0, count - 4), 2))
    partitions = np.stack([a, a + rng.uniform(-1.5, 1.5, a.shape)], axis=1).astype(np.float32)
    return np.concatenate([outline, partitions])[:count]


def measure(args):
    from barebone_crowd_timing import time_solves
    from mppi_numba_amd.barebone import Config, MPPI_Numba, constant_velocity_tracks
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    dt = cfg_kwargs["dt"]
    t = int(cfg_kwargs["T"] / dt)
    rng = np.random.default_rng(0)
    pos = rng.uniform(1.0, 6.0, (DISCS, 2))
    q = {k: v for k, v in params.items() if k != "obstacle_positions"}
    q["obstacle_tracks"] = constant_velocity_tracks(pos, rng.uniform(-0.6, 0.6, (DISCS, 2)), dt, t + 1)
    q["obstacle_radius"] = rng.uniform(0.3, 1.0, DISCS)
    planners = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for count in args.walls:
            planners[count] = MPPI_Numba(Config(**dict(cfg_kwargs, crowd=True)))
            with_walls = dict(q)
            if count:
                with_walls["wall_segments"], with_walls["wall_halfwidth"] = scene_walls(rng, count), 0.1
            planners[count].setup(with_walls)
    us = {count: [] for count in args.walls}
    for _ in range(args.rounds):
        for count in args.walls:
            us[count].append(time_solves(planners[count], args.steps, args.warmup))
    out = dict(n=cfg_kwargs["num_control_rollouts"], t=t, discs=DISCS, walls=list(args.walls),
               us_per_solve={str(c): us[c] for c in args.walls},
               median={str(c): statistics.median(us[c]) for c in args.walls},
               spread={str(c): max(us[c]) - min(us[c]) for c in args.walls},
               rollout_kernel={str(c): planners[c].last_rollout_kernel() for c in args.walls})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds the measurement may take")
    ap.add_argument("--walls", type=int, nargs="*", default=[0, 4, 16, 64])
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--rounds", str(args.rounds), "--walls"] + [str(c) for c in args.walls]
    try:
        done = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        print("no result within %d s" % args.limit)
        return 1
    if done.returncode != 0:
        print("exit status %d\n%s" % (done.returncode, done.stderr[-2000:]))
        return 1
    line = done.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    r = json.loads(line)
    print("\n| walls | us per solve(), median | rounds | spread | kernel |\n|---|---|---|---|---|")
    for c in r["walls"]:
        c = str(c)
        print("| %s | %.1f | %s | %.1f | %s |" % (c, r["median"][c], " ".join("%.1f" % v for v in r["us_per_solve"][c]),
                                               r["spread"][c], r["rollout_kernel"][c].replace("k_rollout_barebone", "")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
