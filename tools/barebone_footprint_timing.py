#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner in crowd mode with a body footprint (params['footprint']: the footprint
forms of k_rollout_barebone_crowd), timed the way tools/barebone_walls_timing.py times solve(): at the notebook's shape
(N = 1000, T = 50) with 20 static discs and 8 walls, and side by side no footprint, the point footprint [[0, 0, 0]] (the
same costs through the footprint form: what the form itself costs), and rectangle_footprint(0.5, 0.5, 0.4) with 3 and with
8 discs.

    python tools/barebone_footprint_timing.py [--steps 1000] [--warmup 100] [--rounds 3] [--limit 120]

One child process under a time limit of --limit seconds holds one handle per footprint; the handles take turns, `rounds`
times each, so every footprint is compared with the others in the same run.  Prints one JSON line and a markdown table; the
spread of a row is (max - min) of its rounds."""
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

DISCS, WALLS = 20, 8
CASES = ("none", "point", "rectangle 3", "rectangle 8")


def footprint_of(case):
    from mppi_numba_amd.barebone import rectangle_footprint
    if case == "none":
        return None
    if case == "point":
        return np.zeros((1, 3), dtype=np.float32)
    return rectangle_footprint(0.5, 0.5, 0.4, int(case.split()[1]))


def measure(args):
    from barebone_crowd_timing import time_solves
    from barebone_walls_timing import scene_walls
    from mppi_numba_amd.barebone import Config, MPPI_Numba
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    t = int(cfg_kwargs["T"] / cfg_kwargs["dt"])
    rng = np.random.default_rng(0)
    q = dict(params)
    q["obstacle_positions"] = rng.uniform(1.0, 6.0, (DISCS, 2))
    q["obstacle_radius"] = rng.uniform(0.3, 1.0, DISCS)
    q["wall_segments"], q["wall_halfwidth"] = scene_walls(rng, WALLS), 0.1
    planners = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for case in CASES:
            planners[case] = MPPI_Numba(Config(**dict(cfg_kwargs, crowd=True)))
            with_body = dict(q)
            if footprint_of(case) is not None:
                with_body["footprint"] = footprint_of(case)
            planners[case].setup(with_body)
    us = {case: [] for case in CASES}
    for _ in range(args.rounds):
        for case in CASES:
            us[case].append(time_solves(planners[case], args.steps, args.warmup))
    out = dict(n=cfg_kwargs["num_control_rollouts"], t=t, discs=DISCS, walls=WALLS, cases=list(CASES),
               us_per_solve=us, median={c: statistics.median(us[c]) for c in CASES},
               spread={c: max(us[c]) - min(us[c]) for c in CASES},
               rollout_kernel={c: planners[c].last_rollout_kernel() for c in CASES})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds the measurement may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--rounds", str(args.rounds)]
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
    print("\n| footprint | us per solve(), median | rounds | spread | kernel |\n|---|---|---|---|---|")
    for c in r["cases"]:
        print("| %s | %.1f | %s | %.1f | %s |" % (c, r["median"][c], " ".join("%.1f" % v for v in r["us_per_solve"][c]),
                                               r["spread"][c], r["rollout_kernel"][c].replace("k_rollout_barebone", "")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
