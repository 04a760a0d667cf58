#!/usr/bin/env python3
"""Wall time of solve() and of rollout() of a barebone handle in crowd mode that holds S disc samples
(params['obstacle_track_samples'], S = 1, 4, 8, 16) beside two baselines from code that was there before the samples:

  (a) the same kind of handle with plain params['obstacle_tracks'] -- one future: the floor of S = 1;
  (b) S consecutive rollout() calls on S handles with plain tracks, one per sample -- what a user had to do without the
      sample forms, and still without the tail over the S costs, which the host would owe.

N = 1024 rollouts, T = 100 steps, K = 20 discs (bench.barebone_problem() otherwise).

    python tools/barebone_disc_samples_timing.py [--steps 300] [--warmup 50] [--rounds 3] [--limit 300]

One child process under a time limit of --limit seconds holds all handles; they take turns, `rounds` times each, so the
figures are compared within one run.  What to look for: the sampled launch at S should cost less than (b) at every S, and
grow much more slowly than S x (a) -- the walk, the goal distance and the walls are shared, and the S cost chains overlap in
the lone cost wave.  Where it does not, tools/stamp_timeline.py says which wave bounds the interval.  Prints one JSON line
and a markdown table; the spread of a figure is (max - min) of its rounds."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SAMPLES = (1, 4, 8, 16)


def time_rollouts(planners, steps, warmup):
    for _ in range(warmup):
        for planner in planners:
            planner.rollout()
    t0 = time.perf_counter()
    for _ in range(steps):
        for planner in planners:
            planner.rollout()
    return 1e6 * (time.perf_counter() - t0) / steps


def measure(args):
    from barebone_crowd_timing import time_solves
    from mppi_numba_amd.barebone import Config, MPPI_Numba, sampled_tracks
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    n, t, K, dt = 1024, 100, 20, cfg_kwargs["dt"]
    cfg_kwargs = dict(cfg_kwargs, T=(t + 0.5) * dt, num_control_rollouts=n, crowd=True, enforce_recommended_limits=False)
    params = {k: v for k, v in params.items() if not k.startswith("obstacle_")}
    rng = np.random.default_rng(0)
    x0, goal = np.asarray(params["x0"], np.float64)[:2], np.asarray(params["xgoal"], np.float64)[:2]
    s = rng.uniform(0.2, 0.9, (K, 1))
    pos = x0 * (1 - s) + goal * s + rng.normal(0, 0.5, (K, 2))
    rad = rng.uniform(0.2, 0.5, K).astype(np.float32)
    smp = sampled_tracks(pos, rng.normal(0, 0.3, (K, 2)), dt, t + 1, 0.3, max(SAMPLES), seed=1)
    with contextlib.redirect_stdout(io.StringIO()):
        plain = [MPPI_Numba(Config(**cfg_kwargs)) for _ in range(max(SAMPLES))]
        for i, planner in enumerate(plain):
            planner.setup(dict(params, obstacle_tracks=smp[i], obstacle_radius=rad))
        sampled = {}
        for S in SAMPLES:
            sampled[S] = MPPI_Numba(Config(**cfg_kwargs))
            sampled[S].setup(dict(params, obstacle_track_samples=smp[:S], obstacle_radius=rad, cvar_alpha=0.5))
    us = {}
    for _ in range(args.rounds):
        us.setdefault("(a) plain tracks: solve()", []).append(time_solves(plain[0], args.steps, args.warmup))
        us.setdefault("(a) plain tracks: rollout()", []).append(time_rollouts(plain[:1], args.steps, args.warmup))
        for S in SAMPLES:
            us.setdefault("S=%d samples: solve()" % S, []).append(time_solves(sampled[S], args.steps, args.warmup))
            us.setdefault("S=%d samples: rollout()" % S, []).append(time_rollouts([sampled[S]], args.steps, args.warmup))
            us.setdefault("(b) %d plain rollout() calls" % S, []).append(time_rollouts(plain[:S], args.steps, args.warmup))
    kernels = {"S=%d samples: solve()" % S: sampled[S].last_rollout_kernel() for S in SAMPLES}
    kernels["(a) plain tracks: solve()"] = plain[0].last_rollout_kernel()
    print(json.dumps(dict(n=n, t=t, discs=K, figures=list(us), us_per_call=us, median={k: statistics.median(v) for k, v in us.items()},
                          spread={k: max(v) - min(v) for k, v in us.items()}, rollout_kernel=kernels)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
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
    print("\n| figure | us per call, median | rounds | spread | kernel |\n|---|---|---|---|---|")
    for name in r["figures"]:
        print("| %s | %.1f | %s | %.1f | %s |" % (name, r["median"][name], " ".join("%.1f" % v for v in r["us_per_call"][name]),
                                               r["spread"][name], r["rollout_kernel"].get(name, "").replace("k_rollout_barebone", "")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
