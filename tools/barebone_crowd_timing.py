#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner in crowd mode (Config(crowd=True): k_rollout_barebone_crowd) against
the default forms on the same moving discs, timed the way `bench.py --workload bb` times solve(): at the notebook's shape
(N = 1000, T = 50) with K discs on tracks of T + 1 rows.

    python tools/barebone_crowd_timing.py [--steps 1000] [--warmup 100] [--rounds 3] [--limit 120]

K in --both (default 2 4 8 16 32 64 80): crowd off and crowd on alternate in the same process, `rounds` times each -- the
comparison is always with crowd off in the same run.  K in --crowd-only (default 128 256 1024; the default forms cannot
launch them) and the fleet batch (B = 64 problems x N = 1024 rollouts, K = 63): crowd on alone.  Every measurement is a
child process of its own under a time limit of --limit seconds; after one that fails or runs out of time nothing further
starts.  Prints one JSON line per measurement and a markdown table at the end."""
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


def time_solves(planner, steps, warmup):
    for _ in range(warmup):
        planner.solve()
    t0 = time.perf_counter()
    for _ in range(steps):
        planner.solve()
    return 1e6 * (time.perf_counter() - t0) / steps


def measure(args):
    """One measurement, in this process: --one K (single handle) or --fleet."""
    from mppi_numba_amd.barebone import Config, MPPI_Batch, MPPI_Numba, constant_velocity_tracks
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    dt = cfg_kwargs["dt"]
    t = int(cfg_kwargs["T"] / dt)
    rng = np.random.default_rng(0)
    modes = (False, True) if args.with_off else (True,)
    planners = {}
    if args.fleet:
        B, n, K = 64, 1024, 63
        angle = np.arange(B) * (2 * np.pi / B)
        ring = 3.0 * np.stack([np.cos(angle), np.sin(angle)], 1) + 3.5
        x0s = np.concatenate([ring, (angle + np.pi)[:, None]], 1).astype(np.float32)
        goals = (7.0 - ring).astype(np.float32)
        tracks = constant_velocity_tracks(ring, (7.0 - 2 * ring) / 6.0, dt, t + 1)  # each robot straight to its goal, 1 m/s
        sets = [(np.ascontiguousarray(np.delete(tracks, b, axis=0)), np.full(B - 1, 0.35, np.float32)) for b in range(B)]
        bare = {k: v for k, v in params.items() if k not in ("obstacle_positions", "obstacle_radius")}
        with contextlib.redirect_stdout(io.StringIO()):
            for crowd in modes:
                planners[crowd] = MPPI_Batch(Config(**dict(cfg_kwargs, num_control_rollouts=n, crowd=crowd,
                                                           enforce_recommended_limits=False)), B)
                planners[crowd].setup(bare, x0s, goals, obstacle_sets=sets)
        shape = dict(problems=B, n=n, t=t, discs=K)
    else:
        K = args.one
        pos = rng.uniform(1.0, 6.0, (K, 2))
        q = {k: v for k, v in params.items() if k != "obstacle_positions"}
        q["obstacle_tracks"] = constant_velocity_tracks(pos, rng.uniform(-0.6, 0.6, (K, 2)), dt, t + 1)
        q["obstacle_radius"] = rng.uniform(0.3, 1.0, K)
        with contextlib.redirect_stdout(io.StringIO()):
            for crowd in modes:
                planners[crowd] = MPPI_Numba(Config(**dict(cfg_kwargs, crowd=crowd)))
                planners[crowd].setup(q)
        shape = dict(n=cfg_kwargs["num_control_rollouts"], t=t, discs=K)
    us = {crowd: [] for crowd in modes}
    for _ in range(args.rounds):
        for crowd in modes:
            us[crowd].append(time_solves(planners[crowd], args.steps, args.warmup))
    out = dict(shape, us_per_solve_crowd=us[True], median_crowd=statistics.median(us[True]),
               rollout_kernel_crowd=planners[True].last_rollout_kernel())
    if args.with_off:
        out.update(us_per_solve_off=us[False], median_off=statistics.median(us[False]),
                   rollout_kernel_off=planners[False].last_rollout_kernel())
        out["crowd_over_off"] = out["median_crowd"] / out["median_off"]
        out["same_result"] = bool(np.array_equal(planners[True].solve(), planners[False].solve()))  # (same seed, same count)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a measurement may take")
    ap.add_argument("--both", type=int, nargs="*", default=[2, 4, 8, 16, 32, 64, 80])
    ap.add_argument("--crowd-only", type=int, nargs="*", default=[128, 256, 1024])
    ap.add_argument("--no-fleet", action="store_true")
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fleet", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--with-off", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None or args.fleet:
        return measure(args)
    common = ["--warmup", str(args.warmup), "--rounds", str(args.rounds)]
    jobs = [(["--one", str(k), "--with-off", "--steps", str(args.steps)], "K = %d" % k) for k in args.both]
    jobs += [(["--one", str(k), "--steps", str(args.steps)], "K = %d" % k) for k in args.crowd_only]
    if not args.no_fleet:
        jobs.append((["--fleet", "--steps", str(max(1, args.steps // 10))], "fleet"))
    rows = []
    for extra, name in jobs:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra + common, timeout=args.limit,
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; nothing further is started" % (name, args.limit))
            return 1
        if done.returncode != 0:
            print("%s: exit status %d; nothing further is started\n%s" % (name, done.returncode, done.stderr[-2000:]))
            return 1
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        rows.append((name, json.loads(line)))
    print("\n| discs | crowd off, us per solve() | crowd on | on / off | crowd kernel |\n|---|---|---|---|---|")
    for name, r in rows:
        off = "%.1f" % r["median_off"] if "median_off" in r else "does not fit"
        ratio = "%.2f" % r["crowd_over_off"] if "median_off" in r else ""
        print("| %s | %s | %.1f | %s | %s |" % (name, off, r["median_crowd"], ratio,
                                              r["rollout_kernel_crowd"].replace("k_rollout_barebone", "")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
