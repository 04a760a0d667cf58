#!/usr/bin/env python3
"""Wall time of one solve() of a batched barebone handle in fleet mode (MPPI_Batch.set_fleet: every robot's walls rebuilt
on the device from the others' plans at the head of the call) beside the same batch holding per-problem wall tracks of
the same counts and rows that nobody refreshes (set_wall_sets): the difference is the refresh -- k_fleet_plans and
k_fleet_walls ahead of the iteration.  Timed the way tools/barebone_wall_tracks_timing.py times solve(), at
B = 64 problems x N = 1024 rollouts, T = 100 steps.

    python tools/barebone_fleet_timing.py [--steps 300] [--warmup 50] [--rounds 3] [--limit 300] [--robots 64]

One child process under a time limit of --limit seconds holds the two handles; they take turns, `rounds` times each, so the
figures are compared within one run.  The robots stand on a ring of 6 m and are bound for its far side.  The wall tracks of
the second handle are the fleet's own rows after the first handle's warm-up (fleet_walls()), so both read 63 walls x 100
rows of the same kind; the fleet's rows then go on following its controls, the tracks stand, which is as close as two
handles get without the host in the middle.  A third figure is refresh_fleet() alone: the two launches plus the wait for
the stream, an upper bound of what the refresh adds to a call that waits anyway.  Prints one JSON line and a markdown
table; the spread of a handle is (max - min) of its rounds."""
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


def measure(args):
    from barebone_crowd_timing import time_solves
    from mppi_numba_amd.barebone import Config, MPPI_Batch
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    B, n, t = args.robots, 1024, 100
    cfg_kwargs = dict(cfg_kwargs, T=(t + 0.5) * cfg_kwargs["dt"], num_control_rollouts=n, crowd=True,
                      enforce_recommended_limits=False)
    params = {k: v for k, v in params.items() if not k.startswith("obstacle_")}
    angle = np.arange(B) * (2 * np.pi / B)
    where = 6.0 * np.stack([np.cos(angle), np.sin(angle)], 1)
    x0s, goals = np.concatenate([where, (angle + np.pi)[:, None]], 1), -where
    with contextlib.redirect_stdout(io.StringIO()):
        fleet, tracks = MPPI_Batch(Config(**cfg_kwargs), B), MPPI_Batch(Config(**cfg_kwargs), B)
        fleet.setup(params, x0s, goals)
        fleet.set_fleet(0.25)
        for _ in range(args.warmup):
            fleet.solve()
        seg, hw, _ = fleet.fleet_walls()
        tracks.setup(params, x0s, goals, wall_sets=[(seg[b], hw[b]) for b in range(B)])
    planners = {"fleet": fleet, "wall tracks": tracks}
    us = {name: [] for name in planners}
    us["refresh_fleet() alone"] = []
    for _ in range(args.rounds):
        for name, planner in planners.items():
            us[name].append(time_solves(planner, args.steps, args.warmup))
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fleet.refresh_fleet()
        us["refresh_fleet() alone"].append(1e6 * (time.perf_counter() - t0) / args.steps)
    out = dict(robots=B, n=n, t=t, handles=list(us), us_per_solve=us, median={k: statistics.median(v) for k, v in us.items()},
               spread={k: max(v) - min(v) for k, v in us.items()},
               rollout_kernel={k: planners[k].last_rollout_kernel() for k in planners})
    out["refresh_us"] = out["median"]["fleet"] - out["median"]["wall tracks"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
    ap.add_argument("--robots", type=int, default=64)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--rounds", str(args.rounds), "--robots", str(args.robots)]
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
    print("\n| handle | us per call, median | rounds | spread | kernel |\n|---|---|---|---|---|")
    for name in r["handles"]:
        print("| %s | %.1f | %s | %.1f | %s |" % (name, r["median"][name], " ".join("%.1f" % v for v in r["us_per_solve"][name]),
                                               r["spread"][name], r["rollout_kernel"].get(name, "").replace("k_rollout_barebone", "")))
    print("\nthe refresh: %.1f us per solve() (fleet - wall tracks)" % r["refresh_us"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
