#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner in crowd mode with walls that move (params['wall_tracks']:
k_rollout_barebone_crowd's CrowdWallTracks form) beside the same walls standing still (params['wall_segments']: the
CrowdWalls form), timed the way tools/barebone_walls_timing.py times solve(): at the notebook's shape (N = 1000, T = 50)
with 8 discs on tracks of T + 1 rows, and 16 and 64 walls.

    python tools/barebone_wall_tracks_timing.py [--steps 1000] [--warmup 100] [--rounds 3] [--limit 120] [--walls 16 64]

One child process under a time limit of --limit seconds holds two handles per wall count -- static walls, and tracks of
T + 1 rows whose row 0 is the static set --; the handles take turns, `rounds` times each, so every figure is compared with
the others in the same run.  The static scenes are those of `tools/barebone_walls_timing.py --walls <the same counts>`
(the same generator, drawn in the same order), so the static figures can be set beside that tool's on another commit.
Prints one JSON line and a markdown table; the spread of a handle is (max - min) of its rounds."""
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


def measure(args):
    from barebone_crowd_timing import time_solves
    from barebone_walls_timing import DISCS, scene_walls
    from mppi_numba_amd.barebone import Config, MPPI_Numba, constant_velocity_tracks, constant_velocity_walls
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    dt = cfg_kwargs["dt"]
    t = int(cfg_kwargs["T"] / dt)
    rng, wall_rng = np.random.default_rng(0), np.random.default_rng(1)
    pos = rng.uniform(1.0, 6.0, (DISCS, 2))
    q = {k: v for k, v in params.items() if k != "obstacle_positions"}
    q["obstacle_tracks"] = constant_velocity_tracks(pos, rng.uniform(-0.6, 0.6, (DISCS, 2)), dt, t + 1)
    q["obstacle_radius"] = rng.uniform(0.3, 1.0, DISCS)
    planners, names = {}, []
    with contextlib.redirect_stdout(io.StringIO()):
        for count in args.walls:
            seg = scene_walls(rng, count)
            moving = constant_velocity_walls(seg, wall_rng.uniform(-0.3, 0.3, (len(seg), 2)), dt, t + 1, at=0.0)
            for kind, walls in (("static", dict(wall_segments=seg)), ("tracks", dict(wall_tracks=moving))):
                name = "%d %s" % (count, kind)
                planners[name] = MPPI_Numba(Config(**dict(cfg_kwargs, crowd=True)))
                planners[name].setup(dict(q, wall_halfwidth=0.1, **walls))
                names.append(name)
    us = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            us[name].append(time_solves(planners[name], args.steps, args.warmup))
    out = dict(n=cfg_kwargs["num_control_rollouts"], t=t, discs=DISCS, handles=names,
               us_per_solve=us, median={k: statistics.median(v) for k, v in us.items()},
               spread={k: max(v) - min(v) for k, v in us.items()},
               rollout_kernel={k: planners[k].last_rollout_kernel() for k in names})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds the measurement may take")
    ap.add_argument("--walls", type=int, nargs="*", default=[16, 64])
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
    for name in r["handles"]:
        print("| %s | %.1f | %s | %.1f | %s |" % (name, r["median"][name], " ".join("%.1f" % v for v in r["us_per_solve"][name]),
                                               r["spread"][name], r["rollout_kernel"][name].replace("k_rollout_barebone", "")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
