#!/usr/bin/env python3
"""Wall time of one solve() with and without clearance rings, timed the way `bench.py --workload bb` times solve().
Two scenes, the handles of each taking turns in one process:

  single  N = 1000 rollouts, T = 50, crowd mode, 70 discs and 65 walls around the way from (0, 0) to (7, 5): without rings,
          with one ring and with four (clearance_staircase(0.5, obs_penalty / 4, R))
  fleet   the B = 8 disc fleet of tools/fleet_bodies_timing.py (N = 1024, T = 50, radius 0.54 m, margin 0.05 m): without
          rings and with two

    python tools/barebone_rings_timing.py [--steps 300] [--warmup 50] [--rounds 5] [--kinds single0,single1,single4,fleet0,fleet2]

A library without clearance rings (an earlier commit) times the handles without rings alone.  Prints one JSON line with the
per-round and median us per solve()."""
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


def time_calls(call, steps, warmup):
    for _ in range(warmup):
        call()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    return 1e6 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kinds", default="single0,single1,single4,fleet0,fleet2",
                    help="which handles take turns: <scene><rings> (single0,fleet0: the process an earlier commit runs)")
    args = ap.parse_args()
    from mppi_numba_amd import barebone
    dt, t, obs_penalty = 0.1, 50, 1e6
    task = dict(dt=dt, goal_tolerance=0.3, dist_weight=10, lambda_weight=1.0, num_opt=1, u_std=np.array([1.0, 1.0]),
                vrange=np.array([0.0, 2.0]), wrange=np.array([-np.pi, np.pi]), obs_penalty=obs_penalty)

    def config(n):
        return barebone.Config(T=(t + 0.5) * dt, dt=dt, num_control_rollouts=n, num_vis_state_rollouts=4, seed=1,
                               enforce_recommended_limits=False, crowd=True)

    def with_rings(params, count):
        if count:
            params = dict(params, clearance_rings=barebone.clearance_staircase(0.5, obs_penalty / 4, count))
        return params

    def single(count):
        rng = np.random.default_rng(70)
        x0, goal = np.array([0.0, 0.0, np.pi / 4]), np.array([7.0, 5.0])
        s = rng.uniform(0.1, 0.9, (70, 1))
        pos = x0[:2] * (1 - s) + goal * s + rng.normal(0, 1.5, (70, 2))
        a = rng.uniform(-1.0, 8.0, (65, 2))
        seg = np.stack([a, a + rng.uniform(-0.8, 0.8, (65, 2))], axis=1)
        params = dict(task, x0=x0, xgoal=goal, obstacle_positions=pos.astype(np.float32),
                      obstacle_radius=rng.uniform(0.1, 0.4, 70).astype(np.float32), wall_segments=seg.astype(np.float32),
                      wall_halfwidth=rng.uniform(0.0, 0.1, 65).astype(np.float32))
        planner = barebone.MPPI_Numba(config(1000))
        planner.setup(with_rings(params, count))
        return planner

    def fleet(count):
        B = 8
        angle = 0.3 + np.arange(B) * (2 * np.pi / B)
        where = 4.0 * np.stack([np.cos(angle), np.sin(angle)], 1)
        x0s, goals = np.concatenate([where, (angle + np.pi)[:, None]], 1), -where
        batch = barebone.MPPI_Batch(config(1024), B)
        batch.setup(with_rings(dict(task, x0=x0s[0].copy(), xgoal=goals[0]), count), x0s, goals)
        batch.set_fleet(0.54, 0.05)
        return batch

    has_rings = hasattr(barebone, "clearance_staircase")
    kinds = [kind for kind in args.kinds.split(",") if kind.endswith("0") or has_rings]
    with contextlib.redirect_stdout(io.StringIO()):
        handles = {kind: (single if kind.startswith("single") else fleet)(int(kind[-1])) for kind in kinds}
    solve = {kind: [] for kind in kinds}
    for _ in range(args.rounds):
        for kind in kinds:
            solve[kind].append(time_calls(handles[kind].solve, args.steps, args.warmup))
    out = {"steps": args.steps, "rounds": args.rounds, "rings": has_rings}
    for kind in kinds:
        out[kind] = {"us_per_solve": solve[kind], "median_solve": statistics.median(solve[kind]),
                     "rollout_kernel": handles[kind].last_rollout_kernel()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
