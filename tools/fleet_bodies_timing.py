#!/usr/bin/env python3
"""Wall time of one solve() of a barebone fleet, timed the way `bench.py --workload bb` times solve(): B = 8 robots x
N = 1024 rollouts, T = 50, crowd mode, the robots on a ring bound for its far side.  Three handles in one process taking
turns: the disc fleet (set_fleet, radius 0.54 m), a fleet of bodies with one disc (the same disc) and a fleet of bodies with
three (rectangle_footprint(0.5, 0.5, 0.4)); and refresh_fleet() alone on each, the refresh's share of a solve().

    python tools/fleet_bodies_timing.py [--problems 8] [--n 1024] [--steps 300] [--warmup 50] [--rounds 5] [--kinds discs,body1,body3]

A library without set_fleet_bodies (an earlier commit) times the disc fleet alone.  Prints one JSON line with the per-round
and median us per call."""
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
    ap.add_argument("--problems", type=int, default=8)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kinds", default="discs,body1,body3", help="which handles take turns (discs alone: the process an earlier commit runs)")
    args = ap.parse_args()
    from mppi_numba_amd import barebone
    B, dt, t = args.problems, 0.1, 50
    angle = 0.3 + np.arange(B) * (2 * np.pi / B)
    where = 4.0 * np.stack([np.cos(angle), np.sin(angle)], 1)
    x0s, goals = np.concatenate([where, (angle + np.pi)[:, None]], 1), -where
    params = dict(dt=dt, x0=x0s[0].copy(), xgoal=goals[0], goal_tolerance=0.3, dist_weight=10, lambda_weight=1.0, num_opt=1,
                  u_std=np.array([1.0, 1.0]), vrange=np.array([0.0, 2.0]), wrange=np.array([-np.pi, np.pi]), obs_penalty=1e6)

    def handle(kind):
        cfg = barebone.Config(T=(t + 0.5) * dt, dt=dt, num_control_rollouts=args.n, num_vis_state_rollouts=4, seed=1,
                              enforce_recommended_limits=False, crowd=True)
        batch = barebone.MPPI_Batch(cfg, B)
        batch.setup(params, x0s, goals)
        if kind == "discs":
            batch.set_fleet(0.54, 0.05)
        elif kind == "body1":
            batch.set_fleet_bodies(np.float32([[0.0, 0.0, 0.54]]), 0.05)
        else:
            batch.set_fleet_bodies(barebone.rectangle_footprint(0.5, 0.5, 0.4), 0.05)
        return batch

    kinds = [kind for kind in args.kinds.split(",") if kind == "discs" or hasattr(barebone.MPPI_Batch, "set_fleet_bodies")]
    with contextlib.redirect_stdout(io.StringIO()):
        handles = {kind: handle(kind) for kind in kinds}
    solve = {kind: [] for kind in kinds}
    refresh = {kind: [] for kind in kinds}
    for _ in range(args.rounds):
        for kind in kinds:
            solve[kind].append(time_calls(handles[kind].solve, args.steps, args.warmup))
        for kind in kinds:
            refresh[kind].append(time_calls(handles[kind].refresh_fleet, args.steps, args.warmup))
    out = {"problems": B, "n": args.n, "t": t, "steps": args.steps, "rounds": args.rounds}
    for kind in kinds:
        out[kind] = {"us_per_solve": solve[kind], "median_solve": statistics.median(solve[kind]),
                     "us_per_refresh": refresh[kind], "median_refresh": statistics.median(refresh[kind]),
                     "refresh_share": statistics.median(refresh[kind]) / statistics.median(solve[kind]),
                     "rollout_kernel": handles[kind].last_rollout_kernel()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
