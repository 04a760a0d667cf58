#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner with the guide round the walls (params['guide']) against the same
handle without it, timed the way `bench.py --workload bb` times solve(): the notebook's shape (N = 1000, T = 50) in crowd
mode, in a room of eight walls on a grid of 64 x 64 cells, two handles side by side in one process.  Beside it the guide's
refresh alone -- refresh_guide(), a launch and a wait for the stream, by the host's clock: the rows only (nothing changed),
and the field and the rows (the goal alternates between two places, so every call builds) -- at 64 x 64 and at 192 x 192
in a spiral of walls; and the rollout and update launches of the loop (mppi_planner_time_kernels) to hold the rows against.
The difference "field and rows" minus "rows" is the field build; both contain the same launch and wait.

    python tools/barebone_guide_timing.py [--steps 2000] [--warmup 200] [--rounds 3] [--reps 200]

Off and on alternate, `rounds` times each; prints one JSON line."""
import argparse
import contextlib
import ctypes as C
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


def time_refresh(planner, reps, goals):
    """us per refresh_guide(); goals: the places the goal alternates between (one: nothing changes, rows only)."""
    for k in range(10):
        planner.params["xgoal"] = goals[k % len(goals)]
        planner.refresh_guide()
    built = planner.guide_fields_built
    t0 = time.perf_counter()
    for k in range(reps):
        planner.params["xgoal"] = goals[k % len(goals)]
        planner.refresh_guide()
    us = 1e6 * (time.perf_counter() - t0) / reps
    assert planner.guide_fields_built - built == (reps if len(goals) > 1 else 0)
    return us


def kernel_times(planner, reps):
    from mppi_numba_amd import _lib
    roll, upd = C.c_float(0), C.c_float(0)
    _lib.call("mppi_planner_time_kernels", planner._handle, None, None, reps, C.byref(roll), C.byref(upd))
    return {"us_rollout": roll.value, "us_update": upd.value}


def room():
    """Eight walls in a 6.4 m square: the outline, a partition with a door, and two screens."""
    from mppi_numba_amd.barebone import polyline_walls
    outline = polyline_walls([(0.3, 0.3), (6.1, 0.3), (6.1, 6.1), (0.3, 6.1)], closed=True)
    inner = np.float32([[[3.2, 0.3], [3.2, 2.6]], [[3.2, 3.6], [3.2, 6.1]], [[1.2, 4.2], [2.4, 4.2]], [[4.2, 2.0], [5.4, 2.0]]])
    return np.concatenate([outline, inner])


def spiral(lo=0.5, hi=18.7, s=0.6):
    """A rectangular spiral of walls, s from turn to turn: the longest shortest path a 19.2 m square holds."""
    pts, length, k = [(lo, lo)], hi - lo, 0
    while length > s:
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[k % 4]
        pts.append((pts[-1][0] + dx * length, pts[-1][1] + dy * length))
        k += 1
        if k >= 3 and k % 2 == 1:
            length -= s
    pts = np.float32(pts)
    return np.stack([pts[:-1], pts[1:]], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--refresh-only", default=None, choices=["64x64", "192x192_spiral"], dest="refresh_only",
                    help="only the refreshes of one grid, rows only and with the field: for a kernel trace "
                         "(rocprofv3 --kernel-trace --stats -- python tools/barebone_guide_timing.py --refresh-only ...)")
    args = ap.parse_args()
    from mppi_numba_amd.barebone import Config, MPPI_Numba
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    params = dict(params, x0=np.array([1.0, 1.0, np.pi / 4]), xgoal=np.array([5.2, 1.0]), wall_segments=room(), wall_halfwidth=0.05)
    guide = dict(origin=(0.0, 0.0), resolution=0.1, shape=(64, 64))
    big = dict(params, x0=np.array([0.8, 0.8, 0.0]), xgoal=np.array([9.5, 9.9]), wall_segments=spiral(), wall_halfwidth=0.0,
               guide=dict(origin=(0.0, 0.0), resolution=0.1, shape=(192, 192)))
    with contextlib.redirect_stdout(io.StringIO()):
        off, on, large = (MPPI_Numba(Config(crowd=True, **cfg_kwargs)) for _ in range(3))
        off.setup(params)
        on.setup(dict(params, guide=guide))
        large.setup(big)
    us = {"off": [], "on": []}
    for _ in range(0 if args.refresh_only else args.rounds):
        us["off"].append(time_solves(off, args.steps, args.warmup))
        us["on"].append(time_solves(on, args.steps, args.warmup))
    med = {k: statistics.median(v) if v else None for k, v in us.items()}
    refresh = {}
    for name, planner, goals in (("64x64", on, [np.array([5.2, 1.0]), np.array([5.2, 5.0])]),
                                 ("192x192_spiral", large, [np.array([9.5, 9.9]), np.array([9.8, 9.9])])):
        if args.refresh_only not in (None, name):
            continue
        rows_only = time_refresh(planner, args.reps, goals[:1])
        with_field = time_refresh(planner, args.reps, goals)
        refresh[name] = {"us_refresh_rows": rows_only, "us_refresh_field_and_rows": with_field, "us_field": with_field - rows_only,
                         "status": int(planner.guide_status())}
    out = {"n": cfg_kwargs["num_control_rollouts"], "t": int(cfg_kwargs["T"] / cfg_kwargs["dt"]), "num_opt": int(params["num_opt"]),
           "walls": len(params["wall_segments"]), "us_per_solve_off": us["off"], "us_per_solve_on": us["on"], "median_off": med["off"],
           "median_on": med["on"], "refresh": refresh}
    if not args.refresh_only:
        out.update(on_minus_off=med["on"] - med["off"], kernels_off=kernel_times(off, args.reps), kernels_on=kernel_times(on, args.reps),
                   rollout_kernel=on.last_rollout_kernel())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
