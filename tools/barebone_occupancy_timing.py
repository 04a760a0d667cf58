#!/usr/bin/env python3
"""Wall time of one solve() of the barebone planner with an occupancy grid (params['occupancy']), timed the way
`bench.py --workload bb` times solve(): the notebook's shape (N = 1000, T = 50) in crowd mode, in a room of eight walls
rasterised onto a grid of 200 x 200 cells, handles side by side in one process:
  off    the same handle without the key (and without the room: the default form)
  grid   the room as params['occupancy']
  discs  the same room as what exists without the key: every occupied cell a disc of radius inflate at the cell's centre
and the field build alone at 200 x 200 and at 512 x 512: the rise of a solve() that follows changed cells (two sets of cells
alternate, so every solve builds) over a solve() that follows unchanged cells, hand-over included in both.

    python tools/barebone_occupancy_timing.py [--steps 2000] [--warmup 200] [--rounds 3]

The handles alternate, `rounds` times each; prints one JSON line."""
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


def time_solves(planner, steps, warmup, cells=None):
    """us per solve(); cells: the sets of cells that alternate from solve to solve (None: nothing changes)."""
    def one(k):
        if cells is not None:
            planner.params["occupancy"]["cells"] = cells[k % len(cells)]
        planner.solve()
    for k in range(warmup):
        one(k)
    t0 = time.perf_counter()
    for k in range(steps):
        one(k)
    return 1e6 * (time.perf_counter() - t0) / steps


def room(scale=1.0):
    """Eight walls in a square of 6.4 m * scale: the outline, a partition with a door, and two screens."""
    from mppi_numba_amd.barebone import polyline_walls
    outline = polyline_walls([(0.3, 0.3), (6.1, 0.3), (6.1, 6.1), (0.3, 6.1)], closed=True)
    inner = np.float32([[[3.2, 0.3], [3.2, 2.6]], [[3.2, 3.6], [3.2, 6.1]], [[1.2, 4.2], [2.4, 4.2]], [[4.2, 2.0], [5.4, 2.0]]])
    return np.concatenate([outline, inner]) * np.float32(scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from mppi_numba_amd.barebone import Config, MPPI_Numba, rasterise_obstacles
    import bench
    cfg_kwargs, params = bench.barebone_problem()
    params = dict(params, x0=np.array([1.0, 1.0, np.pi / 4]), xgoal=np.array([5.2, 1.0]))
    params.pop("obstacle_positions", None)
    params.pop("obstacle_radius", None)
    inflate = 0.1

    def occupancy(shape, res, scale, shift=0):
        cells = rasterise_obstacles((0.0, 0.0), res, shape, room(scale), 0.05 * scale)
        return dict(origin=(0.0, 0.0), resolution=res, cells=np.roll(cells, shift, axis=1), inflate=inflate, substeps=1)

    occ = occupancy((200, 200), 0.032, 1.0)
    iy, ix = np.nonzero(occ["cells"])
    centres = np.stack([(ix + 0.5) * 0.032, (iy + 0.5) * 0.032], axis=1).astype(np.float32)
    as_discs = dict(params, obstacle_positions=centres, obstacle_radius=np.full(len(centres), inflate, np.float32))
    with contextlib.redirect_stdout(io.StringIO()):
        off, grid, discs, changing, large, large_changing = (MPPI_Numba(Config(crowd=True, **cfg_kwargs)) for _ in range(6))
        off.setup(params)
        grid.setup(dict(params, occupancy=occ))
        discs.setup(as_discs)
        changing.setup(dict(params, occupancy=dict(occ)))
        big = occupancy((512, 512), 0.0125, 1.0)
        large.setup(dict(params, occupancy=big))
        large_changing.setup(dict(params, occupancy=dict(big)))
    alternate = {"200x200": [occ["cells"], occupancy((200, 200), 0.032, 1.0, 1)["cells"]],
                 "512x512": [big["cells"], occupancy((512, 512), 0.0125, 1.0, 1)["cells"]]}
    runs = (("off", off, None), ("grid", grid, None), ("discs", discs, None), ("grid_changing", changing, alternate["200x200"]),
            ("grid512", large, None), ("grid512_changing", large_changing, alternate["512x512"]))
    us = {name: [] for name, _, _ in runs}
    for _ in range(args.rounds):
        for name, planner, cells in runs:
            us[name].append(time_solves(planner, args.steps, args.warmup, cells))
    med = {k: statistics.median(v) for k, v in us.items()}
    built = changing.occupancy_fields_built
    assert built >= args.rounds * args.steps, built
    out = {"n": cfg_kwargs["num_control_rollouts"], "t": int(cfg_kwargs["T"] / cfg_kwargs["dt"]), "num_opt": int(params["num_opt"]),
           "occupied_cells": int(len(centres)), "us_per_solve": us, "median": med,
           "grid_minus_off": med["grid"] - med["off"], "discs_minus_grid": med["discs"] - med["grid"],
           "us_field_200x200": med["grid_changing"] - med["grid"], "us_field_512x512": med["grid512_changing"] - med["grid512"],
           "kernels": {name: planner.last_rollout_kernel() for name, planner, _ in runs[:3]}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
