#!/usr/bin/env python3
"""In-kernel clock stamps of k_rollout_scan (developer tool; GPU box only).

    make -C mppi_numba_amd/csrc stamps
    MPPI_HIP_LIB=$PWD/build/libmppi_stamps.so python tools/scan_stamps.py [--n 8192] [--flags N]

Workgroup 5, cycles from the workgroup's first stamp, one row per wave.
k_rollout_scan (math fast): per wave (chunk): entered (0), had its noise and controls (1), reached
barrier 1 (2), barrier 2 (3), had its stage costs (4), reached barrier 3 (5), barrier 4 (6); wave 0 also:
costs written (7); every wave: end (8); wave 0: stage additions done (9), frozen steps done (10), weights (11).
k_rollout_scan_exact: wave 0 = heading walk, wave 1 = position walk: entered (0), walk done (1); wave 2 =
cost walk: stage walk done (1), frozen steps (2), control-cost walk (3), weights written (4), left group 0 (5), 6 (6),
9 (7), 10 .. 12 (10 .. 12); waves 3.. =
chunk waves: increments stored (1), sin / cos + position increments (3),
positions arrived (4), distances done and lookups requested (7), cells there (11), before the wait for the
earlier groups' events (12), events published (5), own events looked up and terminal cost (13), stopped rollouts
(14), selects (15), records stored (6); every wave: end (8), first barrier passed
(9); chunk waves: noise generated (10), control-cost products (2: after the records).
k_rollout_scan_exact as it is launched today: the cost walk is wave 1 (the x | y walk wave 4), and under each
workgroup's rows a derived table sets the stage-cost walk against its producers, group by group (stage_walk_table),
and a second one the position walk against the chunk waves' B phases (increments_table).
A stamp is not free: one more in the cost walker's loop moved its later stamps by 0.2-0.5k cycles
(profiles/HISTORY.md, "C2 rollout: the stage-cost walk")."""
import argparse
import contextlib
import ctypes as C
import io
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


# k_rollout_scan_exact: which chunk wave owns which group of 8 steps (kGroupOfWave), and the slots of the cost
# walker's row (wave 1) that hold "the walk left group g"
GROUP_OF_WAVE = {5: 0, 2: 1, 3: 2, 9: 3, 6: 4, 7: 5, 13: 6, 10: 7, 11: 8, 14: 9, 15: 10, 8: 11, 12: 12}
WALK_LEFT_SLOT = {0: 5, 6: 6, 9: 7, 10: 10, 11: 11, 12: 12}


def stage_walk_table(rows, t0):
    """The stage-cost walk against its producers: per group, when its records were ready (c_done raised: slot 6 of
    its chunk wave), when the cost walker left it, how far behind that is, and the walker's cycles per group since
    the previous group it stamps.  Last line: walk done (slot 1 of wave 1) minus the last c_done."""
    wave_of = {g: c for c, g in GROUP_OF_WAVE.items()}
    walker = rows[1]
    if not walker[0] or not walker[1]:
        return
    print(" stage-cost walk: group, records ready, walker left, behind, walker cycles per group")
    prev_g, prev_left, ready_last = None, None, 0
    for g in sorted(wave_of):
        ready = int(rows[wave_of[g]][6] - t0) if rows[wave_of[g]][6] else None
        ready_last = max(ready_last, ready or 0)
        left = int(walker[WALK_LEFT_SLOT[g]] - t0) if g in WALK_LEFT_SLOT and walker[WALK_LEFT_SLOT[g]] else None
        per = ""
        if left is not None:
            if prev_left is not None:
                per = "%.0f" % ((left - prev_left) / (g - prev_g))
            prev_g, prev_left = g, left
        print("  %5d %8s %8s %8s %8s" % (g, ready if ready is not None else "-", left if left is not None else "-",
                                        left - ready if None not in (left, ready) else "-", per))
    done = int(walker[1] - t0)
    print("  walk done %d, last records ready %d: %d behind" % (done, ready_last, done - ready_last))


def increments_table(rows, t0, glance_back=2):
    """The middle of the launch: position increments against the position walk, group by group.  Per group: when its
    heading increments were stored (slot 1 of its chunk wave), when its headings were there (th_done: NOT stamped --
    the theta walker carries no stamp inside its loop; derived from its end, slot 1 of wave 0, and a constant rate
    since group 0's increments, never earlier than the group's own increments + one group), the chunk wave behind its
    control-cost terms (2), behind b_done (3), xy_done seen (4), the lag xy_done seen - b_done, and whether the walk's
    look at b_done[g] can have hit: the look for group g is issued when the walk has published group g - glance_back
    (2: walk_groups_late_look, the walk as it is; 3: walk_groups, the walk before the look was moved), read here as
    `xy_done[g - glance_back] seen` by that group's chunk wave -- at most a poll late.  Groups 0 and 1 are waited for /
    looked at once at the start of the walk: no glance.  Last lines: both walks' ends, and the
    control-cost terms (cc_done raised: slot 2) against the last records (c_done: slot 6) -- the cost wave looks at
    cc_done with its last fetch."""
    wave_of = {g: c for c, g in GROUP_OF_WAVE.items() if rows[c][0]}
    if not wave_of or not rows[0][1] or not rows[4][1]:
        return
    groups = sorted(wave_of)
    at = lambda g, slot: int(rows[wave_of[g]][slot] - t0) if rows[wave_of[g]][slot] else None  # noqa: E731
    th_end, xy_end = int(rows[0][1] - t0), int(rows[4][1] - t0)
    a0 = at(0, 1) or 0
    rate = (th_end - a0) / len(groups)
    print(" position increments: group, wave, a_done, th_done (derived), ccr done, b_done, xy_done seen, B after th_done,"
          " xy - b, glance")
    th, misses = {}, 0
    for g in groups:
        a, ccr, b, xy = at(g, 1), at(g, 2), at(g, 3), at(g, 4)
        th[g] = int(max(th_end - (groups[-1] - g) * rate, (a or 0) + rate))
        if g >= 2 and b is not None:
            # (a look issued before the walk has published anything: when it starts on group 0)
            seen = at(g - glance_back, 4) if g >= glance_back else (at(0, 3) or 0)
            hit = seen is not None and b < seen
            misses += 0 if hit else 1
            glance = "hit" if hit else "MISS"
        else:
            glance = "-"
        print("  %5d %4d %8s %8d %8s %8s %8s %8s %8s   %s" % (
            g, wave_of[g], a, th[g], ccr, b, xy, b - th[g] if b is not None else "-",
            xy - b if None not in (xy, b) else "-", glance))
    cc_last = max(at(g, 2) or 0 for g in groups)
    c_last = at(groups[-1], 6)
    print("  theta walk done %d (%.0f per group), x | y walk done %d, %d behind; %d glances missed" % (
        th_end, rate, xy_end, xy_end - th_end, misses))
    if c_last is not None:
        print("  last control-cost terms %d, last group's records %d: the terms %d ahead" % (cc_last, c_last, c_last - cc_last))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--math", default="fast", choices=["fast", "exact"])
    ap.add_argument("--workload", default="c2", help="c2s / c2c: the exact three-wave schedule inside the kernel (direct mode; slots 11 .. 15 of waves 0 state, 1 cost, 2 producer: entered, first barrier passed, chunk 0 done, chunk 6 done, loop end)")
    ap.add_argument("--glance-back", type=int, default=2, dest="glance_back",
                    help="position-increments table: the x | y walk looks at b_done[g] when it has published group g - this many "
                         "(2: the kernel as it is; 3: a library from before the look was moved)")
    ap.add_argument("--iterations", type=int, default=1, help="iterations per call (>1: the last launch folds the previous update)")
    args = ap.parse_args()
    from mppi_numba_amd import _lib
    with contextlib.redirect_stdout(io.StringIO()):
        from bench import build_planner as build
        w, cfg, lin, ang, planner, params = build(args.workload, args.n, math=args.math)
        planner.set_debug_flags(args.flags)
        planner.solve()
        planner.iterate_async(20)
        planner.synchronize()
    buf = (C.c_ulonglong * 4096)()
    _lib.call("mppi_debug_read_stamps", buf, 4096, 1)
    for rep in range(3):
        planner.iterate_async(args.iterations)  # (the stamps of the last launch survive)
        planner.synchronize()
        _lib.call("mppi_debug_read_stamps", buf, 4096, 1)
        st = np.array(buf[:], dtype=np.uint64).astype(np.int64)
    print(planner.last_rollout_kernel())
    # workgroup 5 and (exact kernel) workgroup 200; walkers of a launch that applies the previous update itself:
    # 5 combine begins, 6 published, 7 sequence collected
    for title, first in (("workgroup 5", 64), ("workgroup 200", 1024)):
        rows = [st[first + 16 * c: first + 16 * c + 16] for c in range(16)]
        if not any(r[0] for r in rows):
            continue
        t0 = min(int(r[0]) for r in rows if r[0])
        print(title)
        print(" wave  " + "".join("%8d" % k for k in range(16)))
        for c, r in enumerate(rows):
            if r[0]:
                print("%5d  " % c + "".join("%8s" % (int(v - t0) if v else "-") for v in r))
        if args.math == "exact" and args.workload in ("c2", "c2m"):
            stage_walk_table(rows, t0)
            increments_table(rows, t0, args.glance_back)
    rows = [st[64 + 16 * c: 64 + 16 * c + 12] for c in range(16)]
    t0 = min(int(r[0]) for r in rows if r[0])
    # every workgroup's entry / exit (slots 2048 + 2 b, 2049 + 2 b) when the kernel records them
    ent, ext = st[2048:2048 + 1024:2], st[2049:2049 + 1024:2]
    if ent.any():
        e0 = ent[ent > 0].min()
        print("workgroup entries: first %d last %d; exits: first %d last %d (cycles from the first entry)" % (
            0, int(ent.max() - e0), int(ext[ext > 0].min() - e0), int(ext.max() - e0)))
        t0 = e0
    print("k_combine_tiles, first / last workgroup: entry, loads back, minimum, sums, end (cycles from the rollout workgroup's first stamp)")
    for base in (520, 528):
        print("   ", [int(v - t0) if v else None for v in st[base:base + 5]])


if __name__ == "__main__":
    main()
