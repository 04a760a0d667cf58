"""The launch choice of the map modes (csrc/map_plan.h: map_choose and what it is made of) against a table.

The header is plain C++: a small host program compiled with g++ reads states and prints choices.  The expected rows were
written by reading the launch ladders this function replaced (plan_lds_window, unclamped_lookup_ok, scan_plan_compute,
try_launch_pipe, launch_windowed_or_general, launch_rollout_speed_map), not by running it; every LDS size in the table
is worked out a second time here from the layouts the kernel headers document.

The states are those of tests/test_gpu_map_plan.py (whose recorded last_rollout texts are parsed here and held to the
same rows) and the rules no small GPU shape reaches cheaply.  The map quantities are those of bench.py's maps as an
MI355X reports them: 256 x 256 cells of 0.25 m in a ring of 2 zero-traction cells (260 x 260, pitch 264, origin -0.5 m),
traction bytes 0 .. 100 of 0.01 each, dt = 0.1 s (a float32), v in [0, 3] m/s, w in [-pi, pi], start (4 m, 4 m);
256 CUs, 160 KiB of LDS per CU.
"""
import math
import os
import re
import subprocess

import pytest

from test_gpu_map_plan import CASES, EXPECTED

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "map_plan.h")

FIELDS = ["mode", "math", "debug_flags", "speculation_off", "n_local", "T", "num_cus", "lds_per_cu", "inst_set", "inst_tiles",
          "B", "cells16_valid", "cells16_with_risk", "pitch16", "rows", "cols", "lin_max_byte", "ang_max_byte", "sink_ring",
          "grid_packed", "theta_bounded", "lin_lo", "lin_ratio", "ang_lo", "ang_ratio", "dt", "res", "xlo", "ylo", "v_lo",
          "v_hi", "w_lo", "w_hi", "x0", "y0"]

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "%s"
int main() {
  for (;;) {
    MapHeld h;
    std::memset(&h, 0, sizeof(h));
    float px, py;  // a problem of a batched handle: where its window begins
    if (std::scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%lf %%lf %%lf %%lf %%f %%f %%f %%f %%f %%f %%f %%f %%f %%f %%f %%f",
                   &h.mode, &h.math, &h.debug_flags, &h.speculation_off, &h.n_local, &h.T, &h.num_cus, &h.lds_per_cu, &h.inst_set,
                   &h.inst_tiles, &h.B, &h.cells16_valid, &h.cells16_with_risk, &h.pitch16, &h.rows, &h.cols, &h.lin_max_byte,
                   &h.ang_max_byte, &h.sink_ring, &h.grid_packed, &h.theta_bounded, &h.lin_lo, &h.lin_ratio, &h.ang_lo,
                   &h.ang_ratio, &h.dt, &h.res, &h.xlo, &h.ylo, &h.vrange[0], &h.vrange[1], &h.wrange[0], &h.wrange[1], &h.x0,
                   &h.y0, &px, &py) != 37)
      break;
    // (launch_plan.h: map_held fills this from the handle's start and from every problem's of a batched handle)
    const MapStartBounds inside = map_start_bounds(h);
    h.starts_inside = map_start_inside(inside, h.x0, h.y0) && (!h.inst_set || map_start_inside(inside, px, py));
    {  // the bounds on x0 - lo say what the quotient says: around both ends, ulp by ulp, and for this state's start
      const float ends[2] = {inside.dx_end, inside.dy_end};
      const int counts[2] = {h.cols, h.rows};
      for (int a = 0; a < 2 && h.res > 0.0f; ++a) {
        float d = ends[a];
        for (int k = 0; k < 4; ++k) d = std::nextafter(d, 0.0f);
        for (int k = 0; k < 8; ++k, d = std::nextafter(d, INFINITY))
          if ((d / h.res < (float)counts[a]) != (d < ends[a])) { std::printf("bounds_disagree\n"); return 1; }
      }
      const float qx = (h.x0 - h.xlo) / h.res, qy = (h.y0 - h.ylo) / h.res;
      if (h.res > 0.0f && map_start_inside(inside, h.x0, h.y0) != (qx >= 0.0f && qx < (float)h.cols && qy >= 0.0f && qy < (float)h.rows)) {
        std::printf("bounds_disagree\n");
        return 1;
      }
    }
    const MapChoice c = map_choose(h);
    const MapReach r = map_reach(h);
    const WindowPlan& w = c.window;
    int pr0 = 0, pc0 = 0;
    window_origin(h, w, px, py, &pr0, &pc0);
    std::printf("family=%%d finite=%%d unclamped=%%d rotation=%%d pow2=%%d ", (int)c.family, (int)r.finite, (int)map_unclamped_ok(h),
                (int)map_rotation_ok(h), (int)map_res_pow2(h));
    std::printf("w.cells=%%d w.ok=%%d w.lds=%%zu w.r0=%%d w.c0=%%d w.rows=%%d w.cols=%%d w.progressive=%%d w.origins=%%d w.pr0=%%d w.pc0=%%d "
                "w.step_milli=%%ld ", (int)w.cells, (int)w.ok, w.ok ? w.lds : (size_t)0, w.r0, w.c0, w.rows, w.cols, w.progressive,
                (int)w.per_problem_origins, pr0, pc0, (long)(w.step_cells * 1000.0f + 0.5f));
    const ScanPlan& s = c.scan;
    std::printf("s.tile=%%d s.waves=%%d s.chunk_waves=%%d s.lds=%%zu s.pow2res=%%d s.exact=%%d s.direct=%%d s.speed=%%d s.rot_ok=%%d "
                "s.offset=%%d s.map_bytes=%%d s.small_offset=%%d ", s.tile, s.waves, s.chunk_waves, s.lds, (int)s.pow2res, (int)s.exact,
                (int)s.direct, (int)s.speed, (int)s.rot_ok, s.fallback_offset, s.fallback_map_bytes, s.small_offset);
    std::printf("p.triples=%%d p.chunk=%%d p.pow2res=%%d p.cc_lds=%%d p.lds=%%zu p.map_bytes=%%d p.grid=%%d p.block=%%d ", c.triples, c.chunk,
                (int)c.pow2res, (int)c.cc_lds, c.lds, c.map_bytes, c.grid, c.block);
    std::printf("f.waves=%%d f.block=%%d f.grid=%%d f.lone=%%d f.pow2res=%%d f.one_pass=%%d f.speed=%%d f.stash_steps=%%d f.stash_offset=%%d "
                "f.lds=%%zu ", c.waves, c.block, c.grid, (int)c.lone, (int)c.pow2res, (int)c.one_pass, (int)c.speed, c.stash_steps,
                c.stash_offset, c.lds);
    std::printf("g.windowed=%%d g.waves=%%d g.grid=%%d g.lds=%%zu\n", (int)c.windowed, c.waves, c.grid, c.lds);
  }
  return 0;
}
"""

SCAN, SCAN_EXACT, PIPE, FUSED, GENERAL = range(5)
DET, SPEED = 0, 1
EXACT, FAST = 0, 1
NO_SPECULATION, CC_GLOBAL, KEEP_SPECULATING, NO_SCAN_KERNEL, SCAN_FULL_TILES, NO_SCAN_DIRECT = 2, 8, 16, 32, 128, 1024
INF = float("inf")

BUDGET = 160 * 1024 - 1024  # what a launch may ask of a CU's LDS


def held(**over):
    """A state: the c2 bench map and parameters on an MI355X, N = 64, exact math, with `over` on top.  px, py: one problem
    of a batched handle."""
    s = dict(mode=DET, math=EXACT, debug_flags=0, speculation_off=0, n_local=64, T=100, num_cus=256, lds_per_cu=160 * 1024,
             inst_set=0, inst_tiles=0, B=1, cells16_valid=1, cells16_with_risk=0, pitch16=264, rows=260, cols=260,
             lin_max_byte=100, ang_max_byte=100, sink_ring=2, grid_packed=1, theta_bounded=1, lin_lo=0.0, lin_ratio=0.01,
             ang_lo=0.0, ang_ratio=0.01, dt=0.1, res=0.25, xlo=-0.5, ylo=-0.5, v_lo=0.0, v_hi=3.0, w_lo=-math.pi, w_hi=math.pi,
             x0=4.0, y0=4.0, px=0.0, py=0.0)
    assert set(over) <= set(s), over
    s.update(over)
    if s["mode"] == SPEED and "cells16_with_risk" not in over:
        s["cells16_with_risk"] = 1
    return s


def batch(per_problem, problems=64, **over):
    """A batched handle as c5 builds it (the sampler's table still reaches byte 100)."""
    return held(n_local=per_problem * problems, inst_set=1, inst_tiles=per_problem // 64, B=problems, **over)


# ---- the layouts of the kernel headers, worked out here -------------------------------------------------------------
def head(T):
    """[T] double2 control ratios | [T] float2 controls (rounded up to double2)"""
    return 16 * (T + (T + 1) // 2)


def window_lds(T, rows, cols, cell=2):
    return head(T) + rows * cols * cell


def ring(chunk):
    """k_rollout_pipe, per wave triple: xy[2][C][64] float2 + qd[2][C][64] double2 + cell[2][C][64] uint16"""
    return 2 * chunk * 64 * 8 + 2 * chunk * 64 * 16 + 2 * chunk * 64 * 2


def pipe_lds(T, rows, cols, triples, chunk, cc_lds):
    return window_lds(T, rows, cols) + triples * ring(chunk) + (triples * T * 64 * 8 if cc_lds else 0)


def scan_lds(R, W):
    """k_rollout_scan: records {sg, pen}[CHL] and cc[CHL] per (chunk, rollout), noise [8 W][R] float2, small arrays"""
    chl = 8 // (64 // R)
    return W * 64 * chl * 8 + W * 64 * chl * 4 + W * 8 * R * 8 + (R * (16 + 8 + 8 + 4) + 64 + 8 * 18 + W * 64)


def scan_exact_parts(W):
    """k_rollout_scan_exact: e2 | ccr | grp | p2 | small"""
    plane = W * 8 * 32 * 8
    small = W * 8 * (16 + 8) + 32 * 64 + 64 + 8 * 18 + 8 * 16 * 4 + 2 * W * 32 * 16
    return plane, plane, 2 * plane, (8 * W + 1) * 32 * 8, small


def fallback_bytes(W, rows, cols):
    """[8 W] float2 controls | 16-bit window | one chunk ring of 8 steps"""
    return 8 * W * 8 + rows * cols * 2 + ring(8)


def up16(x):
    return (x + 15) // 16 * 16


def scan_exact_lds(W, window=None, direct=False):
    """(lds, offset, map_bytes, small_offset) of a k_rollout_scan_exact launch; window: (rows, cols) or None"""
    e2, ccr, grp, p2, small = scan_exact_parts(W)
    total = e2 + ccr + grp + p2 + small
    if direct:  # noise | control-cost terms | {controls, window, ring} | small arrays
        need = up16(fallback_bytes(W, *window))
        return max(e2 + ccr + need + small, 40 * 1024), e2 + ccr, window[0] * window[1] * 2, e2 + ccr + need
    if window is None:
        return max(total, 40 * 1024), -1, 0, 0
    need = fallback_bytes(W, *window)
    if need <= grp + p2:  # in the LDS of the walks' groups and positions, dead by then
        return max(total, 40 * 1024), e2 + ccr, window[0] * window[1] * 2, 0
    if up16(total) + need <= BUDGET:  # behind everything
        return max(total, up16(total) + need), up16(total), window[0] * window[1] * 2, 0
    return max(total, 40 * 1024), -1, 0, 0  # no room: one wave rolls a failed tile out


def stash(T, lds_win, waves):
    """(steps, offset, lds): the noise of the first steps behind the window, in multiples of 8 steps"""
    off = up16(lds_win)
    steps = min((BUDGET - off) // (waves * 64 * 8), T) // 8 * 8
    return (steps, off, off + waves * steps * 64 * 8) if steps >= 8 else (0, 0, lds_win)


# ---- expected choices -------------------------------------------------------------------------------------------------
def window(rows, cols, r0=0, c0=0, T=100, cell=2, ok=1, progressive=1, origins=0, pr0=0, pc0=0, step_milli=1200):
    return {"w.cells": 1, "w.ok": ok, "w.lds": window_lds(T, rows, cols, cell) if ok else 0, "w.r0": r0, "w.c0": c0,
            "w.rows": rows, "w.cols": cols, "w.progressive": progressive, "w.origins": origins, "w.pr0": pr0, "w.pc0": pc0,
            "w.step_milli": step_milli}


def scan(family, tile, waves, chunk_waves, lds, pow2res=1, direct=0, speed=0, rot_ok=1, offset=-1, map_bytes=0, small_offset=0):
    return {"family": family, "s.tile": tile, "s.waves": waves, "s.chunk_waves": chunk_waves, "s.lds": lds, "s.pow2res": pow2res,
            "s.exact": int(family == SCAN_EXACT), "s.direct": direct, "s.speed": speed, "s.rot_ok": rot_ok, "s.offset": offset,
            "s.map_bytes": map_bytes, "s.small_offset": small_offset}


def pipe(triples, chunk, cc_lds, lds, map_bytes, grid, pow2res=1):
    return {"family": PIPE, "p.triples": triples, "p.chunk": chunk, "p.pow2res": pow2res, "p.cc_lds": cc_lds, "p.lds": lds,
            "p.map_bytes": map_bytes, "p.grid": grid, "p.block": 192 * triples}


def fused(waves, lds, lone=0, one_pass=0, speed=0, stash_steps=0, stash_offset=0, pow2res=1):
    return {"family": FUSED, "f.waves": waves, "f.block": 64 * waves, "f.lone": lone, "f.pow2res": pow2res,
            "f.one_pass": one_pass, "f.speed": speed, "f.stash_steps": stash_steps, "f.stash_offset": stash_offset, "f.lds": lds}


def general(windowed, waves, lds):
    return {"family": GENERAL, "g.windowed": windowed, "g.waves": waves, "g.lds": lds}


W142 = window(142, 144)  # T = 100 from (4 m, 4 m): 121 + 2 cells of reach around cell 18, clipped at row 0 / column 0
WIN = window_lds(100, 142, 144)
assert WIN == 43296
C5WIN = window_lds(100, 247, 256)  # a batch: the full reach square 2 * 123 + 1, columns (247 + 7) / 8 * 8 + 8
SPEEDWIN = window_lds(100, 142, 144, cell=4)
WHOLE200 = window_lds(200, 260, 264)  # T = 200: 243 cells of reach cover the map

# the states of tests/test_gpu_map_plan.py, by the name of the case
GPU_ROWS = {
    "c2_64_exact": (held(), dict(W142, **scan(SCAN_EXACT, 32, 16, 13, 151952, offset=53248, map_bytes=40896))),
    "c2_64_fast": (held(math=FAST), dict(W142, **scan(SCAN, 32, 13, 13, 68752))),
    "c2_64_fast_full_tiles": (held(math=FAST, debug_flags=SCAN_FULL_TILES), dict(W142, **scan(SCAN, 64, 13, 13, 136464))),
    "c2_64_exact_direct": (held(debug_flags=NO_SPECULATION),
                           dict(W142, **scan(SCAN_EXACT, 32, 16, 13, 140176, direct=1, offset=53248, map_bytes=40896, small_offset=121600))),
    "c2_64_exact_pipe": (held(debug_flags=NO_SCAN_KERNEL), dict(W142, **pipe(1, 8, 1, 121120, 40896, 1))),
    "c2_8192_last_scan": (held(n_local=8192), dict(W142, **scan(SCAN_EXACT, 32, 16, 13, 151952, offset=53248, map_bytes=40896))),
    "c2_8224_first_pipe": (held(n_local=8224), dict(W142, **pipe(1, 8, 1, 121120, 40896, 129))),
    "c2_16384_one_triple": (held(n_local=16384), dict(W142, **pipe(1, 8, 1, 121120, 40896, 256))),
    "c2_16448_two_triples": (held(n_local=16448), dict(W142, **pipe(2, 8, 0, 96544, 40896, 129))),
    "c2_32768_two_triples": (held(n_local=32768), dict(W142, **pipe(2, 8, 0, 96544, 40896, 256))),
    "c2_32832_fused_lone": (held(n_local=32832), dict(W142, **fused(4, 157984, lone=1, stash_steps=56, stash_offset=43296))),
    "c2_64_general_windowed": (held(debug_flags=NO_SCAN_KERNEL, w_lo=-4.0, w_hi=4.0), dict(W142, **general(1, 4, 43296))),
    "c2l_64_pipe": (held(T=200), dict(window(260, 264, T=200), **pipe(1, 6, 0, 162048, 137280, 1))),
    "c2m_64_exact": (held(mode=SPEED), dict(window(142, 144, cell=4), **scan(SCAN_EXACT, 32, 16, 13, 151952, speed=1))),
    "c2m_64_exact_fused": (held(mode=SPEED, debug_flags=NO_SCAN_KERNEL), dict(window(142, 144, cell=4), **fused(4, 84192, speed=1))),
    "c2m_64_fast": (held(mode=SPEED, math=FAST), dict(window(142, 144, cell=4), **fused(4, 84192, speed=1, one_pass=1))),
    # c5: problem 0 of bench.batch_problems starts at (52.1 m, 28.5 m), cell (210, 116): rows from 116 - 123 -> 0,
    # columns from 210 - 123 = 87 -> 80, shifted inwards to 264 - 256 = 8
    "c5_64_exact": (batch(64, px=52.09889602661133, py=28.52578353881836),
                    dict(window(247, 256, origins=1, pr0=0, pc0=8), **scan(SCAN_EXACT, 32, 16, 13, 151952))),
    "c5_256_exact": (batch(256), dict(window(247, 256, origins=1), **pipe(1, 8, 0, 155488, 126464, 256))),
    "c5_64_fast_fused": (batch(64, math=FAST, debug_flags=NO_SCAN_KERNEL), dict(window(247, 256, origins=1), **fused(1, 128864, one_pass=1))),
    "c5_256_fast_fused": (batch(256, math=FAST, debug_flags=NO_SCAN_KERNEL), dict(window(247, 256, origins=1), **fused(4, 128864, one_pass=1))),
}

# a taller map (300 rows) at T = 200: the window grows with the start row (4 + 244 rows of reach, clipped at row 0)
def tall(y0, **over):
    return held(T=200, rows=300, y0=y0, **over)


OTHER_ROWS = [
    # T = 104 against 105: 13 chunk waves are the exact kernel's limit; beyond, k_rollout_pipe
    (held(T=104), dict(window(146, 152, T=104), **scan(SCAN_EXACT, 32, 16, 13, 151952, offset=53248, map_bytes=146 * 152 * 2))),
    (held(T=105), dict(window(148, 152, T=105), **pipe(1, 8, 1, 127904, 148 * 152 * 2, 1))),
    # the fast kernel: a wave per 8 steps, 16 at the most; beyond, the one-pass fused kernel (the pipeline is exact only)
    (held(math=FAST, T=128), dict(window(175, 176, T=128), **scan(SCAN, 32, 16, 16, 84304))),
    (held(math=FAST, T=129), dict(window(176, 176, T=129), **fused(4, window_lds(129, 176, 176), one_pass=1))),
    # the fast kernel in full tiles: one round of 64-rollout workgroups
    (held(math=FAST, debug_flags=SCAN_FULL_TILES, n_local=16384), dict(W142, **scan(SCAN, 64, 13, 13, 136464))),
    (held(math=FAST, debug_flags=SCAN_FULL_TILES, n_local=16448), dict(W142, **fused(4, 43296, one_pass=1))),
    # chunks of 8 -> 6 -> 4 -> 2 steps as the window grows (248, 255, 262, 286 rows of 264 columns)
    (tall(0.6), dict(window(248, 264, T=200), **pipe(1, 8, 0, 162368, 248 * 264 * 2, 1))),
    (tall(2.3), dict(window(255, 264, T=200), **pipe(1, 6, 0, 159408, 255 * 264 * 2, 1))),
    (tall(4.0), dict(window(262, 264, T=200), **pipe(1, 4, 0, 156448, 262 * 264 * 2, 1))),
    (tall(10.0), dict(window(286, 264, T=200), **pipe(1, 2, 0, 162464, 286 * 264 * 2, 1))),
    # two triples only with chunks of 4 steps at the least: the whole-map window of T = 200 leaves chunks of 2 -> fused
    # (8 of the 200 steps' noise kept: 10 fit, rounded down to a multiple of 8)
    (held(T=200, n_local=32768), dict(window(260, 264, T=200), **fused(4, 158464, lone=1, stash_steps=8, stash_offset=WHOLE200))),
    # ... 5 waves: 8 steps still fit; 6 waves: 6 fit, none is kept
    (held(T=200, n_local=81920), dict(window(260, 264, T=200), **fused(5, WHOLE200 + 5 * 8 * 512, stash_steps=8, stash_offset=WHOLE200))),
    (held(T=200, n_local=98304), dict(window(260, 264, T=200), **fused(6, WHOLE200))),
    # three triples per CU: beyond the pipeline's launch bounds
    (held(n_local=49152), dict(W142, **fused(4, 157984, lone=1, stash_steps=56, stash_offset=43296))),
    # LONE at 4 waves per workgroup, not at 5 (46 steps fit beside 5 waves: 40 kept)
    (held(n_local=65536), dict(W142, **fused(4, 157984, lone=1, stash_steps=56, stash_offset=43296))),
    (held(n_local=65600), dict(W142, **fused(5, 43296 + 5 * 40 * 512, stash_steps=40, stash_offset=43296))),
    # the control-cost products kept out of LDS by the debug flag
    (held(debug_flags=NO_SCAN_KERNEL | CC_GLOBAL), dict(W142, **pipe(1, 8, 0, 69920, 40896, 1))),
    # batched handles: 3 tiles per problem have no divisor >= 4 -- 3 waves in one round, not 1 wave in three;
    # c5 at full size: 16 waves in one round; beside 16 waves no 8 steps of noise fit
    (batch(192, problems=256, math=FAST, debug_flags=NO_SCAN_KERNEL), dict(window(247, 256, origins=1), **fused(3, 128864, one_pass=1))),
    (batch(4096), dict(window(247, 256, origins=1), **fused(16, 128864))),
    # ... and a problem in the far corner: its window shifted inwards to the last 247 rows and 256 columns
    (batch(256, px=63.0, py=63.0), dict(window(247, 256, origins=1, pr0=13, pc0=8), **pipe(1, 8, 0, 155488, 126464, 256))),
    # a window clipped at the high borders, and one clipped nowhere (T = 40 from the middle: the failed tiles' region
    # does not fit in the walks' LDS and goes behind everything)
    (held(x0=60.0, y0=60.0), dict(window(141, 152, r0=119, c0=112), **scan(SCAN_EXACT, 32, 16, 13, 151952, offset=53248, map_bytes=141 * 152 * 2))),
    (held(T=40, x0=32.0, y0=32.0), dict(window(103, 112, r0=79, c0=72, T=40), **scan(SCAN_EXACT, 32, 10, 5, 110320, offset=60304, map_bytes=103 * 112 * 2))),
    # no sink ring: the address goes unclamped only where the reach square lies inside the map
    (held(T=40, x0=32.0, y0=32.0, sink_ring=0), dict(unclamped=1, **scan(SCAN_EXACT, 32, 10, 5, 110320, offset=60304, map_bytes=103 * 112 * 2))),
    (held(sink_ring=0), dict(unclamped=0, **scan(SCAN_EXACT, 32, 16, 13, 151952, pow2res=0, offset=53248, map_bytes=40896))),
    (held(sink_ring=0, debug_flags=NO_SCAN_KERNEL), dict(unclamped=0, **pipe(1, 8, 1, 121120, 40896, 1, pow2res=0))),
    # a start cell OUTSIDE the map: the ring stops who enters it, not who begins beyond it, and the unclamped address
    # saturates at 0 only -- the clamped address, whatever the ring (this row said 1 until the start cell was looked at;
    # on the GPU: tests/test_gpu_border.py)
    # (its window: the 123 cells of reach around cell -18, clipped at row 0 / column 0)
    (held(x0=-5.0, y0=-5.0), dict(window(106, 112), unclamped=0, **scan(SCAN_EXACT, 32, 16, 13, 151952, pow2res=0, offset=53248, map_bytes=106 * 112 * 2))),
    (held(x0=-5.0, y0=-5.0, debug_flags=NO_SCAN_KERNEL), dict(window(106, 112), unclamped=0, **pipe(1, 8, 1, pipe_lds(100, 106, 112, 1, 8, 1), 106 * 112 * 2, 1, pow2res=0))),
    # ... the map is 260 x 260 cells of 0.25 m from -0.5 m: the last cell inside begins at 64.25 m, the first one outside
    # at 64.5 m on the high sides and just below -0.5 m on the low sides
    (held(x0=64.49, y0=64.49), dict(unclamped=1, **{"s.pow2res": 1})),
    (held(x0=-0.5, y0=-0.5), dict(unclamped=1, **{"s.pow2res": 1})),
    (held(x0=64.5), dict(unclamped=0, **{"s.pow2res": 0})),
    (held(y0=64.5), dict(unclamped=0, **{"s.pow2res": 0})),
    (held(x0=-0.51), dict(unclamped=0, **{"s.pow2res": 0})),
    (held(y0=-0.51), dict(unclamped=0, **{"s.pow2res": 0})),
    # ... a batched handle: every problem's start counts (px, py), beside the handle's own
    (batch(64, px=63.0, py=63.0), dict(unclamped=1, **{"s.pow2res": 1})),
    (batch(64, px=64.5, py=10.0), dict(unclamped=0, **{"s.pow2res": 0})),
    (batch(64, px=10.0, py=-0.75), dict(unclamped=0, **{"s.pow2res": 0})),
    (batch(256, px=70.0, py=70.0), dict(window(247, 256, origins=1, pr0=13, pc0=8), unclamped=0, **pipe(1, 8, 0, 155488, 126464, 256, pow2res=0))),
    # ... the speed-map form of the time-parallel kernel has no unclamped address: the flag is its cell arithmetic alone
    (held(mode=SPEED, x0=70.0, y0=70.0), dict(unclamped=0, **{"s.pow2res": 1, "s.speed": 1})),
    # a reach that is not finite: the whole map, no progressive copy, the clamped address; a failed tile by one wave
    (held(v_hi=INF), dict(window(260, 264, progressive=0, step_milli=0), finite=0, unclamped=0, **scan(SCAN_EXACT, 32, 16, 13, 151952, pow2res=0))),
    # a resolution that is no power of two (same cells: the origin and the speed scaled with it)
    (held(res=0.75, xlo=-1.5, ylo=-1.5, x0=12.0, y0=12.0, v_hi=9.0, debug_flags=NO_SCAN_KERNEL), dict(pow2=0, **pipe(1, 8, 1, 121120, 40896, 1, pow2res=0))),
    # the speed-map mode refuses the direct form and fast math: the fused kernel
    (held(mode=SPEED, debug_flags=NO_SPECULATION), dict(window(142, 144, cell=4), **fused(4, 84192, speed=1))),
    (held(mode=SPEED, speculation_off=1), dict(window(142, 144, cell=4), **fused(4, 84192, speed=1))),
    # ... and has no windowed general kernel
    (held(mode=SPEED, debug_flags=NO_SCAN_KERNEL, w_lo=-4.0, w_hi=4.0), dict(rotation=0, **general(0, 1, 2400))),
    (held(mode=SPEED, cells16_with_risk=0), {"w.cells": 0, **general(0, 1, 2400)}),
    # a map the planner has stopped speculating on: direct; not for the fast kernel; the two debug flags
    (held(speculation_off=1), dict(W142, **scan(SCAN_EXACT, 32, 16, 13, 140176, direct=1, offset=53248, map_bytes=40896, small_offset=121600))),
    (held(speculation_off=1, math=FAST), dict(W142, **fused(4, 43296, one_pass=1))),
    (held(speculation_off=1, debug_flags=KEEP_SPECULATING), dict(W142, **scan(SCAN_EXACT, 32, 16, 13, 151952, offset=53248, map_bytes=40896))),
    (held(speculation_off=1, debug_flags=NO_SCAN_DIRECT), dict(W142, **pipe(1, 8, 1, 121120, 40896, 1))),
    # no 16-bit cells: the general kernel on the global cells; a heading that is not bounded: no rotation
    (held(cells16_valid=0), {"w.cells": 0, **general(0, 1, 2400)}),
    (held(theta_bounded=0, debug_flags=NO_SCAN_KERNEL), dict(rotation=1, **general(1, 4, 43296))),
    # fewer CUs: the borders move with them
    (held(n_local=4096, num_cus=128), dict(W142, **scan(SCAN_EXACT, 32, 16, 13, 151952, offset=53248, map_bytes=40896))),
    (held(n_local=4128, num_cus=128), dict(W142, **pipe(1, 8, 1, 121120, 40896, 65))),
]


@pytest.fixture(scope="module")
def choose(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("map_plan")
    src = tmp / "choose.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp / "choose"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])

    def run(states):
        text = "".join(" ".join(repr(s[k]) for k in FIELDS + ["px", "py"]) + "\n" for s in states)
        out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
        assert len(out) == len(states)
        return [{k: int(v) for k, v in (item.split("=") for item in line.split())} for line in out]
    return run


def test_map_choose_matches_the_table(choose):
    rows = list(GPU_ROWS.values()) + OTHER_ROWS
    for (state, want), got in zip(rows, choose([s for s, _ in rows])):
        for key, value in want.items():
            assert got[key] == value, "state %s: %s = %s, the table says %s" % (state, key, got[key], value)


def test_the_tables_lds_sizes_follow_from_the_kernels_layouts():
    """Every LDS size of the table once more, from the layouts (head, ring, scan_lds, scan_exact_parts, fallback_bytes)."""
    for state, want in list(GPU_ROWS.values()) + OTHER_ROWS:
        T, family = state["T"], want.get("family")
        W = (T + 7) // 8
        win = (want["w.rows"], want["w.cols"]) if want.get("w.ok") else None
        if "w.lds" in want and want["w.ok"]:
            assert want["w.lds"] == window_lds(T, *win, cell=4 if state["cells16_with_risk"] else 2) <= BUDGET
        if family == SCAN:
            assert want["s.lds"] == max(scan_lds(want["s.tile"], W), 40 * 1024), state
        elif family == SCAN_EXACT:
            if want["s.speed"]:
                win = None  # (32-bit cells: no exact schedule inside)
            elif win is None:  # (rows that give no window: the c2 window unless the state says otherwise)
                win = (want["s.map_bytes"] // 2 // 144, 144) if want["s.map_bytes"] == 40896 else (103, 112) if want["s.map_bytes"] else None
            lds = scan_exact_lds(W, win, direct=bool(want["s.direct"]))
            assert (want["s.lds"], want["s.offset"], want["s.map_bytes"], want["s.small_offset"]) == lds, (state, lds)
        elif family == PIPE:
            rows_cols = win or (want["p.map_bytes"] // 2 // 144, 144)
            assert want["p.map_bytes"] == rows_cols[0] * rows_cols[1] * 2
            assert want["p.lds"] == pipe_lds(T, *rows_cols, want["p.triples"], want["p.chunk"], want["p.cc_lds"]) <= BUDGET, state
            if want["p.chunk"] < 8:  # the next larger chunk did not fit
                assert pipe_lds(T, *rows_cols, want["p.triples"], want["p.chunk"] + 2, 0) > BUDGET, state
            if not want["p.cc_lds"] and not state["debug_flags"] & CC_GLOBAL:
                assert pipe_lds(T, *rows_cols, want["p.triples"], want["p.chunk"], 1) > BUDGET, state
        elif family == FUSED and win:
            lds_win = want["w.lds"]
            if want["f.one_pass"] or want["f.speed"]:
                assert (want["f.stash_steps"], want["f.lds"]) == (0, lds_win), state
            else:
                assert (want["f.stash_steps"], want["f.stash_offset"], want["f.lds"]) == stash(T, lds_win, want["f.waves"]), state


FIELD = re.compile(r"(\w+)=(\d+)x?(\d+)?")


def test_recorded_texts_agree_with_the_table():
    """tile, waves, lds, chunk, triples, window, waves_per_wg and noise_kept of the texts recorded on an MI355X
    (tests/test_gpu_map_plan.py) against the rows of the same states."""
    assert set(EXPECTED) == set(GPU_ROWS) == {c[0] for c in CASES}
    for name, text in EXPECTED.items():
        want = GPU_ROWS[name][1]
        said = {m.group(1): m for m in FIELD.finditer(text)}
        family = want["family"]
        kernel = text.split(" ")[0]
        assert kernel == {SCAN: "k_rollout_scan", SCAN_EXACT: "k_rollout_scan_exact", PIPE: "k_rollout_pipe",
                          FUSED: "k_rollout_fused<one pass>" if want.get("f.one_pass") else "k_rollout_fused",
                          GENERAL: "k_rollout_map"}[family].split(" ")[0], name
        checked = 0
        for key, field in (("tile", "s.tile"), ("waves", "s.waves"), ("chunk", "p.chunk"), ("triples_per_wg", "p.triples"),
                           ("noise_kept", "f.stash_steps"), ("lds", "s.lds" if family in (SCAN, SCAN_EXACT) else "p.lds"),
                           ("waves_per_wg", "f.waves" if family == FUSED else "g.waves")):
            if key in said:
                assert int(said[key].group(2)) == want[field], (name, key)
                checked += 1
        if "window" in said:
            assert (int(said["window"].group(2)), int(said["window"].group(3))) == (want["w.rows"], want["w.cols"]), name
            checked += 1
        assert checked >= 2, name  # (the general kernel's text says its waves and its window, no more)
