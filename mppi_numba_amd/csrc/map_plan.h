// map_plan.h -- which kernel a rollout launch of the map modes (deterministic dynamics, speed map) runs and with what
// geometry, as a pure function of what the handle holds.  Plain C++ without a HIP type: a host program compiles it on
// its own (tests/test_map_plan.py pins the table).  map_held(p) (launch_plan.h) fills the state from a handle; the
// launchers there carry a choice out.  What depends on the running loop is not this choice's business: whether the launch
// generates its noise and the noise blocks of spare CUs are noise_plan.h's, a pending update update_plan.h's.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <initializer_list>

#include "../../include/mppi_hip.h"
#include "lds_layouts.h"

// What the choice depends on, and nothing else: no pointer.  map_held() zeroes it first, so two of them compare with
// memcmp (the planner caches the choice on the state it was computed from).
struct MapHeld {
  int mode, math, debug_flags, speculation_off;
  int n_local, T, num_cus, lds_per_cu;
  int inst_set, inst_tiles, B;                    // a batched handle: tiles of 64 rollouts per problem, problems
  int cells16_valid, cells16_with_risk, pitch16;  // the 16-bit (speed map: 32-bit) cells the LDS window is copied from
  int rows, cols, lin_max_byte, ang_max_byte, sink_ring, grid_packed;  // PackedMaps (handles.h)
  int theta_bounded;  // |theta| stays inside the two-term pi/2 reduction over the horizon (launch_rollout)
  int starts_inside;  // every start cell is a cell of the map (map_start_inside): x0, and each problem's of a batched handle
  double lin_lo, lin_ratio, ang_lo, ang_ratio;
  float dt, res, xlo, ylo, vrange[2], wrange[2], x0, y0;
  int drive;  // barebone mode: MPPI_DRIVE_UNICYCLE (0), or MPPI_DRIVE_CAR: wrange is the curvature range, the yaw rate v * kappa
};

inline int map_ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// ---- how far a rollout gets ----------------------------------------------------------------------------------------
// vmax, wmax: max |v|, max |w| of the control ranges (car mode: max |w| = max |v| * max |kappa|, the largest yaw rate a step
// can apply); trmax_*: max |traction| of the packed grids (barebone mode: 1);
// step_cells: cells per step at the most, dt * max|v| * max|traction| / res; reach_m: metres within the horizon, finite or not
struct MapReach {
  double vmax, wmax, trmax_lin, trmax_ang, step_cells, reach_m;
  bool finite;
};

inline MapReach map_reach(const MapHeld& h) {
  MapReach r;
  r.vmax = std::fmax(std::fabs((double)h.vrange[0]), std::fabs((double)h.vrange[1]));
  r.wmax = std::fmax(std::fabs((double)h.wrange[0]), std::fabs((double)h.wrange[1]));
  if (h.mode == MPPI_MODE_BAREBONE && h.drive == MPPI_DRIVE_CAR) r.wmax = r.vmax * r.wmax;
  r.trmax_lin = std::fmax(std::fabs(h.lin_lo), std::fabs(h.lin_lo + (double)h.lin_max_byte * h.lin_ratio));
  r.trmax_ang = h.mode == MPPI_MODE_BAREBONE
                    ? 1.0
                    : std::fmax(std::fabs(h.ang_lo), std::fabs(h.ang_lo + (double)h.ang_max_byte * h.ang_ratio));
  r.step_cells = (double)h.dt * r.vmax * r.trmax_lin / (double)h.res;
  r.reach_m = (double)h.T * (double)h.dt * r.vmax * r.trmax_lin;
  r.finite = std::isfinite(r.reach_m);
  return r;
}

// Incremental trig, (cos, sin) advanced by rotation: the host bounds the heading increment |dt * w * traction| by 0.36 rad
// (barebone mode: traction 1) and the horizon by 2000 steps.
inline bool map_rotation_ok(const MapHeld& h) {
  const MapReach r = map_reach(h);
  const double dmax = (double)h.dt * r.wmax * r.trmax_ang;
  return std::isfinite(dmax) && dmax <= 0.36 && h.T <= 2000;
}

// res == 2^k exactly: four-instruction cell coordinates
inline bool map_res_pow2(const MapHeld& h) {
  int res_exp = 0;
  return std::frexp((double)h.res, &res_exp) == 0.5;
}

// The exact schedule's state role (rollout_kernels.h, PipeWindow<POW2RES = true>) forms its LDS address without the
// [0, last] clamp -- one instruction per coordinate on the horizon's only dependent chain.  That is sound on a map no
// rollout can leave: the reference's padded maps (a ring of zero-traction cells at least as wide as one step is long:
// terrain.py:511-583 -- whoever enters it stays), or a reach square that lies strictly inside the map.  Anything else
// (an mppi_tdm filled through the C API without such a ring, a window clipped by the border) takes the variant with the
// exact floor division and the clamp, i.e. the border cell, like k_rollout_map and k_rollout_fused.
// Either argument holds only for a rollout that STARTS on the map: the ring stops who enters it, not who begins beyond
// it, and the float-to-unsigned conversion of the unclamped address saturates at 0 only, so a start cell beyond a high
// border would index past the window.  MapHeld::starts_inside says so for x0 and for every problem of a batched handle
// (tests/test_map_plan.py, tests/test_gpu_border.py).
// The test is the kernels' own arithmetic: d = x0 - lo in float32, and 0 <= d / res < cols (the quotient is exact where
// the answer matters, a power of two).  d / res grows with d, so the bound on the quotient is a bound on d, found once
// per state: a batched handle asks for every problem, several times an iteration.
struct MapStartBounds {
  float xlo, ylo, dx_end, dy_end;  // inside: 0 <= x0 - xlo < dx_end and 0 <= y0 - ylo < dy_end
};
inline float map_start_end(float res, int n) {  // the smallest d with d / res >= n; a resolution that is not positive: 0
  if (!(res > 0.0f) || !std::isfinite(res) || n <= 0) return 0.0f;
  float d = (float)n * res;
  while (d / res >= (float)n && d > 0.0f) d = std::nextafter(d, 0.0f);
  while (d / res < (float)n) d = std::nextafter(d, INFINITY);
  return d;
}
inline MapStartBounds map_start_bounds(const MapHeld& h) {
  return MapStartBounds{h.xlo, h.ylo, map_start_end(h.res, h.cols), map_start_end(h.res, h.rows)};
}
inline bool map_start_inside(const MapStartBounds& b, float x0, float y0) {
  const float dx = x0 - b.xlo, dy = y0 - b.ylo;
  return dx >= 0.0f && dx < b.dx_end && dy >= 0.0f && dy < b.dy_end;  // (a NaN start: no)
}

inline bool map_unclamped_ok(const MapHeld& h) {
  const MapReach r = map_reach(h);
  if (!std::isfinite(r.step_cells)) return false;
  if (!h.starts_inside) return false;
  if (h.grid_packed && (double)h.sink_ring >= std::ceil(r.step_cells + 1e-3)) return true;
  if (h.inst_set) return false;  // (per-problem windows are shifted inwards at the border)
  const double reach = std::ceil((double)h.T * r.step_cells) + 2.0;
  const double xi0 = std::floor(((double)h.x0 - (double)h.xlo) / (double)h.res);
  const double yi0 = std::floor(((double)h.y0 - (double)h.ylo) / (double)h.res);
  return yi0 - reach > 0.0 && yi0 + reach + 1.0 < (double)h.rows && xi0 - reach > 0.0 && xi0 + reach + 1.0 < (double)h.cols;
}

// ---- the LDS window ------------------------------------------------------------------------------------------------
// Whether the rollout can keep its map in LDS: the window of 16-bit cells (speed map: 32-bit, 16 bits + risk byte) must
// cover every cell reachable from the start within the horizon (plus a margin; columns in multiples of 8) and fit next
// to the staged controls.  A batched handle has one window SIZE for all problems (the full reach square, clipped to the
// map size) and one ORIGIN per problem, shifted inwards at the map border (window_origin).
struct WindowPlan {
  bool cells = false;  // the mode's cells exist: the fields below mean something
  bool ok = false;     // ... and the window fits
  size_t lds = 0;      // bytes of {staged controls, window}
  int r0 = 0, c0 = 0, rows = 0, cols = 0;
  float step_cells = 0.0f;  // the rollouts spread at most this far per step (0: unknown) ...
  int progressive = 0;      // ... so the window can be copied as the horizon advances
  bool per_problem_origins = false;
  long reach = 0;           // half width of the reach square in cells (where the window is one)
};

inline long map_cell(float x, float lo, float res) { return (long)std::floor(((double)x - (double)lo) / (double)res); }
inline size_t map_lds_head(int T) { return 16 * ((size_t)T + (size_t)(T + 1) / 2); }  // [T] double2 ratios | [T] float2 controls

inline WindowPlan map_window(const MapHeld& h) {
  WindowPlan w;
  if (!h.cells16_valid) return w;
  if (h.mode == MPPI_MODE_SPEED_MAP ? !h.cells16_with_risk : h.mode != MPPI_MODE_DET) return w;
  w.cells = true;
  const size_t head = map_lds_head(h.T);
  const size_t budget = (size_t)h.lds_per_cu - 1024;  // leave room for the runtime's own use
  const size_t cell_bytes = h.cells16_with_risk ? 4 : 2;
  const size_t whole = (size_t)h.rows * h.pitch16 * cell_bytes;
  const MapReach r = map_reach(h);
  w.step_cells = r.finite ? (float)r.step_cells : 0.0f;
  w.progressive = r.finite ? 1 : 0;
  size_t bytes = whole + 1;
  long r0 = 0, c0 = 0, wr = h.rows, wc = h.pitch16;
  if (r.finite) {
    const long reach = (long)std::ceil(r.reach_m / (double)h.res) + 2;
    w.reach = reach;
    if (h.inst_set) {
      wr = std::min((long)h.rows, 2 * reach + 1);
      wc = std::min((long)h.pitch16, (2 * reach + 1 + 7) / 8 * 8 + 8);
      bytes = (size_t)wr * (size_t)wc * cell_bytes;
    } else {
      const long xi0 = map_cell(h.x0, h.xlo, h.res), yi0 = map_cell(h.y0, h.ylo, h.res);
      r0 = std::max(0L, yi0 - reach);
      c0 = std::max(0L, xi0 - reach) / 8 * 8;
      const long r1 = std::min((long)h.rows, yi0 + reach + 1);
      const long c1 = std::min((long)h.pitch16, (std::min((long)h.cols, xi0 + reach + 1) + 7) / 8 * 8);
      if (r1 > r0 && c1 > c0) {
        wr = r1 - r0; wc = c1 - c0;
        bytes = (size_t)wr * (size_t)wc * cell_bytes;
      }
    }
  }
  const bool reach_window = bytes < whole;  // smaller than the map: less to copy, more LDS left
  w.lds = head + (reach_window ? bytes : whole);
  if (w.lds > budget) return w;
  w.ok = true;
  w.per_problem_origins = reach_window && h.inst_set;
  w.r0 = reach_window ? (int)r0 : 0; w.c0 = reach_window ? (int)c0 : 0;  // (a batch: 0, the origins are per problem)
  w.rows = reach_window ? (int)wr : h.rows; w.cols = reach_window ? (int)wc : h.pitch16;
  return w;
}

// a batched handle: where the window of the problem that starts at (x0, y0) begins
inline void window_origin(const MapHeld& h, const WindowPlan& w, float x0, float y0, int* r0, int* c0) {
  *r0 = *c0 = 0;
  if (!w.per_problem_origins) return;
  *r0 = (int)std::min(std::max(0L, map_cell(y0, h.ylo, h.res) - w.reach), (long)h.rows - w.rows);
  *c0 = (int)std::min(std::max(0L, map_cell(x0, h.xlo, h.res) - w.reach) / 8 * 8, (long)h.pitch16 - w.cols);
}

// ---- the choice ----------------------------------------------------------------------------------------------------
// Decided per launch from measurements (profiles/r06_families.md; history: r01_ablation.md, r02_stamps.md, r03_scan_notes.md):
//   every tile of 32 rollouts a CU, T <= 104    k_rollout_scan_exact / k_rollout_scan (time-parallel)
//   one or two tiles of 64 per CU               k_rollout_pipe   (exact three-wave schedule)
//   beyond (throughput regime)                  k_rollout_fused  (one wave per tile, 4..16 per CU)
//   no LDS window / no incremental trig         k_rollout_map    (general)
// (Rounds 2-5 had two speculative pipelines between the first two, k_rollout_deep and k_rollout_spec; re-measured at the
//  end of round 6 against the exact pipeline and the throughput kernel on one box neither won by 5 % anywhere it was still
//  selected -- k_rollout_spec lost by a factor of two at T = 200 -- and both were removed: profiles/r06_families.md.)
enum MapFamily { kMapScan = 0, kMapScanExact = 1, kMapPipe = 2, kMapFused = 3, kMapGeneral = 4 };

// k_rollout_scan / k_rollout_scan_exact: the launch geometry
struct ScanPlan {
  int waves = 0, chunk_waves = 0;  // waves per workgroup: one per 8 steps (+ the three walkers of the exact kernel); ... of which work on 8 steps each
  int tile = 32;                   // rollouts per workgroup: 32 (two lanes per rollout) or 64
  size_t lds = 0;
  bool pow2res = false;
  bool exact = false;  // k_rollout_scan_exact: the three running sums walked with the reference's roundings
  // k_rollout_scan_exact on a map the planner has stopped speculating on (round 5): every tile runs the exact
  // three-wave schedule at once (ScanFallback::direct) -- noise, folded update and tile packets as ever, so the
  // iteration stays one launch and the kernel family does not depend on the map
  bool direct = false;
  bool speed = false;   // the speed-map form (32-bit cells; exact arithmetic only, no exact schedule inside)
  bool rot_ok = false;  // the exact schedule's state role may rotate (cos, sin) by the exact heading increment
  // where the exact schedule's controls | window | ring live -- a failed tile's, or every tile's (direct) -- and, direct,
  // the small arrays; offset < 0: no room, a failed tile is rolled out step by step by one wave
  int fallback_offset = -1, fallback_map_bytes = 0, small_offset = 0;
};

// A choice: the family, the window, and every number the launch and the last_rollout text need.
struct MapChoice {
  MapFamily family = kMapGeneral;
  WindowPlan window;
  ScanPlan scan;  // the scan families
  // the other three: waves per workgroup (pipe: three per triple), threads, workgroups (fused and general: from N), LDS
  int waves = 1, block = 64, grid = 0;
  size_t lds = 0;
  bool pow2res = false;  // (pipe: ... and no rollout can leave the map, map_unclamped_ok)
  // pipe: wave triples per workgroup, steps per chunk (8, 6, 4, 2), the window's bytes, the control-cost products in LDS
  // (else in a global scratch array)
  int triples = 0, chunk = 0, map_bytes = 0;
  bool cc_lds = false;
  // fused: workgroups of at most four waves (nobody hides a wave's trips to memory: LONE); MPPI_MATH_FAST: one pass over
  // the noise, the control cost added once; the speed-map form; the noise of the first steps kept in LDS for the second pass
  bool lone = false, one_pass = false, speed = false;
  int stash_steps = 0, stash_offset = 0;
  // general: k_rollout_map on the LDS window (deterministic dynamics only), else on the global cells
  bool windowed = false;
};

// ---- k_rollout_scan (rollout_scan_kernel.h): the time-parallel rollout of MPPI_MATH_FAST, and k_rollout_scan_exact ----
// Eligible: 16-bit cells (the reference's own maps always are), a horizon of at most 16 waves of 8 steps, LDS for the
// per-step records, and a map the speculation pays on.
inline bool map_scan(const MapHeld& h, const WindowPlan& w, ScanPlan* out) {
  using L = mppi::ScanExactLds;
  if (h.debug_flags & MPPI_DEBUG_NO_SCAN_KERNEL) return false;
  // (round 6) the speed-map mode too: its dynamics run on nominal traction -- the walks' assumption by construction --
  // and the risk byte comes with the (32-bit) cell; exact arithmetic only, no direct form (rollout_scan_exact_kernel.h)
  const bool speed = h.mode == MPPI_MODE_SPEED_MAP;
  const bool exact = h.math == MPPI_MATH_EXACT;
  if (h.mode != MPPI_MODE_DET && !speed) return false;
  if (!h.cells16_valid || (h.cells16_with_risk != 0) != speed) return false;
  if (speed && !exact) return false;
  // (MPPI_DEBUG_NO_SPECULATION: "the speculative kernels on their exact schedule from the first step" -- for this kernel
  //  that is the direct launch, whatever the map has shown so far: how the tests reach it on any map)
  const bool stopped = h.speculation_off && !(h.debug_flags & MPPI_DEBUG_KEEP_SPECULATING);
  if (stopped && !exact) return false;  // (the tolerance kernel has no exact schedule inside)
  const bool direct = (stopped || (h.debug_flags & MPPI_DEBUG_NO_SPECULATION)) && exact;
  if (direct && ((h.debug_flags & MPPI_DEBUG_NO_SCAN_DIRECT) || !h.grid_packed || speed)) return false;
  ScanPlan plan;
  plan.direct = direct; plan.exact = exact; plan.speed = speed;
  plan.chunk_waves = map_ceil_div(h.T, 8);
  if (plan.exact && plan.chunk_waves > L::kMaxChunkWaves) return false;  // (T <= 104; beyond, k_rollout_pipe)
  plan.waves = plan.exact ? L::waves(plan.chunk_waves) : plan.chunk_waves;
  if (plan.waves > 16) return false;
  plan.tile = (!plan.exact && (h.debug_flags & MPPI_DEBUG_SCAN_FULL_TILES)) ? 64 : 32;
  // one round of workgroups over the CUs: beyond that the kernels with one wave per tile win (a
  // 32-rollout workgroup lasts ~10 us whatever N is: N = 16384 would be two rounds against 18 us
  // of k_rollout_pipe, N = 65536 eight against 78 us of k_rollout_fused)
  if (map_ceil_div(h.n_local, plan.tile) > h.num_cus) return false;
  plan.lds = plan.exact ? L::total(plan.chunk_waves)
                        : (plan.tile == 64 ? mppi::ScanLds<64>::total(plan.waves) : mppi::ScanLds<32>::total(plan.waves));
  // (the accumulating wave reads up to two groups of records past the last one: keep that inside the allocation)
  plan.lds = std::max(plan.lds, (size_t)40 * 1024);
  const size_t budget = (size_t)h.lds_per_cu - 1024;
  if (plan.lds > budget) return false;
  // (the template flag also selects the unclamped address of the exact schedule inside the kernel -- direct launches
  //  and re-executed tiles: only where no rollout can leave the map; the speed-map form has no exact schedule inside:
  //  its lookups all clamp)
  plan.pow2res = map_res_pow2(h) && (speed || (h.grid_packed && map_unclamped_ok(h)));
  plan.rot_ok = map_rotation_ok(h);
  // The exact schedule inside the kernel needs its controls, the 16-bit window of the cells reachable within the horizon
  // and one chunk ring in LDS.  A direct launch runs every tile on it: noise | control-cost terms | {controls, window,
  // ring} | small arrays (the walks' groups and positions do not exist); no window: k_rollout_pipe / the general kernels.
  // Else it re-executes a tile whose vote fails (rollout_scan_exact_kernel.h, scan_exact_reexecute): in the LDS of the
  // walks' groups and positions, dead by then -- or behind everything when the horizon is too short for that region to
  // hold them -- or not at all (offset stays < 0: one wave rolls such a tile out step by step).
  if (plan.direct && !w.ok) return false;
  if (plan.exact && !speed && w.ok) {
    const int W = plan.chunk_waves;
    const size_t map_bytes = (size_t)w.rows * (size_t)w.cols * 2, need = mppi::ScanFallbackLds::bytes(8 * W, (int)map_bytes);
    const size_t total = (L::total(W) + 15) & ~(size_t)15;
    const bool inside = plan.direct || need <= L::grp(W) + L::p2(W);
    if (inside || total + need <= budget) {
      plan.fallback_offset = inside ? (int)(L::e2(W) + L::ccr(W)) : (int)total;
      plan.fallback_map_bytes = (int)map_bytes;
    }
    if (plan.direct) {
      plan.small_offset = plan.fallback_offset + (int)((need + 15) & ~(size_t)15);
      plan.lds = std::max((size_t)plan.small_offset + L::small(W), (size_t)40 * 1024);
      if (plan.lds > budget) return false;
    } else if (!inside && plan.fallback_offset >= 0) {
      plan.lds = std::max(plan.lds, total + need);
    }
  }
  *out = plan;
  return true;
}

// ---- k_rollout_pipe: the map window in LDS + the incremental trig ---------------------------------------------------
inline bool map_pipe(const MapHeld& h, const WindowPlan& w, MapChoice* c) {
  const int N = h.n_local, T = h.T, tiles = map_ceil_div(N, 64);
  const size_t lds_win = w.lds, budget = (size_t)h.lds_per_cu - 1024;
  int pairs = map_ceil_div(tiles, h.num_cus);  // wave triples per workgroup
  if (pairs < 1) pairs = 1;
  if (pairs > mppi::kPipeMaxTriples) pairs = mppi::kPipeMaxTriples + 1;  // (beyond the kernel's launch bounds: the throughput kernel's)
  // batched handle: the triples of a workgroup share one problem's window and controls
  auto divisor = [&]() { if (h.inst_set) while (h.inst_tiles % pairs != 0) --pairs; };
  divisor();
  auto ring_bytes = [&](int chunk) { return (size_t)pairs * (size_t)mppi::pipe_ring_bytes(chunk); };
  int chunk = 0;
  for (;;) {  // fewer triples per workgroup (more workgroups than CUs) before giving the kernel up
    // (6: the whole-map window of the long horizons -- 135 KiB at T = 200 -- leaves room for chunks of six steps but
    //  not of eight; every chunk costs ~340 cycles beside its steps, so six instead of four is 28 cycles per step)
    for (int cnd : {8, 6, 4, 2})
      if (lds_win + ring_bytes(cnd) <= budget) { chunk = cnd; break; }
    if (chunk > 0 || pairs == 1) break;
    --pairs;
    divisor();
  }
  // The pipelined kernel is the low-latency choice: it wins while one workgroup per CU covers the problem with one
  // wave triple, and with two when chunks of four steps at least fit beside the window (measured at the end of round 6,
  // N x T, us per iteration pipe | fused: 8192 x 200 44 | 79; 16384 x 100 39 | 53; 16384 x 200 63 | 85;
  // 32768 x 100 55 | 60; 32768 x 200 (chunks of two) 102 | 77; 49152 x 100 (three triples) 74 | 48:
  // profiles/r06_families.md).  Beyond that the fused kernel, 4..16 waves per CU, has the better throughput.
  const bool latency_regime = pairs <= mppi::kPipeMaxTriples && (pairs == 1 || chunk >= 4) && map_ceil_div(tiles, pairs) <= h.num_cus;
  if (chunk == 0 || !latency_regime) return false;
  c->triples = pairs;
  c->chunk = chunk;
  c->pow2res = map_res_pow2(h) && map_unclamped_ok(h);
  // control-cost products in LDS when there is room, else in a global scratch array
  const size_t cc_bytes = (size_t)pairs * T * 64 * sizeof(double);
  c->cc_lds = lds_win + ring_bytes(chunk) + cc_bytes <= budget && !(h.debug_flags & MPPI_DEBUG_CC_GLOBAL);
  c->lds = lds_win + ring_bytes(chunk) + (c->cc_lds ? cc_bytes : 0);
  c->map_bytes = (int)(lds_win - map_lds_head(T));
  c->waves = 3 * pairs;
  c->block = 192 * pairs;
  c->grid = map_ceil_div(N, 64 * pairs);
  return true;
}

// Waves (tiles of 64 rollouts) per workgroup of the one-wave-per-tile kernels that keep the map
// window in LDS.  The window makes it one workgroup per CU, so the workgroup is sized to cover
// the problem in one round: at least 4 waves (one per SIMD, and enough lanes to copy the
// window), at most 16.  Batched handle: a workgroup stays inside one problem, i.e. the count
// divides the tiles per problem -- among the divisors the one with the fewest rounds, then the
// smallest (1536 tiles: 8 waves in 1 round, not 4 waves in 2; measured 130 -> 105 us).
inline int fused_waves_per_workgroup(const MapHeld& h) {
  const int tiles = map_ceil_div(h.n_local, 64);
  int waves = map_ceil_div(tiles, h.num_cus);
  waves = waves < 4 ? 4 : (waves > 16 ? 16 : waves);
  if (!h.inst_set) return waves;
  int best = 0, best_rounds = 1 << 30;
  for (int lowest : {4, 1}) {  // (at least four where a divisor allows it)
    if (best) break;
    for (int d = lowest; d <= 16; ++d) {
      if (h.inst_tiles % d != 0) continue;
      const int rounds = map_ceil_div(map_ceil_div(tiles, d), h.num_cus);
      if (rounds < best_rounds) { best = d; best_rounds = rounds; }  // ascending: ties keep the smallest
    }
  }
  return best;
}

// ---- k_rollout_fused: one wave per tile on the LDS window, (cos, sin) by rotation ------------------------------------
inline void map_fused(const MapHeld& h, const WindowPlan& w, MapChoice* c) {
  const bool exact = h.math == MPPI_MATH_EXACT;
  c->speed = h.mode == MPPI_MODE_SPEED_MAP;
  c->one_pass = !exact;
  c->lone = exact && !c->speed && c->waves <= 4;
  // Round 6 (exact mode reads the noise twice): what the window leaves of the CU's LDS keeps the noise of the first
  // steps for the second pass -- one workgroup per CU either way (DevParams::stash_steps; N = 65536, T = 100: 56 of
  // the 100 steps of each of the four waves); in multiples of 8 steps
  const size_t off = (w.lds + 15) & ~(size_t)15, limit = (size_t)h.lds_per_cu - 1024, per_step = (size_t)c->waves * 64 * 8;
  const int steps = limit > off ? std::min((int)((limit - off) / per_step), h.T) & ~7 : 0;
  if (exact && !c->speed && steps >= 8) {
    c->stash_steps = steps;
    c->stash_offset = (int)off;
    c->lds = off + per_step * (size_t)steps;
  }
}

// The state must hold a map mode (deterministic dynamics or speed map).
inline MapChoice map_choose(const MapHeld& h) {
  MapChoice c;
  c.window = map_window(h);
  const WindowPlan& w = c.window;
  const bool speed = h.mode == MPPI_MODE_SPEED_MAP, exact = h.math == MPPI_MATH_EXACT;
  const bool rot = h.theta_bounded && map_rotation_ok(h);
  if (map_scan(h, w, &c.scan)) {
    c.family = c.scan.exact ? kMapScanExact : kMapScan;
  } else if (w.ok && rot && exact && !speed && map_pipe(h, w, &c)) {
    c.family = kMapPipe;
  } else {  // one wave per tile of 64; on the window one workgroup per CU: at most one round of workgroups over the CUs
    c.family = w.ok && rot ? kMapFused : kMapGeneral;
    c.windowed = w.ok && (rot || !speed);
    c.waves = c.windowed ? fused_waves_per_workgroup(h) : 1;
    c.block = 64 * c.waves;
    c.grid = map_ceil_div(h.n_local, c.block);
    c.lds = c.windowed ? w.lds : map_lds_head(h.T);
    c.pow2res = map_res_pow2(h);
    if (c.family == kMapFused) map_fused(h, w, &c);
  }
  return c;
}
