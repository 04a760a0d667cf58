// guide_kernels.h -- the guide round the walls (mppi_planner_set_guide): a shortest-path distance field from every problem's
// goal over a grid whose cells the shared static walls block, and per time step a "carrot", the point on the shortest path
// from the robot's cell that is lead + j * pace ahead.  The rollouts meet the carrots as they meet a goal track (GoalRows,
// relative = 1: step t reads row t + 1 whatever the track offset is).  The arithmetic is guide_grid.h's; the bits are pinned
// by tests/guide_model.py.  While an occupancy grid is held as well (mppi_planner_set_occupancy), its cells block too:
// GuideOccupancy, below; tests/occupancy_model.py has that mask.
//
// Two plain launches on the planner's stream, at the head of a call that starts iterations, behind the fleet's refresh: no
// flags, no atomics, no waits between workgroups, every loop bounded and every index clamped.
//
// k_guide_field: one workgroup of 1024 threads per problem, only when the guide, the static walls or a goal changed.  The
// field lives in LDS, uint32 [ny][nx] (147456 bytes at the cap of 192 x 192).  Prologue: the walls' constants are staged 64
// at a time and every thread tests its cells' centres against the tile.  Then relaxation in place until a whole sweep
// changes no cell (__syncthreads_or): every stored value is the length of a real path and values only fall, so the least
// fixed point is reached in any order -- the integers make the order invisible.  A thread walks a run of consecutive cells,
// along a row upwards and downwards in sweeps 0 and 1 of four and along a column in sweeps 2 and 3, so a sweep carries a
// distance along a whole run of a corridor in its direction and not one cell; the loop is bounded at nx * ny sweeps, the
// longest path there is.  Epilogue: the field goes to memory with, per cell, the move a descent takes from it (guide_next;
// kGuideNoMove without one) -- the byte table k_guide_rows chases.
//
// k_guide_rows: one workgroup of 256 threads per problem, at every refresh.  The descent is a dependent chain -- the move
// of a cell names the next cell -- of up to (lead + T * pace) / res cells on a lone lane, about an LDS load's latency a
// cell (~9 cycles per dependent instruction on a lone wave, and the load on top).  So what the chain
// reads is kept close and small: the problem's move table, a byte a cell (36 KiB at the cap, where the field would be 144),
// is pulled into LDS first, and the remaining length is carried by subtraction (D[c] = D[n] + w along a descent), never
// loaded.  Thread 0 walks kGuideStretch cells at a time into LDS, then all threads pick their rows from the stretch
// (guide_first_reach): row j is the first cell that is lead_u + j * pace_u nearer to the goal than the start.
#pragma once
#include "guide_grid.h"
#include "occupancy_grid.h"
#include "rollout_kernels.h"

namespace mppi {

// The grid as the kernels take it, and the row choice's units (guide_units, formed on the host).
struct GuideGrid {
  float x_min, y_min, res, inflate;
  int nx, ny;
  int lead_u, pace_u;
};

// The occupancy grid as k_guide_field takes it (mppi_planner_set_occupancy; field nullptr: none held): a guide cell whose
// centre lies inside the grid on a cell with D2 <= thr is blocked -- thr: occupancy_threshold with R = inflate_occ +
// inflate_guide, formed on the host.  The two grids need not coincide.
struct GuideOccupancy {
  const uint32_t* field;
  float x_min, y_min, res;
  int nx, ny;
  uint32_t thr;
};

constexpr int kGuideFieldThreads = 1024;
constexpr size_t kGuideFieldStaticLds = 4096;  // an upper bound of k_guide_field's static LDS (the wall tile: 3072 bytes, and the barrier's word)
constexpr int kGuideRowsThreads = 256;
constexpr int kGuideStretch = 256;  // cells of the descent thread 0 walks between two row choices

// dynamic LDS: [ny * nx] uint32, the field.  seg / hw: the shared static walls (one row: [wall]).  field, moves: [B][ny * nx]
__global__ __launch_bounds__(kGuideFieldThreads) void k_guide_field(DevParams P, GuideGrid g, const float4* __restrict__ seg,
                                                                    const float* __restrict__ hw, int n_walls,
                                                                    uint32_t* __restrict__ field, uint8_t* __restrict__ moves,
                                                                    GuideOccupancy occ) {
  extern __shared__ uint32_t guide_field_lds[];
  __shared__ GuideWall tile[64];
  static_assert(sizeof(tile) + 512 <= kGuideFieldStaticLds, "kGuideFieldStaticLds: what the host adds to the dynamic size");
  uint32_t* D = guide_field_lds;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int nx = g.nx, ny = g.ny, cells = nx * ny;
  if (P.inst != nullptr) {  // (a batched launch: the problem's own goal)
    const BatchInst I = P.inst[b];
    P.xg = I.xg;
    P.yg = I.yg;
  }
  // this thread's run of consecutive cells [c_lo, c_hi)
  const int per = (cells + kGuideFieldThreads - 1) / kGuideFieldThreads;
  const int c_lo = min(tid * per, cells), c_hi = min(c_lo + per, cells);
  for (int c = c_lo; c < c_hi; ++c) D[c] = kGuideUnreached;
  for (int k0 = 0; k0 < n_walls; k0 += 64) {
    __syncthreads();  // (the tile's last readers have left)
    if (tid < 64 && k0 + tid < n_walls) {
      const float4 sg = seg[k0 + tid];
      tile[tid] = guide_wall(sg.x, sg.y, sg.z, sg.w, hw[k0 + tid], g.inflate);
    }
    __syncthreads();
    const int nk = min(64, n_walls - k0);
    for (int c = c_lo; c < c_hi; ++c) {
      if (D[c] == kGuideBlocked) continue;
      const int iy = c / nx, ix = c - iy * nx;
      const double cx = guide_centre(g.x_min, g.res, ix), cy = guide_centre(g.y_min, g.res, iy);
      bool hit = false;
      for (int k = 0; k < nk && !hit; ++k) hit = guide_blocked(cx, cy, tile[k]);
      if (hit) D[c] = kGuideBlocked;
    }
  }
  if (occ.field != nullptr) {  // (uniform; a thread's own cells: no barrier needed)
    for (int c = c_lo; c < c_hi; ++c) {
      const int iy = c / nx, ix = c - iy * nx;
      int ox = 0, oy = 0;
      if (occupancy_cell(guide_centre(g.x_min, g.res, ix), occ.x_min, occ.res, occ.nx, &ox) &&
          occupancy_cell(guide_centre(g.y_min, g.res, iy), occ.y_min, occ.res, occ.ny, &oy) &&
          occ.field[(size_t)oy * (size_t)occ.nx + (size_t)ox] <= occ.thr)
        D[c] = kGuideBlocked;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int gc = guide_cell_of(P.yg, g.y_min, g.res, ny) * nx + guide_cell_of(P.xg, g.x_min, g.res, nx);
    if (D[gc] != kGuideBlocked) D[gc] = 0u;
  }
  __syncthreads();
  for (int sweep = 0; sweep < cells; ++sweep) {
    int changed = 0;
    const bool down = (sweep & 1) != 0, columns = (sweep & 2) != 0;
    for (int i = 0; i < c_hi - c_lo; ++i) {
      const int r = down ? c_hi - 1 - i : c_lo + i;  // the cell's place in this sweep's order: along the rows, or the columns
      int ix, iy;
      if (columns) {
        ix = r / ny;
        iy = r - ix * ny;
      } else {
        iy = r / nx;
        ix = r - iy * nx;
      }
      const int c = iy * nx + ix;
      const uint32_t now = D[c];
      if (now == kGuideBlocked) continue;
      uint32_t best;
      (void)guide_next(D, nx, ny, ix, iy, &best);
      if (best < now) {
        D[c] = best;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  field += (size_t)b * (size_t)cells;
  moves += (size_t)b * (size_t)cells;
  for (int c = c_lo; c < c_hi; ++c) {
    const int iy = c / nx, ix = c - iy * nx;
    uint32_t best;
    moves[c] = (uint8_t)guide_next(D, nx, ny, ix, iy, &best);
    field[c] = D[c];
  }
}

// dynamic LDS: [ny * nx] bytes, the problem's move table.  done: closed_loop's per-problem flags (a parked problem's rows are
// the goal), or nullptr.  rows: [B][T + 1]; status: [B].
__global__ __launch_bounds__(kGuideRowsThreads) void k_guide_rows(DevParams P, GuideGrid g, const uint32_t* __restrict__ field,
                                                                  const uint8_t* __restrict__ moves, const int* __restrict__ done,
                                                                  float2* __restrict__ rows, int* __restrict__ status) {
  extern __shared__ uint8_t guide_moves_lds[];
  __shared__ uint32_t left[kGuideStretch];   // R_i of the stretch
  __shared__ uint16_t where[kGuideStretch];  // c_i of the stretch (a cell index is below kGuideCellsMax < 65536)
  __shared__ int stretch_len, stretch_last;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, T = P.n_steps;
  const int nx = g.nx, ny = g.ny, cells = nx * ny;
  if (P.inst != nullptr) {  // (a batched launch: the problem's own start and goal)
    const BatchInst I = P.inst[b];
    P.x0 = I.x0; P.y0 = I.y0;
    P.xg = I.xg; P.yg = I.yg;
  }
  field += (size_t)b * (size_t)cells;
  moves += (size_t)b * (size_t)cells;
  rows += (size_t)b * (size_t)(T + 1);
  const float2 goal = make_float2(P.xg, P.yg);
  for (int j = tid; j <= T; j += kGuideRowsThreads) rows[j] = goal;  // (every row this launch does not pick is the goal)
  // the verdicts every thread reaches alike, from two or three uniform loads
  const int gc = guide_cell_of(P.yg, g.y_min, g.res, ny) * nx + guide_cell_of(P.xg, g.x_min, g.res, nx);
  const int c0 = guide_cell_of(P.y0, g.y_min, g.res, ny) * nx + guide_cell_of(P.x0, g.x_min, g.res, nx);
  int verdict = kGuideStatusOk;
  uint32_t R0 = 0u;
  if (field[gc] == kGuideBlocked) {
    verdict = kGuideStatusGoalBlocked;
  } else if (done == nullptr || done[b] == 0) {
    R0 = field[c0];
    if (R0 >= kGuideUnreached) {  // inside the inflated band, or a pocket: out by the cheapest way, if there is one
      const int k = moves[c0];
      if (k >= 8) {
        verdict = kGuideStatusNoWayOut;
      } else {
        const int c1 = min(max(c0 + guide_dy(k) * nx + guide_dx(k), 0), cells - 1);
        R0 = field[c1] + guide_move_cost(k);
      }
    }
  }
  if (tid == 0) status[b] = verdict;
  if (verdict != kGuideStatusOk || (done != nullptr && done[b] != 0)) return;  // (uniform over the workgroup)
  for (int c = tid; c < cells; c += kGuideRowsThreads) guide_moves_lds[c] = moves[c];
  const long long reach = (long long)g.lead_u + (long long)T * (long long)g.pace_u;
  // thread 0's place on the descent
  int cell = c0, steps = 0;
  uint32_t R = R0;
  long long gain_before = -1;  // R_0 - R of the last cell of the stretch before: rows up to that gain are picked
  for (int stretch = 0; stretch <= cells / kGuideStretch + 1; ++stretch) {
    __syncthreads();  // (the table is staged; the last stretch's readers have left)
    if (tid == 0) {
      int n = 0, last = 0;
      while (n < kGuideStretch) {
        left[n] = R;
        where[n] = (uint16_t)cell;
        ++n;
        if (R == 0u || (long long)(R0 - R) >= reach || steps >= cells) { last = 1; break; }
        const int k = guide_moves_lds[cell];
        if (k >= 8) { last = 1; break; }
        cell = min(max(cell + guide_dy(k) * nx + guide_dx(k), 0), cells - 1);
        R = R >= guide_move_cost(k) ? R - guide_move_cost(k) : 0u;
        ++steps;
      }
      stretch_len = n;
      stretch_last = last;
    }
    __syncthreads();
    const int n = stretch_len;
    const long long gain_here = (long long)(R0 - left[n - 1]);
    for (int j = tid; j <= T; j += kGuideRowsThreads) {
      const long long a = (long long)g.lead_u + (long long)j * (long long)g.pace_u;
      if (a <= gain_before || a > gain_here) continue;  // picked in a stretch before, or further on
      const int i = min(guide_first_reach(left, n, R0, a), n - 1);
      if (left[i] != 0u) {
        const int c = where[i], iy = c / nx, ix = c - iy * nx;
        rows[j] = make_float2((float)guide_centre(g.x_min, g.res, ix), (float)guide_centre(g.y_min, g.res, iy));
      }
    }
    gain_before = gain_here;
    if (stretch_last) break;  // (uniform: read behind the barrier)
  }
}

}  // namespace mppi
