// cvar_plan.h -- the CVaR mode's launches and how sampled traction becomes the cell words the rollouts gather, as pure
// functions of what the handles hold: which CVaR rollout kernel runs (cvar_choose), the geometry of the sharded reduction
// (cvar_reduce_choose), the route from the TDMs to the cell words (cells_choose) and the geometry of a TDM's sampling
// kernel (sample_choose).  Plain C++ without a HIP type: a host program compiles it on its own (tests/test_cvar_plan.py
// pins the tables).  cvar_held(p) and cells_held(p, ...) (launch_plan.h) fill the states from the handles; the launchers
// there and in mppi_api.hip carry a choice out and keep every side effect.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>

#include "map_plan.h"
#include "noise_plan.h"

inline int cvar_pow2(int v) {  // the next power of two (host_common.h: next_pow2)
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// ---- which CVaR rollout kernel runs ----------------------------------------------------------------------------------
// What the choice depends on, and nothing else: no pointer.  cvar_held() zeroes it first.  map: what map_rotation_ok and
// map_res_pow2 read -- and math, T, n_local and theta_bounded, which are read from there too.
struct CvarHeld {
  MapHeld map;
  int num_grid_samples;   // M, this rank's
  int m_count;            // ranks the samples are sharded over (1: not sharded)
  int want_sample_costs;
  int pad_;
};
static_assert(sizeof(CvarHeld) == sizeof(MapHeld) + 4 * sizeof(int), "CvarHeld has padding nobody zeroes by name");

constexpr size_t kCvarLdsPlain = 64 * 1024;   // beyond: the launch needs the dynamic-LDS attribute; the fast kernel's limit
constexpr size_t kCvarLdsMax = 160 * 1024;    // beyond: refused

// LDS in bytes: [T] double2 control ratios (fast: + [T] double) | [next_pow2(M)] float costs of the samples
inline size_t cvar_lds_general(int T, int mp2) { return 16 * (size_t)T + 4 * (size_t)mp2; }
inline size_t cvar_lds_fast(int T, int mp2) { return 24 * (size_t)T + 4 * (size_t)mp2; }

// where the per-sample costs go: nowhere, the handle's sample_costs, or -- samples sharded over ranks -- this rank's slab
// of the gather buffer (whether they are wanted or not: the reduction reads them)
enum CvarCosts { kCvarCostsNone = 0, kCvarCostsSampleCosts = 1, kCvarCostsSlab = 2 };

struct CvarChoice {
  int refused = 0;            // the general kernel's LDS exceeds 160 KiB (lds: that size, for the refusal's text)
  int launch = kLaunchCvar;   // kLaunchCvarFast | kLaunchCvar: what noise_plan.h is told of the coming launch
  int fast = 0;               // k_rollout_tdm_fast: (cos, sin) by rotation; else k_rollout_tdm
  int cost_f32 = 0;           // fast kernel, MPPI_MATH_FAST: the <cost f32> form
  int exact = 0;              // general kernel: the template flag its text names
  int pow2res = 0;            // fast kernel only
  int threads = 0, mp2 = 0, workgroups = 0;
  size_t lds = 0;             // of the kernel that runs
  int set_attribute = 0;      // ... and it needs hipFuncAttributeMaxDynamicSharedMemorySize (the general kernel only)
  int costs_to = kCvarCostsNone;
};

inline CvarChoice cvar_choose(const CvarHeld& h) {
  CvarChoice c;
  const int T = h.map.T, M = h.num_grid_samples;
  const bool exact = h.map.math == MPPI_MATH_EXACT;
  c.mp2 = cvar_pow2(M);
  c.threads = noise_cvar_threads(M);
  c.workgroups = h.map.n_local;
  c.exact = exact;
  // (the 160 KiB check is made on the general kernel's size, before anything else, whichever kernel would run: the fast
  //  kernel's LDS is the larger of the two, so it never runs where this refuses)
  c.lds = cvar_lds_general(T, c.mp2);
  if (c.lds > kCvarLdsMax) {
    c.refused = 1;
    return c;
  }
  c.costs_to = h.m_count > 1 ? kCvarCostsSlab : (h.want_sample_costs ? kCvarCostsSampleCosts : kCvarCostsNone);
  // the fast kernel: |theta| bounded over the horizon, the heading increment within the rotation's proof, LDS within 64 KiB
  c.fast = h.map.theta_bounded && map_rotation_ok(h.map) && cvar_lds_fast(T, c.mp2) <= kCvarLdsPlain;
  if (c.fast) {
    c.launch = kLaunchCvarFast;
    c.lds = cvar_lds_fast(T, c.mp2);
    c.cost_f32 = !exact;
    c.pow2res = map_res_pow2(h.map);
  } else {
    // (kept as it is: the general kernel never takes pow2res -- its text names exact= only)
    c.set_attribute = c.lds > kCvarLdsPlain;
  }
  return c;
}

// ---- samples sharded over GPUs: every rank reduces all N control samples over all M costs (k_cvar_reduce) -------------
inline int cvar_numel(int m_total, float cvar_alpha) {  // mppi.py:716-717 over m_total samples
  const int numel = (int)std::ceil((double)m_total * (double)cvar_alpha);
  return numel < 1 ? 1 : (numel > m_total ? m_total : numel);
}

struct CvarReduceChoice {
  int refused = 0;  // too many samples over all shards for the reduction's 64 KiB of LDS
  int m_total = 0, mp2 = 0, threads = 0, numel = 0;
  size_t lds = 0;
};

inline CvarReduceChoice cvar_reduce_choose(int num_grid_samples, int m_count, float cvar_alpha) {
  CvarReduceChoice c;
  c.m_total = num_grid_samples * m_count;
  c.mp2 = cvar_pow2(c.m_total);
  c.threads = c.mp2 > 1024 ? 1024 : (c.mp2 < 64 ? 64 : c.mp2);  // one element per thread when it fits
  c.lds = 4 * (size_t)c.mp2;
  c.refused = c.lds > kCvarLdsPlain;
  c.numel = cvar_numel(c.m_total, cvar_alpha);
  return c;
}

// ---- the template ladder of the Philox samplers: the bins a thread keeps in registers, 8 | 16 | 32 | 64 ----------------
// (for at most 64 bins; the callers send more elsewhere)
inline int bins_form(int bins) { return bins <= 8 ? 0 : (bins <= 16 ? 1 : (bins <= 32 ? 2 : 3)); }

// ---- from the TDMs to the cell words ------------------------------------------------------------------------------------
// What the route depends on, and nothing else: no pointer.  cells_held() zeroes it first.
struct CellsHeld {
  int mode, M;
  int for_solve;     // asked by solve()'s sampling step (sample_for_solve): only there may the draws go straight into the cells
  int same_tdm;      // lin == ang
  int lin_rng, ang_rng, lin_bins, ang_bins;
  int alpha_positive;  // alpha_dyn > 0
  int lin_first_sample, ang_first_sample;
  int rows, cols;
  int lin_compact_ok, ang_compact_ok;
  int lin_injected, ang_injected, lin_injected_nonneg, ang_injected_nonneg;  // injected_min >= 0
  int has_risk;      // lin's
  int packed_match;  // the cell words were packed from these generations of both TDMs
};
static_assert(sizeof(CellsHeld) == 21 * sizeof(int), "CellsHeld has padding nobody zeroes by name");

enum CellsRoute { kCellsNothing = 0, kCellsSample = 1, kCellsPackSingle = 2, kCellsPackMulti = 3 };
enum CellsMirror { kMirrorNone = 0, kMirror16 = 1, kMirror32Risk = 2 };

struct CellsChoice {
  int route = kCellsNothing;
  unsigned grid_x = 0, grid_y = 1;  // of the route's kernel (256 threads)
  // sample: the bins form and the cell groups (4 cells each) the Philox counters are laid over
  int bins = 0;
  long cell_groups = 0;
  // pack single: the mirror the LDS windows are copied from -- 16-bit cells, or (speed-map mode) 32-bit cells with the risk
  // byte in the same buffer; its pitch, the 16-bit units it needs and its kernel's grid.  Every other route leaves none:
  // cells16_valid is cleared on every repack.
  int mirror = kMirrorNone;
  int pitch16 = 0;
  size_t mirror_units = 0;
  unsigned mirror_grid = 0;
};

inline CellsChoice cells_choose(const CellsHeld& h) {
  CellsChoice c;
  if (h.mode == MPPI_MODE_BAREBONE) return c;
  // solve() of a CVaR planner, Philox generators: both TDMs sampled straight into the cell words the rollout gathers
  // (k_sample_cellsM_philox), no (G, R, C) int8 grids and no transpose.
  // (Kept as they are: a lin TDM passed as ang too falls back to sample + pack; and a one-hot TDM whose unchanged maps the
  //  ordinary sampling step would skip is sampled again here -- one_hot is not among the inputs.)
  bool into_cells = h.for_solve && h.mode == MPPI_MODE_TDM && !h.same_tdm && h.lin_rng == MPPI_RNG_PHILOX &&
                    h.ang_rng == MPPI_RNG_PHILOX && h.lin_bins <= 64 && h.ang_bins <= 64 && h.alpha_positive &&
                    h.lin_first_sample == h.ang_first_sample;
  // a wave of this kernel sets up the thresholds of its 4 cells for M/64 rounds of draws: measured
  // against sample + sample + transpose, 65 vs 61 us at M = 128 and 192 vs 363 us at M = 1024
  if (h.M < 192) into_cells = false;
  if (into_cells) {
    c.route = kCellsSample;
    c.cell_groups = (long)h.rows * ((h.cols + 3) / 4);
    c.bins = bins_form(std::max(h.lin_bins, h.ang_bins));
    c.grid_x = (unsigned)map_ceil_div(c.cell_groups, 4);
    return c;
  }
  // (solve()'s sampling step is about to sample: whether the cells then need packing is asked again behind it)
  if (h.for_solve || h.packed_match) return c;
  if (h.M != 1) {
    c.route = kCellsPackMulti;
    c.grid_x = (unsigned)(h.rows * map_ceil_div(h.cols, 64));
    c.grid_y = (unsigned)map_ceil_div(h.M, 64);
    return c;
  }
  c.route = kCellsPackSingle;
  c.grid_x = (unsigned)map_ceil_div((long)h.rows * h.cols, 256);
  // every byte of both grids in [0, 127]: the sampler's table, or what was injected
  const bool lin_7bit = h.lin_injected ? h.lin_injected_nonneg : h.lin_compact_ok;
  const bool ang_7bit = h.ang_injected ? h.ang_injected_nonneg : h.ang_compact_ok;
  // (kept as it is: lin's own compact_ok -- its masks are 0/1 -- is asked besides the 7-bit test on both grids)
  if (h.lin_compact_ok && lin_7bit && ang_7bit) {
    c.mirror = h.mode == MPPI_MODE_SPEED_MAP && h.has_risk ? kMirror32Risk : kMirror16;
    c.pitch16 = map_ceil_div(h.cols, 8) * 8;
    c.mirror_units = (size_t)h.rows * c.pitch16 * (c.mirror == kMirror32Risk ? 2 : 1);
    c.mirror_grid = (unsigned)map_ceil_div((long)h.rows * c.pitch16, 256);  // a thread per cell, 16-bit or 32-bit
  }
  return c;
}

// ---- a TDM's sampling kernel: the draws into the (G, R, C) int8 grids --------------------------------------------------
enum SampleKernel { kSampleColumns = 0, kSampleGeneric = 1, kSampleXoroshiro = 2 };

struct SampleChoice {
  int kernel = kSampleColumns;
  unsigned grid_x = 0, grid_y = 1;
  int block = 256;
  long cell_groups = 0;                   // Philox: groups of 4 cells
  int bins = 0, chunks = 0, g_chunk = 0;  // columns: the bins form; the samples split over `chunks` workgroups, g_chunk each
  int threads = 0;                        // xoroshiro: one generator state per thread
};

inline SampleChoice sample_choose(int rng, int bins, int rows, int cols, int G, int thread_dim_x, int thread_dim_y) {
  SampleChoice c;
  if (rng != MPPI_RNG_PHILOX) {
    c.kernel = kSampleXoroshiro;
    c.threads = G * thread_dim_x * thread_dim_y;
    c.block = 64;
    c.grid_x = (unsigned)map_ceil_div(c.threads, 64);
    return c;
  }
  c.cell_groups = (long)rows * ((cols + 3) / 4);
  if (bins > 64) {
    c.kernel = kSampleGeneric;
    c.grid_x = (unsigned)map_ceil_div((long)G * c.cell_groups, 256);
    return c;
  }
  c.bins = bins_form(bins);
  // enough workgroups to fill the chip, as many samples per thread as that allows
  c.chunks = map_ceil_div(256L * 1024, c.cell_groups);
  c.chunks = c.chunks < 1 ? 1 : (c.chunks > G ? G : c.chunks);
  c.g_chunk = (map_ceil_div(G, c.chunks) + 1) & ~1;  // even: a Philox block serves a pair of samples
  c.grid_x = (unsigned)map_ceil_div(c.cell_groups, 256);
  c.grid_y = (unsigned)map_ceil_div(G, c.g_chunk);
  return c;
}
