// launch_plan.h -- the launches of an iteration: packing of the map cells, the rollout kernels of every mode, the
// update / exchange launches, the iteration loop with its hipGraph replay.  What is launched and with what geometry is
// decided by the pure functions of map_plan.h, cvar_plan.h, barebone_plan.h, noise_plan.h and update_plan.h; here are the
// adapters that fill their states from a handle (map_held, cvar_held, cells_held, update_held, noise_held) and the
// launchers that carry a choice out and keep every side effect.  Host code only; the C ABI shims that call into it are in
// mppi_api.hip (which is the only file that includes this one: everything here has internal linkage).
#pragma once
#include "handles.h"
#include "update_plan.h"

static int tdm_max_byte(const mppi_tdm* t) { return t->injected ? (int)t->injected_max : t->table_max; }

// ---- helpers -------------------------------------------------------------------
static int check_tdms(const mppi_planner* p, const mppi_tdm* lin, const mppi_tdm* ang) {
  if (p->cfg.mode == MPPI_MODE_BAREBONE) return MPPI_OK;
  REQUIRE(lin && ang, MPPI_ERR_INVALID, "lin/ang TDM required in this mode");
  REQUIRE(lin->maps_set && ang->maps_set, MPPI_ERR_STATE, "TDM maps not set");
  REQUIRE(lin->cfg.device == p->cfg.device && ang->cfg.device == p->cfg.device, MPPI_ERR_INVALID,
          "planner and TDMs live on different devices");
  REQUIRE(lin->rows == ang->rows && lin->cols == ang->cols, MPPI_ERR_INVALID,
          "lin and ang TDMs differ in padded size (%dx%d vs %dx%d)", lin->rows, lin->cols, ang->rows,
          ang->cols);
  REQUIRE(lin->cfg.num_grids == p->cfg.num_grid_samples && ang->cfg.num_grids == p->cfg.num_grid_samples,
          MPPI_ERR_INVALID, "TDM num_grids (%d, %d) != planner num_grid_samples (%d)", lin->cfg.num_grids,
          ang->cfg.num_grids, p->cfg.num_grid_samples);
  REQUIRE(lin->cfg.max_rows == ang->cfg.max_rows && lin->cfg.max_cols == ang->cfg.max_cols, MPPI_ERR_INVALID,
          "lin and ang TDMs differ in max_map_dim");
  REQUIRE(p->cfg.mode != MPPI_MODE_SPEED_MAP || lin->has_risk, MPPI_ERR_STATE,
          "speed-map mode needs lin TDM's risk traction map");
  return MPPI_OK;
}

// the map fields come from what the cell words were packed from (zeros before that, and in barebone mode)
static DevParams make_dev_params(const mppi_planner* p) {
  const mppi_params& a = p->params;
  const PackedMaps& m = p->packed;
  DevParams d;
  memset(&d, 0, sizeof(d));
  d.x0 = a.x0[0]; d.y0 = a.x0[1]; d.th0 = a.x0[2];
  d.xg = a.xgoal[0]; d.yg = a.xgoal[1];
  d.v_lo = a.vrange[0]; d.v_hi = a.vrange[1];
  d.w_lo = a.wrange[0]; d.w_hi = a.wrange[1];
  d.dt = a.dt;
  d.gt2 = a.goal_tolerance * a.goal_tolerance;  // float32 product (mppi.py:960)
  d.lambda = a.lambda_weight;
  d.obs_cost = a.obs_cost;
  d.unk_cost = a.unknown_cost;
  d.res = a.res > 0.f ? a.res : 1.f;
  d.inv_res = 1.0f / d.res;
  d.xlo = a.xlo; d.ylo = a.ylo;
  d.cvar_alpha = a.cvar_alpha;
  // (samples sharded over GPUs: the local kernel's own reduction is not used; cvar_reduce_choose)
  d.numel = cvar_numel(p->cfg.num_grid_samples, a.cvar_alpha);
  d.dist_weight = a.dist_weight;
  d.v_post_den = (double)a.v_post_rollout + 1e-6;
  d.lin_lo = m.lin_lo; d.lin_ratio = m.lin_ratio; d.rows = m.rows; d.cols = m.cols;
  d.ang_lo = m.ang_lo; d.ang_ratio = m.ang_ratio;
  d.lin_zero_byte = -1;
  for (int b = 0; b < 128 && m.lin_grid; ++b)
    if (std::fma(d.lin_ratio, (double)b, d.lin_lo) == 0.0) { d.lin_zero_byte = b; break; }
  d.lin_max_byte = m.lin_max_byte;
  d.ang_max_byte = m.ang_max_byte;
  d.s0sq = (double)a.u_std[0] * (double)a.u_std[0];
  d.s1sq = (double)a.u_std[1] * (double)a.u_std[1];
  d.n_local = p->n_local;
  d.n_steps = p->cfg.num_steps;
  d.n_grids = p->cfg.num_grid_samples;
  const BareboneScene& sc = p->scene;
  d.n_obstacles = sc.shared.max;
  // (discs that move: a batch reads each problem's offset from its BatchInst, as it reads the start state)
  d.track_rows = sc.samples.on ? sc.samples.rows : sc.tracks.rows;  // (disc samples stand where the tracks do; no tracks: 0 rows)
  // (wall tracks share the offset: rollout_crowd_kernel.h clamps it against the walls' own row count)
  // (... and so does a goal track, against its own)
  d.track_off = (sc.tracks.on || sc.samples.on || sc.wall_tracks.on || sc.goal.on) && !p->inst_set ? p->inst_host[0].track_off : 0;
  d.inst = p->inst_set ? p->inst_dev : nullptr;
  d.inst_tiles = p->inst_tiles;
  d.n_inst = p->n_inst;
  d.spec_failures = p->spec_fail_dev;
  d.cc_k0 = (float)((double)a.lambda_weight / d.s0sq);
  d.cc_k1 = (float)((double)a.lambda_weight / d.s1sq);
  d.inv_v_post_den = 1.0 / d.v_post_den;
  d.neg_log2e_over_lambda = -1.4426950408889634 / (double)a.lambda_weight;
  d.car = p->drive == MPPI_DRIVE_CAR ? 1 : 0;
  return d;
}

static int reserve_cells(mppi_planner* p, const mppi_tdm* lin, int M) {
  size_t need = (size_t)lin->rows * lin->cols * M;
  if (need > p->cells_capacity) {
    HIP_TRY(hipStreamSynchronize(p->stream));
    dev_free(p->cells);
    p->cells_capacity = 0;  // (stays 0 if the allocation below fails)
    TRY(dev_alloc(&p->cells, need));
    p->cells_capacity = need;
  }
  return MPPI_OK;
}

// the cell words now hold these TDMs' grids: what the launches need to know of them (the only writer of p->packed)
static void note_packed(mppi_planner* p, const mppi_tdm* lin, const mppi_tdm* ang) {
  PackedMaps& m = p->packed;
  if (m.lin_maps != lin->maps_version) p->speculation_off = false;  // a new map: speculate again
  m.lin_maps = lin->maps_version; m.lin_grid = lin->grid_version;
  m.ang_maps = ang->maps_version; m.ang_grid = ang->grid_version;
  m.lin_lo = lin->lo; m.lin_ratio = lin->ratio; m.ang_lo = ang->lo; m.ang_ratio = ang->ratio;
  m.rows = lin->rows; m.cols = lin->cols;
  m.lin_max_byte = tdm_max_byte(lin); m.ang_max_byte = tdm_max_byte(ang);
  m.sink_ring = lin->injected ? lin->injected_sink_ring : lin->maps_sink_ring;
  m.risk = lin->risk;
}

// ---- from the TDMs to the cell words: what the route depends on (cvar_plan.h: cells_choose), read off the handles --
//      the only place that does.  for_solve: asked by sample_for_solve, with the alpha_dyn it samples at. ----------------
static CellsHeld cells_held(const mppi_planner* p, const mppi_tdm* lin, const mppi_tdm* ang, bool for_solve, double alpha_dyn) {
  CellsHeld h;
  memset(&h, 0, sizeof(h));
  h.mode = p->cfg.mode; h.M = p->cfg.num_grid_samples; h.for_solve = for_solve;
  if (h.mode == MPPI_MODE_BAREBONE) return h;  // (no TDMs)
  h.same_tdm = lin == ang;
  h.lin_rng = lin->cfg.rng; h.ang_rng = ang->cfg.rng; h.lin_bins = lin->bins; h.ang_bins = ang->bins;
  h.alpha_positive = alpha_dyn > 0.0;
  h.lin_first_sample = lin->first_sample; h.ang_first_sample = ang->first_sample;
  h.rows = lin->rows; h.cols = lin->cols;
  h.lin_compact_ok = lin->compact_ok; h.ang_compact_ok = ang->compact_ok;
  h.lin_injected = lin->injected; h.ang_injected = ang->injected;
  h.lin_injected_nonneg = lin->injected_min >= 0; h.ang_injected_nonneg = ang->injected_min >= 0;
  h.has_risk = lin->has_risk;
  const PackedMaps& m = p->packed;
  h.packed_match = m.lin_maps == lin->maps_version && m.lin_grid == lin->grid_version && m.ang_maps == ang->maps_version &&
                   m.ang_grid == ang->grid_version;
  return h;
}

// solve() of a CVaR planner: both TDMs sampled straight into the cell words the rollout gathers; the int8 grids follow
// on demand from the same counters (tdm_materialize)
static int sample_into_cells(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, double alpha_dyn, const CellsChoice& c) {
  const int M = p->cfg.num_grid_samples;
  TRY(reserve_cells(p, lin, M));
  static const decltype(&k_sample_cellsM_philox<8>) forms[4] = {k_sample_cellsM_philox<8>, k_sample_cellsM_philox<16>,
                                                                k_sample_cellsM_philox<32>, k_sample_cellsM_philox<64>};
  hipLaunchKernelGGL(forms[c.bins], dim3(c.grid_x), dim3(256), 0, p->stream, lin->pmf, lin->bins, lin->table, lin->cfg.seed,
                     lin->epoch, ang->pmf, ang->bins, ang->table, ang->cfg.seed, ang->epoch, lin->obs, lin->unk, lin->rows,
                     lin->cols, alpha_dyn, M, p->cells, (uint64_t)(lin->first_sample >> 1) * (uint64_t)c.cell_groups);
  if (hipGetLastError() != hipSuccess) return fail(MPPI_ERR_HIP, "k_sample_cellsM_philox launch failed");
  for (mppi_tdm* t : {lin, ang}) {
    t->sampled_epoch = t->epoch++;
    t->sampled_alpha = alpha_dyn;
    t->sampled_maps_version = t->maps_version;
    t->grid_stale = true;  // the int8 grids of these draws do not exist yet
    t->injected = false;
    t->grid_version = next_generation();
  }
  p->cells16_valid = false;
  note_packed(p, lin, ang);
  return MPPI_OK;
}

// (re)build the packed cell words when the sampled grids or the masks changed
static int ensure_packed(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang) {
  if (p->cfg.mode == MPPI_MODE_BAREBONE) return MPPI_OK;
  // solve() samples the traction grids itself; the stage-level entry points use what is there
  REQUIRE(lin->grid_version > 0 && ang->grid_version > 0, MPPI_ERR_STATE,
          "traction grids have never been sampled: call mppi_tdm_sample_grids (or mppi_planner_solve) first");
  const CellsChoice c = cells_choose(cells_held(p, lin, ang, false, 0.0));
  if (c.route == kCellsNothing) return MPPI_OK;
  const int M = p->cfg.num_grid_samples;
  TRY(reserve_cells(p, lin, M));
  // (another planner may have sampled these TDMs straight into ITS cell words)
  TRY(tdm_materialize(lin, p->stream));
  TRY(tdm_materialize(ang, p->stream));
  p->cells16_valid = false;
  if (c.route == kCellsPackMulti) {
    hipLaunchKernelGGL(k_pack_cells_multi, dim3(c.grid_x, c.grid_y), dim3(256), 0, p->stream, lin->grid, ang->grid,
                       lin->cfg.max_rows, lin->cfg.max_cols, lin->obs, lin->unk, lin->rows, lin->cols, M, p->cells);
  } else {
    hipLaunchKernelGGL(k_pack_cells_single, dim3(c.grid_x), dim3(256), 0, p->stream, lin->grid, ang->grid, lin->cfg.max_cols,
                       lin->obs, lin->unk, lin->rows, lin->cols, p->cells);
    if (c.mirror != kMirrorNone) {
      p->pitch16 = c.pitch16;
      if (c.mirror_units > p->cells16_capacity) {
        HIP_TRY(hipStreamSynchronize(p->stream));
        dev_free(p->cells16);
        p->cells16_capacity = 0;  // (stays 0 if the allocation below fails)
        TRY(dev_alloc(&p->cells16, c.mirror_units));
        p->cells16_capacity = c.mirror_units;
      }
      if (c.mirror == kMirror32Risk)
        hipLaunchKernelGGL(k_pack_cells32_risk, dim3(c.mirror_grid), dim3(256), 0, p->stream, lin->grid, ang->grid,
                           lin->cfg.max_cols, lin->obs, lin->unk, lin->risk, lin->rows, lin->cols, p->pitch16,
                           reinterpret_cast<uint32_t*>(p->cells16));
      else
        hipLaunchKernelGGL(k_pack_cells16, dim3(c.mirror_grid), dim3(256), 0, p->stream, lin->grid, ang->grid,
                           lin->cfg.max_cols, lin->obs, lin->unk, lin->rows, lin->cols, p->pitch16, p->cells16);
      p->cells16_valid = true;
      p->cells16_with_risk = c.mirror == kMirror32Risk;
    }
  }
  HIP_TRY(hipGetLastError());
  note_packed(p, lin, ang);
  return MPPI_OK;
}

// the TDMs checked, their maps packed if they changed, and the launches' parameters
static int prepare_launch(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, DevParams* d) {
  TRY(check_tdms(p, lin, ang));
  TRY(ensure_packed(p, lin, ang));
  *d = make_dev_params(p);
  return MPPI_OK;
}

// describe one noise generation (advances the Philox epoch); `back` > 0: the Philox block generated `back` epochs ago,
// by value (nothing advances)
static NoiseJob make_noise_job(mppi_planner* p, float2* target, int back = 0) {
  NoiseJob j;
  j.out = target;
  j.states = (p->cfg.rng == MPPI_RNG_XOROSHIRO) ? p->states : nullptr;
  j.seed = p->cfg.seed;
  // graph mode: the epoch is split into a by-value part that stays the same from one replay to
  // the next and the device-side count of executed updates (bumps_launched mirrors it: every
  // earlier update is ahead of this generator in stream order)
  const bool by_counter = p->graph_on && !back;
  j.gen_counter = by_counter ? (const uint64_t*)p->gen_dev : nullptr;
  j.epoch = by_counter ? p->noise_epoch - p->bumps_launched : p->noise_epoch - (uint64_t)back;
  j.n_local = p->n_local;
  j.n_offset = p->n_offset;
  j.n_steps = p->cfg.num_steps;
  j.std0 = p->params.u_std[0];
  j.std1 = p->params.u_std[1];
  if (p->cfg.rng == MPPI_RNG_PHILOX && !back) ++p->noise_epoch;
  return j;
}

// the next iteration's noise, by `extra` workgroups appended to a rollout launch; none: an empty job
static NoiseJob next_noise_job(mppi_planner* p, int extra) {
  NoiseJob j;
  memset(&j, 0, sizeof(j));
  return extra > 0 ? make_noise_job(p, p->noise_buf[p->noise_cur ^ 1]) : j;
}

// time-correlated noise is on (mppi_planner_set_noise_smoothing: barebone mode and Philox only)
static bool noise_smoothing_on(const mppi_planner* p) { return p->smooth_beta[0] != 0.0f || p->smooth_beta[1] != 0.0f; }

// The one place every generator launch comes from: in line, beside the rollout, beside the update, sample_noise, and a
// block generated again (`back`).  The handle's smoothing coefficients pick the kernel: none, k_noise as ever; else
// k_noise_smooth, a workgroup per tile, over the same job.  `ev_start` / `ev_stop` (mppi_planner_time_noise): the
// dispatch's own begin / end.
static int launch_noise(mppi_planner* p, float2* target, hipStream_t stream = nullptr, int back = 0,
                        hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
  long total = (long)noise_items(p->n_local, p->cfg.num_steps, p->cfg.rng == MPPI_RNG_PHILOX);  // one thread per item
  NoiseJob job = make_noise_job(p, target, back);
  hipStream_t on = stream ? stream : p->stream;
  if (noise_smoothing_on(p)) {
    NoiseSmoothJob smooth;
    smooth.job = job;
    smooth.beta0 = p->smooth_beta[0]; smooth.beta1 = p->smooth_beta[1];
    smooth.gain0 = p->smooth_gain[0]; smooth.gain1 = p->smooth_gain[1];
    const dim3 tiles(ceil_div(p->n_local, 64)), threads(64 * kSmoothWaves);
    const size_t lds = noise_smooth_lds(p->cfg.num_steps);
    if (ev_start || ev_stop) hipExtLaunchKernelGGL(k_noise_smooth, tiles, threads, lds, on, ev_start, ev_stop, 0, smooth);
    else hipLaunchKernelGGL(k_noise_smooth, tiles, threads, lds, on, smooth);
  } else if (ev_start || ev_stop) {
    hipExtLaunchKernelGGL(k_noise, dim3(ceil_div(total, 256)), dim3(256), 0, on, ev_start, ev_stop, 0, job);
  } else {
    hipLaunchKernelGGL(k_noise, dim3(ceil_div(total, 256)), dim3(256), 0, on, job);
  }
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

// ---- acceleration limits on the sampled controls (mppi_planner_set_control_limits; control_limits.h) ------------------
// The steps of the two components under the params in force: +inf where a component stays as drawn.
static void control_limit_steps(const mppi_planner* p, float d[2]) {
  for (int c = 0; c < 2; ++c) d[c] = p->limits_held ? control_limit_step_size(p->limit_accel[c], p->params.dt) : INFINITY;
}
// limits are held and at least one of them binds: the pass has something to do
static bool control_limits_on(const mppi_planner* p) {
  float d[2];
  control_limit_steps(p, d);
  return control_limit_binds(d[0]) || control_limit_binds(d[1]);
}

// The pass over `block`, in place, on the main stream: the block becomes the effective noise of the feasible sequences
// next to the u the stream holds at that point -- the one the coming rollout launch reads -- and the anchors.  u and the
// anchors are read from device memory; the box and the steps travel by value (graph_signature).
static int launch_noise_limit(mppi_planner* p, float2* block) {
  NoiseLimitJob j;
  j.block = block;
  j.u = p->u;
  j.anchor = p->anchor;
  j.n_local = p->n_local; j.n_steps = p->cfg.num_steps; j.inst_tiles = p->inst_tiles;
  j.lo0 = p->params.vrange[0]; j.hi0 = p->params.vrange[1];
  j.lo1 = p->params.wrange[0]; j.hi1 = p->params.wrange[1];
  float d[2];
  control_limit_steps(p, d);
  j.d0 = d[0]; j.d1 = d[1];
  const size_t lds = noise_limit_lds(p->cfg.num_steps);  // (the problem's controls)
  REQUIRE(lds <= 64 * 1024, MPPI_ERR_INVALID, "num_steps %d too large for the control limits", p->cfg.num_steps);
  hipLaunchKernelGGL(k_noise_limit, dim3(ceil_div(p->n_local, 64)), dim3(64), lds, p->stream, j);
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

// ---- the map modes: what the launch choice depends on (map_plan.h), read off a handle ----------------------------
static MapHeld map_held(const mppi_planner* p) {
  const mppi_params& a = p->params;
  const PackedMaps& m = p->packed;
  MapHeld h;
  memset(&h, 0, sizeof(h));  // (padding included: the choice is cached on a memcmp of this)
  h.mode = p->cfg.mode; h.math = p->cfg.math; h.debug_flags = p->debug_flags; h.speculation_off = p->speculation_off;
  h.n_local = p->n_local; h.T = p->cfg.num_steps; h.num_cus = p->num_cus; h.lds_per_cu = p->lds_per_cu;
  h.inst_set = p->inst_set; h.inst_tiles = p->inst_tiles; h.B = p->B;
  h.cells16_valid = p->cells16_valid; h.cells16_with_risk = p->cells16_with_risk; h.pitch16 = p->pitch16;
  h.rows = m.rows; h.cols = m.cols; h.lin_max_byte = m.lin_max_byte; h.ang_max_byte = m.ang_max_byte;
  h.sink_ring = m.sink_ring; h.grid_packed = m.lin_grid != 0;
  h.theta_bounded = p->theta_bounded;
  h.lin_lo = m.lin_lo; h.lin_ratio = m.lin_ratio; h.ang_lo = m.ang_lo; h.ang_ratio = m.ang_ratio;
  h.dt = a.dt; h.res = a.res; h.xlo = a.xlo; h.ylo = a.ylo;
  h.vrange[0] = a.vrange[0]; h.vrange[1] = a.vrange[1]; h.wrange[0] = a.wrange[0]; h.wrange[1] = a.wrange[1];
  h.x0 = a.x0[0]; h.y0 = a.x0[1];
  h.drive = p->drive;
  const MapStartBounds inside = map_start_bounds(h);
  h.starts_inside = map_start_inside(inside, h.x0, h.y0);
  if (p->inst_set)  // (the host mirror of the per-problem starts: what the window origins are planned from, apply_window)
    for (const BatchInst& I : p->inst_host) h.starts_inside = h.starts_inside && map_start_inside(inside, I.x0, I.y0);
  return h;
}

// A window plan (map_plan.h: map_window) into the launch parameters, and a batched handle's per-problem window origins
// into its host mirror -- the only place that writes them.  false: no LDS window.
static bool apply_window(mppi_planner* p, const MapHeld& h, const WindowPlan& w, DevParams& d, size_t* lds_bytes) {
  if (!w.cells) return false;
  d.pitch16 = p->pitch16;
  d.win_step_cells = w.step_cells;
  d.win_progressive = w.progressive;
  if (p->inst_set)
    for (BatchInst& I : p->inst_host) window_origin(h, w, I.x0, I.y0, &I.win_r0, &I.win_c0);
  if (!w.ok) return false;
  d.win_r0 = w.r0; d.win_c0 = w.c0; d.win_rows = w.rows; d.win_cols = w.cols;
  *lds_bytes = w.lds;
  return true;
}

// Decide whether the rollout can keep its map in LDS; fills the window fields of `d`.
static bool plan_lds_window(mppi_planner* p, DevParams& d, size_t* lds_bytes) {
  const MapHeld h = map_held(p);
  return apply_window(p, h, map_window(h), d, lds_bytes);
}

// ---- the CVaR mode: what its kernel choice depends on (cvar_plan.h: cvar_choose), read off a handle -- the only place
//      that does ------------------------------------------------------------------------------------------------------
static CvarHeld cvar_held(const mppi_planner* p) {
  CvarHeld h;
  memset(&h, 0, sizeof(h));
  h.map = map_held(p);
  h.num_grid_samples = p->cfg.num_grid_samples; h.m_count = p->m_count; h.want_sample_costs = p->want_sample_costs;
  return h;
}

// per-problem start / goal / window origin -> device, when they changed
static int upload_instances(mppi_planner* p) {
  if (!p->inst_set || !p->inst_dirty) return MPPI_OK;
  HIP_TRY(hipMemcpyAsync(p->inst_dev, p->inst_host.data(), sizeof(BatchInst) * (size_t)p->B,
                         hipMemcpyHostToDevice, p->stream));
  p->inst_dirty = false;
  return MPPI_OK;
}

// Rollout and update launches go through the extended launch call: with p->kev_start / kev_stop
// set (mppi_planner_time_kernels) the runtime stamps the dispatch's own begin / end -- what
// rocprofv3 reads -- into those events; with both null it is an ordinary launch.
// (A launch whose noise came from the second stream and that does not look at the generator's flag itself is ordered
//  behind it by the event, here, at the last moment: the launchers know which kernel runs.)
static void settle_noise_wait(mppi_planner* p) {
  if (!p->noise_wait_pending) return;
  p->noise_wait_pending = false;
  (void)hipStreamWaitEvent(p->stream, p->ev_noise_ready, 0);
}
#define MPPI_KLAUNCH(kernel, grid, block, lds, stream, ...) \
  (settle_noise_wait(p), hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, p->kev_start, p->kev_stop, 0, __VA_ARGS__))
// ... the kernels that do (DevParams::noise_flag; their DevParams through noise_flag_params)
#define MPPI_KLAUNCH_WAITS_ITSELF(kernel, grid, block, lds, stream, ...) \
  hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, p->kev_start, p->kev_stop, 0, __VA_ARGS__)
// MPPI_NO_NOISE_FLAG: the streams are ordered by events only, the wait of rounds 1-5
static bool noise_flag_disabled() {
  static const bool disabled = getenv("MPPI_NO_NOISE_FLAG") != nullptr;
  return disabled;
}
static bool flag_words(const mppi_planner* p) { return p->noise_flag_dev && p->progress_dev; }
static DevParams noise_flag_params(mppi_planner* p, DevParams d) {
  d.flag_fault = p->flag_fault_dev;
  if (p->noise_now.consumer == kOrderFlag && p->noise_wait_pending) {  // (not pending: an update settled in front has waited)
    d.noise_flag = p->noise_flag_dev;
    d.noise_flag_expect = p->noise_flag_expect;
    p->noise_wait_pending = false;
  } else {
    settle_noise_wait(p);
  }
  // (a stage-level launch signals too: nobody waits for it)
  if (noise_launch_signals(flag_words(p), noise_flag_disabled(), p->graph_on, p->stream_flags_off)) {
    d.progress = p->progress_dev;
    d.progress_value = ++p->progress_seq;
  }
  return d;
}


// ---- the launch choice of the map modes (map_plan.h: map_choose), cached on the state it was computed from ----------
// It is asked several times per iteration (which kernel runs, whether it generates its noise, whether the next launch
// can take this one's update, whether the peer exchange is usable).  map_choose is a pure function of MapHeld and the
// key is the whole MapHeld: a hit cannot be stale.
static const MapChoice& map_choice(const mppi_planner* p, const MapHeld& h) {
  if (!p->choice_valid || memcmp(&p->choice_held, &h, sizeof(h)) != 0) {
    p->choice_cached = map_choose(h);
    p->choice_held = h;
    p->choice_valid = true;
  }
  return p->choice_cached;
}

// inside an iteration: the rollout launch about to be made is the one the iteration's noise was chosen for
static int check_chosen_launch(const mppi_planner* p, int launch) {
  REQUIRE(p->noise_now.launch == kLaunchNone || p->noise_now.launch == launch, MPPI_ERR_STATE,
          "internal: rollout launch %d behind a noise choice made for launch %d", launch, p->noise_now.launch);
  return MPPI_OK;
}

// the next rollout launch runs a time-parallel kernel (k_rollout_scan, k_rollout_scan_exact): its geometry
static bool scan_plan(const mppi_planner* p, ScanPlan* out) {
  if (p->cfg.mode != MPPI_MODE_DET && p->cfg.mode != MPPI_MODE_SPEED_MAP) return false;
  const MapChoice& c = map_choice(p, map_held(p));
  if (c.family != kMapScan && c.family != kMapScanExact) return false;
  if (out) *out = c.scan;
  return true;
}

// the iteration loop may let the rollout launch generate its own noise: Philox counters only
static bool scan_generates_noise(const mppi_planner* p) {
  return !(p->debug_flags & MPPI_DEBUG_SCAN_READ_NOISE) && p->cfg.rng == MPPI_RNG_PHILOX && scan_plan(p, nullptr);
}

// ---- the update: what its choice depends on (update_plan.h), read off a handle -- the only place that does ----------
// The arguments are launch_iteration's; a stage-level call has none.  launch_iteration adds what only it knows
// (want_next, have_noise, side_stream_pays).
static UpdateHeld update_held(const mppi_planner* p, bool prof = false, bool defer_exchange = false, bool may_leave_apply = false) {
  UpdateHeld h;
  memset(&h, 0, sizeof(h));
  h.mode = p->cfg.mode; h.world_size = p->cfg.world_size; h.has_comm = p->comm != nullptr; h.m_count = p->m_count;
  h.B = p->B; h.inst_set = p->inst_set; h.n_local = p->n_local; h.n_inst = p->n_inst; h.inst_tiles = p->inst_tiles;
  h.T = p->cfg.num_steps; h.rng = p->cfg.rng;
  h.debug_flags = p->debug_flags; h.fold_off = p->fold_off; h.p2p_on = p->p2p_on; h.graph_on = p->graph_on;
  h.stream_flags_off = p->stream_flags_off; h.flags_env_off = noise_flag_disabled();
  h.flag_words = flag_words(p);
  h.prof = prof; h.defer_exchange = defer_exchange; h.may_leave_apply = may_leave_apply; h.mirror_now = p->mirror_now;
  h.scan_packets_fresh = p->scan_packets_fresh; h.tile_packets_fresh = p->tile_packets_fresh; h.scan_tile = p->scan_tile;
  ScanPlan next;
  h.next_scan = scan_plan(p, &next);
  h.next_tile = h.next_scan ? next.tile : 0;
  return h;
}

// the noise of the last iteration into noise_buf when it exists as counters only
static int materialize_noise(mppi_planner* p) {
  if (!p->noise_virtual) return MPPI_OK;
  TRY(launch_noise(p, p->noise, nullptr, p->noise_virtual_back));  // the block the last rollout launch consumed
  p->noise_virtual = false;
  return MPPI_OK;
}

// this exchange's view of the inboxes; every exchange uses the other set
static PeerExchange make_peer_exchange(mppi_planner* p) {
  PeerExchange X;
  memset(&X, 0, sizeof(X));
  for (int g = 0; g < p->cfg.world_size; ++g) X.inbox[g] = p->peer_inbox[g];
  X.world = p->cfg.world_size;
  X.rank = p->cfg.rank;
  X.fault = p->p2p_fault_dev;
  // how long a rank waits for its peers before it gives the call up (~0.3 us per poll: ~5 s by default; the ranks of a
  // control loop call solve() together, but a host may be late by a map update or a garbage collection)
  static const int max_polls = getenv("MPPI_P2P_MAX_POLLS") ? atoi(getenv("MPPI_P2P_MAX_POLLS")) : (1 << 24);
  X.max_polls = max_polls;
  X.set = p->p2p_index & 1;
  ++p->p2p_index;
  ++p->p2p_exchanges;
  return X;
}

static PendingApply make_pending_apply(mppi_planner* p, int tiles);  // (with the update launches, below)

static int launch_scan(mppi_planner* p, const DevParams& d, const ScanPlan& plan) {
  const int N = p->n_local, T = p->cfg.num_steps;
  const bool speed = plan.speed;
  REQUIRE(!speed || (plan.exact && !plan.direct), MPPI_ERR_STATE, "internal: speed-map mode on a kernel that does not serve it");
  const int tiles = ceil_div(N, plan.tile);
  REQUIRE(p->tile_packets[0] && p->tile_packets[1], MPPI_ERR_STATE, "internal: no tile packet buffers on this handle");
  const bool gen = p->noise_now.source == kNoiseInKernel;
  ScanPackets pk;
  pk.tiles = p->tile_packets[p->tpk_cur ^ 1];  // (the other one may be read by this very launch: reduce_pending)
  pk.n_tiles = tiles;
  NoiseJob gen_job;
  memset(&gen_job, 0, sizeof(gen_job));
  if (gen) gen_job = make_noise_job(p, nullptr);  // (advances the Philox epoch: this iteration's block)
  // a loop that stores its noise (debug flag; the stage-level calls): CUs without a workgroup
  // produce the next iteration's, as in k_rollout_pipe.  (Producing it in the launch's own tail, by
  // the waves that idle while one wave accumulates the costs, was measured: the stage gained is lost
  // again to the slower accumulation and the noise reads -- profiles/r03_scan_notes.md.)
  const int extra = p->noise_now.extra_blocks;
  REQUIRE(!extra || (!plan.exact && tiles + extra == p->num_cus), MPPI_ERR_STATE, "internal: %d noise blocks chosen for %d tiles", extra, tiles);
  const NoiseJob next_job = next_noise_job(p, extra);
  if (p->reduce_pending) {
    REQUIRE(!p->apply_pending, MPPI_ERR_STATE, "internal: tile packets left to a launch that cannot reduce them");
    REQUIRE(tiles_can_reduce(tiles, T) && plan.tile == p->scan_tile, MPPI_ERR_STATE, "internal: %d workgroups cannot combine the tile packets of %d steps", tiles, T);
  }
  // an update left to this launch (launch_update): the rank packets, or the previous launch's `tiles` tile packets
  const PendingApply pend = make_pending_apply(p, tiles);
  if (!plan.direct) p->spec_launches += 1;
  // Exact kernel: where a tile whose vote fails is re-executed, or (direct) every tile runs (map_plan.h: map_scan)
  REQUIRE(!plan.direct || plan.fallback_offset >= 0, MPPI_ERR_STATE, "internal: direct exact schedule without its map window");
  const ScanFallback fallback = {plan.fallback_offset, plan.fallback_map_bytes, plan.direct ? 1 : 0, plan.rot_ok ? 1 : 0, plan.small_offset};
#define MPPI_LAUNCH_SCAN_EXACT(P2, GEN)                                                                    \
  do {                                                                                                    \
    auto kern = speed ? k_rollout_scan_exact<P2, GEN, false, true>                                        \
                      : (plan.direct ? k_rollout_scan_exact<P2, GEN, true> : k_rollout_scan_exact<P2, GEN, false>); \
    if (plan.lds > 64 * 1024)                                                                             \
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                                    \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));            \
    MPPI_KLAUNCH(kern, dim3(tiles), dim3(64 * plan.waves), plan.lds, p->stream, d, p->cells16, p->cells,   \
                 p->noise, gen_job, p->u, p->costs, p->w_rel, pk, pend, fallback,                          \
                 (const int8_t*)(speed ? p->packed.risk : nullptr));                                       \
  } while (0)
#define MPPI_LAUNCH_SCAN(RR, P2, GEN)                                                                      \
  do {                                                                                                    \
    auto kern = k_rollout_scan<RR, P2, GEN>;                                                              \
    if (plan.lds > 64 * 1024)                                                                             \
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                                    \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));            \
    MPPI_KLAUNCH(kern, dim3(tiles + extra), dim3(64 * plan.waves), plan.lds, p->stream, d, p->cells16,    \
                 p->noise, gen_job, p->u, p->costs, p->w_rel, pk, tiles, next_job, pend);                  \
  } while (0)
#define MPPI_LAUNCH_SCAN_G(RR, P2)               \
  do {                                           \
    if (gen) MPPI_LAUNCH_SCAN(RR, P2, true);     \
    else MPPI_LAUNCH_SCAN(RR, P2, false);        \
  } while (0)
  if (plan.exact) {
    if (plan.pow2res && gen) MPPI_LAUNCH_SCAN_EXACT(true, true);
    else if (plan.pow2res) MPPI_LAUNCH_SCAN_EXACT(true, false);
    else if (gen) MPPI_LAUNCH_SCAN_EXACT(false, true);
    else MPPI_LAUNCH_SCAN_EXACT(false, false);
  } else if (plan.tile == 64 && plan.pow2res) MPPI_LAUNCH_SCAN_G(64, true);
  else if (plan.tile == 64) MPPI_LAUNCH_SCAN_G(64, false);
  else if (plan.pow2res) MPPI_LAUNCH_SCAN_G(32, true);
  else MPPI_LAUNCH_SCAN_G(32, false);
#undef MPPI_LAUNCH_SCAN_G
#undef MPPI_LAUNCH_SCAN
#undef MPPI_LAUNCH_SCAN_EXACT
  HIP_TRY(hipGetLastError());
  const bool applied_here = p->apply_pending || p->reduce_pending;
  if (applied_here) {  // the first tile's workgroup has written the updated sequence into the other buffer
    std::swap(p->u, p->u_alt);
    p->u_parity ^= 1;
    if (p->reduce_pending) {
      ++p->reduce_index;
      ++p->reduced_applies;
    } else {
      ++p->folded_applies;
    }
    p->apply_pending = p->reduce_pending = false;
  }
  p->tpk_cur ^= 1;
  char buf[384];
  snprintf(buf, sizeof(buf),
           "k_rollout_scan%s tile=%d waves=%d pow2res=%d noise=%s lds=%zu noise_blocks=%d problems=%d%s%s",
           plan.exact ? (speed ? "_exact speed_map" : "_exact") : "", plan.tile, plan.waves, (int)plan.pow2res, gen ? "in-kernel" : "read", plan.lds, extra,
           p->inst_set ? p->B : 0, !plan.exact ? "" : (plan.direct ? " direct=1 (exact three-wave schedule, no speculation)" : (fallback.offset >= 0 ? " failed_tiles=pipelined" : " failed_tiles=one_wave")), applied_here ? (pend.reduce_tiles ? " applies_update=1 reduces_tiles=1" : " applies_update=1") : "");
  p->last_rollout = buf;
  p->tile_packets_fresh = false;  // (w_rel is relative to this kernel's own tiles: tbeta, not tile_beta)
  p->scan_packets_fresh = true;
  p->scan_tile = plan.tile;
  p->noise_virtual = gen;
  p->noise_virtual_back = 1 + (next_job.out ? 1 : 0);  // (the launch may have produced its successor's block too)
  return MPPI_OK;
}

// ---- the map modes: one launcher per kernel family, carrying out a choice (map_plan.h) ----------
static int launch_pipe(mppi_planner* p, const DevParams& d, const MapChoice& c) {
  const int N = p->n_local, T = p->cfg.num_steps;
  // spare CUs generate the next iteration's noise inside this launch (no spare CU: in line)
  const int extra = p->noise_now.extra_blocks;
  REQUIRE(!extra || c.grid + extra == p->num_cus, MPPI_ERR_STATE, "internal: %d noise blocks chosen for %d workgroups", extra, c.grid);
  const NoiseJob next_job = next_noise_job(p, extra);
  if (!c.cc_lds && !p->cc_scratch) TRY(dev_alloc(&p->cc_scratch, (size_t)ceil_div(N, 64) * 64 * T));
  // the compile-time form: [chunk 8, 6, 4, 2][POW2RES][CC_LDS]
#define MPPI_PIPE_FORMS(CH) \
  {{k_rollout_pipe<CH, false, false>, k_rollout_pipe<CH, false, true>}, {k_rollout_pipe<CH, true, false>, k_rollout_pipe<CH, true, true>}}
  static const decltype(&k_rollout_pipe<8, true, true>) forms[4][2][2] = {MPPI_PIPE_FORMS(8), MPPI_PIPE_FORMS(6), MPPI_PIPE_FORMS(4), MPPI_PIPE_FORMS(2)};
#undef MPPI_PIPE_FORMS
  const auto kern = forms[(8 - c.chunk) / 2][c.pow2res][c.cc_lds];
  if (c.lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds));
  MPPI_KLAUNCH(kern, dim3(c.grid + extra), dim3(c.block), c.lds, p->stream, d, p->cells16, p->noise, p->u, p->costs, p->w_rel,
               p->tile_beta, p->cc_scratch, c.map_bytes, c.grid, next_job);
  char buf[256];
  snprintf(buf, sizeof(buf),
           "k_rollout_pipe chunk=%d pow2res=%d cc_lds=%d triples_per_wg=%d window=%dx%d@(%d,%d) lds=%zu "
           "noise_blocks=%d problems=%d",
           c.chunk, (int)c.pow2res, (int)c.cc_lds, c.triples, d.win_rows, d.win_cols, d.win_r0, d.win_c0, c.lds, extra,
           p->inst_set ? p->B : 0);
  p->last_rollout = buf;
  p->tile_packets_fresh = true;
  return MPPI_OK;
}

// k_rollout_fused, the deterministic-dynamics and the speed-map forms
static int launch_fused(mppi_planner* p, DevParams d, const MapChoice& c) {
  const bool P2 = c.pow2res;
  auto fused = c.speed ? (c.one_pass ? (P2 ? k_rollout_fused<true, true, true> : k_rollout_fused<false, true, true>)
                                     : (P2 ? k_rollout_fused<true, true> : k_rollout_fused<false, true>))
               : c.one_pass ? (P2 ? k_rollout_fused<true, false, true> : k_rollout_fused<false, false, true>)
               : c.lone ? (P2 ? k_rollout_fused<true, false, false, true> : k_rollout_fused<false, false, false, true>)
                        : (P2 ? k_rollout_fused<true> : k_rollout_fused<false>);
  d.stash_steps = c.stash_steps;
  d.stash_offset = c.stash_offset;
  if (c.lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fused), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds));
  MPPI_KLAUNCH_WAITS_ITSELF(fused, dim3(c.grid), dim3(c.block), c.lds, p->stream, noise_flag_params(p, d), p->cells16,
                            p->noise, p->u, p->costs, p->w_rel, p->tile_beta);
  char buf[200];
  int len = snprintf(buf, sizeof(buf), "k_rollout_fused%s%s pow2res=%d waves_per_wg=%d window=%dx%d problems=%d",
                     c.one_pass ? "<one pass>" : "", c.speed ? " speed_map" : "", (int)P2, c.waves, d.win_rows, d.win_cols,
                     p->inst_set ? p->B : 0);
  if (!c.speed) snprintf(buf + len, sizeof(buf) - len, " noise_kept=%d", c.stash_steps);
  p->last_rollout = buf;
  p->tile_packets_fresh = true;
  return MPPI_OK;
}

// k_rollout_map: no incremental trig, or no LDS window
template <bool EXACT, bool BOUNDED>
static int launch_general(mppi_planner* p, const DevParams& d, const MapChoice& c) {
  const bool speed = p->cfg.mode == MPPI_MODE_SPEED_MAP;
  const auto kern = c.windowed ? k_rollout_map<MAP_DET, EXACT, BOUNDED, true>
                               : (speed ? k_rollout_map<MAP_SPEED, EXACT, BOUNDED, false> : k_rollout_map<MAP_DET, EXACT, BOUNDED, false>);
  if (c.windowed && c.lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds));
  MPPI_KLAUNCH(kern, dim3(c.grid), dim3(c.block), c.lds, p->stream, d, p->cells,
               c.windowed ? p->cells16 : (const uint16_t*)nullptr, (const int8_t*)(speed ? p->packed.risk : nullptr), p->noise, p->u, p->costs);
  char buf[200];
  if (c.windowed)
    snprintf(buf, sizeof(buf), "k_rollout_map det lds_window exact=%d waves_per_wg=%d window=%dx%d problems=%d", (int)EXACT, c.waves,
             d.win_rows, d.win_cols, p->inst_set ? p->B : 0);
  else
    snprintf(buf, sizeof(buf), "k_rollout_map %s global_cells exact=%d", speed ? "speed_map" : "det", (int)EXACT);
  p->last_rollout = buf;
  return MPPI_OK;
}

// deterministic-dynamics and speed-map mode: ask the choice, carry it out
template <bool EXACT, bool BOUNDED>
static int launch_rollout_map(mppi_planner* p, DevParams d) {
  p->tile_packets_fresh = false;
  const MapHeld h = map_held(p);
  const MapChoice c = map_choice(p, h);
  TRY(check_chosen_launch(p, c.family + 1));
  size_t lds_win = 0;
  (void)apply_window(p, h, c.window, d, &lds_win);
  TRY(upload_instances(p));
  switch (c.family) {
    case kMapScan:
    case kMapScanExact: return launch_scan(p, d, c.scan);
    case kMapPipe: TRY(launch_pipe(p, d, c)); break;
    case kMapFused: TRY(launch_fused(p, d, c)); break;
    case kMapGeneral: TRY((launch_general<EXACT, BOUNDED>(p, d, c))); break;
  }
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

// CVaR mode: ask the choice (cvar_plan.h: cvar_choose), allocate what it names, launch its form, write the text
static int launch_rollout_tdm(mppi_planner* p, const DevParams& d) {
  const int N = p->n_local, T = p->cfg.num_steps, M = p->cfg.num_grid_samples;
  const CvarChoice c = cvar_choose(cvar_held(p));
  REQUIRE(!c.refused, MPPI_ERR_INVALID, "T=%d, M=%d need %zu bytes of LDS (> 160 KiB)", T, M, c.lds);
  static const decltype(&k_rollout_tdm<true>) general[2] = {k_rollout_tdm<false>, k_rollout_tdm<true>};  // [EXACT]
  static const decltype(&k_rollout_tdm_fast<true, true>) fast[2][2] = {  // [POW2RES][cost f32]
      {k_rollout_tdm_fast<false, false>, k_rollout_tdm_fast<false, true>}, {k_rollout_tdm_fast<true, false>, k_rollout_tdm_fast<true, true>}};
  if (c.set_attribute)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(general[c.exact]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds));
  if (c.costs_to == kCvarCostsSampleCosts && !p->sample_costs) TRY(dev_alloc(&p->sample_costs, (size_t)N * M));
  if (c.costs_to == kCvarCostsSlab && !p->slabs) TRY(dev_alloc(&p->slabs, (size_t)p->m_count * N * M));
  // sharded samples: the per-sample costs go into this rank's slab of the gather buffer
  float* const sc_dst = c.costs_to == kCvarCostsSlab ? p->slabs + (size_t)p->m_rank * N * M
                                                     : (c.costs_to == kCvarCostsSampleCosts ? p->sample_costs : nullptr);
  p->tile_packets_fresh = false;
  TRY(upload_instances(p));
  TRY(check_chosen_launch(p, c.launch));
  if (c.fast) {
    // the next iteration's noise by workgroups appended to the grid (they run in the launch's tail)
    const int extra = p->noise_now.extra_blocks;
    const NoiseJob next_job = next_noise_job(p, extra);
    MPPI_KLAUNCH(fast[c.pow2res][c.cost_f32], dim3(N + extra), dim3(c.threads), c.lds, p->stream, d, p->cells, p->noise, p->u,
                 p->costs, sc_dst, c.mp2, N, next_job);
    p->last_rollout = std::string(c.cost_f32 ? "k_rollout_tdm_fast<cost f32>" : "k_rollout_tdm_fast") + " pow2res=" +
                      (c.pow2res ? "1" : "0") + " noise_blocks=" + std::to_string(extra);
  } else {
    MPPI_KLAUNCH(general[c.exact], dim3(N), dim3(c.threads), c.lds, p->stream, d, p->cells, p->noise, p->u, p->costs, sc_dst, c.mp2);
    p->last_rollout = "k_rollout_tdm exact=" + std::to_string(c.exact);
  }
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

// The barebone mode: the launch choice and one launcher per kernel family
#include "barebone_launch.h"

template <bool EXACT, bool BOUNDED>
static int launch_rollout_t(mppi_planner* p, DevParams d) {
  p->scan_packets_fresh = false;
  if (p->noise_virtual && p->noise_now.source != kNoiseInKernel) TRY(materialize_noise(p));  // the coming kernel reads its noise
  switch (p->cfg.mode) {
    case MPPI_MODE_DET:
    case MPPI_MODE_SPEED_MAP: return launch_rollout_map<EXACT, BOUNDED>(p, d);
    case MPPI_MODE_TDM: return launch_rollout_tdm(p, d);
    case MPPI_MODE_BAREBONE: {
      TRY(check_chosen_launch(p, kLaunchBarebone));
      p->tile_packets_fresh = false;
      // (cos, sin) by rotation where the host can bound the heading increment: |dt * w| <= 0.36 rad, T <= 2000
      const bool rot = EXACT && map_rotation_ok(map_held(p));
      return p->inst_set ? launch_barebone<EXACT, true>(p, d, rot) : launch_barebone<EXACT, false>(p, d, rot);
    }
    default:
      return fail(MPPI_ERR_INVALID, "bad mode");
  }
}


static int launch_apply(mppi_planner* p);
static int settle_reduce_pending(mppi_planner* p);

// |theta| can never exceed |theta0| + T*dt*max|w|*max(traction): when that is far
// inside the range of the two-term pi/2 reduction, the kernels drop the libm branch
static bool refresh_theta_bounded(mppi_planner* p) {
  const mppi_params& a = p->params;
  const MapReach reach = map_reach(map_held(p));
  double th0_max = std::fabs((double)a.x0[2]);
  if (p->inst_set) {
    th0_max = 0.0;
    for (const BatchInst& I : p->inst_host) th0_max = std::fmax(th0_max, std::fabs((double)I.th0));
  }
  const double theta_bound = th0_max + (double)p->cfg.num_steps * (double)a.dt * reach.wmax * reach.trmax_ang;
  return p->theta_bounded = std::isfinite(theta_bound) && theta_bound < 5.0e4;
}

static int launch_rollout(mppi_planner* p, const DevParams& d) {
  REQUIRE(p->B == 1 || p->inst_set, MPPI_ERR_STATE,
          "num_instances = %d: call mppi_planner_set_instances before solving", p->B);
  REQUIRE((size_t)p->cfg.num_steps * sizeof(double2) <= 64 * 1024, MPPI_ERR_INVALID, "num_steps %d too large",
          p->cfg.num_steps);
  // an update left to its consumer (launch_update) and a rollout kernel that will not take it
  if (p->apply_pending || p->reduce_pending) {
    const UpdateHeld held = update_held(p);
    if (p->apply_pending && !rollout_keeps_pending_packets(held)) TRY(launch_apply(p));  // (sharded updates fold in deterministic-dynamics mode only)
    if (p->reduce_pending && !next_rollout_takes(held).reduces_tiles) TRY(settle_reduce_pending(p));
  }
  const bool bounded = refresh_theta_bounded(p);
  // mppi_planner_time_kernels on a two-stream loop: the kernels of the throughput regime stamp their own begin / end
  DevParams dk = d;
  dk.ktime = p->ktime_rollout_slot;
  dk.ktime_waves = p->ktime_waves;
  if (p->cfg.math != MPPI_MATH_EXACT) return launch_rollout_t<false, false>(p, dk);
  return bounded ? launch_rollout_t<true, true>(p, dk) : launch_rollout_t<true, false>(p, dk);
}

// ---- CVaR mode, samples sharded over GPUs: all-gather of the (N, M/G) cost slabs, then every
//      rank reduces all N control samples over all M costs ---------------
static int launch_cvar_reduce(mppi_planner* p) {
  const int N = p->n_local, Ml = p->cfg.num_grid_samples;
  const CvarReduceChoice c = cvar_reduce_choose(Ml, p->m_count, p->params.cvar_alpha);
  REQUIRE(!c.refused, MPPI_ERR_INVALID, "M = %d samples over all shards: too many for the CVaR reduction", c.m_total);
  if (p->want_sample_costs && p->sample_costs == nullptr) TRY(dev_alloc(&p->sample_costs, (size_t)N * c.m_total));
  hipLaunchKernelGGL(k_cvar_reduce, dim3(N), dim3(c.threads), c.lds, p->stream, p->slabs, p->m_count, N, Ml, c.numel,
                     p->params.cvar_alpha, p->costs, p->want_sample_costs ? p->sample_costs : (float*)nullptr, c.mp2);
  HIP_TRY(hipGetLastError());
  p->tile_packets_fresh = false;
  p->sample_costs_local_only = false;
  return MPPI_OK;
}

// inside the iteration loop: RCCL all-gather of the slabs on the planner's stream, then the reduction
static int exchange_sample_costs(mppi_planner* p) {
  if (p->m_count <= 1) return MPPI_OK;
  REQUIRE(p->comm, MPPI_ERR_STATE,
          "samples sharded over %d ranks but no communicator: call mppi_planner_comm_init "
          "(or drive rollout / sample_costs_local / sample_costs_apply / update yourself)", p->m_count);
  const size_t len = (size_t)p->n_local * p->cfg.num_grid_samples;
  RCCL_TRY(g_rccl.AllGather(p->slabs + (size_t)p->m_rank * len, p->slabs, len, ncclFloat, p->comm, p->stream));
  return launch_cvar_reduce(p);
}

// ---- the update: launch_update carries out a choice (update_plan.h: update_choose), one launcher
//      per kernel family.  The choice is pure; every side effect on the handle happens here. ---------------------------
static_assert(kUpdateRowsBlock == kRowThreads, "update_plan.h and update_kernels.h disagree");

// where a local launch leaves this rank's packet for an exchange; the host mirror, written by solve()'s last update only
static double* update_packet(const mppi_planner* p) { return p->packets + (size_t)p->cfg.rank * p->B * packet_len(p->cfg.num_steps); }
static float2* update_mirror(const mppi_planner* p) { return p->mirror_now ? p->u_host_dev : (float2*)nullptr; }

// k_combine_tiles: the rollout launch (a time-parallel kernel) has reduced w_rel * noise over every tile
static int launch_combine_tiles(mppi_planner* p, const UpdateChoice& c) {
  const mppi_params& a = p->params;
  p->scan_packets_fresh = false;
  p->tile_packets_fresh = false;
  unsigned long long* gen = p->graph_on ? p->gen_dev : (unsigned long long*)nullptr;
  // (graph replay: this launch also accounts for the iterations whose update ran inside a rollout launch)
  const unsigned long long bump = 1ull + (unsigned long long)p->bumps_owed;
  PeerExchange peers;
  memset(&peers, 0, sizeof(peers));
  if (c.peers_ride) peers = make_peer_exchange(p);  // (exchanged inside the launch; advances the inbox set)
  static const decltype(&k_combine_tiles<true>) forms[2] = {k_combine_tiles<false>, k_combine_tiles<true>};  // [APPLY]
  MPPI_KLAUNCH(forms[c.apply_here], dim3(c.grid_x, c.grid_y), dim3(c.block), 0, p->stream, p->tile_packets[p->tpk_cur],
               c.per_problem_tiles, p->cfg.num_steps, a.lambda_weight, update_packet(p), p->u, p->u_prev, update_mirror(p),
               a.vrange[0], a.vrange[1], a.wrange[0], a.wrange[1], p->stats, gen, bump, p->published, peers);
  if (p->graph_on) p->bumps_launched += bump;
  p->bumps_owed = 0;
  p->reduce_index = 0;  // (the flags are all clear again)
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

// k_update_rows, with k_tile_weights in front where the choice says so: applies the update, or leaves this rank's
// packet for the exchange
static int launch_update_rows(mppi_planner* p, const UpdateChoice& c) {
  const mppi_params& a = p->params;
  if (p->noise_virtual) TRY(materialize_noise(p));  // the row kernel streams the noise
  if (c.tile_weights_first)
    MPPI_KLAUNCH(k_tile_weights, dim3(p->n_tiles), dim3(64), 0, p->stream, p->costs, p->n_local, a.lambda_weight,
                 p->w_rel, p->tile_beta);
  p->tile_packets_fresh = false;
  REQUIRE(c.lds <= kUpdateLdsMax, MPPI_ERR_INVALID, "too many rollouts per GPU for the update kernel (%d)", p->n_local);
  // the compile-time form: [APPLY][TC 1, 4][FROM_COSTS][slim: 256 threads]
#define MPPI_ROWS_FORMS(APPLY, TC)                                              \
  {{k_update_rows<APPLY, TC, false>, k_update_rows<APPLY, TC, false, kUpdateRowsSlimBlock>}, \
   {k_update_rows<APPLY, TC, true>, k_update_rows<APPLY, TC, true, kUpdateRowsSlimBlock>}}
  static const decltype(&k_update_rows<true, 1, true>) forms[2][2][2][2] = {{MPPI_ROWS_FORMS(false, 1), MPPI_ROWS_FORMS(false, 4)},
                                                                           {MPPI_ROWS_FORMS(true, 1), MPPI_ROWS_FORMS(true, 4)}};
#undef MPPI_ROWS_FORMS
  const auto kern = forms[c.apply_here][c.rows_per_wg == 4][c.from_costs][c.slim];
  // (slim: the launch signals its start to the gate kernel in front of the noise generator beside it)
  MPPI_KLAUNCH(kern, dim3(c.grid_x, c.grid_y), dim3(c.block), c.lds_launch, p->stream, c.from_costs ? p->costs : p->w_rel,
               p->tile_beta, p->n_inst, p->inst_tiles, p->noise, p->cfg.num_steps, a.lambda_weight, update_packet(p), p->u,
               p->u_prev, update_mirror(p), a.vrange[0], a.vrange[1], a.wrange[0], a.wrange[1], p->stats,
               p->graph_on ? p->gen_dev : (unsigned long long*)nullptr, p->ktime_update_slot, p->ktime_waves,
               c.slim ? p->progress_dev : (unsigned long long*)nullptr, c.slim ? p->progress_seq : 0ull);
  if (p->graph_on) ++p->bumps_launched;
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

static int launch_update_kernel(mppi_planner* p, const UpdateChoice& c) {
  return c.kernel == kUpdateCombineTiles ? launch_combine_tiles(p, c) : launch_update_rows(p, c);
}

// (out of place into the handle's other control buffer, like an update applied by its consumer: every
//  sharded iteration flips the two, and an even number of iterations -- a graph -- restores them)
static int launch_apply(mppi_planner* p) {
  const mppi_params& a = p->params;
  hipLaunchKernelGGL(k_apply, dim3(p->B), dim3(kUpdateThreads), 0, p->stream, p->packets, p->cfg.world_size,
                     p->cfg.rank, p->cfg.num_steps, a.lambda_weight, p->u, p->u_alt, p->u_prev, update_mirror(p), a.vrange[0],
                     a.vrange[1], a.wrange[0], a.wrange[1], p->stats);
  HIP_TRY(hipGetLastError());
  std::swap(p->u, p->u_alt);
  p->u_parity ^= 1;
  p->apply_pending = false;
  return MPPI_OK;
}

// What a time-parallel rollout launch over `tiles` workgroups needs to take the update left to it (PendingApply): the
// gathered rank packets (apply_pending), or the previous launch's tile packets -- as many as this launch has tiles:
// launch_scan has checked -- which it combines and applies itself (reduce_pending; several GPUs: with the peer
// exchange in between).  Nothing pending: all zero.
static PendingApply make_pending_apply(mppi_planner* p, int tiles) {
  PendingApply pend;
  memset(&pend, 0, sizeof(pend));
  if (!p->apply_pending && !p->reduce_pending) return pend;
  const mppi_params& a = p->params;
  pend.packets = p->packets;  // (not read when the tiles are reduced; non-null: "an update is pending")
  pend.u_out = p->u_alt;
  pend.u_prev = p->u_prev;
  pend.stats = p->stats;
  pend.world = p->reduce_pending ? 1 : p->cfg.world_size;
  pend.stride = p->B * packet_len(p->cfg.num_steps);
  pend.lambda = a.lambda_weight;
  pend.v_lo = a.vrange[0]; pend.v_hi = a.vrange[1];
  pend.w_lo = a.wrange[0]; pend.w_hi = a.wrange[1];
  if (p->reduce_pending) {
    pend.reduce_tiles = p->tile_packets[p->tpk_cur];
    pend.reduce_n_tiles = tiles;
    pend.published = p->published;
    pend.flag_set = p->reduce_index & 1;
    pend.fault = p->fold_fault_dev;
    pend.max_polls = p->fold_max_polls;
    if (p->p2p_on) pend.peers = make_peer_exchange(p);  // (advances the inbox set)
  }
  return pend;
}

// tile packets left to a rollout launch that will not come (another kernel family, a stage-level call): the
// ordinary combination, applied here on any number of GPUs
static int settle_reduce_pending(mppi_planner* p) {
  p->reduce_pending = false;
  p->scan_packets_fresh = true;
  return launch_update_kernel(p, update_local_launch(update_held(p), kUpdateLocalApply));
}

static int launch_update(mppi_planner* p, const UpdateChoice& c, bool prof) {
  p->mirror_done = p->mirror_now;
  if (c.route == kUpdateLeaveTiles) {  // no launch here
    p->scan_packets_fresh = false;
    p->reduce_pending = true;
    if (p->graph_on) ++p->bumps_owed;
    return MPPI_OK;
  }
  if (c.route == kUpdatePacketOnly) return launch_update_kernel(p, c);
  if (c.route == kUpdateLocalApply) {
    TRY(launch_update_kernel(p, c));
    if (prof) {
      HIP_TRY(hipEventRecord(p->ev_stage[3], p->stream));
      HIP_TRY(hipEventRecord(p->ev_stage[4], p->stream));
    }
    return MPPI_OK;
  }
  REQUIRE(p->comm, MPPI_ERR_STATE,
          "world_size %d but no communicator: call mppi_planner_comm_init (or use update_local/update_apply)",
          p->cfg.world_size);
  TRY(launch_update_kernel(p, c));
  const int len = p->B * packet_len(p->cfg.num_steps);
  if (prof) HIP_TRY(hipEventRecord(p->ev_stage[3], p->stream));
  // one all-gather of (2T+2) doubles per problem and iteration, in place
  TraceRange tr("mppi:all_gather_packets");
  RCCL_TRY(g_rccl.AllGather(p->packets + (size_t)p->cfg.rank * len, p->packets, (size_t)len, ncclDouble, p->comm,
                            p->stream));
  if (prof) HIP_TRY(hipEventRecord(p->ev_stage[4], p->stream));
  if (c.route == kUpdateGatherLeaveApply) {
    p->apply_pending = true;
    return MPPI_OK;
  }
  return launch_apply(p);
}

// The stage-level calls: mppi_planner_update, and mppi_planner_update_local with `defer_exchange` (stop after this
// rank's packet: the caller exchanges the packets and applies them)
static int launch_update(mppi_planner* p, bool prof, bool defer_exchange = false) {
  return launch_update(p, update_choose(update_held(p, prof, defer_exchange)), prof);
}

// ---- the noise: what its choice depends on (noise_plan.h), read off a handle -- the only place that does --------------
// The arguments are launch_iteration's.  The coming rollout launch is asked of the existing choices, behind
// refresh_theta_bounded: launch_iteration used to ask map_choose in front of it -- which cannot change whether a
// time-parallel kernel runs or generates its noise (map_scan does not read theta_bounded), while the pipelined, fused and
// CVaR launchers, which do depend on it, decided their noise blocks and flags behind it, inside launch_rollout.
static NoiseHeld noise_held(const mppi_planner* p, bool have_noise, bool want_next, bool prof, bool defer_exchange, bool may_leave_apply) {
  NoiseHeld h;
  memset(&h, 0, sizeof(h));
  h.rng = p->cfg.rng; h.n_local = p->n_local; h.T = p->cfg.num_steps; h.num_cus = p->num_cus; h.num_grid_samples = p->cfg.num_grid_samples;
  h.debug_flags = p->debug_flags; h.graph_on = p->graph_on; h.stream_flags_off = p->stream_flags_off;
  h.flags_env_off = noise_flag_disabled(); h.flag_words = flag_words(p);
  h.want_next = want_next; h.have_noise = have_noise;
  h.noise_on_side_stream = p->noise_on_side_stream; h.prev_signalled = p->progress_capable_last;
  switch (p->cfg.mode) {
    case MPPI_MODE_DET:
    case MPPI_MODE_SPEED_MAP: {
      const MapChoice& c = map_choice(p, map_held(p));
      const bool scan = c.family == kMapScan || c.family == kMapScanExact;
      h.launch = c.family + 1;
      h.workgroups = scan ? ceil_div(p->n_local, c.scan.tile) : c.grid;
      h.scan_exact = scan && c.scan.exact;
      break;
    }
    case MPPI_MODE_TDM: {
      const CvarChoice c = cvar_choose(cvar_held(p));
      h.launch = c.launch;
      h.workgroups = c.workgroups;
      break;
    }
    case MPPI_MODE_BAREBONE: h.launch = kLaunchBarebone; break;
  }
  UpdateHeld u = update_held(p, prof, defer_exchange, may_leave_apply);
  u.scan_packets_fresh = h.launch == kLaunchScan || h.launch == kLaunchScanExact;  // (what the coming launch leaves)
  u.want_next = 1;
  h.update_can_host = update_noise_beside(u);
  return h;
}

// The one generator on noise_stream: into the other noise buffer, held back behind that buffer's last reader as chosen,
// announced through the flag, ev_noise_ready behind it.
static int launch_noise_ahead(mppi_planner* p, const NoiseChoice& c) {
  switch (c.hold) {
    case kHoldEventBehind:  // (ordered behind the rollout launch itself)
      HIP_TRY(hipEventRecord(p->ev_buf_free, p->stream));
      [[fallthrough]];
    case kHoldEventFront: HIP_TRY(hipStreamWaitEvent(p->noise_stream, p->ev_buf_free, 0)); break;
    case kHoldGate:  // (on the start of the launch that signalled last: the rollout, or the update beside which this runs)
      hipLaunchKernelGGL(k_wait_progress, dim3(1), dim3(64), 0, p->noise_stream, p->progress_dev, p->progress_seq, p->flag_fault_dev);
      HIP_TRY(hipGetLastError());
      break;
    default: return fail(MPPI_ERR_STATE, "internal: a generator on the second stream that nothing holds back");
  }
  TraceRange tr(c.beside_update ? "mppi:noise_beside_update" : "mppi:noise_ahead");
  TRY(launch_noise(p, p->noise_buf[p->noise_cur ^ 1], p->noise_stream));
  p->used_side_stream = true;
  if (c.announce != kAnnounceNone) {
    p->noise_flag_expect = ++p->noise_flag_seq;
    if (c.announce == kAnnounceFlag) {  // (else the test hook: a generator the consumer never hears of)
      hipLaunchKernelGGL(k_set_noise_flag, dim3(1), dim3(1), 0, p->noise_stream, p->noise_flag_dev, p->noise_flag_expect);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipEventRecord(p->ev_noise_ready, p->noise_stream));
  p->noise_on_side_stream = true;
  // graph mode: join before the update, which advances the epoch counter the generator reads
  // (and a captured iteration must not leave a fork open)
  return c.join ? join_noise_ahead(p) : MPPI_OK;
}

// One iteration: {noise unless it was produced ahead, rollout (+ the next iteration's noise when
// `want_next`), update}.  `have_noise`: noise_buf[noise_cur ^ 1] already holds this iteration's
// noise; on return it says the same for the following iteration.  Where the noise comes from, who produces the next
// iteration's and how the streams are ordered around it: noise_choose (noise_plan.h).
static int launch_iteration(mppi_planner* p, const DevParams& d, bool& have_noise, bool want_next, bool prof,
                            bool defer_exchange = false, bool may_leave_apply = false) {
  const bool ktime_stamps = p->ktime_index >= 0 && p->ktime_dev && p->ktime_use_stamps;  // (mppi_planner_time_kernels)
  if (prof) HIP_TRY(hipEventRecord(p->ev_stage[0], p->stream));
  (void)refresh_theta_bounded(p);
  const NoiseChoice noise = noise_choose(noise_held(p, have_noise, want_next, prof, defer_exchange, may_leave_apply));
  if (noise.source == kNoiseInKernel) {
    if (noise.discard_ahead) discard_noise_ahead(p);
  } else if (noise.source == kNoiseAhead) {
    p->noise_cur ^= 1;
    // (ordered behind the generator by the rollout launch itself: its flag, or the event -- settle_noise_wait)
    p->noise_wait_pending = noise.consumer != kOrderNone;
    p->noise_on_side_stream = false;
    p->noise_virtual = false;
  } else {
    TraceRange tr("mppi:noise");
    p->noise_virtual = false;
    TRY(launch_noise(p, p->noise_buf[p->noise_cur]));
  }
  p->noise = p->noise_buf[p->noise_cur];
  // Acceleration limits: this iteration's block is there (a block produced ahead once the main stream has waited for its
  // generator, as the rollout launch would have), and so is the u the previous update left -- which is why the pass is
  // in line, behind both, and the generator ahead keeps producing unlimited blocks.
  if (control_limits_on(p)) {
    TraceRange tr("mppi:noise_limit");
    settle_noise_wait(p);
    TRY(launch_noise_limit(p, p->noise));
  }
  if (prof) HIP_TRY(hipEventRecord(p->ev_stage[1], p->stream));
  // (the other noise buffer was last read by the previous update, which is behind us on this stream)
  if (noise.record_front) HIP_TRY(hipEventRecord(p->ev_buf_free, p->stream));
  {
    TraceRange tr("mppi:rollout");
    // mppi_planner_time_kernels.  A loop with the second stream in it is timed by the kernels themselves (device
    // stamps, no event anywhere near the launches -- see there); every other loop by start / stop events on the launches.
    if (ktime_stamps) {
      p->ktime_markers = true;
      p->ktime_rollout_slot = p->ktime_dev + 4 * (size_t)p->ktime_waves * (size_t)p->ktime_index;
    } else if (p->ktime_index >= 0) {
      p->kev_start = p->ktime_events[4 * (size_t)p->ktime_index];
      p->kev_stop = p->ktime_events[4 * (size_t)p->ktime_index + 1];
    }
    p->noise_now = noise;
    const int rc = launch_rollout(p, d);
    p->noise_now = NoiseChoice();
    p->kev_start = p->kev_stop = nullptr;
    p->ktime_rollout_slot = nullptr;
    settle_noise_wait(p);  // (a path that launched nothing: whatever follows on the stream still needs the noise)
    TRY(rc);
  }
  if (p->m_count > 1) {
    TraceRange tr("mppi:exchange_sample_costs");
    TRY(exchange_sample_costs(p));
  }
  if (noise.beside_rollout) TRY(launch_noise_ahead(p, noise));
  p->progress_capable_last = noise.signals;
  // How this iteration's weights become the next u (update_plan.h), decided from what the rollout launch has left.
  // beside_update: the next iteration's noise is generated beside the update launch -- which runs slim
  // (k_update_rows<.., 256>: a quarter of the waves, the same bytes in flight) and signals its start to the generator's
  // gate kernel.  (MPPI_NO_NOISE_FLAG: no flags, no second stream here)
  UpdateHeld held = update_held(p, prof, defer_exchange, may_leave_apply);
  held.want_next = want_next && noise.source != kNoiseInKernel; held.have_noise = noise.have_after_rollout;
  held.side_stream_pays = noise.side_stream_pays;
  const UpdateChoice update = update_choose(held);
  REQUIRE(update.beside_update == (noise.beside_update != 0), MPPI_ERR_STATE, "internal: the update launch and the noise choice disagree on the generator beside the update");
  if (update.beside_update) ++p->progress_seq;
  if (prof) HIP_TRY(hipEventRecord(p->ev_stage[2], p->stream));
  TraceRange tr_update("mppi:update");
  const int ktime_slot = p->ktime_index;
  if (p->ktime_index >= 0) {
    if (ktime_stamps) {
      p->ktime_update_slot = p->ktime_dev + 4 * (size_t)p->ktime_waves * (size_t)p->ktime_index + 2 * (size_t)p->ktime_waves;
    } else {
      p->kev_start = p->ktime_events[4 * (size_t)p->ktime_index + 2];
      p->kev_stop = p->ktime_events[4 * (size_t)p->ktime_index + 3];
    }
    ++p->ktime_index;
  }
  {
    const int rc = launch_update(p, update, prof);
    p->kev_start = p->kev_stop = nullptr;
    p->ktime_update_slot = nullptr;
    TRY(rc);
    if (noise.beside_update) TRY(launch_noise_ahead(p, noise));  // gated on this update launch's start
    // (an update left to the next rollout launch has no launch of its own to time)
    if (ktime_slot >= 0 && (size_t)ktime_slot < p->ktime_update_ran.size()) p->ktime_update_ran[(size_t)ktime_slot] = !p->reduce_pending;
  }
  have_noise = noise.have_noise;
  if (prof) HIP_TRY(hipEventRecord(p->ev_stage[5], p->stream));
  return MPPI_OK;
}

// Everything the launches of an iteration take by value or derive on the host: a captured graph
// may be replayed only while none of it has changed.
static void graph_signature(const mppi_planner* p, const DevParams& d, std::vector<unsigned char>& out) {
  struct Sig {
    DevParams d;
    mppi_params params;
    const void *cells, *cells16, *cc, *sample_costs, *u;
    uint64_t lin_maps, lin_grid, ang_maps, ang_grid, epoch_bias, wall_gen, wtrk_gen, gtrk_gen, fleet_gen, smp_gen, fp_gen, ring_gen, guide_gen, occ_gen;
    int noise_cur, inst_set, want_sample_costs, speculation_off, debug_flags, pad;
    float smooth_beta[2];
    float limit_steps[2];
    int limits_held, pad2;
  } sig;
  memset(&sig, 0, sizeof(sig));
  sig.d = d;
  sig.params = p->params;
  if (p->inst_set) {  // batched handle: start and goal are read from device memory, not from arguments
    sig.d.x0 = sig.d.y0 = sig.d.th0 = sig.d.xg = sig.d.yg = 0.0f;
    memset(sig.params.x0, 0, sizeof(sig.params.x0));
    memset(sig.params.xgoal, 0, sizeof(sig.params.xgoal));
  }
  sig.cells = p->cells; sig.cells16 = p->cells16; sig.cc = p->cc_scratch;
  sig.sample_costs = p->sample_costs; sig.u = p->u;
  sig.lin_maps = p->packed.lin_maps; sig.lin_grid = p->packed.lin_grid;
  sig.ang_maps = p->packed.ang_maps; sig.ang_grid = p->packed.ang_grid;
  sig.epoch_bias = p->noise_epoch - p->bumps_launched;
  const BareboneScene& sc = p->scene;
  sig.wall_gen = sc.walls.gen;  // (the walls' generation, not their address: a new set may land where the old one was)
  sig.wtrk_gen = sc.wall_tracks.gen;
  sig.gtrk_gen = sc.goal.gen;  // (the goal track's likewise)
  sig.fleet_gen = sc.fleet.gen;  // (the fleet storage's: renewed when it is rebuilt, not when its rows are refreshed)
  sig.smp_gen = sc.samples.gen;  // (the disc samples')
  sig.fp_gen = sc.footprint.gen;  // (the body footprint's: its rows are a by-value argument of the captured launches)
  sig.ring_gen = sc.rings.gen;  // (the clearance rings' likewise)
  sig.guide_gen = sc.guide.gen;  // (the guide's: renewed when it is set, not when its field or its rows are refreshed)
  sig.occ_gen = sc.occupancy.gen;  // (the occupancy grid's: renewed with its shape, geometry, inflate or substeps, not with its cells)
  sig.smooth_beta[0] = p->smooth_beta[0]; sig.smooth_beta[1] = p->smooth_beta[1];  // (the noise smoothing's coefficients: by value in the generator's argument)
  control_limit_steps(p, sig.limit_steps);  // (the acceleration limits: the steps, on or off, and -- in params -- the box: by value)
  sig.limits_held = p->limits_held ? 1 : 0;
  sig.noise_cur = p->noise_cur; sig.inst_set = p->inst_set; sig.want_sample_costs = p->want_sample_costs;
  sig.speculation_off = p->speculation_off ? 1 : 0; sig.debug_flags = p->debug_flags;
  sig.pad = (p->p2p_on ? 2 : 0) | (p->p2p_index & 1);  // (the inbox set of the peer exchange is a by-value argument)
  out.assign(reinterpret_cast<unsigned char*>(&sig), reinterpret_cast<unsigned char*>(&sig) + sizeof(sig));
}

// `timed`: bracket the iterations with events for mppi_planner_last_elapsed_ms / stage_times
// (iterate_async, profiling); solve() on the control path skips them
// called where the host has just waited for the stream: did speculation pay on this map?
static void review_speculation(mppi_planner* p) {
  if (!p->spec_fail_host) return;
  if (p->spec_launches == 0) {  // (nothing speculative ran: whatever the word holds is stale)
    *p->spec_fail_host = 0u;
    return;
  }
  const uint64_t failed = *p->spec_fail_host;
  // A launch lasts as long as its slowest tile, and a tile whose vote fails is rolled out twice: ONE failing tile
  // makes its launch slower than the exact schedule would have been.  Every speculative kernel runs ONE round of
  // workgroups (k_rollout_scan*: a tile per CU; the speculative pipelines of rounds 2-5 likewise: up to three tiles in
  // one workgroup per CU), so the criterion is per launch for all of them.  C2 shape, round 5: 15.2 us when every
  // vote holds, 21.6 us on the exact schedule (direct), ~40 us with a failing tile -- speculation pays while
  // P(fail) * (40 - 21.6) < (1 - P) * (21.6 - 15.2), i.e. fewer than one launch in four fails (the longer horizons'
  // speculative against exact pipeline then: 36 / 48 / 85 us, the same quarter).  The kernels count failed tiles: at
  // least one per four launches -> stop.
  if (4 * failed >= p->spec_launches) {
    p->speculation_off = true;
    // Several GPUs on the peer exchange: which tiles fail their vote differs from rank to rank (every rank rolls out
    // its own noise), so ranks reach this point in different iterations -- and the exchange only works while all of
    // them launch kernels that carry it.  Stopping is therefore allowed where the kernel FAMILY survives it
    // (k_rollout_scan_exact on its exact schedule: ScanPlan::direct -- same packets, same exchange, whatever the
    // other ranks run); where it would mean another family (window too large, tolerance kernel) this rank keeps
    // speculating: slower on such a map, never a rank that has left the exchange its peers still wait in.
    if (p->p2p_on && p->cfg.world_size > 1 && !scan_plan(p, nullptr)) p->speculation_off = false;
  }
  *p->spec_fail_host = 0u;
  p->spec_launches = 0;
}

// `part_of_group_loop` (mppi_group_iterate_async's round robin over devices): this call is one turn of a longer loop
// on this handle -- `more_follow`: further turns come, so the last iteration of this one may leave its update to the
// next turn's first rollout launch like any other iteration -- and the loop's events belong to the caller.
static int run_iterations(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, int iterations, bool timed = true,
                          bool mirror_last = false, bool part_of_group_loop = false, bool more_follow = false) {
  REQUIRE(p->params_set, MPPI_ERR_STATE, "params not set");
  DevParams d;
  TRY(prepare_launch(p, lin, ang, &d));
  p->iterations_since_wait += iterations;
  timed = (timed || p->profile_stages) && !part_of_group_loop;
  if (timed) HIP_TRY(hipEventRecord(p->ev_begin, p->stream));
  // The noise of iteration k+1 does not depend on iteration k.  When the pipelined rollout
  // kernel runs, its spare workgroups generate it into the other half of the double buffer
  // (same launch, no extra dependency); otherwise it is generated in line.
  // (a sharded handle replays too: RCCL's all-gather is captured into the graph with the kernels;
  //  without a communicator the exchange is host-staged and cannot be captured)
  const bool use_graph = p->graph_on && !p->profile_stages && (p->cfg.world_size == 1 || p->comm);
  if (!use_graph) {
    // Every iteration, the last one of a call included, asks for its successor's noise: when the
    // rollout kernel can produce it on the side (spare workgroups, second stream) the next call --
    // the next control step -- starts with its noise already there (`primed`).
    bool have_noise = p->primed;
    for (int k = 0; k < iterations; ++k) {
      // profiled iteration: a steady-state one when there is one, else the last
      bool prof = p->profile_stages && !part_of_group_loop && k == (iterations >= 3 ? iterations - 2 : iterations - 1);
      p->mirror_now = mirror_last && k == iterations - 1;
      const int rc = launch_iteration(p, d, have_noise, true, prof, false, k + 1 < iterations || more_follow);
      p->mirror_now = false;
      TRY(rc);
    }
    p->primed = have_noise;
  } else {
    // Graph mode.  Every iteration also asks for the noise of its successor (`primed`; kernels that
    // cannot produce it ahead generate in line instead), so that all iterations look alike; two of
    // them bring the noise double buffer back to where it was and are what gets captured.
    // Host-side effects of a launch (which kernel, window plan, instance upload, lazy allocations)
    // happen in the direct iteration that precedes any capture.
    bool have_noise = p->primed;
    int k = 0;
    if (p->inst_set && p->inst_dirty) {  // batched handle: new start states -> window origins, upload
      size_t unused = 0;
      DevParams plan = d;
      (void)plan_lds_window(p, plan, &unused);
      TRY(upload_instances(p));
    }
    // (a rollout kernel that computes its own noise has nothing to prime: its iterations are alike from the start)
    if (((!have_noise && !scan_generates_noise(p)) || !p->graph_warm) && k < iterations) {
      TRY(launch_iteration(p, d, have_noise, true, false));
      p->graph_warm = true;
      ++k;
    }
    const int chunk = p->graph_chunk;  // iterations per graph: even (noise double buffer)
    while (iterations - k >= chunk) {
      std::vector<unsigned char> sig;
      graph_signature(p, d, sig);
      sig.push_back(have_noise ? 1 : 0);
      const int slot = (p->noise_cur & 1) | ((p->u_parity & 1) << 1) | ((p->tpk_cur & 1) << 2);
      if (!p->graph_exec[slot] || sig != p->graph_sig[slot]) {
        if (p->graph_exec[slot]) { (void)hipGraphExecDestroy(p->graph_exec[slot]); p->graph_exec[slot] = nullptr; }
        if (p->graph[slot]) { (void)hipGraphDestroy(p->graph[slot]); p->graph[slot] = nullptr; }
        p->graph_sig[slot].clear();
        const bool primed_before = have_noise;
        const uint64_t spec_before = p->spec_launches;
        const int u_parity_before = p->u_parity, tpk_before = p->tpk_cur;
        HIP_TRY(hipStreamBeginCapture(p->stream, hipStreamCaptureModeThreadLocal));
        int rc = MPPI_OK;
        // (the last iteration of a graph applies its update itself: a graph starts and ends with nothing pending)
        for (int j = 0; j < chunk && rc == MPPI_OK; ++j)
          rc = launch_iteration(p, d, have_noise, true, false, false, j + 1 < chunk);
        hipError_t end = hipStreamEndCapture(p->stream, &p->graph[slot]);
        if (rc != MPPI_OK) return rc;
        HIP_TRY(end);
        REQUIRE(have_noise == primed_before, MPPI_ERR_STATE, "graph capture: the iterations are not alike");
        HIP_TRY(hipGraphInstantiate(&p->graph_exec[slot], p->graph[slot], nullptr, nullptr, 0));
        p->graph_sig[slot] = sig;
        p->graph_spec_launches[slot] = p->spec_launches - spec_before;
        // (one GPU, updates applied inside rollout launches: all but the last iteration of the graph change control
        //  buffers -- an odd number when the graph holds an even number of iterations)
        p->graph_u_flip[slot] = (p->u_parity ^ u_parity_before) & 1;
        p->graph_tpk_flip[slot] = (p->tpk_cur ^ tpk_before) & 1;
        ++p->graph_captures;
        // (capturing ran the host side of two iterations; the launch below runs their device side)
      } else {
        // the host-side counters a direct launch of the two iterations would have advanced
        if (p->cfg.rng == MPPI_RNG_PHILOX) p->noise_epoch += (uint64_t)chunk;
        p->bumps_launched += (uint64_t)chunk;
        // (the replayed kernels count their failed tiles like the captured ones did)
        p->spec_launches += p->graph_spec_launches[slot];
        if (p->graph_u_flip[slot]) {
          std::swap(p->u, p->u_alt);
          p->u_parity ^= 1;
        }
        p->tpk_cur ^= p->graph_tpk_flip[slot];
      }
      HIP_TRY(hipGraphLaunch(p->graph_exec[slot], p->stream));
      ++p->graph_replays;
      k += chunk;
    }
    for (; k < iterations; ++k) TRY(launch_iteration(p, d, have_noise, true, false, false, k + 1 < iterations));
    p->primed = have_noise;
  }
  if (timed) {
    HIP_TRY(hipEventRecord(p->ev_end, p->stream));
    p->elapsed_pending = true;
    p->last_iterations = iterations;
  }
  return MPPI_OK;
}

static int finish_timing(mppi_planner* p) {
  if (!p->elapsed_pending) return MPPI_OK;
  HIP_TRY(hipEventSynchronize(p->ev_end));
  HIP_TRY(hipEventElapsedTime(&p->last_elapsed_ms, p->ev_begin, p->ev_end));
  if (p->profile_stages && p->last_iterations > 0) {
    // ev_stage: 0 noise | 1 rollout | 2 update-local | 3 collective | 4 apply .. ev_end
    float noise, roll, upd, coll, tail;
    HIP_TRY(hipEventElapsedTime(&noise, p->ev_stage[0], p->ev_stage[1]));
    HIP_TRY(hipEventElapsedTime(&roll, p->ev_stage[1], p->ev_stage[2]));
    HIP_TRY(hipEventElapsedTime(&upd, p->ev_stage[2], p->ev_stage[3]));
    HIP_TRY(hipEventElapsedTime(&coll, p->ev_stage[3], p->ev_stage[4]));
    HIP_TRY(hipEventElapsedTime(&tail, p->ev_stage[4], p->ev_stage[5]));
    p->stage_ms[0] = noise;
    p->stage_ms[1] = roll;
    p->stage_ms[2] = upd + tail;
    p->stage_ms[3] = coll;
  }
  p->elapsed_pending = false;
  return MPPI_OK;
}

// grids are sampled once per solve(), not per optimisation iteration
// (mppi.py:247-248, 321-322, 391-394); the deterministic modes pass alpha_dyn = 1
static int sample_for_solve(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang) {
  if (p->cfg.mode == MPPI_MODE_BAREBONE) return MPPI_OK;
  TraceRange tr("mppi:sample_grids");
  double alpha = (p->cfg.mode == MPPI_MODE_TDM) ? p->params.alpha_dyn : 1.0;
  const CellsChoice c = cells_choose(cells_held(p, lin, ang, true, alpha));
  if (c.route == kCellsSample) return sample_into_cells(p, lin, ang, alpha, c);
  TRY(tdm_sample_on(lin, alpha, p->stream));
  TRY(tdm_sample_on(ang, alpha, p->stream));
  return MPPI_OK;
}
