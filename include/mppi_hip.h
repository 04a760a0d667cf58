/*
 * mppi_hip.h -- C ABI of libmppi_hip.so, the MI355X (gfx950) MPPI rollout engine.
 *
 * The reference (mit-acl/mppi_numba) has no FFI: its device boundary is the
 * set of numba calls made by mppi_numba/mppi.py, terrain.py and config.py
 * (cuda.device_array / cuda.to_device / copy_to_host / kernel[grid, block](...)).
 * Each entry point below replaces one such group of calls; the reference
 * file:line it stands in for is given next to it (paths relative to
 * /root/reference/mppi_numba).  The Python host code binds this header with
 * ctypes (mppi_numba_amd/_lib.py); INTEGRATION.md shows the binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 (MPPI_OK) or a negative mppi_status; the text of
 *     the last failure on the calling thread is mppi_last_error();
 *   - handles are opaque and not thread-safe; one host thread drives a handle,
 *     as in the reference (single Python thread, default stream);
 *   - host arrays are owned by the caller, device memory by the library;
 *   - every call is synchronous from the caller's point of view unless its
 *     name ends in _async;
 *   - host-side array layouts are the reference's: noise (N,T,2) f32, u (T,2)
 *     f32, costs/weights (N) f32, sampled grids (G,R,C) int8, maps (Rp,Cp) int8,
 *     pmf (B,Rp,Cp) int8, state rollouts (V,T+1,3) f32, all C-contiguous.
 *     Device-side layouts are private to the library.
 */
#ifndef MPPI_HIP_H
#define MPPI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPPI_HIP_ABI_VERSION 2

typedef enum mppi_status {
  MPPI_OK = 0,
  MPPI_ERR_INVALID = -1,   /* bad argument / shape mismatch                   */
  MPPI_ERR_HIP = -2,       /* a HIP runtime call failed                        */
  MPPI_ERR_STATE = -3,     /* call sequence error (maps or params not set ...) */
  MPPI_ERR_NO_DEVICE = -4, /* no usable gfx950 device                          */
  MPPI_ERR_COMM = -5,      /* RCCL failure, or a peer of the peer exchange that did not deliver */
  MPPI_ERR_BUSY = -6       /* the device did not run all workgroups of a rollout launch side by side (another tenant, a
                              CU mask): the controls handed over inside that launch did not arrive in time; the control
                              sequence of the call is not valid, later calls update through a launch of their own */
} mppi_status;

/* which of the reference's solve_* variants the planner runs (mppi.py:193-211) */
typedef enum mppi_mode {
  MPPI_MODE_DET = 0,       /* use_det_dynamics                 mppi.py:308-375 */
  MPPI_MODE_SPEED_MAP = 1, /* use_nom_dynamics_with_speed_map  mppi.py:237-305 */
  MPPI_MODE_TDM = 2,       /* use_tdm (CVaR over M samples)    mppi.py:376-531 */
  MPPI_MODE_BAREBONE = 3   /* barebone_mppi_numba.ipynb: no maps, disc obstacles */
} mppi_mode;

typedef enum mppi_rng_kind {
  MPPI_RNG_PHILOX = 0,    /* rocRAND Philox4x32-10, counter keyed by the GLOBAL
                             (rollout, step) index: results do not depend on the
                             number of GPUs                                     */
  MPPI_RNG_XOROSHIRO = 1  /* bit-compatible with numba.cuda.random
                             (xoroshiro128+, stream per thread) for seed -> u
                             known-answer tests against the reference           */
} mppi_rng_kind;

typedef enum mppi_math_kind {
  MPPI_MATH_EXACT = 0, /* float64 trig/sqrt where the reference's CPU path has
                          float64: costs bit-identical to it (default)          */
  MPPI_MATH_FAST = 1   /* float32 sincosf/sqrtf in the general kernel: ~1 ulp cost
                          differences.  For numerical comparison; NOT faster -- the
                          pipelined / fused kernels exist for the exact path only */
} mppi_math_kind;

const char* mppi_last_error(void);
int mppi_abi_version(void);

/* ---- device query: replaces the import-time query of config.py:9-12 ------- */
typedef struct mppi_device_props {
  int max_threads_per_block;
  int max_block_dim_x;
  int max_grid_dim_x;
  int wavefront_size;
  int compute_units;
  int lds_bytes_per_cu;
  char gcn_arch[64];
  char name[128];
} mppi_device_props;

int mppi_device_count(int* count);
int mppi_device_props_get(int device, mppi_device_props* out);

/* ---- traction distribution map (TDM_Numba) -------------------------------- */
typedef struct mppi_tdm mppi_tdm;

typedef struct mppi_tdm_cfg {
  int device;
  int num_grids;        /* M for use_tdm, 1 for the deterministic modes
                           (terrain.py:171-177)                                 */
  int max_rows;         /* cfg.max_map_dim: allocation of sample_grid_batch     */
  int max_cols;
  int thread_dim_x;     /* cfg.tdm_sample_thread_dim (only shapes the xoroshiro
                           compatible stream->cell mapping, terrain.py:645-668) */
  int thread_dim_y;
  int rng;              /* mppi_rng_kind */
  int _reserved;
  uint64_t seed;
} mppi_tdm_cfg;

/* terrain.py:164-180 init_device_vars_before_sampling */
int mppi_tdm_create(const mppi_tdm_cfg* cfg, mppi_tdm** out);
int mppi_tdm_destroy(mppi_tdm* tdm);

/* terrain.py:331-333,370-371,405-406,495,506: upload of the padded PMF grid,
 * masks and (speed-map mode) padded risk traction map.  bin_to_int8[b] is
 * np.int8(100.*(bin_values[b]-lo)/(hi-lo)) (terrain.py:689) evaluated by the
 * host in the dtypes the reference would hold; traction_lo / traction_ratio are
 * bin_values_bounds[0] and 0.01*(bounds[1]-bounds[0]) (mppi.py:674-675).
 * risk may be NULL. */
int mppi_tdm_set_maps(mppi_tdm* tdm, const int8_t* pmf, int bins, int rows, int cols,
                      const int8_t* bin_to_int8, double traction_lo, double traction_ratio,
                      const int8_t* obstacle, const int8_t* unknown, const int8_t* risk);

/* Map preprocessing on the device (replaces the numpy code of
 * terrain.py:408-495 and the padding of terrain.py:511-583): the RAW PMF grid
 * (bins, src_rows, src_cols) and masks (src_rows, src_cols; NULL = zeros) in, on the
 * device: crop to (valid_rows, valid_cols) from the origin, ring of pad_cells
 * zero-traction cells, and per kind
 *   MPPI_PREP_TDM    the PMF itself                             (use_tdm)
 *   MPPI_PREP_DET    one-hot PMF at the CVaR_alpha bin          (use_det_dynamics)
 *   MPPI_PREP_SPEED  nominal PMF + int8 risk traction map       (use_nom_dynamics_with_speed_map)
 * bin_values / bounds are the float32 copies the reference holds (terrain.py:393-394);
 * the remaining arguments are those of mppi_tdm_set_maps.  *bad_columns (may be NULL)
 * receives the number of raw PMF columns that do not sum to 100.  Bit-identical to the
 * host path. */
typedef enum mppi_prep_kind { MPPI_PREP_TDM = 0, MPPI_PREP_DET = 1, MPPI_PREP_SPEED = 2 } mppi_prep_kind;
int mppi_tdm_set_maps_from_pmf(mppi_tdm* tdm, int kind, const int8_t* pmf, int bins, int src_rows,
                               int src_cols, int valid_rows, int valid_cols, int pad_cells,
                               const float* bin_values, const float bounds[2], double alpha,
                               const int8_t* bin_to_int8, double traction_lo, double traction_ratio,
                               const int8_t* obstacle, const int8_t* unknown, int* bad_columns);
/* the maps as held on the device; any pointer may be NULL.  pmf (bins, rows, cols),
 * obstacle / unknown / risk (rows, cols) with rows, cols the PADDED size */
int mppi_tdm_get_maps(mppi_tdm* tdm, int8_t* pmf, int8_t* obstacle, int8_t* unknown, int8_t* risk);

/* terrain.py:610-622 sample_grids (kernel terrain.py:633-695) */
int mppi_tdm_sample_grids(mppi_tdm* tdm, double alpha_dyn);

/* test/visualisation access to sample_grid_batch_d, host layout
 * (num_grids, max_rows, max_cols); set writes the [:, :rows, :cols] window */
int mppi_tdm_set_sampled_grids(mppi_tdm* tdm, const int8_t* grids, int rows, int cols);
int mppi_tdm_get_sampled_grids(mppi_tdm* tdm, int8_t* out);

/* xoroshiro-compatible generator only: copy the (streams, 2) uint64 states */
int mppi_tdm_rng_states(mppi_tdm* tdm, uint64_t* out, long capacity, long* count);

/* ---- planner (MPPI_Numba) -------------------------------------------------- */
typedef struct mppi_planner mppi_planner;

typedef struct mppi_planner_cfg {
  int device;
  int mode;                   /* mppi_mode */
  int num_control_rollouts;   /* N over ALL ranks                               */
  int num_steps;              /* T = int(cfg.T / cfg.dt)                        */
  int num_grid_samples;       /* M (1 unless MPPI_MODE_TDM)                     */
  int num_vis_state_rollouts; /* V                                              */
  int rng;                    /* mppi_rng_kind                                  */
  int math;                   /* mppi_math_kind                                 */
  int rank;                   /* this handle owns rollouts
                                 [rank*N/world, (rank+1)*N/world)               */
  int world_size;
  int num_instances;          /* batched multi-query extension (below): B
                                 problems in one handle; 0 or 1 = one problem   */
  uint64_t seed;
} mppi_planner_cfg;

/* mppi.py:214-234 move_mppi_task_vars_to_device: one struct instead of nine
 * to_device calls.  Fields the reference casts to np.float32 are float. */
typedef struct mppi_params {
  float x0[3];
  float xgoal[2];
  float vrange[2];
  float wrange[2];
  float u_std[2];
  float dt;
  float goal_tolerance;
  float v_post_rollout;
  float lambda_weight;
  float cvar_alpha;
  float obs_cost;
  float unknown_cost;
  float res;          /* lin_tdm.res                                  */
  float xlo;          /* float32(lin_tdm.padded_xlimits[0])           */
  float ylo;          /* float32(lin_tdm.padded_ylimits[0])           */
  double dist_weight; /* passed to the kernels as a Python number     */
  double alpha_dyn;   /* params['alpha_dyn'] (use_tdm), else 1.0      */
  int num_opt;
  int _reserved;
} mppi_params;

/* mppi.py:108-127 init_device_vars_before_solving */
int mppi_planner_create(const mppi_planner_cfg* cfg, mppi_planner** out);
int mppi_planner_destroy(mppi_planner* p);

int mppi_planner_set_params(mppi_planner* p, const mppi_params* params);

/* barebone notebook: params['obstacle_positions'] (K,2), ['obstacle_radius'] (K) */
int mppi_planner_set_disc_obstacles(mppi_planner* p, const float* positions, const float* radii,
                                    int count);

/* ---- batched multi-query (not in the reference; BASELINE.json configs[4]) ------
 * One handle solves B = cfg.num_instances independent MPPI problems per launch.
 * They share the maps and every field of mppi_params except the start state and
 * the goal; each has its own N = num_control_rollouts samples, control sequence,
 * minimum cost and normaliser.  Instance b is bit-identical to a single-instance
 * handle given the same noise.  Array shapes with B > 1: u (B,T,2), costs and
 * weights (B,N_local), noise (B*N_local,T,2), packets B*(2T+2) doubles per rank.
 * Needs N/world_size to be a multiple of 64.  MPPI_MODE_BAREBONE: the problems share the disc set
 * of mppi_planner_set_disc_obstacles, or each has its own (below); world_size must be 1.
 * x0: (count,3) float32, xgoal: (count,2) float32; count must equal B.  A handle with B = 1
 * also takes count = 0 (x0, xgoal ignored): back to the start / goal of mppi_params. */
int mppi_planner_set_instances(mppi_planner* p, int count, const float* x0, const float* xgoal);

/* MPPI_MODE_BAREBONE only: one disc set per problem.  count must equal B; disc_counts [B] >= 0,
 * positions (sum of the counts, 2) float32 and radii (sum) float32, problem b's discs following
 * problem b-1's.  Problem b's costs are bit-identical to a single-problem handle given its discs
 * (in the same order) through mppi_planner_set_disc_obstacles.  count = 0: every problem back to
 * the shared set.  Unchanged arrays cost a comparison and no synchronisation; a change drops the
 * captured graphs.  MPPI_ERR_INVALID for a map mode, a negative count, count not 0 and not B, or
 * a largest set whose discs and the T control ratios need more than 64 KiB of LDS (16*T + 16*K). */
int mppi_planner_set_instance_disc_obstacles(mppi_planner* p, int count, const int* disc_counts,
                                             const float* positions, const float* radii);

/* MPPI_MODE_BAREBONE only: discs that move.  A track is `rows` >= 1 predicted centres of a disc,
 * row j its centre at time j*dt from "now"; tracks is (sum of the counts, rows, 2) float32, radii
 * (sum) float32.  count = 1: disc_counts[0] discs shared by every problem; count = B: one set per
 * problem, laid out as for mppi_planner_set_instance_disc_obstacles.  Each problem has a track
 * offset s >= 0 ("now" is row s; below).  In a rollout the state after step t (t = 0 .. T-1) is
 * tested against row min(s + t + 1, rows - 1) of every disc of its problem: the disc where it will
 * be when the robot gets there, at its last predicted place once the track has ended.  The test,
 * the cost and their roundings are those of the static discs, so tracks whose rows are all equal
 * give the bits of the static set.  While tracks are set they take the place of both static sets;
 * count = 0 (or disc_counts NULL) clears them and the static sets apply again.  Unchanged arrays
 * cost a comparison; a change drops the captured graphs and sets every offset to 0.
 * MPPI_ERR_INVALID for a map mode, rows < 1, a negative count, count not 0 / 1 / B, or a largest
 * set that needs more than 64 KiB of LDS (16*T + 16*T*K bytes). */
int mppi_planner_set_disc_tracks(mppi_planner* p, int count, const int* disc_counts, int rows,
                                 const float* tracks, const float* radii);
/* offsets [B] int >= 0, count must equal B.  An offset travels with its problem's start state (no
 * synchronisation; graph replay needs no new capture for it on a handle with instances set).
 * mppi_planner_closed_loop advances the offset of every problem that is still running by one per
 * control step, on the device; afterwards get returns offset_before + steps_taken[b]. */
int mppi_planner_set_track_offsets(mppi_planner* p, int count, const int* offsets);
int mppi_planner_get_track_offsets(mppi_planner* p, int count, int* offsets);

/* MPPI_MODE_BAREBONE only (any other mode: MPPI_ERR_INVALID): crowd mode, off by default.  While it
 * is on, the three disc hand-overs above and the launch take any disc count that device memory
 * holds -- the 64 KiB limits do not apply -- and the rollout of a set with kCrowdMinDiscs discs or
 * more (launch_plan.h) runs k_rollout_barebone_crowd, which reads the discs from memory, counts the
 * hits of every step in parallel over the horizon and then adds obs_cost once per hit: the bits
 * of the default forms.  Everything else is unchanged.  Turning it off while the handle holds a
 * set the default forms cannot launch returns MPPI_ERR_INVALID (the message names the set) and
 * the handle stays in crowd mode with what it had.  A change drops the captured graphs. */
int mppi_planner_set_crowd(mppi_planner* p, int on);
int mppi_planner_get_crowd(mppi_planner* p, int* on);

/* MPPI_MODE_BAREBONE in crowd mode only: disc samples -- S sampled futures of K moving discs, as a
 * predictor of pedestrians hands them out.  positions is (samples, disc_count, rows, 2) float32:
 * sample s is a track set as for mppi_planner_set_disc_tracks (rows are instants, "now" is the
 * problem's track offset, the state after step t meets row min(offset + t + 1, rows - 1)); radii
 * (disc_count) float32, finite and >= 0.  The cost of a rollout under sample s is, bit for bit, the
 * cost of the crowd launch with that sample as its disc tracks; walls, wall tracks, the fleet's
 * walls and a goal track stay in force and do not depend on s.  The rollout's cost is the CVaR tail
 * over its S costs (mppi_params::cvar_alpha, 0 < alpha <= 1; the reference's mppi.py:716-755 with
 * block_width = S): sorted descending iff alpha < 1, the strided float32 tree over the first
 * numel = ceil(S * alpha) entries, divided in double.  S = 1 is the plain track set to the bit.
 * While held the samples are the disc source of every launch (the tracks' place: the shared static
 * set rests) and every problem of a batched handle sees the same set; they count as disc tracks
 * wherever rows are counted (mppi_planner_closed_loop advances "now").  samples = 0 clears.
 * Unchanged input costs a comparison; a change drops the captured graphs and, for a set of more
 * than one row, sets every offset to 0.  mppi_planner_describe_last_rollout ends in
 * " samples=<S> numel=<n>".  MPPI_ERR_INVALID for a map mode, crowd mode off, samples outside
 * [0, 16] (kCrowdSamplesMax), rows < 1, disc_count + walls > 65535 (a step's hits are counted in
 * 16 bits), a radius that is negative or not finite, or per-problem disc sets / disc tracks held.
 * While samples are held, mppi_planner_set_disc_tracks and
 * mppi_planner_set_instance_disc_obstacles with a count, and mppi_planner_set_crowd(p, 0), are
 * refused (MPPI_ERR_INVALID): one owner of the disc source. */
int mppi_planner_set_disc_track_samples(mppi_planner* p, int samples, int disc_count, int rows,
                                        const float* positions, const float* radii);

/* MPPI_MODE_BAREBONE in crowd mode only: wall obstacles.  A wall is a segment A -> B with a
 * half-width h >= 0; segments is (count, 4) float32 -- ax ay bx by -- and halfwidths (count)
 * float32.  Step t of a rollout (t = 0 .. T-1) moves the robot from P (the position before the
 * step, the start state for t = 0) to Q; it hits the wall iff the distance between the closed
 * segments PQ and AB is <= h, so a step that jumps a thin wall is a hit.  Every wall hit counts
 * like a disc hit of that step: obs_cost once more, nothing after the freeze at the goal; walls do
 * not stop a rollout, and a position inside a wall is counted at the step that ends there and at
 * the step that starts there.  The test is division-free and runs in double on the widened
 * float32 inputs (rollout_crowd_kernel.h, crowd_wall_hit; tests/wall_model.py is its numpy form).
 * These walls are static and shared by every problem of a batched handle (walls that move and
 * per-problem sets: mppi_planner_set_wall_tracks below).  A handle that holds walls launches
 * k_rollout_barebone_crowd's WALLS form whatever its disc count (mppi_planner_describe_last_rollout
 * ends in " walls=<count>"), and mppi_planner_set_crowd(p, 0) returns MPPI_ERR_INVALID until they
 * are cleared.  count = 0 clears them (segments, halfwidths ignored).  Unchanged arrays cost a
 * comparison; a change drops the captured graphs.  MPPI_ERR_INVALID for a map mode, a handle that
 * is not in crowd mode, a negative or non-finite half-width, or a non-finite endpoint. */
int mppi_planner_set_walls(mppi_planner* p, const float* segments, const float* halfwidths, int count);

/* MPPI_MODE_BAREBONE in crowd mode only: walls that move, and a wall set per problem.  count = 1:
 * one set for every problem; count = B: one per problem, wall_counts[b] >= 0 walls each; the sets
 * lie one after the other in problem order, segments (sum W_b, rows, 4) float32 -- ax ay bx by --
 * and halfwidths (sum W_b) float32, static per wall.  Row j of a wall is the segment it occupies
 * during control interval j, from j*dt to (j+1)*dt after "now".  Step t of a rollout is interval
 * s + t -- s: the problem's track offset (mppi_planner_set_track_offsets; one "now" per problem,
 * shared with the disc tracks) -- and is tested as mppi_planner_set_walls describes against row
 * min(s + t, rows - 1) of every wall of its problem.  (A disc row is an instant: the post-step
 * position meets row s + t + 1.  Each kind clamps against its own row count.)  rows = 1, or equal
 * rows, is a static wall to the bit.  A wall that itself jumps over the robot between two rows is
 * seen only if its rows are sweeps of the wall's motion; the sweep of a translating segment, a
 * parallelogram, is not provided.
 * While a handle holds such a set, the walls of mppi_planner_set_walls rest; count = 0 clears it
 * and they apply again.  The launches are k_rollout_barebone_crowd's CrowdWallTracks form
 * (mppi_planner_describe_last_rollout ends in " walls=<largest count> wall_rows=<rows>"),
 * mppi_planner_closed_loop advances s with every control step when rows > 1, and
 * mppi_planner_set_crowd(p, 0) returns MPPI_ERR_INVALID until the set is cleared.  Unchanged
 * arrays cost a comparison; a change drops the captured graphs and, when rows > 1, sets every
 * offset to 0 (clearing does so unless disc tracks are held).  MPPI_ERR_INVALID -- the handle
 * keeps what it had -- for a map mode, a handle that is not in crowd mode, rows < 1, a negative
 * count, count not 0 / 1 / B, a negative or non-finite half-width, or a non-finite endpoint. */
int mppi_planner_set_wall_tracks(mppi_planner* p, int count, const int* wall_counts, int rows,
                                 const float* segments, const float* halfwidths);

/* MPPI_MODE_BAREBONE only (any other mode: MPPI_ERR_INVALID): a goal that moves.  count = 1: one
 * track for every problem; count = B: one per problem; xy is (count, rows, 2) float32, rows >= 1
 * common to the call.  Row j is the goal's position at time j*dt from "now" -- an instant, like a
 * disc row -- and "now" is the problem's track offset s (mppi_planner_set_track_offsets: one "now"
 * per problem, shared with the disc and wall tracks).  The state after step t of a rollout is
 * measured against row min(s + t + 1, rows - 1): the stage term dist_weight * d^2, the goal test
 * d^2 <= goal_tolerance^2 ("reached": within the tolerance of where the goal is at that instant),
 * the freeze and the terminal term are those of the static goal on a goal that changes with t.
 * Past its last row the goal stays at its last place; rows = 1, or equal rows, is a static goal to
 * the bit.  While a handle holds goal tracks, params.xgoal and the goals of
 * mppi_planner_set_instances rest; count = 0 clears them and the static goals apply again.
 * The default family then launches its track forms with the goal rows staged in LDS behind the disc
 * rows (8*T bytes more; a set that no longer fits in 64 KiB goes to the crowd kernel in crowd mode
 * and is refused with MPPI_ERR_INVALID, naming the bytes, otherwise); the crowd kernel takes the
 * step's row by a wave-uniform load, with every wall form.  mppi_planner_describe_last_rollout ends
 * in " goal_rows=<rows>".  mppi_planner_closed_loop advances s with every control step when
 * rows > 1 and tests the new state against row min(s_new, rows - 1): the goal where it is at the
 * time of the new state.  Unchanged arrays cost a comparison; a change builds the new device copy
 * before the old one is freed (a failure leaves the handle as it was), drops the captured graphs
 * and, when rows > 1, sets every offset to 0 (clearing does so unless disc or wall tracks are
 * held).  MPPI_ERR_INVALID for a map mode, rows < 1, count not 0 / 1 / B or a non-finite
 * coordinate. */
int mppi_planner_set_goal_tracks(mppi_planner* p, int count, int rows, const float* xy);

/* MPPI_MODE_BAREBONE: a guide round the walls.  The rollouts steer by the straight-line distance
 * to the goal and look T * dt ahead; in a room whose door lies on the side away from the goal that
 * is a wall to lean on for ever.  While the guide is on the device keeps, per problem, a
 * shortest-path distance field from the problem's static goal (params.xgoal, or the goal of
 * mppi_planner_set_instances) over a grid whose cells the shared static walls of
 * mppi_planner_set_walls block, and fills the problem's goal rows with "carrots" on the shortest
 * path from its start.  Every value is an integer or a double rounded once (csrc/guide_grid.h):
 *   grid     nx * ny <= 36864 cells (192 x 192) of side res > 0; cell (iy, ix) has the centre
 *            cx = (double)x_min + ((double)ix + 0.5) * (double)res, cy likewise; a point belongs to
 *            cell clamp(floor(((double)x - (double)x_min) / (double)res), 0, nx - 1): outside the
 *            grid, to the nearest border cell
 *   blocked  a cell whose centre is within h_k + inflate of some wall k (the rollouts' own
 *            point-to-segment test with hh = ((double)h_k + (double)inflate)^2).  inflate >= 0 and
 *            2 * inflate^2 >= res^2: then no move between free neighbouring centres touches a
 *            wall, diagonal moves included.  Discs, disc tracks, wall tracks, per-problem wall
 *            sets and the fleet's walls are NOT rasterised: the rollouts' hit tests deal with them
 *   field    uint32 [ny][nx]: 0xFFFFFFFF blocked, 0xFFFFFFFE free without a path, else the length
 *            of the shortest path to the goal's cell over free cells, 12 a straight move, 17 a
 *            diagonal one.  A goal in a blocked cell: status 1, every free cell without a path
 *   descent  from the start's cell c_0 to the in-grid neighbour with a path that minimises
 *            D[n] + w, the first minimum in the order (1,0) (0,1) (-1,0) (0,-1) (1,1) (-1,1)
 *            (-1,-1) (1,-1); R_i the length still to go (a start in a blocked cell walks out the
 *            cheapest way: R_0 = D[c_1] + w; without such a neighbour: status 2)
 *   rows     units(m) = floor((double)m / (double)res * 12.0); for j = 0 .. T row j is the centre,
 *            rounded to float32, of the first c_i with R_0 - R_i >= units(lead) + j * units(pace),
 *            or the goal itself when there is none, when that cell is the goal's, or under status
 *            1 or 2.  lead, pace >= 0 and units(lead) + T * units(pace) < 2^31
 * The state after step t of a rollout is measured against row t + 1 as against a goal track's row
 * (stage term, goal test, freeze, terminal term), whatever the track offsets are: the guide
 * neither reads nor advances nor resets them.  Both kernel families take the rows, the crowd
 * kernel with every form that takes goal tracks; mppi_planner_describe_last_rollout ends in
 * " goal_rows=<T+1> guide=<nx>x<ny>".  The field is built on the planner's stream at the head of
 * the next call that starts iterations -- mppi_planner_solve, mppi_planner_iterate_async,
 * mppi_planner_rollout, each control step of mppi_planner_closed_loop -- and only when the guide,
 * the static walls or a goal has changed; the rows are walked at the head of every such call,
 * behind the fleet's refresh, from the start states as they are on the device (closed_loop: a
 * problem that has arrived gets the goal in every row, and arrival is tested against the true
 * goal).  A refresh writes into the same arrays: captured graphs stay valid.  Keep lead above the
 * goal tolerance: a rollout that catches its carrot freezes as with any goal track.
 * An unchanged hand-over costs a comparison; a change drains the stream and drops the captured
 * graphs; on = 0 turns the guide off (the other arguments are ignored).  MPPI_ERR_INVALID, the
 * handle keeping what it held: a map mode, world_size > 1, goal tracks held (and
 * mppi_planner_set_goal_tracks with count > 0 while the guide is on), a value that is not finite,
 * res <= 0, nx or ny < 1 or more than 36864 cells, inflate < 0 or 2 * inflate^2 < res^2, lead or
 * pace < 0, or units that do not fit. */
int mppi_planner_set_guide(mppi_planner* p, int on, float x_min, float y_min, float res, int nx, int ny,
                           float inflate, float lead, float pace);
/* *fields_built: how often this handle has built the field */
int mppi_planner_get_guide(mppi_planner* p, int* on, int* nx, int* ny, unsigned long long* fields_built);
/* the refresh alone -- the field if something it depends on changed, then the rows -- and a wait
 * for the stream: for drawing and for tests.  MPPI_ERR_STATE without a guide */
int mppi_planner_guide_refresh(mppi_planner* p);
/* out: [B][ny][nx], the field of the last build (MPPI_ERR_STATE before the first) */
int mppi_planner_get_guide_field(mppi_planner* p, unsigned* out);
/* xy: [B][T+1][2], status: [B] -- of the last refresh */
int mppi_planner_get_guide_rows(mppi_planner* p, float* xy, int* status);

/* MPPI_MODE_BAREBONE, crowd mode: an occupancy grid -- a costmap -- as one more counted obstacle.
 * cells: [ny][nx] bytes, non-zero = occupied; 1 <= nx, ny <= 512; one grid for every problem of a
 * batch.  The device keeps the clearance field D2, uint32 [ny][nx]: the least
 * (ix - jx)^2 + (iy - jy)^2 over the occupied cells (jy, jx) -- 0 on an occupied cell, 0xFFFFFFFF
 * everywhere when none is occupied -- built by k_occupancy_field (csrc/occupancy_kernels.h) on the
 * planner's stream at the head of the next call that starts iterations, only when the cells have
 * changed.  Every value of the test is an integer or a double formed from widened float32 inputs
 * in the order written, no product fused into a sum (csrc/occupancy_grid.h):
 *   points   a point robot is the body of one disc (0, 0, 0); for body disc i of radius rho_i, A
 *            and B are its float32 centres at the pre-step and the post-step state (the centres
 *            of mppi_planner_set_footprint; step 0: the start state, heading included).  With
 *            M = substeps, test point k = 1 .. M is (double)B for k == M, else
 *            (double)A + ((double)k / (double)M) * ((double)B - (double)A), the product rounded
 *   inside   q = floor((X - (double)origin) / (double)res) per axis; inside iff 0 <= q <= n - 1 on
 *            both (a NaN is outside).  A point outside the grid is free
 *   verdict  at level l (0: the hit; l >= 1: clearance ring l of margin m_l): inside and
 *            D2[cell] <= thr[i][l], thr = min(floor(R * R / (res * res)), 0xFFFFFFFE) with
 *            R = ((double)inflate + (double)rho_i) + m_l
 *   count    the grid is ONE obstacle: a step whose any test point of any body disc hits adds one
 *            hit (one more rounded addition of obs_penalty); a step near at ring l adds one to n_l
 * A chord without a hit keeps every point of it more than
 * R - |AB| / (2 M) - res * sqrt(2) / 2 from every occupied cell's centre: choose inflate and
 * substeps from that; substeps = 1 is the post-step test, as for discs.  Every launch of a handle
 * that holds a grid is a grid form of the crowd kernel -- a footprint form with one CrowdGrid last
 * in the pack -- and mppi_planner_describe_last_rollout ends in " grid=<nx>x<ny>".  While a guide
 * is on as well, a guide cell whose centre lies inside the grid on a cell with D2 <= thr_g,
 * R = (double)inflate + (double)inflate_guide, is blocked too; the grid's field is built ahead of
 * the guide's, and new cells rebuild both.
 * An unchanged hand-over costs a comparison.  New cells of the same shape, geometry, inflate and
 * substeps land in the same arrays: captured graphs stay valid.  Any other change drains the
 * stream and drops the captured graphs; on = 0 clears (the other arguments are ignored).
 * MPPI_ERR_INVALID, the handle keeping what it held: a map mode, crowd mode off (and
 * mppi_planner_set_crowd(p, 0) while a grid is held), world_size > 1, disc samples held (and
 * mppi_planner_set_disc_track_samples while a grid is held), a value that is not finite,
 * res <= 0, inflate < 0, nx or ny outside 1 .. 512, substeps outside 1 .. 8, NULL cells.
 * Limits: outside the grid is free; one obs_penalty for the grid as a whole; the grid does not
 * move (a new grid per control step is the way to move it); the fleet's refresh and the
 * simulated world do not read it; the chord stands in for the arc, as with any footprint. */
int mppi_planner_set_occupancy(mppi_planner* p, int on, float x_min, float y_min, float res, int nx, int ny,
                               float inflate, int substeps, const unsigned char* cells);
/* *fields_built: how often this handle has built the clearance field */
int mppi_planner_get_occupancy(mppi_planner* p, int* on, int* nx, int* ny, unsigned long long* fields_built);
/* the field's build alone, if the cells have changed, and a wait for the stream: for drawing and
 * for tests.  MPPI_ERR_STATE without a grid */
int mppi_planner_occupancy_refresh(mppi_planner* p);
/* out: [ny][nx], the clearance field (MPPI_ERR_STATE while it has not been built for the cells held) */
int mppi_planner_get_occupancy_field(mppi_planner* p, unsigned* out);

/* MPPI_MODE_BAREBONE, a batched handle (num_instances B >= 2) in crowd mode: fleet mode -- the
 * problems are robots that avoid each other's plans.  count = B turns it on, halfwidths (B, B-1)
 * float32: row a holds reader a's half-width against every other robot b in ascending b, a
 * skipped (r_a + r_b + margin, formed by the caller); count = 0 turns it off (halfwidths ignored).
 * While it is on the library rebuilds every reader's wall set from the other robots' CURRENT plans
 * at the head of every call that starts iterations -- mppi_planner_solve, mppi_planner_rollout,
 * mppi_planner_iterate_async and each control step of mppi_planner_closed_loop -- once per call,
 * never between the iterations of a call, on the planner's stream and without the host.  The plan
 * of robot b is the noise-free rollout c_0 .. c_T of its control sequence from its start state
 * (the state step of the rollouts with zero noise, the clip to vrange / wrange included: the bits
 * of mppi_planner_get_instance_state_rollout's row 0 when the controls lie inside the ranges); it
 * goes on past the goal.  Row j of the wall that stands for b is the segment [c_j, c_{j+1}], the
 * capsule b sweeps in control interval j, and step t of a rollout of reader a is tested against
 * row t of every other robot as mppi_planner_set_walls describes: these rows are always counted
 * from "now", whatever the problem's track offset is, and fleet mode neither reads nor advances
 * nor resets that offset -- disc tracks and goal tracks keep their meaning beside it.  Behind the
 * B - 1 others every reader's set holds the static walls of mppi_planner_set_walls with their own
 * half-widths (they rest while per-problem sets are held, so the library places them itself); the
 * storage is rebuilt when fleet mode is set or those walls change (new arrays first: a failure
 * leaves the handle as it was; the captured graphs are dropped), never at a refresh, so graph
 * replay needs no new capture from one control step to the next.  In mppi_planner_closed_loop a
 * problem that has reached its goal is parked: its rows are the degenerate segment at its final
 * float32 position.  A host-driven loop parks a robot by giving it zero controls
 * (mppi_planner_set_u) where vrange admits 0.  Before the first solve the controls are zero and
 * every plan stands at its start.  All robots plan at once, each against the others' plans of the
 * previous control step (shifted): a Jacobi sweep, not the in-turn order of one planner per robot.
 * The launches are k_rollout_barebone_crowd's CrowdWallTracks form;
 * mppi_planner_describe_last_rollout holds " walls=<B-1+W> wall_rows=<T> fleet=<B>" (at its end,
 * or ahead of " goal_rows=<rows>").  One owner of the per-problem sets at a time:
 * MPPI_ERR_INVALID for mppi_planner_set_wall_tracks with a count while fleet mode is on and for
 * mppi_planner_set_fleet while wall tracks or per-problem sets are held; also for a map mode, a
 * handle with B < 2, count not 0 / B, a handle that is not in crowd mode (and
 * mppi_planner_set_crowd(p, 0) while fleet mode is on), or a negative or non-finite half-width. */
int mppi_planner_set_fleet(mppi_planner* p, int count, const float* halfwidths);
/* *on: B while fleet mode is on, else 0 */
int mppi_planner_get_fleet(mppi_planner* p, int* on);
/* the refresh alone (for tests and for drawing): the rows from the current controls and start
 * states, then waits for the stream.  MPPI_ERR_STATE unless fleet mode is on. */
int mppi_planner_fleet_refresh(mppi_planner* p);
/* seg (B, B-1, T, 4) float32 -- ax ay bx by --: reader a's others in ascending order, as the last
 * refresh left them (before the first one: walls nobody can touch, 1e18).  MPPI_ERR_STATE unless
 * fleet mode is on. */
int mppi_planner_get_fleet_walls(mppi_planner* p, float* seg);

/* MPPI_MODE_BAREBONE, crowd mode: a body footprint -- the robot as `count` discs (1 .. 8) rigidly
 * attached to its pose, so that the heading counts in the hit tests.  discs (count, 3) float32,
 * rows (ox, oy, rho): a body disc's centre in the robot frame (x along the heading, y to the left)
 * and its radius, rho >= 0, everything finite; count = 0 clears (discs ignored), and the robot is
 * its reference point again: every launch then has the kernel form, the arguments and the bits it
 * had before.  One footprint for every problem of a batch.  At a float32 state (x, y, th), with
 * s, c the float64 sine and cosine of (double)th, body disc i has its centre at
 *     cx = (float)((double)x + ((double)ox * c - (double)oy * s))
 *     cy = (float)((double)y + ((double)ox * s + (double)oy * c))
 * (products and sums in double in the order written, no fma, one rounding).  Discs: body disc i
 * touches disc k at step t iff the disc test of the launches says so with the centre at the
 * post-step state in place of the position and (r_k + rho_i)^2, the sum in double, in place of
 * r_k^2; the body touches disc k iff any of its discs does, and the step's disc hits are the
 * number of discs touched -- one hit per obstacle, however many body discs reach it.  Walls:
 * during step t body disc i moves from its centre at the pre-step state (step 0: the start state,
 * heading included) to its centre at the post-step state; the wall test of mppi_planner_set_walls
 * is applied to that segment with the half-width h_k + rho_i (the sum in double), and the body hits
 * wall k iff any of its discs does.  (A point of a turning body moves on an arc; its chord is what
 * is tested: the arc leaves it by at most |o| * (1 - cos(dt * w / 2)).)  The disc rows, the wall
 * rows, per-problem sets and disc samples are chosen as without a footprint; the goal distance,
 * the goal test, the freeze and the terminal term are the reference point's; a hit adds obs_cost
 * once, as before.  While a footprint is held every rollout launch is k_rollout_barebone_crowd,
 * whatever else the handle holds, and mppi_planner_describe_last_rollout ends in
 * " footprint=<count>".  A change drops the captured graphs.  MPPI_ERR_INVALID, the handle keeping
 * what it had: count > 8 or negative, a negative radius or a value that is not finite, a handle
 * that is not barebone or not in crowd mode (and mppi_planner_set_crowd(p, 0) while a footprint is
 * held), fleet mode on (and mppi_planner_set_fleet with a count while a footprint is held: the
 * fleet's half-widths already contain the reader's body). */
int mppi_planner_set_footprint(mppi_planner* p, const float* discs, int count);
/* discs (8, 3) float32: the first *count rows are the footprint held (*count = 0: none) */
int mppi_planner_get_footprint(mppi_planner* p, float* discs, int* count);

/* MPPI_MODE_BAREBONE, crowd mode: clearance rings -- a soft cost for passing close, as a staircase.
 * rings (count, 2) float32, 1 <= count <= 4, rows (margin, penalty): margins finite, > 0 and
 * strictly increasing, penalties finite and >= 0; count = 0 clears (rings ignored), and every
 * launch then has the kernel form, the arguments and the bits it had before.  One set for every
 * problem of a batch.  With m = (double)margin_l, obstacle k of a step is NEAR at ring l iff the
 * step would touch it were it m larger:
 *   disc k, point robot    the disc test of the launches -- the float32 difference widened, then
 *                          fma(ex, ex, ey * ey) - rr, near iff !(diff > 0) -- with rr = R * R,
 *                          R = (double)r_k + m
 *   disc k, a footprint    the footprint's disc test with R = ((double)r_k + rho_i) + m; near iff
 *                          any body disc is
 *   wall k, point robot    the wall test of mppi_planner_set_walls with hh = H * H,
 *                          H = (double)h_k + m
 *   wall k, a footprint    H = ((double)h_k + rho_i) + m per body disc chord; near iff any chord is
 * A step that crosses a wall is inside every ring.  The walls of fleet mode and of a body fleet are
 * walls like any other; in a body fleet a robot is near at ring l once, however many of its slots
 * are.  n_l(t): the obstacles near at ring l in step t, the hit ones included (n_l >= hits, and
 * n_1 <= n_2 <= ...).  The step's cost chain: the distance term; `hits` float32-rounded additions
 * of (double)obs_cost, as before; for l = 1 .. count, n_l additions
 * c1 = (float)((double)c1 + (double)penalty_l); the freeze, as before.  (Additions and not a
 * product: a ring whose penalty is obs_cost costs what a second copy of the obstacles, m larger,
 * costs, to the bit.)  The goal distance, the goal test, the freeze, the terminal term and the
 * control cost do not know about rings.  While rings are held every rollout launch is
 * k_rollout_barebone_crowd, whatever else the handle holds, and
 * mppi_planner_describe_last_rollout ends in " rings=<count>" (behind " footprint=<F>" if there is
 * one).  A change drops the captured graphs.  MPPI_ERR_INVALID, the handle keeping what it had:
 * count > 4 or negative, a bad row, a handle that is not barebone or not in crowd mode (and
 * mppi_planner_set_crowd(p, 0) while rings are held), disc samples held (and
 * mppi_planner_set_disc_track_samples with samples while rings are held: the sample forms count no
 * rings), more than 65535 discs and walls in a step at a launch. */
int mppi_planner_set_clearance_rings(mppi_planner* p, const float* rings, int count);
/* rings (4, 2) float32: the first *count rows are the rings held (*count = 0: none) */
int mppi_planner_get_clearance_rings(mppi_planner* p, float* rings, int* count);

/* MPPI_MODE_BAREBONE with MPPI_RNG_PHILOX: time-correlated control noise.  beta = (beta_v, beta_w)
 * float32, each in [0, 1), one coefficient for the linear and one for the angular control
 * component.  With w[n, t, c] the float32 value the white generator stores for rollout n, step t,
 * component c (u_std[c] times the Box-Muller normal of that rollout's Philox block under the block's
 * epoch), every generated block holds, per rollout and component, in float32
 *     g_c        = (float)sqrt(1 - (double)beta_c * (double)beta_c)                 (host, once)
 *     e[n, 0, c] = w[n, 0, c]
 *     e[n, t, c] = fadd_rn(fmul_rn(beta_c, e[n, t-1, c]), fmul_rn(g_c, w[n, t, c]))   t = 1 .. T-1
 * -- two rounded products and one rounded sum, never an fma (csrc/noise_smooth.h).  Step 0 is the
 * white draw and the gain is sqrt(1 - beta^2): every step keeps the standard deviation u_std[c], and
 * the lag-k correlation is beta_c^k.  A component with beta_c = 0 keeps its white noise.  The
 * recurrence restarts with every block: nothing is carried from one iteration or control step to
 * the next.  Philox counters, epochs, the rollout offset of a shard and the device-side epoch count
 * of graph replay are those of the white generator: the block a handle draws at epoch k is the
 * filter of the block a handle with the same seed and no smoothing draws at epoch k.  Every
 * generator launch of the handle follows -- in line, ahead on the second stream, beside the update,
 * mppi_planner_sample_noise -- and so does what mppi_planner_get_noise returns;
 * mppi_planner_set_noise stores what it is given, unfiltered.  The control-cost term of the rollout
 * is unchanged (it weighs the noise by diag(u_std^2), as for white noise).  One setting for every
 * problem of a batched handle.  NULL or (0, 0) clears: the white generator's launch, bit for bit.
 * The coefficients travel by value in the generator's argument: a change drains the stream and
 * drops the captured graphs, and a block already generated ahead is generated again, same epoch,
 * under the new coefficients, so that from the next call on the noise is what a handle that had
 * them from the start would draw at that epoch; equal values again cost a comparison.
 * MPPI_ERR_INVALID, the handle keeping what it had: a coefficient that is not finite, < 0 or >= 1,
 * a handle that is not in barebone mode (the map modes draw their noise inside the rollout launch),
 * coefficients other than (0, 0) on a MPPI_RNG_XOROSHIRO handle (that generator exists for parity
 * with the reference from the seed). */
int mppi_planner_set_noise_smoothing(mppi_planner* p, const float beta[2]);
int mppi_planner_get_noise_smoothing(mppi_planner* p, float beta[2]);
/* (measurement) average duration in microseconds of the noise generator's launch alone -- the kernel
 * the handle's smoothing setting selects -- over `reps` launches, each with its own start / stop
 * events as in mppi_planner_time_kernels.  The launches write the noise buffer no iteration is
 * reading and advance nothing.  MPPI_RNG_PHILOX only. */
int mppi_planner_time_noise(mppi_planner* p, int reps, float* us_noise);

/* MPPI_MODE_BAREBONE: acceleration limits on the sampled controls.  accel = (a_v, a_w) float32, m/s^2 and rad/s^2, each
 * > 0; +inf leaves a component as drawn.  While limits are held, every noise block an iteration is about to consume is
 * passed through one more kernel, k_noise_limit, in place, between "the block is there" and the rollout launch.  Per
 * rollout and component, with u[t] the control sequence the rollout launch reads, e[t] the block as generated (white,
 * or filtered by mppi_planner_set_noise_smoothing), (lo, hi) the component's range of mppi_params, a the problem's
 * applied control (below), all in float32, every operation rounded once (csrc/control_limits.h):
 *     d     = fmul_rn(accel_c, params.dt)                                   (host, at the launch)
 *     p     = clip(a, lo, hi)
 *     c     = clip(fadd_rn(u[t], e[t]), lo, hi)                             t = 0 .. T-1
 *     p     = fminf(fmaxf(c, fsub_rn(p, d)), fadd_rn(p, d))
 *     e'[t] = fsub_rn(p, u[t])
 * and the block holds e' -- the effective noise -- from then on: the rollouts, the control-cost term, the update and
 * mppi_planner_get_noise all see it.  The set "inside the box, no step larger than d, counted from the anchor" is convex
 * and every p sequence lies in it, so the update's weighted mean u + sum(w e') / sum(w) lies in it too, whatever u was
 * before.  What the rollouts re-form as clip(fl(u + e')) differs from p by rounding only: consecutive applied controls
 * differ by at most d + 2^-20 * (max(|lo|, |hi|) + d).  The recurrence restarts with every block from the anchor.  The
 * pass runs on the planner's stream behind the previous update (it needs the u that update left), so a block generated
 * ahead on the second stream is waited for first and the generator keeps producing unlimited blocks.
 * mppi_planner_sample_noise limits what it draws; mppi_planner_set_noise stores what it is given;
 * mppi_planner_limit_noise runs the pass alone over the block the handle holds (MPPI_ERR_STATE without limits).  One
 * pair for every problem of a batched handle; symmetric (no separate braking bound); first differences only.
 * NULL clears.  The steps and the box travel by value in the launch: a change drains the stream and drops the captured
 * graphs; equal values again cost a comparison.  MPPI_ERR_INVALID, the handle keeping what it had: a value that is NaN
 * or <= 0, a handle that is not in barebone mode. */
int mppi_planner_set_control_limits(mppi_planner* p, const float accel[2]);
/* *held = 1 and accel = the pair held, or *held = 0 and accel untouched */
int mppi_planner_get_control_limits(mppi_planner* p, float accel[2], int* held);
int mppi_planner_limit_noise(mppi_planner* p);
/* MPPI_MODE_BAREBONE: the control in force when the next plan starts -- the anchor the limits count from.  u (count, 2)
 * float32 rows (v, w), finite; count = 1 (every problem) or B.  A device array of B rows, zero at creation, stored
 * whether or not limits are held and read by the pass at its launch (at replay, for a captured one): a new anchor drops
 * no graph.  mppi_planner_closed_loop stores the u0 it applies into it at every control step while limits are held (a
 * problem that has arrived is left alone).  mppi_planner_get_applied_control: u (B, 2). */
int mppi_planner_set_applied_control(mppi_planner* p, int count, const float* u);
int mppi_planner_get_applied_control(mppi_planner* p, float* u);

/* MPPI_MODE_BAREBONE: the vehicle.  MPPI_DRIVE_UNICYCLE (the notebook's, at creation): the second control is the yaw
 * rate w.  MPPI_DRIVE_CAR: the second control is the path curvature kappa in 1/m -- tan(steering angle) / wheelbase --
 * and the yaw rate a step applies is the float32 product w = fmul_rn(v, kappa) of the clipped controls, rounded once,
 * never an fma: the car turns only while it moves, and reversing with the wheel turned left swings the heading the other
 * way.  wrange of mppi_params is then the curvature range, u_std[1] the curvature noise, and the second component of
 * mppi_planner_set_control_limits bounds the curvature's rate (k_noise_limit is unchanged).  The rollouts of both kernel
 * families, the visualisation rollouts (row 0: u_cur unclipped, w = fmul_rn(v, kappa)), the fleets' plans and the
 * simulated world of mppi_planner_closed_loop (float64: th += dt * ((double)v * (double)kappa), the product exact) follow;
 * everything downstream of the pose is what it was.  The host's bounds on the heading increment -- (cos, sin) by rotation
 * iff dt * max|w| <= 0.36 rad -- take max|w| = max|v| * max|kappa|.  mppi_planner_last_rollout_kernel gains " drive=car"
 * at the end, in both families; with MPPI_DRIVE_UNICYCLE every bit, every launch and every name is as before.  The value
 * travels by value in the launches: a change drains the stream and drops the captured graphs; an equal value again costs
 * a comparison.  One drive for every problem of a batched handle.  MPPI_ERR_INVALID, the handle keeping what it had: a
 * handle that is not in barebone mode, a value that is neither of the two. */
#define MPPI_DRIVE_UNICYCLE 0
#define MPPI_DRIVE_CAR 1
int mppi_planner_set_drive(mppi_planner* p, int drive);
int mppi_planner_get_drive(mppi_planner* p, int* drive);

/* MPPI_MODE_BAREBONE, a batched handle (B >= 2) in crowd mode: a body fleet -- fleet mode for
 * robots that are not discs.  Every robot of the batch is the same body of n_discs discs (1 .. 8),
 * discs (n_discs, 3) float32 with the rows and the rules of mppi_planner_set_footprint; count = B
 * turns it on, count = 0 turns it off (as mppi_planner_set_fleet(p, 0, NULL) does, for either kind
 * of fleet; the body goes with it).  Everything mppi_planner_set_fleet says about the refresh, the
 * rows counted from "now", the static walls, parking, the Jacobi lag of the plans and graph replay
 * holds.  What differs:
 *   plans   the noise-free rollout with its heading kept: states s_0 .. s_T = (x, y, th) float32; a
 *           parked robot stands at its start pose, heading included.
 *   walls   body disc k of robot b has its centre c_j^k at state s_j as mppi_planner_set_footprint
 *           forms it, to the bit, and sweeps the segment [c_j^k, c_{j+1}^k] in control interval j
 *           (the chord for the arc, as for any footprint).  Reader a is given that segment as a wall
 *           of half-width (float)((double)rho_k + (double)margin); margin finite, rho_k + margin >= 0.
 *   reader  the reader's own body enters as for any wall: body disc i's chord against the wall
 *           with the half-width h + rho_i, the sum in double.
 *   hits    a step of a rollout hits robot b iff ANY body disc of the reader hits ANY wall of b:
 *           one hit, obs_cost once, however many pairs touch.  The static walls behind the fleet
 *           slots count one hit per wall, as with any footprint.
 *   slots   reader a's set: (B - 1) * Fp fleet slots, Fp = n_discs rounded up to a power of two,
 *           robot `other` (ascending, a skipped) disc k at other * Fp + k; the padding slots
 *           k >= n_discs repeat the last disc.  Then the W static walls.  Work per (step, rollout):
 *           n_discs * ((B - 1) * Fp + W) wall tests -- a body of 3, 5, 6 or 7 discs pays for its
 *           padding.  The size limits of the fleet apply to this slot count.
 * One body for the whole fleet (per-robot bodies are not provided).  The body is held as the handle's
 * footprint: mppi_planner_get_footprint gives its rows, every launch is a footprint form with wall
 * tracks, and mppi_planner_describe_last_rollout holds
 * " walls=<(B-1)*Fp+W> wall_rows=<T> fleet=<B>" and ends in " footprint=<n_discs>".  The same
 * arguments again are a no-op; a change drains the stream and drops the captured graphs.
 * MPPI_ERR_INVALID, the handle keeping what it had: the refusals of mppi_planner_set_fleet (a map
 * mode, B < 2, count not 0 / B, a sharded handle, no crowd mode, wall tracks held), a footprint held
 * through mppi_planner_set_footprint, a disc fleet on (and mppi_planner_set_fleet with half-widths
 * while a body fleet is on: the kinds change through "off"), bad rows or a bad margin.  While any
 * fleet is on mppi_planner_set_footprint is refused; in a body fleet its clear as well. */
int mppi_planner_set_fleet_bodies(mppi_planner* p, int count, const float* discs, int n_discs, double margin);
/* *n_discs: the body discs of the body fleet that is on, else 0; *margin: its margin */
int mppi_planner_get_fleet_bodies(mppi_planner* p, int* n_discs, double* margin);
/* seg (B, B-1, F, T, 4) float32 -- ax ay bx by --: reader a's others in ascending order, body disc
 * k of each, as the last refresh left them, the padding slots left out.  MPPI_ERR_STATE unless a
 * body fleet is on; there mppi_planner_get_fleet_walls is refused (MPPI_ERR_INVALID). */
int mppi_planner_get_fleet_body_walls(mppi_planner* p, float* seg);

/* mppi.py:539-542 shift_optimal_control_sequence / mppi.py:305,375 copy_to_host */
int mppi_planner_set_u(mppi_planner* p, const float* u);
int mppi_planner_get_u(mppi_planner* p, float* u);
int mppi_planner_get_u_prev(mppi_planner* p, float* u);
/* device-side u[:-k] = u[k:] (tail kept), no host round trip */
int mppi_planner_shift_u(mppi_planner* p, int num_shifts);

/* mppi.py:186-531 solve(): samples both TDMs once, then num_opt x
 * {sample noise, rollout, update}; writes the (T,2) control sequence.
 * lin/ang are NULL in MPPI_MODE_BAREBONE. */
int mppi_planner_solve(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, float* u_out);

/* the same without sampling the TDMs and without the final copy: `iterations`
 * back-to-back {noise, rollout, update} on the planner's stream */
int mppi_planner_iterate_async(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, int iterations);
int mppi_planner_synchronize(mppi_planner* p);

/* stage-level entry points (the individual kernel launches of mppi.py:259-303),
 * used by the parity tests to inject identical noise / grids / costs */
int mppi_planner_sample_noise(mppi_planner* p);                              /* mppi.py:1354 */
int mppi_planner_set_noise(mppi_planner* p, const float* noise);             /* (N_local,T,2) */
int mppi_planner_get_noise(mppi_planner* p, float* noise);
int mppi_planner_rollout(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang);     /* mppi.py:613-1111 */
int mppi_planner_set_costs(mppi_planner* p, const float* costs);             /* (N_local) */
int mppi_planner_get_costs(mppi_planner* p, float* costs);
/* (N_local,M), TDM mode; MPPI_MODE_BAREBONE while disc samples are held: (N_local,S) -- (B*N,S) for
 * a batched handle --, the per-sample costs before the tail, in sample order.  NULL arms recording
 * for the rollouts that follow; a pointer fetches. */
int mppi_planner_get_sample_costs(mppi_planner* p, float* costs);
int mppi_planner_update(mppi_planner* p);                                    /* mppi.py:1113-1191 */
int mppi_planner_get_weights(mppi_planner* p, float* weights);               /* normalised, (N_local) */

/* mppi.py:545-608 get_state_rollout -> (V, T+1, 3) */
int mppi_planner_get_state_rollout(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, float* out);
/* the same for problem `instance` of a batched handle (get_state_rollout = instance 0) */
int mppi_planner_get_instance_state_rollout(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, int instance,
                                            float* out);

/* xoroshiro-compatible generator only: copy the (N_local*T, 2) uint64 states */
int mppi_planner_rng_states(mppi_planner* p, uint64_t* out, long capacity, long* count);

/* hipEvent timing (planner's stream) of the stages of the LAST iteration of the
 * last solve/iterate call, in ms; recorded only while profiling is enabled:
 * [0] noise  [1] rollout  [2] update (weights + weighted sum + apply)  [3] collective */
int mppi_planner_set_profiling(mppi_planner* p, int enabled);
int mppi_planner_stage_times(mppi_planner* p, float ms[4]);
/* (new; measurement) average duration in microseconds of the rollout launch and of the update
 * launch over `reps` ordinary iterations of the loop (iterate_async): every launch carries its
 * own start / stop events, filled by the runtime with the dispatch's begin / end timestamps --
 * the durations rocprofv3 --kernel-trace reports -- with nothing inserted between the kernels
 * (bench.py's roofline figures). */
int mppi_planner_time_kernels(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, int reps, float* us_rollout,
                              float* us_update);
/* GPU time (ms, hipEvents on the planner's stream) of the last iterate_async call (of the
 * last solve too while profiling is enabled; solve() does not time itself otherwise) */
int mppi_planner_last_elapsed_ms(mppi_planner* p, float* ms);

/* tracing hook: with MPPI_ROCTX=1 in the environment the library brackets solve / sample_grids /
 * noise / rollout / exchange / update / closed_loop with roctx ranges (names "mppi:...") for
 * `rocprofv3 --marker-trace --kernel-trace`; returns 1 when the ranges are live, else 0 */
int mppi_trace_ranges_enabled(void);

/* diagnostic: which rollout kernel variant (and its launch geometry) the last rollout used */
int mppi_planner_describe_last_rollout(mppi_planner* p, char* buf, int capacity);

/* diagnostic: compares the library's single-block Philox4x32-10 with rocRAND's engine on
 * 65536 (seed, subsequence, offset) triples; *mismatches must come back 0 */
/* developer switches for the parity tests, which pin every rollout kernel variant by name
 * (mppi_planner_describe_last_rollout).  With MPPI_MATH_EXACT the costs never depend on them (every
 * variant has the reference's bits); u agrees to float32 resolution between kernel families (the
 * update's float64 summation tree follows the rollout kernel's tiles of 32 or 64 rollouts: both sit
 * far inside the 1e-5 the reference's own unordered float32 atomics allow).  With MPPI_MATH_FAST they select between kernels that agree to
 * float32 tolerance only -- and so does whatever else decides which kernel runs there: N, the map
 * (a failed traction vote re-runs a tile sequentially; a map that keeps failing switches the
 * speculative kernels off until it changes). */
#define MPPI_DEBUG_NO_SPEC_KERNEL 1  /* retired (round 6: k_rollout_spec removed, profiles/r06_families.md); accepted, no effect */
#define MPPI_DEBUG_NO_SPECULATION 2  /* the speculative kernels on their exact schedule from the first step */
#define MPPI_DEBUG_NO_DEEP_KERNEL 4  /* retired (round 6: k_rollout_deep removed); accepted, no effect */
#define MPPI_DEBUG_CC_GLOBAL 8       /* control-cost products in the global scratch array even when LDS has room */
#define MPPI_DEBUG_KEEP_SPECULATING 16 /* keep the speculative kernels on a map where their tiles keep falling back */
/* MPPI_MATH_FAST, the time-parallel rollout (k_rollout_scan): */
#define MPPI_DEBUG_NO_SCAN_KERNEL 32     /* not the time-parallel kernels: k_rollout_pipe / k_rollout_fused / k_rollout_map instead */
#define MPPI_DEBUG_SCAN_READ_NOISE 64    /* the iteration loop stores its noise and the kernel reads it (as the stage-level calls do) */
#define MPPI_DEBUG_SCAN_FULL_TILES 128   /* workgroups of 64 rollouts (one lane per rollout) instead of 32 (two) */
#define MPPI_DEBUG_NO_FOLDED_APPLY 256   /* sharded handle: every iteration's update by its own k_apply launch, never by the next rollout launch */
#define MPPI_DEBUG_NO_REDUCE_FOLD 512    /* one GPU: every iteration's update by its own k_combine_tiles launch, never reduced and applied by the next rollout launch */
#define MPPI_DEBUG_NO_SCAN_DIRECT 1024   /* a map the planner has stopped speculating on: k_rollout_pipe + k_update_rows (round 4) instead of k_rollout_scan_exact on its exact schedule (one launch per iteration) */
#define MPPI_DEBUG_DROP_NOISE_FLAG 2048  /* test hook: the noise generator on the second stream does not announce itself -- the launch that waits for it gives up after ~60 ms, the next draining call returns MPPI_ERR_BUSY and the handle orders its streams with events from then on */
int mppi_planner_set_debug_flags(mppi_planner* p, int flags);
/* How long a workgroup of a rollout launch polls for the controls its sibling workgroups publish inside the launch
 * (update folded into the next rollout launch: rollout_scan*_kernel.h) before it gives the launch up: `polls` of
 * ~0.3-1 us each (default 2^20, about a second; test hook).  After a give-up the next call that waits for the handle's
 * stream -- synchronize, solve, and every stage-level call that returns data (get_u, get_costs, rollout, update ...) --
 * returns MPPI_ERR_BUSY and the handle stops folding (mppi_planner_fold_state: folding, faults so far).  Calling
 * mppi_planner_set_fold_poll_limit again re-arms the handle: it folds again (and gives up again if the device is still
 * shared). */
int mppi_planner_set_fold_poll_limit(mppi_planner* p, int polls);
int mppi_planner_fold_state(mppi_planner* p, int* folding, long* faults);
/* developer / test hook: occupy `workgroups` compute units of `device` (one workgroup each: 100 KiB of LDS) for
 * `milliseconds` on a stream of its own, so that a rollout launch beside it cannot have all its workgroups resident */
int mppi_debug_occupy_cus(int device, int workgroups, int milliseconds);
int mppi_selftest_philox(int device, int* mismatches);
/* developer instrumentation: in-kernel clock stamps of a -DMPPI_STAMPS build
 * (csrc/Makefile target `stamps`, tools/stamp_timeline.py); MPPI_ERR_STATE otherwise */
int mppi_debug_read_stamps(unsigned long long* out, int count, int clear);
/* hipGraph replay of the iteration loop (off by default).  A sharded handle needs its RCCL
 * communicator first: the all-gather is captured with the kernels.
 * iterations_per_graph: 0 = off, else an even number (the noise double buffer must come
 * back to where it was).  When on, every iteration also produces the noise of its
 * successor, that many iterations are captured into a graph the first time and replayed
 * for as long as nothing a kernel argument carries has changed (parameters, maps, start
 * state of a single-problem handle ...); the Philox call epoch then lives in device
 * memory.  Results are identical to the direct loop.  Worth it for loops of many
 * iterations (params.num_opt, iterate_async); a handle whose start state changes every
 * call re-captures every call unless it is a batched handle (set_instances), whose
 * start / goal live in device memory. */
int mppi_planner_set_graph_replay(mppi_planner* p, int iterations_per_graph);
int mppi_planner_graph_stats(mppi_planner* p, long* captures, long* replays);
/* developer measurement: wall microseconds per iteration of `iterations` (even) x {noise,
 * rollout, update}, launched directly vs replayed from a captured hipGraph, `replays`
 * times each.  Replays reuse the captured arguments: a measurement, not a way to plan. */
int mppi_planner_graph_probe(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, int iterations, int replays,
                             float* us_direct, float* us_graph);

/* ---- the simulated world of the closed-loop demo, on the device ------
 * mppi_world replaces TractionGrid (terrain.py:750-785): float64 (rows, cols) grids of linear and
 * angular traction, resolution and lower limits as in its constructor (terrain.py:754-773).
 *   create            TractionGrid.__init__; lin / ang may be NULL (zeros) when the grids are drawn
 *                     on the device afterwards
 *   get               TractionGrid.get (terrain.py:776-782) for `count` points xy[count][2]:
 *                     the cell's (lin, ang), (0, 0) outside the grid; Python's float // rule
 *   get_grids         TractionGrid.get_grids (terrain.py:784-785)
 *   sample_true_dist  TDM_Numba.sample_grids_true_dist (terrain.py:586-608): every cell draws from
 *                     the densities of its terrain type, linear and angular independently.  The
 *                     densities are host objects; the device draws uniformly (Philox4x32-10 keyed by
 *                     seed, counter = cell index and call number) from the pools of samples every
 *                     Terrain keeps (terrain.py:44-46): lin_pool / ang_pool [n_terrains][pool_len],
 *                     terrain_of_cell [rows*cols] = row of the pools for each cell.               */
typedef struct mppi_world mppi_world;
int mppi_world_create(int device, int rows, int cols, double res, double xlo, double ylo, const double* lin,
                      const double* ang, mppi_world** out);
int mppi_world_destroy(mppi_world* w);
int mppi_world_get(mppi_world* w, const double* xy, int count, double* lin_out, double* ang_out);
int mppi_world_get_grids(mppi_world* w, double* lin, double* ang);
int mppi_world_sample_true_dist(mppi_world* w, const int32_t* terrain_of_cell, int n_terrains, const double* lin_pool,
                                const double* ang_pool, int pool_len, uint64_t seed);
/* The notebooks' closed loop (test.ipynb cell 4: solve -> TractionGrid.get -> float64 Euler step ->
 * shift_and_update(x_new, useq, 1) -> goal check) for every problem of a batched handle
 * (set_instances, count >= 1), max_steps times or until every problem is within goal_tolerance of
 * its goal, without a host round trip per control step: the new start state, the LDS window
 * origin and the shifted control sequence are written by a kernel on the planner's stream.
 *   dt     the world's Euler step (cfg.dt as the notebook uses it, float64); <= 0: params.dt
 *   x_init [B][3] float64 start states (NULL: the instances' float32 start states)
 *   xhist  [B][max_steps+1][3] float64, row 0 = start, rows never reached = NaN
 *   uhist  [B][max_steps][2]   float32, the control applied at every step (NaN likewise)
 *   steps_taken [B]            steps until the goal test passed (or the number of steps run)
 * Afterwards the handle is where the notebook's loop would have left it (start states, shifted u).
 * MPPI_MODE_BAREBONE: lin = ang = w = NULL, the barebone notebook's loop (cell 7): the nominal
 * unicycle, x += dt*cos(th)*u0, y += dt*sin(th)*u0, th += dt*u1 in float64.  The map modes need w. */
int mppi_planner_closed_loop(mppi_planner* p, mppi_tdm* lin, mppi_tdm* ang, mppi_world* w, int max_steps,
                             double dt, double goal_tolerance, const double* x_init, double* xhist, float* uhist,
                             int* steps_taken);

/* ---- multi-GPU: N sharded over ranks, one RCCL all-gather of (2T+2) floats
 *      per iteration (not in the reference) ------------------------------------ */
#define MPPI_COMM_ID_BYTES 128
int mppi_comm_unique_id(char id[MPPI_COMM_ID_BYTES]);
int mppi_planner_comm_init(mppi_planner* p, const char id[MPPI_COMM_ID_BYTES]);
/* ranks RCCL itself reports for the handle's communicator (ncclCommCount); 0 without one */
int mppi_planner_comm_count(mppi_planner* p, int* ranks);
/* The peer exchange: the same sharding without a collective on the iteration's path.  Every rank owns an inbox
 * in fine-grained device memory; the workgroup that has combined the local tiles for step t of an update writes the
 * rank's four numbers for that step straight into every rank's inbox (peer access inside one process, IPC-mapped
 * memory across processes: xGMI on a multi-GPU node) and waits for the others' in its own -- inside the next
 * rollout launch, or inside the update launch that closes a loop.  A sharded iteration of the time-parallel exact
 * kernel (deterministic dynamics, one round of tiles: BASELINE configs[1] per GPU) is then ONE launch; u has the bits
 * of the all-gather + k_apply path.  Handles the kernels cannot serve keep using the communicator.
 *   p2p_export   this rank's inbox as an opaque handle (hipIpcMemHandle_t) for the other processes
 *   p2p_connect  the handles of all `count` = world_size ranks, in rank order (the own one is ignored)
 *   group_p2p_connect  one process driving `count` devices: planners[g] is rank g
 *   p2p_stats    connected?, exchanges performed so far, how the inbox was allocated
 * A rank whose peers stop sending (a dead process) does not hang: after a few seconds of polling (MPPI_P2P_MAX_POLLS) its kernels raise
 * a fault word and run on without waiting again; mppi_planner_solve / mppi_planner_synchronize then return
 * MPPI_ERR_COMM (the control sequence of that call is not valid; reconnect before using the exchange again). */
#define MPPI_P2P_HANDLE_BYTES 64
int mppi_planner_p2p_export(mppi_planner* p, char handle[MPPI_P2P_HANDLE_BYTES]);
int mppi_planner_p2p_connect(mppi_planner* p, const char* handles, int count);
int mppi_group_p2p_connect(mppi_planner** planners, int count);
int mppi_planner_p2p_stats(mppi_planner* p, int* connected, long* exchanges, char* kind, int capacity);
/* all ranks together, after connecting: every rank writes `token` (neither 0 nor all ones, the same on all ranks, new for every
 * call) into every inbox and waits up to ~timeout_ms for the others' -- without trapping.  *heard == world_size: peer
 * stores reach this rank's running kernels, the exchange can be trusted; otherwise switch it off on ALL ranks. */
int mppi_planner_p2p_ping(mppi_planner* p, unsigned long long token, int timeout_ms, int* heard);
/* a connected exchange switched off and on again (all ranks alike; off: the handle's communicator is used) */
int mppi_planner_p2p_set_enabled(mppi_planner* p, int enabled);
/* One process driving `count` devices: planners[g] is rank g of `count` on its own device.
 * comm_init creates all communicators inside one RCCL group; iterate_async runs `iterations` x
 * {per device: noise, rollout, shard packet | one group of all-gathers | per device: apply} and
 * returns without waiting (mppi_planner_synchronize each handle).  Replaces, for a multi-GPU
 * planner, the single-device numba context of the reference (config.py:9, mppi.py:186-303). */
int mppi_group_comm_init(mppi_planner** planners, int count);
int mppi_group_iterate_async(mppi_planner** planners, mppi_tdm** lins, mppi_tdm** angs, int count, int iterations);
/* host-staged alternative to RCCL (the exchange itself is then done by the
 * caller, e.g. over gloo): packet = {beta, den, num[T][2]} of the local shard,
 * 2T+2 doubles; update_apply takes the packets of all ranks in rank order */
int mppi_planner_packet_len(mppi_planner* p, int* doubles);
/* ---- multi-GPU, CVaR mode: the M traction-map samples sharded over ranks ------
 * Rank r of G rolls ALL N control samples (rollout_numba, mppi.py:613-755) over traction samples
 * [r*M/G, (r+1)*M/G): its TDMs draw exactly those samples of the unsharded set
 * (mppi_tdm_set_sample_shard: first sample, even; Philox generator), its planner is created with
 * num_grid_samples = M/G, world_size = 1 and told its place (mppi_planner_set_sample_sharding,
 * before comm_init).  Per iteration ONE RCCL all-gather of the (N, M/G) float32 per-sample costs
 * (N*M*4 bytes in total); every rank then sorts / averages all M costs of every control sample
 * (the reference's order, mppi.py:716-755: costs have the bits of the unsharded launch) and runs
 * the control update locally -- all ranks hold the same u without a second collective.
 * sample_costs_local / sample_costs_apply are the host-staged form of the exchange (after
 * mppi_planner_rollout; slabs: (G, N, M/G) in rank order), followed by mppi_planner_update. */
int mppi_tdm_set_sample_shard(mppi_tdm* t, int first_sample);
int mppi_planner_set_sample_sharding(mppi_planner* p, int rank, int count);
int mppi_planner_sample_costs_local(mppi_planner* p, float* slab);
int mppi_planner_sample_costs_apply(mppi_planner* p, const float* slabs, int count);
int mppi_planner_update_local(mppi_planner* p, double* packet);
int mppi_planner_update_apply(mppi_planner* p, const double* packets, int count);
/* update_apply followed by the NEXT iteration's rollout (its noise already sampled) as one call: when
 * that rollout is one of the time-parallel kernels its launch forms u from the packets itself (every
 * wave the 8 steps it owns, k_apply's expressions and order: same bits) and no k_apply is launched --
 * what mppi_planner_iterate_async does between the iterations of a sharded handle (a sharded iteration
 * is then rollout, rank packet, all-gather: three launches instead of four).  Otherwise exactly
 * update_apply + rollout. */
int mppi_planner_update_apply_and_rollout(mppi_planner* p, const double* packets, int count, mppi_tdm* lin,
                                          mppi_tdm* ang);

#ifdef __cplusplus
}
#endif
#endif /* MPPI_HIP_H */
