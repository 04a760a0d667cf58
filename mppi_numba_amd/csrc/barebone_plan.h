// barebone_plan.h -- which kernel a barebone rollout launch runs, as a pure function of what the handle holds.
// Plain C++ without a HIP type: a host program compiles it on its own (tests/test_barebone_plan.py pins the table).
// barebone_held(p) (barebone_launch.h) fills the state from a handle; the launchers there carry a choice out.
#pragma once

#include <algorithm>
#include <cstddef>

// Crowd mode (mppi_planner_set_crowd; rollout_crowd_kernel.h): from this many discs on -- the largest problem's count --
// the rollout runs k_rollout_barebone_crowd.  Every form gives the same bits, so the crossover is a timing decision, to be
// taken from tools/barebone_crowd_timing.py (solve() at N = 1000, T = 50, crowd off and on side by side; profiles/HISTORY.md,
// "Barebone crowd mode").  NOT MEASURED YET: 5 is the lowest value the design allows -- up to four discs under rotation the
// KD forms are a single basic block -- and tests/test_gpu_barebone_crowd.py expects the crowd kernel from five discs on.
// Below it the default forms run (they fit: a set this small needs 16 * T * (1 + K) bytes at the most -- and where a long
// horizon's tracks do not, the crowd kernel runs).
constexpr int kCrowdMinDiscs = 5;

constexpr size_t kBareboneLdsMax = 64 * 1024;  // what a launch of the default family may ask for

// The LDS of k_rollout_barebone in bytes (rollout_kernels.h):
//   [T] double2 control ratios | [slots] float4 discs                  the static forms
//   [T] double2 control ratios | [T][slots] float4, a row per step     the track forms
//   ... | [T] float2 goal positions behind the disc rows               the goal forms (track forms only)
// A row has one slot at the least.  spare_slots: the classic single launch of a static set has always asked for its KD
// padding on top of the set's own slots -- more than the kernel touches, but the dynamic LDS size is part of the launch.
inline size_t barebone_lds(int T, int slots, bool track_form, bool goal_form, int spare_slots = 0) {
  const size_t row = 16 * (size_t)std::max(1, slots);
  return 16 * (size_t)T + (track_form ? (size_t)T * row : row) + (goal_form ? 8 * (size_t)T : 0) + 16 * (size_t)spare_slots;
}

// The limits of the crowd family, k_rollout_barebone_crowd (rollout_crowd_kernel.h): defined here, once, for the kernel, the
// handle (handles.h) and the host code alike.
constexpr int kCrowdChunkMax = 16;          // steps per chunk at the most (the walker keeps a chunk's noise in registers)
// Disc samples (mppi_planner_set_disc_track_samples): S sampled futures of the moving discs, the rollout's cost the CVaR tail
// over its S costs.  Crowd family only.
constexpr int kCrowdSamplesMax = 16;
constexpr int kCrowdSampleHitsMax = 65535;  // the sample and ring forms count a step's hits in 16 bits: discs + walls at the most
constexpr size_t kCrowdSampleLdsAim = 64 * 1024;  // the chunk of a sample form shrinks towards this
constexpr int kCrowdFootprintMax = 8;       // body footprint (mppi_planner_set_footprint): discs at the most
constexpr int kCrowdRingsMax = 4;           // clearance rings (mppi_planner_set_clearance_rings): rows at the most

// The dynamic LDS of k_rollout_barebone_crowd in bytes -- the one definition: the choice, the launcher and the kernel's
// pointer arithmetic (rollout_crowd_kernel.h) all follow this layout:
//   [T] double2 control ratios | [2][C][64] double goal distance | [2][C (+ 1 with walls)][64] float2 position (with walls,
//   slot 0: the chunk's entry position) | [2][C][64] int hits | two "tile done" words    the plain forms (samples = 0)
//   ... | [2][C][S][64] uint16 hits in place of the int hits | two words | [S][64] float running costs    the sample forms
//   ... | [2][C][1 + R][64] uint16 counts in place of the int hits                     the ring forms (R clearance rings)
//   ... | [2][C (+ 1 with walls)][64] float heading, slot for slot beside the positions | [3][8] double, the footprint's
//   rows (ox | oy | rho)                                                               the footprint forms (behind all of that)
//   ... | [8][1 + 4] uint32, the grid's thresholds; the positions and the headings with the entry slot, as with walls
//                                                                                      the grid forms (footprint forms all)
constexpr size_t crowd_lds(int T, int C, bool walls, int samples = 0, bool footprint = false, int rings = 0, bool grid = false) {
  const size_t hits = samples > 0 ? (size_t)2 * C * samples * 64 * 2 + (size_t)samples * 64 * 4
                      : rings > 0 ? (size_t)2 * C * (1 + rings) * 64 * 2 : (size_t)2 * C * 64 * 4;
  const size_t entry = walls || grid ? 1 : 0;
  const size_t heading = footprint ? (size_t)2 * (C + entry) * 64 * 4 + 3 * 8 * 8 : 0;
  return 16 * (size_t)T + (size_t)2 * C * 64 * 8 + (size_t)2 * (C + entry) * 64 * 8 + hits + 8 + heading + (grid ? 8 * 5 * 4 : 0);
}
static_assert(crowd_lds(100, 16, false) == 16 * 100 + 2 * 16 * 64 * (8 + 8 + 4) + 8 &&
                  crowd_lds(50, 14, true) == 16 * 50 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 64 * 4 + 8 &&
                  crowd_lds(50, 14, true, 2) == 16 * 50 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 2 * 64 * 2 + 2 * 64 * 4 + 8 &&
                  crowd_lds(37, 14, true, 3) == 16 * 37 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 3 * 64 * 2 + 3 * 64 * 4 + 8 &&
                  crowd_lds(100, 16, false, 0, true) == 16 * 100 + 2 * 16 * 64 * (8 + 8 + 4) + 8 + 2 * 16 * 64 * 4 + 192 &&
                  crowd_lds(37, 14, true, 3, true) == 16 * 37 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 3 * 64 * 2 + 3 * 64 * 4 + 8 + 2 * 15 * 64 * 4 + 192 &&
                  crowd_lds(100, 16, false, 0, false, 1) == 16 * 100 + 2 * 16 * 64 * (8 + 8) + 2 * 16 * 2 * 64 * 2 + 8 &&
                  crowd_lds(37, 14, true, 0, true, 4) == 16 * 37 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 5 * 64 * 2 + 8 + 2 * 15 * 64 * 4 + 192 &&
                  crowd_lds(37, 14, false, 0, true, 0, true) == 16 * 37 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 64 * 4 + 8 + 2 * 15 * 64 * 4 + 192 + 160 &&
                  crowd_lds(37, 14, true, 0, true, 0, true) == crowd_lds(37, 14, true, 0, true) + 160 &&
                  crowd_lds(50, 14, false, 0, true, 4, true) == 16 * 50 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 5 * 64 * 2 + 8 + 2 * 15 * 64 * 4 + 192 + 160,
              "crowd_lds: the layout above, byte for byte -- plain, sample, footprint, ring and grid forms");

// C steps per chunk for a workgroup of W waves: the largest multiple of the W - 2 counters within kCrowdChunkMax, every
// counter the same share.  A sample form gives up whole shares while its LDS is above kCrowdSampleLdsAim (one share stays).
inline int crowd_chunk(int W, int T = 0, bool walls = false, int samples = 0, bool footprint = false) {
  const int counters = std::min(std::max(W - 2, 1), kCrowdChunkMax);
  int C = (kCrowdChunkMax / counters) * counters;
  while (samples > 0 && C > counters && crowd_lds(T, C, walls, samples, footprint) > kCrowdSampleLdsAim) C -= counters;
  return C;
}

// What the choice depends on.
struct BareboneHeld {
  int T = 0;
  bool batched = false;  // one launch over the problems of mppi_planner_set_instances
  bool rot = false;      // (cos, sin) by rotation (rotation_ok, exact math)
  bool crowd = false;
  int n_obstacles = 0;   // the shared static set
  bool inst_obs_on = false;
  int inst_obs_max = 0;  // a static set per problem: the largest
  bool trk_on = false;
  int trk_max = 0, trk_rows = 0;  // disc tracks: the largest problem's count
  int n_walls = 0;
  bool wtrk_on = false, fleet_on = false, gtrk_on = false;
  int samples = 0;                   // disc samples: S (0: none held), ...
  int smp_discs = 0, smp_rows = 0;   // ... K discs of L rows each
  int crowd_waves = 16;              // crowd family: waves per workgroup (crowd_shape of barebone_launch.h)
  int footprint = 0;                 // body footprint: F discs (0: the robot is its reference point)
  int rings = 0;                     // clearance rings: R rows (0: none held)
  bool grid = false;                 // an occupancy grid (mppi_planner_set_occupancy) is held
};

enum BareboneFamily { kBareboneDefault = 0, kBareboneCrowd = 1, kBareboneRefused = 2 };
enum BareboneDiscs { kDiscsShared = 0, kDiscsOwn = 1, kDiscsTracks = 2, kDiscsSamples = 3 };
// a refusal: the set that does not fit in 64 KiB of LDS (and crowd mode is off); disc samples, a body footprint, or clearance
// rings, without crowd mode
enum BareboneLimit { kLimitNone = 0, kLimitStaticDiscs = 1, kLimitDiscTracks = 2, kLimitGoalTrack = 3, kLimitSamplesNeedCrowd = 4,
                     kLimitFootprintNeedsCrowd = 5, kLimitRingsNeedCrowd = 6 };

struct BareboneChoice {
  BareboneFamily family = kBareboneDefault;
  BareboneDiscs discs = kDiscsShared;
  int kmax = 0;             // the largest problem's disc count
  int kd = -1;              // default family: disc slots fixed at compile time (2, 4), or -1: the run-time loop
  bool track_form = false;  // default family: a row of disc slots per step (disc tracks, or static discs under a goal track)
  bool goal_form = false;   // a goal that moves
  int walls = 0;            // crowd family: 0 none, 1 static walls, 2 wall tracks / per-problem sets / fleet
  size_t lds = 0;           // default family: the dynamic LDS launched; a sample form, a footprint form, a ring form: likewise
  BareboneLimit limit = kLimitNone;
  int samples = 0;          // crowd family: 0, or the sample form over this many disc samples
  int chunk = 0;            // a sample form: steps per chunk; a footprint form, a ring form: likewise
  int footprint = 0;        // crowd family: 0, or the footprint form over this many body discs
  int rings = 0;            // crowd family: 0, or the ring form over this many clearance rings
  bool grid = false;        // crowd family: the grid form (a footprint form: a point robot runs as the one-disc body (0, 0, 0))
};

// Crowd mode: does a launch go to the crowd kernel?  own_lds: what the default form holds at the least.  Walls are the
// crowd kernel's alone: a handle that holds any always goes there.
inline bool crowd_launch(const BareboneHeld& h, int kmax, size_t own_lds) {
  return h.crowd && (h.n_walls > 0 || h.wtrk_on || h.fleet_on || kmax >= kCrowdMinDiscs || own_lds > kBareboneLdsMax);
}

// The disc source: tracks take the place of both static sets, a problem's own set that of the shared one.  A goal that
// moves runs the track forms (static discs as tracks of one row).  The KD forms are chosen by the largest problem's count
// under rotation; a track form whose padded row does not fit falls back to the loop over the problem's own row.
// Disc samples are a disc source of the crowd family alone: they take the place of the tracks, run as TRACKS forms, and
// take static shared walls as wall tracks of one row (walls = 1 stays the choice; crowd_form, below, names the argument).
// A body footprint (mppi_planner_set_footprint) is the crowd family's alone as well: a handle that holds one always goes
// there, whatever it holds otherwise -- no discs and no walls included --, and launches a footprint form: a TRACKS form, static
// discs as tracks of one row, static shared walls as wall tracks of one row, with the chunk and the LDS of the choice.
// Clearance rings (mppi_planner_set_clearance_rings) likewise: the crowd family always, a TRACKS form with the chunk and the
// LDS of the choice, with or without a footprint.  (The hand-over keeps rings and disc samples apart.)
// An occupancy grid (mppi_planner_set_occupancy; the hand-over wants crowd mode and keeps it apart from disc samples)
// likewise: the crowd family always -- no discs and no walls included --, a footprint form with the chunk and the LDS of the
// choice, whether or not a footprint is held.
inline BareboneChoice barebone_choose(const BareboneHeld& h) {
  BareboneChoice c;
  c.footprint = h.footprint;
  c.rings = h.rings;
  c.grid = h.grid;
  if (h.rings > 0 && !h.crowd) {
    c.family = kBareboneRefused;
    c.limit = kLimitRingsNeedCrowd;
    return c;
  }
  if (h.footprint > 0 && !h.crowd) {
    c.family = kBareboneRefused;
    c.limit = kLimitFootprintNeedsCrowd;
    return c;
  }
  if (h.samples > 0) {
    c.discs = kDiscsSamples;
    c.kmax = h.smp_discs;
    c.goal_form = h.gtrk_on;
    c.track_form = true;
    c.walls = (h.wtrk_on || h.fleet_on) ? 2 : (h.n_walls > 0 ? 1 : 0);
    c.samples = h.samples;
    if (!h.crowd) {
      c.family = kBareboneRefused;
      c.limit = kLimitSamplesNeedCrowd;
      return c;
    }
    c.family = kBareboneCrowd;
    c.chunk = crowd_chunk(h.crowd_waves, h.T, c.walls != 0, c.samples, c.footprint > 0);
    c.lds = crowd_lds(h.T, c.chunk, c.walls != 0, c.samples, c.footprint > 0);
    return c;
  }
  c.discs = h.trk_on ? kDiscsTracks : (h.inst_obs_on ? kDiscsOwn : kDiscsShared);
  c.kmax = h.trk_on ? h.trk_max : (h.inst_obs_on ? h.inst_obs_max : h.n_obstacles);
  c.goal_form = h.gtrk_on;
  c.track_form = h.trk_on || h.gtrk_on;
  c.walls = (h.wtrk_on || h.fleet_on) ? 2 : (h.n_walls > 0 ? 1 : 0);
  const size_t own_lds = barebone_lds(h.T, c.kmax, c.track_form, c.goal_form);
  if (h.footprint > 0 || h.rings > 0 || h.grid) {
    c.family = kBareboneCrowd;
    c.track_form = true;
    c.chunk = crowd_chunk(h.crowd_waves);
    c.lds = crowd_lds(h.T, c.chunk, c.walls != 0, 0, h.footprint > 0 || h.grid, h.rings, h.grid);
    return c;
  }
  if (crowd_launch(h, c.kmax, own_lds)) {
    c.family = kBareboneCrowd;
    return c;
  }
  c.kd = !h.rot ? -1 : (c.kmax <= 2 ? 2 : (c.kmax <= 4 ? 4 : -1));
  if (c.track_form && c.kd > 0 && barebone_lds(h.T, c.kd, true, c.goal_form) > kBareboneLdsMax) c.kd = -1;  // (a long horizon)
  size_t checked;  // the size held against the limit
  if (c.track_form || h.batched) {
    checked = c.lds = barebone_lds(h.T, c.kd > 0 ? c.kd : c.kmax, c.track_form, c.goal_form);
  } else {  // the classic single launch of a static set: checked without the padding, launched with it on top
    checked = own_lds;
    c.lds = barebone_lds(h.T, c.kmax, false, false, /*spare_slots=*/std::max(0, c.kd));
  }
  if (checked > kBareboneLdsMax) {
    c.family = kBareboneRefused;
    c.limit = c.goal_form ? kLimitGoalTrack : (c.track_form ? kLimitDiscTracks : kLimitStaticDiscs);
  }
  return c;
}

// The form of a crowd launch: which instantiation of k_rollout_barebone_crowd<EXACT, ROT, BATCHED, TRACKS, WALLS, pack...>
// a choice of the crowd family runs, and what the launcher (launch_barebone_crowd of barebone_launch.h) does to the
// arguments on the way.  The pack is in one order -- walls, goal, samples or rings, footprint, grid:
//   walls      kCrowdWallsStatic: one CrowdWalls; kCrowdWallsTracks: one CrowdWallTracks; none: no argument, WALLS = false
//   goal       one GoalRows
//   samples    one CrowdSamples
//   rings      one CrowdRings (never beside samples: the hand-over keeps them apart)
//   footprint  one CrowdFootprint
//   grid       one CrowdGrid (always behind a CrowdFootprint, never beside samples)
// and THE TABLE OF FORMS is crowd_form_legal: every combination of ROT, TRACKS, the wall kind and the goal without samples,
// rings and footprint (12 per ROT), and under any of those three TRACKS forms only, never CrowdWalls (2 wall kinds x goal x
// {samples, rings, neither} x footprint, less the plain one: 20 per ROT).  ROT exists under exact math only, so the library
// holds 64 forms per BATCHED with EXACT and 32 without: 192.  tests/test_barebone_form_plan.py pins the table.
// The grid forms on top: TRACKS forms with a CrowdFootprint, 2 wall kinds x goal x rings = 8 per ROT, 48 in the library:
// 240.  tests/test_occupancy_plan.py pins those.
enum CrowdWallKind { kCrowdWallsNone = 0, kCrowdWallsStatic = 1, kCrowdWallsTracks = 2 };
struct CrowdForm {
  bool rot = false;     // ROT: (cos, sin) by rotation
  bool tracks = false;  // TRACKS: the discs as rows, one per step
  CrowdWallKind walls = kCrowdWallsNone;
  bool goal = false, samples = false, rings = false, footprint = false;
  bool grid = false;      // an occupancy grid: one CrowdGrid, last of the pack
  bool disc_row = false;  // static discs run as tracks of one row: DevParams::track_rows = 1
  bool wall_row = false;  // static shared walls run as wall tracks of one row: their [wall] array is the [row][wall] array
};
constexpr bool crowd_form_legal(const CrowdForm& f) {
  const bool extra = f.samples || f.rings || f.footprint || f.grid;
  return !(f.samples && f.rings) && (!extra || (f.tracks && f.walls != kCrowdWallsStatic)) && (!f.grid || (f.footprint && !f.samples));
}

// The normalisation rules.  Samples, a footprint and rings run as TRACKS forms: static discs become tracks of one row (the
// samples are rows already), static shared walls wall tracks of one row.  rot: (cos, sin) by rotation -- launch_rollout_t
// grants it under exact math only.  A grid form carries a footprint whether or not one is held.  A choice with rings or a
// grid beside samples maps to a form that is not legal; the launcher refuses.
inline CrowdForm crowd_form(const BareboneChoice& c, bool rot) {
  CrowdForm f;
  f.rot = rot;
  f.goal = c.goal_form;
  f.samples = c.samples > 0;
  f.rings = c.rings > 0;
  f.grid = c.grid;
  f.footprint = c.footprint > 0 || c.grid;
  const bool extra = f.samples || f.rings || f.footprint;
  f.tracks = c.discs == kDiscsTracks || extra;
  f.disc_row = extra && c.discs != kDiscsTracks && c.discs != kDiscsSamples;
  f.wall_row = extra && c.walls == 1;
  f.walls = c.walls == 0 ? kCrowdWallsNone : (c.walls == 2 || extra ? kCrowdWallsTracks : kCrowdWallsStatic);
  return f;
}
