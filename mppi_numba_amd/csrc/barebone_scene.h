// barebone_scene.h -- what a planner holds of the barebone mode's hand-overs (barebone_api.h): one owning struct per kind of
// set, instantiated as often as the kind is held, and BareboneScene with all of them.  Every struct has a release() that
// frees its device arrays; none has a destructor that calls HIP -- mppi_planner_destroy keeps its explicit order.
// The *_host members are what was handed over (an unchanged hand-over is recognised by them); a `gen` is next_generation()
// at every change and 0 while the set is off -- what the graph signature holds of the set.  Included by handles.h.
#pragma once
#include "host_common.h"
#include "barebone_plan.h"

// Discs: counts, centres [disc][row] and radii; one set for every problem (counts has one entry) or one per problem, the
// sets one after the other -- each problem's range is in its BatchInst (disc0, n_discs: note_instance_discs).  A static set
// is a set of one row.  pos_rows: the centres once more as [row][disc] (all problems' discs side by side), so that the discs
// a step of the crowd kernel tests are contiguous -- the tracks' alone, kept while crowd mode is on.
struct DiscSet {
  bool on = false;
  float2* pos = nullptr;
  float* r = nullptr;
  float2* pos_rows = nullptr;
  int rows = 0;
  int max = 0;  // the largest problem's count
  std::vector<int> counts;
  std::vector<float> pos_host, r_host;
  void release() { dev_free(pos); dev_free(r); dev_free(pos_rows); }
};

// Disc samples (mppi_planner_set_disc_track_samples; crowd mode only): `count` sampled futures of `discs` discs, `rows` rows
// each, shared by every problem.  While on they are the disc source -- the tracks' place: the shared static set rests,
// BatchInst::track_off is "now" -- and every rollout launch is a sample form of the crowd kernel.  pos_rows: [row][sample]
// [disc], so that all a step tests is contiguous; pos_host: as handed over, [sample][disc][row].  The per-sample costs go to
// mppi_planner::sample_costs ([n_local][count]) while want_sample_costs.
struct DiscSamples {
  bool on = false;
  float2* pos_rows = nullptr;
  float* r = nullptr;
  int count = 0, discs = 0, rows = 0;
  uint64_t gen = 0;
  std::vector<float> pos_host, r_host;
  void release() { dev_free(pos_rows); dev_free(r); }
};

// Walls (crowd mode only): segments (ax, ay, bx, by) as [row][wall] -- a step's walls are contiguous, all problems' walls
// side by side -- and half-widths; one set for every problem (counts has one entry) or one per problem, the sets one after
// the other with {wall0, count} per problem in `range` (wall tracks only).  seg_host: as handed over, [wall][row].
struct WallSet {
  bool on = false;
  float4* seg_rows = nullptr;
  float* hw = nullptr;
  int2* range = nullptr;
  int rows = 0;
  int max = 0;  // the largest problem's count
  uint64_t gen = 0;
  std::vector<int> counts;
  std::vector<float> seg_host, hw_host;
  void release() { dev_free(seg_rows); dev_free(hw); dev_free(range); }
};

// Fleet mode (mppi_planner_set_fleet; a batched handle in crowd mode): every problem's wall set is made of the OTHER
// problems' current plans, rebuilt on the device at the head of every call that starts iterations (fleet_kernels.h).
// seg_rows: [T][B * slots] in the layout of WallSet::seg_rows, problem a's slots at a * slots -- the B - 1 others in
// ascending order, then the static walls as they were when the storage was built (they rest while per-problem sets are held,
// so they are copied into every row here); hw: [B * slots]; range: {a * slots, slots}; plan: [B][T + 1] positions of the
// noise-free rollouts.  The rows are counted from "now" (CrowdWallTracks::relative): BatchInst::track_off is neither read for
// them nor advanced.  gen: renewed whenever the storage is rebuilt (fleet mode set, static walls changed) -- a refresh writes
// into the same arrays and changes nothing a captured launch holds.
// A body fleet (mppi_planner_set_fleet_bodies): every robot is the same `body` discs (0: a disc fleet, or none), and reader
// a's fleet slots are the others' body discs, `group` = Fp slots a robot (the count rounded up to a power of two; the padding
// slots repeat the last disc) -- (B - 1) * Fp slots, then the static walls.  The body is held as the scene's footprint as
// well, so that every launch is a footprint form with wall tracks (the reader's own body), which counts a robot once
// (CrowdFootprint::group, grouped).  heads: [B][T + 1] headings beside plan; centres: [B][T + 1][body] body disc centres.
struct FleetArrays {
  float4* seg_rows = nullptr;
  float* hw = nullptr;
  int2* range = nullptr;
  float2* plan = nullptr;
  float* heads = nullptr;
  float2* centres = nullptr;
  int slots = 0;
  int group = 1, body = 0;
  uint64_t gen = 0;
  bool on() const { return seg_rows != nullptr; }
  void release() { dev_free(seg_rows); dev_free(hw); dev_free(range); dev_free(plan); dev_free(heads); dev_free(centres); }
};

// A goal that moves (mppi_planner_set_goal_tracks): `rows` positions per track, [track][row]; one track for every problem
// (count == 1) or one per problem (count == B).  While on the rollouts measure the state after step t against row
// min(track_off + t + 1, rows - 1) and params.xgoal / BatchInst::xg, yg rest; the default family launches its track forms
// only (static discs as tracks of one row).
struct GoalTracks {
  bool on = false;
  float2* xy = nullptr;
  int rows = 0, count = 0;
  uint64_t gen = 0;
  std::vector<float> host;
  void release() { dev_free(xy); }
};

// A guide round the walls (mppi_planner_set_guide; guide_kernels.h): per problem a shortest-path field from its goal over a
// grid whose cells the shared static walls block, and T + 1 goal rows on the shortest path from its start, which the
// launches take as GoalRows (relative: counted from "now").  field: [B][ny * nx]; moves: [B][ny * nx], the move a descent
// takes from every cell; rows: [B][T + 1]; status: [B].  The parameters are as handed over; lead_u, pace_u: lead and pace in
// the field's units.  dirty: the field is rebuilt at the head of the next call that starts iterations -- set by a change of
// the guide or of the static walls; a changed goal is seen there, against goals_built, the goals of the last build.
// gen: renewed when the guide is set -- a refresh writes into the same arrays and changes nothing a captured launch holds.
struct GuideArrays {
  bool on = false;
  float x_min = 0.0f, y_min = 0.0f, res = 1.0f, inflate = 0.0f, lead = 0.0f, pace = 0.0f;
  int nx = 0, ny = 0, lead_u = 0, pace_u = 0;
  uint32_t* field = nullptr;
  uint8_t* moves = nullptr;
  float2* rows = nullptr;
  int* status = nullptr;
  uint64_t gen = 0;
  bool dirty = false;
  unsigned long long fields_built = 0;
  std::vector<float> goals_built;
  void release() { dev_free(field); dev_free(moves); dev_free(rows); dev_free(status); }
};

// An occupancy grid (mppi_planner_set_occupancy; crowd mode only; occupancy_kernels.h, occupancy_grid.h): one grid for every
// problem.  mask: the cells bit-packed, [ny][words] uint64; field: [ny][nx] uint32, the clearance field the launches read
// through CrowdGrid.  cells_host: the cells as handed over (an unchanged hand-over is recognised by them); mask_host: what
// goes to `mask` at the next build.  dirty: the field is rebuilt at the head of the next call that starts iterations -- new
// cells of the same shape land in the same arrays and change nothing a captured launch holds.  gen: renewed when the shape,
// the geometry, inflate or substeps change.
struct OccupancyArrays {
  bool on = false;
  float x_min = 0.0f, y_min = 0.0f, res = 1.0f, inflate = 0.0f;
  int nx = 0, ny = 0, substeps = 1;
  unsigned long long* mask = nullptr;
  uint32_t* field = nullptr;
  uint64_t gen = 0;
  bool dirty = false;
  unsigned long long fields_built = 0;
  std::vector<unsigned char> cells_host;
  std::vector<unsigned long long> mask_host;
  int words() const { return (nx + 63) / 64; }
  void release() { dev_free(mask); dev_free(field); }
};

// Rows that the launches take by value (crowd mode only): no device array, `count` rows of Width floats as handed over.
template <int MaxRows, int Width>
struct ValueRows {
  int count = 0;
  float host[MaxRows * Width] = {};
  uint64_t gen = 0;
  void set(const float* rows, int n, uint64_t generation) {
    memset(host, 0, sizeof(host));
    if (n > 0) memcpy(host, rows, sizeof(float) * Width * (size_t)n);
    count = n;
    gen = generation;
  }
};

struct BareboneScene {
  // the three disc sets and their precedence: while tracks.on the launches take these and neither static set (the row that is
  // "now" is BatchInst::track_off of inst_host; problem 0's for the classic single launch: make_dev_params); else a
  // problem's own set while own.on (mppi_planner_set_instance_disc_obstacles); else the shared one, of shared.max discs
  DiscSet shared, own, tracks;
  DiscSamples samples;
  // crowd mode (mppi_planner_set_crowd): no LDS limit on the disc sets; k_rollout_barebone_crowd reads them from memory
  bool crowd = false;
  // static walls shared by every problem (mppi_planner_set_walls: one row, no range; walls.max > 0: every rollout launch is a
  // wall form of the crowd kernel), and walls that move or per-problem sets (mppi_planner_set_wall_tracks), while which the
  // static walls rest; the row that is "now" is the disc tracks' BatchInst::track_off
  WallSet walls, wall_tracks;
  FleetArrays fleet;
  std::vector<float> fleet_hw_host;  // what was handed over: [B][B - 1]; a body fleet: what was made of it, [B][(B - 1) * Fp]
  double fleet_margin = 0.0;
  GoalTracks goal;
  // the guide owns the goal rows while it is on: goal tracks and the guide exclude each other
  GuideArrays guide;
  // a body footprint (mppi_planner_set_footprint; not beside the fleet, whose body fleet holds its own here): discs
  // (ox, oy, rho) in the robot frame, one footprint for every problem -- CrowdFootprint takes the rows
  ValueRows<kCrowdFootprintMax, 3> footprint;
  // clearance rings (mppi_planner_set_clearance_rings; not beside disc samples): rows (margin, penalty), one set for every
  // problem -- CrowdRings takes the rows
  ValueRows<kCrowdRingsMax, 2> rings;
  // an occupancy grid (mppi_planner_set_occupancy; not beside disc samples): one more counted obstacle of every launch, and
  // blocked cells of the guide
  OccupancyArrays occupancy;
  void release() {
    shared.release(); own.release(); tracks.release(); samples.release();
    walls.release(); wall_tracks.release(); fleet.release(); goal.release(); guide.release(); occupancy.release();
  }
};
