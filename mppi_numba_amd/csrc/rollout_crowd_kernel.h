// Crowd mode of the barebone rollout (mppi_planner_set_crowd): disc sets of any size, read from memory -- and every obstacle
// kind that is counted rather than summed: walls, clearance rings, a body footprint, sampled futures of the discs.
//
// WHY COUNTING IS ENOUGH.  k_rollout_barebone keeps a row of disc slots per step in LDS (64 KiB: 39 moving discs at T = 100)
// and, above four discs, appends one float32-rounded addition per disc and step to the one dependent chain of a lone wave.
// Three facts let the obstacles leave that chain without changing a bit of the result:
//   - a rollout's state never depends on the obstacles,
//   - an obstacle that is not hit adds +0.0 -- the identity: the running cost is never -0.0 (it starts at +0.0, and a sum is
//     -0.0 only when both terms are),
//   - every obstacle that is hit adds the same (double)obs_cost.
// So the cost after step t depends on the obstacles only through HOW MANY of them the step touches, an integer that any
// number of waves may count in any order.  (obs_cost = +-inf is where the forms part: 0.0 * inf is NaN there.)
//
// THE PIPELINE.  One workgroup of W >= 3 waves serves one tile of 64 rollouts of one problem and walks the horizon in chunks
// of C steps.  The three phases of a chunk run on different waves, and the chunks are pipelined through double-buffered
// LDS (crowd_lds, barebone_plan.h) -- in interval i of the loop, one barrier per interval:
//   walk   wave 0       chunk i      the state step of k_rollout_barebone (barebone_next_pose), state in registers across
//                                    chunks; post-step (x, y) -> LDS [step][lane]
//   count  waves 2..W-1 chunk i-1    counter q owns the chunk's steps j = q, q + (W-2), ...: a (step, lane) pair has one
//                                    owner, so there are no atomics.  Counts and the goal distance -> LDS [step][lane]
//   cost   wave 1       chunk i-2    the reference's chain: the distance term, then `hits` rounded additions of obs_cost
//                                    (a wave-uniform loop to the wave's largest count, predicated per lane), then the freeze
//                                    at the goal
// and after the last chunk wave 1 adds the terminal term and the T control-cost terms as k_rollout_barebone does.
// When every rollout of the tile has reached the goal the workgroup stops (what is left of the horizon adds nothing).
//
// WHAT THE OWNER OF A (STEP, LANE) DOES -- the walk, `while (j < cl)`, in this order:
//   1  the step's discs, 64 at a time: every lane loads one disc and its square (load_disc: a coalesced load, the next
//      tile's in flight during the tests; tracks: row min(now + t + 1, last) of the [row][disc] copy, so a step's discs are
//      contiguous), the tests read them lane by lane as wave-uniform values -- the double-precision test of
//      k_rollout_barebone on the post-step position Q, four discs a trip
//   2  behind the step's last disc tile, the walls, 64 at a time: every lane loads one wall and forms its constants
//      (load_wall: d = B - A, d.d, h * h; the next tile in flight), the tests read them lane by lane.  A wall is a segment
//      A -> B with a half-width h >= 0 (float32); step t moves the robot from P (the position before the step, x0 for
//      t = 0) to Q, and it hits the wall iff the distance between the closed segments PQ and AB is <= h: a step that jumps
//      a thin wall is a hit (no tunnelling).  crowd_wall_hit is the test: division-free, every operation in double on the
//      widened float32 inputs, no fma -- tests/wall_model.py is the same arithmetic in numpy, and tests/test_wall_model.py
//      compares it with exact rational arithmetic.  A wall hit counts like a disc hit, into the same count.
//      The counters need P as well as Q, and the position before a chunk's first step lies in the buffer the walker is
//      overwriting in that very interval -- so with walls a position buffer has C + 1 slots per lane: the walker stores
//      the chunk's entry position (x0 ahead of chunk 0) in slot 0 and the post-step positions behind it
//   3  the count store, int32 [step][lane], and the goal distance of Q
// and the cost wave reads the count where the chain wants its `hits`.  Each feature below adds to this walk and nowhere else,
// chosen by the type of an optional argument (`if constexpr`, and trip counts that are the literal 1 without the feature):
// a form without the argument holds none of the feature's code.  The text holds the walk twice: once for the forms without
// clearance rings (disc samples included) and once for the ring forms, with 1 + R counts where the other has one.
//
// STATIC WALLS, CrowdWalls (mppi_planner_set_walls): one set, shared by the problems.  The walls do not change with the
// step, so the first tile is loaded once per chunk and every step starts from it.
//
// WALL TRACKS, CrowdWallTracks (mppi_planner_set_wall_tracks): walls that move, and a wall set per problem.  Every wall has
// `rows` segments, row j the segment it occupies during control interval j (from j * dt to (j + 1) * dt after "now"); step
// t of a rollout IS interval s + t (s: the problem's track offset, the one the disc tracks have), so it is tested against
// row min(s + t, rows - 1) of every wall.  (A disc row is an instant, and the post-step position is tested against row
// s + t + 1; a wall row is an interval.  Each kind clamps against its own row count.)  The device copy is [row][wall], all
// problems' walls side by side, so a step's walls are contiguous; a problem's range of a row is {wall0, count} of the range
// array (none: one set for every problem).  The walls change with the step, so the tile in flight behind a step's last wall
// tile is the first tile of the owner's NEXT step -- as with the disc tiles.  One row, or equal rows, is a static wall to the
// bit.  A wall that itself jumps over the robot between two rows is seen only if its rows are sweeps: a row is tested where
// it lies.
//
// A GOAL THAT MOVES, GoalRows (mppi_planner_set_goal_tracks): the only reader of the goal is the walk's goal distance, once
// per (step, lane): the owner of step c0 + j takes row min(s + c0 + j + 1, rows - 1) of the problem's goal track -- a
// wave-uniform load -- where it took P.xg / P.yg.  The cost wave, the walker and the wall code do not know.
//
// A FLEET (mppi_planner_set_fleet; fleet_kernels.h): the per-problem wall sets are made by the library itself, of the
// other problems' plans, ahead of every call -- so their row 0 is always "now".  One field of CrowdWallTracks says so
// (relative): the walls' "now" is then 0 whatever the problem's track offset is, while the disc tracks and the goal track
// of the same launch keep reading theirs at the offset.  Nothing else of the kernel knows.
//
// DISC SAMPLES, CrowdSamples (mppi_planner_set_disc_track_samples): S sampled futures of the moving discs (TRACKS forms only;
// walls: the CrowdWallTracks form only, static shared walls as tracks of one row).  A rollout's cost under sample s is the
// cost of the plain launch with that sample as its tracks, bit for bit; the rollout's cost is the CVaR tail over its S costs
// (mppi.py:716-755 with block_width = S, as k_rollout_tdm restates it).  The device copy is [row][sample][disc] --
// disc_pitch = S * K: all that a step tests is contiguous.
//   count  the owner loads the position once and walks the step's S * ceil(K / 64) disc tiles, sample after sample (sm); the
//          walls are counted once, behind sample 0's last tile, and their number is added to every sample's count.  S counts
//          of 16 bits (the hand-over refuses K + walls > 65535) -> LDS [step][sample][lane], one goal distance as before.
//   cost   S chains that share nd2 and start from the same done / reached / d2 freeze; the running costs live in LDS
//          [S][64], the loop is sample-outer, steps-of-the-chunk-inner (a register array indexed by a run-time s would go
//          to scratch memory).  Without samples S is the literal 1 and the one chain is the loop's body.
//   tail   the terminal term and the T control-cost terms onto each of the S costs in the existing order; the S values to
//          the sample-cost array when recording is on; per lane a compare-exchange network over its LDS column (descending,
//          iff cvar_alpha < 1), the strided float32 tree over the first numel entries walked serially -- the tree's shape
//          fixes the bits, not who executes it --, the division in double.
//
// A BODY FOOTPRINT, CrowdFootprint (mppi_planner_set_footprint): the robot as up to kCrowdFootprintMax discs rigidly attached
// to its pose -- by value, so its rows are wave-uniform (TRACKS forms only; walls: the CrowdWallTracks form only, static
// discs and static shared walls as tracks of one row).  Body disc i = (ox, oy, rho) has its centre at
// (float)(x + (ox * c - oy * s)), (float)(y + (ox * s + oy * c)): s, c the full sincos_f64<false> of the state's float32
// heading, products and sums in double, one rounding (crowd_body_centres).
//   walk   beside each position the walker publishes the float32 heading: one more LDS plane, [2][C (+ 1)][64] float behind
//          everything else, entry slot included -- one store, nothing on the walker's dependent chain.  The count waves set
//          the pace of these forms and need the registers: the walker loads a chunk's noise at the chunk's head and carries
//          none across the barrier (the other forms keep the next chunk's in flight: 32 registers live in every wave)
//   count  the owner forms the centres of the post-step state once per step, at the step's first disc tile, and keeps them
//          in registers to its last -- loops unrolled to 8, predicated on the uniform count: a register array indexed at run
//          time would go to scratch memory.  A lane holds its disc's radius, not the square: a disc is touched iff ANY body
//          disc touches it, the test with pos := the centre and rr := (r + rho)^2 in double (crowd_body_touches), one disc a
//          trip.  A wall is hit iff ANY body disc's chord, pre-step centre -> post-step centre, hits it: crowd_wall_hit
//          unchanged with hh := (h + rho)^2.  Eight unrolled copies of that test cost some 900 bytes of scratch a lane, so
//          the walls go the other way round (crowd_body_wall_hits): a run-time loop over the body's discs around ONE copy
//          of the test, the rows read from LDS ([3][8] double behind the headings, written once), both centres formed on
//          the spot from the two states and their sines and cosines (the second sincos_f64 of a step), one bit per wall
//          OR-ed over the body.  One hit per obstacle, however many body discs reach it.  (An offset point of a turning
//          body moves on an arc; the chord is what is tested: the arc leaves it by at most |o| * (1 - cos(dt * w / 2)).)
//   cost   the cost wave, the tail and the CVaR tail do not know; the goal distance is the reference point's.
//
// A FLEET OF BODIES (mppi_planner_set_fleet_bodies; fleet_kernels.h): a footprint form with fleet wall tracks in which the
// first `grouped` walls of every problem's set are the other robots' body discs, `group` slots a robot -- a power of two, so
// a robot's slots never straddle a tile of 64.  A robot is hit iff ANY body disc of the reader hits ANY of its slots, and
// that is ONE hit: crowd_body_wall_hits folds the tile's hit mask group by group (crowd_fold.h: log2(group) shift-ORs and a
// leader mask below g = clamp(grouped - wbase, 0, 64), a population count of the rest).  Two integers by value in
// CrowdFootprint -- wave-uniform; group = 1, grouped = 0 is the plain population count.  The forms without a CrowdFootprint
// hold the empty CrowdFootprintRows.
//
// CLEARANCE RINGS, CrowdRings (mppi_planner_set_clearance_rings): a cost that rises on the way in, as a staircase -- so it
// stays a matter of counting.  R <= 4 rows (margin m_l, penalty c_l), by value, widened on the host (TRACKS forms only;
// walls: the CrowdWallTracks form only; no disc samples).  Obstacle k is NEAR at ring l iff the step would touch it were it
// m_l larger: the disc test with rr := ((double)r + m_l)^2 (a body: ((r + rho) + m_l)^2), the wall test with
// hh := ((double)h + m_l)^2 (a body: ((h + rho) + m_l)^2); a step that crosses a wall is inside every ring.
//   count  the owner forms 1 + R counts where it formed one (its own copy of the walk, with its own loaders): the hits as
//          ever and n_l, the obstacles near at ring l (the hit ones among them).  A disc's d2 is formed once and held against
//          1 + R squares, which every lane forms for its disc when the tile is loaded.  A wall's test
//          runs once as well: crowd_wall_parts gives the crossing bit and, of each of the four crowd_near calls, the pair
//          (num, den) of the branch taken -- near(hh) is num <= hh * den, den = 1.0 in the two end branches (the product is
//          exact) --, and level l's verdict is crossing || any(num_i <= hh_l * den_i): at level 0 crowd_wall_hit's on every
//          input.  (The forms without rings keep crowd_wall_hit and its short-circuit.)  A body: crowd_body_ring_touches and
//          crowd_body_wall_ring_hits, the footprint's two helpers at 1 + R sizes.  A body fleet folds each level's own
//          mask (crowd_fold_count): a robot is near once, however many of its slots are.  1 + R counts of 16 bits -> LDS
//          [step][level][lane] (the hand-over refuses K + walls > 65535).
//   cost   behind the `hits` additions of obs_cost, for l = 1 .. R, n_l rounded additions of c_l -- the same wave-uniform,
//          per-lane-predicated loop.  Repeated additions and not a product: a ring with c_l = obs_cost is a second copy of
//          the obstacles, m_l larger, to the bit.  A ring with c_l = 0 adds +0.0: the identity (see above).
//
// AN OCCUPANCY GRID, CrowdGrid (mppi_planner_set_occupancy; occupancy_grid.h, occupancy_kernels.h): a costmap as ONE more
// counted obstacle.  The launch takes the clearance field D2 -- uint32 [ny][nx], the squared distance in cells to the nearest
// occupied cell, built by k_occupancy_field ahead of the launch, 1 MiB at the cap and L2-resident -- and thr[i][l], the
// threshold of body disc i at level l (0: the hit, l >= 1: ring l), formed on the host.  A grid form is always a footprint
// form (a point robot runs as the one-disc body (0, 0, 0): its centres are the stored positions to the bit), a TRACKS form,
// never beside CrowdWalls or CrowdSamples; CrowdGrid is the last of the pack.
//   walk   the position buffer and the heading plane have the entry slot (C + 1) whether or not there are walls: with
//          substeps > 1 the counters need the pre-step pose
//   count  behind the step's last wall tile the owner walks the body's discs (a run-time loop, rows and thresholds from LDS
//          -- [8][1 + 4] uint32 behind the footprint's rows) and the M = substeps test points of each chord (occupancy_point:
//          k == M is the post-step centre itself, so M = 1 never forms the pre-step centre), finds each point's cell
//          (occupancy_cell: a point outside the grid, or a NaN, is free) and holds ONE load of D2 against the 1 + R
//          thresholds: level l is touched iff D2 <= thr[i][l] for some point of some disc.  The step's count of every level
//          touched rises by one.  M, F and 1 + R are wave-uniform; the loads are per lane
//   cost   the cost wave and the tail do not know
//
// REGISTERS.  One wall test and what the other waves keep do not fit 128 registers together: the compiler's report, gfx950,
// scratch bytes a lane over the 192 forms (zero was not reached), read from the report of the commit that merged the plain
// and the sample walk, whose figures are its parent's in every form --
//                 no footprint, no walls   no footprint, walls   footprint, no walls   footprint, walls
//   plain               0 .. 132               96 .. 248              0 .. 40             248 .. 348
//   disc samples        0 .. 128               88 .. 208              0 .. 36             248 .. 340
//   rings               0 .. 144              156 .. 284             20 .. 52             308 .. 392
// The register allocator of this kernel answers to edits that change no operation (profiles/HISTORY.md has two entries on
// it): a change of this file is compared with its parent in that report, form by form, before it is timed.
// The 48 grid forms (the commit that added them; the 192 forms above kept their registers, scratch, LDS and SGPR spills, three
// batched ring-footprint-wall forms report fewer spilled VGPRs in the same scratch) -- scratch bytes a lane:
//                 footprint + grid, no walls   footprint + grid, walls
//   plain                60 .. 104                  320 .. 408
//   rings                80 .. 128                  372 .. 468
#pragma once
#include <type_traits>

#include "barebone_plan.h"
#include "crowd_fold.h"
#include "occupancy_grid.h"
#include "rollout_kernels.h"

namespace mppi {

// kCrowdChunkMax, kCrowdFootprintMax, kCrowdRingsMax and the dynamic LDS -- crowd_lds(T, C, walls, samples, footprint,
// rings), its layout drawn beside it -- are barebone_plan.h's: the kernel's pointers below walk that layout.
constexpr int kCrowdWavesMax = 16;   // one workgroup: 1024 threads

// The walls of a launch (WALLS): seg[k] = (ax, ay, bx, by), halfwidth[k]; shared by every problem of a batch.
struct CrowdWalls {
  const float4* seg;
  const float* halfwidth;
  int count;
};

// The walls of a launch that move or differ from problem to problem (mppi_planner_set_wall_tracks): seg[row * pitch + k],
// `pitch` walls per row (the sets of all problems side by side), halfwidth[k] static per wall.  range[b] = {wall0, count}:
// problem b's walls within a row; nullptr: every problem has the walls [0, max_count).  relative != 0 (fleet mode,
// mppi_planner_set_fleet): the rows are rebuilt ahead of every call and always counted from "now" -- step t meets row
// min(t, rows - 1) whatever the problem's track offset is.
struct CrowdWallTracks {
  const float4* seg;
  const float* halfwidth;
  const int2* range;
  int max_count;  // the largest problem's count
  int rows, pitch;
  int relative;
};

// The disc samples of a launch: `count` samples, obs_pos [row][sample][disc]; the CVaR tail over the first `numel` of a
// rollout's costs (sorted descending iff DevParams::cvar_alpha < 1); sample_costs: [n][count], or nullptr (not recorded).
struct CrowdSamples {
  float* sample_costs;
  int count, numel;
};

// The body footprint of a launch: `count` discs (ox, oy, rho) in the robot frame, x along the heading, y to the left.
// A body fleet (mppi_planner_set_fleet_bodies): the first `grouped` walls of every problem's set are the other robots' body
// discs, `group` slots a robot (1, 2, 4 or 8); a robot is hit once, however many of its slots are (crowd_fold.h).  Else
// group = 1, grouped = 0: every wall counts for itself.
// (The rows are a struct of their own: a form without a footprint holds an empty CrowdFootprintRows where it always did,
// and compiles to the code it compiled to before the two integers were there.)
struct CrowdFootprintRows {
  double ox[kCrowdFootprintMax], oy[kCrowdFootprintMax], rho[kCrowdFootprintMax];  // (the float32 rows, widened on the host)
  int count;
};
struct CrowdFootprint : CrowdFootprintRows {
  int group, grouped;
};

// The clearance rings of a launch: `count` rows (margin, penalty), the float32 rows widened on the host; margins ascending.
struct CrowdRings {
  int count;
  double margin[kCrowdRingsMax], penalty[kCrowdRingsMax];
};

// The occupancy grid of a launch (mppi_planner_set_occupancy): the clearance field [ny][nx] (occupancy_kernels.h), the
// geometry, `substeps` test points per chord and thr[i][l], the threshold of body disc i at level l (0: the hit, l >= 1:
// ring l) in squared cells -- formed on the host (occupancy_threshold), non-decreasing in l; rows past the body and levels
// past the last ring are not read.
struct CrowdGrid {
  const uint32_t* field;
  float x_min, y_min, res;
  int nx, ny, substeps;
  uint32_t thr[kCrowdFootprintMax][1 + kCrowdRingsMax];
};

__device__ __forceinline__ float crowd_lane_f32(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double crowd_lane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// near(X; U, dU, LL): is the point X = U + (wx, wy) within sqrt(hh) of the segment U -> U + dU, LL = dU.dU?  By the sign
// of the projection s: before U, past U + dU, or beside the segment (squared cross product against hh * LL; no division).
// A degenerate segment (dU = 0) has s = 0: the first branch.
__device__ __forceinline__ bool crowd_near(double wx, double wy, double ux, double uy, double LL, double hh) {
  const double s = wx * ux + wy * uy;
  if (s <= 0.0) return wx * wx + wy * wy <= hh;
  if (s >= LL) {
    const double vx = wx - ux, vy = wy - uy;
    return vx * vx + vy * vy <= hh;
  }
  const double c = wx * uy - wy * ux;
  return c * c <= hh * LL;
}

// Does the step P -> Q hit the wall A -> B (d = B - A, LLd = d.d, hh = h * h)?  The segments cross (strictly opposite
// signs of the orientations, both ways) or an endpoint of one is within h of the other.
__device__ __forceinline__ bool crowd_wall_hit(double px, double py, double qx, double qy, double ax, double ay, double bx,
                                               double by, double dx, double dy, double LLd, double hh) {
  const double ex = qx - px, ey = qy - py, LLe = ex * ex + ey * ey;
  const double pax = px - ax, pay = py - ay, qax = qx - ax, qay = qy - ay;  // P - A, Q - A
  const double apx = ax - px, apy = ay - py, bpx = bx - px, bpy = by - py;  // A - P, B - P
  const double o1 = dx * pay - dy * pax, o2 = dx * qay - dy * qax;
  const double o3 = ex * apy - ey * apx, o4 = ex * bpy - ey * bpx;
  const bool crossing = ((o1 > 0.0 && o2 < 0.0) || (o1 < 0.0 && o2 > 0.0)) && ((o3 > 0.0 && o4 < 0.0) || (o3 < 0.0 && o4 > 0.0));
  return crossing || crowd_near(pax, pay, dx, dy, LLd, hh) || crowd_near(qax, qay, dx, dy, LLd, hh) ||
         crowd_near(apx, apy, ex, ey, LLe, hh) || crowd_near(bpx, bpy, ex, ey, LLe, hh);
}

// crowd_near with the half-width left open: the branch taken gives (num, den), and near(hh) is num <= hh * den -- the end
// branches have den = 1.0, where the product is hh itself; the third is crowd_near's c * c <= hh * LL as it stands.
__device__ __forceinline__ void crowd_near_parts(double wx, double wy, double ux, double uy, double LL, double& num, double& den) {
  const double s = wx * ux + wy * uy;
  if (s <= 0.0) {
    num = wx * wx + wy * wy;
    den = 1.0;
  } else if (s >= LL) {
    const double vx = wx - ux, vy = wy - uy;
    num = vx * vx + vy * vy;
    den = 1.0;
  } else {
    const double c = wx * uy - wy * ux;
    num = c * c;
    den = LL;
  }
}

// crowd_wall_hit with the half-width left open (clearance rings: one test, 1 + R verdicts): the crossing bit and the
// (num, den) pairs of its four crowd_near calls, in their order.  crowd_wall_verdict(parts, h * h) is crowd_wall_hit.
struct CrowdWallParts {
  bool crossing;
  double num[4], den[4];
};
__device__ __forceinline__ CrowdWallParts crowd_wall_parts(double px, double py, double qx, double qy, double ax, double ay,
                                                           double bx, double by, double dx, double dy, double LLd) {
  const double ex = qx - px, ey = qy - py, LLe = ex * ex + ey * ey;
  const double pax = px - ax, pay = py - ay, qax = qx - ax, qay = qy - ay;  // P - A, Q - A
  const double apx = ax - px, apy = ay - py, bpx = bx - px, bpy = by - py;  // A - P, B - P
  const double o1 = dx * pay - dy * pax, o2 = dx * qay - dy * qax;
  const double o3 = ex * apy - ey * apx, o4 = ex * bpy - ey * bpx;
  CrowdWallParts w;
  w.crossing = ((o1 > 0.0 && o2 < 0.0) || (o1 < 0.0 && o2 > 0.0)) && ((o3 > 0.0 && o4 < 0.0) || (o3 < 0.0 && o4 > 0.0));
  crowd_near_parts(pax, pay, dx, dy, LLd, w.num[0], w.den[0]);
  crowd_near_parts(qax, qay, dx, dy, LLd, w.num[1], w.den[1]);
  crowd_near_parts(apx, apy, ex, ey, LLe, w.num[2], w.den[2]);
  crowd_near_parts(bpx, bpy, ex, ey, LLe, w.num[3], w.den[3]);
  return w;
}
__device__ __forceinline__ bool crowd_wall_verdict(const CrowdWallParts& w, double hh) {
  return w.crossing || w.num[0] <= hh * w.den[0] || w.num[1] <= hh * w.den[1] || w.num[2] <= hh * w.den[2] || w.num[3] <= hh * w.den[3];
}

// The centres of the body's discs at the state (x, y, th): s, c from the full sincos_f64 (never the rotation form: the
// centres are defined on the state's rounded heading alone), products and sums in double in this order, no fma (the build
// contracts nothing), one rounding to float32.  Entries past fp.count are not touched.  s, c: kept for the walls.
__device__ __forceinline__ void crowd_body_centres(const CrowdFootprint& fp, float x, float y, float th,
                                                   float (&cx)[kCrowdFootprintMax], float (&cy)[kCrowdFootprintMax], double& s,
                                                   double& c) {
  sincos_f64<false>((double)th, s, c);
#pragma unroll
  for (int i = 0; i < kCrowdFootprintMax; ++i) {
    if (i < fp.count) {
      const double ox = fp.ox[i], oy = fp.oy[i];
      cx[i] = (float)((double)x + (ox * c - oy * s));
      cy[i] = (float)((double)y + (ox * s + oy * c));
    }
  }
}

// Does any body disc touch the disc at (ox, oy) of radius r?  The disc test of the count waves with pos := the centre and
// rr := (r + rho)^2.
__device__ __forceinline__ bool crowd_body_touches(const CrowdFootprint& fp, const float (&cx)[kCrowdFootprintMax],
                                                   const float (&cy)[kCrowdFootprintMax], float ox, float oy, double r) {
  bool any = false;
#pragma unroll
  for (int i = 0; i < kCrowdFootprintMax; ++i) {
    if (i < fp.count) {
      const double ex = (double)(cx[i] - ox), ey = (double)(cy[i] - oy);
      const double R = r + fp.rho[i];
      const double diff = fma(ex, ex, ey * ey) - R * R;
      any = any || !(diff > 0.0);
    }
  }
  return any;
}

// How many of a tile's wt walls does the body hit during a step?  Lane l of sg, dx, dy, LLd, h holds wall l (h: the
// half-width itself, the body disc's radius is added before the square).  A wall is hit iff ANY body disc's chord, its
// centre before the step -> its centre after it, hits it: one bit per wall, OR-ed over the body's discs.  The loop over
// the discs is a run-time loop around ONE copy of the wall test, so nothing here may live in a register array: the rows
// come from LDS (rows: [3][8] double, ox | oy | rho -- uniform reads) and both centres are formed on the spot from the
// two states and their sines and cosines, in crowd_body_centres' arithmetic: the same bits.
// wbase: the tile's first wall within the problem's set; the walls below `grouped` count once per aligned group of `group`
// (a body fleet: the slots of one other robot), the rest one each (crowd_fold_count; wave-uniform integers).
__device__ __forceinline__ int crowd_body_wall_hits(const double* rows, int count, float px, float py, double sp, double cp,
                                                    float qx, float qy, double sq, double cq, const float4& sg, double dx,
                                                    double dy, double LLd, double h, int wt, int wbase, int group, int grouped) {
  unsigned long long mask = 0ull;
  for (int i = 0; i < count; ++i) {
    const double ox = rows[i], oy = rows[kCrowdFootprintMax + i], rho = rows[2 * kCrowdFootprintMax + i];
    const double pcx = (double)(float)((double)px + (ox * cp - oy * sp)), pcy = (double)(float)((double)py + (ox * sp + oy * cp));
    const double qcx = (double)(float)((double)qx + (ox * cq - oy * sq)), qcy = (double)(float)((double)qy + (ox * sq + oy * cq));
    for (int l = 0; l < wt; ++l) {
      const double ax = (double)crowd_lane_f32(sg.x, l), ay = (double)crowd_lane_f32(sg.y, l);
      const double bx = (double)crowd_lane_f32(sg.z, l), by = (double)crowd_lane_f32(sg.w, l);
      const double H = crowd_lane_f64(h, l) + rho;
      if (crowd_wall_hit(pcx, pcy, qcx, qcy, ax, ay, bx, by, crowd_lane_f64(dx, l), crowd_lane_f64(dy, l), crowd_lane_f64(LLd, l), H * H))
        mask |= 1ull << l;
    }
  }
  return crowd_fold_count(mask, group, crowd_fold_span(grouped, wbase));
}

// Clearance rings: crowd_body_touches at 1 + R sizes -- n[0] takes the touch, n[l] whether any body disc is within
// ((r + rho) + m_l) of the disc.  One d2 per body disc, held against every level's square.
__device__ __forceinline__ void crowd_body_ring_touches(const CrowdFootprint& fp, const CrowdRings& rg, const float (&cx)[kCrowdFootprintMax],
                                                        const float (&cy)[kCrowdFootprintMax], float ox, float oy, double r,
                                                        int (&n)[1 + kCrowdRingsMax]) {
  bool any[1 + kCrowdRingsMax] = {};
#pragma unroll
  for (int i = 0; i < kCrowdFootprintMax; ++i) {
    if (i < fp.count) {
      const double ex = (double)(cx[i] - ox), ey = (double)(cy[i] - oy);
      const double d2 = fma(ex, ex, ey * ey), R0 = r + fp.rho[i];
      any[0] = any[0] || !(d2 - R0 * R0 > 0.0);
#pragma unroll
      for (int q = 0; q < kCrowdRingsMax; ++q) {
        if (q < rg.count) {
          const double R = R0 + rg.margin[q];
          any[q + 1] = any[q + 1] || !(d2 - R * R > 0.0);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q <= kCrowdRingsMax; ++q) n[q] += any[q] ? 1 : 0;
}

// Clearance rings: crowd_body_wall_hits at 1 + R sizes, H := ((h + rho) + m_l) per body disc chord.  Still a run-time loop
// over the body around ONE copy of the wall test (crowd_wall_parts); a mask per level, each folded on its own.
__device__ __forceinline__ void crowd_body_wall_ring_hits(const double* rows, int count, const CrowdRings& rg, float px, float py,
                                                          double sp, double cp, float qx, float qy, double sq, double cq,
                                                          const float4& sg, double dx, double dy, double LLd, double h, int wt,
                                                          int wbase, int group, int grouped, int (&n)[1 + kCrowdRingsMax]) {
  unsigned long long mask[1 + kCrowdRingsMax] = {};
  for (int i = 0; i < count; ++i) {
    const double ox = rows[i], oy = rows[kCrowdFootprintMax + i], rho = rows[2 * kCrowdFootprintMax + i];
    const double pcx = (double)(float)((double)px + (ox * cp - oy * sp)), pcy = (double)(float)((double)py + (ox * sp + oy * cp));
    const double qcx = (double)(float)((double)qx + (ox * cq - oy * sq)), qcy = (double)(float)((double)qy + (ox * sq + oy * cq));
    for (int l = 0; l < wt; ++l) {
      const double ax = (double)crowd_lane_f32(sg.x, l), ay = (double)crowd_lane_f32(sg.y, l);
      const double bx = (double)crowd_lane_f32(sg.z, l), by = (double)crowd_lane_f32(sg.w, l);
      const CrowdWallParts w = crowd_wall_parts(pcx, pcy, qcx, qcy, ax, ay, bx, by, crowd_lane_f64(dx, l), crowd_lane_f64(dy, l),
                                                crowd_lane_f64(LLd, l));
      const double H0 = crowd_lane_f64(h, l) + rho;
      if (crowd_wall_verdict(w, H0 * H0)) mask[0] |= 1ull << l;
#pragma unroll
      for (int q = 0; q < kCrowdRingsMax; ++q) {
        if (q < rg.count) {
          const double H = H0 + rg.margin[q];
          if (crowd_wall_verdict(w, H * H)) mask[q + 1] |= 1ull << l;
        }
      }
    }
  }
  const int span = crowd_fold_span(grouped, wbase);
#pragma unroll
  for (int q = 0; q <= kCrowdRingsMax; ++q) n[q] += crowd_fold_count(mask[q], group, span);  // (a level past the last: an empty mask)
}

// The occupancy grid: at which of `levels` levels (0: the hit, then the rings) does the step touch the grid?  any[l] is set
// iff some test point of some body disc's chord lies inside the grid on a cell whose clearance is within the disc's
// threshold of the level.  A run-time loop over the body around one copy of the lookup, as crowd_body_wall_hits: the rows
// and the thresholds (thr: [8][1 + 4] uint32) come from LDS, both centres are formed on the spot in crowd_body_centres'
// arithmetic -- the pre-step one only when there is a test point short of the chord's end.  The trip counts are uniform.
template <int LEVELS>
__device__ __forceinline__ void crowd_grid_touches(const CrowdGrid& g, const uint32_t* thr, const double* rows, int count, float px,
                                                   float py, double sp, double cp, float qx, float qy, double sq, double cq,
                                                   int levels, bool (&any)[LEVELS]) {
  const int M = g.substeps;
  for (int i = 0; i < count; ++i) {
    const double ox = rows[i], oy = rows[kCrowdFootprintMax + i];
    const float bx = (float)((double)qx + (ox * cq - oy * sq)), by = (float)((double)qy + (ox * sq + oy * cq));
    float ax = bx, ay = by;
    if (M > 1) {
      ax = (float)((double)px + (ox * cp - oy * sp));
      ay = (float)((double)py + (ox * sp + oy * cp));
    }
    for (int k = 1; k <= M; ++k) {
      int ix = 0, iy = 0;
      if (occupancy_cell(occupancy_point(ax, bx, k, M), g.x_min, g.res, g.nx, &ix) &&
          occupancy_cell(occupancy_point(ay, by, k, M), g.y_min, g.res, g.ny, &iy)) {
        const uint32_t d2 = g.field[(size_t)iy * (size_t)g.nx + (size_t)ix];
#pragma unroll
        for (int q = 0; q < LEVELS; ++q) {
          if (q < levels) any[q] = any[q] || d2 <= thr[i * (1 + kCrowdRingsMax) + q];
        }
      }
    }
  }
}

// The optional arguments of the kernel, one accessor each.  The walls, if there are any, are the first of the pack.
// (obs_pos: static discs [disc]; TRACKS: the [row][disc] copy of the tracks, `disc_pitch` discs per row.)
template <typename Arg>
constexpr bool kCrowdWallArg = std::is_same_v<Arg, CrowdWalls> || std::is_same_v<Arg, CrowdWallTracks>;
__device__ __forceinline__ CrowdWalls crowd_walls_of() { return CrowdWalls{nullptr, nullptr, 0}; }
template <typename First, typename... Rest>
__device__ __forceinline__ auto crowd_walls_of(const First& first, const Rest&...) {
  if constexpr (kCrowdWallArg<First>) return first;
  else return crowd_walls_of();
}
// The one order of the pack: walls, GoalRows, CrowdSamples or CrowdRings, CrowdFootprint, CrowdGrid -- each at most once,
// nothing else.
template <typename Arg>
constexpr int kCrowdArgRank = kCrowdWallArg<Arg> ? 0 : std::is_same_v<Arg, GoalRows> ? 1
                              : (std::is_same_v<Arg, CrowdSamples> || std::is_same_v<Arg, CrowdRings>) ? 2
                              : std::is_same_v<Arg, CrowdFootprint> ? 3 : std::is_same_v<Arg, CrowdGrid> ? 4 : -1;
template <typename... WallArgs>
constexpr bool crowd_pack_in_order() {
  const int ranks[] = {kCrowdArgRank<WallArgs>..., 5};
  int before = -1;
  for (int r : ranks) {
    if (r <= before) return false;
    before = r;
  }
  return true;
}
template <typename... WallArgs>
constexpr bool kCrowdRings = (std::is_same_v<WallArgs, CrowdRings> || ...);
__device__ __forceinline__ CrowdRings crowd_rings_of() { return CrowdRings{0, {}, {}}; }
template <typename First, typename... Rest>
__device__ __forceinline__ CrowdRings crowd_rings_of(const First& first, const Rest&... rest) {
  if constexpr (std::is_same_v<First, CrowdRings>) return first;
  else return crowd_rings_of(rest...);
}
template <typename... WallArgs>
constexpr bool kCrowdWallTracks = (std::is_same_v<WallArgs, CrowdWallTracks> || ...);
template <typename... WallArgs>
constexpr bool kCrowdSamples = (std::is_same_v<WallArgs, CrowdSamples> || ...);
template <typename... WallArgs>
constexpr bool kCrowdFootprint = (std::is_same_v<WallArgs, CrowdFootprint> || ...);
__device__ __forceinline__ CrowdFootprintRows crowd_footprint_of() { return CrowdFootprintRows{{}, {}, {}, 0}; }
template <typename First, typename... Rest>
__device__ __forceinline__ auto crowd_footprint_of(const First& first, const Rest&... rest) {
  if constexpr (std::is_same_v<First, CrowdFootprint>) return first;
  else return crowd_footprint_of(rest...);
}
// (what a grid form keeps of the step's pre-step heading between the walls and the grid; nothing in the other forms)
template <bool GRID>
struct CrowdGridHeading {};
template <>
struct CrowdGridHeading<true> {
  double s = 0.0, c = 1.0;
};
template <typename... WallArgs>
constexpr bool kCrowdGrid = (std::is_same_v<WallArgs, CrowdGrid> || ...);
struct CrowdNoGrid {};
__device__ __forceinline__ CrowdNoGrid crowd_grid_of() { return CrowdNoGrid{}; }
template <typename First, typename... Rest>
__device__ __forceinline__ auto crowd_grid_of(const First& first, const Rest&... rest) {
  if constexpr (std::is_same_v<First, CrowdGrid>) return first;
  else return crowd_grid_of(rest...);
}
__device__ __forceinline__ CrowdSamples crowd_samples_of() { return CrowdSamples{nullptr, 0, 1}; }
template <typename First, typename... Rest>
__device__ __forceinline__ CrowdSamples crowd_samples_of(const First& first, const Rest&... rest) {
  if constexpr (std::is_same_v<First, CrowdSamples>) return first;
  else return crowd_samples_of(rest...);
}

// WallArgs, the optional arguments, in the one order crowd_pack_in_order polices -- the table of the forms that exist is
// crowd_form_legal (barebone_plan.h), and launch_barebone_crowd (barebone_launch.h) builds the pack from it:
//   walls      nothing (WALLS = false), one CrowdWalls (WALLS = true: static walls
//              shared by the problems) or one CrowdWallTracks (WALLS = true: wall tracks, per-problem sets)
//   goal       with a goal that moves, one GoalRows
//   samples    with disc samples, one CrowdSamples (TRACKS, and no CrowdWalls), or
//   rings      with clearance rings, one CrowdRings (TRACKS, no CrowdWalls, no CrowdSamples)
//   footprint  with a body footprint, one CrowdFootprint (TRACKS, and no CrowdWalls)
//   grid       with an occupancy grid, one CrowdGrid (behind a CrowdFootprint -- a point robot is the one-disc body
//              (0, 0, 0) --, never beside CrowdSamples)
template <bool EXACT, bool ROT, bool BATCHED, bool TRACKS, bool WALLS = false, typename... WallArgs>
__global__ __launch_bounds__(64 * kCrowdWavesMax) void k_rollout_barebone_crowd(
    DevParams P, const float2* __restrict__ obs_pos, const float* __restrict__ obs_r, const float2* __restrict__ noise,
    const float2* __restrict__ u, float* __restrict__ costs, int C, int disc_pitch, WallArgs... wall_args) {
  constexpr bool GOALS = kGoalRows<WallArgs...>;
  constexpr bool SAMPLES = kCrowdSamples<WallArgs...>;
  constexpr bool FOOT = kCrowdFootprint<WallArgs...>;
  constexpr bool RINGS = kCrowdRings<WallArgs...>;
  constexpr bool GRID = kCrowdGrid<WallArgs...>;
  static_assert(sizeof...(WallArgs) == (WALLS ? 1 : 0) + (GOALS ? 1 : 0) + (SAMPLES ? 1 : 0) + (RINGS ? 1 : 0) + (FOOT ? 1 : 0) + (GRID ? 1 : 0),
                "WALLS: one CrowdWalls or CrowdWallTracks argument; a goal that moves: one GoalRows behind it; disc samples: "
                "one CrowdSamples behind that, or clearance rings: one CrowdRings; a body footprint: one CrowdFootprint "
                "behind that; an occupancy grid: one CrowdGrid behind that; else none");
  static_assert(crowd_pack_in_order<WallArgs...>(), "the pack's order: walls, GoalRows, CrowdSamples or CrowdRings, CrowdFootprint, CrowdGrid");
  constexpr bool WTRK = kCrowdWallTracks<WallArgs...>;
  static_assert(!SAMPLES || (TRACKS && WTRK == WALLS), "disc samples: TRACKS forms, walls as CrowdWallTracks");
  static_assert(!FOOT || (TRACKS && WTRK == WALLS), "a body footprint: TRACKS forms, walls as CrowdWallTracks");
  static_assert(!RINGS || (TRACKS && WTRK == WALLS && !SAMPLES), "clearance rings: TRACKS forms, walls as CrowdWallTracks, no disc samples");
  static_assert(!GRID || (FOOT && !SAMPLES), "an occupancy grid: footprint forms (a point robot: the one-disc body), no disc samples");
  [[maybe_unused]] const auto grid = crowd_grid_of(wall_args...);  // (CrowdGrid, or nothing)
  [[maybe_unused]] const CrowdRings rg = crowd_rings_of(wall_args...);
  [[maybe_unused]] const int NL = 1 + rg.count;  // RINGS: counts per (step, lane)
  [[maybe_unused]] const auto fp = crowd_footprint_of(wall_args...);  // (CrowdFootprint, or the empty rows)
  [[maybe_unused]] const CrowdSamples smp = crowd_samples_of(wall_args...);
  [[maybe_unused]] const int S = SAMPLES ? smp.count : 1;
  [[maybe_unused]] GoalRows G = goal_rows_of(wall_args...);
  [[maybe_unused]] const auto walls = crowd_walls_of(wall_args...);
  [[maybe_unused]] int wall0 = 0, wcount = 0;  // WTRK: this problem's walls within a row
  if constexpr (WTRK) wcount = walls.max_count;
  extern __shared__ double2 uos[];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, NC = ((int)blockDim.x >> 6) - 2;
  if (P.ktime && threadIdx.x == 0) P.ktime[blockIdx.x] = (unsigned long long)wall_clock64();  // (one slot per tile)
  if constexpr (BATCHED) {
    const int b = (int)blockIdx.x / P.inst_tiles;  // (uniform over the workgroup)
    u = select_instance(P, u, b);
    const BatchInst I = P.inst[b];
    obs_pos += I.disc0;
    obs_r += I.disc0;
    P.n_obstacles = I.n_discs;
    if constexpr (TRACKS || WTRK || GOALS) P.track_off = I.track_off;
    if constexpr (GOALS) G.xy += (size_t)b * (size_t)G.stride;
    if constexpr (WTRK) {
      if (walls.range) {
        const int2 r = walls.range[b];
        wall0 = r.x;
        wcount = r.y;
      }
    }
  }
  const int T = P.n_steps, K = P.n_obstacles;
  double* nd2s = reinterpret_cast<double*>(uos + T);
  constexpr int kEntry = (WALLS || GRID) ? 1 : 0;  // position slots ahead of a chunk's first step
  const int CP = C + kEntry;
  float2* poss = reinterpret_cast<float2*>(nd2s + 2 * C * 64);
  int* cnts = reinterpret_cast<int*>(poss + 2 * CP * 64);
  int* tile_done = cnts + 2 * C * 64;  // [2], used in turn: a wave still looks at one while wave 1 writes the other
  // SAMPLES: [2][C][S][64] 16-bit hits where the int hits are, the two words behind them, then [S][64] running costs
  [[maybe_unused]] unsigned short* cnts16 = reinterpret_cast<unsigned short*>(cnts);
  [[maybe_unused]] float* scost = nullptr;
  if constexpr (SAMPLES) {
    tile_done = reinterpret_cast<int*>(cnts16 + (size_t)2 * C * S * 64);
    scost = reinterpret_cast<float*>(tile_done + 2);
    if (wave == 1)  // (the cost wave's own columns: nobody else touches them)
      for (int s = 0; s < S; ++s) scost[s * 64 + lane] = 0.0f;
  }
  // RINGS: [2][C][NL][64] 16-bit counts where the int hits are, the two words behind them
  if constexpr (RINGS) tile_done = reinterpret_cast<int*>(cnts16 + (size_t)2 * C * NL * 64);
  // FOOT: [2][CP][64] float headings behind everything else, slot for slot beside the positions
  [[maybe_unused]] float* heads = nullptr;
  if constexpr (FOOT && SAMPLES) heads = scost + (size_t)S * 64;
  else if constexpr (FOOT) heads = reinterpret_cast<float*>(tile_done + 2);
  // ... and behind them the footprint's rows once more, [3][8] double: what the walls' run-time loop over the body reads
  [[maybe_unused]] double* fprows = nullptr;
  if constexpr (FOOT) {
    fprows = reinterpret_cast<double*>(heads + (size_t)2 * CP * 64);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < kCrowdFootprintMax; ++i) {
        fprows[i] = fp.ox[i];
        fprows[kCrowdFootprintMax + i] = fp.oy[i];
        fprows[2 * kCrowdFootprintMax + i] = fp.rho[i];
      }
    }
  }
  // GRID: ... and behind those the grid's thresholds, [8][1 + 4] uint32, for the same reason
  [[maybe_unused]] uint32_t* gthr = nullptr;
  if constexpr (GRID) {
    gthr = reinterpret_cast<uint32_t*>(fprows + 3 * kCrowdFootprintMax);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < kCrowdFootprintMax * (1 + kCrowdRingsMax); ++i)
        gthr[i] = grid.thr[i / (1 + kCrowdRingsMax)][i % (1 + kCrowdRingsMax)];
    }
  }
  if (threadIdx.x < 2) tile_done[threadIdx.x] = 0;
  stage_control_ratios(P, u, uos);  // (ends with a barrier)
  const int n = blockIdx.x * 64 + lane;
  const bool live = n < P.n_local;
  const int nn = live ? n : P.n_local - 1;
  const float2* col = noise + tile_index(0, nn, T);  // this lane's column; rows are 64 apart
  const int n_chunks = (T + C - 1) / C;
  // the walker's
  float x = P.x0, y = P.y0, th = P.th0;
  [[maybe_unused]] double rs = 0.0, rc = 1.0;
  float2 e_cur[kCrowdChunkMax];
  if (wave == 0) {
    if (ROT) sincos_f64<false>((double)th, rs, rc);
    if constexpr (!FOOT) {
#pragma unroll
      for (int j = 0; j < kCrowdChunkMax; ++j) e_cur[j] = col[(size_t)min(j, T - 1) * 64];
    }
  }
  // the cost wave's
  float cost = 0.0f;
  double d2 = 1e9;
  bool done = false, reached = false;
  [[maybe_unused]] const int last = P.track_rows - 1, now = min(max(P.track_off, 0), last);  // (an offset past the end: the last row)
  // ... and the walls' "now": the same raw offset against the walls' own row count (fleet rows: always row 0)
  [[maybe_unused]] int wlast = 0, wnow = 0;
  if constexpr (WTRK) {
    wlast = walls.rows - 1;
    wnow = walls.relative ? 0 : min(max(P.track_off, 0), wlast);
  }
  // ... and the goal track's
  [[maybe_unused]] int glast = 0, gnow = 0;
  if constexpr (GOALS) {
    glast = G.rows - 1;
    // (relative is 0 or 1: the mask keeps the offset or clears it -- G.relative ? 0 : min(max(P.track_off, 0), glast), in
    // the form that leaves the scratch of every goal form what it was: profiles/HISTORY.md, "Barebone guide")
    gnow = min(max(P.track_off, 0) & (G.relative - 1), glast);
  }

  for (int ph = 0; ph < n_chunks + 2; ++ph) {
    if (wave == 0) {
      if (ph < n_chunks) {  // ---- walk chunk ph
        const int c0 = ph * C, cl = min(C, T - c0);
        // the next chunk's noise is in flight during this chunk's steps.  FOOT: the count waves set the pace and need the
        // registers -- the walker loads a chunk's noise at its head and carries nothing across the barrier
        [[maybe_unused]] float2 e_nxt[kCrowdChunkMax];
        if constexpr (FOOT) {
#pragma unroll
          for (int j = 0; j < kCrowdChunkMax; ++j) e_cur[j] = col[(size_t)min(c0 + j, T - 1) * 64];
        } else {
#pragma unroll
          for (int j = 0; j < kCrowdChunkMax; ++j) e_nxt[j] = col[(size_t)min(c0 + C + j, T - 1) * 64];
        }
        float2* out = poss + (size_t)((ph & 1) * CP + kEntry) * 64 + lane;
        if constexpr (WALLS || GRID) out[-64] = make_float2(x, y);  // where the chunk's first step starts
        [[maybe_unused]] float* hout = nullptr;
        if constexpr (FOOT) hout = heads + (size_t)((ph & 1) * CP + kEntry) * 64 + lane;
        if constexpr (FOOT && (WALLS || GRID)) hout[-64] = th;  // ... and how the body lies there
#pragma unroll
        for (int j = 0; j < kCrowdChunkMax; ++j) {
          if (j < cl) {
            float nx, ny, nth;
            barebone_next_pose<EXACT, ROT>(P, u[c0 + j], e_cur[j], x, y, th, rs, rc, nx, ny, nth);
            if (ROT) rotate_sincos_f64((double)nth - (double)th, rs, rc);  // exact increment of the ROUNDED heading
            x = nx; y = ny; th = nth;  // (past the goal the state goes on -- nobody looks at it: the cost wave freezes)
            out[j * 64] = make_float2(nx, ny);
            if constexpr (FOOT) hout[j * 64] = nth;
          }
        }
        if constexpr (!FOOT) {
#pragma unroll
          for (int j = 0; j < kCrowdChunkMax; ++j) e_cur[j] = e_nxt[j];
        }
      }
    } else if (wave == 1) {
      if (ph >= 2) {  // ---- cost of chunk ph - 2
        const int c = ph - 2, c0 = c * C, cl = min(C, T - c0);
        const size_t at = (size_t)((c & 1) * C) * 64 + lane;
        // One chain per sample -- S is the literal 1 without samples --, sample-outer, steps-of-the-chunk-inner: the samples'
        // running costs live in LDS (a register array indexed by a run-time s would go to scratch memory) and pass through
        // `cost` one after the other.  The freeze is the same for every sample: each starts from the chunk's, the last one keeps it
        [[maybe_unused]] const double d2_in = d2;
        [[maybe_unused]] const bool done_in = done, reached_in = reached;
        for (int s = 0; s < S; ++s) {
          if constexpr (SAMPLES) {
            cost = scost[s * 64 + lane];
            d2 = d2_in; done = done_in; reached = reached_in;
          }
          for (int j = 0; j < cl; ++j) {
            const double nd2 = nd2s[at + j * 64];
            [[maybe_unused]] const unsigned short* cn = cnts16 + ((size_t)((c & 1) * C + j) * NL) * 64 + lane;  // RINGS: [level][lane]
            int hits;
            if constexpr (SAMPLES) hits = cnts16[(at - lane + (size_t)j * 64) * S + s * 64 + lane];
            else if constexpr (RINGS) hits = cn[0];
            else hits = cnts[at + j * 64];
            float c1 = (float)((double)cost + P.dist_weight * nd2);
            for (int h = 0; __any(h < hits); ++h)
              if (h < hits) c1 = (float)((double)c1 + (double)P.obs_cost);
            if constexpr (RINGS) {  // the rings' additions behind the hits'
#pragma unroll
              for (int q = 0; q < kCrowdRingsMax; ++q) {
                if (q < rg.count) {  // (uniform)
                  const int near = cn[(q + 1) * 64];
                  const double pen = rg.penalty[q];
                  for (int h = 0; __any(h < near); ++h)
                    if (h < near) c1 = (float)((double)c1 + pen);
                }
              }
            }
            const bool hit_goal = nd2 <= (double)P.gt2, act = !done;
            cost = act ? c1 : cost;
            d2 = act ? nd2 : d2;
            reached = reached || (act && hit_goal);
            done = done || hit_goal;
          }
          if constexpr (SAMPLES) scost[s * 64 + lane] = cost;
        }
        if (__all(done) && lane == 0) tile_done[ph & 1] = 1;
      }
    } else {
      const int c = ph - 1;
      if (c >= 0 && c < n_chunks) {  // ---- count chunk ph - 1
        const int c0 = c * C, cl = min(C, T - c0);
        const size_t at = (size_t)((c & 1) * C) * 64 + lane;
        const size_t atp = (size_t)((c & 1) * CP + kEntry) * 64 + lane;  // poss[atp + j * 64]: the position after step c0 + j
        // this lane's disc of the tile [base, base + 64) as step c0 + j sees it; past the problem's last disc: a disc
        // nobody can touch (k_rollout_barebone's far slot)
        auto load_disc = [&](int j, int sm, int base, float2& op, double& rr) {
          const int k = base + lane;
          op = make_float2(1e18f, 1e18f);
          float r = 0.0f;
          if (j < cl && k < K) {
            const float2* row = TRACKS ? obs_pos + (size_t)min(now + c0 + j + 1, last) * (size_t)disc_pitch : obs_pos;
            if constexpr (SAMPLES) row += (size_t)sm * (size_t)K;  // (the row's samples lie side by side, K discs each)
            op = row[k];
            r = obs_r[k];
          }
          if constexpr (FOOT) rr = (double)r;  // (the body discs' radii are added before the square)
          else rr = (double)r * (double)r;
        };
        // this lane's wall of the tile [wbase, wbase + 64) with its constants; past the last wall: a wall nobody can touch.
        // The walls do not change with the step: the first tile is loaded once per chunk
        [[maybe_unused]] auto load_wall = [&](int wbase, float4& sg, double& dx, double& dy, double& LLd, double& hh) {
          const int k = wbase + lane;
          sg = make_float4(1e18f, 1e18f, 1e18f, 1e18f);
          float h = 0.0f;
          if constexpr (WALLS && !WTRK) {
            if (k < walls.count) {
              sg = walls.seg[k];
              h = walls.halfwidth[k];
            }
          }
          dx = (double)sg.z - (double)sg.x;
          dy = (double)sg.w - (double)sg.y;
          LLd = dx * dx + dy * dy;
          hh = (double)h * (double)h;
        };
        // WTRK: the walls change with the step -- the tile as step c0 + wj sees it: row min(wnow + c0 + wj, wlast), the
        // problem's own range of it; the same constants, formed the same way
        [[maybe_unused]] auto load_wall_row = [&](int wj, int wbase, float4& sg, double& dx, double& dy, double& LLd, double& hh) {
          const int k = wbase + lane;
          sg = make_float4(1e18f, 1e18f, 1e18f, 1e18f);
          float h = 0.0f;
          if constexpr (WTRK) {
            if (wj < cl && k < wcount) {
              sg = walls.seg[(size_t)min(wnow + c0 + wj, wlast) * (size_t)walls.pitch + (size_t)(wall0 + k)];
              h = walls.halfwidth[wall0 + k];
            }
          }
          dx = (double)sg.z - (double)sg.x;
          dy = (double)sg.w - (double)sg.y;
          LLd = dx * dx + dy * dy;
          if constexpr (FOOT) hh = (double)h;  // (the body discs' radii are added before the square)
          else hh = (double)h * (double)h;
        };
        // FOOT: the body's centres at the post-step state of the step in hand (formed at the step's first tile, kept to its
        // last) and, for the walls, at its pre-step state
        constexpr int kLanes = FOOT ? 1 : 4;  // discs tested per trip of the test loop (a body: up to 8 tests a disc as it is)
        [[maybe_unused]] float qcx[kCrowdFootprintMax] = {}, qcy[kCrowdFootprintMax] = {};
        [[maybe_unused]] double sq = 0.0, cq = 1.0;  // (sine and cosine of the post-step heading)
        [[maybe_unused]] float4 sg0;
        [[maybe_unused]] double dx0, dy0, LLd0, hh0;
        // (RINGS: its own loaders, below -- a tile's lane holds 1 + R squares)
        if constexpr (WTRK && !RINGS) load_wall_row(wave - 2, 0, sg0, dx0, dy0, LLd0, hh0);  // (the first tile of the first step owned)
        else if constexpr (WALLS && !RINGS) load_wall(0, sg0, dx0, dy0, LLd0, hh0);
        if constexpr (RINGS) {
          // The plain walk below with 1 + R counts.  A lane holds of its disc (wall) the squares of every level, formed when
          // the tile is loaded: (r)^2 | ((double)r + m_l)^2.  A body: the size itself, the sums are formed per body disc.
          constexpr int kSq = FOOT ? 1 : 1 + kCrowdRingsMax;
          auto load_ring_disc = [&](int dj, int dbase, float2& op, double (&rr)[kSq]) {
            const int k = dbase + lane;
            op = make_float2(1e18f, 1e18f);
            float r = 0.0f;
            if (dj < cl && k < K) {
              op = obs_pos[(size_t)min(now + c0 + dj + 1, last) * (size_t)disc_pitch + (size_t)k];
              r = obs_r[k];
            }
            if constexpr (FOOT) {
              rr[0] = (double)r;
            } else {
              rr[0] = (double)r * (double)r;
#pragma unroll
              for (int q = 0; q < kCrowdRingsMax; ++q) {
                const double R = (double)r + rg.margin[q];
                rr[q + 1] = q < rg.count ? R * R : 0.0;
              }
            }
          };
          [[maybe_unused]] auto load_ring_wall = [&](int wj, int wbase, float4& sg, double& dx, double& dy, double& LLd, double (&hh)[kSq]) {
            const int k = wbase + lane;
            sg = make_float4(1e18f, 1e18f, 1e18f, 1e18f);
            float h = 0.0f;
            if constexpr (WTRK) {
              if (wj < cl && k < wcount) {
                sg = walls.seg[(size_t)min(wnow + c0 + wj, wlast) * (size_t)walls.pitch + (size_t)(wall0 + k)];
                h = walls.halfwidth[wall0 + k];
              }
            }
            dx = (double)sg.z - (double)sg.x;
            dy = (double)sg.w - (double)sg.y;
            LLd = dx * dx + dy * dy;
            if constexpr (FOOT) {
              hh[0] = (double)h;
            } else {
              hh[0] = (double)h * (double)h;
#pragma unroll
              for (int q = 0; q < kCrowdRingsMax; ++q) {
                const double H = (double)h + rg.margin[q];
                hh[q + 1] = q < rg.count ? H * H : 0.0;
              }
            }
          };
          int j = wave - 2, base = 0;
          int n[1 + kCrowdRingsMax] = {};
          float2 op;
          double rr[kSq];
          load_ring_disc(j, base, op, rr);
          [[maybe_unused]] double hq0[kSq];
          if constexpr (WALLS) load_ring_wall(wave - 2, 0, sg0, dx0, dy0, LLd0, hq0);  // (the first tile of the first step owned)
          while (j < cl) {
            int nj = j, nbase = base + 64;
            if (nbase >= K) { nj = j + NC; nbase = 0; }
            float2 op_nxt;
            double rr_nxt[kSq];
            load_ring_disc(nj, nbase, op_nxt, rr_nxt);  // (in flight during this tile's tests)
            const float2 pos = poss[atp + j * 64];
            if constexpr (FOOT) {
              if (base == 0) crowd_body_centres(fp, pos.x, pos.y, heads[atp + j * 64], qcx, qcy, sq, cq);  // (once per step)
            }
            const int kt = min(64, K - base);
            for (int l0 = 0; l0 < kt; l0 += kLanes) {
#pragma unroll
              for (int l = l0; l < l0 + kLanes; ++l) {  // (kt is not a multiple of 4: the lanes past it hold the far disc)
                const float ox = crowd_lane_f32(op.x, l), oy = crowd_lane_f32(op.y, l);
                if constexpr (FOOT) {
                  crowd_body_ring_touches(fp, rg, qcx, qcy, ox, oy, crowd_lane_f64(rr[0], l), n);
                } else {
                  const double ex = (double)(pos.x - ox), ey = (double)(pos.y - oy);
                  const double dd = fma(ex, ex, ey * ey);
#pragma unroll
                  for (int q = 0; q < kSq; ++q) {
                    if (q < NL) {
                      const double diff = dd - crowd_lane_f64(rr[q], l);
                      n[q] += (diff > 0.0) ? 0 : 1;
                    }
                  }
                }
              }
            }
            if (nj != j) {  // the step's last tile
              [[maybe_unused]] CrowdGridHeading<GRID> gh;  // GRID: sine and cosine of the heading before the step
              if constexpr (WALLS) {  // ... then this problem's walls as this step sees them, against P -> Q
                const float2 pre = poss[atp + j * 64 - 64];  // (j = 0: the entry slot)
                [[maybe_unused]] const double px = (double)pre.x, py = (double)pre.y, qx = (double)pos.x, qy = (double)pos.y;
                [[maybe_unused]] double sp = 0.0, cp = 1.0;  // FOOT: of the heading before the step
                if constexpr (FOOT) sincos_f64<false>((double)heads[atp + j * 64 - 64], sp, cp);
                if constexpr (GRID) { gh.s = sp; gh.c = cp; }
                float4 sg = sg0;
                double dx = dx0, dy = dy0, LLd = LLd0, hq[kSq];
#pragma unroll
                for (int q = 0; q < kSq; ++q) hq[q] = hq0[q];
                for (int wbase = 0; wbase < wcount; wbase += 64) {
                  float4 sg_nxt;
                  double dx_nxt, dy_nxt, LLd_nxt, hq_nxt[kSq];
                  const bool more = wbase + 64 < wcount;  // (else: the first tile of this counter's next step)
                  load_ring_wall(more ? j : nj, more ? wbase + 64 : 0, sg_nxt, dx_nxt, dy_nxt, LLd_nxt, hq_nxt);
                  const int wt = min(64, wcount - wbase);
                  if constexpr (FOOT) {
                    crowd_body_wall_ring_hits(fprows, fp.count, rg, pre.x, pre.y, sp, cp, pos.x, pos.y, sq, cq, sg, dx, dy, LLd, hq[0], wt,
                                              wbase, fp.group, fp.grouped, n);
                  } else {
                    for (int l = 0; l < wt; ++l) {
                      const double ax = (double)crowd_lane_f32(sg.x, l), ay = (double)crowd_lane_f32(sg.y, l);
                      const double bx = (double)crowd_lane_f32(sg.z, l), by = (double)crowd_lane_f32(sg.w, l);
                      const CrowdWallParts w = crowd_wall_parts(px, py, qx, qy, ax, ay, bx, by, crowd_lane_f64(dx, l),
                                                                crowd_lane_f64(dy, l), crowd_lane_f64(LLd, l));
#pragma unroll
                      for (int q = 0; q < kSq; ++q) {
                        if (q < NL) n[q] += crowd_wall_verdict(w, crowd_lane_f64(hq[q], l)) ? 1 : 0;
                      }
                    }
                  }
                  sg = sg_nxt; dx = dx_nxt; dy = dy_nxt; LLd = LLd_nxt;
#pragma unroll
                  for (int q = 0; q < kSq; ++q) hq[q] = hq_nxt[q];
                }
                sg0 = sg; dx0 = dx; dy0 = dy; LLd0 = LLd;
#pragma unroll
                for (int q = 0; q < kSq; ++q) hq0[q] = hq[q];
              }
              if constexpr (GRID) {  // ... then the grid: one more obstacle, counted once at every level it is touched at
                const float2 pre = poss[atp + j * 64 - 64];
                if constexpr (!WALLS) {
                  if (grid.substeps > 1) sincos_f64<false>((double)heads[atp + j * 64 - 64], gh.s, gh.c);
                }
                bool any[1 + kCrowdRingsMax] = {};
                crowd_grid_touches(grid, gthr, fprows, fp.count, pre.x, pre.y, gh.s, gh.c, pos.x, pos.y, sq, cq, NL, any);
#pragma unroll
                for (int q = 0; q <= kCrowdRingsMax; ++q) n[q] += any[q] ? 1 : 0;
              }
              unsigned short* cn = cnts16 + ((size_t)((c & 1) * C + j) * NL) * 64 + lane;
#pragma unroll
              for (int q = 0; q <= kCrowdRingsMax; ++q) {
                if (q < NL) cn[q * 64] = (unsigned short)n[q];
                n[q] = 0;
              }
              if constexpr (GOALS) nd2s[at + j * 64] = barebone_goal_d2(G.xy[min(gnow + c0 + j + 1, glast)], pos.x, pos.y);
              else nd2s[at + j * 64] = barebone_goal_d2(P, pos.x, pos.y);
            }
            j = nj; base = nbase; op = op_nxt;
#pragma unroll
            for (int q = 0; q < kSq; ++q) rr[q] = rr_nxt[q];
          }
        } else {
          // One walk for the plain and the sample forms: a step's S sets of discs (no samples: the one set, sm = 0), tile after
          // tile, the next tile in flight; the walls once per step, behind sample 0's last tile
          int j = wave - 2, sm = 0, base = 0, hits = 0;
          [[maybe_unused]] int whits = 0;  // SAMPLES: the step's wall hits, added to every sample's count
          float2 op;
          double rr;
          load_disc(j, sm, base, op, rr);
          while (j < cl) {
            int nj = j, nsm = sm, nbase = base + 64;
            if (nbase >= K) {
              nbase = 0;
              if constexpr (!SAMPLES) nj = j + NC;
              else if (++nsm == S) { nsm = 0; nj = j + NC; }
            }
            float2 op_nxt;
            double rr_nxt;
            load_disc(nj, nsm, nbase, op_nxt, rr_nxt);  // (in flight during this tile's tests)
            const float2 pos = poss[atp + j * 64];
            if constexpr (FOOT) {
              if ((!SAMPLES || sm == 0) && base == 0) crowd_body_centres(fp, pos.x, pos.y, heads[atp + j * 64], qcx, qcy, sq, cq);  // (once per step)
            }
            const int kt = min(64, K - base);
            for (int l0 = 0; l0 < kt; l0 += kLanes) {
#pragma unroll
              for (int l = l0; l < l0 + kLanes; ++l) {  // (kt is not a multiple of 4: the lanes past it hold the far disc)
                const float ox = crowd_lane_f32(op.x, l), oy = crowd_lane_f32(op.y, l);
                const double rrl = crowd_lane_f64(rr, l);
                if constexpr (FOOT) {
                  hits += crowd_body_touches(fp, qcx, qcy, ox, oy, rrl) ? 1 : 0;
                } else {
                  const double ex = (double)(pos.x - ox), ey = (double)(pos.y - oy);
                  const double diff = fma(ex, ex, ey * ey) - rrl;
                  hits += (diff > 0.0) ? 0 : 1;
                }
              }
            }
            if (SAMPLES ? nbase == 0 : nj != j) {  // the sample's last tile (no samples: the step's)
              [[maybe_unused]] CrowdGridHeading<GRID> gh;  // GRID: sine and cosine of the heading before the step
              if constexpr (WALLS) {
                if (!SAMPLES || sm == 0) {  // the step's walls, once, against the step's segment P -> Q
                  const float2 pre = poss[atp + j * 64 - 64];  // (j = 0: the entry slot)
                  [[maybe_unused]] const double px = (double)pre.x, py = (double)pre.y, qx = (double)pos.x, qy = (double)pos.y;
                  [[maybe_unused]] double sp = 0.0, cp = 1.0;  // FOOT: of the heading before the step
                  if constexpr (FOOT) sincos_f64<false>((double)heads[atp + j * 64 - 64], sp, cp);
                  if constexpr (GRID) { gh.s = sp; gh.c = cp; }
                  float4 sg = sg0;
                  double dx = dx0, dy = dy0, LLd = LLd0, hh = hh0;
                  if constexpr (SAMPLES) whits = 0;
                  if constexpr (WTRK) {  // this problem's walls as this step sees them
                    for (int wbase = 0; wbase < wcount; wbase += 64) {
                      float4 sg_nxt;
                      double dx_nxt, dy_nxt, LLd_nxt, hh_nxt;
                      const bool more = wbase + 64 < wcount;  // (else: the first tile of this counter's next step)
                      load_wall_row(more ? j : SAMPLES ? j + NC : nj, more ? wbase + 64 : 0, sg_nxt, dx_nxt, dy_nxt, LLd_nxt, hh_nxt);  // (in flight during this tile's tests)
                      const int wt = min(64, wcount - wbase);
                      if constexpr (FOOT) {
                        const int wh = crowd_body_wall_hits(fprows, fp.count, pre.x, pre.y, sp, cp, pos.x, pos.y, sq, cq, sg, dx, dy, LLd, hh, wt, wbase, fp.group, fp.grouped);
                        if constexpr (SAMPLES) whits += wh;
                        else hits += wh;
                      } else {
                        for (int l = 0; l < wt; ++l) {
                          const double ax = (double)crowd_lane_f32(sg.x, l), ay = (double)crowd_lane_f32(sg.y, l);
                          const double bx = (double)crowd_lane_f32(sg.z, l), by = (double)crowd_lane_f32(sg.w, l);
                          const int wh = crowd_wall_hit(px, py, qx, qy, ax, ay, bx, by, crowd_lane_f64(dx, l), crowd_lane_f64(dy, l),
                                                        crowd_lane_f64(LLd, l), crowd_lane_f64(hh, l))
                                             ? 1 : 0;
                          if constexpr (SAMPLES) whits += wh;
                          else hits += wh;
                        }
                      }
                      sg = sg_nxt; dx = dx_nxt; dy = dy_nxt; LLd = LLd_nxt; hh = hh_nxt;
                    }
                    sg0 = sg; dx0 = dx; dy0 = dy; LLd0 = LLd; hh0 = hh;
                  } else {  // static walls (never beside samples): every step starts from the chunk's first tile
                    for (int wbase = 0; wbase < walls.count; wbase += 64) {
                      float4 sg_nxt;
                      double dx_nxt, dy_nxt, LLd_nxt, hh_nxt;
                      load_wall(wbase + 64, sg_nxt, dx_nxt, dy_nxt, LLd_nxt, hh_nxt);  // (in flight during this tile's tests)
                      const int wt = min(64, walls.count - wbase);
                      for (int l = 0; l < wt; ++l) {
                        const double ax = (double)crowd_lane_f32(sg.x, l), ay = (double)crowd_lane_f32(sg.y, l);
                        const double bx = (double)crowd_lane_f32(sg.z, l), by = (double)crowd_lane_f32(sg.w, l);
                        hits += crowd_wall_hit(px, py, qx, qy, ax, ay, bx, by, crowd_lane_f64(dx, l), crowd_lane_f64(dy, l),
                                               crowd_lane_f64(LLd, l), crowd_lane_f64(hh, l))
                                    ? 1 : 0;
                      }
                      sg = sg_nxt; dx = dx_nxt; dy = dy_nxt; LLd = LLd_nxt; hh = hh_nxt;
                    }
                  }
                }
              }
              if constexpr (GRID) {  // ... then the grid: one more obstacle, one hit however many test points touch it
                const float2 pre = poss[atp + j * 64 - 64];
                if constexpr (!WALLS) {
                  if (grid.substeps > 1) sincos_f64<false>((double)heads[atp + j * 64 - 64], gh.s, gh.c);
                }
                bool any[1] = {};
                crowd_grid_touches(grid, gthr, fprows, fp.count, pre.x, pre.y, gh.s, gh.c, pos.x, pos.y, sq, cq, 1, any);
                hits += any[0] ? 1 : 0;
              }
              if constexpr (SAMPLES) cnts16[(at - lane + (size_t)j * 64) * S + sm * 64 + lane] = (unsigned short)(hits + whits);
              else cnts[at + j * 64] = hits;
              if (!SAMPLES || sm == 0) {
                if constexpr (GOALS) nd2s[at + j * 64] = barebone_goal_d2(G.xy[min(gnow + c0 + j + 1, glast)], pos.x, pos.y);
                else nd2s[at + j * 64] = barebone_goal_d2(P, pos.x, pos.y);
              }
              hits = 0;
            }
            j = nj; sm = nsm; base = nbase; op = op_nxt; rr = rr_nxt;
          }
        }
      }
    }
    __syncthreads();
    if (tile_done[ph & 1]) break;  // (uniform: every rollout of the tile is at its goal)
  }
  if (wave != 1) return;
  // The tail onto each of the S costs (S = 1: onto `cost` itself; the samples' pass through it), wave 1 alone -- no barrier:
  // the terminal term, then the T control-cost terms -- loads and products once and batched, the float32-rounded additions
  // per sample in order
  for (int s = 0; s < S; ++s) {
    if constexpr (SAMPLES) cost = scost[s * 64 + lane];
    cost = (float)((double)cost + (reached ? 0.0 : 1.0) * d2);
    if constexpr (SAMPLES) scost[s * 64 + lane] = cost;
  }
  int t0 = 0;
  for (; t0 + kNoiseBatch <= T; t0 += kNoiseBatch) {
    double cc[kNoiseBatch];
#pragma unroll
    for (int j = 0; j < kNoiseBatch; ++j) cc[j] = control_cost(P, uos[t0 + j], col[(size_t)(t0 + j) * 64]);
    for (int s = 0; s < S; ++s) {
      if constexpr (SAMPLES) cost = scost[s * 64 + lane];
#pragma unroll
      for (int j = 0; j < kNoiseBatch; ++j) cost = (float)((double)cost + cc[j]);
      if constexpr (SAMPLES) scost[s * 64 + lane] = cost;
    }
  }
  for (int t = t0; t < T; ++t) {
    const double cc = control_cost(P, uos[t], col[(size_t)t * 64]);
    for (int s = 0; s < S; ++s) {
      if constexpr (SAMPLES) cost = scost[s * 64 + lane];
      cost = (float)((double)cost + cc);
      if constexpr (SAMPLES) scost[s * 64 + lane] = cost;
    }
  }
  if constexpr (SAMPLES) {  // the CVaR over the lane's column
    if (smp.sample_costs && live)
      for (int s = 0; s < S; ++s) smp.sample_costs[(size_t)n * (size_t)S + s] = scost[s * 64 + lane];
    if (P.cvar_alpha < 1.0f) {  // descending: odd-even transposition, S rounds of compare-exchange
      for (int r = 0; r < S; ++r)
        for (int i = r & 1; i + 1 < S; i += 2) {
          const float a = scost[i * 64 + lane], b = scost[(i + 1) * 64 + lane];
          scost[i * 64 + lane] = a < b ? b : a;
          scost[(i + 1) * 64 + lane] = a < b ? a : b;
        }
    }
    const int numel = smp.numel;  // the strided float32 tree over the first numel entries (mppi.py:744-751)
    for (int st = 1; st < numel; st <<= 1)
      for (int i = 0; i + st < numel; i += 2 * st) scost[i * 64 + lane] = scost[i * 64 + lane] + scost[(i + st) * 64 + lane];
    cost = (float)((double)scost[lane] / (double)numel);
  }
  if (live) costs[n] = cost;
  if (P.ktime && lane == 0) P.ktime[P.ktime_waves + blockIdx.x] = (unsigned long long)wall_clock64();
}

}  // namespace mppi
