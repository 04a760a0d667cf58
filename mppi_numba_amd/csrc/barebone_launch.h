// barebone_launch.h -- the rollout launches of the barebone mode: barebone_choose (barebone_plan.h) decides, one launcher
// per kernel family carries the choice out.  Included by launch_plan.h, between its launch helpers and launch_rollout_t.
//
// The default family, k_rollout_barebone (rollout_kernels.h): one workgroup per tile of 64 rollouts; on a batched handle one
// launch over the B problems, one workgroup per tile of one problem.  Every problem's discs are a range of one pair of
// arrays -- the shared set, the concatenated per-problem sets or the tracks -- named by its BatchInst (note_instance_discs).
// The KD forms are chosen by the LARGEST problem's count; a smaller problem's slots past its own count hold the far,
// radius-0 disc (+0.0 added), so every problem keeps the bits of its own single-problem launch.
// The crowd family, k_rollout_barebone_crowd (rollout_crowd_kernel.h): crowd mode from kCrowdMinDiscs discs on, for sets
// that do not fit in LDS, and for every launch with walls, disc samples, a body footprint, clearance rings or an occupancy grid.  Which of its
// forms runs is crowd_form's answer (barebone_plan.h: the table of forms and the rules); launch_barebone_crowd builds the
// kernel's argument pack from it once, one crowd_append step per optional argument.
#pragma once

#include <type_traits>

#include "barebone_plan.h"

// What the choice depends on, from the handle (in the order of BareboneHeld's fields).  rot: (cos, sin) by rotation.
static void crowd_shape(const mppi_planner* p, int* waves, int* chunk);
static BareboneHeld barebone_held(const mppi_planner* p, bool rot = false) {
  int W = 0, C = 0;
  crowd_shape(p, &W, &C);
  const BareboneScene& s = p->scene;
  return BareboneHeld{p->cfg.num_steps, p->inst_set, rot, s.crowd, s.shared.max, s.own.on, s.own.max,
                      s.tracks.on, s.tracks.max, s.tracks.rows, s.walls.max, s.wall_tracks.on, s.fleet.on(), s.goal.on || s.guide.on,
                      s.samples.on ? s.samples.count : 0, s.samples.discs, s.samples.rows, W, s.footprint.count, s.rings.count,
                      s.occupancy.on};
}

// The disc arrays of a choice.  Crowd family: the tracks as their [row][disc] copy.
static const DiscSet& barebone_disc_set(const mppi_planner* p, const BareboneChoice& c) {
  return c.discs == kDiscsTracks ? p->scene.tracks : (c.discs == kDiscsOwn ? p->scene.own : p->scene.shared);
}
static const float2* barebone_disc_pos(const mppi_planner* p, const BareboneChoice& c) {
  if (c.discs == kDiscsSamples) return p->scene.samples.pos_rows;
  return c.discs == kDiscsTracks && c.family == kBareboneCrowd ? p->scene.tracks.pos_rows : barebone_disc_set(p, c).pos;
}
static const float* barebone_disc_rad(const mppi_planner* p, const BareboneChoice& c) {
  return c.discs == kDiscsSamples ? p->scene.samples.r : barebone_disc_set(p, c).r;
}

// The goal tracks as a launch takes them: a batched launch reads problem b's rows at b * rows, or everybody's at 0.  While
// the guide is on (mppi_planner_set_guide) the rows are its own: T + 1 per problem, counted from "now" (relative = 1).
static int goal_rows_held(const mppi_planner* p) { return p->scene.guide.on ? p->cfg.num_steps + 1 : p->scene.goal.rows; }
template <bool BATCHED>
static GoalRows goal_rows_arg(const mppi_planner* p) {
  const int rows = goal_rows_held(p);
  if (p->scene.guide.on) return GoalRows{p->scene.guide.rows, rows, BATCHED ? rows : 0, 1};
  const GoalTracks& g = p->scene.goal;
  return GoalRows{g.xy, rows, BATCHED && g.count > 1 ? rows : 0, 0};
}
// ... and what mppi_planner_describe_last_rollout says of them
static std::string goal_rows_text(const mppi_planner* p) {
  const GuideArrays& g = p->scene.guide;
  return " goal_rows=" + std::to_string(goal_rows_held(p)) + (g.on ? " guide=" + std::to_string(g.nx) + "x" + std::to_string(g.ny) : std::string());
}

// The default family.  Static discs: <EXACT, ROT, KD, BATCHED>; disc tracks: the TRACKS forms, a row of disc slots per step;
// a goal that moves (mppi_planner_set_goal_tracks): the TRACKS forms with the goal rows as one more argument -- static discs
// are tracks of one row there (DevParams::track_rows = 1: every step's row of slots holds the same discs -- DESIGN.md
// section 8: a static disc to the bit), so the goal track costs one template flag on the track forms and no form of its own.
template <bool EXACT, bool BATCHED>
static int launch_barebone_default(mppi_planner* p, DevParams d, const BareboneChoice& c, bool rot) {
  const float2* pos = barebone_disc_pos(p, c);
  const float* rad = barebone_disc_rad(p, c);
  const bool tracks = c.discs == kDiscsTracks;
  if (c.goal_form && !tracks) d.track_rows = 1;
  const dim3 grid(ceil_div(p->n_local, 64)), block(64);
  auto launch = [&](auto rot_c, auto kd_c) {
    constexpr bool ROT = decltype(rot_c)::value;
    constexpr int KD = decltype(kd_c)::value;
    if (c.goal_form)
      MPPI_KLAUNCH((k_rollout_barebone<EXACT, ROT, KD, BATCHED, true, GoalRows>), grid, block, c.lds, p->stream, d, pos, rad,
                   p->noise, p->u, p->costs, goal_rows_arg<BATCHED>(p));
    else if (c.track_form)
      MPPI_KLAUNCH((k_rollout_barebone<EXACT, ROT, KD, BATCHED, true>), grid, block, c.lds, p->stream, d, pos, rad, p->noise,
                   p->u, p->costs);
    else
      MPPI_KLAUNCH((k_rollout_barebone<EXACT, ROT, KD, BATCHED>), grid, block, c.lds, p->stream, d, pos, rad, p->noise, p->u,
                   p->costs);
  };
  if (c.kd == 2) launch(std::true_type(), std::integral_constant<int, 2>());
  else if (c.kd == 4) launch(std::true_type(), std::integral_constant<int, 4>());
  else if (rot) launch(std::true_type(), std::integral_constant<int, -1>());
  else launch(std::false_type(), std::integral_constant<int, -1>());
  p->last_rollout = "k_rollout_barebone exact=" + std::to_string((int)EXACT) + " rotation=" + std::to_string((int)rot);
  if (BATCHED || c.track_form)  // (the classic single launch of a static set names no disc form)
    p->last_rollout += (c.kd > 0 ? " discs<=" + std::to_string(c.kd) : std::string(" discs=loop")) +
                       (tracks ? " tracks=" + std::to_string(p->scene.tracks.rows) : std::string()) +
                       (!c.track_form && c.discs == kDiscsOwn ? " own_discs=1" : "") +
                       (BATCHED ? " problems=" + std::to_string(p->B) : std::string()) +
                       (c.goal_form ? goal_rows_text(p) : std::string());
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

// W waves per workgroup and C steps per chunk.  One tile is one workgroup whatever W is, so few tiles (N = 1000: 16 on
// 256 CUs) get the whole 16 waves -- 14 counters -- and a launch that fills the device on its own gets fewer: about 32
// waves per CU in all.  C: crowd_chunk (barebone_plan.h).
static void crowd_shape(const mppi_planner* p, int* waves, int* chunk) {
  const int tiles = ceil_div(p->n_local, 64);
  const int W = std::min(kCrowdWavesMax, std::max(4, (32 * p->num_cus) / tiles));
  *waves = W;
  *chunk = crowd_chunk(W);
}

// The wall tracks as a launch takes them: the user's (rows counted from the problem's track offset), or in fleet mode the
// sets the library makes of the other problems' plans (fleet_kernels.h; rows counted from "now": relative = 1).
// (the classic single launch has one problem: the first set, which starts at wall 0)
template <bool BATCHED>
static CrowdWallTracks wall_tracks_arg(const mppi_planner* p) {
  const FleetArrays& f = p->scene.fleet;
  if (f.on()) return CrowdWallTracks{f.seg_rows, f.hw, f.range, f.slots, p->cfg.num_steps, p->B * f.slots, 1};
  const WallSet& w = p->scene.wall_tracks;
  const bool own = BATCHED && w.counts.size() > 1;
  return CrowdWallTracks{w.seg_rows, w.hw, own ? w.range : nullptr, own ? w.max : w.counts[0], w.rows, (int)w.hw_host.size(), 0};
}

// Static shared walls as wall tracks of one row (the sample, footprint and ring forms): they are held as [row][wall] of
// one row.
static CrowdWallTracks wall_row_arg(const mppi_planner* p) {
  const WallSet& w = p->scene.walls;
  return CrowdWallTracks{w.seg_rows, w.hw, nullptr, w.max, 1, w.max, 0};
}

// The disc samples as a launch takes them: the CVaR tail's length, and where the per-sample costs go while they are wanted.
static CrowdSamples samples_arg(const mppi_planner* p, const BareboneChoice& c, const DevParams& d) {
  return CrowdSamples{p->want_sample_costs ? p->sample_costs : nullptr, c.samples, cvar_numel(c.samples, d.cvar_alpha)};
}

// The body footprint as a launch takes it.  A grid form without a footprint held: the point robot as the one-disc body
// (0, 0, 0) -- the zeroed rows, one of them.
static CrowdFootprint footprint_arg(const mppi_planner* p) {
  CrowdFootprint fp{};
  const auto& held = p->scene.footprint;
  const FleetArrays& f = p->scene.fleet;
  fp.count = held.count == 0 && p->scene.occupancy.on ? 1 : held.count;
  const bool bodies = f.on() && f.body > 0;  // a body fleet: the others' slots count once per robot
  fp.group = bodies ? f.group : 1;
  fp.grouped = bodies ? (p->B - 1) * f.group : 0;
  for (int i = 0; i < held.count; ++i) {  // (the float32 rows widened here: exact, and the kernel's scalar operands as they are)
    fp.ox[i] = (double)held.host[3 * i];
    fp.oy[i] = (double)held.host[3 * i + 1];
    fp.rho[i] = (double)held.host[3 * i + 2];
  }
  return fp;
}

// The clearance rings as a launch takes them: the float32 rows widened (exact).
static CrowdRings rings_arg(const mppi_planner* p) {
  CrowdRings rg{};
  const auto& held = p->scene.rings;
  rg.count = held.count;
  for (int l = 0; l < held.count; ++l) {
    rg.margin[l] = (double)held.host[2 * l];
    rg.penalty[l] = (double)held.host[2 * l + 1];
  }
  return rg;
}

// The occupancy grid as a launch takes it: thr[i][l] of body disc i at level l (0: the hit, l >= 1: ring l), formed here once
// per launch in double on the widened float32 inputs (occupancy_threshold); the body is the one footprint_arg gives.
static CrowdGrid grid_arg(const mppi_planner* p) {
  const OccupancyArrays& o = p->scene.occupancy;
  const CrowdFootprint fp = footprint_arg(p);
  const CrowdRings rg = rings_arg(p);
  CrowdGrid g{};
  g.field = o.field;
  g.x_min = o.x_min; g.y_min = o.y_min; g.res = o.res;
  g.nx = o.nx; g.ny = o.ny; g.substeps = o.substeps;
  for (int i = 0; i < fp.count; ++i)
    for (int l = 0; l <= rg.count; ++l) g.thr[i][l] = occupancy_threshold(o.inflate, fp.rho[i], l == 0 ? 0.0 : rg.margin[l - 1], o.res);
  return g;
}

// The form a TRACKS flag and a pack of argument types name, and one optional argument of the pack: if the form has it, go on
// with it appended, else go on without.  An argument that the table (crowd_form_legal) has no form for behind the pack so
// far is never appended, so no kernel outside the table is ever named.
template <bool TRACKS, typename... Pack>
constexpr CrowdForm crowd_form_of() {
  CrowdForm f;
  f.tracks = TRACKS;
  f.walls = kCrowdWallTracks<Pack...> ? kCrowdWallsTracks : ((std::is_same_v<Pack, CrowdWalls> || ...) ? kCrowdWallsStatic : kCrowdWallsNone);
  f.goal = kGoalRows<Pack...>;
  f.samples = kCrowdSamples<Pack...>;
  f.rings = kCrowdRings<Pack...>;
  f.footprint = kCrowdFootprint<Pack...>;
  f.grid = kCrowdGrid<Pack...>;
  return f;
}
template <bool TRACKS, typename Make, typename Next, typename... Pack>
static int crowd_append(bool has, Make make, Next next, Pack... pack) {
  if constexpr (crowd_form_legal(crowd_form_of<TRACKS, Pack..., decltype(make())>())) {
    if (has) return next(pack..., make());
  }
  return has ? fail(MPPI_ERR_STATE, "crowd launch: a form outside the table of forms") : next(pack...);
}

// The crowd family: k_rollout_barebone_crowd<EXACT, ROT, BATCHED, TRACKS, WALLS, pack...>.  crowd_form (barebone_plan.h) turns
// the choice into the form -- the table of forms and every normalisation rule are there -- and the pack is built here once, in
// its one order: walls, goal, samples or rings, footprint, grid.  The disc set: the tracks ([row][disc] copy), the samples
// ([row][sample][disc]), a problem's own static set, or the shared one.  The walls: CrowdWalls, static walls shared by the
// problems; CrowdWallTracks, wall tracks and per-problem sets -- they come first: while they are held the static walls rest --,
// fleet mode, which takes the same form with the sets it makes itself, the static walls copied into them, and static walls as
// one row under samples, a footprint or rings.  Those three run with the chunk and the LDS of the choice.
template <bool EXACT, bool BATCHED>
static int launch_barebone_crowd(mppi_planner* p, DevParams d, const BareboneChoice& c, bool rot) {
  const CrowdForm f = crowd_form(c, rot);
  const BareboneScene& sc = p->scene;
  REQUIRE(!(f.rings && f.samples), MPPI_ERR_STATE, "clearance rings beside disc samples: the hand-over keeps them apart");
  REQUIRE(!(f.grid && f.samples), MPPI_ERR_STATE, "an occupancy grid beside disc samples: the hand-over keeps them apart");
  int W = 0, C = 0;
  crowd_shape(p, &W, &C);
  if (f.samples || f.footprint || f.rings) C = c.chunk;  // (the chunk of the choice: a sample form's shrinks to its LDS)
  const size_t lds = crowd_lds(p->cfg.num_steps, C, c.walls != 0, c.samples, f.footprint, c.rings, f.grid);
  const bool fits = lds <= (size_t)p->lds_per_cu;
  if (f.rings)
    REQUIRE(fits, MPPI_ERR_INVALID, "%d clearance rings and %d steps: the crowd kernel needs %zu bytes of LDS", c.rings, p->cfg.num_steps, lds);
  else if (f.footprint)
    REQUIRE(fits, MPPI_ERR_INVALID, "a footprint and %d steps: the crowd kernel needs %zu bytes of LDS", p->cfg.num_steps, lds);
  else if (f.samples)
    REQUIRE(fits, MPPI_ERR_INVALID, "%d disc samples and %d steps: the crowd kernel needs %zu bytes of LDS", c.samples, p->cfg.num_steps, lds);
  if (f.rings || f.samples) {  // (their counts of a step are 16 bits wide)
    const int walls = c.walls == 2 ? (sc.fleet.on() ? sc.fleet.slots : sc.wall_tracks.max) : (c.walls == 1 ? sc.walls.max : 0);
    const bool counted = (long)c.kmax + (long)walls + (f.grid ? 1 : 0) <= (long)kCrowdSampleHitsMax;  // (the grid is one obstacle)
    if (f.rings)
      REQUIRE(counted, MPPI_ERR_INVALID, "clearance rings: %d discs and %d walls, more than the %d a step's 16-bit counter holds", c.kmax,
              walls, kCrowdSampleHitsMax);
    else
      REQUIRE(counted, MPPI_ERR_INVALID, "disc samples: %d discs and %d walls, more than the %d hits a step's 16-bit counter holds",
              c.kmax, walls, kCrowdSampleHitsMax);
  }
  if (f.samples && p->want_sample_costs && !p->sample_costs) TRY(dev_alloc(&p->sample_costs, (size_t)p->n_local * (size_t)kCrowdSamplesMax));
  if (c.walls == 2) REQUIRE(BATCHED || !sc.fleet.on(), MPPI_ERR_STATE, "fleet mode: a launch over the problems of the batch (mppi_planner_set_instances)");
  if (c.walls != 0)  // (the launch without walls is left as it was: the attribute call below refuses what the device cannot hold)
    REQUIRE(fits, MPPI_ERR_INVALID, "%d steps and walls: the crowd kernel needs %zu bytes of LDS", p->cfg.num_steps, lds);
  if (f.disc_row) d.track_rows = 1;
  const bool tracks = c.discs == kDiscsTracks;
  const float2* pos = barebone_disc_pos(p, c);
  const float* rad = barebone_disc_rad(p, c);
  const int pitch = c.samples > 0 ? c.samples * c.kmax : (tracks ? (int)sc.tracks.r_host.size() : 0);
  const dim3 grid(ceil_div(p->n_local, 64)), block(64 * W);
  auto dispatch = [&](auto rot_c, auto tracks_c) -> int {
    constexpr bool ROT = decltype(rot_c)::value, TRACKS = decltype(tracks_c)::value;
    auto launch = [&](auto... pack) -> int {  // (without walls: the kernel and its arguments as they were before there were any)
      constexpr bool WALLS = crowd_form_of<TRACKS, decltype(pack)...>().walls != kCrowdWallsNone;
      const auto kern = &k_rollout_barebone_crowd<EXACT, ROT, BATCHED, TRACKS, WALLS, decltype(pack)...>;
      if (lds > 64 * 1024)  // (a horizon of more than ~1500 steps)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      MPPI_KLAUNCH(kern, grid, block, lds, p->stream, d, pos, rad, p->noise, p->u, p->costs, C, pitch, pack...);
      return MPPI_OK;
    };
    auto grid_l = [&](auto... pack) -> int { return crowd_append<TRACKS>(f.grid, [&] { return grid_arg(p); }, launch, pack...); };
    auto footprint = [&](auto... pack) -> int { return crowd_append<TRACKS>(f.footprint, [&] { return footprint_arg(p); }, grid_l, pack...); };
    auto rings = [&](auto... pack) -> int { return crowd_append<TRACKS>(f.rings, [&] { return rings_arg(p); }, footprint, pack...); };
    auto samples = [&](auto... pack) -> int { return crowd_append<TRACKS>(f.samples, [&] { return samples_arg(p, c, d); }, rings, pack...); };
    auto goal = [&](auto... pack) -> int { return crowd_append<TRACKS>(f.goal, [&] { return goal_rows_arg<BATCHED>(p); }, samples, pack...); };
    if (f.walls == kCrowdWallsTracks) return goal(f.wall_row ? wall_row_arg(p) : wall_tracks_arg<BATCHED>(p));
    if (f.walls == kCrowdWallsStatic) return goal(CrowdWalls{sc.walls.seg_rows, sc.walls.hw, sc.walls.max});
    return goal();
  };
  auto with_tracks = [&](auto rot_c) -> int { return f.tracks ? dispatch(rot_c, std::true_type()) : dispatch(rot_c, std::false_type()); };
  if constexpr (EXACT) TRY(f.rot ? with_tracks(std::true_type()) : with_tracks(std::false_type()));
  else TRY(with_tracks(std::false_type()));  // (ROT is exact math's alone: launch_rollout_t grants rot under it only)
  const bool fleet = c.walls == 2 && sc.fleet.on();
  p->last_rollout = "k_rollout_barebone_crowd exact=" + std::to_string((int)EXACT) + " rotation=" + std::to_string((int)rot) +
                    " waves=" + std::to_string(W) + " chunk=" + std::to_string(C) +
                    (tracks ? " tracks=" + std::to_string(p->scene.tracks.rows) : std::string()) +
                    (c.samples > 0 ? " tracks=" + std::to_string(sc.samples.rows) : std::string()) +
                    (BATCHED ? " problems=" + std::to_string(p->B) : std::string()) +
                    (c.walls == 1 ? " walls=" + std::to_string(sc.walls.max) : std::string()) +
                    (c.walls == 2 && !fleet ? " walls=" + std::to_string(sc.wall_tracks.max) + " wall_rows=" + std::to_string(sc.wall_tracks.rows) : std::string()) +
                    (fleet ? " walls=" + std::to_string(sc.fleet.slots) + " wall_rows=" + std::to_string(p->cfg.num_steps) +
                                 " fleet=" + std::to_string(p->B) : std::string()) +
                    (c.goal_form ? goal_rows_text(p) : std::string()) +
                    (c.samples > 0 ? " samples=" + std::to_string(c.samples) + " numel=" + std::to_string(cvar_numel(c.samples, d.cvar_alpha))
                                   : std::string()) +
                    (c.footprint > 0 ? " footprint=" + std::to_string(c.footprint) : std::string()) +
                    (c.rings > 0 ? " rings=" + std::to_string(c.rings) : std::string()) +
                    (c.grid ? " grid=" + std::to_string(sc.occupancy.nx) + "x" + std::to_string(sc.occupancy.ny) : std::string());
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

// A set that does not fit in 64 KiB of LDS while crowd mode is off.
static int barebone_refuse(const BareboneChoice& c, int T) {
  if (c.limit == kLimitFootprintNeedsCrowd)
    return fail(MPPI_ERR_INVALID, "a footprint of %d discs needs crowd mode: only the crowd kernel has footprint forms", c.footprint);
  if (c.limit == kLimitRingsNeedCrowd)
    return fail(MPPI_ERR_INVALID, "%d clearance rings need crowd mode: only the crowd kernel has ring forms", c.rings);
  if (c.limit == kLimitSamplesNeedCrowd)
    return fail(MPPI_ERR_INVALID, "%d disc samples need crowd mode: only the crowd kernel has sample forms", c.samples);
  if (c.limit == kLimitGoalTrack)
    return fail(MPPI_ERR_INVALID, "%d discs, %d steps and a goal track: %zu bytes, more than 64 KiB of LDS", c.kmax, T, c.lds);
  if (c.limit == kLimitDiscTracks)
    return fail(MPPI_ERR_INVALID, "%d disc tracks and %d steps: %zu bytes, more than 64 KiB of LDS", c.kmax, T, c.lds);
  return fail(MPPI_ERR_INVALID, "%d disc obstacles and %d steps: more than 64 KiB of LDS", c.kmax, T);
}

// One barebone rollout launch: fill the state, choose, refuse or launch.  rot: (cos, sin) by rotation (launch_rollout_t).
template <bool EXACT, bool BATCHED>
static int launch_barebone(mppi_planner* p, DevParams d, bool rot) {
  if (BATCHED) TRY(upload_instances(p));
  const BareboneHeld held = barebone_held(p, rot);
  const BareboneChoice c = barebone_choose(held);
  if (!BATCHED) d.n_obstacles = c.kmax;  // (the classic single launch: the count is a kernel argument, the set the one chosen)
  if (c.family == kBareboneRefused) return barebone_refuse(c, held.T);
  TRY(c.family == kBareboneCrowd ? (launch_barebone_crowd<EXACT, BATCHED>(p, d, c, rot))
                                 : (launch_barebone_default<EXACT, BATCHED>(p, d, c, rot)));
  if (d.car) p->last_rollout += " drive=car";  // (car-like steering, mppi_planner_set_drive: either family, last of the text)
  return MPPI_OK;
}
