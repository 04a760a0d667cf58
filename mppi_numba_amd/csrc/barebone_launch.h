// barebone_launch.h -- the rollout launches of the barebone mode: barebone_choose (barebone_plan.h) decides, one launcher
// per kernel family carries the choice out.  Included by launch_plan.h, between its launch helpers and launch_rollout_t.
//
// The default family, k_rollout_barebone (rollout_kernels.h): one workgroup per tile of 64 rollouts; on a batched handle one
// launch over the B problems, one workgroup per tile of one problem.  Every problem's discs are a range of one pair of
// arrays -- the shared set, the concatenated per-problem sets or the tracks -- named by its BatchInst (note_instance_discs).
// The KD forms are chosen by the LARGEST problem's count; a smaller problem's slots past its own count hold the far,
// radius-0 disc (+0.0 added), so every problem keeps the bits of its own single-problem launch.
// The crowd family, k_rollout_barebone_crowd (rollout_crowd_kernel.h): crowd mode from kCrowdMinDiscs discs on, for sets
// that do not fit in LDS, and for every launch with walls.
#pragma once

#include <type_traits>

#include "barebone_plan.h"

// What the choice depends on, from the handle (in the order of BareboneHeld's fields).  rot: (cos, sin) by rotation.
static void crowd_shape(const mppi_planner* p, int* waves, int* chunk);
static BareboneHeld barebone_held(const mppi_planner* p, bool rot = false) {
  int W = 0, C = 0;
  crowd_shape(p, &W, &C);
  return BareboneHeld{p->cfg.num_steps, p->inst_set, rot, p->crowd, p->n_obstacles, p->inst_obs_on, p->inst_obs_max,
                      p->trk_on, p->trk_max, p->trk_rows, p->n_walls, p->wtrk_on, p->fleet_on, p->gtrk_on,
                      p->smp_on ? p->smp_count : 0, p->smp_discs, p->smp_rows, W, p->fp_count, p->ring_count};
}

// The disc arrays of a choice.  Crowd family: the tracks as their [row][disc] copy.
static const float2* barebone_disc_pos(const mppi_planner* p, const BareboneChoice& c) {
  if (c.discs == kDiscsSamples) return p->smp_pos_rows;
  if (c.discs == kDiscsTracks) return c.family == kBareboneCrowd ? p->trk_pos_rows : p->trk_pos;
  return c.discs == kDiscsOwn ? p->inst_obs_pos : p->obs_pos;
}
static const float* barebone_disc_rad(const mppi_planner* p, const BareboneChoice& c) {
  if (c.discs == kDiscsSamples) return p->smp_r;
  return c.discs == kDiscsTracks ? p->trk_r : (c.discs == kDiscsOwn ? p->inst_obs_r : p->obs_r);
}

// The goal tracks as a launch takes them: a batched launch reads problem b's rows at b * rows, or everybody's at 0.
template <bool BATCHED>
static GoalRows goal_rows_arg(const mppi_planner* p) {
  return GoalRows{p->gtrk_xy, p->gtrk_rows, BATCHED && p->gtrk_count > 1 ? p->gtrk_rows : 0};
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
                       (tracks ? " tracks=" + std::to_string(p->trk_rows) : std::string()) +
                       (!c.track_form && c.discs == kDiscsOwn ? " own_discs=1" : "") +
                       (BATCHED ? " problems=" + std::to_string(p->B) : std::string()) +
                       (c.goal_form ? " goal_rows=" + std::to_string(p->gtrk_rows) : std::string());
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

// W waves per workgroup and C steps per chunk.  One tile is one workgroup whatever W is, so few tiles (N = 1000: 16 on
// 256 CUs) get the whole 16 waves -- 14 counters -- and a launch that fills the device on its own gets fewer: about 32
// waves per CU in all.  C: the largest multiple of the counters within kCrowdChunkMax, every counter the same share.
static void crowd_shape(const mppi_planner* p, int* waves, int* chunk) {
  const int tiles = ceil_div(p->n_local, 64);
  const int W = std::min(kCrowdWavesMax, std::max(4, (32 * p->num_cus) / tiles));
  *waves = W;
  *chunk = (kCrowdChunkMax / std::min(W - 2, kCrowdChunkMax)) * std::min(W - 2, kCrowdChunkMax);
}
// (barebone_plan.h restates the chunk and the LDS formula for the host: a sample form's chunk is chosen there)
static_assert(kCrowdChunkSteps == kCrowdChunkMax, "barebone_plan.h and rollout_crowd_kernel.h disagree on the chunk");
static_assert(kCrowdFootprintMax * 3 == sizeof(mppi_planner::fp_host) / sizeof(float), "handles.h and rollout_crowd_kernel.h disagree on the footprint");
static_assert(crowd_lds_bytes(37, 14, true, 3, true) == 16 * 37 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 3 * 64 * 2 + 3 * 64 * 4 + 8 + 2 * 15 * 64 * 4 + 192 &&
                  crowd_lds_bytes(100, 16, false, 0, true) == 16 * 100 + 2 * 16 * 64 * (8 + 8 + 4) + 8 + 2 * 16 * 64 * 4 + 192,
              "crowd_lds_bytes: the footprint forms' layout crowd_lds (barebone_plan.h) restates");
static_assert(kCrowdRingsMax * 2 == sizeof(mppi_planner::ring_host) / sizeof(float), "handles.h and rollout_crowd_kernel.h disagree on the rings");
static_assert(crowd_lds_bytes(37, 14, true, 0, true, 4) == 16 * 37 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 5 * 64 * 2 + 8 + 2 * 15 * 64 * 4 + 192 &&
                  crowd_lds_bytes(100, 16, false, 0, false, 1) == 16 * 100 + 2 * 16 * 64 * (8 + 8) + 2 * 16 * 2 * 64 * 2 + 8,
              "crowd_lds_bytes: the ring forms' layout crowd_lds (barebone_plan.h) restates");
static_assert(crowd_lds_bytes(37, 14, true, 3) == 16 * 37 + 2 * 14 * 64 * 8 + 2 * 15 * 64 * 8 + 2 * 14 * 3 * 64 * 2 + 3 * 64 * 4 + 8 &&
                  crowd_lds_bytes(100, 16, false) == 16 * 100 + 2 * 16 * 64 * (8 + 8 + 4) + 8,
              "crowd_lds_bytes: the layout crowd_lds (barebone_plan.h) restates");

// The wall tracks as a launch takes them: the user's (rows counted from the problem's track offset), or in fleet mode the
// sets the library makes of the other problems' plans (fleet_kernels.h; rows counted from "now": relative = 1).
// (the classic single launch has one problem: the first set, which starts at wall 0)
template <bool BATCHED>
static CrowdWallTracks wall_tracks_arg(const mppi_planner* p) {
  if (p->fleet_on)
    return CrowdWallTracks{p->fleet_seg_rows, p->fleet_hw, p->fleet_range, p->fleet_slots, p->cfg.num_steps, p->B * p->fleet_slots, 1};
  const bool own = BATCHED && p->wtrk_counts_host.size() > 1;
  return CrowdWallTracks{p->wtrk_seg_rows, p->wtrk_hw, own ? p->wtrk_range : nullptr,
                         own ? p->wtrk_max : p->wtrk_counts_host[0], p->wtrk_rows, (int)p->wtrk_hw_host.size(), 0};
}

// The crowd family: k_rollout_barebone_crowd<EXACT, ROT, BATCHED, TRACKS, WALLS, wall argument, goal argument>.
// The disc set: the tracks ([row][disc] copy), a problem's own static set, or the shared one.  The wall form of the
// choice: 1, static walls shared by the problems (CrowdWalls), whatever the discs are; 2, wall tracks and per-problem sets
// (CrowdWallTracks) -- they come first: while they are held the static walls rest -- and fleet mode, which takes the same
// form with the sets it makes itself, the static walls copied into them.  A goal that moves: one GoalRows argument
// more, behind the walls'.  Disc samples (mppi_planner_set_disc_track_samples): the sample forms, one CrowdSamples argument
// at the end -- TRACKS forms over the [row][sample][disc] copy, with the chunk and the LDS of the choice.  A body footprint
// (mppi_planner_set_footprint): the footprint forms, one CrowdFootprint argument behind everything else -- TRACKS forms
// whatever the discs are (static discs: tracks of one row, DevParams::track_rows = 1, as the default family's goal forms
// take them), static shared walls as wall tracks of one row, with or without a CrowdSamples argument.
static CrowdFootprint footprint_arg(const mppi_planner* p) {
  CrowdFootprint fp{};
  fp.count = p->fp_count;
  const bool bodies = p->fleet_on && p->fleet_body > 0;  // a body fleet: the others' slots count once per robot
  fp.group = bodies ? p->fleet_group : 1;
  fp.grouped = bodies ? (p->B - 1) * p->fleet_group : 0;
  for (int i = 0; i < p->fp_count; ++i) {  // (the float32 rows widened here: exact, and the kernel's scalar operands as they are)
    fp.ox[i] = (double)p->fp_host[3 * i];
    fp.oy[i] = (double)p->fp_host[3 * i + 1];
    fp.rho[i] = (double)p->fp_host[3 * i + 2];
  }
  return fp;
}

// The clearance rings as a launch takes them: the float32 rows widened (exact).
static CrowdRings rings_arg(const mppi_planner* p) {
  CrowdRings rg{};
  rg.count = p->ring_count;
  for (int l = 0; l < p->ring_count; ++l) {
    rg.margin[l] = (double)p->ring_host[2 * l];
    rg.penalty[l] = (double)p->ring_host[2 * l + 1];
  }
  return rg;
}

template <bool EXACT, bool BATCHED>
static int launch_barebone_crowd(mppi_planner* p, DevParams d, const BareboneChoice& c, bool rot) {
  int W = 0, C = 0;
  crowd_shape(p, &W, &C);
  if (c.samples > 0 || c.footprint > 0 || c.rings > 0) C = c.chunk;  // (a sample form: the chunk of the choice, shrunk to its LDS)
  const size_t lds = crowd_lds_bytes(p->cfg.num_steps, C, c.walls != 0, c.samples, c.footprint > 0, c.rings);  // the size launched
  if (c.rings > 0) {
    REQUIRE(c.samples == 0, MPPI_ERR_STATE, "clearance rings beside disc samples: the hand-over keeps them apart");
    REQUIRE(lds == c.lds && lds == crowd_lds(p->cfg.num_steps, C, c.walls != 0, 0, c.footprint > 0, c.rings), MPPI_ERR_STATE,
            "clearance rings: the choice and the kernel disagree on the LDS (%zu, %zu bytes)", c.lds, lds);
    REQUIRE(lds <= (size_t)p->lds_per_cu, MPPI_ERR_INVALID, "%d clearance rings and %d steps: the crowd kernel needs %zu bytes of LDS",
            c.rings, p->cfg.num_steps, lds);
    const int walls = c.walls == 2 ? (p->fleet_on ? p->fleet_slots : p->wtrk_max) : (c.walls == 1 ? p->n_walls : 0);
    REQUIRE((long)c.kmax + (long)walls <= (long)kCrowdSampleHitsMax, MPPI_ERR_INVALID,
            "clearance rings: %d discs and %d walls, more than the %d a step's 16-bit counter holds", c.kmax, walls, kCrowdSampleHitsMax);
    if (c.discs != kDiscsTracks) d.track_rows = 1;  // (static discs: tracks of one row)
  }
  if (c.footprint > 0) {
    REQUIRE(lds == c.lds && lds == crowd_lds(p->cfg.num_steps, C, c.walls != 0, c.samples, true, c.rings), MPPI_ERR_STATE,
            "footprint: the choice and the kernel disagree on the LDS (%zu, %zu bytes)", c.lds, lds);
    REQUIRE(lds <= (size_t)p->lds_per_cu, MPPI_ERR_INVALID, "a footprint and %d steps: the crowd kernel needs %zu bytes of LDS",
            p->cfg.num_steps, lds);
    if (c.discs != kDiscsTracks && c.discs != kDiscsSamples) d.track_rows = 1;  // (static discs: tracks of one row)
  }
  if (c.samples > 0) {
    REQUIRE(lds == c.lds && lds == crowd_lds(p->cfg.num_steps, C, c.walls != 0, c.samples, c.footprint > 0), MPPI_ERR_STATE,
            "disc samples: the choice and the kernel disagree on the LDS (%zu, %zu bytes)", c.lds, lds);
    REQUIRE(lds <= (size_t)p->lds_per_cu, MPPI_ERR_INVALID, "%d disc samples and %d steps: the crowd kernel needs %zu bytes of LDS",
            c.samples, p->cfg.num_steps, lds);
    const int walls = c.walls == 2 ? (p->fleet_on ? p->fleet_slots : p->wtrk_max) : (c.walls == 1 ? p->n_walls : 0);
    REQUIRE((long)c.kmax + (long)walls <= (long)kCrowdSampleHitsMax, MPPI_ERR_INVALID,
            "disc samples: %d discs and %d walls, more than the %d hits a step's 16-bit counter holds", c.kmax, walls, kCrowdSampleHitsMax);
    if (p->want_sample_costs && !p->sample_costs) TRY(dev_alloc(&p->sample_costs, (size_t)p->n_local * (size_t)kCrowdSamplesMax));
  }
  if (c.walls == 2) REQUIRE(BATCHED || !p->fleet_on, MPPI_ERR_STATE, "fleet mode: a launch over the problems of the batch (mppi_planner_set_instances)");
  if (c.walls != 0)  // (the launch without walls is left as it was: the attribute call below refuses what the device cannot hold)
    REQUIRE(lds <= (size_t)p->lds_per_cu, MPPI_ERR_INVALID, "%d steps and walls: the crowd kernel needs %zu bytes of LDS", p->cfg.num_steps, lds);
  const bool tracks = c.discs == kDiscsTracks;
  const float2* pos = barebone_disc_pos(p, c);
  const float* rad = barebone_disc_rad(p, c);
  const int pitch = c.samples > 0 ? c.samples * c.kmax : (tracks ? (int)p->trk_r_host.size() : 0);
  const dim3 grid(ceil_div(p->n_local, 64)), block(64 * W);
  auto launch = [&](auto kern, auto... extra) -> int {
    if (lds > 64 * 1024)  // (a horizon of more than ~1500 steps)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    MPPI_KLAUNCH(kern, grid, block, lds, p->stream, d, pos, rad, p->noise, p->u, p->costs, C, pitch, extra...);
    return MPPI_OK;
  };
  auto dispatch = [&](auto rot_c, auto tracks_c) -> int {
    constexpr bool ROT = EXACT && decltype(rot_c)::value, TRACKS = decltype(tracks_c)::value;
    auto with_walls = [&](auto... walls) -> int {  // (without walls: the kernel and its arguments as they were before there were any)
      constexpr bool WALLS = sizeof...(walls) > 0;
      if (c.goal_form)
        return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, TRACKS, WALLS, decltype(walls)..., GoalRows>, walls..., goal_rows_arg<BATCHED>(p));
      return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, TRACKS, WALLS, decltype(walls)...>, walls...);
    };
    if (c.walls == 2) return with_walls(wall_tracks_arg<BATCHED>(p));
    if (c.walls == 1) return with_walls(CrowdWalls{p->wall_seg, p->wall_hw, p->n_walls});
    return with_walls();
  };
  // disc samples: TRACKS forms with one CrowdSamples behind the other arguments; static shared walls as wall tracks of one
  // row (their [wall] array IS the [row][wall] array of one row)
  auto dispatch_samples = [&](auto rot_c) -> int {
    constexpr bool ROT = EXACT && decltype(rot_c)::value;
    const CrowdSamples smp{p->want_sample_costs ? p->sample_costs : nullptr, c.samples, cvar_numel(c.samples, d.cvar_alpha)};
    auto with_walls = [&](auto... walls) -> int {
      constexpr bool WALLS = sizeof...(walls) > 0;
      if (c.goal_form)
        return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., GoalRows, CrowdSamples>, walls...,
                      goal_rows_arg<BATCHED>(p), smp);
      return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., CrowdSamples>, walls..., smp);
    };
    if (c.walls == 2) return with_walls(wall_tracks_arg<BATCHED>(p));
    if (c.walls == 1) return with_walls(CrowdWallTracks{p->wall_seg, p->wall_hw, nullptr, p->n_walls, 1, p->n_walls, 0});
    return with_walls();
  };
  // a body footprint: TRACKS forms with one CrowdFootprint at the very end; the walls as the sample forms take them
  auto dispatch_footprint = [&](auto rot_c, auto samples_c) -> int {
    constexpr bool ROT = EXACT && decltype(rot_c)::value, SMP = decltype(samples_c)::value;
    const CrowdFootprint fp = footprint_arg(p);
    const CrowdSamples smp{p->want_sample_costs ? p->sample_costs : nullptr, c.samples, cvar_numel(std::max(c.samples, 1), d.cvar_alpha)};
    auto with_walls = [&](auto... walls) -> int {
      constexpr bool WALLS = sizeof...(walls) > 0;
      if constexpr (SMP) {
        if (c.goal_form)
          return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., GoalRows, CrowdSamples, CrowdFootprint>,
                        walls..., goal_rows_arg<BATCHED>(p), smp, fp);
        return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., CrowdSamples, CrowdFootprint>, walls..., smp, fp);
      } else {
        if (c.goal_form)
          return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., GoalRows, CrowdFootprint>, walls...,
                        goal_rows_arg<BATCHED>(p), fp);
        return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., CrowdFootprint>, walls..., fp);
      }
    };
    if (c.walls == 2) return with_walls(wall_tracks_arg<BATCHED>(p));
    if (c.walls == 1) return with_walls(CrowdWallTracks{p->wall_seg, p->wall_hw, nullptr, p->n_walls, 1, p->n_walls, 0});
    return with_walls();
  };
  // clearance rings: TRACKS forms with one CrowdRings behind the goal rows and, with a body footprint, one CrowdFootprint
  // behind that; the walls as the sample forms take them
  auto dispatch_rings = [&](auto rot_c, auto foot_c) -> int {
    constexpr bool ROT = EXACT && decltype(rot_c)::value, FOOT = decltype(foot_c)::value;
    const CrowdRings rg = rings_arg(p);
    auto with_walls = [&](auto... walls) -> int {
      constexpr bool WALLS = sizeof...(walls) > 0;
      if constexpr (FOOT) {
        const CrowdFootprint fp = footprint_arg(p);
        if (c.goal_form)
          return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., GoalRows, CrowdRings, CrowdFootprint>,
                        walls..., goal_rows_arg<BATCHED>(p), rg, fp);
        return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., CrowdRings, CrowdFootprint>, walls..., rg, fp);
      } else {
        if (c.goal_form)
          return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., GoalRows, CrowdRings>, walls...,
                        goal_rows_arg<BATCHED>(p), rg);
        return launch(&k_rollout_barebone_crowd<EXACT, ROT, BATCHED, true, WALLS, decltype(walls)..., CrowdRings>, walls..., rg);
      }
    };
    if (c.walls == 2) return with_walls(wall_tracks_arg<BATCHED>(p));
    if (c.walls == 1) return with_walls(CrowdWallTracks{p->wall_seg, p->wall_hw, nullptr, p->n_walls, 1, p->n_walls, 0});
    return with_walls();
  };
  if (c.rings > 0 && c.footprint > 0 && rot) TRY(dispatch_rings(std::true_type(), std::true_type()));
  else if (c.rings > 0 && c.footprint > 0) TRY(dispatch_rings(std::false_type(), std::true_type()));
  else if (c.rings > 0 && rot) TRY(dispatch_rings(std::true_type(), std::false_type()));
  else if (c.rings > 0) TRY(dispatch_rings(std::false_type(), std::false_type()));
  else if (c.footprint > 0 && c.samples > 0 && rot) TRY(dispatch_footprint(std::true_type(), std::true_type()));
  else if (c.footprint > 0 && c.samples > 0) TRY(dispatch_footprint(std::false_type(), std::true_type()));
  else if (c.footprint > 0 && rot) TRY(dispatch_footprint(std::true_type(), std::false_type()));
  else if (c.footprint > 0) TRY(dispatch_footprint(std::false_type(), std::false_type()));
  else if (c.samples > 0 && rot) TRY(dispatch_samples(std::true_type()));
  else if (c.samples > 0) TRY(dispatch_samples(std::false_type()));
  else if (rot && tracks) TRY(dispatch(std::true_type(), std::true_type()));
  else if (rot) TRY(dispatch(std::true_type(), std::false_type()));
  else if (tracks) TRY(dispatch(std::false_type(), std::true_type()));
  else TRY(dispatch(std::false_type(), std::false_type()));
  const bool fleet = c.walls == 2 && p->fleet_on;
  p->last_rollout = "k_rollout_barebone_crowd exact=" + std::to_string((int)EXACT) + " rotation=" + std::to_string((int)rot) +
                    " waves=" + std::to_string(W) + " chunk=" + std::to_string(C) +
                    (tracks ? " tracks=" + std::to_string(p->trk_rows) : std::string()) +
                    (c.samples > 0 ? " tracks=" + std::to_string(p->smp_rows) : std::string()) +
                    (BATCHED ? " problems=" + std::to_string(p->B) : std::string()) +
                    (c.walls == 1 ? " walls=" + std::to_string(p->n_walls) : std::string()) +
                    (c.walls == 2 && !fleet ? " walls=" + std::to_string(p->wtrk_max) + " wall_rows=" + std::to_string(p->wtrk_rows) : std::string()) +
                    (fleet ? " walls=" + std::to_string(p->fleet_slots) + " wall_rows=" + std::to_string(p->cfg.num_steps) +
                                 " fleet=" + std::to_string(p->B) : std::string()) +
                    (c.goal_form ? " goal_rows=" + std::to_string(p->gtrk_rows) : std::string()) +
                    (c.samples > 0 ? " samples=" + std::to_string(c.samples) + " numel=" + std::to_string(cvar_numel(c.samples, d.cvar_alpha))
                                   : std::string()) +
                    (c.footprint > 0 ? " footprint=" + std::to_string(c.footprint) : std::string()) +
                    (c.rings > 0 ? " rings=" + std::to_string(c.rings) : std::string());
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
  if (c.family == kBareboneCrowd) return launch_barebone_crowd<EXACT, BATCHED>(p, d, c, rot);
  return launch_barebone_default<EXACT, BATCHED>(p, d, c, rot);
}
