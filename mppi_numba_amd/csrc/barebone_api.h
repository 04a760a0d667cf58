// barebone_api.h -- the hand-overs of the barebone mode (include/mppi_hip.h): disc sets, disc tracks, crowd mode, walls,
// disc samples, wall tracks, goal tracks, fleet mode, track offsets.  Included by mppi_api.hip behind launch_plan.h.
//
// Every hand-over goes the same way: check the arguments; return at once when what is handed over is what is held
// (the Python mirror hands its arrays over with every solve: unchanged arrays cost a comparison, not a synchronisation and
// two allocations); else synchronise, build the new device arrays, and only when that has succeeded free the old ones,
// commit and drop the captured graphs, whose launches hold the arrays, the counts and the kernel form by value.  A failed
// allocation or copy leaves the handle as it was.  What is held lives in mppi_planner::scene (barebone_scene.h); behind the
// setters' own checks the way above is written once per kind of set: hand_over_discs (the shared set, the per-problem sets,
// the disc tracks), hand_over_walls (the static walls, the wall tracks), hand_over_rows (the footprint, the clearance rings).
#pragma once

// Barebone mode: every problem's range of the disc arrays its launch gets (BatchInst::disc0, n_discs) -- its own set
// (mppi_planner_set_instance_disc_obstacles) or the shared one.  Uploaded with the start states.
static void note_instance_discs(mppi_planner* p) {
  if (p->cfg.mode != MPPI_MODE_BAREBONE) return;
  const BareboneScene& s = p->scene;
  // (discs that move take the place of both static sets: mppi_planner_set_disc_tracks)
  const DiscSet& d = s.tracks.on ? s.tracks : (s.own.on ? s.own : s.shared);
  const bool own = d.counts.size() > 1;
  int k0 = 0;
  for (int b = 0; b < p->B; ++b) {
    BatchInst& I = p->inst_host[(size_t)b];
    if (s.samples.on) {  // (disc samples: one set of K discs for every problem, the samples side by side within a row)
      I.disc0 = 0;
      I.n_discs = s.samples.discs;
    } else {
      I.disc0 = own ? k0 : 0;
      I.n_discs = d.on ? d.counts[own ? (size_t)b : 0] : 0;
    }
    k0 += I.n_discs;
  }
  p->inst_dirty = true;
}

// ---- shared helpers of the hand-overs ------------------------------------------------------------------------------------
// `count` sets are handed over: none, one per problem or -- where `shared` names it ("set", "track") -- one for every problem.
static int check_set_count(const mppi_planner* p, int count, const char* shared) {
  if (shared == nullptr)
    REQUIRE(count == 0 || count == p->B, MPPI_ERR_INVALID, "count %d: must be 0 or num_instances %d", count, p->B);
  else
    REQUIRE(count == 0 || count == 1 || count == p->B, MPPI_ERR_INVALID,
            "count %d: must be 0, 1 (one %s for every problem) or num_instances %d", count, shared, p->B);
  return MPPI_OK;
}

// The sets' sizes: none negative; their total and the largest.  noun: "disc", "wall".
static int sum_counts(int count, const int* counts, const char* noun, long* total, int* largest) {
  *total = 0;
  *largest = 0;
  for (int b = 0; b < count; ++b) {
    REQUIRE(counts[b] >= 0, MPPI_ERR_INVALID, "problem %d: negative %s count %d", b, noun, counts[b]);
    *total += counts[b];
    *largest = std::max(*largest, counts[b]);
  }
  return MPPI_OK;
}

// Is what is held equal to what is handed over?  (counts, or one of the float arrays)
template <typename T>
static bool same_as_held(const std::vector<T>& held, const T* given, size_t n) {
  return held.size() == n && (n == 0 || memcmp(given, held.data(), sizeof(T) * n) == 0);
}

// n half-widths: finite and not negative.  noun: "wall", "fleet pair".
static int check_halfwidths(const float* hw, size_t n, const char* noun) {
  for (size_t k = 0; k < n; ++k)
    REQUIRE(std::isfinite(hw[k]) && hw[k] >= 0.0f, MPPI_ERR_INVALID, "%s %zu: half-width %g is negative or not finite", noun, k, (double)hw[k]);
  return MPPI_OK;
}

// n items of `rows` rows of `per_row` coordinates each: all finite.  noun: "wall", "goal track".
static int check_finite(const float* v, size_t n, size_t rows, size_t per_row, const char* noun) {
  for (size_t i = 0; i < n * rows * per_row; ++i)
    REQUIRE(std::isfinite(v[i]), MPPI_ERR_INVALID, "%s %zu, row %zu: a coordinate is not finite", noun, i / per_row / rows, i / per_row % rows);
  return MPPI_OK;
}

// The row of the tracks that is "now" (BatchInst::track_off) is one number per problem, shared by the three kinds of track;
// the disc tracks own it, then the wall tracks, then the goal tracks.  A hand-over makes row 0 "now" again
//   - when it brings tracks that move (more than one row; disc tracks: any), whatever else is held;
//   - when it clears tracks that moved and no kind that ranks above them still counts the rows:
//       disc tracks cleared   -> always (nothing ranks above them)
//       wall tracks cleared   -> unless disc tracks are held
//       goal tracks cleared   -> unless disc tracks or wall tracks of more than one row are held
//   - never when neither the old nor the new set moves (a set of one row is static: it leaves "now" alone).
enum TrackKind { kGoalTracks = 0, kWallTracks = 1, kDiscTracks = 2 };
static void reset_track_offsets(mppi_planner* p, TrackKind kind, bool moved, bool cleared) {
  const BareboneScene& s = p->scene;
  const bool above = (kind < kDiscTracks && (s.tracks.on || s.samples.on)) || (kind < kWallTracks && s.wall_tracks.on && s.wall_tracks.rows > 1);
  if (!moved || (cleared && above)) return;
  for (BatchInst& I : p->inst_host) I.track_off = 0;
  p->inst_dirty = true;
}

// Staged upload.  dev_stage: one new device array of n items (one at the least), filled from the host.  staged: runs the
// caller's sequence of them; a failure frees what the sequence had got, and the handle still holds what it held.
// The commit: the arrays are staged into a fresh struct of the set's kind (barebone_scene.h), which is completed on the
// host; the held one is released and takes the fresh one's place whole, host mirrors and all.
template <typename T>
static int dev_stage(T** fresh, const void* src, size_t n) {
  TRY(dev_alloc(fresh, n));
  if (n > 0) HIP_TRY(hipMemcpy(*fresh, src, sizeof(T) * n, hipMemcpyHostToDevice));
  return MPPI_OK;
}
template <typename Stage, typename... T>
static int staged(Stage&& stage, T*&... fresh) {
  const int rc = stage();
  if (rc != MPPI_OK) (dev_free(fresh), ...);
  return rc;
}

// [item][row] as handed over -> [row][item], so that what a step reads is contiguous (crowd kernel: disc tracks, wall tracks)
template <typename T>
static std::vector<T> by_row(const float* v, size_t items, size_t rows) {
  std::vector<T> out(std::max<size_t>(1, items * rows));
  for (size_t k = 0; k < items; ++k)
    for (size_t r = 0; r < rows; ++r) memcpy(&out[r * items + k], v + (sizeof(T) / sizeof(float)) * (k * rows + r), sizeof(T));
  return out;
}

// ---- discs ---------------------------------------------------------------------------------------------------------------
// One disc set of the three (BareboneScene: shared, own, tracks), checked by its setter: `count` sets (0: the set is cleared)
// of counts[b] discs, `total` in all and kmax in the largest, `rows` centres per disc.  tracks: the set counts rows -- a
// change makes row 0 "now" again -- and crowd mode keeps its [row][disc] copy.
static int hand_over_discs(mppi_planner* p, DiscSet& held, bool tracks, int count, const int* counts, long total, int kmax, int rows,
                           const float* pos, const float* r) {
  const size_t n_pos = (size_t)total * (size_t)rows;
  if (count == 0 ? !held.on
                 : (held.on && rows == held.rows && same_as_held(held.counts, counts, (size_t)count) &&
                    same_as_held(held.pos_host, pos, 2 * n_pos) && same_as_held(held.r_host, r, (size_t)total)))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  DiscSet fresh;
  if (count > 0)
    TRY(staged([&]() -> int {
      TRY(dev_stage(&fresh.pos, pos, n_pos));
      TRY(dev_stage(&fresh.r, r, (size_t)total));
      if (tracks && p->scene.crowd) TRY(dev_stage(&fresh.pos_rows, by_row<float2>(pos, (size_t)total, (size_t)rows).data(), n_pos));
      return MPPI_OK;
    }, fresh.pos, fresh.r, fresh.pos_rows));
  fresh.on = count > 0;
  fresh.rows = count > 0 ? rows : 0;
  fresh.max = kmax;
  fresh.counts.assign(counts, counts + count);
  fresh.pos_host.assign(pos, pos + 2 * n_pos);
  fresh.r_host.assign(r, r + (size_t)total);
  held.release();
  held = std::move(fresh);
  drop_graphs(p);  // (the arrays, the counts, the row count and the kernel form are arguments of the captured launches)
  if (tracks) reset_track_offsets(p, kDiscTracks, true, count == 0);
  note_instance_discs(p);
  return MPPI_OK;
}

// The shared set: one set of one row for every problem.
extern "C" int mppi_planner_set_disc_obstacles(mppi_planner* p, const float* positions, const float* radii,
                                               int count) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(count >= 0 && (count == 0 || (positions && radii)), MPPI_ERR_INVALID, "bad obstacle arrays");
  // (the barebone mirror hands the obstacles over with every solve(): barebone_mppi_numba.ipynb cell 3 uploads them per call)
  return hand_over_discs(p, p->scene.shared, false, count > 0 ? 1 : 0, &count, count, count, 1, positions, radii);
}

// Barebone batch: one disc set per problem, the sets one after the other.  count == 0: every problem back to the shared set.
extern "C" int mppi_planner_set_instance_disc_obstacles(mppi_planner* p, int count, const int* disc_counts,
                                                        const float* positions, const float* radii) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "disc obstacles belong to the barebone mode (mode %d)",
          p->cfg.mode);
  TRY(check_set_count(p, count, nullptr));
  long total = 0;
  int kmax = 0;
  if (count > 0) {
    REQUIRE(!p->scene.samples.on, MPPI_ERR_INVALID,
            "the handle holds disc samples, which every problem shares: clear them first (mppi_planner_set_disc_track_samples with samples 0)");
    REQUIRE(disc_counts, MPPI_ERR_INVALID, "NULL disc_counts");
    TRY(sum_counts(count, disc_counts, "disc", &total, &kmax));
    REQUIRE(total <= (1L << 30), MPPI_ERR_INVALID, "too many discs (%ld)", total);
    REQUIRE(total == 0 || (positions && radii), MPPI_ERR_INVALID, "NULL positions or radii");
    // what a launch holds in LDS at the least: the control ratios and the largest problem's discs (an empty set asks for nothing)
    REQUIRE(p->scene.crowd || kmax == 0 || barebone_lds(p->cfg.num_steps, kmax, false, false) <= kBareboneLdsMax, MPPI_ERR_INVALID,
            "a problem with %d disc obstacles and %d steps: more than 64 KiB of LDS", kmax, p->cfg.num_steps);
  }
  return hand_over_discs(p, p->scene.own, false, count, disc_counts, total, kmax, 1, positions, radii);
}

// Barebone mode: discs that move.  `rows` predicted centres per disc (row j: where it is j * dt from "now"), one set shared
// by every problem (count == 1) or one per problem (count == B), laid out like the static per-problem sets.  A change makes
// row 0 "now" again.  Crowd mode keeps the tracks once more as [row][disc] (DiscSet::pos_rows).
extern "C" int mppi_planner_set_disc_tracks(mppi_planner* p, int count, const int* disc_counts, int rows,
                                            const float* tracks, const float* radii) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "disc tracks belong to the barebone mode (mode %d)",
          p->cfg.mode);
  if (disc_counts == nullptr) count = 0;
  TRY(check_set_count(p, count, "set"));
  long total = 0;
  int kmax = 0;
  if (count > 0) {
    REQUIRE(!p->scene.samples.on, MPPI_ERR_INVALID,
            "the handle holds disc samples, the disc source of its launches: clear them first (mppi_planner_set_disc_track_samples with samples 0)");
    REQUIRE(rows >= 1 && rows <= (1 << 20), MPPI_ERR_INVALID, "rows %d: a track has at least one row", rows);
    TRY(sum_counts(count, disc_counts, "disc", &total, &kmax));
    REQUIRE(total * (long)rows <= (1L << 30), MPPI_ERR_INVALID, "too many track rows (%ld discs x %d)", total, rows);
    REQUIRE(total == 0 || (tracks && radii), MPPI_ERR_INVALID, "NULL tracks or radii");
    // what a launch holds in LDS at the least: the control ratios and a row of the largest problem's discs per step
    const size_t lds = barebone_lds(p->cfg.num_steps, kmax, true, false);
    REQUIRE(p->scene.crowd || lds <= kBareboneLdsMax, MPPI_ERR_INVALID,
            "a problem with %d disc tracks and %d steps: %zu bytes, more than 64 KiB of LDS", kmax, p->cfg.num_steps, lds);
  }
  return hand_over_discs(p, p->scene.tracks, true, count, disc_counts, total, kmax, rows, tracks, radii);
}

// Disc samples (include/mppi_hip.h): S sampled futures of K moving discs, `rows` rows each, handed over [sample][disc][row]
// and shared by every problem; crowd mode only.  The device keeps them [row][sample][disc] -- all that a step tests is
// contiguous.  While held they are the disc source of every launch (the tracks' place; the shared static set rests) and
// count as disc tracks wherever the rows are counted.  A change takes a new generation and makes row 0 "now" again.
extern "C" int mppi_planner_set_disc_track_samples(mppi_planner* p, int samples, int disc_count, int rows, const float* positions,
                                                   const float* radii) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "disc samples belong to the barebone mode (mode %d)", p->cfg.mode);
  REQUIRE(samples >= 0 && samples <= kCrowdSamplesMax, MPPI_ERR_INVALID, "samples %d: must be 0 (none) to %d", samples, kCrowdSamplesMax);
  BareboneScene& s = p->scene;
  size_t n_pos = 0;
  if (samples > 0) {
    REQUIRE(s.crowd, MPPI_ERR_INVALID,
            "disc samples need crowd mode: only the crowd kernel has sample forms (mppi_planner_set_crowd(p, 1) first)");
    REQUIRE(s.rings.count == 0, MPPI_ERR_INVALID,
            "the handle holds %d clearance rings, and the sample forms count no rings: clear them first "
            "(mppi_planner_set_clearance_rings(p, NULL, 0))", s.rings.count);
    REQUIRE(!s.occupancy.on, MPPI_ERR_INVALID,
            "the handle holds an occupancy grid, and the sample forms look up no grid: clear it first (mppi_planner_set_occupancy with on 0)");
    REQUIRE(rows >= 1 && rows <= (1 << 20), MPPI_ERR_INVALID, "rows %d: a track has at least one row", rows);
    REQUIRE(disc_count >= 0, MPPI_ERR_INVALID, "negative disc count %d", disc_count);
    const int walls = s.fleet.on() ? s.fleet.slots : (s.wall_tracks.on ? s.wall_tracks.max : s.walls.max);
    REQUIRE((long)disc_count + (long)walls <= (long)kCrowdSampleHitsMax, MPPI_ERR_INVALID,
            "%d discs and %d walls: a sample form counts a step's hits in 16 bits, %d at the most", disc_count, walls, kCrowdSampleHitsMax);
    REQUIRE((long)samples * (long)disc_count * (long)rows <= (1L << 30), MPPI_ERR_INVALID,
            "too many sample rows (%d samples x %d discs x %d)", samples, disc_count, rows);
    REQUIRE(disc_count == 0 || (positions && radii), MPPI_ERR_INVALID, "NULL positions or radii");
    for (int k = 0; k < disc_count; ++k)
      REQUIRE(std::isfinite(radii[k]) && radii[k] >= 0.0f, MPPI_ERR_INVALID, "disc %d: radius %g is negative or not finite", k, (double)radii[k]);
    REQUIRE(!s.own.on, MPPI_ERR_INVALID,
            "the handle holds per-problem disc sets; disc samples are shared by every problem: clear the sets first "
            "(mppi_planner_set_instance_disc_obstacles with count 0)");
    REQUIRE(!(s.tracks.on && s.tracks.counts.size() > 1), MPPI_ERR_INVALID,
            "the handle holds per-problem disc tracks; disc samples are shared by every problem: clear the tracks first "
            "(mppi_planner_set_disc_tracks with count 0)");
    n_pos = (size_t)samples * (size_t)disc_count * (size_t)rows;
  }
  DiscSamples& held = s.samples;
  if (samples == 0 ? !held.on
                   : (held.on && samples == held.count && disc_count == held.discs && rows == held.rows &&
                      same_as_held(held.pos_host, positions, 2 * n_pos) && same_as_held(held.r_host, radii, (size_t)disc_count)))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  DiscSamples fresh;
  if (samples > 0) {  // [sample][disc][row] is [item][row] with S * K items: by_row gives [row][sample][disc]
    TRY(staged([&]() -> int {
      TRY(dev_stage(&fresh.pos_rows, by_row<float2>(positions, (size_t)samples * (size_t)disc_count, (size_t)rows).data(), n_pos));
      TRY(dev_stage(&fresh.r, radii, (size_t)disc_count));
      return MPPI_OK;
    }, fresh.pos_rows, fresh.r));
    fresh.on = true;
    fresh.count = samples;
    fresh.discs = disc_count;
    fresh.rows = rows;
    fresh.gen = next_generation();
    fresh.pos_host.assign(positions, positions + 2 * n_pos);
    fresh.r_host.assign(radii, radii + (size_t)disc_count);
  }
  const bool moved = held.rows > 1 || fresh.rows > 1;  // (a set of one row is static: it leaves "now" alone)
  held.release();
  held = std::move(fresh);
  drop_graphs(p);  // (the arrays, the counts and the kernel form are arguments of the captured launches)
  reset_track_offsets(p, kDiscTracks, moved, samples == 0);
  note_instance_discs(p);
  return MPPI_OK;
}

// Crowd mode (include/mppi_hip.h).  Off -> on: the [row][disc] copy of the tracks the handle holds.  On -> off: only when
// the default family can launch every set the handle holds -- the tracks, the per-problem sets and the shared set each on
// their own (clearing one brings the next back), and what is launched now with its goal track: barebone_choose is asked.
extern "C" int mppi_planner_set_crowd(mppi_planner* p, int on) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "crowd mode belongs to the barebone mode (mode %d)", p->cfg.mode);
  BareboneScene& s = p->scene;
  if ((on != 0) == s.crowd) return MPPI_OK;
  if (!on) {
    REQUIRE(!s.samples.on, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds disc samples, which only the crowd kernel rolls out (clear them first)");
    REQUIRE(s.walls.max == 0, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds %d walls, which only the crowd kernel tests (clear the walls first)", s.walls.max);
    REQUIRE(!s.wall_tracks.on, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds wall tracks, which only the crowd kernel tests (clear them first)");
    REQUIRE(!s.fleet.on(), MPPI_ERR_INVALID,
            "crowd mode stays on: the handle is in fleet mode, whose walls only the crowd kernel tests (mppi_planner_set_fleet(p, 0, NULL) first)");
    REQUIRE(s.footprint.count == 0, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds a footprint of %d discs, which only the crowd kernel tests (mppi_planner_set_footprint(p, NULL, 0) first)",
            s.footprint.count);
    REQUIRE(s.rings.count == 0, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds %d clearance rings, which only the crowd kernel counts (mppi_planner_set_clearance_rings(p, NULL, 0) first)",
            s.rings.count);
    REQUIRE(!s.occupancy.on, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds an occupancy grid, which only the crowd kernel looks up (mppi_planner_set_occupancy with on 0 first)");
    BareboneHeld now = barebone_held(p);  // (without rotation: every set at its own size, the least a launch can ask for)
    now.crowd = false;
    BareboneHeld own = now, shared = now, tracks = now;
    tracks.gtrk_on = own.gtrk_on = shared.gtrk_on = false;
    own.trk_on = shared.trk_on = shared.inst_obs_on = false;
    const struct { bool held; BareboneHeld state; const char* what; } sets[] = {
        {s.tracks.on, tracks, "disc tracks"}, {s.own.on, own, "per-problem disc obstacles"},
        {true, shared, "disc obstacles"}, {s.goal.on || s.guide.on, now, "discs held with a goal track"}};
    for (const auto& set : sets) {
      const BareboneChoice c = barebone_choose(set.state);
      REQUIRE(!set.held || c.family != kBareboneRefused, MPPI_ERR_INVALID,
              "crowd mode stays on: the %s (%d discs, %d steps) need %zu bytes, more than 64 KiB of LDS", set.what, c.kmax, now.T, c.lds);
    }
  }
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float2* pos_rows = nullptr;
  if (on && s.tracks.on)
    TRY(staged([&]() -> int {
      const size_t total = s.tracks.r_host.size(), rows = (size_t)s.tracks.rows;
      return dev_stage(&pos_rows, by_row<float2>(s.tracks.pos_host.data(), total, rows).data(), total * rows);
    }, pos_rows));
  dev_free(s.tracks.pos_rows);
  s.tracks.pos_rows = pos_rows;
  s.crowd = on != 0;
  drop_graphs(p);  // (the kernel form is part of the captured launches)
  return MPPI_OK;
}

extern "C" int mppi_planner_get_crowd(mppi_planner* p, int* on) {
  REQUIRE(p && on, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "crowd mode belongs to the barebone mode (mode %d)", p->cfg.mode);
  *on = p->scene.crowd ? 1 : 0;
  return MPPI_OK;
}

// ---- fleet mode (include/mppi_hip.h; fleet_kernels.h) ------------------------------------------------------------------------
// The device arrays of a fleet (FleetArrays, barebone_scene.h) are built new-first, so that a failure leaves the handle with
// what it had.
// pair_hw: [B][(B - 1) * group] half-widths, reader a's others in ascending order, `group` slots each (a disc fleet: 1; a
// body fleet of `body` discs: that count rounded up to a power of two); the static walls (W of them) behind the others'
// slots in every reader's range and in every row.  Until the first refresh a fleet slot holds the wall nobody can touch.
static int fleet_build(mppi_planner* p, const float* pair_hw, const float* wall_seg, const float* wall_hw, int W, int group, int body,
                       FleetArrays* out) {
  const int B = p->B, T = p->cfg.num_steps, O = (B - 1) * group, S = O + W;
  const size_t pitch = (size_t)B * (size_t)S;
  REQUIRE((long)pitch <= (1L << 24) && (long)pitch * (long)T <= (1L << 28), MPPI_ERR_INVALID,
          "fleet of %d with %d static walls and %d steps: too many wall rows (%zu walls x %d)", B, W, T, pitch, T);
  std::vector<float4> rows(pitch * (size_t)T);
  std::vector<float> hw(pitch);
  std::vector<int2> range((size_t)B);
  for (int a = 0; a < B; ++a) {
    range[(size_t)a] = make_int2(a * S, S);
    for (int k = 0; k < S; ++k) {
      const bool other = k < O;
      hw[(size_t)a * S + k] = other ? pair_hw[(size_t)a * O + k] : wall_hw[k - O];
      const float* w = other ? nullptr : wall_seg + 4 * (size_t)(k - O);
      const float4 sg = other ? make_float4(1e18f, 1e18f, 1e18f, 1e18f) : make_float4(w[0], w[1], w[2], w[3]);
      for (int j = 0; j < T; ++j) rows[(size_t)j * pitch + (size_t)a * S + k] = sg;
    }
  }
  FleetArrays f;
  f.slots = S;
  f.group = group;
  f.body = body;
  const size_t states = (size_t)B * (size_t)(T + 1);
  TRY(staged([&]() -> int {
    TRY(dev_stage(&f.seg_rows, rows.data(), rows.size()));
    TRY(dev_stage(&f.hw, hw.data(), hw.size()));
    TRY(dev_stage(&f.range, range.data(), range.size()));
    TRY(dev_alloc(&f.plan, (size_t)B * (size_t)(T + 1)));
    HIP_TRY(hipMemset(f.plan, 0, sizeof(float2) * states));
    if (body > 0) {
      TRY(dev_alloc(&f.heads, states));
      TRY(dev_alloc(&f.centres, states * (size_t)body));
      HIP_TRY(hipMemset(f.heads, 0, sizeof(float) * states));
      HIP_TRY(hipMemset(f.centres, 0, sizeof(float2) * states * (size_t)body));
    }
    return MPPI_OK;
  }, f.seg_rows, f.hw, f.range, f.plan, f.heads, f.centres));
  *out = f;
  return MPPI_OK;
}

// (the stream has drained) the old arrays go; the handle takes the new ones (or none) and a new generation
static void fleet_commit(mppi_planner* p, const FleetArrays& f) {
  p->scene.fleet.release();
  p->scene.fleet = f;
  p->scene.fleet.gen = f.on() ? next_generation() : 0;
}

// ---- walls ---------------------------------------------------------------------------------------------------------------
// One wall set of the two (BareboneScene: walls, wall_tracks), checked by its setter: `count` sets (0: the set is cleared) of
// counts[b] walls, `total` in all and wmax in the largest, `rows` segments per wall, handed over [wall][row] and kept
// [row][wall].  ranges: {wall0, count} per problem beside them (the wall tracks).  also: staged behind the set's own arrays
// in the same stage, so that a failure there leaves the walls as they were too (the static walls: the fleet's storage).
// A change takes a new generation and, for walls that move (rows > 1), makes row 0 "now" again.
template <typename Also>
static int hand_over_walls(mppi_planner* p, WallSet& held, bool ranges, int count, const int* counts, long total, int wmax, int rows,
                           const float* seg, const float* hw, Also&& also) {
  const size_t n_seg = (size_t)total * (size_t)rows;
  if (count == 0 ? !held.on
                 : (held.on && rows == held.rows && same_as_held(held.counts, counts, (size_t)count) &&
                    same_as_held(held.seg_host, seg, 4 * n_seg) && same_as_held(held.hw_host, hw, (size_t)total)))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  WallSet fresh;
  std::vector<int2> range((size_t)count);
  for (int b = 0, k0 = 0; b < count; k0 += counts[b], ++b) range[(size_t)b] = make_int2(k0, counts[b]);
  TRY(staged([&]() -> int {
    if (count > 0) {
      TRY(dev_stage(&fresh.seg_rows, by_row<float4>(seg, (size_t)total, (size_t)rows).data(), n_seg));
      TRY(dev_stage(&fresh.hw, hw, (size_t)total));
      if (ranges) TRY(dev_stage(&fresh.range, range.data(), range.size()));
    }
    return also();
  }, fresh.seg_rows, fresh.hw, fresh.range));
  fresh.on = count > 0;
  fresh.rows = count > 0 ? rows : 0;
  fresh.max = wmax;
  fresh.gen = count > 0 ? next_generation() : 0;
  fresh.counts.assign(counts, counts + count);
  fresh.seg_host.assign(seg, seg + 4 * n_seg);
  fresh.hw_host.assign(hw, hw + (size_t)total);
  const bool moved = held.rows > 1 || fresh.rows > 1;
  held.release();
  held = std::move(fresh);
  drop_graphs(p);  // (the arrays, the counts, the row count and the kernel form are arguments of the captured launches)
  reset_track_offsets(p, kWallTracks, moved, count == 0);
  if (!ranges) p->scene.guide.dirty = true;  // (the static walls have changed: the guide's field is rasterised from them)
  return MPPI_OK;
}

// Walls (include/mppi_hip.h): crowd mode only -- they are one more source of hits for the count waves of
// k_rollout_barebone_crowd<..., WALLS> and nothing the default forms know.  Static and shared by every problem: one set of
// one row.
extern "C" int mppi_planner_set_walls(mppi_planner* p, const float* segments, const float* halfwidths, int count) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "walls belong to the barebone mode (mode %d)", p->cfg.mode);
  REQUIRE(count >= 0 && count <= (1 << 24) && (count == 0 || (segments && halfwidths)), MPPI_ERR_INVALID, "bad wall arrays (count %d)", count);
  BareboneScene& s = p->scene;
  REQUIRE(count == 0 || s.crowd, MPPI_ERR_INVALID,
          "walls need crowd mode: only the crowd kernel tests them (mppi_planner_set_crowd(p, 1) first)");
  TRY(check_halfwidths(halfwidths, (size_t)count, "wall"));
  TRY(check_finite(segments, (size_t)count, 1, 4, "wall"));
  // fleet mode: these walls lie behind the other robots in every reader's set -- the fleet storage is rebuilt with the
  // new walls, in the same stage
  FleetArrays fleet;
  TRY(hand_over_walls(p, s.walls, false, count > 0 ? 1 : 0, &count, count, count, 1, segments, halfwidths, [&]() -> int {
    if (!s.fleet.on()) return MPPI_OK;
    return fleet_build(p, s.fleet_hw_host.data(), segments, halfwidths, count, s.fleet.group, s.fleet.body, &fleet);
  }));
  if (fleet.on()) fleet_commit(p, fleet);
  return MPPI_OK;
}

// Walls that move, and a wall set per problem (include/mppi_hip.h): crowd mode only, like the static walls.  `rows`
// segments per wall, one set shared by every problem (count == 1) or one per problem (count == B), the sets one after the
// other, each [wall][row].
extern "C" int mppi_planner_set_wall_tracks(mppi_planner* p, int count, const int* wall_counts, int rows,
                                            const float* segments, const float* halfwidths) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "wall tracks belong to the barebone mode (mode %d)", p->cfg.mode);
  if (wall_counts == nullptr) count = 0;
  TRY(check_set_count(p, count, "set"));
  long total = 0;
  int wmax = 0;
  if (count > 0) {
    REQUIRE(!p->scene.fleet.on(), MPPI_ERR_INVALID,
            "the handle is in fleet mode, which owns the per-problem wall sets: turn it off first (mppi_planner_set_fleet(p, 0, NULL))");
    REQUIRE(p->scene.crowd, MPPI_ERR_INVALID,
            "wall tracks need crowd mode: only the crowd kernel tests them (mppi_planner_set_crowd(p, 1) first)");
    REQUIRE(rows >= 1 && rows <= (1 << 20), MPPI_ERR_INVALID, "rows %d: a wall track has at least one row", rows);
    TRY(sum_counts(count, wall_counts, "wall", &total, &wmax));
    REQUIRE(total <= (1L << 24) && total * (long)rows <= (1L << 28), MPPI_ERR_INVALID, "too many wall track rows (%ld walls x %d)", total, rows);
    REQUIRE(total == 0 || (segments && halfwidths), MPPI_ERR_INVALID, "NULL segments or halfwidths");
    TRY(check_halfwidths(halfwidths, (size_t)total, "wall"));
    TRY(check_finite(segments, (size_t)total, (size_t)rows, 4, "wall"));
  }
  return hand_over_walls(p, p->scene.wall_tracks, true, count, wall_counts, total, wmax, rows, segments, halfwidths, [] { return MPPI_OK; });
}

// ---- goal tracks ---------------------------------------------------------------------------------------------------------
// A goal that moves (include/mppi_hip.h): `rows` positions per track, one track for every problem (count == 1) or one per
// problem (count == B), [track][row].  A change takes a new generation and, for a goal that moves (rows > 1), makes row 0
// "now" again.
extern "C" int mppi_planner_set_goal_tracks(mppi_planner* p, int count, int rows, const float* xy) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "goal tracks belong to the barebone mode (mode %d)", p->cfg.mode);
  TRY(check_set_count(p, count, "track"));
  size_t n_xy = 0;
  if (count > 0) {
    REQUIRE(!p->scene.guide.on, MPPI_ERR_INVALID,
            "the handle holds a guide, which owns the goal rows: turn it off first (mppi_planner_set_guide with on 0)");
    REQUIRE(rows >= 1 && rows <= (1 << 20), MPPI_ERR_INVALID, "rows %d: a goal track has at least one row", rows);
    REQUIRE((long)count * (long)rows <= (1L << 28), MPPI_ERR_INVALID, "too many goal track rows (%d tracks x %d)", count, rows);
    REQUIRE(xy, MPPI_ERR_INVALID, "NULL xy");
    n_xy = (size_t)count * (size_t)rows;
    TRY(check_finite(xy, (size_t)count, (size_t)rows, 2, "goal track"));
  }
  GoalTracks& held = p->scene.goal;
  if (count == 0 ? !held.on : (held.on && rows == held.rows && count == held.count && same_as_held(held.host, xy, 2 * n_xy)))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  GoalTracks fresh;
  if (count > 0) {
    TRY(staged([&]() -> int { return dev_stage(&fresh.xy, xy, n_xy); }, fresh.xy));
    fresh.on = true;
    fresh.rows = rows;
    fresh.count = count;
    fresh.gen = next_generation();
    fresh.host.assign(xy, xy + 2 * n_xy);
  }
  const bool moved = held.rows > 1 || fresh.rows > 1;
  held.release();
  held = std::move(fresh);
  drop_graphs(p);  // (the array, the row count and the kernel form are arguments of the captured launches)
  reset_track_offsets(p, kGoalTracks, moved, count == 0);
  return MPPI_OK;
}

// The two kinds of fleet go through "off": one message for both directions.
static const char* const kFleetKinds =
    "the handle is in a fleet of the other kind (mppi_planner_set_fleet: discs with half-widths per pair; "
    "mppi_planner_set_fleet_bodies: one body of discs for every robot): turn it off first (mppi_planner_set_fleet(p, 0, NULL))";

// Fleet mode (include/mppi_hip.h): the storage is built here and whenever the static walls change, never at a refresh.
extern "C" int mppi_planner_set_fleet(mppi_planner* p, int count, const float* halfwidths) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "fleet mode belongs to the barebone mode (mode %d)", p->cfg.mode);
  BareboneScene& s = p->scene;
  if (count == 0) {
    if (!s.fleet.on()) return MPPI_OK;
    HIP_TRY(hipSetDevice(p->cfg.device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (s.fleet.body > 0) {  // (a body fleet holds its body as the handle's footprint: it goes with the fleet)
      s.footprint.set(nullptr, 0, 0);
      s.fleet_margin = 0.0;
    }
    fleet_commit(p, FleetArrays());
    s.fleet_hw_host.clear();
    drop_graphs(p);  // (the arrays and the kernel form are arguments of the captured launches)
    return MPPI_OK;
  }
  REQUIRE(p->B >= 2, MPPI_ERR_INVALID,
          "fleet mode needs a batched handle of at least two problems, one per robot (num_instances %d)", p->B);
  REQUIRE(count == p->B, MPPI_ERR_INVALID, "count %d: must be 0 (off) or num_instances %d", count, p->B);
  REQUIRE(p->cfg.world_size == 1, MPPI_ERR_INVALID, "fleet mode drives an unsharded handle");
  REQUIRE(s.crowd, MPPI_ERR_INVALID,
          "fleet mode needs crowd mode: only the crowd kernel tests walls (mppi_planner_set_crowd(p, 1) first)");
  REQUIRE(!s.wall_tracks.on, MPPI_ERR_INVALID,
          "the handle holds wall tracks or per-problem wall sets; fleet mode makes every problem's set itself: clear them "
          "first (mppi_planner_set_wall_tracks with count 0)");
  REQUIRE(!(s.fleet.on() && s.fleet.body > 0), MPPI_ERR_INVALID, "%s", kFleetKinds);
  REQUIRE(s.footprint.count == 0, MPPI_ERR_INVALID,
          "the handle holds a footprint; the fleet's half-widths already contain the reader's body: clear it first "
          "(mppi_planner_set_footprint(p, NULL, 0))");
  REQUIRE(halfwidths, MPPI_ERR_INVALID, "NULL halfwidths");
  const size_t pairs = (size_t)p->B * (size_t)(p->B - 1);
  TRY(check_halfwidths(halfwidths, pairs, "fleet pair"));
  if (s.fleet.on() && memcmp(halfwidths, s.fleet_hw_host.data(), sizeof(float) * pairs) == 0) return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  FleetArrays fleet;
  TRY(fleet_build(p, halfwidths, s.walls.seg_host.data(), s.walls.hw_host.data(), s.walls.max, 1, 0, &fleet));
  fleet_commit(p, fleet);
  s.fleet_hw_host.assign(halfwidths, halfwidths + pairs);
  drop_graphs(p);
  return MPPI_OK;
}

// n footprint rows (ox, oy, rho): all finite, no negative radius.
static int check_footprint_rows(const float* discs, int n) {
  for (int i = 0; i < n; ++i) {
    REQUIRE(std::isfinite(discs[3 * i]) && std::isfinite(discs[3 * i + 1]) && std::isfinite(discs[3 * i + 2]), MPPI_ERR_INVALID,
            "footprint disc %d: a value is not finite", i);
    REQUIRE(discs[3 * i + 2] >= 0.0f, MPPI_ERR_INVALID, "footprint disc %d: radius %g is negative", i, (double)discs[3 * i + 2]);
  }
  return MPPI_OK;
}

// A body fleet (include/mppi_hip.h): the fleet of robots that are n_discs discs each.  The storage as in the disc fleet,
// with Fp slots a robot; the body is held as the handle's footprint as well, so barebone_choose sees fleet_on with
// footprint = n_discs and picks the footprint form with wall tracks.
extern "C" int mppi_planner_set_fleet_bodies(mppi_planner* p, int count, const float* discs, int n_discs, double margin) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "fleet mode belongs to the barebone mode (mode %d)", p->cfg.mode);
  if (count == 0) return mppi_planner_set_fleet(p, 0, nullptr);
  BareboneScene& s = p->scene;
  REQUIRE(p->B >= 2, MPPI_ERR_INVALID,
          "fleet mode needs a batched handle of at least two problems, one per robot (num_instances %d)", p->B);
  REQUIRE(count == p->B, MPPI_ERR_INVALID, "count %d: must be 0 (off) or num_instances %d", count, p->B);
  REQUIRE(p->cfg.world_size == 1, MPPI_ERR_INVALID, "fleet mode drives an unsharded handle");
  REQUIRE(s.crowd, MPPI_ERR_INVALID,
          "fleet mode needs crowd mode: only the crowd kernel tests walls (mppi_planner_set_crowd(p, 1) first)");
  REQUIRE(!s.wall_tracks.on, MPPI_ERR_INVALID,
          "the handle holds wall tracks or per-problem wall sets; fleet mode makes every problem's set itself: clear them "
          "first (mppi_planner_set_wall_tracks with count 0)");
  REQUIRE(!(s.fleet.on() && s.fleet.body == 0), MPPI_ERR_INVALID, "%s", kFleetKinds);
  REQUIRE(s.fleet.body > 0 || s.footprint.count == 0, MPPI_ERR_INVALID,
          "the handle holds a footprint; a body fleet carries its own body: clear it first (mppi_planner_set_footprint(p, NULL, 0))");
  REQUIRE(n_discs >= 1 && n_discs <= kCrowdFootprintMax, MPPI_ERR_INVALID, "body of %d discs: must be 1 to %d", n_discs, kCrowdFootprintMax);
  REQUIRE(discs, MPPI_ERR_INVALID, "NULL discs");
  TRY(check_footprint_rows(discs, n_discs));
  REQUIRE(std::isfinite(margin), MPPI_ERR_INVALID, "margin %g is not finite", margin);
  for (int k = 0; k < n_discs; ++k)
    REQUIRE((double)discs[3 * k + 2] + margin >= 0.0, MPPI_ERR_INVALID,
            "body disc %d: radius %g and margin %g give a negative half-width", k, (double)discs[3 * k + 2], margin);
  if (s.fleet.on() && s.fleet.body == n_discs && margin == s.fleet_margin &&
      memcmp(discs, s.footprint.host, sizeof(float) * 3 * (size_t)n_discs) == 0)
    return MPPI_OK;
  int group = 1;
  while (group < n_discs) group *= 2;
  // every reader sees the same body: slot k of every other robot has half-width float32(rho_k + margin), the sum in
  // double; the padding slots repeat the last disc
  const size_t per = (size_t)(p->B - 1) * (size_t)group;
  std::vector<float> hw((size_t)p->B * per);
  for (size_t i = 0; i < hw.size(); ++i) {
    const int k = std::min((int)(i % (size_t)group), n_discs - 1);
    hw[i] = (float)((double)discs[3 * k + 2] + margin);
  }
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  FleetArrays fleet;
  TRY(fleet_build(p, hw.data(), s.walls.seg_host.data(), s.walls.hw_host.data(), s.walls.max, group, n_discs, &fleet));
  fleet_commit(p, fleet);
  s.fleet_hw_host = hw;
  s.fleet_margin = margin;
  s.footprint.set(discs, n_discs, next_generation());
  drop_graphs(p);  // (the arrays, the rows, the counts and the kernel form are arguments of the captured launches)
  return MPPI_OK;
}

// *n_discs: the body discs of the body fleet that is on, else 0; *margin: its margin
extern "C" int mppi_planner_get_fleet_bodies(mppi_planner* p, int* n_discs, double* margin) {
  REQUIRE(p && n_discs && margin, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "fleet mode belongs to the barebone mode (mode %d)", p->cfg.mode);
  *n_discs = p->scene.fleet.body;  // (0 while no body fleet is on)
  *margin = p->scene.fleet.on() ? p->scene.fleet_margin : 0.0;
  return MPPI_OK;
}

extern "C" int mppi_planner_get_fleet(mppi_planner* p, int* on) {
  REQUIRE(p && on, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "fleet mode belongs to the barebone mode (mode %d)", p->cfg.mode);
  *on = p->scene.fleet.on() ? p->B : 0;
  return MPPI_OK;
}

// ---- rows by value: a body footprint, clearance rings ---------------------------------------------------------------------
// The rows are a by-value argument of the launches: there is no device array, so nothing to stage -- but the stream is
// drained like everywhere else, and a change takes a new generation (the graph signature's view of the rows) and drops the
// captured graphs.
template <int MaxRows, int Width>
static int hand_over_rows(mppi_planner* p, ValueRows<MaxRows, Width>& held, const float* rows, int count) {
  if (count == held.count && (count == 0 || memcmp(rows, held.host, sizeof(float) * Width * (size_t)count) == 0)) return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  held.set(rows, count, count > 0 ? next_generation() : 0);
  drop_graphs(p);  // (the rows, the count and the kernel form are arguments of the captured launches)
  return MPPI_OK;
}

// A body footprint (include/mppi_hip.h): crowd mode only, and not beside the fleet.
extern "C" int mppi_planner_set_footprint(mppi_planner* p, const float* discs, int count) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "a footprint belongs to the barebone mode (mode %d)", p->cfg.mode);
  REQUIRE(count >= 0 && count <= kCrowdFootprintMax, MPPI_ERR_INVALID, "footprint of %d discs: must be 0 (none) to %d", count, kCrowdFootprintMax);
  const BareboneScene& s = p->scene;
  REQUIRE(!(s.fleet.on() && s.fleet.body > 0), MPPI_ERR_INVALID,
          "the handle is in a body fleet, which carries its own body: turn the fleet off first (mppi_planner_set_fleet(p, 0, NULL))");
  if (count > 0) {
    REQUIRE(discs, MPPI_ERR_INVALID, "NULL discs");
    REQUIRE(s.crowd, MPPI_ERR_INVALID,
            "a footprint needs crowd mode: only the crowd kernel has footprint forms (mppi_planner_set_crowd(p, 1) first)");
    REQUIRE(!s.fleet.on(), MPPI_ERR_INVALID,
            "the handle is in fleet mode, whose half-widths already contain the reader's body: turn it off first "
            "(mppi_planner_set_fleet(p, 0, NULL))");
    TRY(check_footprint_rows(discs, count));
  }
  return hand_over_rows(p, p->scene.footprint, discs, count);
}

extern "C" int mppi_planner_get_footprint(mppi_planner* p, float* discs, int* count) {
  REQUIRE(p && discs && count, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "a footprint belongs to the barebone mode (mode %d)", p->cfg.mode);
  memcpy(discs, p->scene.footprint.host, sizeof(p->scene.footprint.host));
  *count = p->scene.footprint.count;
  return MPPI_OK;
}

// Clearance rings (include/mppi_hip.h): crowd mode only, and not beside disc samples.
extern "C" int mppi_planner_set_clearance_rings(mppi_planner* p, const float* rings, int count) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "clearance rings belong to the barebone mode (mode %d)", p->cfg.mode);
  REQUIRE(count >= 0 && count <= kCrowdRingsMax, MPPI_ERR_INVALID, "%d clearance rings: must be 0 (none) to %d", count, kCrowdRingsMax);
  if (count > 0) {
    REQUIRE(rings, MPPI_ERR_INVALID, "NULL rings");
    REQUIRE(p->scene.crowd, MPPI_ERR_INVALID,
            "clearance rings need crowd mode: only the crowd kernel has ring forms (mppi_planner_set_crowd(p, 1) first)");
    REQUIRE(!p->scene.samples.on, MPPI_ERR_INVALID,
            "the handle holds disc samples, and the sample forms count no rings: clear them first "
            "(mppi_planner_set_disc_track_samples with samples 0)");
    for (int l = 0; l < count; ++l) {
      const float m = rings[2 * l], c = rings[2 * l + 1];
      REQUIRE(std::isfinite(m) && m > 0.0f, MPPI_ERR_INVALID, "ring %d: margin %g is not finite and positive", l, (double)m);
      REQUIRE(l == 0 || m > rings[2 * l - 2], MPPI_ERR_INVALID, "ring %d: margin %g does not exceed ring %d's %g", l, (double)m, l - 1,
              (double)rings[2 * l - 2]);
      REQUIRE(std::isfinite(c) && c >= 0.0f, MPPI_ERR_INVALID, "ring %d: penalty %g is negative or not finite", l, (double)c);
    }
  }
  return hand_over_rows(p, p->scene.rings, rings, count);
}

extern "C" int mppi_planner_get_clearance_rings(mppi_planner* p, float* rings, int* count) {
  REQUIRE(p && rings && count, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "clearance rings belong to the barebone mode (mode %d)", p->cfg.mode);
  memcpy(rings, p->scene.rings.host, sizeof(p->scene.rings.host));
  *count = p->scene.rings.count;
  return MPPI_OK;
}

// The row of every problem's tracks that is "now".  It travels with the start state: a kernel argument of the classic
// single launch, the problem's BatchInst otherwise -- no synchronisation, and nothing a captured graph holds.
extern "C" int mppi_planner_set_track_offsets(mppi_planner* p, int count, const int* offsets) {
  REQUIRE(p && offsets, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "disc tracks belong to the barebone mode (mode %d)",
          p->cfg.mode);
  REQUIRE(count == p->B, MPPI_ERR_INVALID, "count %d != num_instances %d of this handle", count, p->B);
  for (int b = 0; b < count; ++b) REQUIRE(offsets[b] >= 0, MPPI_ERR_INVALID, "problem %d: negative track offset %d", b, offsets[b]);
  for (int b = 0; b < count; ++b) p->inst_host[(size_t)b].track_off = offsets[b];
  p->inst_dirty = true;
  return MPPI_OK;
}

extern "C" int mppi_planner_get_track_offsets(mppi_planner* p, int count, int* offsets) {
  REQUIRE(p && offsets, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "disc tracks belong to the barebone mode (mode %d)",
          p->cfg.mode);
  REQUIRE(count == p->B, MPPI_ERR_INVALID, "count %d != num_instances %d of this handle", count, p->B);
  for (int b = 0; b < count; ++b) offsets[b] = p->inst_host[(size_t)b].track_off;
  return MPPI_OK;
}

// Fleet mode: every reader's rows from the robots' current controls and start states, on the planner's stream -- at the
// head of every call that starts iterations (solve, iterate_async, the stage-level rollout, each control step of
// closed_loop), once per call.  done: closed_loop's per-problem flags (a robot at its goal stands), else nullptr.
// The arrays stay where they are: nothing a captured graph holds changes.
static int fleet_refresh(mppi_planner* p, const int* done) {
  const FleetArrays& f = p->scene.fleet;
  if (!f.on()) return MPPI_OK;
  REQUIRE(p->params_set, MPPI_ERR_STATE, "params not set");
  REQUIRE(p->inst_set, MPPI_ERR_STATE, "num_instances = %d: call mppi_planner_set_instances before solving", p->B);
  TRY(upload_instances(p));
  const DevParams d = make_dev_params(p);
  const int B = p->B, T = p->cfg.num_steps;
  REQUIRE((size_t)T * sizeof(double2) <= 64 * 1024, MPPI_ERR_INVALID, "num_steps %d too large", T);  // (as launch_rollout)
  const size_t lds = fleet_plans_lds_bytes(T);  // (28 bytes a step: 112 KiB at the 4096 steps the line above admits)
  const bool exact = p->cfg.math == MPPI_MATH_EXACT, body = f.body > 0;
  auto plans = body ? (exact ? &k_fleet_plans<true, true> : &k_fleet_plans<false, true>)
                    : (exact ? &k_fleet_plans<true, false> : &k_fleet_plans<false, false>);
  if (lds > 64 * 1024)  // (a horizon of more than ~2300 steps)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(plans), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(plans, dim3(B), dim3(64), lds, p->stream, d, p->u, done, f.plan, body ? f.heads : nullptr);
  HIP_TRY(hipGetLastError());
  if (body) {  // the body discs' centres once per (robot, state), then the scatter into every reader's slots
    const int states = B * (T + 1), F = f.body, Fp = f.group;
    hipLaunchKernelGGL(k_fleet_body_centres, dim3(ceil_div(states, 256)), dim3(256), 0, p->stream, f.plan, f.heads, f.centres, states,
                       footprint_arg(p));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fleet_body_walls, dim3(ceil_div((long)B * (B - 1) * Fp, 256), T), dim3(256), 0, p->stream, f.centres, f.seg_rows, B, T,
                       f.slots, F, Fp);
    HIP_TRY(hipGetLastError());
    return MPPI_OK;
  }
  hipLaunchKernelGGL(k_fleet_walls, dim3(ceil_div((long)B * (B - 1), 256), T), dim3(256), 0, p->stream, f.plan, f.seg_rows, B, T,
                     f.slots);
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

extern "C" int mppi_planner_fleet_refresh(mppi_planner* p) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->scene.fleet.on(), MPPI_ERR_STATE, "the handle is not in fleet mode (mppi_planner_set_fleet)");
  HIP_TRY(hipSetDevice(p->cfg.device));
  TRY(fleet_refresh(p, nullptr));
  return drain_stream(p);
}

// ---- an occupancy grid (include/mppi_hip.h; occupancy_kernels.h, occupancy_grid.h) ---------------------------------------------
// The hand-over: the values are checked, an unchanged hand-over costs a comparison.  New cells of the same shape, geometry,
// inflate and substeps are packed into the host copy of the mask and mark the field dirty: the arrays stay where they are,
// the captured graphs stay valid.  Anything else drains the stream, builds the new arrays before the old ones are freed,
// takes a new generation and drops the captured graphs.  Nothing is launched here: the field is built on the planner's
// stream at the head of the next call that starts iterations (occupancy_refresh).
static void occupancy_pack(const unsigned char* cells, int nx, int ny, std::vector<unsigned long long>& mask) {
  const size_t words = (size_t)((nx + 63) / 64);
  mask.resize(words * (size_t)ny);
  for (int y = 0; y < ny; ++y) {
    const unsigned char* row = cells + (size_t)y * (size_t)nx;
    for (size_t w = 0; w < words; ++w) {  // (no branch on a cell's value: a lidar's grid is noise to a predictor)
      const int n = std::min(64, nx - (int)(64 * w));
      unsigned long long bits = 0ull;
      for (int i = 0; i < n; ++i) bits |= (unsigned long long)(row[64 * w + (size_t)i] != 0) << i;
      mask[(size_t)y * words + w] = bits;
    }
  }
}

extern "C" int mppi_planner_set_occupancy(mppi_planner* p, int on, float x_min, float y_min, float res, int nx, int ny, float inflate,
                                          int substeps, const unsigned char* cells) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "an occupancy grid belongs to the barebone mode (mode %d)", p->cfg.mode);
  BareboneScene& s = p->scene;
  OccupancyArrays& held = s.occupancy;
  if (!on) {
    if (!held.on) return MPPI_OK;
    HIP_TRY(hipSetDevice(p->cfg.device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    OccupancyArrays off;
    off.fields_built = held.fields_built;
    held.release();
    held = std::move(off);
    drop_graphs(p);  // (the field, the geometry and the kernel form are arguments of the captured launches)
    s.guide.dirty = true;  // (the guide's blocked cells were the grid's as well)
    return MPPI_OK;
  }
  REQUIRE(s.crowd, MPPI_ERR_INVALID,
          "an occupancy grid needs crowd mode: only the crowd kernel has grid forms (mppi_planner_set_crowd(p, 1) first)");
  REQUIRE(p->cfg.world_size == 1, MPPI_ERR_INVALID, "an occupancy grid drives an unsharded handle (world_size %d)", p->cfg.world_size);
  REQUIRE(!s.samples.on, MPPI_ERR_INVALID,
          "the handle holds disc samples, and the sample forms look up no grid: clear them first "
          "(mppi_planner_set_disc_track_samples with samples 0)");
  REQUIRE(cells, MPPI_ERR_INVALID, "NULL cells");
  REQUIRE(std::isfinite(x_min) && std::isfinite(y_min) && std::isfinite(res) && std::isfinite(inflate), MPPI_ERR_INVALID,
          "occupancy: a value is not finite");
  REQUIRE(res > 0.0f, MPPI_ERR_INVALID, "occupancy: resolution %g must be > 0", (double)res);
  REQUIRE(inflate >= 0.0f, MPPI_ERR_INVALID, "occupancy: inflate %g must be >= 0", (double)inflate);
  REQUIRE(nx >= 1 && ny >= 1 && nx <= kOccupancyDimMax && ny <= kOccupancyDimMax, MPPI_ERR_INVALID,
          "occupancy: a grid of %d x %d cells: both 1 to %d", ny, nx, kOccupancyDimMax);
  REQUIRE(substeps >= 1 && substeps <= kOccupancySubstepsMax, MPPI_ERR_INVALID, "occupancy: substeps %d: must be 1 to %d", substeps,
          kOccupancySubstepsMax);
  const size_t n_cells = (size_t)nx * (size_t)ny;
  const bool same_arrays = held.on && nx == held.nx && ny == held.ny && x_min == held.x_min && y_min == held.y_min && res == held.res &&
                           inflate == held.inflate && substeps == held.substeps;
  if (same_arrays) {
    if (memcmp(cells, held.cells_host.data(), n_cells) == 0) return MPPI_OK;
    std::vector<unsigned long long> mask;  // (compared as "occupied or not": any non-zero value is an occupied cell)
    occupancy_pack(cells, nx, ny, mask);
    held.cells_host.assign(cells, cells + n_cells);
    if (mask == held.mask_host) return MPPI_OK;
    held.mask_host.swap(mask);
    held.dirty = true;
    return MPPI_OK;
  }
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  OccupancyArrays fresh;
  fresh.nx = nx; fresh.ny = ny;
  TRY(staged([&]() -> int {
    TRY(dev_alloc(&fresh.mask, (size_t)fresh.words() * (size_t)ny));
    TRY(dev_alloc(&fresh.field, n_cells));
    return MPPI_OK;
  }, fresh.mask, fresh.field));
  fresh.on = true;
  fresh.x_min = x_min; fresh.y_min = y_min; fresh.res = res; fresh.inflate = inflate;
  fresh.substeps = substeps;
  fresh.gen = next_generation();
  fresh.dirty = true;
  fresh.fields_built = held.fields_built;
  fresh.cells_host.assign(cells, cells + n_cells);
  occupancy_pack(cells, nx, ny, fresh.mask_host);
  held.release();
  held = std::move(fresh);
  drop_graphs(p);  // (the field, the geometry, the thresholds and the kernel form are arguments of the captured launches)
  s.guide.dirty = true;
  return MPPI_OK;
}

extern "C" int mppi_planner_get_occupancy(mppi_planner* p, int* on, int* nx, int* ny, unsigned long long* fields_built) {
  REQUIRE(p && on && nx && ny && fields_built, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "an occupancy grid belongs to the barebone mode (mode %d)", p->cfg.mode);
  const OccupancyArrays& o = p->scene.occupancy;
  *on = o.on ? 1 : 0;
  *nx = o.nx;
  *ny = o.ny;
  *fields_built = o.fields_built;
  return MPPI_OK;
}

// The grid's refresh, on the planner's stream at the head of every call that starts iterations, ahead of the guide's (whose
// blocked cells read the field): the mask goes to the device and the field is built when the cells have changed, else
// nothing.  The arrays stay where they are: nothing a captured graph holds changes.
static int occupancy_refresh(mppi_planner* p) {
  OccupancyArrays& o = p->scene.occupancy;
  if (!o.on || !o.dirty) return MPPI_OK;
  const int words = o.words();
  HIP_TRY(hipMemcpyAsync(o.mask, o.mask_host.data(), sizeof(unsigned long long) * o.mask_host.size(), hipMemcpyHostToDevice, p->stream));
  hipLaunchKernelGGL(k_occupancy_field, dim3(words, ceil_div(o.ny, kOccupancyBand)), dim3(64, kOccupancyBand),
                     sizeof(unsigned short) * 64 * (size_t)o.ny, p->stream, o.mask, o.nx, o.ny, words, o.field);
  HIP_TRY(hipGetLastError());
  o.dirty = false;
  ++o.fields_built;
  p->scene.guide.dirty = true;  // (the guide's blocked cells are the grid's as well)
  return MPPI_OK;
}

extern "C" int mppi_planner_occupancy_refresh(mppi_planner* p) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->scene.occupancy.on, MPPI_ERR_STATE, "the handle holds no occupancy grid (mppi_planner_set_occupancy)");
  HIP_TRY(hipSetDevice(p->cfg.device));
  TRY(occupancy_refresh(p));
  return drain_stream(p);
}

// out: [ny][nx], the field of the last build
extern "C" int mppi_planner_get_occupancy_field(mppi_planner* p, unsigned* out) {
  REQUIRE(p && out, MPPI_ERR_INVALID, "NULL argument");
  const OccupancyArrays& o = p->scene.occupancy;
  REQUIRE(o.on, MPPI_ERR_STATE, "the handle holds no occupancy grid (mppi_planner_set_occupancy)");
  REQUIRE(o.fields_built > 0 && !o.dirty, MPPI_ERR_STATE,
          "the clearance field has not been built for these cells yet (mppi_planner_occupancy_refresh, or a solve)");
  return copy_out(p, out, o.field, sizeof(uint32_t) * (size_t)o.nx * (size_t)o.ny);
}

// ---- a guide round the walls (include/mppi_hip.h; guide_kernels.h, guide_grid.h) ---------------------------------------------
// The hand-over: the parameters are checked, an unchanged hand-over does nothing, a change drains the stream, builds the new
// arrays before the old ones are freed, takes a new generation, drops the captured graphs and marks the field dirty.  Nothing
// is launched here: the field is built on the planner's stream at the head of the next call that starts iterations.
extern "C" int mppi_planner_set_guide(mppi_planner* p, int on, float x_min, float y_min, float res, int nx, int ny, float inflate,
                                      float lead, float pace) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "the guide belongs to the barebone mode (mode %d)", p->cfg.mode);
  GuideArrays& held = p->scene.guide;
  if (!on) {
    if (!held.on) return MPPI_OK;
    HIP_TRY(hipSetDevice(p->cfg.device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    GuideArrays off;
    off.fields_built = held.fields_built;
    held.release();
    held = off;
    drop_graphs(p);  // (the rows and the kernel form are arguments of the captured launches)
    return MPPI_OK;
  }
  const int T = p->cfg.num_steps;
  REQUIRE(p->cfg.world_size == 1, MPPI_ERR_INVALID, "the guide drives an unsharded handle (world_size %d)", p->cfg.world_size);
  REQUIRE(!p->scene.goal.on, MPPI_ERR_INVALID,
          "the handle holds goal tracks; the guide owns the goal rows: clear them first (mppi_planner_set_goal_tracks with count 0)");
  REQUIRE(std::isfinite(x_min) && std::isfinite(y_min) && std::isfinite(res) && std::isfinite(inflate) && std::isfinite(lead) &&
              std::isfinite(pace), MPPI_ERR_INVALID, "guide: a value is not finite");
  REQUIRE(res > 0.0f, MPPI_ERR_INVALID, "guide: resolution %g must be > 0", (double)res);
  REQUIRE(nx >= 1 && ny >= 1 && (long)nx * (long)ny <= (long)kGuideCellsMax, MPPI_ERR_INVALID,
          "guide: a grid of %d x %d cells: both at least 1 and %d cells (192 x 192) at the most", ny, nx, kGuideCellsMax);
  REQUIRE(inflate >= 0.0f && 2.0 * (double)inflate * (double)inflate >= (double)res * (double)res, MPPI_ERR_INVALID,
          "guide: inflate %g is below resolution / sqrt(2) = %g: a diagonal move between free cells could touch a wall", (double)inflate,
          (double)res / std::sqrt(2.0));
  REQUIRE(lead >= 0.0f && pace >= 0.0f, MPPI_ERR_INVALID, "guide: lead %g and pace %g must be >= 0", (double)lead, (double)pace);
  const double lead_u = guide_units(lead, res), pace_u = guide_units(pace, res);
  REQUIRE(lead_u + (double)T * pace_u < 2147483648.0, MPPI_ERR_INVALID,
          "guide: lead %g and pace %g over %d steps at resolution %g: more than 2^31 units of resolution / 12", (double)lead, (double)pace, T,
          (double)res);
  if (held.on && x_min == held.x_min && y_min == held.y_min && res == held.res && nx == held.nx && ny == held.ny &&
      inflate == held.inflate && lead == held.lead && pace == held.pace)
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  GuideArrays fresh;
  const size_t cells = (size_t)nx * (size_t)ny, B = (size_t)p->B, rows = B * (size_t)(T + 1);
  TRY(staged([&]() -> int {
    TRY(dev_alloc(&fresh.field, B * cells));
    TRY(dev_alloc(&fresh.moves, B * cells));
    TRY(dev_alloc(&fresh.rows, rows));
    TRY(dev_alloc(&fresh.status, B));
    HIP_TRY(hipMemset(fresh.rows, 0, sizeof(float2) * rows));
    HIP_TRY(hipMemset(fresh.status, 0, sizeof(int) * B));
    return MPPI_OK;
  }, fresh.field, fresh.moves, fresh.rows, fresh.status));
  fresh.on = true;
  fresh.x_min = x_min; fresh.y_min = y_min; fresh.res = res; fresh.inflate = inflate; fresh.lead = lead; fresh.pace = pace;
  fresh.nx = nx; fresh.ny = ny;
  fresh.lead_u = (int)lead_u; fresh.pace_u = (int)pace_u;
  fresh.gen = next_generation();
  fresh.dirty = true;
  fresh.fields_built = held.fields_built;
  held.release();
  held = std::move(fresh);
  drop_graphs(p);  // (the rows, their count and the kernel form are arguments of the captured launches)
  return MPPI_OK;
}

extern "C" int mppi_planner_get_guide(mppi_planner* p, int* on, int* nx, int* ny, unsigned long long* fields_built) {
  REQUIRE(p && on && nx && ny && fields_built, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "the guide belongs to the barebone mode (mode %d)", p->cfg.mode);
  const GuideArrays& g = p->scene.guide;
  *on = g.on ? 1 : 0;
  *nx = g.nx;
  *ny = g.ny;
  *fields_built = g.fields_built;
  return MPPI_OK;
}

// The guide's refresh, on the planner's stream at the head of every call that starts iterations, behind the fleet's: the
// field when something it depends on has changed -- the guide or the static walls (dirty), or a goal, seen here against the
// goals of the last build --, then the rows from the start states as they are on the device.  done: closed_loop's
// per-problem flags (a parked problem's rows are the goal), else nullptr.  The arrays stay where they are: nothing a
// captured graph holds changes.
static int guide_refresh(mppi_planner* p, const int* done) {
  GuideArrays& g = p->scene.guide;
  if (!g.on) return MPPI_OK;
  REQUIRE(p->params_set, MPPI_ERR_STATE, "params not set");
  REQUIRE(p->B == 1 || p->inst_set, MPPI_ERR_STATE, "num_instances = %d: call mppi_planner_set_instances before solving", p->B);
  TRY(upload_instances(p));
  const DevParams d = make_dev_params(p);
  const int B = p->B, cells = g.nx * g.ny;
  auto goal_of = [&](int b, int k) {  // the goals as the launches will see them
    return p->inst_set ? (k == 0 ? p->inst_host[(size_t)b].xg : p->inst_host[(size_t)b].yg) : p->params.xgoal[k];
  };
  bool moved = g.goals_built.size() != (size_t)2 * B;  // (compared as numbers: -0.0 is 0.0, and no allocation on this path)
  for (int b = 0; b < B && !moved; ++b)
    moved = g.goals_built[(size_t)2 * b] != goal_of(b, 0) || g.goals_built[(size_t)2 * b + 1] != goal_of(b, 1);
  const GuideGrid grid{g.x_min, g.y_min, g.res, g.inflate, g.nx, g.ny, g.lead_u, g.pace_u};
  if (g.dirty || moved) {
    const WallSet& w = p->scene.walls;
    // the occupancy grid, if one is held: its cells within inflate_occ + inflate_guide of an occupied one block as well
    const OccupancyArrays& o = p->scene.occupancy;
    GuideOccupancy occ{};
    if (o.on) occ = GuideOccupancy{o.field, o.x_min, o.y_min, o.res, o.nx, o.ny, occupancy_threshold(o.inflate, (double)g.inflate, 0.0, o.res)};
    const size_t lds = sizeof(uint32_t) * (size_t)cells;
    if (lds + kGuideFieldStaticLds > 64 * 1024)  // (from about 124 x 124 cells on: the wall tile's static LDS counts too)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_guide_field), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_guide_field, dim3(B), dim3(kGuideFieldThreads), lds, p->stream, d, grid, w.on ? w.seg_rows : nullptr,
                       w.on ? w.hw : nullptr, w.on ? w.max : 0, g.field, g.moves, occ);
    HIP_TRY(hipGetLastError());
    g.goals_built.resize((size_t)2 * B);
    for (int b = 0; b < B; ++b) {
      g.goals_built[(size_t)2 * b] = goal_of(b, 0);
      g.goals_built[(size_t)2 * b + 1] = goal_of(b, 1);
    }
    g.dirty = false;
    ++g.fields_built;
  }
  hipLaunchKernelGGL(k_guide_rows, dim3(B), dim3(kGuideRowsThreads), (size_t)cells, p->stream, d, grid, g.field, g.moves, done, g.rows,
                     g.status);
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

extern "C" int mppi_planner_guide_refresh(mppi_planner* p) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->scene.guide.on, MPPI_ERR_STATE, "the handle holds no guide (mppi_planner_set_guide)");
  HIP_TRY(hipSetDevice(p->cfg.device));
  TRY(occupancy_refresh(p));
  TRY(guide_refresh(p, nullptr));
  return drain_stream(p);
}

// out: [B][ny][nx], the field of the last build
extern "C" int mppi_planner_get_guide_field(mppi_planner* p, unsigned* out) {
  REQUIRE(p && out, MPPI_ERR_INVALID, "NULL argument");
  const GuideArrays& g = p->scene.guide;
  REQUIRE(g.on, MPPI_ERR_STATE, "the handle holds no guide (mppi_planner_set_guide)");
  REQUIRE(!g.goals_built.empty(), MPPI_ERR_STATE, "the guide's field has not been built yet (mppi_planner_guide_refresh, or a solve)");
  return copy_out(p, out, g.field, sizeof(uint32_t) * (size_t)p->B * (size_t)g.nx * (size_t)g.ny);
}

// xy: [B][T + 1][2]; status: [B] -- of the last refresh
extern "C" int mppi_planner_get_guide_rows(mppi_planner* p, float* xy, int* status) {
  REQUIRE(p && xy && status, MPPI_ERR_INVALID, "NULL argument");
  const GuideArrays& g = p->scene.guide;
  REQUIRE(g.on, MPPI_ERR_STATE, "the handle holds no guide (mppi_planner_set_guide)");
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipMemcpyAsync(status, g.status, sizeof(int) * (size_t)p->B, hipMemcpyDeviceToHost, p->stream));
  return copy_out(p, xy, g.rows, sizeof(float2) * (size_t)p->B * (size_t)(p->cfg.num_steps + 1));
}
