// barebone_api.h -- the hand-overs of the barebone mode (include/mppi_hip.h): disc sets, disc tracks, crowd mode, walls,
// disc samples, wall tracks, goal tracks, fleet mode, track offsets.  Included by mppi_api.hip behind launch_plan.h.
//
// Every hand-over goes the same way: check the arguments; return at once when what is handed over is what is held
// (the Python mirror hands its arrays over with every solve: unchanged arrays cost a comparison, not a synchronisation and
// two allocations); else synchronise, build the new device arrays, and only when that has succeeded free the old ones,
// commit and drop the captured graphs, whose launches hold the arrays, the counts and the kernel form by value.  A failed
// allocation or copy leaves the handle as it was.
#pragma once

// Barebone mode: every problem's range of the disc arrays its launch gets (BatchInst::disc0, n_discs) -- its own set
// (mppi_planner_set_instance_disc_obstacles) or the shared one.  Uploaded with the start states.
static void note_instance_discs(mppi_planner* p) {
  if (p->cfg.mode != MPPI_MODE_BAREBONE) return;
  int k0 = 0;
  for (int b = 0; b < p->B; ++b) {
    BatchInst& I = p->inst_host[(size_t)b];
    if (p->smp_on) {  // (disc samples: one set of K discs for every problem, the samples side by side within a row)
      I.disc0 = 0;
      I.n_discs = p->smp_discs;
    } else if (p->trk_on) {  // (discs that move take the place of both static sets: mppi_planner_set_disc_tracks)
      const bool own = p->trk_counts_host.size() > 1;
      I.disc0 = own ? k0 : 0;
      I.n_discs = p->trk_counts_host[own ? (size_t)b : 0];
    } else {
      I.disc0 = p->inst_obs_on ? k0 : 0;
      I.n_discs = p->inst_obs_on ? p->inst_obs_counts_host[(size_t)b] : p->n_obstacles;
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
  const bool above = (kind < kDiscTracks && (p->trk_on || p->smp_on)) || (kind < kWallTracks && p->wtrk_on && p->wtrk_rows > 1);
  if (!moved || (cleared && above)) return;
  for (BatchInst& I : p->inst_host) I.track_off = 0;
  p->inst_dirty = true;
}

// Staged upload.  dev_stage: one new device array of n items (one at the least), filled from the host.  staged: runs the
// caller's sequence of them; a failure frees what the sequence had got, and the handle still holds what it held.
// dev_take: the commit -- the old array goes, the handle takes the new one (or none).
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
template <typename T>
static void dev_take(T*& held, T* fresh) {
  dev_free(held);
  held = fresh;
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
extern "C" int mppi_planner_set_disc_obstacles(mppi_planner* p, const float* positions, const float* radii,
                                               int count) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(count >= 0 && (count == 0 || (positions && radii)), MPPI_ERR_INVALID, "bad obstacle arrays");
  // (the barebone mirror hands the obstacles over with every solve(): barebone_mppi_numba.ipynb cell 3 uploads them per call)
  if (count == p->n_obstacles && same_as_held(p->obs_pos_host, positions, 2 * (size_t)count) &&
      same_as_held(p->obs_r_host, radii, (size_t)count))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float2* pos = nullptr;
  float* r = nullptr;
  if (count > 0)
    TRY(staged([&]() -> int {
      TRY(dev_stage(&pos, positions, (size_t)count));
      TRY(dev_stage(&r, radii, (size_t)count));
      return MPPI_OK;
    }, pos, r));
  dev_take(p->obs_pos, pos);
  dev_take(p->obs_r, r);
  p->obs_pos_host.assign(positions, positions + 2 * (size_t)count);
  p->obs_r_host.assign(radii, radii + (size_t)count);
  p->n_obstacles = count;
  note_instance_discs(p);
  drop_graphs(p);  // (the count is a by-value argument of the captured launches)
  return MPPI_OK;
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
    REQUIRE(!p->smp_on, MPPI_ERR_INVALID,
            "the handle holds disc samples, which every problem shares: clear them first (mppi_planner_set_disc_track_samples with samples 0)");
    REQUIRE(disc_counts, MPPI_ERR_INVALID, "NULL disc_counts");
    TRY(sum_counts(count, disc_counts, "disc", &total, &kmax));
    REQUIRE(total <= (1L << 30), MPPI_ERR_INVALID, "too many discs (%ld)", total);
    REQUIRE(total == 0 || (positions && radii), MPPI_ERR_INVALID, "NULL positions or radii");
    // what a launch holds in LDS at the least: the control ratios and the largest problem's discs (an empty set asks for nothing)
    REQUIRE(p->crowd || kmax == 0 || barebone_lds(p->cfg.num_steps, kmax, false, false) <= kBareboneLdsMax, MPPI_ERR_INVALID,
            "a problem with %d disc obstacles and %d steps: more than 64 KiB of LDS", kmax, p->cfg.num_steps);
  }
  if (count == 0 ? !p->inst_obs_on
                 : (p->inst_obs_on && same_as_held(p->inst_obs_counts_host, disc_counts, (size_t)count) &&
                    same_as_held(p->inst_obs_pos_host, positions, 2 * (size_t)total) &&
                    same_as_held(p->inst_obs_r_host, radii, (size_t)total)))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float2* pos = nullptr;
  float* r = nullptr;
  if (count > 0)
    TRY(staged([&]() -> int {
      TRY(dev_stage(&pos, positions, (size_t)total));
      TRY(dev_stage(&r, radii, (size_t)total));
      return MPPI_OK;
    }, pos, r));
  dev_take(p->inst_obs_pos, pos);
  dev_take(p->inst_obs_r, r);
  p->inst_obs_on = count > 0;
  p->inst_obs_max = kmax;
  p->inst_obs_counts_host.assign(disc_counts, disc_counts + count);
  p->inst_obs_pos_host.assign(positions, positions + 2 * (size_t)total);
  p->inst_obs_r_host.assign(radii, radii + (size_t)total);
  drop_graphs(p);  // (the arrays and the largest count are arguments of the captured launches)
  note_instance_discs(p);
  return MPPI_OK;
}

// Barebone mode: discs that move.  `rows` predicted centres per disc (row j: where it is j * dt from "now"), one set shared
// by every problem (count == 1) or one per problem (count == B), laid out like the static per-problem sets.  A change makes
// row 0 "now" again.  Crowd mode keeps the tracks once more as [row][disc] (trk_pos_rows).
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
    REQUIRE(!p->smp_on, MPPI_ERR_INVALID,
            "the handle holds disc samples, the disc source of its launches: clear them first (mppi_planner_set_disc_track_samples with samples 0)");
    REQUIRE(rows >= 1 && rows <= (1 << 20), MPPI_ERR_INVALID, "rows %d: a track has at least one row", rows);
    TRY(sum_counts(count, disc_counts, "disc", &total, &kmax));
    REQUIRE(total * (long)rows <= (1L << 30), MPPI_ERR_INVALID, "too many track rows (%ld discs x %d)", total, rows);
    REQUIRE(total == 0 || (tracks && radii), MPPI_ERR_INVALID, "NULL tracks or radii");
    // what a launch holds in LDS at the least: the control ratios and a row of the largest problem's discs per step
    const size_t lds = barebone_lds(p->cfg.num_steps, kmax, true, false);
    REQUIRE(p->crowd || lds <= kBareboneLdsMax, MPPI_ERR_INVALID,
            "a problem with %d disc tracks and %d steps: %zu bytes, more than 64 KiB of LDS", kmax, p->cfg.num_steps, lds);
  }
  const size_t n_pos = (size_t)total * (size_t)rows;
  if (count == 0 ? !p->trk_on
                 : (p->trk_on && rows == p->trk_rows && same_as_held(p->trk_counts_host, disc_counts, (size_t)count) &&
                    same_as_held(p->trk_pos_host, tracks, 2 * n_pos) && same_as_held(p->trk_r_host, radii, (size_t)total)))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float2 *pos = nullptr, *pos_rows = nullptr;
  float* r = nullptr;
  if (count > 0)
    TRY(staged([&]() -> int {
      TRY(dev_stage(&pos, tracks, n_pos));
      TRY(dev_stage(&r, radii, (size_t)total));
      if (p->crowd) TRY(dev_stage(&pos_rows, by_row<float2>(tracks, (size_t)total, (size_t)rows).data(), n_pos));
      return MPPI_OK;
    }, pos, r, pos_rows));
  dev_take(p->trk_pos, pos);
  dev_take(p->trk_r, r);
  dev_take(p->trk_pos_rows, pos_rows);
  p->trk_on = count > 0;
  p->trk_rows = count > 0 ? rows : 0;
  p->trk_max = kmax;
  p->trk_counts_host.assign(disc_counts, disc_counts + count);
  p->trk_pos_host.assign(tracks, tracks + 2 * n_pos);
  p->trk_r_host.assign(radii, radii + (size_t)total);
  drop_graphs(p);  // (the arrays, the row count and the kernel form are arguments of the captured launches)
  reset_track_offsets(p, kDiscTracks, true, count == 0);
  note_instance_discs(p);
  return MPPI_OK;
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
  size_t n_pos = 0;
  if (samples > 0) {
    REQUIRE(p->crowd, MPPI_ERR_INVALID,
            "disc samples need crowd mode: only the crowd kernel has sample forms (mppi_planner_set_crowd(p, 1) first)");
    REQUIRE(p->ring_count == 0, MPPI_ERR_INVALID,
            "the handle holds %d clearance rings, and the sample forms count no rings: clear them first "
            "(mppi_planner_set_clearance_rings(p, NULL, 0))", p->ring_count);
    REQUIRE(rows >= 1 && rows <= (1 << 20), MPPI_ERR_INVALID, "rows %d: a track has at least one row", rows);
    REQUIRE(disc_count >= 0, MPPI_ERR_INVALID, "negative disc count %d", disc_count);
    const int walls = p->fleet_on ? p->fleet_slots : (p->wtrk_on ? p->wtrk_max : p->n_walls);
    REQUIRE((long)disc_count + (long)walls <= (long)kCrowdSampleHitsMax, MPPI_ERR_INVALID,
            "%d discs and %d walls: a sample form counts a step's hits in 16 bits, %d at the most", disc_count, walls, kCrowdSampleHitsMax);
    REQUIRE((long)samples * (long)disc_count * (long)rows <= (1L << 30), MPPI_ERR_INVALID,
            "too many sample rows (%d samples x %d discs x %d)", samples, disc_count, rows);
    REQUIRE(disc_count == 0 || (positions && radii), MPPI_ERR_INVALID, "NULL positions or radii");
    for (int k = 0; k < disc_count; ++k)
      REQUIRE(std::isfinite(radii[k]) && radii[k] >= 0.0f, MPPI_ERR_INVALID, "disc %d: radius %g is negative or not finite", k, (double)radii[k]);
    REQUIRE(!p->inst_obs_on, MPPI_ERR_INVALID,
            "the handle holds per-problem disc sets; disc samples are shared by every problem: clear the sets first "
            "(mppi_planner_set_instance_disc_obstacles with count 0)");
    REQUIRE(!(p->trk_on && p->trk_counts_host.size() > 1), MPPI_ERR_INVALID,
            "the handle holds per-problem disc tracks; disc samples are shared by every problem: clear the tracks first "
            "(mppi_planner_set_disc_tracks with count 0)");
    n_pos = (size_t)samples * (size_t)disc_count * (size_t)rows;
  }
  if (samples == 0 ? !p->smp_on
                   : (p->smp_on && samples == p->smp_count && disc_count == p->smp_discs && rows == p->smp_rows &&
                      same_as_held(p->smp_pos_host, positions, 2 * n_pos) && same_as_held(p->smp_r_host, radii, (size_t)disc_count)))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float2* pos_rows = nullptr;
  float* r = nullptr;
  if (samples > 0)  // [sample][disc][row] is [item][row] with S * K items: by_row gives [row][sample][disc]
    TRY(staged([&]() -> int {
      TRY(dev_stage(&pos_rows, by_row<float2>(positions, (size_t)samples * (size_t)disc_count, (size_t)rows).data(), n_pos));
      TRY(dev_stage(&r, radii, (size_t)disc_count));
      return MPPI_OK;
    }, pos_rows, r));
  dev_take(p->smp_pos_rows, pos_rows);
  dev_take(p->smp_r, r);
  const bool moved = p->smp_rows > 1 || (samples > 0 && rows > 1);  // (a set of one row is static: it leaves "now" alone)
  p->smp_on = samples > 0;
  p->smp_count = samples;
  p->smp_discs = samples > 0 ? disc_count : 0;
  p->smp_rows = samples > 0 ? rows : 0;
  p->smp_gen = samples > 0 ? next_generation() : 0;
  p->smp_pos_host.assign(positions, positions + 2 * n_pos);
  p->smp_r_host.assign(radii, radii + (samples > 0 ? (size_t)disc_count : 0));
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
  if ((on != 0) == p->crowd) return MPPI_OK;
  if (!on) {
    REQUIRE(!p->smp_on, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds disc samples, which only the crowd kernel rolls out (clear them first)");
    REQUIRE(p->n_walls == 0, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds %d walls, which only the crowd kernel tests (clear the walls first)", p->n_walls);
    REQUIRE(!p->wtrk_on, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds wall tracks, which only the crowd kernel tests (clear them first)");
    REQUIRE(!p->fleet_on, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle is in fleet mode, whose walls only the crowd kernel tests (mppi_planner_set_fleet(p, 0, NULL) first)");
    REQUIRE(p->fp_count == 0, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds a footprint of %d discs, which only the crowd kernel tests (mppi_planner_set_footprint(p, NULL, 0) first)",
            p->fp_count);
    REQUIRE(p->ring_count == 0, MPPI_ERR_INVALID,
            "crowd mode stays on: the handle holds %d clearance rings, which only the crowd kernel counts (mppi_planner_set_clearance_rings(p, NULL, 0) first)",
            p->ring_count);
    BareboneHeld now = barebone_held(p);  // (without rotation: every set at its own size, the least a launch can ask for)
    now.crowd = false;
    BareboneHeld own = now, shared = now, tracks = now;
    tracks.gtrk_on = own.gtrk_on = shared.gtrk_on = false;
    own.trk_on = shared.trk_on = shared.inst_obs_on = false;
    const struct { bool held; BareboneHeld state; const char* what; } sets[] = {
        {p->trk_on, tracks, "disc tracks"}, {p->inst_obs_on, own, "per-problem disc obstacles"},
        {true, shared, "disc obstacles"}, {p->gtrk_on, now, "discs held with a goal track"}};
    for (const auto& s : sets) {
      const BareboneChoice c = barebone_choose(s.state);
      REQUIRE(!s.held || c.family != kBareboneRefused, MPPI_ERR_INVALID,
              "crowd mode stays on: the %s (%d discs, %d steps) need %zu bytes, more than 64 KiB of LDS", s.what, c.kmax, now.T, c.lds);
    }
  }
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float2* pos_rows = nullptr;
  if (on && p->trk_on)
    TRY(staged([&]() -> int {
      const size_t total = p->trk_r_host.size(), rows = (size_t)p->trk_rows;
      return dev_stage(&pos_rows, by_row<float2>(p->trk_pos_host.data(), total, rows).data(), total * rows);
    }, pos_rows));
  dev_take(p->trk_pos_rows, pos_rows);
  p->crowd = on != 0;
  drop_graphs(p);  // (the kernel form is part of the captured launches)
  return MPPI_OK;
}

extern "C" int mppi_planner_get_crowd(mppi_planner* p, int* on) {
  REQUIRE(p && on, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "crowd mode belongs to the barebone mode (mode %d)", p->cfg.mode);
  *on = p->crowd ? 1 : 0;
  return MPPI_OK;
}

// ---- fleet mode (include/mppi_hip.h; fleet_kernels.h) ------------------------------------------------------------------------
// The device arrays of a fleet: built new-first, so that a failure leaves the handle with what it had.
struct FleetArrays {
  float4* seg_rows = nullptr;
  float* hw = nullptr;
  int2* range = nullptr;
  float2* plan = nullptr;
  float* heads = nullptr;      // a body fleet: [B][T + 1] headings ...
  float2* centres = nullptr;   // ... and [B][T + 1][body] body disc centres
  int slots = 0;
  int group = 1, body = 0;     // slots per other robot; body discs per robot (0: a disc fleet)
};

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

// (the stream has drained) the handle takes the new arrays and a new generation
static void fleet_commit(mppi_planner* p, const FleetArrays& f) {
  dev_take(p->fleet_seg_rows, f.seg_rows);
  dev_take(p->fleet_hw, f.hw);
  dev_take(p->fleet_range, f.range);
  dev_take(p->fleet_plan, f.plan);
  dev_take(p->fleet_heads, f.heads);
  dev_take(p->fleet_centres, f.centres);
  p->fleet_slots = f.slots;
  p->fleet_group = f.group;
  p->fleet_body = f.body;
  p->fleet_on = f.seg_rows != nullptr;
  p->fleet_gen = p->fleet_on ? next_generation() : 0;
}

// ---- walls ---------------------------------------------------------------------------------------------------------------
// Walls (include/mppi_hip.h): crowd mode only -- they are one more source of hits for the count waves of
// k_rollout_barebone_crowd<..., WALLS> and nothing the default forms know.  A change takes a new generation (the graph
// signature's view of the walls).
extern "C" int mppi_planner_set_walls(mppi_planner* p, const float* segments, const float* halfwidths, int count) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "walls belong to the barebone mode (mode %d)", p->cfg.mode);
  REQUIRE(count >= 0 && count <= (1 << 24) && (count == 0 || (segments && halfwidths)), MPPI_ERR_INVALID, "bad wall arrays (count %d)", count);
  REQUIRE(count == 0 || p->crowd, MPPI_ERR_INVALID,
          "walls need crowd mode: only the crowd kernel tests them (mppi_planner_set_crowd(p, 1) first)");
  TRY(check_halfwidths(halfwidths, (size_t)count, "wall"));
  TRY(check_finite(segments, (size_t)count, 1, 4, "wall"));
  if (count == p->n_walls && same_as_held(p->wall_seg_host, segments, 4 * (size_t)count) &&
      same_as_held(p->wall_hw_host, halfwidths, (size_t)count))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float4* seg = nullptr;
  float* hw = nullptr;
  // fleet mode: these walls lie behind the other robots in every reader's set -- the fleet storage is rebuilt with the
  // new walls, in the same stage
  FleetArrays fleet;
  TRY(staged([&]() -> int {
    if (count > 0) TRY(dev_stage(&seg, segments, (size_t)count));
    if (count > 0) TRY(dev_stage(&hw, halfwidths, (size_t)count));
    if (p->fleet_on) TRY(fleet_build(p, p->fleet_hw_host.data(), segments, halfwidths, count, p->fleet_group, p->fleet_body, &fleet));
    return MPPI_OK;
  }, seg, hw));
  if (p->fleet_on) fleet_commit(p, fleet);
  dev_take(p->wall_seg, seg);
  dev_take(p->wall_hw, hw);
  p->wall_seg_host.assign(segments, segments + 4 * (size_t)count);
  p->wall_hw_host.assign(halfwidths, halfwidths + (size_t)count);
  p->n_walls = count;
  p->wall_gen = count > 0 ? next_generation() : 0;
  drop_graphs(p);  // (the arrays, the count and the kernel form are arguments of the captured launches)
  return MPPI_OK;
}

// Walls that move, and a wall set per problem (include/mppi_hip.h): crowd mode only, like the static walls.  `rows`
// segments per wall, one set shared by every problem (count == 1) or one per problem (count == B), the sets one after the
// other, each [wall][row].  The device keeps them [row][wall] -- a step's walls are contiguous -- with {wall0, count} per
// problem beside them.  A change takes a new generation and, for walls that move (rows > 1), makes row 0 "now" again.
extern "C" int mppi_planner_set_wall_tracks(mppi_planner* p, int count, const int* wall_counts, int rows,
                                            const float* segments, const float* halfwidths) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "wall tracks belong to the barebone mode (mode %d)", p->cfg.mode);
  if (wall_counts == nullptr) count = 0;
  TRY(check_set_count(p, count, "set"));
  long total = 0;
  int wmax = 0;
  if (count > 0) {
    REQUIRE(!p->fleet_on, MPPI_ERR_INVALID,
            "the handle is in fleet mode, which owns the per-problem wall sets: turn it off first (mppi_planner_set_fleet(p, 0, NULL))");
    REQUIRE(p->crowd, MPPI_ERR_INVALID,
            "wall tracks need crowd mode: only the crowd kernel tests them (mppi_planner_set_crowd(p, 1) first)");
    REQUIRE(rows >= 1 && rows <= (1 << 20), MPPI_ERR_INVALID, "rows %d: a wall track has at least one row", rows);
    TRY(sum_counts(count, wall_counts, "wall", &total, &wmax));
    REQUIRE(total <= (1L << 24) && total * (long)rows <= (1L << 28), MPPI_ERR_INVALID, "too many wall track rows (%ld walls x %d)", total, rows);
    REQUIRE(total == 0 || (segments && halfwidths), MPPI_ERR_INVALID, "NULL segments or halfwidths");
    TRY(check_halfwidths(halfwidths, (size_t)total, "wall"));
    TRY(check_finite(segments, (size_t)total, (size_t)rows, 4, "wall"));
  }
  const size_t n_seg = (size_t)total * (size_t)rows;
  if (count == 0 ? !p->wtrk_on
                 : (p->wtrk_on && rows == p->wtrk_rows && same_as_held(p->wtrk_counts_host, wall_counts, (size_t)count) &&
                    same_as_held(p->wtrk_seg_host, segments, 4 * n_seg) && same_as_held(p->wtrk_hw_host, halfwidths, (size_t)total)))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float4* seg_rows = nullptr;
  float* hw = nullptr;
  int2* range = nullptr;
  if (count > 0) {
    std::vector<int2> ranges((size_t)count);
    for (int b = 0, k0 = 0; b < count; k0 += wall_counts[b], ++b) ranges[(size_t)b] = make_int2(k0, wall_counts[b]);
    TRY(staged([&]() -> int {
      TRY(dev_stage(&seg_rows, by_row<float4>(segments, (size_t)total, (size_t)rows).data(), std::max<size_t>(1, n_seg)));
      TRY(dev_stage(&hw, halfwidths, (size_t)total));
      TRY(dev_stage(&range, ranges.data(), ranges.size()));
      return MPPI_OK;
    }, seg_rows, hw, range));
  }
  dev_take(p->wtrk_seg_rows, seg_rows);
  dev_take(p->wtrk_hw, hw);
  dev_take(p->wtrk_range, range);
  const bool moved = p->wtrk_rows > 1 || (count > 0 && rows > 1);
  p->wtrk_on = count > 0;
  p->wtrk_rows = count > 0 ? rows : 0;
  p->wtrk_max = wmax;
  p->wtrk_gen = count > 0 ? next_generation() : 0;
  p->wtrk_counts_host.assign(wall_counts, wall_counts + count);
  p->wtrk_seg_host.assign(segments, segments + 4 * n_seg);
  p->wtrk_hw_host.assign(halfwidths, halfwidths + (size_t)total);
  drop_graphs(p);  // (the arrays, the counts, the row count and the kernel form are arguments of the captured launches)
  reset_track_offsets(p, kWallTracks, moved, count == 0);
  return MPPI_OK;
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
    REQUIRE(rows >= 1 && rows <= (1 << 20), MPPI_ERR_INVALID, "rows %d: a goal track has at least one row", rows);
    REQUIRE((long)count * (long)rows <= (1L << 28), MPPI_ERR_INVALID, "too many goal track rows (%d tracks x %d)", count, rows);
    REQUIRE(xy, MPPI_ERR_INVALID, "NULL xy");
    n_xy = (size_t)count * (size_t)rows;
    TRY(check_finite(xy, (size_t)count, (size_t)rows, 2, "goal track"));
  }
  if (count == 0 ? !p->gtrk_on
                 : (p->gtrk_on && rows == p->gtrk_rows && count == p->gtrk_count && same_as_held(p->gtrk_host, xy, 2 * n_xy)))
    return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float2* fresh = nullptr;
  if (count > 0) TRY(staged([&]() -> int { return dev_stage(&fresh, xy, n_xy); }, fresh));
  dev_take(p->gtrk_xy, fresh);
  const bool moved = p->gtrk_rows > 1 || (count > 0 && rows > 1);
  p->gtrk_on = count > 0;
  p->gtrk_rows = count > 0 ? rows : 0;
  p->gtrk_count = count;
  p->gtrk_gen = count > 0 ? next_generation() : 0;
  p->gtrk_host.assign(xy, xy + 2 * n_xy);
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
  if (count == 0) {
    if (!p->fleet_on) return MPPI_OK;
    HIP_TRY(hipSetDevice(p->cfg.device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (p->fleet_body > 0) {  // (a body fleet holds its body as the handle's footprint: it goes with the fleet)
      memset(p->fp_host, 0, sizeof(p->fp_host));
      p->fp_count = 0;
      p->fp_gen = 0;
      p->fleet_margin = 0.0;
    }
    fleet_commit(p, FleetArrays());
    p->fleet_hw_host.clear();
    drop_graphs(p);  // (the arrays and the kernel form are arguments of the captured launches)
    return MPPI_OK;
  }
  REQUIRE(p->B >= 2, MPPI_ERR_INVALID,
          "fleet mode needs a batched handle of at least two problems, one per robot (num_instances %d)", p->B);
  REQUIRE(count == p->B, MPPI_ERR_INVALID, "count %d: must be 0 (off) or num_instances %d", count, p->B);
  REQUIRE(p->cfg.world_size == 1, MPPI_ERR_INVALID, "fleet mode drives an unsharded handle");
  REQUIRE(p->crowd, MPPI_ERR_INVALID,
          "fleet mode needs crowd mode: only the crowd kernel tests walls (mppi_planner_set_crowd(p, 1) first)");
  REQUIRE(!p->wtrk_on, MPPI_ERR_INVALID,
          "the handle holds wall tracks or per-problem wall sets; fleet mode makes every problem's set itself: clear them "
          "first (mppi_planner_set_wall_tracks with count 0)");
  REQUIRE(!(p->fleet_on && p->fleet_body > 0), MPPI_ERR_INVALID, "%s", kFleetKinds);
  REQUIRE(p->fp_count == 0, MPPI_ERR_INVALID,
          "the handle holds a footprint; the fleet's half-widths already contain the reader's body: clear it first "
          "(mppi_planner_set_footprint(p, NULL, 0))");
  REQUIRE(halfwidths, MPPI_ERR_INVALID, "NULL halfwidths");
  const size_t pairs = (size_t)p->B * (size_t)(p->B - 1);
  TRY(check_halfwidths(halfwidths, pairs, "fleet pair"));
  if (p->fleet_on && memcmp(halfwidths, p->fleet_hw_host.data(), sizeof(float) * pairs) == 0) return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  FleetArrays fleet;
  TRY(fleet_build(p, halfwidths, p->wall_seg_host.data(), p->wall_hw_host.data(), p->n_walls, 1, 0, &fleet));
  fleet_commit(p, fleet);
  p->fleet_hw_host.assign(halfwidths, halfwidths + pairs);
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
  REQUIRE(p->B >= 2, MPPI_ERR_INVALID,
          "fleet mode needs a batched handle of at least two problems, one per robot (num_instances %d)", p->B);
  REQUIRE(count == p->B, MPPI_ERR_INVALID, "count %d: must be 0 (off) or num_instances %d", count, p->B);
  REQUIRE(p->cfg.world_size == 1, MPPI_ERR_INVALID, "fleet mode drives an unsharded handle");
  REQUIRE(p->crowd, MPPI_ERR_INVALID,
          "fleet mode needs crowd mode: only the crowd kernel tests walls (mppi_planner_set_crowd(p, 1) first)");
  REQUIRE(!p->wtrk_on, MPPI_ERR_INVALID,
          "the handle holds wall tracks or per-problem wall sets; fleet mode makes every problem's set itself: clear them "
          "first (mppi_planner_set_wall_tracks with count 0)");
  REQUIRE(!(p->fleet_on && p->fleet_body == 0), MPPI_ERR_INVALID, "%s", kFleetKinds);
  REQUIRE(p->fleet_body > 0 || p->fp_count == 0, MPPI_ERR_INVALID,
          "the handle holds a footprint; a body fleet carries its own body: clear it first (mppi_planner_set_footprint(p, NULL, 0))");
  REQUIRE(n_discs >= 1 && n_discs <= kCrowdFootprintMax, MPPI_ERR_INVALID, "body of %d discs: must be 1 to %d", n_discs, kCrowdFootprintMax);
  REQUIRE(discs, MPPI_ERR_INVALID, "NULL discs");
  TRY(check_footprint_rows(discs, n_discs));
  REQUIRE(std::isfinite(margin), MPPI_ERR_INVALID, "margin %g is not finite", margin);
  for (int k = 0; k < n_discs; ++k)
    REQUIRE((double)discs[3 * k + 2] + margin >= 0.0, MPPI_ERR_INVALID,
            "body disc %d: radius %g and margin %g give a negative half-width", k, (double)discs[3 * k + 2], margin);
  if (p->fleet_on && p->fleet_body == n_discs && margin == p->fleet_margin &&
      memcmp(discs, p->fp_host, sizeof(float) * 3 * (size_t)n_discs) == 0)
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
  TRY(fleet_build(p, hw.data(), p->wall_seg_host.data(), p->wall_hw_host.data(), p->n_walls, group, n_discs, &fleet));
  fleet_commit(p, fleet);
  p->fleet_hw_host = hw;
  p->fleet_margin = margin;
  memset(p->fp_host, 0, sizeof(p->fp_host));
  memcpy(p->fp_host, discs, sizeof(float) * 3 * (size_t)n_discs);
  p->fp_count = n_discs;
  p->fp_gen = next_generation();
  drop_graphs(p);  // (the arrays, the rows, the counts and the kernel form are arguments of the captured launches)
  return MPPI_OK;
}

// *n_discs: the body discs of the body fleet that is on, else 0; *margin: its margin
extern "C" int mppi_planner_get_fleet_bodies(mppi_planner* p, int* n_discs, double* margin) {
  REQUIRE(p && n_discs && margin, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "fleet mode belongs to the barebone mode (mode %d)", p->cfg.mode);
  *n_discs = p->fleet_on ? p->fleet_body : 0;
  *margin = p->fleet_on ? p->fleet_margin : 0.0;
  return MPPI_OK;
}

extern "C" int mppi_planner_get_fleet(mppi_planner* p, int* on) {
  REQUIRE(p && on, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "fleet mode belongs to the barebone mode (mode %d)", p->cfg.mode);
  *on = p->fleet_on ? p->B : 0;
  return MPPI_OK;
}

// ---- a body footprint ----------------------------------------------------------------------------------------------------
// A body footprint (include/mppi_hip.h): crowd mode only, and not beside the fleet.  The rows are a by-value argument of the
// launches: there is no device array, so nothing to stage -- but the stream is drained like everywhere else, and a change
// takes a new generation (the graph signature's view of the footprint) and drops the captured graphs.
extern "C" int mppi_planner_set_footprint(mppi_planner* p, const float* discs, int count) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "a footprint belongs to the barebone mode (mode %d)", p->cfg.mode);
  REQUIRE(count >= 0 && count <= kCrowdFootprintMax, MPPI_ERR_INVALID, "footprint of %d discs: must be 0 (none) to %d", count, kCrowdFootprintMax);
  REQUIRE(!(p->fleet_on && p->fleet_body > 0), MPPI_ERR_INVALID,
          "the handle is in a body fleet, which carries its own body: turn the fleet off first (mppi_planner_set_fleet(p, 0, NULL))");
  if (count > 0) {
    REQUIRE(discs, MPPI_ERR_INVALID, "NULL discs");
    REQUIRE(p->crowd, MPPI_ERR_INVALID,
            "a footprint needs crowd mode: only the crowd kernel has footprint forms (mppi_planner_set_crowd(p, 1) first)");
    REQUIRE(!p->fleet_on, MPPI_ERR_INVALID,
            "the handle is in fleet mode, whose half-widths already contain the reader's body: turn it off first "
            "(mppi_planner_set_fleet(p, 0, NULL))");
    TRY(check_footprint_rows(discs, count));
  }
  if (count == p->fp_count && (count == 0 || memcmp(discs, p->fp_host, sizeof(float) * 3 * (size_t)count) == 0)) return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  memset(p->fp_host, 0, sizeof(p->fp_host));
  if (count > 0) memcpy(p->fp_host, discs, sizeof(float) * 3 * (size_t)count);
  p->fp_count = count;
  p->fp_gen = count > 0 ? next_generation() : 0;
  drop_graphs(p);  // (the rows, the count and the kernel form are arguments of the captured launches)
  return MPPI_OK;
}

extern "C" int mppi_planner_get_footprint(mppi_planner* p, float* discs, int* count) {
  REQUIRE(p && discs && count, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "a footprint belongs to the barebone mode (mode %d)", p->cfg.mode);
  memcpy(discs, p->fp_host, sizeof(p->fp_host));
  *count = p->fp_count;
  return MPPI_OK;
}

// ---- clearance rings -----------------------------------------------------------------------------------------------------
// Clearance rings (include/mppi_hip.h): crowd mode only, and not beside disc samples.  Like the footprint's, the rows are a
// by-value argument of the launches: nothing to stage, a new generation and no captured graphs at every change.
extern "C" int mppi_planner_set_clearance_rings(mppi_planner* p, const float* rings, int count) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "clearance rings belong to the barebone mode (mode %d)", p->cfg.mode);
  REQUIRE(count >= 0 && count <= kCrowdRingsMax, MPPI_ERR_INVALID, "%d clearance rings: must be 0 (none) to %d", count, kCrowdRingsMax);
  if (count > 0) {
    REQUIRE(rings, MPPI_ERR_INVALID, "NULL rings");
    REQUIRE(p->crowd, MPPI_ERR_INVALID,
            "clearance rings need crowd mode: only the crowd kernel has ring forms (mppi_planner_set_crowd(p, 1) first)");
    REQUIRE(!p->smp_on, MPPI_ERR_INVALID,
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
  if (count == p->ring_count && (count == 0 || memcmp(rings, p->ring_host, sizeof(float) * 2 * (size_t)count) == 0)) return MPPI_OK;
  HIP_TRY(hipSetDevice(p->cfg.device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  memset(p->ring_host, 0, sizeof(p->ring_host));
  if (count > 0) memcpy(p->ring_host, rings, sizeof(float) * 2 * (size_t)count);
  p->ring_count = count;
  p->ring_gen = count > 0 ? next_generation() : 0;
  drop_graphs(p);  // (the rows, the count and the kernel form are arguments of the captured launches)
  return MPPI_OK;
}

extern "C" int mppi_planner_get_clearance_rings(mppi_planner* p, float* rings, int* count) {
  REQUIRE(p && rings && count, MPPI_ERR_INVALID, "NULL argument");
  REQUIRE(p->cfg.mode == MPPI_MODE_BAREBONE, MPPI_ERR_INVALID, "clearance rings belong to the barebone mode (mode %d)", p->cfg.mode);
  memcpy(rings, p->ring_host, sizeof(p->ring_host));
  *count = p->ring_count;
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
  if (!p->fleet_on) return MPPI_OK;
  REQUIRE(p->params_set, MPPI_ERR_STATE, "params not set");
  REQUIRE(p->inst_set, MPPI_ERR_STATE, "num_instances = %d: call mppi_planner_set_instances before solving", p->B);
  TRY(upload_instances(p));
  const DevParams d = make_dev_params(p);
  const int B = p->B, T = p->cfg.num_steps;
  REQUIRE((size_t)T * sizeof(double2) <= 64 * 1024, MPPI_ERR_INVALID, "num_steps %d too large", T);  // (as launch_rollout)
  const size_t lds = fleet_plans_lds_bytes(T);  // (28 bytes a step: 112 KiB at the 4096 steps the line above admits)
  const bool exact = p->cfg.math == MPPI_MATH_EXACT, body = p->fleet_body > 0;
  auto plans = body ? (exact ? &k_fleet_plans<true, true> : &k_fleet_plans<false, true>)
                    : (exact ? &k_fleet_plans<true, false> : &k_fleet_plans<false, false>);
  if (lds > 64 * 1024)  // (a horizon of more than ~2300 steps)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(plans), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(plans, dim3(B), dim3(64), lds, p->stream, d, p->u, done, p->fleet_plan, body ? p->fleet_heads : nullptr);
  HIP_TRY(hipGetLastError());
  if (body) {  // the body discs' centres once per (robot, state), then the scatter into every reader's slots
    const int states = B * (T + 1), F = p->fleet_body, Fp = p->fleet_group;
    hipLaunchKernelGGL(k_fleet_body_centres, dim3(ceil_div(states, 256)), dim3(256), 0, p->stream, p->fleet_plan, p->fleet_heads,
                       p->fleet_centres, states, footprint_arg(p));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fleet_body_walls, dim3(ceil_div((long)B * (B - 1) * Fp, 256), T), dim3(256), 0, p->stream, p->fleet_centres,
                       p->fleet_seg_rows, B, T, p->fleet_slots, F, Fp);
    HIP_TRY(hipGetLastError());
    return MPPI_OK;
  }
  hipLaunchKernelGGL(k_fleet_walls, dim3(ceil_div((long)B * (B - 1), 256), T), dim3(256), 0, p->stream, p->fleet_plan,
                     p->fleet_seg_rows, B, T, p->fleet_slots);
  HIP_TRY(hipGetLastError());
  return MPPI_OK;
}

extern "C" int mppi_planner_fleet_refresh(mppi_planner* p) {
  REQUIRE(p, MPPI_ERR_INVALID, "NULL planner");
  REQUIRE(p->fleet_on, MPPI_ERR_STATE, "the handle is not in fleet mode (mppi_planner_set_fleet)");
  HIP_TRY(hipSetDevice(p->cfg.device));
  TRY(fleet_refresh(p, nullptr));
  return drain_stream(p);
}

