// update_plan.h -- how the weights of a rollout launch become the next u: which route the update takes (left to the next
// rollout launch, a local launch, an all-gather), which kernel a local launch runs and in what form, and what the next
// rollout launch can take over -- as pure functions of what the handle holds.  Plain C++ without a HIP type: a host
// program compiles it on its own (tests/test_update_plan.py pins the table).  update_held(p, ...) (launch_plan.h) fills
// the state from a handle; launch_update and its launchers there carry a choice out and keep every side effect.
#pragma once

#include <algorithm>
#include <cstddef>

#include "../../include/mppi_hip.h"
#include "lds_layouts.h"

// What the choice depends on, and nothing else: no pointer.
struct UpdateHeld {
  // configuration
  int mode, world_size, has_comm, m_count, B, inst_set, n_local, n_inst, inst_tiles, T, rng;
  // switches: ... flags_env_off: MPPI_NO_NOISE_FLAG; flag_words: the noise flag and the progress word both exist
  int debug_flags, fold_off, p2p_on, graph_on, stream_flags_off, flags_env_off, flag_words;
  // this call (launch_iteration's arguments; a stage-level call: all zero but mirror_now)
  int prof, defer_exchange, may_leave_apply, mirror_now, want_next, have_noise, side_stream_pays;
  // what the last rollout launch left
  int scan_packets_fresh, tile_packets_fresh, scan_tile;
  // what the next rollout launch would be (map_plan.h: map_choose): a time-parallel kernel, and its tile
  int next_scan, next_tile;
};

inline int update_ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// ---- the limits, each written once -----------------------------------------------------------------------------------
// k_update_rows keeps one float per tile of a problem in LDS (two when it forms the tile weights from the costs itself)
constexpr size_t kUpdateLdsMax = 60 * 1024;
inline size_t update_rows_lds(int inst_tiles, bool from_costs) { return sizeof(float) * (size_t)inst_tiles * (from_costs ? 2 : 1); }
inline bool update_from_costs_fits(int inst_tiles) { return update_rows_lds(inst_tiles, true) <= kUpdateLdsMax; }
// rows per workgroup of k_update_rows: 4 where the grid would otherwise be thousands of short-lived workgroups
inline bool update_many_rows(int T, int B) { return (long)T * B >= 2048; }
constexpr int kUpdateRowsBlock = 1024, kUpdateRowsSlimBlock = 256;  // (update_kernels.h: kRowThreads, THREADS)
// (below ~4M rollout-steps a noise generator takes less than the ~12 us a cross-stream dependency costs)
inline bool update_noise_is_long(int n_local, int T) { return (long)n_local * T >= 4L * 1000 * 1000; }

// One GPU: whether a rollout launch over `tiles` workgroups can combine its predecessor's tile packets itself
// (update_kernels.h, PendingApply::reduce_tiles): step t in workgroup t, at most two steps per idle walker wave.
inline bool tiles_can_reduce(int tiles, int n_steps) { return 4 * tiles >= n_steps; }

// ---- what the next rollout launch takes ------------------------------------------------------------------------------
// one problem per handle, all its traction samples here: what every fold and the peer exchange ask
inline bool update_one_problem(const UpdateHeld& h) { return h.B == 1 && !h.inst_set && h.m_count == 1; }
inline bool update_single_gpu(const UpdateHeld& h) { return h.world_size == 1 && !h.has_comm; }

// Several GPUs without a collective: the peer exchange is connected and the kernels that carry it will run (the
// time-parallel kernels leave tile packets; one problem per handle).  Decided from things every rank has alike.
inline bool update_p2p_usable(const UpdateHeld& h) {
  return h.p2p_on && h.world_size > 1 && h.world_size <= mppi::kMaxFoldedRanks && update_one_problem(h) &&
         h.mode == MPPI_MODE_DET && h.next_scan;
}

struct RolloutTakes {
  bool applies_packets;  // the gathered rank packets of a sharded update (PendingApply)
  bool reduces_tiles;    // the tile packets of the launch before it: combines and applies them, no update kernel
};

// What the NEXT rollout launch of this handle can take over from an update.
// (Kept as it is: reduces_tiles admits the speed-map mode, while the packet fold and the peer exchange -- through which
//  several GPUs reach reduces_tiles -- admit deterministic dynamics only.)
inline RolloutTakes next_rollout_takes(const UpdateHeld& h) {
  const bool common = !(h.debug_flags & MPPI_DEBUG_NO_FOLDED_APPLY) && update_one_problem(h) && !h.mirror_now && h.next_scan;
  RolloutTakes t;
  t.applies_packets = common && h.world_size <= mppi::kMaxFoldedRanks && h.mode == MPPI_MODE_DET;
  t.reduces_tiles = common && !h.fold_off && !(h.debug_flags & MPPI_DEBUG_NO_REDUCE_FOLD) &&
                    (update_single_gpu(h) || update_p2p_usable(h)) &&
                    (h.mode == MPPI_MODE_DET || h.mode == MPPI_MODE_SPEED_MAP) && h.next_tile == h.scan_tile &&
                    tiles_can_reduce(update_ceil_div(h.n_local, h.next_tile), h.T);
  return t;
}

// Whether a rollout launch about to be made keeps the rank packets an update left to it (launch_rollout; else k_apply
// runs in front of it).  (Kept as it is: the mode and the kernel family alone, not the whole of applies_packets -- a
// debug flag set or a mirror asked for since the packets were left does not take them away from the launch.)
inline bool rollout_keeps_pending_packets(const UpdateHeld& h) { return h.mode == MPPI_MODE_DET && h.next_scan; }

// ---- the choice ------------------------------------------------------------------------------------------------------
enum UpdateRoute {
  kUpdateLeaveTiles = 0,        // no launch: the next rollout launch combines the tile packets and applies
  kUpdateLocalApply = 1,        // a local launch combines the tiles or streams the rows, and applies
  kUpdatePacketOnly = 2,        // a local launch writes this rank's packet; the caller exchanges (stage-level calls, groups)
  kUpdateGatherApply = 3,       // this rank's packet, all-gather, k_apply
  kUpdateGatherLeaveApply = 4,  // this rank's packet, all-gather; the next rollout launch applies
};
enum UpdateKernel { kUpdateNoKernel = 0, kUpdateCombineTiles = 1, kUpdateRows = 2 };

struct UpdateChoice {
  UpdateRoute route = kUpdateLocalApply;
  // the local launch (every route but the first)
  UpdateKernel kernel = kUpdateNoKernel;
  bool apply_here = false;     // the kernel's APPLY form: u is updated by this launch
  bool peers_ride = false;     // combine-tiles: the peer exchange happens inside the launch
  bool tile_weights_first = false, from_costs = false, slim = false;  // rows: k_tile_weights in front; FROM_COSTS; 256 threads
  int rows_per_wg = 1;         // rows: TC
  int per_problem_tiles = 0;   // combine-tiles: tile packets per problem
  int grid_x = 0, grid_y = 0, block = 0;
  size_t lds = 0;              // rows: what the tile arrays need (refused above kUpdateLdsMax) ...
  size_t lds_launch = 0;       // ... and what the launch asks for
  // the next iteration's noise is generated beside this update launch, which runs slim and signals its start
  bool beside_update = false;
};

// Where the rollout fills the SIMDs by itself (more than 8 of its waves per CU: the batched handles) a generator beside
// it only takes its issue slots; but the update behind it is bound by memory: there the next iteration's noise is
// generated beside the UPDATE launch.  It needs the streams' flags, a generation long enough to pay, and -- the last
// line -- the route that applies locally through k_update_rows within its LDS bound: one GPU, tile weights or costs,
// no tile packets.  update_choose relies on that implication and tests/test_update_plan.py holds it.
inline bool update_noise_beside(const UpdateHeld& h) {
  return h.want_next && !h.have_noise && !h.side_stream_pays && !h.flags_env_off && !h.graph_on && !h.prof &&
         !h.defer_exchange && h.flag_words && !h.stream_flags_off && h.rng == MPPI_RNG_PHILOX &&
         update_noise_is_long(h.n_local, h.T) &&
         !h.scan_packets_fresh && update_single_gpu(h) && h.m_count == 1 && update_from_costs_fits(h.inst_tiles);
}

inline UpdateRoute update_route(const UpdateHeld& h) {
  if (h.defer_exchange) return kUpdatePacketOnly;
  const bool may_leave = h.may_leave_apply && !h.prof;  // (a profiled iteration times an update launch of its own)
  const RolloutTakes next = next_rollout_takes(h);
  // Local or collective.  (Kept as they are: a communicator on a single rank takes the collective route -- it
  // exercises the same path as N ranks; samples sharded (m_count > 1): every rank holds all N costs and all the noise,
  // so the update is local whatever the world size.)
  if (update_single_gpu(h) || h.m_count > 1 || (update_p2p_usable(h) && h.scan_packets_fresh))
    return may_leave && h.scan_packets_fresh && next.reduces_tiles ? kUpdateLeaveTiles : kUpdateLocalApply;
  return may_leave && next.applies_packets ? kUpdateGatherLeaveApply : kUpdateGatherApply;
}

// The local launch of `route` (not kUpdateLeaveTiles), whatever update_route says of the state: tile packets left to a
// rollout launch that will not come are settled by the local-apply launch on any number of GPUs (settle_reduce_pending).
inline UpdateChoice update_local_launch(const UpdateHeld& h, UpdateRoute route) {
  UpdateChoice c;
  c.route = route;
  c.apply_here = route == kUpdateLocalApply;
  c.grid_y = h.B;
  if (h.scan_packets_fresh) {
    // the rollout launch (a time-parallel kernel) has reduced w_rel * noise over every tile: combine the tiles
    c.kernel = kUpdateCombineTiles;
    c.per_problem_tiles = update_ceil_div(h.n_inst, h.scan_tile);
    // (kept as it is: weaker than update_p2p_usable -- any connected exchange of several ranks rides, usable or not)
    c.peers_ride = c.apply_here && h.p2p_on && h.world_size > 1;
    c.grid_x = h.T;
    c.block = 64;
    return c;
  }
  // rollout kernels without the weight epilogue: the row kernel forms the tile weights itself from the costs (same
  // bits) unless there are too many tiles for its LDS arrays
  c.kernel = kUpdateRows;
  c.from_costs = !h.tile_packets_fresh && update_from_costs_fits(h.inst_tiles);
  c.tile_weights_first = !h.tile_packets_fresh && !c.from_costs;
  c.rows_per_wg = update_many_rows(h.T, h.B) ? 4 : 1;
  c.grid_x = update_ceil_div(h.T, c.rows_per_wg);
  c.beside_update = c.slim = update_noise_beside(h);
  // (slim: 256 threads with four times the loads in flight each and at most two workgroups per CU -- 60 KiB of LDS each)
  c.block = c.slim ? kUpdateRowsSlimBlock : kUpdateRowsBlock;
  c.lds = update_rows_lds(h.inst_tiles, c.from_costs);
  c.lds_launch = c.slim ? std::max(c.lds, kUpdateLdsMax) : c.lds;
  return c;
}

inline UpdateChoice update_choose(const UpdateHeld& h) {
  const UpdateRoute route = update_route(h);
  if (route != kUpdateLeaveTiles) return update_local_launch(h, route);
  UpdateChoice c;
  c.route = route;
  return c;
}
