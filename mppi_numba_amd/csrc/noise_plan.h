// noise_plan.h -- where an iteration's noise comes from, who produces the next iteration's, and how the two streams are
// ordered around it, as a pure function of what the handle holds.  Plain C++ without a HIP type: a host program compiles
// it on its own (tests/test_noise_plan.py pins the table).  noise_held(p, ...) (launch_plan.h) fills the state from a
// handle; launch_iteration and launch_noise_ahead there carry a choice out and keep every side effect.
//
//   this iteration's noise                                  the consumer waits behind the generator by
//   in the rollout launch, from the Philox counters        --
//   taken from ahead: blocks of the previous launch        -- (the same stream)
//   taken from ahead: the second stream                    the flag (k_rollout_fused looks itself) or ev_noise_ready
//   in line                                                -- (the same stream)
//
//   the next iteration's noise                              the generator waits behind the buffer's last reader by
//   spare / appended workgroups of the rollout launch      -- (the previous update is ahead of the launch)
//   second stream beside the rollout                       ev_buf_free in front | the launch's progress word | ev_buf_free behind
//   second stream beside the update                        the update launch's progress word
//   none of these: in line, by the next iteration
#pragma once

#include <algorithm>

#include "update_plan.h"

// the coming rollout launch (map modes: MapFamily + 1); 0: no iteration is being launched
enum NoiseLaunch {
  kLaunchNone = 0, kLaunchScan = 1, kLaunchScanExact = 2, kLaunchPipe = 3, kLaunchFused = 4, kLaunchGeneral = 5,
  kLaunchCvarFast = 6, kLaunchCvar = 7, kLaunchBarebone = 8,
};

// What the choice depends on, and nothing else: no pointer.
struct NoiseHeld {
  // configuration
  int rng, n_local, T, num_cus, num_grid_samples;
  // switches: debug_flags: MPPI_DEBUG_SCAN_READ_NOISE and MPPI_DEBUG_DROP_NOISE_FLAG matter; flags_env_off:
  // MPPI_NO_NOISE_FLAG; flag_words: the noise flag and the progress word exist
  int debug_flags, graph_on, stream_flags_off, flags_env_off, flag_words;
  // this call (launch_iteration's arguments)
  int want_next, have_noise;
  // what is in flight: the noise ahead is still on the second stream; the previous iteration's rollout launch signalled
  int noise_on_side_stream, prev_signalled;
  // the coming rollout launch (map_choose; the CVaR and barebone launchers): which, its workgroups (scan: tiles), and
  // whether a time-parallel kernel is the exact one
  int launch, workgroups, scan_exact;
  // update_choose for the coming update, asked as if the rollout launch left no noise and the second stream did not pay
  // beside it: the update launch would host the generator (update_plan.h: update_noise_beside)
  int update_can_host;
};

// ---- the limits, each written once -----------------------------------------------------------------------------------
// (below ~4M rollout-steps the generator takes less than the ~12 us a cross-stream dependency costs: update_noise_is_long)
// and above 8 rollout waves per CU the register file has room for one generator wave per SIMD only: the generator
// crawls beside the rollout, slows it, and still collides with the update (measured in round 1, profiles/r01_ablation.md,
// and again in round 6 with a bound of 16: C5 187 us against 178, profiles/r06_ns_notes.md section 3)
constexpr int kSideStreamMaxWaves = 8;
inline bool side_stream_pays(int n_local, int T, int num_cus) {
  return update_noise_is_long(n_local, T) && update_ceil_div(update_ceil_div(n_local, 64), num_cus) <= kSideStreamMaxWaves;
}

// threads of the CVaR kernels: one per traction sample, whole waves, at most 1024
inline int noise_cvar_threads(int num_grid_samples) { return std::min(update_ceil_div(num_grid_samples, 64) * 64, 1024); }

// k_rollout_fused signals its start through the progress word (a captured launch would signal a stale number)
inline bool noise_launch_signals(bool flag_words, bool flags_env_off, bool graph_on, bool stream_flags_off) {
  return flag_words && !flags_env_off && !graph_on && !stream_flags_off;
}

// ---- the choice ------------------------------------------------------------------------------------------------------
enum NoiseSource { kNoiseInLine = 0, kNoiseAhead = 1, kNoiseInKernel = 2 };
enum NoiseOrder { kOrderNone = 0, kOrderFlag = 1, kOrderEvent = 2 };
enum NoiseHold { kHoldNone = 0, kHoldEventFront = 1, kHoldGate = 2, kHoldEventBehind = 3 };
enum NoiseAnnounce { kAnnounceNone = 0, kAnnounceFlag = 1, kAnnounceDropped = 2 };

// All zero: no iteration is being launched (a stage-level rollout reads the noise that is there and appends nothing).
struct NoiseChoice {
  int launch = kLaunchNone;     // the launch this was chosen for: the launchers check that it is the one they make
  int source = kNoiseInLine;    // this iteration's noise
  int discard_ahead = 0;        // in-kernel: noise produced ahead by an earlier, different kind of launch is dropped
  int consumer = kOrderNone;    // taken from the second stream: how the rollout launch is ordered behind the generator
  int extra_blocks = 0;         // workgroups the rollout launch appends for the next iteration's noise
  int side_stream_pays = 0;
  int record_front = 0;         // ev_buf_free is recorded in front of the rollout launch
  int signals = 0;              // the rollout launch signals its start (the next iteration's prev_signalled)
  int beside_rollout = 0, beside_update = 0;  // the second stream generates beside the rollout | the update ...
  int hold = kHoldNone;         // ... held back behind the buffer's last reader so ...
  int announce = kAnnounceNone; // ... and says so through the flag (dropped: the sequence number moves, nothing is stored)
  int join = 0;                 // graph mode: the main stream waits for the generator before the update
  int have_after_rollout = 0;   // noise_buf[noise_cur ^ 1] holds the next iteration's noise behind the rollout launch ...
  int have_noise = 0;           // ... and on return
};

inline NoiseChoice noise_choose(const NoiseHeld& h) {
  NoiseChoice c;
  c.launch = h.launch;
  const bool philox = h.rng == MPPI_RNG_PHILOX;
  const bool scan = h.launch == kLaunchScan || h.launch == kLaunchScanExact;
  const bool flags_on = h.flag_words && !h.flags_env_off && !h.stream_flags_off;
  bool want_next = h.want_next != 0;
  // MPPI_MATH_FAST or exact over a map the time-parallel kernel takes: the rollout launch computes its noise from the
  // Philox counters itself; nothing is generated ahead, nothing is stored
  if (scan && philox && !(h.debug_flags & MPPI_DEBUG_SCAN_READ_NOISE)) {
    c.source = kNoiseInKernel;
    c.discard_ahead = h.have_noise;
    want_next = false;
  } else if (h.have_noise) {
    c.source = kNoiseAhead;
    // (graph mode has joined the streams already: noise_on_side_stream is never set there)
    if (h.noise_on_side_stream) c.consumer = h.launch == kLaunchFused && flags_on ? kOrderFlag : kOrderEvent;
  }
  // The blocks a rollout launch appends.  (Kept as they are: the time-parallel kernel appends for the tolerance kernel
  // only -- the exact one generates in line -- and asks for Philox; the pipelined kernel does not ask.)
  if (want_next && h.launch == kLaunchScan && philox && h.workgroups < h.num_cus) c.extra_blocks = h.num_cus - h.workgroups;
  if (want_next && h.launch == kLaunchPipe && h.workgroups < h.num_cus) c.extra_blocks = h.num_cus - h.workgroups;
  if (want_next && h.launch == kLaunchCvarFast && philox) {  // (they run in the launch's tail)
    const long rows = (long)update_ceil_div(h.n_local, 64) * ((h.T + 1) / 2);  // of 64 Philox items, two steps each (rng_kernels.h: noise_items)
    const long per_block = (long)(noise_cvar_threads(h.num_grid_samples) / 64) * 4;
    c.extra_blocks = (int)std::min(2L * h.num_cus, (long)update_ceil_div(rows, per_block));
  }
  c.side_stream_pays = side_stream_pays(h.n_local, h.T, h.num_cus);
  // The generator on the second stream must not start before the previous update -- the last reader of the buffer it
  // overwrites -- is complete.  A rollout launch that signals its own start provides that without anything in front of it
  // on this stream; the event recorded there held the launch back by ~6 us.
  // (Kept as it is: the event is left out when the PREVIOUS iteration's launch signalled, not when the coming one will --
  //  it is made up for behind the launch, one iteration without overlap, should this one not -- and it is recorded
  //  whenever the second stream would pay, also in front of a launch that appends the blocks itself.)
  c.record_front = want_next && c.side_stream_pays && (!h.prev_signalled || h.graph_on);
  c.signals = h.launch == kLaunchFused && noise_launch_signals(h.flag_words, h.flags_env_off, h.graph_on, h.stream_flags_off);
  c.beside_rollout = want_next && !c.extra_blocks && c.side_stream_pays;
  c.have_after_rollout = c.extra_blocks > 0 || c.beside_rollout;
  if (c.beside_rollout) {
    c.hold = c.record_front ? kHoldEventFront : (c.signals ? kHoldGate : kHoldEventBehind);
    // (kept as it is: the generator announces itself whatever MPPI_NO_NOISE_FLAG and stream_flags_off say of the consumer)
    if (h.flag_words && !h.graph_on) c.announce = h.debug_flags & MPPI_DEBUG_DROP_NOISE_FLAG ? kAnnounceDropped : kAnnounceFlag;
    c.join = h.graph_on;
  }
  // Where the rollout fills the SIMDs by itself the generator runs beside the update launch, gated on its start.
  // (Kept as it is: the test hook that drops the flag does not reach this generator.)
  c.beside_update = want_next && !c.have_after_rollout && !c.side_stream_pays && h.update_can_host;
  if (c.beside_update) {
    c.hold = kHoldGate;
    c.announce = kAnnounceFlag;
  }
  c.have_noise = c.have_after_rollout || c.beside_update;
  return c;
}
