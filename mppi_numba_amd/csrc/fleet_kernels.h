// fleet_kernels.h -- fleet mode of a batched barebone handle (mppi_planner_set_fleet): robots that avoid each other's plans.
//
// Every problem of the batch is a robot, and the wall set of reader a is made of the OTHER robots' current plans: the
// plan of robot b is the noise-free rollout of its control sequence u[b] from its start state -- barebone_next_pose with
// e = 0, the clip included, the bits of k_state_rollout<false, true> and of oracle.state_rollout_barebone with zero noise
// -- and row j of the wall that stands for b is the segment [c_j, c_{j+1}] its centre covers during control interval j
// (barebone.swept_walls).  With half-width r_a + r_b + margin the crowd kernel's CrowdWallTracks form tests step t of a's
// rollouts against the capsule b sweeps in the same interval: crowd_wall_hit, unchanged.  The rows are counted from "now"
// (CrowdWallTracks::relative): they are rebuilt at the head of every call that starts iterations.
//
// Two plain launches on the planner's stream ahead of the iterations; no flags, no atomics, no waits between workgroups.
//
// k_fleet_plans: one wave per robot.  A robot's walk is three chains of one rounded operation per step -- the heading, x
// and y -- and a lone wave issues a dependent instruction about every 9 cycles, so the chains are kept as short as the
// arithmetic allows and everything that does not depend on them is done across the lanes:
//   1. 64 steps at a time, lane l clips step k0 + l's controls and forms dt * v and dt * w (float32 products);
//   2. the heading is walked in registers, one v_add_f32 per step on a value read from lane l's register (readlane with a
//      constant lane: the 64 steps are unrolled); lane l keeps the heading BEFORE its step;
//   3. every lane takes the full sincos_f64 of its heading (never the rotation form: no bound on |dt * w| applies) and
//      leaves (sin, cos) and dt * v in LDS;
//   4. lanes 0 and 1 walk x and y from LDS -- one instruction stream for both chains, eight steps' operands loaded
//      ahead of the eight dependent steps -- into an LDS copy of the plan, which the wave then stores coalesced.
// A parked robot (done[b] != 0: closed_loop, at its goal) stands: every row is the degenerate segment at its start state,
// which holds the float32 of its final position.
//
// k_fleet_walls: one thread per (row, reader, other).  The CrowdWallTracks layout is seg[row * pitch + wall0_a + slot], so
// within a row a reader's B - 1 fleet slots are contiguous and consecutive readers follow at a stride of `slots`; the
// threads are numbered in that order and the float4 stores of a row are contiguous but for the static walls' slots
// between the readers, which are written once when the storage is built and never here.  The plans are read from the
// [B][T + 1] scratch (B * (T + 1) * 8 bytes: cache resident).  Two launches rather than one: the scatter needs every
// robot's plan, and a single launch would either store 16 bytes at a stride of a whole reader (one robot per workgroup)
// or need a wait between workgroups.
//
// A FLEET OF BODIES (mppi_planner_set_fleet_bodies): every robot is the same F discs attached to its pose, and reader a is
// given, for every other robot b and body disc k, the segment the disc's centre covers in control interval j.
// k_fleet_plans<., true> stores the T + 1 headings it walks anyway beside the positions; k_fleet_body_centres forms the
// centres once per (robot, state) -- B * (T + 1) sine / cosine pairs, never one per reader -- in crowd_body_centres'
// arithmetic; k_fleet_body_walls scatters them into the CrowdWallTracks layout, Fp slots a robot (F rounded up to a power of
// two, the padding slots repeating the last disc).  Three plain launches; the disc fleet's two are what they were.
#pragma once
#include "rollout_crowd_kernel.h"

namespace mppi {

// dynamic LDS of k_fleet_plans: [Tp] double2 (sin, cos) | [Tp] float dt * v | [T + 1] float2 plan; Tp: T rounded up to 64
__host__ __device__ constexpr size_t fleet_plans_lds_bytes(int T) {
  return (sizeof(double2) + sizeof(float)) * (size_t)((T + 63) & ~63) + sizeof(float2) * (size_t)(T + 1);
}

constexpr int kFleetBatch = 8;  // steps whose operands lanes 0 and 1 load ahead of the dependent walk

// HEADS (a body fleet): the T + 1 float32 headings of the plan, the final one included, to heads[b][0 .. T] -- the
// heading before step t is what lane t of its block of 64 holds anyway.  Without it nothing is stored there.
template <bool EXACT, bool HEADS = false>
__global__ __launch_bounds__(64) void k_fleet_plans(DevParams P, const float2* __restrict__ u, const int* __restrict__ done,
                                                    float2* __restrict__ plans, float* __restrict__ heads = nullptr) {
  extern __shared__ double2 fleet_trig[];
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x, T = P.n_steps;
  const int Tp = (T + 63) & ~63;
  u = select_instance(P, u, b);  // (a fleet is a batched handle: P.inst is set)
  float2* out = plans + (size_t)b * (size_t)(T + 1);
  if (done != nullptr && done[b] != 0) {  // (uniform over the workgroup) parked: it stands where it arrived
    for (int t = lane; t <= T; t += 64) out[t] = make_float2(P.x0, P.y0);
    if constexpr (HEADS)  // ... as it stood: its start state holds the float32 of its final heading
      for (int t = lane; t <= T; t += 64) heads[(size_t)b * (size_t)(T + 1) + t] = P.th0;
    return;
  }
  float* dtvs = reinterpret_cast<float*>(fleet_trig + Tp);
  float2* pos = reinterpret_cast<float2*>(dtvs + Tp);
  float th = P.th0;
  for (int k0 = 0; k0 < T; k0 += 64) {
    const int t = k0 + lane;
    float dtv = 0.0f, dtw = 0.0f;
    if (t < T) {  // barebone_next_pose's controls with e = 0
      const float2 ut = u[t];
      const float v = clip_f32(ut.x + 0.0f, P.v_lo, P.v_hi);
      const float w = barebone_yaw_rate(P, v, clip_f32(ut.y + 0.0f, P.w_lo, P.w_hi));
      dtv = P.dt * v;
      dtw = P.dt * w;
    }
    float mine = th;  // the heading before step k0 + lane
#pragma unroll
    for (int l = 0; l < 64; ++l) {
      mine = l == lane ? th : mine;
      th = th + crowd_lane_f32(dtw, l);  // nth = th + P.dt * w (steps past the horizon add 0 behind the last one used)
    }
    if (EXACT) {
      double sn, cs;
      sincos_f64<false>((double)mine, sn, cs);
      fleet_trig[t] = make_double2(sn, cs);
    } else {
      float sn, cs;
      sincosf(mine, &sn, &cs);
      fleet_trig[t] = make_double2((double)sn, (double)cs);  // (exact both ways)
    }
    dtvs[t] = dtv;
    if constexpr (HEADS)
      if (t < T) heads[(size_t)b * (size_t)(T + 1) + t] = mine;
  }
  if constexpr (HEADS)  // (steps past the horizon added 0: th is the heading after step T - 1)
    if (lane == 0) heads[(size_t)b * (size_t)(T + 1) + T] = th;
  __syncthreads();
  if (lane < 2) {  // lane 0: x with the cosines, lane 1: y with the sines
    const double* tr = reinterpret_cast<const double*>(fleet_trig) + (1 - lane);
    float* o = reinterpret_cast<float*>(pos) + lane;
    float c = lane == 0 ? P.x0 : P.y0;
    o[0] = c;
    for (int t0 = 0; t0 < T; t0 += kFleetBatch) {
      double f[kFleetBatch];
      float dv[kFleetBatch], r[kFleetBatch];
#pragma unroll
      for (int j = 0; j < kFleetBatch; ++j) {
        const int t = min(t0 + j, T - 1);
        f[j] = tr[2 * t];
        dv[j] = dtvs[t];
      }
#pragma unroll
      for (int j = 0; j < kFleetBatch; ++j) {  // nx = (float)fma((double)dtv, cs, (double)x); fast math: fmaf(dtv, cs, x)
        if (EXACT) c = (float)fma((double)dv[j], f[j], (double)c);
        else c = fmaf(dv[j], (float)f[j], c);
        r[j] = c;
      }
#pragma unroll
      for (int j = 0; j < kFleetBatch; ++j)
        if (t0 + j < T) o[2 * (t0 + j + 1)] = r[j];
    }
  }
  __syncthreads();
  for (int t = lane; t <= T; t += 64) out[t] = pos[t];
}

// grid (ceil(B * (B - 1) / 256), T), block 256.  slots: wall slots per reader (B - 1 + the static walls).
__global__ __launch_bounds__(256) void k_fleet_walls(const float2* __restrict__ plans, float4* __restrict__ seg, int B, int T,
                                                     int slots) {
  const int j = (int)blockIdx.y;                             // the row: control interval j from "now"
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;    // reader * (B - 1) + slot
  if (i >= B * (B - 1) || j >= T) return;
  const int a = i / (B - 1), slot = i - a * (B - 1);
  const int b = slot + (slot >= a ? 1 : 0);  // the others in ascending order, skipping the reader
  const float2* c = plans + (size_t)b * (size_t)(T + 1) + j;
  const float2 c0 = c[0], c1 = c[1];
  seg[(size_t)j * ((size_t)B * (size_t)slots) + (size_t)a * (size_t)slots + (size_t)slot] = make_float4(c0.x, c0.y, c1.x, c1.y);
}

// ---- a body fleet (mppi_planner_set_fleet_bodies): every robot is F discs attached to its pose -------------------------
// k_fleet_body_centres: one thread per (robot, state) -- B * (T + 1) sine / cosine pairs, never one per reader.  The centres
// of the F body discs at state j of robot b's plan, in crowd_body_centres' arithmetic (the full sincos_f64<false> of the
// float32 heading whatever the math mode is, products and sums in double in its order, one rounding): the bits the crowd
// kernel forms for a rollout in that state.  centres: [B][T + 1][F] float2.  The rows come by value (CrowdFootprint).
__global__ __launch_bounds__(256) void k_fleet_body_centres(const float2* __restrict__ plans, const float* __restrict__ heads,
                                                            float2* __restrict__ centres, int states, CrowdFootprint fp) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;  // robot * (T + 1) + state
  if (i >= states) return;
  const float2 c = plans[i];
  float cx[kCrowdFootprintMax], cy[kCrowdFootprintMax];
  double sn, cs;
  crowd_body_centres(fp, c.x, c.y, heads[i], cx, cy, sn, cs);
  float2* out = centres + (size_t)i * (size_t)fp.count;
#pragma unroll
  for (int k = 0; k < kCrowdFootprintMax; ++k)
    if (k < fp.count) out[k] = make_float2(cx[k], cy[k]);
}

// k_fleet_body_walls: one thread per (row, reader, slot), numbered like k_fleet_walls' so that a row's stores stay
// contiguous.  A reader's fleet slots: (B - 1) * Fp, the other robot `o` (ascending, the reader skipped) at o * Fp, its
// body disc k at o * Fp + k; Fp is F rounded up to a power of two, and the padding slots F <= k < Fp repeat disc F - 1
// (a duplicate cannot change the OR over a robot's slots).  grid (ceil(B * (B - 1) * Fp / 256), T), block 256.
__global__ __launch_bounds__(256) void k_fleet_body_walls(const float2* __restrict__ centres, float4* __restrict__ seg, int B, int T,
                                                          int slots, int F, int Fp) {
  const int j = (int)blockIdx.y;
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;  // reader * (B - 1) * Fp + slot
  const int per = (B - 1) * Fp;
  if (i >= B * per || j >= T) return;
  const int a = i / per, slot = i - a * per;
  const int o = slot / Fp, k = min(slot - o * Fp, F - 1);
  const int b = o + (o >= a ? 1 : 0);
  const float2* c = centres + ((size_t)b * (size_t)(T + 1) + (size_t)j) * (size_t)F + k;
  const float2 c0 = c[0], c1 = c[F];
  seg[(size_t)j * ((size_t)B * (size_t)slots) + (size_t)a * (size_t)slots + (size_t)slot] = make_float4(c0.x, c0.y, c1.x, c1.y);
}

}  // namespace mppi
