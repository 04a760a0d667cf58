// lds_layouts.h -- how many bytes of LDS the rollout kernels' workgroups lay out, and the limits that size them.
// Plain C++ without a HIP type: the kernel headers include it (and keep the layouts' meaning: which array lives where),
// and so does map_plan.h, which a host program compiles on its own (tests/test_map_plan.py works the sizes out again).
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define MPPI_HD __host__ __device__
#else
#define MPPI_HD
#endif

namespace mppi {

// update_kernels.h: the ranks whose packets one rollout launch can combine (PendingApply, PeerExchange)
constexpr int kMaxFoldedRanks = 16;

// k_rollout_pipe (rollout_kernels.h): wave triples per workgroup, i.e. its launch bounds
constexpr int kPipeMaxTriples = 2;

// PipeRing<C>::kBytesPerPair (rollout_kernels.h): xy[2][C][64] float2 + qd[2][C][64] double2 + cell[2][C][64] uint16
MPPI_HD constexpr int pipe_ring_bytes(int C) { return 2 * C * 64 * (8 + 16 + 2); }

// k_rollout_scan (rollout_scan_kernel.h): a workgroup of W waves over R rollouts
template <int R>
struct ScanLds {
  static constexpr int S = 64 / R;     // lanes per rollout in a wave
  static constexpr int CHL = 8 / S;    // steps per lane
  // per workgroup of W waves (K = W * S chunks of CHL steps, Tp = 8 W steps)
  MPPI_HD static constexpr size_t rec(int W) { return (size_t)W * 64 * CHL * 8; }   // {sg, pen}[CHL] per (chunk, rollout)
  MPPI_HD static constexpr size_t ccr(int W) { return (size_t)W * 64 * CHL * 4; }   // cc[CHL]
  MPPI_HD static constexpr size_t e2(int W) { return (size_t)W * 8 * R * 8; }       // noise [Tp][R] float2
  // + (a sharded iteration's update applied in this launch: update_kernels.h, PendingApply) the ranks'
  //   scales and the updated controls [Tp] float2
  MPPI_HD static constexpr size_t small(int W) {
    return (size_t)R * (16 + 8 + 8 + 4) + 64 + 8 * (kMaxFoldedRanks + 2) + (size_t)W * 64;
  }
  MPPI_HD static constexpr size_t total(int W) { return rec(W) + ccr(W) + e2(W) + small(W); }
  // the three float64 sums of phases A-C, [3][K][R], live where the records of phase D' go
  static_assert(3 * 8 <= CHL * 8, "sums alias the records");
};

// k_rollout_scan_exact (rollout_scan_exact_kernel.h, where the arrays are described): W chunk waves over R = 32 rollouts
struct ScanExactLds {
  static constexpr int R = 32, CHL = 4, kMaxChunkWaves = 13;
  // the waves a workgroup needs for W groups (walkers: waves 0, 4, 1; chunk waves: kGroupOfWave in the kernel)
  MPPI_HD static constexpr int waves(int W) {
    constexpr int need[kMaxChunkWaves] = {6, 6, 6, 10, 10, 10, 14, 14, 14, 15, 16, 16, 16};  // 1 + the highest wave among groups 0 .. W-1 and the walkers
    return need[W - 1];
  }
  MPPI_HD static constexpr size_t plane(int W) { return (size_t)W * 8 * R * 8; }
  MPPI_HD static constexpr size_t e2(int W) { return plane(W); }
  MPPI_HD static constexpr size_t ccr(int W) { return plane(W); }
  MPPI_HD static constexpr size_t grp(int W) { return 2 * plane(W); }
  MPPI_HD static constexpr size_t p2(int W) { return (size_t)(W * 8 + 1) * R * 8; }
  MPPI_HD static constexpr size_t small(int W) {
    return (size_t)W * 8 * (16 + 8) + R * 64 + 64 + 8 * (kMaxFoldedRanks + 2) + 8 * 16 * 4 + (size_t)2 * W * R * 16;
  }
  MPPI_HD static constexpr size_t total(int W) { return e2(W) + ccr(W) + grp(W) + p2(W) + small(W); }
};

// ... where it re-executes a tile on the exact schedule (ScanFallback): [Tp] float2 controls | window | one chunk ring
struct ScanFallbackLds {
  static constexpr int kRingBytes = pipe_ring_bytes(8);
  MPPI_HD static constexpr size_t bytes(int Tp, int map_bytes) { return (size_t)Tp * 8 + (size_t)map_bytes + kRingBytes; }
};

}  // namespace mppi
