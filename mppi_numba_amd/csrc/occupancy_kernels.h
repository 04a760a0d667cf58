// occupancy_kernels.h -- occupancy-grid obstacles (mppi_planner_set_occupancy): the clearance field D2 of the cells, the
// exact squared Euclidean distance transform in cells (occupancy_grid.h states it; tests/occupancy_model.py is the brute
// force).  One plain launch on the planner's stream, at the head of a call that starts iterations, only when the cells, the
// shape or the geometry changed: no atomics, no flags between workgroups, every loop bounded and every index clamped.
//
// The separable form: D2[y][x] = min over rows y' of (y - y')^2 + g(y', x)^2, g the distance along row y' from column x to
// its nearest occupied cell.  The cells arrive bit-packed, [ny][words] uint64 with words = ceil(nx / 64), bit b of word w
// column 64 * w + b (bits past nx are zero): 32 KiB at the cap of 512 x 512.
//
// k_occupancy_field: a workgroup of 64 x kOccupancyBand threads owns a strip of 64 columns -- one word of every row -- and
// a band of kOccupancyBand rows of it.
//   1  g of the WHOLE strip, every row, into LDS ([ny][64] uint16, 64 KiB at the cap; kOccupancyNoCell: the row is
//      empty): a wave holds one row, so the words it reads are wave-uniform -- the strip's own word masked to either side
//      of the lane's bit, then the words to the left by count-leading-zeros and to the right by count-trailing-zeros, the
//      first non-zero one ends each search
//   2  every thread takes the column minimum of its own cell, rows outwards from its own (dy = 0, 1, ...), and stops once
//      dy * dy cannot beat the best so far: a row further out only costs more
// The workgroups of a strip repeat step 1 (ny * 64 searches of at most `words` words each, over a mask that stays in L2);
// at the cap the launch is 8 strips x 32 bands = 256 workgroups, one a CU.
#pragma once
#include <stdint.h>

#include "occupancy_grid.h"

namespace mppi {

constexpr int kOccupancyBand = 16;                 // rows a workgroup writes
constexpr unsigned kOccupancyNoCell = 0xFFFFu;     // g of a row without an occupied cell (a real g is below 512)
static_assert(kOccupancyDimMax * 64 * 2 <= 64 * 1024, "k_occupancy_field: g of a strip, [ny][64] uint16, in 64 KiB of LDS");

__device__ __forceinline__ unsigned occupancy_row_gap(const unsigned long long* __restrict__ row, int words, int w, int b) {
  const unsigned long long own = row[w];
  unsigned best = kOccupancyNoCell;
  const unsigned long long left = own & (~0ull >> (63 - b));  // the bits at and below the lane's
  if (left) {
    best = (unsigned)(b - (63 - __clzll((long long)left)));
  } else {
    for (int v = w - 1; v >= 0; --v) {
      const unsigned long long m = row[v];
      if (m) {
        best = (unsigned)((w - v) * 64 + b - (63 - __clzll((long long)m)));
        break;
      }
    }
  }
  const unsigned long long right = own & (~0ull << b);  // the bits at and above it
  if (right) {
    best = min(best, (unsigned)(__ffsll((long long)right) - 1 - b));
  } else {
    for (int v = w + 1; v < words; ++v) {
      const unsigned long long m = row[v];
      if (m) {
        best = min(best, (unsigned)((v - w) * 64 + (__ffsll((long long)m) - 1) - b));
        break;
      }
    }
  }
  return best;
}

// mask: [ny][words]; field: [ny][nx].  grid (words, ceil(ny / kOccupancyBand)), block (64, kOccupancyBand); dynamic LDS:
// ny * 64 * 2 bytes
__global__ __launch_bounds__(64 * kOccupancyBand) void k_occupancy_field(const unsigned long long* __restrict__ mask, int nx, int ny,
                                                                         int words, uint32_t* __restrict__ field) {
  extern __shared__ __attribute__((aligned(16))) unsigned short occupancy_gap_lds[];
  const int w = (int)blockIdx.x, b = (int)threadIdx.x, ty = (int)threadIdx.y;
  for (int r = ty; r < ny; r += kOccupancyBand)
    occupancy_gap_lds[r * 64 + b] = (unsigned short)occupancy_row_gap(mask + (size_t)r * (size_t)words, words, w, b);
  __syncthreads();
  const int x = w * 64 + b, y = (int)blockIdx.y * kOccupancyBand + ty;
  if (x >= nx || y >= ny) return;
  uint32_t best = kOccupancyFar;
  const int reach = max(y, ny - 1 - y);
  for (int dy = 0; dy <= reach; ++dy) {
    const uint32_t dd = (uint32_t)(dy * dy);
    if (dd >= best) break;
    const int up = y - dy, down = y + dy;
    if (up >= 0) {
      const uint32_t g = occupancy_gap_lds[up * 64 + b];
      if (g != kOccupancyNoCell) best = min(best, dd + g * g);
    }
    if (down < ny) {
      const uint32_t g = occupancy_gap_lds[down * 64 + b];
      if (g != kOccupancyNoCell) best = min(best, dd + g * g);
    }
  }
  field[(size_t)y * (size_t)nx + (size_t)x] = best;
}

}  // namespace mppi
