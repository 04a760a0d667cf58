// occupancy_grid.h -- occupancy-grid obstacles (mppi_planner_set_occupancy): the arithmetic of the test points, the inside
// rule and the thresholds that the crowd kernel (rollout_crowd_kernel.h), k_guide_field (guide_kernels.h) and the hand-over
// call.  Plain C++ without a HIP type: a host program compiles it on its own (tests/test_occupancy_model.py holds it to the
// numpy model bit for bit).
//
//   field      D2[iy][ix], uint32: the least (ix - jx)^2 + (iy - jy)^2 over the occupied cells (jy, jx); 0 on an occupied
//              cell, kOccupancyFar everywhere when none is occupied (occupancy_kernels.h builds it)
//   point      test point k = 1 .. M of the chord A -> B (the float32 centres of a body disc before and after the step):
//              k == M: double(B); else double(A) + mul(double(k) / double(M), double(B) - double(A)), the product rounded
//   inside     q = floor((X - double(origin)) / double(res)) per axis; inside iff q >= 0 && q <= n - 1 on both (a NaN fails
//              the test); a point outside is free: no hit, and near at no ring
//   threshold  thr = min(floor(mul(R, R) / mul(res, res)), 0xFFFFFFFE) as uint32, R = (double(inflate) + rho) + m
//   verdict    inside && D2[cell] <= thr: one integer comparison
// Every value is a double formed from widened float32 inputs in the order written, and no product is ever fused into a
// sum (guide_mul): the bits are the specification.
#pragma once

#include <math.h>
#include <stdint.h>

#include "guide_grid.h"

namespace mppi {

constexpr int kOccupancyDimMax = 512;            // cells per axis at the most
constexpr int kOccupancySubstepsMax = 8;         // test points per chord at the most
constexpr uint32_t kOccupancyFar = 0xFFFFFFFFu;  // the field where no cell is occupied
constexpr uint32_t kOccupancyThrMax = 0xFFFFFFFEu;

// test point k of M on the chord a -> b, one axis
MPPI_GUIDE_HD inline double occupancy_point(float a, float b, int k, int M) {
  if (k == M) return (double)b;
  const double f = (double)k / (double)M;
  return (double)a + guide_mul(f, (double)b - (double)a);
}

// the cell of X along one axis of n cells: false outside the grid (and for a NaN), *cell untouched then
MPPI_GUIDE_HD inline bool occupancy_cell(double X, float lo, float res, int n, int* cell) {
  const double q = floor((X - (double)lo) / (double)res);
  if (!(q >= 0.0 && q <= (double)(n - 1))) return false;
  *cell = (int)q;
  return true;
}

// the threshold of a body disc of radius rho at margin m (0: the hit), in squared cells
MPPI_GUIDE_HD inline uint32_t occupancy_threshold(float inflate, double rho, double margin, float res) {
  const double R = ((double)inflate + rho) + margin;
  const double v = floor(guide_mul(R, R) / guide_mul((double)res, (double)res));
  return !(v < (double)kOccupancyThrMax) ? kOccupancyThrMax : (uint32_t)v;  // (an overflow to +inf included)
}

}  // namespace mppi
