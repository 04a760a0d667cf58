// guide_grid.h -- the guide round the walls (mppi_planner_set_guide): the arithmetic of the grid, the blocked cells, the
// neighbour choice and the row choice that k_guide_field and k_guide_rows (guide_kernels.h) call.  Plain C++ without a HIP
// type: a host program compiles it on its own (tests/test_guide_model.py holds it to the numpy model bit for bit).
//
//   centre    cx = double(x_min) + (double(ix) + 0.5) * double(res)                     the product rounded, then the sum
//   cell_of   clamp(floor((double(x) - double(x_min)) / double(res)), 0, n - 1)        the double clamped, then converted
//   blocked   near(centre - A; d, d.d, hh) for some wall A -> B of half-width h: d = B - A and d.d as the crowd kernel's
//             load_wall forms them, hh = (double(h) + double(inflate))^2, near the crowd kernel's crowd_near
//   field     uint32 per cell: kGuideBlocked, kGuideUnreached, or the length of the shortest path to the goal cell over
//             free cells, 12 a straight move and 17 a diagonal one
//   next      the in-grid neighbour with D < kGuideUnreached that minimises D[n] + w, in the order
//             (1,0) (0,1) (-1,0) (0,-1) (1,1) (-1,1) (-1,-1) (1,-1); the first minimum wins
//   units     floor(double(m) / double(res) * 12.0), on the host
// Every value is a double formed from widened float32 inputs in the order written, and no product is ever fused into a
// sum: the field and the rows are integers or once-rounded doubles, so the bits are the specification.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MPPI_GUIDE_HD __host__ __device__
#else
#define MPPI_GUIDE_HD
#endif

namespace mppi {

constexpr int kGuideCellsMax = 36864;  // 192 x 192: a problem's uint32 field, 147456 bytes, fits one workgroup's LDS
constexpr uint32_t kGuideBlocked = 0xFFFFFFFFu, kGuideUnreached = 0xFFFFFFFEu;
constexpr int kGuideNoMove = 255;  // guide_next: no admissible neighbour
constexpr int kGuideStatusOk = 0, kGuideStatusGoalBlocked = 1, kGuideStatusNoWayOut = 2;

// a rounded product that no compiler contracts with the sum it goes into
MPPI_GUIDE_HD inline double guide_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  volatile double product = a * b;  // (it lands in memory before it is used, whatever the compiler's flags)
  return product;
#endif
}

MPPI_GUIDE_HD inline double guide_centre(float lo, float res, int i) { return (double)lo + guide_mul((double)i + 0.5, (double)res); }

// a point outside the grid belongs to the nearest border cell
MPPI_GUIDE_HD inline int guide_cell_of(float x, float lo, float res, int n) {
  double q = floor(((double)x - (double)lo) / (double)res);
  q = !(q >= 0.0) ? 0.0 : q;  // (a NaN fails the comparison: cell 0, never a conversion of what is no number)
  q = q > (double)(n - 1) ? (double)(n - 1) : q;
  return (int)q;
}

// the constants of a wall as a cell's test takes them (the kernel stages them in LDS, 64 walls at a time)
struct GuideWall {
  double ax, ay, dx, dy, LL, hh;
};
MPPI_GUIDE_HD inline GuideWall guide_wall(float ax, float ay, float bx, float by, float h, float inflate) {
  GuideWall w;
  w.ax = (double)ax;
  w.ay = (double)ay;
  w.dx = (double)bx - (double)ax;
  w.dy = (double)by - (double)ay;
  w.LL = guide_mul(w.dx, w.dx) + guide_mul(w.dy, w.dy);
  const double H = (double)h + (double)inflate;
  w.hh = guide_mul(H, H);
  return w;
}

// crowd_near (rollout_crowd_kernel.h), operation for operation: is X = U + (wx, wy) within sqrt(hh) of the segment U -> U + dU?
MPPI_GUIDE_HD inline bool guide_near(double wx, double wy, double ux, double uy, double LL, double hh) {
  const double s = guide_mul(wx, ux) + guide_mul(wy, uy);
  if (s <= 0.0) return guide_mul(wx, wx) + guide_mul(wy, wy) <= hh;
  if (s >= LL) {
    const double vx = wx - ux, vy = wy - uy;
    return guide_mul(vx, vx) + guide_mul(vy, vy) <= hh;
  }
  const double c = guide_mul(wx, uy) - guide_mul(wy, ux);
  return guide_mul(c, c) <= guide_mul(hh, LL);
}

MPPI_GUIDE_HD inline bool guide_blocked(double cx, double cy, const GuideWall& w) {
  return guide_near(cx - w.ax, cy - w.ay, w.dx, w.dy, w.LL, w.hh);
}

// the eight moves in their order: (dx + 1) and (dy + 1) of move k, two bits each
MPPI_GUIDE_HD inline int guide_dx(int k) { return (int)((0x8246u >> (2 * k)) & 3u) - 1; }
MPPI_GUIDE_HD inline int guide_dy(int k) { return (int)((0x0A19u >> (2 * k)) & 3u) - 1; }
MPPI_GUIDE_HD inline uint32_t guide_move_cost(int k) { return k < 4 ? 12u : 17u; }

// The neighbour of cell (ix, iy) a descent moves to, 0 .. 7, or kGuideNoMove; *best: its D[n] + w (kGuideUnreached without
// one).  One relaxation of the cell is min(D[c], *best).  A field value stays below 17 * kGuideCellsMax: no sum wraps.
template <typename Field>
MPPI_GUIDE_HD inline int guide_next(const Field* D, int nx, int ny, int ix, int iy, uint32_t* best) {
  uint32_t least = kGuideUnreached;
  int move = kGuideNoMove;
  for (int k = 0; k < 8; ++k) {
    const int jx = ix + guide_dx(k), jy = iy + guide_dy(k);
    if (jx < 0 || jx >= nx || jy < 0 || jy >= ny) continue;
    const uint32_t v = D[jy * nx + jx];
    if (v >= kGuideUnreached) continue;
    const uint32_t cand = v + guide_move_cost(k);
    if (cand < least) {
      least = cand;
      move = k;
    }
  }
  *best = least;
  return move;
}

// floor(m / res * 12): a length in the field's units (host; the caller checks the range before it converts)
inline double guide_units(float m, float res) { return floor((double)m / (double)res * 12.0); }

// The row choice over R[0 .. n), the remaining lengths of a stretch of the descent (non-increasing): the first i with
// R0 - R[i] >= a, or n.
template <typename Remaining>
MPPI_GUIDE_HD inline int guide_first_reach(const Remaining* R, int n, uint32_t R0, long long a) {
  int lo = 0, hi = n;  // (the answer lies in [lo, hi])
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)(R0 - (uint32_t)R[mid]) >= a) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

}  // namespace mppi
