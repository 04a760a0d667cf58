// noise_smooth.h -- time-correlated control noise: the step and the gain of the AR(1) recurrence that k_noise_smooth
// (rng_kernels.h) walks over the white draws of k_noise.  Plain C++ without a HIP type: a host program compiles it on its
// own (tests/test_noise_smoothing_model.py holds it to the numpy model bit for bit).
//
//   g        = float32(sqrt(1 - double(beta) * double(beta)))          once, on the host
//   e[0]     = w[0]
//   e[t]     = fadd_rn(fmul_rn(beta, e[t-1]), fmul_rn(g, w[t]))         t = 1 .. T-1
//
// Two rounded products and one rounded sum, never an fma: the bits are the specification.  Step 0 is the white draw and
// the gain is sqrt(1 - beta^2), so every step keeps the standard deviation of w; the lag-k correlation is beta^k.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define MPPI_SMOOTH_HD __host__ __device__
#else
#define MPPI_SMOOTH_HD
#endif

namespace mppi {

// a coefficient the recurrence takes: finite, in [0, 1)  (a NaN fails both comparisons)
MPPI_SMOOTH_HD inline bool noise_smooth_beta_valid(float beta) { return beta >= 0.0f && beta < 1.0f; }

MPPI_SMOOTH_HD inline float noise_smooth_gain(float beta) { return (float)sqrt(1.0 - (double)beta * (double)beta); }

MPPI_SMOOTH_HD inline float noise_smooth_step(float beta, float gain, float e_prev, float w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(__fmul_rn(beta, e_prev), __fmul_rn(gain, w));
#else
  // (the products land in memory before they are added: no host compiler contracts them, whatever its flags)
  volatile float carried = beta * e_prev;
  volatile float fresh = gain * w;
  return carried + fresh;
#endif
}

}  // namespace mppi
