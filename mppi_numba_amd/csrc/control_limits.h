// control_limits.h -- acceleration limits on the sampled controls: the recurrence that k_noise_limit (rng_kernels.h) walks
// over a noise block, per rollout and control component.  Plain C++ without a HIP type: a host program compiles it on its
// own (tests/test_control_limits_model.py holds it to the numpy model bit for bit).
//
//   d      = fmul_rn(float32(accel), float32(dt))                        once, on the host
//   p      = clip_f32(a, lo, hi)                                         the anchor, brought into the box
//   for t = 0 .. T-1:
//     c    = clip_f32(fadd_rn(u[t], e[t]), lo, hi)                       what the rollouts would have applied
//     p    = fminf(fmaxf(c, fsub_rn(p, d)), fadd_rn(p, d))
//     e'[t]= fsub_rn(p, u[t])
//
// All of it float32, every operation rounded once: the bits are the specification.  The set "inside the box, and no step
// changes the control by more than d, counted from the anchor" is convex and p is a point of it: the weighted mean of the
// limited sequences, which is what the update forms, is feasible whatever u was.  A component whose step is +inf is left
// as it was drawn: e' = e bit for bit.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define MPPI_LIMIT_HD __host__ __device__
#else
#define MPPI_LIMIT_HD
#endif

namespace mppi {

// a limit the recurrence takes: not NaN and > 0; +inf (the component stays as drawn) is one
MPPI_LIMIT_HD inline bool control_limit_valid(float accel) { return accel > 0.0f; }

// the largest change of a control from one step to the next
MPPI_LIMIT_HD inline float control_limit_step_size(float accel, float dt) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(accel, dt);
#else
  volatile float d = accel * dt;
  return d;
#endif
}

// a component with this step is skipped
MPPI_LIMIT_HD inline bool control_limit_binds(float d) { return d < INFINITY; }

// max(lo, min(hi, v)): device_math.h's clip_f32, which the rollouts apply
MPPI_LIMIT_HD inline float control_limit_clip(float v, float lo, float hi) { return fmaxf(lo, fminf(hi, v)); }

// c: off the chain
MPPI_LIMIT_HD inline float control_limit_target(float u, float e, float lo, float hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  return control_limit_clip(__fadd_rn(u, e), lo, hi);
#else
  volatile float sum = u + e;
  return control_limit_clip(sum, lo, hi);
#endif
}

// p: the chain
MPPI_LIMIT_HD inline float control_limit_advance(float p, float c, float d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fminf(fmaxf(c, __fsub_rn(p, d)), __fadd_rn(p, d));
#else
  volatile float below = p - d;
  volatile float above = p + d;
  return fminf(fmaxf(c, below), above);
#endif
}

// e': the effective noise
MPPI_LIMIT_HD inline float control_limit_noise(float p, float u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsub_rn(p, u);
#else
  volatile float e = p - u;
  return e;
#endif
}

// One component of one rollout, in place: e[t * stride] for t = 0 .. T-1 (the host's form of the kernel's walk).
MPPI_LIMIT_HD inline void control_limit_chain(const float* u, int u_stride, float* e, int e_stride, int T, float lo, float hi,
                                              float anchor, float d) {
  if (!control_limit_binds(d)) return;
  float p = control_limit_clip(anchor, lo, hi);
  for (int t = 0; t < T; ++t) {
    const float ut = u[(long)t * u_stride];
    p = control_limit_advance(p, control_limit_target(ut, e[(long)t * e_stride], lo, hi), d);
    e[(long)t * e_stride] = control_limit_noise(p, ut);
  }
}

}  // namespace mppi
