// The steps of a constant-twist rollout (validate_control, numerics.hpp:273-330; the dynamic window's samples,
// dynamic_window.cpp:92-286), written ONCE for collision_kernel.hip and footprint_plan_kernel.hip.  Both are compiled without FMA
// contraction and the sums keep the reference's order and parentheses, so every caller gets the same bits.
#pragma once

#include "common.hpp"

namespace eea
{
namespace
{
// Round 6: the constant-twist rollouts of validate_control / the dynamic window are instruction-issue bound (20 dependent steps
// per lane of sincos + normalize_angle_PI + a byte lookup: ~245 instructions per step with the device library's sincos and the
// literal wrap, whose quotient is an fp64 DIVISION).  EEA_TICK_FAST_TRIG (default): sin / cos by the engine's own sincospi_r
// (exact reduction, max error 1.9e-16: common.hpp) of theta / pi, and the wrap's quotient by a multiplication with 1 / (2 pi) --
// a quotient that lands on the other side of an integer is repaired by the wrap's own range fixes, everything else is bitwise
// the literal form.  The outputs the reference pins are integer decisions (collision verdicts, the chosen sample), which
// tests/test_gpu_collision_parity.py / test_gpu_dwa_parity.py / test_gpu_fleet_tick.py check bit for bit against the oracle.
#ifndef EEA_TICK_FAST_TRIG
#define EEA_TICK_FAST_TRIG 1
#endif
__device__ __forceinline__ double wrap_pi_d(double rad)
{
#if EEA_TICK_FAST_TRIG
  const double pi = kPi, two_pi = 2.0 * kPi;
  const double q = floor((rad + pi) * (1.0 / (2.0 * kPi)));
  rad = (rad + pi) - q * two_pi;
  if (rad < 0.0) rad += two_pi;
  if (!(rad < two_pi)) rad -= two_pi;
  return rad - pi;
#else
  return wrap_pi<double>(rad);
#endif
}
__device__ __forceinline__ void tick_sincos(double th, double* s, double* c)
{
#if EEA_TICK_FAST_TRIG
  sincospi_r<double>(th * (1.0 / kPi), s, c);
#else
  sincos(th, s, c);
#endif
}

// FAST: sin / cos by tick_sincos (the rollouts), otherwise by the device library (integrate_twist_kernel).

// body-frame displacement of one step of the twist (u0, u1, u2) (numerics.hpp:273-297): the same every step
template <bool FAST>
__device__ __forceinline__ void body_displacement(double u0, double u1, double u2, double dt, double& d0, double& d1, double& d2)
{
  if (fabs(u2 - 0.0) < 1.0e-12) {
    d0 = u0 * dt;
    d1 = u1 * dt;
    d2 = 0.0;
  } else {
    const double vb0 = u0 * dt, vb1 = u1 * dt, vb2 = u2 * dt;
    double s, cc;
    if constexpr (FAST) tick_sincos(vb2, &s, &cc);
    else sincos(vb2, &s, &cc);
    d0 = (vb0 * s + vb1 * (cc - 1.0)) / vb2;
    d1 = (vb1 * s + vb0 * (1.0 - cc)) / vb2;
    d2 = vb2;
  }
}

// x + Rot(theta) d; the heading wrapped to [-pi, pi) (validate_control, numerics.hpp:325) or left as it is
template <bool FAST>
__device__ __forceinline__ void advance_pose(double& x, double& y, double& th, double d0, double d1, double d2, bool wrap)
{
  double s, cc;
  if constexpr (FAST) tick_sincos(th, &s, &cc);
  else sincos(th, &s, &cc);
  x = x + (cc * d0 + (-s) * d1);
  y = y + (s * d0 + cc * d1);
  th = wrap ? wrap_pi_d(th + d2) : th + d2;
}

// velocity sample sidx = (i, j, k) in the reference's loop order; values by repeated += like the reference
__device__ __forceinline__ void sample_twist(const DwaParams& d, const double (&lower)[3], const double (&delta)[3], unsigned sidx,
                                             double& u0, double& u1, double& u2)
{
  const unsigned k = sidx % d.ns[2], j = (sidx / d.ns[2]) % d.ns[1], i = sidx / (d.ns[2] * d.ns[1]);
  u0 = lower[0];
  u1 = lower[1];
  u2 = lower[2];
  for (unsigned q = 0; q < i; ++q) u0 += delta[0];
  for (unsigned q = 0; q < j; ++q) u1 += delta[1];
  for (unsigned q = 0; q < k; ++q) u2 += delta[2];
}
}  // namespace
}  // namespace eea
