// Per-pixel arithmetic of the Lab chroma loss (csrc/lab_loss.hip): sRGB -> linear -> XYZ (D65) -> Lab -> normalize_lab, and the
// derivative of the two chroma channels wrt the colour.  The rule is restated from reference layers/lab_loss.py:13-48 and from
// kornia.color.rgb_to_lab as published; tests/lab_ref.py holds the same rule in numpy fp64.
// Inputs and outputs are fp32; the chain between them runs in fp64 registers and is rounded ONCE, so every value the kernels write
// is the fp32 rounding of the rule's exact value up to ~1e-12 relative -- whatever an fp32 evaluation order would give lies within
// that evaluation's own rounding error of it.  x^2.4 and the cube root are exp(e log x) with the two short series below (positive
// finite arguments only: the callers pass 1 where the other branch of a threshold is selected).
// Host-compilable: the same functions are checked against the numpy restatement on the CPU (tests/test_lab_cpu.py).
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#define TP_LAB_FN __host__ __device__ __forceinline__
#else
#define TP_LAB_FN inline
#endif

namespace tp_lab {

// log x for finite x > 0: x = m 2^e with m in [sqrt(1/2), sqrt 2), log m = 2 atanh s, s = (m - 1) / (m + 1), |s| <= 0.1716;
// the series is cut after s^12 / 13 (next term < 1.4e-12 relative)
TP_LAB_FN double log_pos(double x) {
  int e;
  double m = frexp(x, &e);
  if (m < 0.70710678118654752) { m *= 2.0; e -= 1; }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double p = 1.0 / 13.0;
  p = fma(p, z, 1.0 / 11.0);
  p = fma(p, z, 1.0 / 9.0);
  p = fma(p, z, 1.0 / 7.0);
  p = fma(p, z, 1.0 / 5.0);
  p = fma(p, z, 1.0 / 3.0);
  p = fma(p, z, 1.0);
  return fma((double)e, 0.69314718055994531, 2.0 * s * p);
}

// exp y for |y| of a few tens: y = k ln 2 + r, |r| <= ln 2 / 2, Taylor series to r^10 / 10! (remainder < 2.3e-13 relative)
TP_LAB_FN double exp_small(double y) {
  const double k = rint(y * 1.4426950408889634);
  double r = fma(-k, 0.69314718036912382, y);
  r = fma(-k, 1.9082149292705877e-10, r);
  double p = 1.0 / 3628800.0;
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)k);
}

constexpr double kSrgbThreshold = 0.04045, kLabThreshold = 0.008856;
constexpr double kWhiteX = 0.95047, kWhiteZ = 1.08883;       // (Y: 1)

// normalised Lab of one colour: lab = (L / 100, (a + 127) / 254, (b + 127) / 254).
// GRAD: also dlin[c] = d linear_c / d colour_c and df[k] = d f(t_k) / d t_k of the SELECTED branches (what torch.where passes on).
template <bool GRAD>
TP_LAB_FN void rgb_to_lab_norm(const float (&rgb)[3], double (&lab)[3], double (&dlin)[3], double (&df)[3]) {
  double lin[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v = (double)rgb[c];
    const bool gamma = v > kSrgbThreshold;                   // (NaN: the linear branch, which passes it on)
    const double lg = log_pos(gamma ? (v + 0.055) / 1.055 : 1.0);
    lin[c] = gamma ? exp_small(2.4 * lg) : v / 12.92;
    if (GRAD) dlin[c] = gamma ? (2.4 / 1.055) * exp_small(1.4 * lg) : 1.0 / 12.92;
  }
  const double t[3] = {fma(0.412453, lin[0], fma(0.357580, lin[1], 0.180423 * lin[2])) / kWhiteX,
                       fma(0.212671, lin[0], fma(0.715160, lin[1], 0.072169 * lin[2])),
                       fma(0.019334, lin[0], fma(0.119193, lin[1], 0.950227 * lin[2])) / kWhiteZ};
  double f[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const bool root = t[k] > kLabThreshold;
    const double tk = root ? t[k] : 1.0;
    const double cb = exp_small(log_pos(tk) * (1.0 / 3.0));
    f[k] = root ? cb : fma(7.787, t[k], 4.0 / 29.0);
    if (GRAD) df[k] = root ? cb / (3.0 * tk) : 7.787;
  }
  lab[0] = (116.0 * f[1] - 16.0) / 100.0;
  lab[1] = (500.0 * (f[0] - f[1]) + 127.0) / 254.0;
  lab[2] = (200.0 * (f[1] - f[2]) + 127.0) / 254.0;
}

// SmoothL1 (beta = 1) of d and its derivative
TP_LAB_FN double smooth_l1(double d) { const double a = fabs(d); return a < 1.0 ? 0.5 * d * d : a - 0.5; }
TP_LAB_FN double smooth_l1_grad(double d) { return fabs(d) >= 1.0 ? (d > 0.0 ? 1.0 : -1.0) : d; }      // (NaN stays NaN)

// d / d colour of ga * a_n + gb * b_n (the two normalised chroma channels), from the factors rgb_to_lab_norm<true> returned
TP_LAB_FN void chroma_grad(double ga, double gb, const double (&dlin)[3], const double (&df)[3], double (&g)[3]) {
  const double gfa = ga * (500.0 / 254.0), gfb = gb * (200.0 / 254.0);
  const double gx = gfa * df[0] / kWhiteX, gy = (gfb - gfa) * df[1], gz = -gfb * df[2] / kWhiteZ;
  g[0] = fma(0.412453, gx, fma(0.212671, gy, 0.019334 * gz)) * dlin[0];
  g[1] = fma(0.357580, gx, fma(0.715160, gy, 0.119193 * gz)) * dlin[1];
  g[2] = fma(0.180423, gx, fma(0.072169, gy, 0.950227 * gz)) * dlin[2];
}

}  // namespace tp_lab
