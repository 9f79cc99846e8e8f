// glibc_logf.h -- logf bit-compatible with glibc >= 2.28, usable in device code.
//
// Why: Frame::isInFrustum predicts the pyramid level with MapPoint::PredictScale (reference
// src/MapPoint.cc:370-379), `ceil(log(ratio)/logScaleFactor)` on a float `ratio`: std::log(float) ==
// libm logf.  A MapPoint seen again from the distance it was created at has ratio == mvScaleFactors[level]
// (MapPoint::UpdateNormalAndDepth, MapPoint.cc:315-355), the quotient is then an exact integer and a
// logf that differs by one ulp moves the predicted level.  glibc's logf is not correctly rounded, so
// a device libm would disagree with it; this header restates glibc's algorithm (sysdeps/ieee754/flt-32/
// e_logf.c, e_logf_data.c -- the ARM "optimized routines" logf): x = 2^k z with z in [OFF, 2 OFF),
// a 16-entry (1/c, log c) table, log(x) = log1p(z/c - 1) + log c + k ln2 with a degree-3 polynomial,
// all in double.  The constants below are glibc's table, ln2 and polynomial coefficients
// (e_logf_data.c, as shipped in libm's read-only data), written as hex-float literals.
// tests/test_local_map.py checks the host build against the host libm (every float in [2^-4, 2^12), a
// stride-97 sweep over all positive floats, zero / subnormals / 1 / inf); tests/test_gpu_local_map.py
// checks the device build.  Plain mul/add and fused evaluation agree with glibc over every positive
// finite float, so the result does not depend on -ffp-contract.
#pragma once
#include <cstdint>

#ifndef ORBFE_HD
#if defined(__HIPCC__)
#define ORBFE_HD __host__ __device__
#else
#define ORBFE_HD
#endif
#endif

namespace orbfe {

// positive finite, zero, +inf inputs (the callers' domain: a ratio of two positive distances); a negative
// or NaN input returns NaN, as glibc's does (without raising the flag)
ORBFE_HD inline float logf_glibc(float x) {
  constexpr double kInvc[16] = {
      0x1.661ec79f8f3bep+0, 0x1.571ed4aaf883dp+0, 0x1.49539f0f010b0p+0, 0x1.3c995b0b80385p+0,
      0x1.30d190c8864a5p+0, 0x1.25e227b0b8ea0p+0, 0x1.1bb4a4a1a343fp+0, 0x1.12358f08ae5bap+0,
      0x1.0953f419900a7p+0, 0x1.0000000000000p+0, 0x1.e608cfd9a47acp-1, 0x1.ca4b31f026aa0p-1,
      0x1.b2036576afce6p-1, 0x1.9c2d163a1aa2dp-1, 0x1.886e6037841edp-1, 0x1.767dcf5534862p-1};
  constexpr double kLogc[16] = {
      -0x1.57bf7808caadep-2, -0x1.2bef0a7c06ddbp-2, -0x1.01eae7f513a67p-2, -0x1.b31d8a68224e9p-3,
      -0x1.6574f0ac07758p-3, -0x1.1aa2bc79c8100p-3, -0x1.a4e76ce8c0e5ep-4, -0x1.1973c5a611cccp-4,
      -0x1.252f438e10c1ep-5, 0x0.0p+0, 0x1.aa5aa5df25984p-5, 0x1.c5e53aa362eb4p-4,
      0x1.526e57720db08p-3, 0x1.bc2860d224770p-3, 0x1.1058bc8a07ee1p-2, 0x1.4043057b6ee09p-2};
  constexpr double kLn2 = 0x1.62e42fefa39efp-1;
  constexpr double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
  constexpr uint32_t OFF = 0x3f330000u;
  uint32_t ix = __builtin_bit_cast(uint32_t, x);
  if (ix == 0x3f800000u) return 0.f;                                    // log(1) = +0 in every rounding mode
  if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {                  // subnormal, zero, inf, nan or negative
    if (ix * 2u == 0u) return -__builtin_huge_valf();                   // log(+-0) = -inf
    if (ix == 0x7f800000u) return x;                                    // log(inf) = inf
    if ((ix & 0x80000000u) || ix * 2u >= 0xff000000u) return __builtin_nanf("");
    ix = __builtin_bit_cast(uint32_t, x * 0x1p23f);                     // subnormal: normalise
    ix -= 23u << 23;
  }
  const uint32_t tmp = ix - OFF;
  const int i = (int)((tmp >> (23 - 4)) % 16u);
  const int k = (int32_t)tmp >> 23;                                     // arithmetic shift
  const uint32_t iz = ix - (tmp & (0x1ffu << 23));
  const double invc = kInvc[i], logc = kLogc[i];
  const double z = (double)__builtin_bit_cast(float, iz);
  const double r = z * invc - 1.0;
  const double y0 = logc + (double)k * kLn2;
  const double r2 = r * r;
  double y = A1 * r + A2;
  y = A0 * r2 + y;
  y = y * r2 + (y0 + r);
  return (float)y;
}

}  // namespace orbfe
