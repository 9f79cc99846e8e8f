// equidistant_tan.h -- Frame::antidistorsionarProyeccionEquidistante (reference src/Frame.cc:355-384) with a certified rounding,
// usable in host and device code.
//
// Why: the reference computes `tan(theta_d)` with the host libm's double tan, which is not correctly rounded (glibc documents an
// error below 1 ULP) and cannot be restated bit for bit.  The function's RESULT is a float, though: the choice between two adjacent
// doubles for tan(theta_d) moves that float only when a float rounding boundary falls between the two projected values -- measured
// 3.6e-8 per coordinate, 7.3e-8 per point (DESIGN_NOTES.md).  So this header
//   1. encloses the real tan(theta) in double-double arithmetic with a proved error bound (tan_enclosure),
//   2. lists every double a libm whose tan errs by LESS THAN 1 ULP could return (tan_candidates),
//   3. runs the rest of the reference arithmetic, exactly as orbfe_undistort_equidistant states it, once per candidate, and
//   4. reports the point as DECIDED when all candidates give the same two floats, else as UNDECIDED with the LOWEST candidate's
//      floats: the caller then asks the host's own std::tan (orbfe_undistort_equidistant).
// A decided result equals the reference's on any host libm whose tan errs by less than 1 ULP.
//
// Arithmetic rules: IEEE double +, -, *, /, sqrt (all correctly rounded) and explicit fma, which is exact on both sides; no
// contraction (-ffp-contract=off in the build, repeated by the pragmas below), no libm call, no table.
//
// ---- tan_enclosure: algorithm and error bound (u = 2^-53) ---------------------------------------------------------------------
// Domain: 1e-8 < theta <= kThetaMax = 1.5 (cos(1.5) = 0.0707: far from the pole; an equidistant lens reaches theta = pi / 2 only
// at a 180-degree field of view).  No argument reduction, so there is no internal breakpoint:
//   x2 = theta * theta           exactly, as a double-double (TwoProd)
//   S  = sum_{k<15} (-1)^k x2^k / (2k+1)!   (= sin(theta) / theta),   C = sum_{k<16} (-1)^k x2^k / (2k)!   (= cos(theta))
//        by Horner's rule in double-double; the coefficients are 1 / n! rounded to double-double (relative error <= u^2),
//        generated with mpmath (tools/find_equidistant_undecided.py --coefficients prints them)
//   T  = (theta * S) / C
// Building blocks and their published relative error bounds (Joldes, Muller, Popescu, "Tight and rigorous error bounds for basic
// building blocks of double-word arithmetic", ACM TOMS 44(2), 2017; all need only the absence of under/overflow, which the domain
// gives: the smallest quantity formed is a low word near 2^-162):
//   dd_add  AccurateDWPlusDW (alg. 6)   <= 3 u^2 + 13 u^3  of the exact sum, cancellation included
//   dd_mul  DWTimesDW with fma (alg. 12) <= 5 u^2
//   dd_mul_d DWTimesFP with fma (alg. 9) <= 2 u^2
//   dd_div  DWDivDW (alg. 17)           <= 15 u^2 + 56 u^3
// Horner: one step computes c_k + x2 * p with relative errors (5 u^2 on the product, 3.1 u^2 on the sum); the classic running error
// bound of Horner's rule gives an ABSOLUTE error of at most 8.1 u^2 * sum_k (2k+1) |c_k| x2^k (1 + O(u^2)), i.e.
//   for C: 8.1 u^2 (cosh(theta) + theta sinh(theta)) <= 8.1 u^2 * 5.55 <  45 u^2       (theta <= 1.5)
//   for S: 8.1 u^2 cosh(theta)                       <= 8.1 u^2 * 2.36 <  20 u^2
// coefficient rounding adds at most u^2 * cosh(1.5) < 2.4 u^2 to either; truncation adds 1.5^32 / 32! < 2^-99 to C and
// 1.5^30 / 31! < 2^-95 to S (alternating series with decreasing terms: the remainder is below the first omitted term).
// Relative to C >= cos(1.5) > 0.0707 and S >= sin(1.5) / 1.5 > 0.66:
//   C: (45 + 2.4) u^2 / 0.0707 + 2^-99 / 0.0707 < 671 u^2 + 2^-95.1 < 2^-94
//   S: (20 + 2.4) u^2 / 0.66 + 2^-95 / 0.66     <  34 u^2 + 2^-94.4 < 2^-94
// theta * S adds 2 u^2, the division 15.1 u^2, and the three factors compose to less than 2^-92.9 relative error in T.
// The enclosure is T -/+ |T.hi| * 2^-80: a margin of 2^12 over the bound, and 2^18 below the 2^-62 half-width that keeps the
// straddling case (three candidates) under one input in 500.  Forming the two end points costs one more rounding of a low word each
// (<= u^2 |T|), which the margin absorbs.  tests/test_equidistant_tan.py checks containment, the half-width and the candidate set
// against mpmath at 60 digits.
#pragma once
#include <cstdint>

#ifndef ORBFE_HD
#if defined(__HIPCC__)
#define ORBFE_HD __host__ __device__
#else
#define ORBFE_HD
#endif
#endif

#if defined(__clang__)
#define ORBFE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ORBFE_NO_CONTRACT   // (g++: the build's -ffp-contract=off)
#endif

namespace orbfe {

constexpr double kThetaMax = 1.5;          // upper end of tan_enclosure's domain (inclusive)
constexpr double kThetaMin = 1e-8;         // the reference's `theta_d > 1e-8` (exclusive)
constexpr double kTanRadius = 0x1p-80;     // relative half-width of the enclosure

struct DD { double hi, lo; };   // hi + lo, |lo| <= ulp(hi) / 2

ORBFE_HD inline DD dd_two_sum(double a, double b) {
  ORBFE_NO_CONTRACT
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
ORBFE_HD inline DD dd_fast_two_sum(double a, double b) {   // |a| >= |b| or a == 0
  ORBFE_NO_CONTRACT
  const double s = a + b;
  return {s, b - (s - a)};
}
ORBFE_HD inline DD dd_two_prod(double a, double b) {
  ORBFE_NO_CONTRACT
  const double p = a * b;
  return {p, __builtin_fma(a, b, -p)};
}
ORBFE_HD inline DD dd_add(DD x, DD y) {
  ORBFE_NO_CONTRACT
  const DD s = dd_two_sum(x.hi, y.hi), t = dd_two_sum(x.lo, y.lo);
  const DD v = dd_fast_two_sum(s.hi, s.lo + t.hi);
  return dd_fast_two_sum(v.hi, t.lo + v.lo);
}
ORBFE_HD inline DD dd_mul(DD x, DD y) {
  ORBFE_NO_CONTRACT
  const DD c = dd_two_prod(x.hi, y.hi);
  const double t0 = x.lo * y.lo;
  const double t1 = __builtin_fma(x.hi, y.lo, t0);
  const double c2 = __builtin_fma(x.lo, y.hi, t1);
  return dd_fast_two_sum(c.hi, c.lo + c2);
}
ORBFE_HD inline DD dd_mul_d(DD x, double y) {
  ORBFE_NO_CONTRACT
  const DD c = dd_two_prod(x.hi, y);
  return dd_fast_two_sum(c.hi, __builtin_fma(x.lo, y, c.lo));
}
ORBFE_HD inline DD dd_div(DD x, DD y) {
  ORBFE_NO_CONTRACT
  const double th = x.hi / y.hi;
  const DD r = dd_mul_d(y, th);
  const double ph = x.hi - r.hi, dl = x.lo - r.lo;
  const double d = ph + dl;
  return dd_fast_two_sum(th, d / y.hi);
}

// [ (hi, lo_l), (hi, hi_l) ] encloses the real tan(theta); ok == false: theta is outside (kThetaMin, kThetaMax] or not finite
struct TanEnclosure {
  double hi, lo_l, hi_l;
  bool ok;
};

ORBFE_HD inline TanEnclosure tan_enclosure(double theta) {
  ORBFE_NO_CONTRACT
  // (-1)^k / (2k+1)! and (-1)^k / (2k)! as double-doubles
  constexpr double kS[15][2] = {
      {0x1.0000000000000p+0, 0x0.0p+0},                      {-0x1.5555555555555p-3, -0x1.5555555555555p-57},
      {0x1.1111111111111p-7, 0x1.1111111111111p-63},         {-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73},
      {0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73},       {-0x1.ae64567f544e4p-26, 0x1.c062e06d1f209p-80},
      {0x1.6124613a86d09p-33, 0x1.f28e0cc748ebep-87},        {-0x1.ae7f3e733b81fp-41, -0x1.1d8656b0ee8cbp-97},
      {0x1.952c77030ad4ap-49, 0x1.ac981465ddc6cp-103},       {-0x1.2f49b46814157p-57, -0x1.2650f61dbdcb4p-112},
      {0x1.71b8ef6dcf572p-66, -0x1.d043ae40c4647p-120},      {-0x1.761b41316381ap-75, 0x1.3423c7d91404fp-130},
      {0x1.3f3ccdd165fa9p-84, -0x1.58ddadf344487p-139},      {-0x1.d1ab1c2dccea3p-94, -0x1.054d0c78aea14p-149},
      {0x1.259f98b4358adp-103, 0x1.eaf8c39dd9bc5p-157}};
  constexpr double kC[16][2] = {
      {0x1.0000000000000p+0, 0x0.0p+0},                      {-0x1.0000000000000p-1, 0x0.0p+0},
      {0x1.5555555555555p-5, 0x1.5555555555555p-59},         {-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65},
      {0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76},        {-0x1.27e4fb7789f5cp-22, -0x1.cbbc05b4fa99ap-76},
      {0x1.1eed8eff8d898p-29, -0x1.2aec959e14c06p-83},       {-0x1.93974a8c07c9dp-37, -0x1.05d6f8a2efd1fp-92},
      {0x1.ae7f3e733b81fp-45, 0x1.1d8656b0ee8cbp-101},       {-0x1.6827863b97d97p-53, -0x1.eec01221a8b0bp-107},
      {0x1.e542ba4020225p-62, 0x1.ea72b4afe3c2fp-120},       {-0x1.0ce396db7f853p-70, 0x1.aebcdbd20331cp-124},
      {0x1.f2cf01972f578p-80, -0x1.9ada5fcc1ab14p-135},      {-0x1.88e85fc6a4e5ap-89, 0x1.71c37ebd16540p-143},
      {0x1.0a18a2635085dp-98, 0x1.b9e2e28e1aa54p-153},       {-0x1.3932c5047d60ep-108, -0x1.832b7b530a627p-162}};
  if (!(theta > kThetaMin && theta <= kThetaMax)) return {0.0, 0.0, 0.0, false};   // NaN fails both comparisons
  const DD x2 = dd_two_prod(theta, theta);
  DD s = {kS[14][0], kS[14][1]}, c = {kC[15][0], kC[15][1]};
  for (int k = 13; k >= 0; k--) s = dd_add(DD{kS[k][0], kS[k][1]}, dd_mul(x2, s));
  for (int k = 14; k >= 0; k--) c = dd_add(DD{kC[k][0], kC[k][1]}, dd_mul(x2, c));
  const DD t = dd_div(dd_mul_d(s, theta), c);
  const double r = t.hi * kTanRadius;   // tan > 0 on the domain; an exact scaling
  return {t.hi, t.lo - r, t.lo + r, true};
}

// Every double within (strictly) 1 ULP of some value of the enclosure, ascending: the two neighbours of the enclosure when it lies
// strictly between two adjacent doubles, three when it contains a double.  (|lo| <= ulp(hi) / 2 and the radius is 2^-27 ulp, so
// hi is the only double the enclosure can contain.)  Returns the count.
ORBFE_HD inline int tan_candidates(const TanEnclosure& e, double out[3]) {
  const uint64_t b = __builtin_bit_cast(uint64_t, e.hi);   // positive, normal, far from the ends of the exponent range
  const double below = __builtin_bit_cast(double, b - 1), above = __builtin_bit_cast(double, b + 1);
  int n = 0;
  if (e.lo_l <= 0.0) out[n++] = below;
  out[n++] = e.hi;
  if (e.hi_l >= 0.0) out[n++] = above;
  return n;
}

// K as the doubles the reference works on (float intrinsics widened)
struct EquidistantCamera { double fx, fy, cx, cy; };

ORBFE_HD inline bool equidistant_finite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u; }

// Frame.cc:366-383 from `scale` on: pu = pw * scale, K * (pu, 1) with its `0.0 *` terms and `/ pr2`, one rounding to float each
ORBFE_HD inline void equidistant_project(const EquidistantCamera& C, double pw0, double pw1, double scale, float* ox, float* oy) {
  ORBFE_NO_CONTRACT
  const double pu0 = pw0 * scale, pu1 = pw1 * scale;
  const double pr0 = C.fx * pu0 + 0.0 * pu1 + C.cx * 1.0;
  const double pr1 = 0.0 * pu0 + C.fy * pu1 + C.cy * 1.0;
  const double pr2 = 0.0 * pu0 + 0.0 * pu1 + 1.0 * 1.0;
  *ox = (float)(pr0 / pr2);
  *oy = (float)(pr1 / pr2);
}

// One point.  Returns true when DECIDED: (*ox, *oy) is then what the reference computes on any libm whose tan errs by less than
// 1 ULP.  false (undecided): the candidates disagree -- (*ox, *oy) is the lowest candidate's result --, a value is NaN / Inf, or
// theta is out of tan_enclosure's domain ((*ox, *oy) is then the input itself); the caller settles it with
// orbfe_undistort_equidistant on the host.
ORBFE_HD inline bool equidistant_verdict(const EquidistantCamera& C, float u, float v, float* ox, float* oy) {
  ORBFE_NO_CONTRACT
  const double pi0 = u, pi1 = v;
  const double pw0 = (pi0 - C.cx) / C.fx, pw1 = (pi1 - C.cy) / C.fy;
  const double theta_d = __builtin_sqrt(pw0 * pw0 + pw1 * pw1);
  if (!(theta_d > kThetaMin)) {   // the `: 1.0` branch (and a NaN theta, which the reference sends the same way)
    equidistant_project(C, pw0, pw1, 1.0, ox, oy);
    return equidistant_finite(*ox) && equidistant_finite(*oy);
  }
  const TanEnclosure e = tan_enclosure(theta_d);
  if (!e.ok) { *ox = u; *oy = v; return false; }
  double cand[3];
  const int nc = tan_candidates(e, cand);
  equidistant_project(C, pw0, pw1, cand[0] / theta_d, ox, oy);
  bool decided = equidistant_finite(*ox) && equidistant_finite(*oy);
  for (int k = 1; k < nc; k++) {
    float x, y;
    equidistant_project(C, pw0, pw1, cand[k] / theta_d, &x, &y);
    decided = decided && __builtin_bit_cast(uint32_t, x) == __builtin_bit_cast(uint32_t, *ox) &&
              __builtin_bit_cast(uint32_t, y) == __builtin_bit_cast(uint32_t, *oy);
  }
  return decided;
}

}  // namespace orbfe
