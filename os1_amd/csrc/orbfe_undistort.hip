// orbfe_undistort.hip -- Frame::UndistortKeyPoints (reference src/Frame.cc:284-319) for the pinhole model, on the GPU.
//
// Behaviour contract: cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) exactly as the host function
// orbfe_undistort_pinhole (orbfe_matcher.hip) states it: normalise with K, five fixed-point iterations of the inverse
// Brown / rational model over k1 k2 p1 p2 k3 k4 k5 k6, the `icdist < 0` fall-back to the undistorted guess, re-projection
// with K including its `0 * x` / `0 * y` terms, one final rounding to float.
//
// Arithmetic: IEEE double add, multiply and divide only -- no libm call, no reciprocal approximation (the library is built
// without fast-math flags, so `/` is the correctly rounded division), and no contraction anywhere in the function (the
// build's -ffp-contract=off, repeated by the pragma below), so every operation rounds on its own as on x86-64.
//
// The kernel stands alone behind k_describe: 2 000 points x 5 dependent iterations is latency, and fp64 registers inside
// the descriptor kernel would cost every caller occupancy.
#include <hip/hip_runtime.h>

#include "equidistant_tan.h"
#include "orbfe_internal.h"

namespace orbfe {

// The distorted position of point i in either input form (UndistortSlots); false: a dead slot, nothing to write.
__device__ __forceinline__ bool undistort_input(const UndistortSlots& A, int i, float& fu, float& fv) {
#pragma clang fp contract(off)
  if (A.sel) {
    const int f = i / A.selPerFrame, s = i - f * A.selPerFrame;
    int l = 0;
    for (int q = 1; q < A.nlevels; q++) l += s >= A.selOff[q];
    if ((uint32_t)(s - A.selOff[l]) >= A.selCount[(long long)f * kMaxLevels + l]) return false;   // dead slot
    const uint32_t xy = A.sel[i].xy;
    fu = (float)(xy & 0xffff);
    fv = (float)(xy >> 16);
    if (l != 0) { const float scale = A.sf[l]; fu *= scale; fv *= scale; }   // ORBextractor.cc:959-965
  } else {
    fu = A.in[2 * (long long)i];
    fv = A.in[2 * (long long)i + 1];
  }
  return true;
}

__global__ __launch_bounds__(64) void k_undistort(UndistortArgs A) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  float fu, fv;
  if (!undistort_input(A, i, fu, fv)) return;
  const CameraModel& C = A.cam;
  const double u = fu, v = fv;
  double x = (u - C.cx) * C.ifx, y = (v - C.cy) * C.ify;
  const double x0 = x, y0 = y;
  for (int it = 0; it < 5; it++) {
    const double r2 = x * x + y * y;
    const double icdist = (1 + ((C.k[7] * r2 + C.k[6]) * r2 + C.k[5]) * r2) / (1 + ((C.k[4] * r2 + C.k[1]) * r2 + C.k[0]) * r2);
    if (icdist < 0) {   // the model folds back on itself here: OpenCV returns the undistorted guess
      x = (u - C.cx) * C.ifx;
      y = (v - C.cy) * C.ify;
      break;
    }
    const double deltaX = 2 * C.k[2] * x * y + C.k[3] * (r2 + 2 * x * x);
    const double deltaY = C.k[2] * (r2 + 2 * y * y) + 2 * C.k[3] * x * y;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  const double xx = C.fx * x + 0 * y + C.cx, yy = 0 * x + C.fy * y + C.cy, ww = 1. / (0 * x + 0 * y + 1);
  A.out[2 * (long long)i] = (float)(xx * ww);
  A.out[2 * (long long)i + 1] = (float)(yy * ww);
}

// The equidistant (fisheye) model of Frame::antidistorsionarProyeccionEquidistante (Frame.cc:355-384): equidistant_tan.h's verdict
// per point.  A decided point's two floats are final.  An undecided one gets the lowest candidate's floats and its index appended to
// the launch's list (the host settles it with its own std::tan): the counter keeps counting past the list's capacity, which tells
// the host to settle the whole launch.  A separate kernel: the double-double series would cost the pinhole kernel its registers.
__global__ __launch_bounds__(64) void k_undistort_equidistant(EquidistantArgs A) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  float fu, fv;
  if (!undistort_input(A, i, fu, fv)) return;
  float ox, oy;
  const bool decided = equidistant_verdict(A.cam, fu, fv, &ox, &oy);
  A.out[2 * (long long)i] = ox;
  A.out[2 * (long long)i + 1] = oy;
  if (A.flags) A.flags[i] = decided ? 0 : 1;
  if (!decided) {
    const uint32_t k = atomicAdd(A.undecided, 1u);
    if (k < (uint32_t)kUndecidedCap) A.undecided[1 + k] = (uint32_t)i;
  }
}

void launch_undistort_equidistant(const EquidistantArgs& A, hipStream_t st) {
  if (A.n <= 0) return;
  hipLaunchKernelGGL(k_undistort_equidistant, dim3((A.n + 63) / 64), dim3(64), 0, st, A);
}

void launch_undistort(const UndistortArgs& A, hipStream_t st) {
  if (A.n <= 0) return;
  hipLaunchKernelGGL(k_undistort, dim3((A.n + 63) / 64), dim3(64), 0, st, A);
}

}  // namespace orbfe
