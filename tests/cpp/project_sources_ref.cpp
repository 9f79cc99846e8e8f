// project_sources_ref.cpp -- the test's reference for the source projection (orbfe_project_sources), independent of
// liborbfe.so.
//
// Restates, line by line and with the oracle's conventions for the cv::Mat arithmetic (oracle/orb_oracle.cpp cvGemm3,
// cvNorm3, predictScale), the part of the two searches between the loop head and GetFeaturesInArea:
//   ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th)          src/ORBmatcher.cc:1313-1347
//   ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, ...)   src/ORBmatcher.cc:1441-1479
//   MapPoint::GetMin/MaxDistanceInvariance, PredictScale                                     src/MapPoint.cc:358-379
// Built by the tests with g++ -ffp-contract=off into a shared object and called through ctypes.
#include <cmath>
#include <cstdint>

namespace {

void gemm3(const float A[9], const float b[3], double alpha, const float* c, double beta, float d[3]) {   // cvGemm3
  for (int i = 0; i < 3; i++) {
    const float t = A[3 * i] * b[0] + A[3 * i + 1] * b[1] + A[3 * i + 2] * b[2];
    d[i] = (float)((double)t * alpha + (double)(c ? c[i] : 0.f) * beta);
  }
}
double norm3(const float v[3]) {   // cv::norm
  double s = 0;
  for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
  return std::sqrt(s);
}
int predictScale(float mfMaxDistance, const float& currentDist, const float& logScaleFactor) {   // MapPoint.cc:370-379
  float ratio;
  ratio = mfMaxDistance / currentDist;
  return std::ceil(std::log(ratio) / logScaleFactor);   // std::log(float) = logf; the int conversion of the return
}

}  // namespace

extern "C" {

// cam: Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, logScaleFactor (OrbfeCamera) of the CURRENT frame; bounds: its mnMinX, mnMaxX,
// mnMinY, mnMaxY.  Source i: MapPoint = table row rows[i] of pos / min_raw / max_raw, octave src_octave[i]
// (LastFrame.mvKeys[i].octave); flags bit 16 = no MapPoint / mvbOutlier[i] (mode 0), no MapPoint / in sAlreadyFound (mode 1);
// bit 2 = isBad() (asked in mode 1 only).  mode 0 = LastFrame form, 1 = KeyFrame form.
// Outputs for a source that does not reach a non-empty GetFeaturesInArea cell range: valid 0, the rest 0.  Returns the
// number of valid sources.
int ref_project_sources(const float* pos, const float* min_raw, const float* max_raw, const int32_t* rows, const uint8_t* flags,
                        const int32_t* src_octave, int n, const float* cam, const float* bounds, int mode, uint8_t* valid,
                        float* uv, int32_t* level) {
  const float* Rcw = cam;
  const float* tcw = cam + 9;
  const float* Ow = cam + 12;   // -Rcw.t()*tcw (:1431), computed by the caller
  const float fx = cam[15], fy = cam[16], cx = cam[17], cy = cam[18], mfLogScaleFactor = cam[19];
  const float mnMinX = bounds[0], mnMaxX = bounds[1], mnMinY = bounds[2], mnMaxY = bounds[3];
  int nValid = 0;
  for (int i = 0; i < n; i++) {
    valid[i] = 0;
    uv[2 * i] = 0.f; uv[2 * i + 1] = 0.f; level[i] = 0;
    if (flags[i] & 16u) continue;                 // :1318-1321 pMP == NULL, mvbOutlier[i] / :1445-1447 NULL, sAlreadyFound
    if (mode == 1 && (flags[i] & 2u)) continue;   // :1447 pMP->isBad()
    const int r = rows[i];
    const float* x3Dw = pos + 3 * (size_t)r;      // pMP->GetWorldPos()
    float x3Dc[3];
    gemm3(Rcw, x3Dw, 1.0, tcw, 1.0, x3Dc);        // Rcw*x3Dw+tcw
    const float xc = x3Dc[0];
    const float yc = x3Dc[1];
    const float invzc = 1.0 / x3Dc[2];            // :1329 / :1455: double division
    if (mode == 0)
      if (invzc < 0) continue;                    // :1332-1333
    float u = fx * xc * invzc + cx;
    float v = fy * yc * invzc + cy;
    if (u < mnMinX || u > mnMaxX) continue;
    if (v < mnMinY || v > mnMaxY) continue;
    int nLevel;
    if (mode == 0) {
      nLevel = src_octave[i];                     // nLastOctave (:1344)
    } else {
      const float PO[3] = {x3Dw[0] - Ow[0], x3Dw[1] - Ow[1], x3Dw[2] - Ow[2]};   // :1466
      float dist3D = norm3(PO);
      const float maxDistance = 1.2f * max_raw[r];   // GetMaxDistanceInvariance
      const float minDistance = 0.8f * min_raw[r];   // GetMinDistanceInvariance
      if (dist3D < minDistance || dist3D > maxDistance) continue;
      nLevel = predictScale(max_raw[r], dist3D, mfLogScaleFactor);
    }
    // A NaN u or v (z = +-0 with x = y = 0) passes the bounds tests; GetFeaturesInArea(u, v, ...) (:1349 / :1481) then
    // computes nMaxCellX or nMaxCellY < 0 (src/Frame.cc:216-230) and returns no index: the source cannot match.
    if (!std::isfinite(u) || !std::isfinite(v)) continue;
    valid[i] = 1;
    uv[2 * i] = u;
    uv[2 * i + 1] = v;
    level[i] = nLevel;
    nValid++;
  }
  return nValid;
}

}  // extern "C"
