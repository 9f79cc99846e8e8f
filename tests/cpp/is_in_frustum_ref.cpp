// is_in_frustum_ref.cpp -- the test's reference for the local-map projection, independent of liborbfe.so.
//
// Restates, line by line and with the oracle's conventions for the cv::Mat arithmetic (oracle/orb_oracle.cpp cvGemm3,
// cvNorm3, cvDot3, predictScale):
//   Tracking::SearchLocalPoints   src/Tracking.cc:798-814   skip mnLastFrameSeen == mCurrentFrame.mnId and isBad(), then
//                                                           isInFrustum(pMP, 0.5) and count nToMatch
//   Frame::isInFrustum            src/Frame.cc:151-207
//   MapPoint::GetMin/MaxDistanceInvariance, PredictScale    src/MapPoint.cc:358-379 (host libm logf)
// Also host libm logf over an array (ref_logf_array).  Built by the tests with g++ -ffp-contract=off into a shared object
// and called through ctypes.
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
double dot3(const float a[3], const float b[3]) {   // Mat::dot
  double r = 0;
  for (int k = 0; k < 3; k++) r += (double)a[k] * (double)b[k];
  return r;
}
int predictScale(float mfMaxDistance, const float& currentDist, const float& logScaleFactor) {   // MapPoint.cc:370-379
  float ratio;
  ratio = mfMaxDistance / currentDist;
  return std::ceil(std::log(ratio) / logScaleFactor);   // std::log(float) = logf; the int conversion of the return
}

}  // namespace

extern "C" {

// cam: Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, logScaleFactor (OrbfeCamera);  bounds: mnMinX, mnMaxX, mnMinY, mnMaxY.
// MapPoint i: table row rows[i] of pos / normal / min_raw / max_raw; flags bit 2 = isBad(), bit 16 = mnLastFrameSeen == mnId.
// Outputs where isInFrustum returned false: in_view 0, the rest 0.  Returns nToMatch.
int ref_search_local_points_projection(const float* pos, const float* normal, const float* min_raw, const float* max_raw,
                                       const int32_t* rows, const uint8_t* flags, int n, const float* cam, const float* bounds,
                                       float viewingCosLimit, uint8_t* in_view, float* proj_xy, int32_t* level, float* view_cos) {
  const float* mRcw = cam;
  const float* mtcw = cam + 9;
  const float* mOw = cam + 12;
  const float fx = cam[15], fy = cam[16], cx = cam[17], cy = cam[18], mfLogScaleFactor = cam[19];
  const float mnMinX = bounds[0], mnMaxX = bounds[1], mnMinY = bounds[2], mnMaxY = bounds[3];
  int nToMatch = 0;
  for (int i = 0; i < n; i++) {
    in_view[i] = 0;
    proj_xy[2 * i] = 0.f; proj_xy[2 * i + 1] = 0.f; level[i] = 0; view_cos[i] = 0.f;
    if (flags[i] & 16u) continue;   // pMP->mnLastFrameSeen == mCurrentFrame.mnId
    if (flags[i] & 2u) continue;    // pMP->isBad()
    const int r = rows[i];
    // bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit)
    const float* P = pos + 3 * (size_t)r;                       // pMP->GetWorldPos()
    float Pc[3];
    gemm3(mRcw, P, 1.0, mtcw, 1.0, Pc);                         // mRcw*P+mtcw
    const float& PcX = Pc[0];
    const float& PcY = Pc[1];
    const float& PcZ = Pc[2];
    if (PcZ < 0.0f) continue;
    const float invz = 1.0f / PcZ;
    const float u = fx * PcX * invz + cx;
    const float v = fy * PcY * invz + cy;
    if (u < mnMinX || u > mnMaxX) continue;
    if (v < mnMinY || v > mnMaxY) continue;
    const float maxDistance = 1.2f * max_raw[r];                 // GetMaxDistanceInvariance
    const float minDistance = 0.8f * min_raw[r];                 // GetMinDistanceInvariance
    const float PO[3] = {P[0] - mOw[0], P[1] - mOw[1], P[2] - mOw[2]};
    const float dist = (float)norm3(PO);
    if (dist < minDistance || dist > maxDistance) continue;
    const float* Pn = normal + 3 * (size_t)r;                   // pMP->GetNormal()
    const float viewCos = (float)(dot3(PO, Pn) / dist);
    if (viewCos < viewingCosLimit) continue;
    const int nPredictedLevel = predictScale(max_raw[r], dist, mfLogScaleFactor);
    in_view[i] = 1;                                             // mbTrackInView
    proj_xy[2 * i] = u;                                         // mTrackProjX
    proj_xy[2 * i + 1] = v;                                     // mTrackProjY
    level[i] = nPredictedLevel;                                 // mnTrackScaleLevel
    view_cos[i] = viewCos;                                      // mTrackViewCos
    nToMatch++;                                                 // pMP->IncreaseVisible(); nToMatch++
  }
  return nToMatch;
}

}  // extern "C"

extern "C" void ref_logf_array(const float* x, int n, float* out) {   // host libm logf, elementwise
  for (int i = 0; i < n; i++) out[i] = std::log(x[i]);
}
