// project_keyframe_ref.cpp -- the test's reference for the keyframe projection (orbfe_project_keyframe), independent of
// liborbfe.so.
//
// Restates, line by line and with the oracle's conventions for the cv::Mat arithmetic (oracle/orb_oracle.cpp cvGemm3,
// cvGemmT3, cvNorm3, cvDot3, decomposeScw, predictScale), the part of the four keyframe-side searches between GetWorldPos()
// and KeyFrame::GetFeaturesInArea:
//   ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th)   src/ORBmatcher.cc:316-357
//   ORBmatcher::Fuse(KeyFrame* pKF, vpMapPoints, th)                                      src/ORBmatcher.cc:833-873
//   ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint)            src/ORBmatcher.cc:973-1015
//   ORBmatcher::SearchBySim3(pKF1, pKF2, ...), both directions                            src/ORBmatcher.cc:1122-1155, 1202-1235
//   KeyFrame::IsInImage                                                                   src/KeyFrame.cc:678-681
//   MapPoint::GetMin/MaxDistanceInvariance, PredictScale                                  src/MapPoint.cc:358-379
// and the matrices each of them computes once per call (:293-298, :949-954, :1075-1084, KeyFrame::SetPose).
// Built by the tests with g++ -ffp-contract=off into a shared object and called through ctypes.
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

void gemm3(const float A[9], const float b[3], double alpha, const float* c, double beta, float d[3]) {   // cvGemm3
  for (int i = 0; i < 3; i++) {
    const float t = A[3 * i] * b[0] + A[3 * i + 1] * b[1] + A[3 * i + 2] * b[2];
    d[i] = (float)((double)t * alpha + (double)(c ? c[i] : 0.f) * beta);
  }
}
void gemmT3(const float A[9], const float b[3], double alpha, float d[3]) {   // alpha * A.t() * b (cvGemmT3)
  for (int i = 0; i < 3; i++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)A[3 * k + i] * (double)b[k];
    d[i] = (float)(s * alpha);
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
bool isInImage(const float* b, const float& x, const float& y) {   // KeyFrame.cc:678-681
  return (x >= b[0] && x < b[1] && y >= b[2] && y < b[3]);
}

}  // namespace

extern "C" {

// Scw (row-major 4x4) -> Rcw, tcw, Ow   (ORBmatcher.cc:293-298 / :949-954)
void ref_decompose_scw(const float* S, float* Rcw, float* tcw, float* Ow) {
  float sR[9], st[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) sR[3 * r + c] = S[4 * r + c];
    st[r] = S[4 * r + 3];
  }
  const float scw = std::sqrt(dot3(sR, sR));           // sqrt(sRcw.row(0).dot(sRcw.row(0)))
  const float inv = (float)(1.0 / (double)scw);         // M/s = M * (1./s), the factor rounded to float
  for (int i = 0; i < 9; i++) Rcw[i] = sR[i] * inv;
  for (int i = 0; i < 3; i++) tcw[i] = st[i] * inv;
  gemmT3(Rcw, tcw, -1.0, Ow);                           // -Rcw.t()*tcw
}

// pKF->GetCameraCenter(): KeyFrame::SetPose computes Ow = -Rwc*tcw with Rwc = Rcw.t() already evaluated (KeyFrame.cc:93-97)
void ref_keyframe_center(const float* Rcw, const float* tcw, float* Ow) {
  float Rwc[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Rwc[3 * r + c] = Rcw[3 * c + r];
  gemm3(Rwc, tcw, -1.0, nullptr, 0.0, Ow);
}

// sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12   (ORBmatcher.cc:1080-1084)
void ref_sim3_matrices(float s12, const float* R12, const float* t12, float* sR12, float* sR21, float* t21) {
  for (int i = 0; i < 9; i++) sR12[i] = R12[i] * s12;
  const float is = (float)(1.0 / (double)s12);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) sR21[3 * r + c] = R12[3 * c + r] * is;
  gemm3(sR21, t12, -1.0, nullptr, 0.0, t21);
}

// MapPoint i = table row rows[i] of pos / normal / min_raw / max_raw; flags bit 2 = isBad(), bit 16 = skipped by the loop
// head (in spAlreadyFound, NULL, IsInKeyFrame, vbAlreadyMatched).  R, t: the first transform; sR, t2: the second (NULL: none);
// Ow: the camera centre; K: fx, fy, cx, cy, mfLogScaleFactor; bounds: the searched keyframe's mnMinX, mnMaxX, mnMinY, mnMaxY.
// Outputs of a point that does not reach GetFeaturesInArea: valid 0, the rest 0; a valid point whose level lies outside
// [0, nlevels) keeps its level and gets radius 0 (the reference would index mvScaleFactors out of range).  reason (optional):
// 0 valid, 1 flagged, 2 depth, 3 image, 4 nearer than 0.8f*min, 5 farther than 1.2f*max, 6 viewing angle.  Returns the number
// of valid points.
int ref_project_keyframe(const float* pos, const float* normal, const float* min_raw, const float* max_raw, const int32_t* rows,
                         const uint8_t* flags, int n, const float* R, const float* t, const float* sR, const float* t2,
                         const float* Ow, const float* K, const float* bounds, int invzInDouble, int checkViewingAngle,
                         int distanceFromCameraPoint, const float* mvScaleFactors, int nlevels, float th, uint8_t* valid, float* uv,
                         int32_t* level, float* radius, uint8_t* reason) {
  const float fx = K[0], fy = K[1], cx = K[2], cy = K[3], mfLogScaleFactor = K[4];
  int nValid = 0;
  for (int i = 0; i < n; i++) {
    valid[i] = 0;
    uv[2 * i] = 0.f; uv[2 * i + 1] = 0.f; level[i] = 0; radius[i] = 0.f;
    if (reason) reason[i] = 1;
    if (flags[i] & (2u | 16u)) continue;
    const size_t r = (size_t)rows[i];
    const float* p3Dw = pos + 3 * r;              // pMP->GetWorldPos()
    float p3Dc[3];
    gemm3(R, p3Dw, 1.0, t, 1.0, p3Dc);            // Rcw*p3Dw+tcw / R1w*p3Dw + t1w
    if (sR) {
      float q[3];
      gemm3(sR, p3Dc, 1.0, t2, 1.0, q);           // sR21*p3Dc1 + t21 / sR12*p3Dc2 + t12
      p3Dc[0] = q[0]; p3Dc[1] = q[1]; p3Dc[2] = q[2];
    }
    if (reason) reason[i] = 2;
    if (p3Dc[2] < 0.0f) continue;                 // Depth must be positive
    float invz;
    if (invzInDouble) invz = 1.0 / p3Dc[2];       // :983 / :1130 / :1210
    else invz = 1 / p3Dc[2];                      // :326 / :840
    const float x = p3Dc[0] * invz;
    const float y = p3Dc[1] * invz;
    const float u = fx * x + cx;
    const float v = fy * y + cy;
    if (reason) reason[i] = 3;
    if (!isInImage(bounds, u, v)) continue;       // Point must be inside the image
    const float maxDistance = 1.2f * max_raw[r];  // GetMaxDistanceInvariance
    const float minDistance = 0.8f * min_raw[r];  // GetMinDistanceInvariance
    float PO[3];
    if (distanceFromCameraPoint) { PO[0] = p3Dc[0]; PO[1] = p3Dc[1]; PO[2] = p3Dc[2]; }   // cv::norm(p3Dc2) / cv::norm(p3Dc1)
    else { PO[0] = p3Dw[0] - Ow[0]; PO[1] = p3Dw[1] - Ow[1]; PO[2] = p3Dw[2] - Ow[2]; }   // PO = p3Dw-Ow
    const float dist3D = norm3(PO);
    if (reason) reason[i] = dist3D < minDistance ? 4 : 5;
    if (dist3D < minDistance || dist3D > maxDistance) continue;
    if (checkViewingAngle) {
      if (reason) reason[i] = 6;
      if (dot3(PO, normal + 3 * r) < 0.5 * dist3D) continue;   // Viewing angle must be less than 60 deg
    }
    const int nPredictedLevel = predictScale(max_raw[r], dist3D, mfLogScaleFactor);
    if (reason) reason[i] = 0;
    valid[i] = 1;
    uv[2 * i] = u;
    uv[2 * i + 1] = v;
    level[i] = nPredictedLevel;
    if (nPredictedLevel >= 0 && nPredictedLevel < nlevels) radius[i] = th * mvScaleFactors[nPredictedLevel];
    nValid++;
  }
  return nValid;
}

}  // extern "C"
