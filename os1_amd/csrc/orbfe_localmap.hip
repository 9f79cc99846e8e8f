// orbfe_localmap.hip -- the local map on the device: Frame::isInFrustum over Tracking's local MapPoints, and that
// projection fused with SearchByProjection(F, vpLocalMapPoints, th); the projection loops of the other searches that read the
// same table (k_project_sources: last frame / keyframe into the current frame; k_project_keyframe: MapPoints into a keyframe
// for SearchByProjection(KeyFrame*, Scw), Fuse, Fuse(Scw) and SearchBySim3), each fused with its search in the same way.
//
// Tracking::SearchLocalPoints (reference src/Tracking.cc:798-825) calls Frame::isInFrustum(pMP, 0.5) (src/Frame.cc:151-207)
// for every local MapPoint on the tracking thread, then ORBmatcher::SearchByProjection on the ones in view.  Here the
// MapPoint fields the projection reads live in a device table (one 64-byte row per MapPoint, kept current by the caller
// with orbfe_local_map_set_rows), k_project_local_map restates isInFrustum one lane per MapPoint, and the fused call leaves
// its results in device memory where the resident frame's window search (orbfe_frame.hip) reads them: one submission of
// three kernels on the matcher's stream, no copy command in between.
//
// The arithmetic is the reference's cv::Mat float arithmetic as the oracle pins it (oracle/orb_oracle.cpp cvGemm3, cvNorm3,
// cvDot3, predictScale; include/orbfe/orb_shim.hpp RestatedOps): Rcw*P+tcw is a float dot in source order with a double
// epilogue, cv::norm and Mat::dot accumulate in double, and PredictScale's log is glibc logf (glibc_logf.h).  The library is
// built with -ffp-contract=off, so every float operation rounds on its own as in the reference.
#include "orbfe_matcher_internal.h"
#include "glibc_logf.h"

#include <atomic>

struct orbfe_frame;
namespace orbfe {
void frame_bounds(const orbfe_frame* f, float out[4]);
int sbp_frame_device_queries(orbfe_matcher* m, orbfe_frame* f, const float* scale_factors, int nlevels, const uint8_t* kp_occupied,
                             const float* d_xy, const int32_t* d_level, const float* d_viewcos, const uint8_t* d_flags,
                             const uint8_t* d_desc, const int32_t* d_desc_row, int n_mp, float th, float nnratio,
                             int32_t* kp_assigned, int* nmatches);
int sbp_uv_frame_device_queries(orbfe_matcher* m, orbfe_frame* f, const float* scale_factors, int nlevels, const uint8_t* kp_occupied,
                                const float* d_xy, const int32_t* d_level, const float* d_angle, const uint8_t* d_valid,
                                const uint8_t* d_claim, const uint8_t* d_desc, const int32_t* d_desc_row, int n_src, float th,
                                int max_dist, int skip_any_occupied, int check_orientation, int32_t* kp_assigned, int* nmatches);
int search_projected_frame_device_queries(orbfe_matcher* m, orbfe_frame* f, const float* scale_factors, int nlevels, float th,
                                          const float* d_xy, const int32_t* d_level, const float* d_radius, const uint8_t* d_valid,
                                          const uint8_t* d_desc, const int32_t* d_desc_row, int n_src, const uint8_t* kp_skip, int claim,
                                          const float* inv_level_sigma2, double chi2, int max_dist, int32_t* best_idx, int32_t* best_dist,
                                          int* nmatches);
void frame_source_arrays(const orbfe_frame* f, const int** oct, const float** angle, int* maxOctave);
void frame_wait_ready(orbfe_frame* f, hipStream_t st);
}  // namespace orbfe

namespace {

constexpr int kRowBytes = 64;        // pos[3], normal[3], mfMinDistance, mfMaxDistance, descriptor[32]
constexpr int kProjThreads = 256;
constexpr int kStageBytes = 80;      // set_rows staging record: row, field mask, pad, the 64-byte row

// set_rows: staged records (page-locked, read in place) -> table rows; fields whose mask bit is clear keep their value.
// Mask bits: 1 pos, 2 normal, 4 min, 8 max, 16 descriptor.
__global__ __launch_bounds__(256) void k_local_map_scatter(const uint8_t* __restrict__ stage, int n, uint8_t* __restrict__ table) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* rec = stage + (size_t)i * kStageBytes;
  const int row = reinterpret_cast<const int*>(rec)[0];
  const unsigned mask = reinterpret_cast<const unsigned*>(rec)[1];
  const float* src = reinterpret_cast<const float*>(rec + 16);
  float* dst = reinterpret_cast<float*>(table + (size_t)row * kRowBytes);
  if (mask & 1u) { dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; }
  if (mask & 2u) { dst[3] = src[3]; dst[4] = src[4]; dst[5] = src[5]; }
  if (mask & 4u) dst[6] = src[6];
  if (mask & 8u) dst[7] = src[7];
  if (mask & 16u) {
    const uint4* s4 = reinterpret_cast<const uint4*>(rec + 48);
    uint4* d4 = reinterpret_cast<uint4*>(table + (size_t)row * kRowBytes + 32);
    d4[0] = s4[0];
    d4[1] = s4[1];
  }
}

struct ProjParams {
  const uint8_t* table;
  const int32_t* rows;         // [n] (page-locked host memory)
  const uint8_t* flags;        // [n]
  int n;
  OrbfeCamera cam;
  float minX, maxX, minY, maxY;
  float cosLimit;
  int nlevels;                 // fused call: levels outside [0, nlevels) are taken out of the search and reported
  // outputs in page-locked host memory (any may be null)
  uint8_t* inView;
  float* xy;
  int32_t* level;
  float* vcos;
  // fused call: the search's queries in device memory (null: projection only)
  float* dxy;
  int32_t* dlevel;
  float* dvcos;
  uint8_t* dflags;
  int32_t* drow;
  int* blockInfo;              // [2 * blocks] page-locked: MapPoints in view, first MapPoint with an out-of-range level (-1)
};

// bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit)  (src/Frame.cc:151-207), one lane per listed MapPoint
__global__ __launch_bounds__(kProjThreads) void k_project_local_map(ProjParams P) {
  __shared__ int firstBad;
  if (threadIdx.x == 0) firstBad = INT_MAX;
  __syncthreads();
  const int i = blockIdx.x * kProjThreads + threadIdx.x;
  bool inView = false;
  float u = 0.f, v = 0.f, viewCos = 0.f;
  int lvl = 0, row = 0;
  unsigned fl = 0;
  if (i < P.n) {
    fl = P.flags[i];
    row = P.rows[i];
    // Tracking.cc:804-807: mnLastFrameSeen == mCurrentFrame.mnId, isBad()
    if (!(fl & (ORBFE_MP_BAD | ORBFE_MP_SKIP))) {
      const float4* R = reinterpret_cast<const float4*>(P.table + (size_t)row * kRowBytes);
      const float4 a = R[0], b = R[1];
      const float Pw[3] = {a.x, a.y, a.z};                  // GetWorldPos()
      const float Pn[3] = {a.w, b.x, b.y};                  // GetNormal()
      const float minRaw = b.z, maxRaw = b.w;               // mfMinDistance, mfMaxDistance
      const OrbfeCamera& C = P.cam;
      // Pc = mRcw*P+mtcw: gemm, float dot in source order, double epilogue (alpha = beta = 1)
      float Pc[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float t = C.Rcw[3 * k] * Pw[0] + C.Rcw[3 * k + 1] * Pw[1] + C.Rcw[3 * k + 2] * Pw[2];
        Pc[k] = (float)((double)t * 1.0 + (double)C.tcw[k] * 1.0);
      }
      if (!(Pc[2] < 0.0f)) {                                // Frame.cc:166-167
        const float invz = 1.0f / Pc[2];
        u = C.fx * Pc[0] * invz + C.cx;
        v = C.fy * Pc[1] * invz + C.cy;
        if (!(u < P.minX || u > P.maxX) && !(v < P.minY || v > P.maxY)) {   // Frame.cc:173-176
          const float maxDistance = 1.2f * maxRaw;          // GetMaxDistanceInvariance (MapPoint.cc:364-368)
          const float minDistance = 0.8f * minRaw;          // GetMinDistanceInvariance (MapPoint.cc:358-362)
          const float PO[3] = {Pw[0] - C.Ow[0], Pw[1] - C.Ow[1], Pw[2] - C.Ow[2]};
          double s = 0.0;                                   // cv::norm(PO)
#pragma unroll
          for (int k = 0; k < 3; k++) s += (double)PO[k] * (double)PO[k];
          const float dist = (float)sqrt(s);
          if (!(dist < minDistance || dist > maxDistance)) {
            double d = 0.0;                                 // PO.dot(Pn)
#pragma unroll
            for (int k = 0; k < 3; k++) d += (double)PO[k] * (double)Pn[k];
            viewCos = (float)(d / (double)dist);
            if (!(viewCos < P.cosLimit)) {
              // PredictScale (MapPoint.cc:370-379): ceil(log(ratio)/logScaleFactor) with float ratio, converted to int as
              // the host does (an out-of-range value becomes INT_MIN)
              const float ratio = maxRaw / dist;
              const float c = ceilf(orbfe::logf_glibc(ratio) / C.logScaleFactor);
              lvl = (c >= -2147483648.0f && c < 2147483648.0f) ? (int)c : INT_MIN;
              inView = true;
            }
          }
        }
      }
    }
    if (!inView) { u = 0.f; v = 0.f; viewCos = 0.f; lvl = 0; }
    if (P.inView) P.inView[i] = inView ? 1 : 0;
    if (P.xy) { P.xy[2 * i] = u; P.xy[2 * i + 1] = v; }
    if (P.level) P.level[i] = lvl;
    if (P.vcos) P.vcos[i] = viewCos;
    if (P.dxy) {
      // the search reads these: a level outside [0, nlevels) is never handed to it (the call fails instead)
      const bool levelOk = lvl >= 0 && lvl < P.nlevels;
      if (inView && !levelOk) atomicMin(&firstBad, i);
      reinterpret_cast<float2*>(P.dxy)[i] = make_float2(u, v);
      P.dlevel[i] = levelOk ? lvl : 0;
      P.dvcos[i] = viewCos;
      P.dflags[i] = (uint8_t)((inView && levelOk ? ORBFE_MP_IN_VIEW : 0u) | (fl & (ORBFE_MP_CANDIDATO | ORBFE_MP_OBSERVED)));
      P.drow[i] = inView ? 2 * row : 0;   // descriptor = 32-byte row 2*row of (table + 32)
    }
  }
  const int count = __syncthreads_count(inView ? 1 : 0);
  if (threadIdx.x == 0) {
    P.blockInfo[2 * blockIdx.x] = count;
    P.blockInfo[2 * blockIdx.x + 1] = firstBad == INT_MAX ? -1 : firstBad;
    __threadfence_system();
  }
}

struct SrcParams {
  const uint8_t* table;
  const int32_t* rows;         // [n] (page-locked host memory)
  const uint8_t* flags;        // [n]
  const int* srcOct;           // [n] the SOURCE frame's resident octaves (mvKeys[i].octave)
  int n;
  int mode;                    // ORBFE_SRC_LAST_FRAME / ORBFE_SRC_KEYFRAME
  OrbfeCamera cam;
  float minX, maxX, minY, maxY;   // the CURRENT frame's bounds
  int nlevels;                 // fused call: levels outside [0, nlevels) are taken out of the search and reported
  // outputs in page-locked host memory (any may be null)
  uint8_t* valid;
  float* uv;
  int32_t* level;
  // fused call: the search's queries in device memory (null: projection only)
  float* dxy;
  int32_t* dlevel;
  uint8_t* dvalid;
  uint8_t* dclaim;
  int32_t* drow;
  int* blockInfo;              // [2 * blocks] page-locked: sources valid, first valid source with an out-of-range level (-1)
};

// The projection loops of ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th)
// (src/ORBmatcher.cc:1313-1347) and (Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (:1441-1479), one lane
// per source keypoint: everything between GetWorldPos() and GetFeaturesInArea.  The source keypoint's angle (the rotation
// check, :1386 / :1515) is not touched here: the search reads it from the source frame's resident copy.
__global__ __launch_bounds__(kProjThreads) void k_project_sources(SrcParams P) {
  __shared__ int firstBad;
  if (threadIdx.x == 0) firstBad = INT_MAX;
  __syncthreads();
  const int i = blockIdx.x * kProjThreads + threadIdx.x;
  bool valid = false;
  float u = 0.f, v = 0.f;
  int lvl = 0, row = 0;
  unsigned fl = 0;
  if (i < P.n) {
    fl = P.flags[i];
    row = P.rows[i];
    // :1318-1321 no MapPoint / mvbOutlier[i] (isBad() is not asked); :1445-1447 no MapPoint / isBad() / in sAlreadyFound
    if (!(fl & (P.mode == ORBFE_SRC_KEYFRAME ? (ORBFE_MP_BAD | ORBFE_MP_SKIP) : ORBFE_MP_SKIP))) {
      const float4* R = reinterpret_cast<const float4*>(P.table + (size_t)row * kRowBytes);
      const float4 a = R[0], b = R[1];
      const float Pw[3] = {a.x, a.y, a.z};                  // GetWorldPos()
      const float maxRaw = b.w, minRaw = b.z;               // mfMaxDistance, mfMinDistance
      const OrbfeCamera& C = P.cam;
      // x3Dc = Rcw*x3Dw+tcw: gemm, float dot in source order, double epilogue (alpha = beta = 1)
      float Pc[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float t = C.Rcw[3 * k] * Pw[0] + C.Rcw[3 * k + 1] * Pw[1] + C.Rcw[3 * k + 2] * Pw[2];
        Pc[k] = (float)((double)t * 1.0 + (double)C.tcw[k] * 1.0);
      }
      const float invzc = (float)(1.0 / (double)Pc[2]);     // :1329 / :1455: a DOUBLE division, rounded to float
      if (P.mode == ORBFE_SRC_KEYFRAME || !(invzc < 0)) {   // :1332-1333 (the KeyFrame form has no such test)
        u = C.fx * Pc[0] * invzc + C.cx;
        v = C.fy * Pc[1] * invzc + C.cy;
        if (!(u < P.minX || u > P.maxX) && !(v < P.minY || v > P.maxY)) {   // :1339-1342 / :1460-1463
          if (P.mode == ORBFE_SRC_KEYFRAME) {
            const float PO[3] = {Pw[0] - C.Ow[0], Pw[1] - C.Ow[1], Pw[2] - C.Ow[2]};   // :1466
            double s = 0.0;                                 // cv::norm(PO)
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)PO[k] * (double)PO[k];
            const float dist3D = (float)sqrt(s);
            const float maxDistance = 1.2f * maxRaw;        // GetMaxDistanceInvariance (MapPoint.cc:364-368)
            const float minDistance = 0.8f * minRaw;        // GetMinDistanceInvariance (MapPoint.cc:358-362)
            if (!(dist3D < minDistance || dist3D > maxDistance)) {   // :1473-1474
              // PredictScale (MapPoint.cc:370-379), converted to int as the host does (an out-of-range value becomes INT_MIN)
              const float ratio = maxRaw / dist3D;
              const float c = ceilf(orbfe::logf_glibc(ratio) / C.logScaleFactor);
              lvl = (c >= -2147483648.0f && c < 2147483648.0f) ? (int)c : INT_MIN;
              valid = true;
            }
          } else {
            lvl = P.srcOct[i];                              // nLastOctave = LastFrame.mvKeys[i].octave (:1344)
            valid = true;
          }
          // z = +-0 with x = y = 0 makes u or v NaN, which passes the bounds tests above (every comparison is false).  The
          // reference then calls GetFeaturesInArea(u, v, ...) (:1349 / :1481) with it, whose cell range (Frame.cc:216-230)
          // comes out empty (nMaxCellX or nMaxCellY < 0): no candidate, no match.  Such a source is written as invalid.
          if (!(fabsf(u) <= 3.402823466e+38f) || !(fabsf(v) <= 3.402823466e+38f)) valid = false;
        }
      }
    }
    if (!valid) { u = 0.f; v = 0.f; lvl = 0; }
    if (P.valid) P.valid[i] = valid ? 1 : 0;
    if (P.uv) { P.uv[2 * i] = u; P.uv[2 * i + 1] = v; }
    if (P.level) P.level[i] = lvl;
    if (P.dxy) {
      // the search reads these: a level outside [0, nlevels) is never handed to it (the call fails instead)
      const bool levelOk = lvl >= 0 && lvl < P.nlevels;
      if (valid && !levelOk) atomicMin(&firstBad, i);
      reinterpret_cast<float2*>(P.dxy)[i] = make_float2(u, v);
      P.dlevel[i] = levelOk ? lvl : 0;
      P.dvalid[i] = valid && levelOk ? 1 : 0;
      P.dclaim[i] = (uint8_t)(fl & ORBFE_MP_OBSERVED);
      P.drow[i] = valid ? 2 * row : 0;    // descriptor = 32-byte row 2*row of (table + 32)
    }
  }
  const int count = __syncthreads_count(valid ? 1 : 0);
  if (threadIdx.x == 0) {
    P.blockInfo[2 * blockIdx.x] = count;
    P.blockInfo[2 * blockIdx.x + 1] = firstBad == INT_MAX ? -1 : firstBad;
    __threadfence_system();
  }
}

struct KfParams {
  const uint8_t* table;
  const int32_t* rows;         // [n] (page-locked host memory)
  const uint8_t* flags;        // [n]
  int n;
  OrbfeKeyFrameProjection proj;
  float minX, maxX, minY, maxY;   // the TARGET keyframe's bounds
  int nlevels;
  float th;
  float sf[32];                // the target keyframe's mvScaleFactors
  // outputs in page-locked host memory (any may be null)
  uint8_t* valid;
  float* uv;
  int32_t* level;
  float* radius;
  // fused call: the search's queries in device memory (null: projection only)
  float* dxy;
  int32_t* dlevel;
  float* dradius;
  uint8_t* dvalid;
  int32_t* drow;
  int* blockInfo;              // [2 * blocks] page-locked: points valid, first valid point with an out-of-range level (-1)
};

// The projection loops of the keyframe-side searches, one lane per listed MapPoint: everything between GetWorldPos() and
// KeyFrame::GetFeaturesInArea in ORBmatcher::SearchByProjection(KeyFrame*, Scw, ...) (src/ORBmatcher.cc:316-357),
// Fuse(KeyFrame*, vpMapPoints, th) (:833-873), Fuse(KeyFrame*, Scw, ...) (:973-1015) and both directions of SearchBySim3
// (:1122-1155, :1202-1235).  The host has computed every matrix once per call; what differs between the four is chosen by
// the three switches of OrbfeKeyFrameProjection.
__global__ __launch_bounds__(kProjThreads) void k_project_keyframe(KfParams P) {
  __shared__ int firstBad;
  if (threadIdx.x == 0) firstBad = INT_MAX;
  __syncthreads();
  const int i = blockIdx.x * kProjThreads + threadIdx.x;
  bool valid = false;
  float u = 0.f, v = 0.f, radius = 0.f;
  int lvl = 0, row = 0;
  if (i < P.n) {
    const unsigned fl = P.flags[i];
    row = P.rows[i];
    if (!(fl & (ORBFE_MP_BAD | ORBFE_MP_SKIP))) {          // isBad() / spAlreadyFound, IsInKeyFrame, vbAlreadyMatched, no MapPoint
      const float4* R = reinterpret_cast<const float4*>(P.table + (size_t)row * kRowBytes);
      const float4 a = R[0], b = R[1];
      const float Pw[3] = {a.x, a.y, a.z};                  // GetWorldPos()
      const float Pn[3] = {a.w, b.x, b.y};                  // GetNormal()
      const float minRaw = b.z, maxRaw = b.w;               // mfMinDistance, mfMaxDistance
      const OrbfeKeyFrameProjection& C = P.proj;
      // p3Dc = Rcw*p3Dw+tcw: gemm, float dot in source order, double epilogue (alpha = beta = 1)
      float p[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float t = C.R[3 * k] * Pw[0] + C.R[3 * k + 1] * Pw[1] + C.R[3 * k + 2] * Pw[2];
        p[k] = (float)((double)t * 1.0 + (double)C.t[k] * 1.0);
      }
      if (C.has_second) {                                   // p3Dc2 = sR21*p3Dc1+t21 (:1124) / p3Dc1 = sR12*p3Dc2+t12 (:1204)
        float q[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const float t = C.sR[3 * k] * p[0] + C.sR[3 * k + 1] * p[1] + C.sR[3 * k + 2] * p[2];
          q[k] = (float)((double)t * 1.0 + (double)C.t2[k] * 1.0);
        }
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
      }
      if (!(p[2] < 0.0f)) {                                 // depth must be positive
        // :326 / :840 `1/p3Dc.at<float>(2)` is a float division; :983 / :1130 / :1210 `1.0/...` a double one, rounded to float
        const float invz = C.invz_in_double ? (float)(1.0 / (double)p[2]) : 1.0f / p[2];
        const float x = p[0] * invz;
        const float y = p[1] * invz;
        u = C.fx * x + C.cx;
        v = C.fy * y + C.cy;
        // KeyFrame::IsInImage (src/KeyFrame.cc:678-681), half-open; a NaN or infinite u, v (z = +-0) fails it by itself
        if (u >= P.minX && u < P.maxX && v >= P.minY && v < P.maxY) {
          const float maxDistance = 1.2f * maxRaw;          // GetMaxDistanceInvariance (MapPoint.cc:364-368)
          const float minDistance = 0.8f * minRaw;          // GetMinDistanceInvariance (MapPoint.cc:358-362)
          float PO[3];
          if (C.distance_from_camera_point) { PO[0] = p[0]; PO[1] = p[1]; PO[2] = p[2]; }   // cv::norm(p3Dc2) (:1143, :1223)
          else { PO[0] = Pw[0] - C.Ow[0]; PO[1] = Pw[1] - C.Ow[1]; PO[2] = Pw[2] - C.Ow[2]; }   // PO = p3Dw-Ow
          double s = 0.0;                                   // cv::norm(PO)
#pragma unroll
          for (int k = 0; k < 3; k++) s += (double)PO[k] * (double)PO[k];
          const float dist3D = (float)sqrt(s);
          if (!(dist3D < minDistance || dist3D > maxDistance)) {
            bool angleOk = true;
            if (C.check_viewing_angle) {                    // PO.dot(Pn)<0.5*dist (:349, :865, :1006)
              double d = 0.0;
#pragma unroll
              for (int k = 0; k < 3; k++) d += (double)PO[k] * (double)Pn[k];
              angleOk = !(d < 0.5 * (double)dist3D);
            }
            if (angleOk) {
              // PredictScale (MapPoint.cc:370-379), converted to int as the host does (an out-of-range value becomes INT_MIN)
              const float ratio = maxRaw / dist3D;
              const float c = ceilf(orbfe::logf_glibc(ratio) / C.logScaleFactor);
              lvl = (c >= -2147483648.0f && c < 2147483648.0f) ? (int)c : INT_MIN;
              valid = true;
            }
          }
        }
      }
    }
    const bool levelOk = lvl >= 0 && lvl < P.nlevels;
    if (!valid) { u = 0.f; v = 0.f; lvl = 0; }
    else if (levelOk) radius = P.th * P.sf[lvl];            // th*pKF->mvScaleFactors[nPredictedLevel]
    if (P.valid) P.valid[i] = valid ? 1 : 0;
    if (P.uv) { P.uv[2 * i] = u; P.uv[2 * i + 1] = v; }
    if (P.level) P.level[i] = lvl;
    if (P.radius) P.radius[i] = radius;
    if (P.dxy) {
      // the search reads these: a level outside [0, nlevels) is never handed to it (the call fails instead)
      if (valid && !levelOk) atomicMin(&firstBad, i);
      reinterpret_cast<float2*>(P.dxy)[i] = make_float2(u, v);
      P.dlevel[i] = valid && levelOk ? lvl : 0;
      P.dradius[i] = radius;
      P.dvalid[i] = valid && levelOk ? 1 : 0;
      P.drow[i] = valid ? 2 * row : 0;    // descriptor = 32-byte row 2*row of (table + 32)
    }
  }
  const int count = __syncthreads_count(valid ? 1 : 0);
  if (threadIdx.x == 0) {
    P.blockInfo[2 * blockIdx.x] = count;
    P.blockInfo[2 * blockIdx.x + 1] = firstBad == INT_MAX ? -1 : firstBad;
    __threadfence_system();
  }
}

__global__ void k_debug_logf(const float* __restrict__ x, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = orbfe::logf_glibc(x[i]);
}

// > 0: page-locked host memory (read by the kernel in place); 0: ordinary host memory; -1: device memory
int host_readable(const void* p) {
  hipPointerAttribute_t attr;
  if (p && hipPointerGetAttributes(&attr, p) == hipSuccess) {
    if (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeManaged) return 1;
    if (attr.type == hipMemoryTypeDevice) return -1;
    return 0;
  }
  (void)hipGetLastError();
  return 0;
}

}  // namespace

struct orbfe_local_map {
  orbfe_matcher* m = nullptr;
  int capacity = 0;
  DevBuf<uint8_t> table;
  PinBuf<uint8_t> stage;           // set_rows records, read by k_local_map_scatter in place
  hipEvent_t staged = nullptr;     // recorded after the last scatter: the staging is free again once it has completed
  PinBuf<uint8_t> io;              // per call: copies of ordinary rows / flags arrays, outputs, per-block summary
  DevBuf<uint8_t> q;               // fused call: the search's queries
  std::vector<uint8_t> seen;       // set_rows duplicate check
  std::shared_ptr<void> refresh;   // scratch of orbfe_local_map_refresh_rows (orbfe_mprefresh.hip); released after the body below
  ~orbfe_local_map() {
    (void)hipSetDevice(m->device);
    if (staged) { (void)hipEventSynchronize(staged); (void)hipEventDestroy(staged); }
    table.release(); stage.release(); io.release(); q.release();
    (void)hipGetLastError();
  }
};

namespace orbfe {
// what orbfe_mprefresh.hip needs of a table: its matcher, size, rows, and the slot of its own scratch
struct LocalMapView {
  orbfe_matcher* m;
  int capacity;
  uint8_t* table;
  std::shared_ptr<void>* scratch;
};
void local_map_view(orbfe_local_map* map, LocalMapView* v) {
  v->m = map->m; v->capacity = map->capacity; v->table = map->table.p; v->scratch = &map->refresh;
}
}  // namespace orbfe

namespace {

struct CallArea {
  const int32_t* rows;
  const uint8_t* flags;
  uint8_t* inView;
  float* xy;
  int32_t* level;
  float* vcos;
  int* blockInfo;
  int blocks;
};

// checks shared by both calls; carves the page-locked area (caller's rows / flags read in place when page-locked)
int prepare(orbfe_matcher* m, orbfe_frame* f, orbfe_local_map* map, const void* cam, const int32_t* rows, const uint8_t* flags,
            int n_mp, CallArea* A) {
  if (!m || !f || !map || !cam || n_mp < 0 || (n_mp && (!rows || !flags))) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  if (map->m != m) { set_err("the local map belongs to another matcher (its uploads are ordered on that matcher's stream)"); return ORBFE_ERR_INVALID; }
  if (orbfe_frame_device(f) != m->device) { set_err("frame and matcher live on different devices"); return ORBFE_ERR_INVALID; }
  HIP_TRY(hipSetDevice(m->device));
  (void)hipGetLastError();
  const int wr = host_readable(rows), wf = host_readable(flags);
  if (n_mp && (wr < 0 || wf < 0)) { set_err("rows and flags must be host memory"); return ORBFE_ERR_INVALID; }
  // a row is an address: one branch-free sweep, and only if it finds a row outside the table a second one over the MapPoints
  // that are projected (skipped and bad ones may carry anything)
  unsigned hi = 0;
  for (int i = 0; i < n_mp; i++) hi = std::max(hi, (unsigned)rows[i]);
  if (hi >= (unsigned)map->capacity)
    for (int i = 0; i < n_mp; i++)
      if (!(flags[i] & (ORBFE_MP_BAD | ORBFE_MP_SKIP)) && (unsigned)rows[i] >= (unsigned)map->capacity) {
        set_err("MapPoint %d: row %d outside the local map (%d rows)", i, rows[i], map->capacity);
        return ORBFE_ERR_INVALID;
      }
  const size_t c = (size_t)std::max(n_mp, 1);
  A->blocks = (n_mp + kProjThreads - 1) / kProjThreads;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += al(bytes); return at; };
  const size_t oR = take(4 * c), oF = take(c), oI = take(c), oX = take(8 * c), oL = take(4 * c), oV = take(4 * c),
               oB = take(8 * (size_t)std::max(A->blocks, 1));
  int rc;
  if ((rc = map->io.ensure(o))) return rc;
  uint8_t* H = map->io.p;
  A->rows = rows; A->flags = flags;
  if (n_mp && wr == 0) { memcpy(H + oR, rows, 4 * (size_t)n_mp); A->rows = (const int32_t*)(H + oR); }
  if (n_mp && wf == 0) { memcpy(H + oF, flags, (size_t)n_mp); A->flags = H + oF; }
  A->inView = H + oI; A->xy = (float*)(H + oX); A->level = (int32_t*)(H + oL); A->vcos = (float*)(H + oV);
  A->blockInfo = (int*)(H + oB);
  return ORBFE_OK;
}

ProjParams params(orbfe_frame* f, orbfe_local_map* map, const OrbfeCamera* cam, float cosLimit, int n_mp, const CallArea& A) {
  ProjParams P{};
  P.table = map->table.p;
  P.rows = A.rows; P.flags = A.flags; P.n = n_mp;
  P.cam = *cam;
  float b[4];
  orbfe::frame_bounds(f, b);
  P.minX = b[0]; P.maxX = b[1]; P.minY = b[2]; P.maxY = b[3];
  P.cosLimit = cosLimit;
  P.blockInfo = A.blockInfo;
  return P;
}

// after the stream has passed the kernel: MapPoints in view, first MapPoint whose level is outside the search's range
void summary(const CallArea& A, int* nInView, int* firstBad) {
  std::atomic_thread_fence(std::memory_order_acquire);
  const volatile int* B = A.blockInfo;
  int cnt = 0, bad = -1;
  for (int b = 0; b < A.blocks; b++) {
    cnt += B[2 * b];
    if (bad < 0 && B[2 * b + 1] >= 0) bad = B[2 * b + 1];
  }
  *nInView = cnt;
  *firstBad = bad;
}

void copy_out(const CallArea& A, int n_mp, uint8_t* in_view, float* proj_xy, int32_t* level, float* view_cos) {
  if (in_view) memcpy(in_view, A.inView, (size_t)n_mp);
  if (proj_xy) memcpy(proj_xy, A.xy, 8 * (size_t)n_mp);
  if (level) memcpy(level, A.level, 4 * (size_t)n_mp);
  if (view_cos) memcpy(view_cos, A.vcos, 4 * (size_t)n_mp);
}

}  // namespace

namespace {

// checks shared by the two source-projection calls, then prepare()'s
int prepare_sources(orbfe_matcher* m, orbfe_frame* cur, orbfe_frame* src, orbfe_local_map* map, const OrbfeCamera* cam, int mode,
                    const int32_t* rows, const uint8_t* flags, int n_src, CallArea* A) {
  if (!cur || !src) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  if (mode != ORBFE_SRC_LAST_FRAME && mode != ORBFE_SRC_KEYFRAME) { set_err("mode must be ORBFE_SRC_LAST_FRAME or ORBFE_SRC_KEYFRAME"); return ORBFE_ERR_INVALID; }
  if (m && orbfe_frame_device(src) != m->device) { set_err("source frame and matcher live on different devices"); return ORBFE_ERR_INVALID; }
  if (n_src != orbfe_frame_size(src)) {
    set_err("n_src (%d) is not the source frame's size (%d): source i is its keypoint i", n_src, orbfe_frame_size(src));
    return ORBFE_ERR_INVALID;
  }
  const int rc = prepare(m, cur, map, cam, rows, flags, n_src, A);
  if (rc) return rc;
  // LAST_FRAME projects a source whatever ORBFE_MP_BAD says (prepare() let the rows of such sources pass unchecked)
  if (mode == ORBFE_SRC_LAST_FRAME)
    for (int i = 0; i < n_src; i++)
      if ((flags[i] & (ORBFE_MP_BAD | ORBFE_MP_SKIP)) == ORBFE_MP_BAD && (unsigned)rows[i] >= (unsigned)map->capacity) {
        set_err("source %d: row %d outside the local map (%d rows)", i, rows[i], map->capacity);
        return ORBFE_ERR_INVALID;
      }
  return ORBFE_OK;
}

SrcParams source_params(orbfe_frame* cur, orbfe_frame* src, orbfe_local_map* map, const OrbfeCamera* cam, int mode, int n_src,
                        const CallArea& A) {
  SrcParams P{};
  P.table = map->table.p;
  P.rows = A.rows; P.flags = A.flags; P.n = n_src;
  P.mode = mode;
  P.cam = *cam;
  float b[4];
  orbfe::frame_bounds(cur, b);
  P.minX = b[0]; P.maxX = b[1]; P.minY = b[2]; P.maxY = b[3];
  P.blockInfo = A.blockInfo;
  return P;
}

}  // namespace

namespace {

// checks shared by the two keyframe-projection calls, then prepare()'s
int prepare_keyframe(orbfe_matcher* m, orbfe_frame* kf, orbfe_local_map* map, const OrbfeKeyFrameProjection* proj, const int32_t* rows,
                     const uint8_t* flags, int n, const float* scale_factors, int nlevels, CallArea* A) {
  if (!scale_factors || nlevels < 1 || nlevels > 32) { set_err("bad argument (scale factors of 1..32 levels are required)"); return ORBFE_ERR_INVALID; }
  if (proj && proj->check_viewing_angle && proj->distance_from_camera_point) {
    set_err("the viewing-angle test reads PO = p3Dw-Ow: it needs the distance from the camera centre");
    return ORBFE_ERR_INVALID;
  }
  return prepare(m, kf, map, proj, rows, flags, n, A);
}

KfParams keyframe_params(orbfe_frame* kf, orbfe_local_map* map, const OrbfeKeyFrameProjection* proj, int n, const float* scale_factors,
                         int nlevels, float th, const CallArea& A) {
  KfParams P{};
  P.table = map->table.p;
  P.rows = A.rows; P.flags = A.flags; P.n = n;
  P.proj = *proj;
  float b[4];
  orbfe::frame_bounds(kf, b);
  P.minX = b[0]; P.maxX = b[1]; P.minY = b[2]; P.maxY = b[3];
  P.nlevels = nlevels;
  P.th = th;
  for (int l = 0; l < nlevels; l++) P.sf[l] = scale_factors[l];
  P.blockInfo = A.blockInfo;
  return P;
}

}  // namespace

extern "C" {

int orbfe_local_map_create(orbfe_matcher* m, int capacity, orbfe_local_map** out) {
  if (!m || !out || capacity <= 0 || capacity > (1 << 26)) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  *out = nullptr;
  HIP_TRY(hipSetDevice(m->device));
  orbfe_local_map* map = new orbfe_local_map();
  map->m = m;
  map->capacity = capacity;
  int rc = map->table.ensure((size_t)capacity * kRowBytes);
  if (!rc && hipMemsetAsync(map->table.p, 0, (size_t)capacity * kRowBytes, m->stream) != hipSuccess) {
    set_err("hipMemsetAsync failed");
    rc = ORBFE_ERR_HIP;
  }
  if (!rc && hipEventCreateWithFlags(&map->staged, hipEventDisableTiming) != hipSuccess) {
    set_err("hipEventCreate failed");
    rc = ORBFE_ERR_HIP;
  }
  if (rc) { delete map; return rc; }
  *out = map;
  return ORBFE_OK;
}

void orbfe_local_map_destroy(orbfe_local_map* map) { delete map; }

int orbfe_local_map_capacity(const orbfe_local_map* map) { return map ? map->capacity : 0; }

int orbfe_local_map_set_rows(orbfe_local_map* map, int n, const int32_t* rows, const float* pos, const float* normal,
                             const float* min_raw, const float* max_raw, const uint8_t* desc) {
  if (!map || n < 0 || (n && !rows)) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  if (n == 0) return ORBFE_OK;
  map->seen.assign((size_t)map->capacity, 0);
  for (int i = 0; i < n; i++) {
    if (rows[i] < 0 || rows[i] >= map->capacity) { set_err("row %d outside the local map (%d rows)", rows[i], map->capacity); return ORBFE_ERR_INVALID; }
    if (map->seen[rows[i]]) { set_err("row %d named twice", rows[i]); return ORBFE_ERR_INVALID; }
    map->seen[rows[i]] = 1;
  }
  orbfe_matcher* m = map->m;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipEventSynchronize(map->staged));   // the previous upload has read its records
  int rc;
  if ((rc = map->stage.ensure((size_t)n * kStageBytes))) return rc;
  const unsigned mask = (pos ? 1u : 0u) | (normal ? 2u : 0u) | (min_raw ? 4u : 0u) | (max_raw ? 8u : 0u) | (desc ? 16u : 0u);
  for (int i = 0; i < n; i++) {
    uint8_t* rec = map->stage.p + (size_t)i * kStageBytes;
    int32_t* hdr = reinterpret_cast<int32_t*>(rec);
    hdr[0] = rows[i];
    hdr[1] = (int32_t)mask;
    float* r = reinterpret_cast<float*>(rec + 16);
    if (pos) memcpy(r, pos + 3 * (size_t)i, 12);
    if (normal) memcpy(r + 3, normal + 3 * (size_t)i, 12);
    if (min_raw) r[6] = min_raw[i];
    if (max_raw) r[7] = max_raw[i];
    if (desc) memcpy(rec + 48, desc + 32 * (size_t)i, 32);
  }
  hipLaunchKernelGGL(k_local_map_scatter, dim3((n + 255) / 256), dim3(256), 0, m->stream, (const uint8_t*)map->stage.p, n, map->table.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(map->staged, m->stream));
  return ORBFE_OK;
}

int orbfe_project_local_map(orbfe_matcher* m, orbfe_frame* f, orbfe_local_map* map, const OrbfeCamera* cam,
                            float view_cos_limit, const int32_t* rows, const uint8_t* flags, int n_mp, uint8_t* in_view,
                            float* proj_xy, int32_t* level, float* view_cos, int* n_in_view) {
  CallArea A;
  int rc = prepare(m, f, map, cam, rows, flags, n_mp, &A);
  if (rc) return rc;
  if (n_in_view) *n_in_view = 0;
  if (n_mp == 0) return ORBFE_OK;
  ProjParams P = params(f, map, cam, view_cos_limit, n_mp, A);
  P.inView = A.inView; P.xy = A.xy; P.level = A.level; P.vcos = A.vcos;
  hipLaunchKernelGGL(k_project_local_map, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(m->stream));
  int cnt = 0, bad = -1;
  summary(A, &cnt, &bad);
  copy_out(A, n_mp, in_view, proj_xy, level, view_cos);
  if (n_in_view) *n_in_view = cnt;
  return ORBFE_OK;
}

int orbfe_search_local_points_frame(orbfe_matcher* m, orbfe_frame* f, orbfe_local_map* map, const OrbfeCamera* cam,
                                    float view_cos_limit, const int32_t* rows, const uint8_t* flags, int n_mp,
                                    const float* scale_factors, int nlevels, const uint8_t* kp_occupied, float th, float nnratio,
                                    uint8_t* in_view, float* proj_xy, int32_t* level, float* view_cos, int32_t* kp_assigned,
                                    int* nmatches, int* n_in_view) {
  if (!nmatches || !n_in_view || !scale_factors || nlevels < 1 || nlevels > 32) {
    set_err("bad argument (scale factors of 1..32 levels, nmatches and n_in_view are required)");
    return ORBFE_ERR_INVALID;
  }
  CallArea A;
  int rc = prepare(m, f, map, cam, rows, flags, n_mp, &A);
  if (rc) return rc;
  const int n = orbfe_frame_size(f);
  if (n && (!kp_occupied || !kp_assigned)) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  *nmatches = 0;
  *n_in_view = 0;
  if (n_mp == 0) {
    for (int i = 0; i < n; i++) kp_assigned[i] = -1;
    return ORBFE_OK;
  }
  const size_t c = (size_t)n_mp;
  const size_t oXY = 0, oL = al(8 * c), oV = oL + al(4 * c), oF = oV + al(4 * c), oR = oF + al(c), total = oR + al(4 * c);
  if ((rc = map->q.ensure(total))) return rc;
  uint8_t* D = map->q.p;
  ProjParams P = params(f, map, cam, view_cos_limit, n_mp, A);
  if (in_view) P.inView = A.inView;
  if (proj_xy) P.xy = A.xy;
  if (level) P.level = A.level;
  if (view_cos) P.vcos = A.vcos;
  P.nlevels = nlevels;
  P.dxy = (float*)(D + oXY); P.dlevel = (int32_t*)(D + oL); P.dvcos = (float*)(D + oV); P.dflags = D + oF; P.drow = (int32_t*)(D + oR);
  hipLaunchKernelGGL(k_project_local_map, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P);
  HIP_TRY(hipGetLastError());
  // the window search and the bookkeeping follow on the same stream; the search returns when its result is back
  if ((rc = orbfe::sbp_frame_device_queries(m, f, scale_factors, nlevels, kp_occupied, P.dxy, P.dlevel, P.dvcos, P.dflags,
                                            map->table.p + 32, P.drow, n_mp, th, nnratio, kp_assigned, nmatches))) {
    (void)hipStreamSynchronize(m->stream);
    return rc;
  }
  if (n == 0) HIP_TRY(hipStreamSynchronize(m->stream));   // (no search was submitted: wait for the projection alone)
  int cnt = 0, bad = -1;
  summary(A, &cnt, &bad);
  *n_in_view = cnt;
  copy_out(A, n_mp, in_view, proj_xy, level, view_cos);
  if (bad >= 0) {
    *nmatches = 0;
    set_err("MapPoint %d: predicted level outside [0, %d)", bad, nlevels);
    return ORBFE_ERR_INVALID;
  }
  return ORBFE_OK;
}

int orbfe_project_sources(orbfe_matcher* m, orbfe_frame* cur_frame, orbfe_frame* src_frame, orbfe_local_map* map,
                          const OrbfeCamera* cam, int mode, const int32_t* rows, const uint8_t* flags, int n_src, uint8_t* valid,
                          float* uv, int32_t* level, int* n_valid) {
  CallArea A;
  int rc = prepare_sources(m, cur_frame, src_frame, map, cam, mode, rows, flags, n_src, &A);
  if (rc) return rc;
  if (n_valid) *n_valid = 0;
  if (n_src == 0) return ORBFE_OK;
  SrcParams P = source_params(cur_frame, src_frame, map, cam, mode, n_src, A);
  const float* srcAngle = nullptr;
  int maxOctave = 0;
  orbfe::frame_source_arrays(src_frame, &P.srcOct, &srcAngle, &maxOctave);
  P.valid = A.inView; P.uv = A.xy; P.level = A.level;
  orbfe::frame_wait_ready(src_frame, m->stream);
  hipLaunchKernelGGL(k_project_sources, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(m->stream));
  int cnt = 0, bad = -1;
  summary(A, &cnt, &bad);
  copy_out(A, n_src, valid, uv, level, nullptr);
  if (n_valid) *n_valid = cnt;
  return ORBFE_OK;
}

int orbfe_search_by_projection_sources_frame(orbfe_matcher* m, orbfe_frame* cur_frame, orbfe_frame* src_frame,
                                             orbfe_local_map* map, const OrbfeCamera* cam, int mode, const int32_t* rows,
                                             const uint8_t* flags, int n_src, const float* scale_factors, int nlevels,
                                             const uint8_t* kp_occupied, float th, int max_dist, int check_orientation,
                                             uint8_t* valid, float* uv, int32_t* level, int32_t* kp_assigned, int* nmatches,
                                             int* n_valid) {
  if (!nmatches || !n_valid || !scale_factors || nlevels < 1 || nlevels > 32) {
    set_err("bad argument (scale factors of 1..32 levels, nmatches and n_valid are required)");
    return ORBFE_ERR_INVALID;
  }
  CallArea A;
  int rc = prepare_sources(m, cur_frame, src_frame, map, cam, mode, rows, flags, n_src, &A);
  if (rc) return rc;
  const int n = orbfe_frame_size(cur_frame);
  if (n && (!kp_occupied || !kp_assigned)) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  *nmatches = 0;
  *n_valid = 0;
  if (n_src == 0) {
    for (int i = 0; i < n; i++) kp_assigned[i] = -1;
    return ORBFE_OK;
  }
  SrcParams P = source_params(cur_frame, src_frame, map, cam, mode, n_src, A);
  const float* srcAngle = nullptr;
  int maxOctave = 0;
  orbfe::frame_source_arrays(src_frame, &P.srcOct, &srcAngle, &maxOctave);
  // nLastOctave indexes mvScaleFactors (:1347): refused up front from the source frame's largest octave
  if (mode == ORBFE_SRC_LAST_FRAME && maxOctave >= nlevels) {
    set_err("the source frame holds a keypoint of octave %d: outside [0, %d)", maxOctave, nlevels);
    return ORBFE_ERR_INVALID;
  }
  const size_t c = (size_t)n_src;
  const size_t oXY = 0, oL = al(8 * c), oR = oL + al(4 * c), oV = oR + al(4 * c), oC = oV + al(c), total = oC + al(c);
  if ((rc = map->q.ensure(total))) return rc;
  uint8_t* D = map->q.p;
  if (valid) P.valid = A.inView;
  if (uv) P.uv = A.xy;
  if (level) P.level = A.level;
  P.nlevels = nlevels;
  P.dxy = (float*)(D + oXY); P.dlevel = (int32_t*)(D + oL); P.drow = (int32_t*)(D + oR); P.dvalid = D + oV; P.dclaim = D + oC;
  orbfe::frame_wait_ready(src_frame, m->stream);
  hipLaunchKernelGGL(k_project_sources, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P);
  HIP_TRY(hipGetLastError());
  // the window search and the bookkeeping follow on the same stream; the search returns when its result is back
  if ((rc = orbfe::sbp_uv_frame_device_queries(m, cur_frame, scale_factors, nlevels, kp_occupied, P.dxy, P.dlevel, srcAngle, P.dvalid,
                                               P.dclaim, map->table.p + 32, P.drow, n_src, th, max_dist,
                                               mode == ORBFE_SRC_KEYFRAME ? 1 : 0, check_orientation, kp_assigned, nmatches))) {
    (void)hipStreamSynchronize(m->stream);
    return rc;
  }
  if (n == 0) HIP_TRY(hipStreamSynchronize(m->stream));   // (no search was submitted: wait for the projection alone)
  int cnt = 0, bad = -1;
  summary(A, &cnt, &bad);
  *n_valid = cnt;
  copy_out(A, n_src, valid, uv, level, nullptr);
  if (bad >= 0) {
    *nmatches = 0;
    set_err("source %d: predicted level outside [0, %d)", bad, nlevels);
    return ORBFE_ERR_INVALID;
  }
  return ORBFE_OK;
}

int orbfe_project_keyframe(orbfe_matcher* m, orbfe_frame* kf_frame, orbfe_local_map* map, const OrbfeKeyFrameProjection* proj,
                           const int32_t* rows, const uint8_t* flags, int n, const float* scale_factors, int nlevels, float th,
                           uint8_t* valid, float* uv, int32_t* level, float* radius, int* n_valid) {
  CallArea A;
  int rc = prepare_keyframe(m, kf_frame, map, proj, rows, flags, n, scale_factors, nlevels, &A);
  if (rc) return rc;
  if (n_valid) *n_valid = 0;
  if (n == 0) return ORBFE_OK;
  KfParams P = keyframe_params(kf_frame, map, proj, n, scale_factors, nlevels, th, A);
  P.valid = A.inView; P.uv = A.xy; P.level = A.level; P.radius = A.vcos;
  hipLaunchKernelGGL(k_project_keyframe, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(m->stream));
  int cnt = 0, bad = -1;
  summary(A, &cnt, &bad);
  copy_out(A, n, valid, uv, level, radius);
  if (n_valid) *n_valid = cnt;
  return ORBFE_OK;
}

int orbfe_search_projected_keyframe_frame(orbfe_matcher* m, orbfe_frame* kf_frame, orbfe_local_map* map,
                                          const OrbfeKeyFrameProjection* proj, const int32_t* rows, const uint8_t* flags, int n,
                                          const float* scale_factors, int nlevels, float th, const uint8_t* kp_skip, int claim,
                                          const float* inv_level_sigma2, double chi2, int max_dist, uint8_t* valid, float* uv,
                                          int32_t* level, int32_t* best_idx, int32_t* best_dist, int* nmatches, int* n_valid) {
  if (!nmatches || !n_valid || (n > 0 && !best_idx)) { set_err("bad argument (best_idx, nmatches and n_valid are required)"); return ORBFE_ERR_INVALID; }
  CallArea A;
  int rc = prepare_keyframe(m, kf_frame, map, proj, rows, flags, n, scale_factors, nlevels, &A);
  if (rc) return rc;
  const int nkp = orbfe_frame_size(kf_frame);
  *nmatches = 0;
  *n_valid = 0;
  for (int i = 0; i < n; i++) {
    best_idx[i] = -1;
    if (best_dist) best_dist[i] = -1;
  }
  if (n == 0) return ORBFE_OK;
  const size_t c = (size_t)n;
  const size_t oXY = 0, oL = al(8 * c), oR = oL + al(4 * c), oA = oR + al(4 * c), oV = oA + al(4 * c), total = oV + al(c);
  if ((rc = map->q.ensure(total))) return rc;
  uint8_t* D = map->q.p;
  KfParams P = keyframe_params(kf_frame, map, proj, n, scale_factors, nlevels, th, A);
  if (valid) P.valid = A.inView;
  if (uv) P.uv = A.xy;
  if (level) P.level = A.level;
  P.dxy = (float*)(D + oXY); P.dlevel = (int32_t*)(D + oL); P.drow = (int32_t*)(D + oR); P.dradius = (float*)(D + oA); P.dvalid = D + oV;
  hipLaunchKernelGGL(k_project_keyframe, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P);
  HIP_TRY(hipGetLastError());
  // the window search and the bookkeeping follow on the same stream; the search returns when its result is back
  if ((rc = orbfe::search_projected_frame_device_queries(m, kf_frame, scale_factors, nlevels, th, P.dxy, P.dlevel, P.dradius, P.dvalid,
                                                         map->table.p + 32, P.drow, n, kp_skip, claim, inv_level_sigma2, chi2,
                                                         max_dist, best_idx, best_dist, nmatches))) {
    (void)hipStreamSynchronize(m->stream);
    return rc;
  }
  if (nkp == 0) HIP_TRY(hipStreamSynchronize(m->stream));   // (no search was submitted: wait for the projection alone)
  int cnt = 0, bad = -1;
  summary(A, &cnt, &bad);
  *n_valid = cnt;
  copy_out(A, n, valid, uv, level, nullptr);
  if (bad >= 0) {
    *nmatches = 0;
    set_err("MapPoint %d: predicted level outside [0, %d)", bad, nlevels);
    return ORBFE_ERR_INVALID;
  }
  return ORBFE_OK;
}

int orbfe_debug_logf(orbfe_matcher* m, const float* x, int n, float* out) {
  if (!m || n < 0 || (n && (!x || !out))) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  if (n == 0) return ORBFE_OK;
  HIP_TRY(hipSetDevice(m->device));
  float* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 2 * sizeof(float) * (size_t)n));
  hipError_t e = hipMemcpyAsync(d, x, sizeof(float) * n, hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_logf, dim3((n + 255) / 256), dim3(256), 0, m->stream, (const float*)d, n, d + n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d + n, sizeof(float) * n, hipMemcpyDeviceToHost, m->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  (void)hipFree(d);
  HIP_TRY(e);
  return ORBFE_OK;
}

int orbfe_debug_logf_host_check(uint32_t lo_bits, uint32_t hi_bits, uint32_t step, long long* mismatches) {
  if (!mismatches || step == 0) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  long long bad = 0;
  for (uint64_t u = lo_bits; u <= hi_bits; u += step) {
    const uint32_t b = (uint32_t)u;
    float f;
    memcpy(&f, &b, 4);
    volatile float vf = f;
    const float r = orbfe::logf_glibc(f), r0 = logf(vf);
    if (memcmp(&r, &r0, 4) && !(r != r && r0 != r0)) bad++;   // (NaN results compare as equal whatever their payload)
  }
  *mismatches = bad;
  return ORBFE_OK;
}

}  // extern "C"
