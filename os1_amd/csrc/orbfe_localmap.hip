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
// One projection core, three kernels.  The arithmetic is the reference's cv::Mat float arithmetic as the oracle pins it
// (oracle/orb_oracle.cpp cvGemm3, cvNorm3, cvDot3, predictScale; include/orbfe/orb_shim.hpp RestatedOps), and every piece of
// it is stated ONCE below: load_row, transform3 (Rcw*P+tcw as cv::gemm computes it), norm3 and dot3 (cv::norm, Mat::dot: double
// accumulation), distance_in_range (the 0.8f / 1.2f invariance), predict_level (PredictScale: glibc logf, glibc_logf.h).  So is
// the framing every kernel shares: ProjCommon, block_begin, write_common (host outputs, the search's common query fields, the
// level rule) and block_summary.  A kernel keeps what is its own: the culling order of its reference loop, its bounds test,
// its 1/z, its extra outputs.  The library is built with -ffp-contract=off, so every float operation rounds on its own as in
// the reference; the order of operations and the operand types of these expressions are the correctness contract of this file.
#include "orbfe_matcher_internal.h"
#include "glibc_logf.h"

#include <atomic>

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
// ---- the projection core ---------------------------------------------------------------------------------------------
struct Row {
  float pos[3];      // GetWorldPos()
  float normal[3];   // GetNormal()
  float minRaw, maxRaw;   // mfMinDistance, mfMaxDistance
};
__device__ __forceinline__ Row load_row(const uint8_t* __restrict__ table, int row) {
  const float4* R = reinterpret_cast<const float4*>(table + (size_t)row * kRowBytes);
  const float4 a = R[0], b = R[1];
  return Row{{a.x, a.y, a.z}, {a.w, b.x, b.y}, b.z, b.w};
}
// out = R*P+t as cv::gemm computes it: float dot in source order, double epilogue (alpha = beta = 1).  out must not alias P.
__device__ __forceinline__ void transform3(const float R[9], const float t[3], const float P[3], float out[3]) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float d = R[3 * k] * P[0] + R[3 * k + 1] * P[1] + R[3 * k + 2] * P[2];
    out[k] = (float)((double)d * 1.0 + (double)t[k] * 1.0);
  }
}
// (float)cv::norm(v): double accumulation in index order
__device__ __forceinline__ float norm3(const float v[3]) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
  return (float)sqrt(s);
}
// a.dot(b): double accumulation in index order; the caller rounds or compares
__device__ __forceinline__ double dot3(const float a[3], const float b[3]) {
  double d = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) d += (double)a[k] * (double)b[k];
  return d;
}
// !(dist < GetMinDistanceInvariance() || dist > GetMaxDistanceInvariance())  (MapPoint.cc:358-368)
__device__ __forceinline__ bool distance_in_range(float dist, float minRaw, float maxRaw) {
  const float maxDistance = 1.2f * maxRaw;
  const float minDistance = 0.8f * minRaw;
  return !(dist < minDistance || dist > maxDistance);
}
// PredictScale (MapPoint.cc:370-379): ceil(log(ratio)/logScaleFactor) with float ratio, converted to int as the host does (an
// out-of-range value becomes INT_MIN)
__device__ __forceinline__ int predict_level(float maxRaw, float dist, float logScaleFactor) {
  const float ratio = maxRaw / dist;
  const float c = ceilf(orbfe::logf_glibc(ratio) / logScaleFactor);
  return (c >= -2147483648.0f && c < 2147483648.0f) ? (int)c : INT_MIN;
}

// what the three kernels' parameter blocks have in common
struct ProjCommon {
  const uint8_t* table;
  const int32_t* rows;         // [n] (page-locked host memory)
  const uint8_t* flags;        // [n]
  int n;
  float minX, maxX, minY, maxY;   // bounds of the frame projected INTO
  int nlevels;                 // fused call: levels outside [0, nlevels) are taken out of the search and reported
  // outputs in page-locked host memory (any may be null)
  uint8_t* valid;
  float* xy;
  int32_t* level;
  // fused call: the search's queries in device memory (null: projection only)
  float* dxy;
  int32_t* dlevel;
  int32_t* drow;
  int* blockInfo;              // [2 * blocks] page-locked: items valid, first valid item with an out-of-range level (-1)
};

// Every lane of the block calls block_begin and block_summary (lanes with i >= n too): both hold a barrier.
__device__ __forceinline__ void block_begin(int* firstBad) {
  if (threadIdx.x == 0) *firstBad = INT_MAX;
  __syncthreads();
}
// Item i after the kernel's own tests: the common host outputs and the search's common query fields (an item that is not
// valid is written as zeros).  Returns whether the search may use the item: a level outside [0, nlevels) is never handed to
// it (the call fails instead, naming the first such item).
__device__ __forceinline__ bool write_common(const ProjCommon& P, int i, bool valid, float u, float v, int lvl, int row, int* firstBad) {
  if (!valid) { u = 0.f; v = 0.f; lvl = 0; }
  if (P.valid) P.valid[i] = valid ? 1 : 0;
  if (P.xy) { P.xy[2 * i] = u; P.xy[2 * i + 1] = v; }
  if (P.level) P.level[i] = lvl;
  const bool levelOk = lvl >= 0 && lvl < P.nlevels;
  if (P.dxy) {
    if (valid && !levelOk) atomicMin(firstBad, i);
    reinterpret_cast<float2*>(P.dxy)[i] = make_float2(u, v);
    P.dlevel[i] = levelOk ? lvl : 0;
    P.drow[i] = valid ? 2 * row : 0;      // descriptor = 32-byte row 2*row of (table + 32)
  }
  return valid && levelOk;
}
__device__ __forceinline__ void block_summary(const ProjCommon& P, bool valid, const int* firstBad) {
  const int count = __syncthreads_count(valid ? 1 : 0);
  if (threadIdx.x == 0) {
    P.blockInfo[2 * blockIdx.x] = count;
    P.blockInfo[2 * blockIdx.x + 1] = *firstBad == INT_MAX ? -1 : *firstBad;
    __threadfence_system();
  }
}

struct ProjParams {
  ProjCommon c;
  OrbfeCamera cam;
  float cosLimit;
  float* vcos;                 // page-locked host output (may be null)
  float* dvcos;                // fused call
  uint8_t* dflags;
};

// bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit)  (src/Frame.cc:151-207), one lane per listed MapPoint
__global__ __launch_bounds__(kProjThreads) void k_project_local_map(ProjParams P) {
  __shared__ int firstBad;
  block_begin(&firstBad);
  const int i = blockIdx.x * kProjThreads + threadIdx.x;
  bool inView = false;
  if (i < P.c.n) {
    float u = 0.f, v = 0.f, viewCos = 0.f;
    int lvl = 0;
    const unsigned fl = P.c.flags[i];
    const int row = P.c.rows[i];
    // Tracking.cc:804-807: mnLastFrameSeen == mCurrentFrame.mnId, isBad()
    if (!(fl & (ORBFE_MP_BAD | ORBFE_MP_SKIP))) {
      const Row r = load_row(P.c.table, row);
      const OrbfeCamera& C = P.cam;
      float Pc[3];
      transform3(C.Rcw, C.tcw, r.pos, Pc);                  // Pc = mRcw*P+mtcw
      if (!(Pc[2] < 0.0f)) {                                // Frame.cc:166-167
        const float invz = 1.0f / Pc[2];
        u = C.fx * Pc[0] * invz + C.cx;
        v = C.fy * Pc[1] * invz + C.cy;
        if (!(u < P.c.minX || u > P.c.maxX) && !(v < P.c.minY || v > P.c.maxY)) {   // Frame.cc:173-176
          const float PO[3] = {r.pos[0] - C.Ow[0], r.pos[1] - C.Ow[1], r.pos[2] - C.Ow[2]};
          const float dist = norm3(PO);
          if (distance_in_range(dist, r.minRaw, r.maxRaw)) {   // Frame.cc:179-186
            viewCos = (float)(dot3(PO, r.normal) / (double)dist);   // PO.dot(Pn)/dist
            if (!(viewCos < P.cosLimit)) {
              lvl = predict_level(r.maxRaw, dist, C.logScaleFactor);
              inView = true;
            }
          }
        }
      }
    }
    if (!inView) viewCos = 0.f;
    const bool searched = write_common(P.c, i, inView, u, v, lvl, row, &firstBad);
    if (P.vcos) P.vcos[i] = viewCos;
    if (P.c.dxy) {
      P.dvcos[i] = viewCos;
      P.dflags[i] = (uint8_t)((searched ? ORBFE_MP_IN_VIEW : 0u) | (fl & (ORBFE_MP_CANDIDATO | ORBFE_MP_OBSERVED)));
    }
  }
  block_summary(P.c, inView, &firstBad);
}

struct SrcParams {
  ProjCommon c;                // (bounds: the CURRENT frame's)
  const int* srcOct;           // [n] the SOURCE frame's resident octaves (mvKeys[i].octave)
  int mode;                    // ORBFE_SRC_LAST_FRAME / ORBFE_SRC_KEYFRAME
  OrbfeCamera cam;
  uint8_t* dvalid;             // fused call
  uint8_t* dclaim;
};

// The projection loops of ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th)
// (src/ORBmatcher.cc:1313-1347) and (Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (:1441-1479), one lane
// per source keypoint: everything between GetWorldPos() and GetFeaturesInArea.  The source keypoint's angle (the rotation
// check, :1386 / :1515) is not touched here: the search reads it from the source frame's resident copy.
__global__ __launch_bounds__(kProjThreads) void k_project_sources(SrcParams P) {
  __shared__ int firstBad;
  block_begin(&firstBad);
  const int i = blockIdx.x * kProjThreads + threadIdx.x;
  bool valid = false;
  if (i < P.c.n) {
    float u = 0.f, v = 0.f;
    int lvl = 0;
    const unsigned fl = P.c.flags[i];
    const int row = P.c.rows[i];
    // :1318-1321 no MapPoint / mvbOutlier[i] (isBad() is not asked); :1445-1447 no MapPoint / isBad() / in sAlreadyFound
    if (!(fl & (P.mode == ORBFE_SRC_KEYFRAME ? (ORBFE_MP_BAD | ORBFE_MP_SKIP) : ORBFE_MP_SKIP))) {
      const Row r = load_row(P.c.table, row);
      const OrbfeCamera& C = P.cam;
      float Pc[3];
      transform3(C.Rcw, C.tcw, r.pos, Pc);                  // x3Dc = Rcw*x3Dw+tcw
      const float invzc = (float)(1.0 / (double)Pc[2]);     // :1329 / :1455: a DOUBLE division, rounded to float
      if (P.mode == ORBFE_SRC_KEYFRAME || !(invzc < 0)) {   // :1332-1333 (the KeyFrame form has no such test)
        u = C.fx * Pc[0] * invzc + C.cx;
        v = C.fy * Pc[1] * invzc + C.cy;
        if (!(u < P.c.minX || u > P.c.maxX) && !(v < P.c.minY || v > P.c.maxY)) {   // :1339-1342 / :1460-1463
          if (P.mode == ORBFE_SRC_KEYFRAME) {
            const float PO[3] = {r.pos[0] - C.Ow[0], r.pos[1] - C.Ow[1], r.pos[2] - C.Ow[2]};   // :1466
            const float dist3D = norm3(PO);
            if (distance_in_range(dist3D, r.minRaw, r.maxRaw)) {   // :1473-1474
              lvl = predict_level(r.maxRaw, dist3D, C.logScaleFactor);
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
    const bool searched = write_common(P.c, i, valid, u, v, lvl, row, &firstBad);
    if (P.c.dxy) {
      P.dvalid[i] = searched ? 1 : 0;
      P.dclaim[i] = (uint8_t)(fl & ORBFE_MP_OBSERVED);
    }
  }
  block_summary(P.c, valid, &firstBad);
}

struct KfParams {
  ProjCommon c;                // (bounds: the TARGET keyframe's; nlevels is set in both call forms: the radius reads it)
  OrbfeKeyFrameProjection proj;
  float th;
  float sf[32];                // the target keyframe's mvScaleFactors
  float* radius;               // page-locked host output (may be null)
  float* dradius;              // fused call
  uint8_t* dvalid;
};

// The projection loops of the keyframe-side searches, one lane per listed MapPoint: everything between GetWorldPos() and
// KeyFrame::GetFeaturesInArea in ORBmatcher::SearchByProjection(KeyFrame*, Scw, ...) (src/ORBmatcher.cc:316-357),
// Fuse(KeyFrame*, vpMapPoints, th) (:833-873), Fuse(KeyFrame*, Scw, ...) (:973-1015) and both directions of SearchBySim3
// (:1122-1155, :1202-1235).  The host has computed every matrix once per call; what differs between the four is chosen by
// the three switches of OrbfeKeyFrameProjection.
__global__ __launch_bounds__(kProjThreads) void k_project_keyframe(KfParams P) {
  __shared__ int firstBad;
  block_begin(&firstBad);
  const int i = blockIdx.x * kProjThreads + threadIdx.x;
  bool valid = false;
  if (i < P.c.n) {
    float u = 0.f, v = 0.f, radius = 0.f;
    int lvl = 0;
    const unsigned fl = P.c.flags[i];
    const int row = P.c.rows[i];
    if (!(fl & (ORBFE_MP_BAD | ORBFE_MP_SKIP))) {          // isBad() / spAlreadyFound, IsInKeyFrame, vbAlreadyMatched, no MapPoint
      const Row r = load_row(P.c.table, row);
      const OrbfeKeyFrameProjection& C = P.proj;
      float p[3];
      transform3(C.R, C.t, r.pos, p);                       // p3Dc = Rcw*p3Dw+tcw
      if (C.has_second) {                                   // p3Dc2 = sR21*p3Dc1+t21 (:1124) / p3Dc1 = sR12*p3Dc2+t12 (:1204)
        float q[3];
        transform3(C.sR, C.t2, p, q);
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
        if (u >= P.c.minX && u < P.c.maxX && v >= P.c.minY && v < P.c.maxY) {
          float PO[3];
          if (C.distance_from_camera_point) { PO[0] = p[0]; PO[1] = p[1]; PO[2] = p[2]; }   // cv::norm(p3Dc2) (:1143, :1223)
          else { PO[0] = r.pos[0] - C.Ow[0]; PO[1] = r.pos[1] - C.Ow[1]; PO[2] = r.pos[2] - C.Ow[2]; }   // PO = p3Dw-Ow
          const float dist3D = norm3(PO);
          if (distance_in_range(dist3D, r.minRaw, r.maxRaw)) {
            // PO.dot(Pn)<0.5*dist (:349, :865, :1006)
            if (!C.check_viewing_angle || !(dot3(PO, r.normal) < 0.5 * (double)dist3D)) {
              lvl = predict_level(r.maxRaw, dist3D, C.logScaleFactor);
              valid = true;
            }
          }
        }
      }
    }
    const bool searched = write_common(P.c, i, valid, u, v, lvl, row, &firstBad);
    if (searched) radius = P.th * P.sf[lvl];                // th*pKF->mvScaleFactors[nPredictedLevel]
    if (P.radius) P.radius[i] = radius;
    if (P.c.dxy) {
      P.dradius[i] = radius;
      P.dvalid[i] = searched ? 1 : 0;
    }
  }
  block_summary(P.c, valid, &firstBad);
}

__global__ void k_debug_logf(const float* __restrict__ x, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = orbfe::logf_glibc(x[i]);
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

// checks shared by all six calls; carves the page-locked area (caller's rows / flags read in place when page-locked)
int prepare(orbfe_matcher* m, orbfe_frame* f, orbfe_local_map* map, const void* cam, const int32_t* rows, const uint8_t* flags,
            int n_mp, CallArea* A) {
  if (!m || !f || !map || !cam || n_mp < 0 || (n_mp && (!rows || !flags))) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  if (map->m != m) { set_err("the local map belongs to another matcher (its uploads are ordered on that matcher's stream)"); return ORBFE_ERR_INVALID; }
  if (orbfe_frame_device(f) != m->device) { set_err("frame and matcher live on different devices"); return ORBFE_ERR_INVALID; }
  HIP_TRY(hipSetDevice(m->device));
  (void)hipGetLastError();
  // 0: ordinary host memory (copied below), 1: page-locked (read in place); anything else is some device's memory
  const int wr = orbfe::gpu_readable(rows, m->device), wf = orbfe::gpu_readable(flags, m->device);
  if (n_mp && ((unsigned)wr > 1u || (unsigned)wf > 1u)) { set_err("rows and flags must be host memory"); return ORBFE_ERR_INVALID; }
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

// the common parameter part of a call that projects n items into frame f, every host output switched on
ProjCommon common_params(orbfe_frame* f, orbfe_local_map* map, int n, const CallArea& A) {
  ProjCommon c{};
  c.table = map->table.p;
  c.rows = A.rows; c.flags = A.flags; c.n = n;
  float b[4];
  orbfe::frame_bounds(f, b);
  c.minX = b[0]; c.maxX = b[1]; c.minY = b[2]; c.maxY = b[3];
  c.valid = A.inView; c.xy = A.xy; c.level = A.level;
  c.blockInfo = A.blockInfo;
  return c;
}

// the source frame's part of a source projection: its resident octaves (and angles, largest octave), ordered behind its build
SrcParams source_params(orbfe_frame* cur, orbfe_frame* src, orbfe_local_map* map, const OrbfeCamera* cam, int mode, int n_src,
                        const CallArea& A, const float** srcAngle, int* maxOctave) {
  SrcParams P{};
  P.c = common_params(cur, map, n_src, A);
  P.mode = mode;
  P.cam = *cam;
  orbfe::frame_source_arrays(src, &P.srcOct, srcAngle, maxOctave);
  return P;
}

KfParams keyframe_params(orbfe_frame* kf, orbfe_local_map* map, const OrbfeKeyFrameProjection* proj, int n, const float* scale_factors,
                         int nlevels, float th, const CallArea& A) {
  KfParams P{};
  P.c = common_params(kf, map, n, A);
  P.c.nlevels = nlevels;
  P.proj = *proj;
  P.th = th;
  for (int l = 0; l < nlevels; l++) P.sf[l] = scale_factors[l];
  P.radius = A.vcos;
  return P;
}

// Fused call: the kernel writes only the host outputs the caller asked for, and the search's queries into map->q -- the
// common three arrays, then the kernel's own two (aBytes / bBytes per item).
int fused_params(orbfe_local_map* map, int nlevels, const void* valid, const void* xy, const void* level, ProjCommon* c, size_t aBytes,
                 void** a, size_t bBytes, void** b) {
  if (!valid) c->valid = nullptr;
  if (!xy) c->xy = nullptr;
  if (!level) c->level = nullptr;
  c->nlevels = nlevels;
  const size_t n = (size_t)c->n;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += al(bytes); return at; };
  const size_t oXY = take(8 * n), oL = take(4 * n), oR = take(4 * n), oA = take(aBytes * n), oB = take(bBytes * n);
  const int rc = map->q.ensure(o);
  if (rc) return rc;
  uint8_t* D = map->q.p;
  c->dxy = (float*)(D + oXY); c->dlevel = (int32_t*)(D + oL); c->drow = (int32_t*)(D + oR);
  *a = D + oA; *b = D + oB;
  return ORBFE_OK;
}

// after the stream has passed the kernel: items valid, first valid item whose level is outside the search's range
void summary(const CallArea& A, int* nValid, int* firstBad) {
  std::atomic_thread_fence(std::memory_order_acquire);
  const volatile int* B = A.blockInfo;
  int cnt = 0, bad = -1;
  for (int b = 0; b < A.blocks; b++) {
    cnt += B[2 * b];
    if (bad < 0 && B[2 * b + 1] >= 0) bad = B[2 * b + 1];
  }
  *nValid = cnt;
  *firstBad = bad;
}

// the caller's output arrays (any may be null); aux: viewing cosines / radii
struct Outputs {
  uint8_t* valid;
  float* xy;
  int32_t* level;
  float* aux;
};
void copy_out(const CallArea& A, int n, const Outputs& O) {
  if (O.valid) memcpy(O.valid, A.inView, (size_t)n);
  if (O.xy) memcpy(O.xy, A.xy, 8 * (size_t)n);
  if (O.level) memcpy(O.level, A.level, 4 * (size_t)n);
  if (O.aux) memcpy(O.aux, A.vcos, 4 * (size_t)n);
}

// A projection-only call after prepare(): launch, wait, count, copy out.
template <class Launch>
int run_projection(orbfe_matcher* m, const CallArea& A, int n, Launch launch, const Outputs& O, int* count) {
  if (count) *count = 0;
  if (n == 0) return ORBFE_OK;
  launch();
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(m->stream));
  int cnt = 0, bad = -1;
  summary(A, &cnt, &bad);
  copy_out(A, n, O);
  if (count) *count = cnt;
  return ORBFE_OK;
}

// A fused call once its parameters stand: the projection kernel, then the window search and the bookkeeping on the same
// stream (search() returns when its result is back; `searched` says whether it submitted anything, i.e. the frame has
// keypoints).  `what` names an item in the error text.
template <class Launch, class Search>
int run_fused(orbfe_matcher* m, const CallArea& A, int n, int nlevels, bool searched, const char* what, Launch launch, Search search,
              const Outputs& O, int* nmatches, int* count) {
  launch();
  HIP_TRY(hipGetLastError());
  const int rc = search();
  if (rc) {
    (void)hipStreamSynchronize(m->stream);
    return rc;
  }
  if (!searched) HIP_TRY(hipStreamSynchronize(m->stream));   // (no search was submitted: wait for the projection alone)
  int cnt = 0, bad = -1;
  summary(A, &cnt, &bad);
  *count = cnt;
  copy_out(A, n, O);
  if (bad >= 0) {
    *nmatches = 0;
    set_err("%s %d: predicted level outside [0, %d)", what, bad, nlevels);
    return ORBFE_ERR_INVALID;
  }
  return ORBFE_OK;
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
  const int rc = prepare(m, f, map, cam, rows, flags, n_mp, &A);
  if (rc) return rc;
  ProjParams P{};
  P.c = common_params(f, map, n_mp, A);
  P.cam = *cam; P.cosLimit = view_cos_limit; P.vcos = A.vcos;
  return run_projection(m, A, n_mp, [&] { hipLaunchKernelGGL(k_project_local_map, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P); },
                        Outputs{in_view, proj_xy, level, view_cos}, n_in_view);
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
  ProjParams P{};
  P.c = common_params(f, map, n_mp, A);
  P.cam = *cam; P.cosLimit = view_cos_limit; P.vcos = view_cos ? A.vcos : nullptr;
  if ((rc = fused_params(map, nlevels, in_view, proj_xy, level, &P.c, 4, (void**)&P.dvcos, 1, (void**)&P.dflags))) return rc;
  return run_fused(
      m, A, n_mp, nlevels, n != 0, "MapPoint",
      [&] { hipLaunchKernelGGL(k_project_local_map, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P); },
      [&] {
        return orbfe::sbp_frame_device_queries(m, f, scale_factors, nlevels, kp_occupied, P.c.dxy, P.c.dlevel, P.dvcos, P.dflags,
                                               map->table.p + 32, P.c.drow, n_mp, th, nnratio, kp_assigned, nmatches);
      },
      Outputs{in_view, proj_xy, level, view_cos}, nmatches, n_in_view);
}

int orbfe_project_sources(orbfe_matcher* m, orbfe_frame* cur_frame, orbfe_frame* src_frame, orbfe_local_map* map,
                          const OrbfeCamera* cam, int mode, const int32_t* rows, const uint8_t* flags, int n_src, uint8_t* valid,
                          float* uv, int32_t* level, int* n_valid) {
  CallArea A;
  const int rc = prepare_sources(m, cur_frame, src_frame, map, cam, mode, rows, flags, n_src, &A);
  if (rc) return rc;
  const float* srcAngle = nullptr;
  int maxOctave = 0;
  const SrcParams P = source_params(cur_frame, src_frame, map, cam, mode, n_src, A, &srcAngle, &maxOctave);
  return run_projection(m, A, n_src,
                        [&] {
                          orbfe::frame_wait_ready(src_frame, m->stream);
                          hipLaunchKernelGGL(k_project_sources, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P);
                        },
                        Outputs{valid, uv, level, nullptr}, n_valid);
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
  const float* srcAngle = nullptr;
  int maxOctave = 0;
  SrcParams P = source_params(cur_frame, src_frame, map, cam, mode, n_src, A, &srcAngle, &maxOctave);
  // nLastOctave indexes mvScaleFactors (:1347): refused up front from the source frame's largest octave
  if (mode == ORBFE_SRC_LAST_FRAME && maxOctave >= nlevels) {
    set_err("the source frame holds a keypoint of octave %d: outside [0, %d)", maxOctave, nlevels);
    return ORBFE_ERR_INVALID;
  }
  if ((rc = fused_params(map, nlevels, valid, uv, level, &P.c, 1, (void**)&P.dvalid, 1, (void**)&P.dclaim))) return rc;
  return run_fused(
      m, A, n_src, nlevels, n != 0, "source",
      [&] {
        orbfe::frame_wait_ready(src_frame, m->stream);
        hipLaunchKernelGGL(k_project_sources, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P);
      },
      [&] {
        return orbfe::sbp_uv_frame_device_queries(m, cur_frame, scale_factors, nlevels, kp_occupied, P.c.dxy, P.c.dlevel, srcAngle, P.dvalid,
                                                  P.dclaim, map->table.p + 32, P.c.drow, n_src, th, max_dist,
                                                  mode == ORBFE_SRC_KEYFRAME ? 1 : 0, check_orientation, kp_assigned, nmatches);
      },
      Outputs{valid, uv, level, nullptr}, nmatches, n_valid);
}

int orbfe_project_keyframe(orbfe_matcher* m, orbfe_frame* kf_frame, orbfe_local_map* map, const OrbfeKeyFrameProjection* proj,
                           const int32_t* rows, const uint8_t* flags, int n, const float* scale_factors, int nlevels, float th,
                           uint8_t* valid, float* uv, int32_t* level, float* radius, int* n_valid) {
  CallArea A;
  const int rc = prepare_keyframe(m, kf_frame, map, proj, rows, flags, n, scale_factors, nlevels, &A);
  if (rc) return rc;
  const KfParams P = keyframe_params(kf_frame, map, proj, n, scale_factors, nlevels, th, A);
  return run_projection(m, A, n, [&] { hipLaunchKernelGGL(k_project_keyframe, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P); },
                        Outputs{valid, uv, level, radius}, n_valid);
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
  *nmatches = 0;
  *n_valid = 0;
  for (int i = 0; i < n; i++) {
    best_idx[i] = -1;
    if (best_dist) best_dist[i] = -1;
  }
  if (n == 0) return ORBFE_OK;
  KfParams P = keyframe_params(kf_frame, map, proj, n, scale_factors, nlevels, th, A);
  P.radius = nullptr;
  if ((rc = fused_params(map, nlevels, valid, uv, level, &P.c, 4, (void**)&P.dradius, 1, (void**)&P.dvalid))) return rc;
  return run_fused(
      m, A, n, nlevels, orbfe_frame_size(kf_frame) != 0, "MapPoint",
      [&] { hipLaunchKernelGGL(k_project_keyframe, dim3(A.blocks), dim3(kProjThreads), 0, m->stream, P); },
      [&] {
        return orbfe::search_projected_frame_device_queries(m, kf_frame, scale_factors, nlevels, th, P.c.dxy, P.c.dlevel, P.dradius, P.dvalid,
                                                            map->table.p + 32, P.c.drow, n, kp_skip, claim, inv_level_sigma2, chi2,
                                                            max_dist, best_idx, best_dist, nmatches);
      },
      Outputs{valid, uv, level, nullptr}, nmatches, n_valid);
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