// orbfe_ransac.hip -- the inlier tests of the two RANSAC solvers that follow the BoW searches: Sim3Solver::CheckInliers with its
// two Project calls (src/Sim3Solver.cc:343-367, :385-406; loop closing) and PnPsolver::CheckInliers (src/PnPsolver.cc:313-344;
// relocalisation), for a flat list of hypotheses that belong to several solvers ("segments") at once.  C ABI: include/orbfe.h
// (RANSAC scoring section); argument check: ransac_plan.h.  The minimal-set solvers (Horn's closed form with cv::eigen, EPnP)
// stay with the application; what comes here are their results.  The selection among the counts is sequential and stays on the
// host (include/orbfe/RansacScoring.h).
//
// What decides the bits.  Every expression is the reference's, operation for operation, without contraction (the library is
// built -ffp-contract=off).  SIM3: Rcw*X + tcw is cv::gemm's small-matrix path (oracle/cv_small.h cvGemm3) -- a float dot
// product taken left to right, then (float)((double)t + (double)tcw); 1/z is a float division; fx*x + cx is float; dist.dot(dist)
// is a double sum of double products rounded to float; mvnMaxError is size_t in the reference and arrives here as the float the
// comparison converts it to.  PNP: mRi and mti are double, so Xc, Yc and the divisor are double expressions rounded to float
// once; ue = uc + fu*Xc*invZc is double; distX is the double difference rounded to float; error2 is float.  A NaN compares
// false and is an outlier; nothing tests the sign of z.  A hypothesis' count is a sum of integers (popcounts), so unlike the
// Initializer's float scores it needs no ordered sum: any reduction gives the same number.
#include "orbfe_matcher_internal.h"
#include "ransac_plan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
enum { SIM3 = 0, PNP = 1 };

// u, v of Sim3Solver::Project (:399-404) for one point; T: the top three rows of the 4x4, row-major (r00 r01 r02 t0 r10 ...).
__device__ __forceinline__ void project_sim3(const float* T, float x0, float x1, float x2, float fx, float fy, float cx, float cy, float& u,
                                             float& v) {
  const float t0 = T[0] * x0 + T[1] * x1 + T[2] * x2;
  const float t1 = T[4] * x0 + T[5] * x1 + T[6] * x2;
  const float t2 = T[8] * x0 + T[9] * x1 + T[10] * x2;
  const float X = (float)((double)t0 + (double)T[3]);
  const float Y = (float)((double)t1 + (double)T[7]);
  const float Z = (float)((double)t2 + (double)T[11]);
  const float invz = 1.0f / Z;
  const float x = X * invz;
  const float y = Y * invz;
  u = fx * x + cx;
  v = fy * y + cy;
}

// dist.dot(dist) of a 2x1 float Mat
__device__ __forceinline__ float dot2(float dx, float dy) { return (float)((double)dx * (double)dx + (double)dy * (double)dy); }

// Sim3Solver.cc:351-366 for one correspondence.  row: X3Dc1[3] X3Dc2[3] P1im1[2] P2im2[2] maxErr1 maxErr2.
// h: T12 (12 floats), T21 (12 floats).  cam: fx fy cx cy of mK1, then of mK2.
__device__ __forceinline__ bool inlier_sim3(const float4* __restrict__ row, const float* h, const float* cam) {
  const float4 a = row[0], b = row[1], c = row[2];
  float u, v;
  project_sim3(h, a.w, b.x, b.y, cam[0], cam[1], cam[2], cam[3], u, v);          // vP2im1 = Project(mvX3Dc2, mT12i, mK1)
  const float err1 = dot2(b.z - u, b.w - v);                                    // mvP1im1[i] - vP2im1[i]
  project_sim3(h + 12, a.x, a.y, a.z, cam[4], cam[5], cam[6], cam[7], u, v);    // vP1im2 = Project(mvX3Dc1, mT21i, mK2)
  const float err2 = dot2(u - c.x, v - c.y);                                    // vP1im2[i] - mvP2im2[i]
  return err1 < c.z && err2 < c.w;
}

// PnPsolver.cc:319-343 for one correspondence.  row: P3Dw[3] P2D[2] maxErr, two floats of padding.
// h: mRi[9] mti[3] in double.  cam: uc vc fu fv in double.
__device__ __forceinline__ bool inlier_pnp(const float4* __restrict__ row, const double* h, const double* cam) {
  const float4 a = row[0], b = row[1];
  const float px = a.x, py = a.y, pz = a.z, u = a.w, v = b.x, maxErr = b.y;
  const float Xc = (float)(h[0] * px + h[1] * py + h[2] * pz + h[9]);
  const float Yc = (float)(h[3] * px + h[4] * py + h[5] * pz + h[10]);
  const float invZc = (float)(1.0 / (h[6] * px + h[7] * py + h[8] * pz + h[11]));
  const double ue = cam[0] + cam[2] * Xc * invZc;
  const double ve = cam[1] + cam[3] * Yc * invZc;
  const float distX = (float)((double)u - ue);
  const float distY = (float)((double)v - ve);
  const float error2 = distX * distX + distY * distY;
  return error2 < maxErr;
}

// One workgroup per hypothesis.  The hypothesis, its segment and the segment's camera are block-uniform; a lane takes one
// correspondence, a wave 64 consecutive ones, and the wave's ballot is their mask word.  wordOff[k]: the first word of
// hypothesis k; words at and beyond ceil(n / 64) do not exist, bits at and above n in the last word are 0 (their lanes vote false).
template <int MODEL>
__global__ __launch_bounds__(kThreads) void k_ransac_score(const float4* __restrict__ corr, const int32_t* __restrict__ segOff,
                                                            const int32_t* __restrict__ hypSeg, const int64_t* __restrict__ wordOff,
                                                            const uint8_t* __restrict__ cams, const uint8_t* __restrict__ hyps,
                                                            int32_t* __restrict__ counts, unsigned long long* __restrict__ masks) {
  __shared__ int s_cnt[kWaves];
  constexpr int kRow = MODEL == SIM3 ? 3 : 2;   // float4 per staged correspondence
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = blockIdx.x;
  const int seg = hypSeg[k];
  const int first = segOff[seg], n = segOff[seg + 1] - first;
  const uint8_t* cam = cams + 32 * (size_t)seg;    // 8 floats or 4 doubles
  const uint8_t* hyp = hyps + 96 * (size_t)k;      // 24 floats or 12 doubles
  const float4* rows = corr + (size_t)kRow * (size_t)first;
  unsigned long long* words = masks + wordOff[k];
  int cnt = 0;
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + tid;
    bool in = false;
    if (i < n) {
      if (MODEL == SIM3) in = inlier_sim3(rows + (size_t)kRow * (size_t)i, reinterpret_cast<const float*>(hyp), reinterpret_cast<const float*>(cam));
      else in = inlier_pnp(rows + (size_t)kRow * (size_t)i, reinterpret_cast<const double*>(hyp), reinterpret_cast<const double*>(cam));
    }
    const unsigned long long word = __ballot(in);
    const int w0 = base + 64 * wave;             // the wave's first correspondence
    if (lane == 0 && w0 < n) {
      words[w0 >> 6] = word;
      cnt += __builtin_popcountll(word);
    }
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) total += s_cnt[w];
    counts[k] = total;
  }
}

struct RansacScratch {
  DevBuf<uint8_t> d_in;     // the call's upload: layout, cameras, hypotheses, correspondences
  PinBuf<uint8_t> h_in;
  PinBuf<uint8_t> h_out;    // counts, then the packed mask words, written by the kernel where the host reads them
  ~RansacScratch() { d_in.release(); h_in.release(); h_out.release(); }
};

// hypA / hypB: T12 and T21 (12 floats each) for SIM3; Rt (12 doubles) twice for PNP.
template <int MODEL>
int score(orbfe_matcher* m, int n_seg, const int32_t* seg_off, const float* corr, const void* cams, int n_hyp, const int32_t* hyp_seg,
          const void* hypA, const void* hypB, int32_t* counts, const int64_t* mask_off, uint64_t* masks) {
  if (!m) { set_err("invalid argument: matcher is NULL"); return ORBFE_ERR_INVALID; }
  orbfe::RansacPlan plan;
  if (orbfe::ransac_check(n_seg, seg_off, corr, cams, n_hyp, hyp_seg, hypA, hypB, mask_off, masks != nullptr, plan)) {
    set_err("invalid argument: %s", plan.why);
    return ORBFE_ERR_INVALID;
  }
  if (!counts && !masks) return ORBFE_OK;
  HIP_TRY(hipSetDevice(m->device));
  RansacScratch* S = scratch_in<RansacScratch>(m->ransac);
  const size_t ns = (size_t)n_seg, nh = (size_t)n_hyp, nc = (size_t)plan.nCorr, nw = (size_t)plan.words;
  constexpr size_t kRowBytes = MODEL == SIM3 ? 48 : 32;
  // the upload image, each part on a 256-byte boundary
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += al(bytes); return at; };
  const size_t oSeg = take(4 * (ns + 1)), oHypSeg = take(4 * nh), oWord = take(8 * nh), oCam = take(32 * ns), oHyp = take(96 * nh),
               oCorr = take(kRowBytes * nc), inBytes = o;
  const size_t oMasks = al(4 * nh), outBytes = oMasks + 8 * nw;
  int rc;
  if ((rc = S->h_in.ensure(inBytes)) || (rc = S->d_in.ensure(inBytes)) || (rc = S->h_out.ensure(outBytes))) return rc;
  uint8_t* H = S->h_in.p;
  int32_t* hs = reinterpret_cast<int32_t*>(H + oSeg);
  for (size_t s = 0; s <= ns; s++) hs[s] = seg_off[s] - plan.base;
  memcpy(H + oHypSeg, hyp_seg, 4 * nh);
  int64_t* hw = reinterpret_cast<int64_t*>(H + oWord);
  orbfe::ransac_packed_offsets(seg_off, n_hyp, hyp_seg, hw);
  memcpy(H + oCam, cams, 32 * ns);
  if (MODEL == SIM3) {
    float* hh = reinterpret_cast<float*>(H + oHyp);
    const float *a = static_cast<const float*>(hypA), *b = static_cast<const float*>(hypB);
    for (size_t k = 0; k < nh; k++) { memcpy(hh + 24 * k, a + 12 * k, 48); memcpy(hh + 24 * k + 12, b + 12 * k, 48); }
    if (nc) memcpy(H + oCorr, corr + (size_t)orbfe::kRansacSim3Row * (size_t)plan.base, 48 * nc);
  } else {
    memcpy(H + oHyp, hypA, 96 * nh);
    float* hc = reinterpret_cast<float*>(H + oCorr);
    const float* c = corr + (size_t)orbfe::kRansacPnPRow * (size_t)plan.base;   // (never formed from a NULL corr: nc == 0 then)
    for (size_t i = 0; i < nc; i++) { memcpy(hc + 8 * i, c + 6 * i, 24); hc[8 * i + 6] = 0.f; hc[8 * i + 7] = 0.f; }
  }
  HIP_TRY(hipMemcpyAsync(S->d_in.p, H, inBytes, hipMemcpyHostToDevice, m->stream));
  const uint8_t* D = S->d_in.p;
  hipLaunchKernelGGL(k_ransac_score<MODEL>, dim3((unsigned)n_hyp), dim3(kThreads), 0, m->stream, reinterpret_cast<const float4*>(D + oCorr),
                     reinterpret_cast<const int32_t*>(D + oSeg), reinterpret_cast<const int32_t*>(D + oHypSeg),
                     reinterpret_cast<const int64_t*>(D + oWord), D + oCam, D + oHyp, reinterpret_cast<int32_t*>(S->h_out.p),
                     reinterpret_cast<unsigned long long*>(S->h_out.p + oMasks));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(m->stream));   // the results are in host memory: no copy command follows the kernel
  if (counts) memcpy(counts, S->h_out.p, 4 * nh);
  if (masks) {
    const uint64_t* R = reinterpret_cast<const uint64_t*>(S->h_out.p + oMasks);
    if (!mask_off) memcpy(masks, R, 8 * nw);
    else
      for (size_t k = 0; k < nh; k++) {
        const size_t w = (size_t)((k + 1 < nh ? hw[k + 1] : (int64_t)nw) - hw[k]);
        if (w) memcpy(masks + mask_off[k], R + hw[k], 8 * w);
      }
  }
  return ORBFE_OK;
}

}  // namespace

extern "C" {

int orbfe_score_sim3_hypotheses(orbfe_matcher* m, int n_seg, const int32_t* seg_off, const float* corr, const float* cams, int n_hyp,
                                const int32_t* hyp_seg, const float* T12, const float* T21, int32_t* counts, const int64_t* mask_off,
                                uint64_t* masks) {
  return score<SIM3>(m, n_seg, seg_off, corr, cams, n_hyp, hyp_seg, T12, T21, counts, mask_off, masks);
}

int orbfe_score_pnp_hypotheses(orbfe_matcher* m, int n_seg, const int32_t* seg_off, const float* corr, const double* cams, int n_hyp,
                               const int32_t* hyp_seg, const double* Rt, int32_t* counts, const int64_t* mask_off, uint64_t* masks) {
  return score<PNP>(m, n_seg, seg_off, corr, cams, n_hyp, hyp_seg, Rt, Rt, counts, mask_off, masks);
}

size_t orbfe_ransac_mask_words(int n_seg, const int32_t* seg_off, int n_hyp, const int32_t* hyp_seg) {
  orbfe::RansacPlan plan;
  if (orbfe::ransac_check_layout(n_seg, seg_off, n_hyp, hyp_seg, plan)) {
    set_err("invalid argument: %s", plan.why);
    return 0;
  }
  return (size_t)plan.words;
}

}  // extern "C"
