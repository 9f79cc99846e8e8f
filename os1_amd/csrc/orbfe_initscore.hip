// orbfe_initscore.hip -- the scoring passes of the monocular initialiser: Initializer::CheckHomography and CheckFundamental
// (src/Initializer.cc:305-388, :390-468) for every RANSAC hypothesis at once, and the keep-the-best rule of FindHomography /
// FindFundamental (:148-171, :199-222).  C ABI: include/orbfe.h (initialiser section).  The 8-point solves (ComputeH21,
// ComputeF21: cv::SVD) stay with the application; what comes here are their results, n_hyp matrices per model.
//
// What decides the bits.  (1) Every expression is the reference's, operation for operation, in float, without contraction
// (the library is built -ffp-contract=off); `1.0/(float expression)` is a double division rounded to float.  (2) A
// hypothesis' score is a float sum taken over the matches IN ORDER, two terms per match; float addition is not associative,
// so no tree or wave reduction may take its place.  One workgroup therefore owns one hypothesis: its 256 lanes compute the
// 2N terms in parallel into LDS, a chunk of kChunk matches at a time, and one lane adds the chunk up in order while the
// others already fill the second buffer.  A rejected term is stored as +0.0f: x + (+0) == x for every x but -0, and the
// running sum starts at +0 and only ever receives terms >= +0 or NaN.  (3) `chi > th` rejects; a NaN chi does not (the
// comparison is false), counts as an inlier and poisons the sum, as in the reference; a NaN score then never wins, because
// `currentScore > score` is false for it.
#include "orbfe_matcher_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 1024;          // matches per LDS chunk (two chunks of float2 terms: 16 KB per workgroup)
constexpr int kMaskPerBlock = 1024;   // matches per block of k_init_select: four flags per lane, one 32-bit store
constexpr int kGatherThreads = 1024;

// The two terms of match p = (u1, v1, u2, v2) under hypothesis m, +0 where the reference adds nothing; returns bIn.
// MODEL 0: m[0..8] = H21, m[9..17] = H12 (Initializer.cc:337-385).  MODEL 1: m[0..8] = F21 (:413-465).
template <int MODEL>
__device__ __forceinline__ bool terms(const float* m, const float4 p, const float invSigmaSquare, float& c1, float& c2) {
  const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
  bool bIn = true;
  if (MODEL == 0) {
    const float th = 5.991f;
    const float h11 = m[0], h12 = m[1], h13 = m[2], h21 = m[3], h22 = m[4], h23 = m[5], h31 = m[6], h32 = m[7], h33 = m[8];
    const float h11inv = m[9], h12inv = m[10], h13inv = m[11], h21inv = m[12], h22inv = m[13], h23inv = m[14], h31inv = m[15],
                h32inv = m[16], h33inv = m[17];
    const float w2in1inv = (float)(1.0 / (double)(h31inv * u2 + h32inv * v2 + h33inv));
    const float u2in1 = (h11inv * u2 + h12inv * v2 + h13inv) * w2in1inv;
    const float v2in1 = (h21inv * u2 + h22inv * v2 + h23inv) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; c1 = 0.f; }
    else c1 = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(h31 * u1 + h32 * v1 + h33));
    const float u1in2 = (h11 * u1 + h12 * v1 + h13) * w1in2inv;
    const float v1in2 = (h21 * u1 + h22 * v1 + h23) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; c2 = 0.f; }
    else c2 = th - chiSquare2;
  } else {
    const float th = 3.841f, thScore = 5.991f;
    const float f11 = m[0], f12 = m[1], f13 = m[2], f21 = m[3], f22 = m[4], f23 = m[5], f31 = m[6], f32 = m[7], f33 = m[8];
    const float a2 = f11 * u1 + f12 * v1 + f13;
    const float b2 = f21 * u1 + f22 * v1 + f23;
    const float c2l = f31 * u1 + f32 * v1 + f33;
    const float num2 = a2 * u2 + b2 * v2 + c2l;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; c1 = 0.f; }
    else c1 = thScore - chiSquare1;
    const float a1 = f11 * u2 + f21 * v2 + f31;
    const float b1 = f12 * u2 + f22 * v2 + f32;
    const float c1l = f13 * u2 + f23 * v2 + f33;
    const float num1 = a1 * u1 + b1 * v1 + c1l;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; c2 = 0.f; }
    else c2 = thScore - chiSquare2;
  }
  return bIn;
}

// hyp: [3][K][9] = H21, H12, F21.  The 18 (9) floats of hypothesis h of a model, block-uniform.
__device__ __forceinline__ void load_hyp(const float* __restrict__ hyp, int K, int model, int h, float m[18]) {
  const float* a = hyp + ((size_t)(model ? 2 : 0) * K + h) * 9;
  const float* b = hyp + ((size_t)K + h) * 9;
#pragma unroll
  for (int i = 0; i < 9; i++) { m[i] = a[i]; m[9 + i] = model ? 0.f : b[i]; }
}

// grid (K, models): block (h, y) scores hypothesis h of model y (of model 1 when the homographies are absent).
__global__ __launch_bounds__(kThreads) void k_init_score(const float4* __restrict__ pts, int n, const float* __restrict__ hyp, int K,
                                                          int hasH, float invSigmaSquare, float* __restrict__ scores /* [2][K] */) {
  __shared__ float2 s_c[2][kChunk];
  const int tid = threadIdx.x, h = blockIdx.x, model = hasH ? (int)blockIdx.y : 1;
  float m[18];
  load_hyp(hyp, K, model, h, m);
  float score = 0.f;
  int buf = 0;
  for (int base = 0; base < n; base += kChunk, buf ^= 1) {
    const int cnt = min(kChunk, n - base), padded = (cnt + 1) & ~1;   // the walk reads two matches at a time
    for (int j = tid; j < padded; j += kThreads) {
      float c1 = 0.f, c2 = 0.f;
      if (j < cnt) {
        const float4 p = pts[base + j];
        if (model == 0) terms<0>(m, p, invSigmaSquare, c1, c2);
        else terms<1>(m, p, invSigmaSquare, c1, c2);
      }
      s_c[buf][j] = make_float2(c1, c2);
    }
    // one barrier per chunk: lane 0 reaches the next one only after its walk of this buffer, and the other lanes write this
    // buffer again only behind that next barrier
    __syncthreads();
    if (tid == 0) {
      const float4* q = reinterpret_cast<const float4*>(s_c[buf]);
#pragma unroll 4
      for (int j = 0; j < padded / 2; j++) {
        const float4 v = q[j];
        score += v.x; score += v.y; score += v.z; score += v.w;
      }
    }
  }
  if (tid == 0) scores[model * K + h] = score;
}

// Words of the page-locked result block: [scores H: K][scores F: K][best H, best F][best score H, best score F]
// [flags H: W words][flags F: W words], W = ceil(n / 4), one byte per match.
__host__ __device__ inline size_t out_words(int K, int n) { return 2 * (size_t)K + 4 + 2 * (size_t)((n + 3) / 4); }

// grid (ceil(n / kMaskPerBlock), 2): block (x, y) repeats the selection of model y (K compares) and writes the winner's flags of its
// kMaskPerBlock matches; blocks x == 0 also write the model's scores and winner.
__global__ __launch_bounds__(kThreads) void k_init_select(const float4* __restrict__ pts, int n, const float* __restrict__ hyp, int K,
                                                           int hasH, int hasF, float invSigmaSquare, const float* __restrict__ scores,
                                                           uint32_t* __restrict__ out) {
  __shared__ float s_best[kThreads];
  __shared__ int s_idx[kThreads];
  const int tid = threadIdx.x, model = blockIdx.y;
  if (model == 0 ? !hasH : !hasF) return;
  // `if(currentScore>score)` with score = 0 at the start: the first of the largest scores above 0; NaN never compares greater
  float best = 0.f;
  int idx = -1;
  for (int k = tid; k < K; k += kThreads) {
    const float s = scores[model * K + k];
    if (s > best) { best = s; idx = k; }
  }
  s_best[tid] = best; s_idx[tid] = idx;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < kThreads; t++) {
      const float b = s_best[t];
      const int i = s_idx[t];
      if (i >= 0 && (b > best || (b == best && i < idx))) { best = b; idx = i; }
    }
    s_best[0] = best; s_idx[0] = idx;
  }
  __syncthreads();
  best = s_best[0]; idx = s_idx[0];
  const size_t W = (size_t)((n + 3) / 4);
  if (blockIdx.x == 0) {
    for (int k = tid; k < K; k += kThreads) out[(size_t)model * K + k] = __float_as_uint(scores[model * K + k]);
    if (tid == 0) {
      out[2 * (size_t)K + model] = (uint32_t)idx;
      out[2 * (size_t)K + 2 + model] = __float_as_uint(best);
    }
  }
  const int i0 = blockIdx.x * kMaskPerBlock + tid * 4;
  if (i0 >= n) return;
  uint32_t word = 0u;
  if (idx >= 0) {
    float m[18];
    load_hyp(hyp, K, model, idx, m);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (i0 + u >= n) break;
      float c1, c2;
      const float4 p = pts[i0 + u];
      const bool in = model == 0 ? terms<0>(m, p, invSigmaSquare, c1, c2) : terms<1>(m, p, invSigmaSquare, c1, c2);
      word |= (in ? 1u : 0u) << (8 * u);
    }
  }
  out[2 * (size_t)K + 4 + (size_t)model * W + (size_t)(i0 >> 2)] = word;
}

// Initializer.cc:54-63 on the device: the matched pairs (i, matches12[i]), i ascending, become pts[0..N) with the coordinates
// of the two resident frames.  One block; the positions come from ballots and a running base.
__global__ __launch_bounds__(kGatherThreads) void k_init_gather(const int32_t* __restrict__ m12, int n1, const float* __restrict__ x1,
                                                                 const float* __restrict__ y1, const float* __restrict__ x2,
                                                                 const float* __restrict__ y2, int n2, float4* __restrict__ pts, int cap) {
  __shared__ int wtot[kGatherThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int running = 0;
  for (int base = 0; base < n1; base += kGatherThreads) {
    const int i = base + tid;
    const int mm = i < n1 ? m12[i] : -1;
    const bool valid = mm >= 0 && mm < n2;
    const unsigned long long mask = __ballot(valid);
    if (lane == 0) wtot[wave] = __builtin_popcountll(mask);
    __syncthreads();
    int off = running + __builtin_popcountll(mask & ((1ull << lane) - 1ull)), all = 0;
    for (int w = 0; w < kGatherThreads / 64; w++) {
      if (w < wave) off += wtot[w];
      all += wtot[w];
    }
    if (valid && off < cap) pts[off] = make_float4(x1[i], y1[i], x2[mm], y2[mm]);
    running += all;
    __syncthreads();
  }
}

struct InitScratch {
  DevBuf<uint8_t> d_in;      // the call's upload: hypotheses, then the points or matches12
  PinBuf<uint8_t> h_in;
  DevBuf<float4> d_pts;      // the gathered points of the resident-frame form
  DevBuf<float> d_scores;
  PinBuf<uint32_t> h_out;    // the kernels' results, written where the host reads them
  ~InitScratch() { d_in.release(); h_in.release(); d_pts.release(); d_scores.release(); h_out.release(); }
};

struct Outs {
  float *scores_h, *scores_f;
  int32_t *best_h, *best_f;
  float *best_score_h, *best_score_f;
  uint8_t *inliers_h, *inliers_f;
};

int check_common(const orbfe_matcher* m, int n_hyp, const float* H21, const float* H12, const float* F21) {
  if (!m) { set_err("invalid argument: matcher is NULL"); return ORBFE_ERR_INVALID; }
  if (n_hyp < 1) { set_err("invalid argument: n_hyp = %d (at least one hypothesis)", n_hyp); return ORBFE_ERR_INVALID; }
  if ((H21 != nullptr) != (H12 != nullptr)) { set_err("invalid argument: H21 and H12 come together (both or neither)"); return ORBFE_ERR_INVALID; }
  if (!H21 && !F21) { set_err("invalid argument: neither homographies nor fundamental matrices given"); return ORBFE_ERR_INVALID; }
  return ORBFE_OK;
}

// Bytes of the hypotheses at the head of the upload arena; what follows starts at hyp_bytes(K).
size_t hyp_bytes(int K) { return al(sizeof(float) * 27 * (size_t)K); }

int stage_hyps(InitScratch* S, int K, size_t extra, const float* H21, const float* H12, const float* F21) {
  int rc;
  const size_t total = hyp_bytes(K) + al(extra);
  if ((rc = S->h_in.ensure(total)) || (rc = S->d_in.ensure(total))) return rc;
  float* h = reinterpret_cast<float*>(S->h_in.p);
  const size_t one = 9 * (size_t)K;
  if (H21) { memcpy(h, H21, sizeof(float) * one); memcpy(h + one, H12, sizeof(float) * one); }
  if (F21) memcpy(h + 2 * one, F21, sizeof(float) * one);
  return ORBFE_OK;
}

// The two kernels over n > 0 points in device memory, then the results to the caller's arrays.
int score_and_select(orbfe_matcher* m, InitScratch* S, const float4* d_pts, int n, float sigma, int K, bool hasH, bool hasF, const Outs& O) {
  int rc;
  if ((rc = S->d_scores.ensure(2 * (size_t)K)) || (rc = S->h_out.ensure(out_words(K, n)))) return rc;
  const float invSigmaSquare = 1.0 / (sigma * sigma);   // Initializer.cc:335, :411
  const float* hyp = reinterpret_cast<const float*>(S->d_in.p);
  hipLaunchKernelGGL(k_init_score, dim3((unsigned)K, (hasH ? 1u : 0u) + (hasF ? 1u : 0u)), dim3(kThreads), 0, m->stream, d_pts, n, hyp, K,
                     hasH ? 1 : 0, invSigmaSquare, S->d_scores.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_init_select, dim3((unsigned)((n + kMaskPerBlock - 1) / kMaskPerBlock), 2u), dim3(kThreads), 0, m->stream, d_pts, n,
                     hyp, K, hasH ? 1 : 0, hasF ? 1 : 0, invSigmaSquare, (const float*)S->d_scores.p, S->h_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(m->stream));   // the results are in host memory: no copy command follows the kernels
  const uint32_t* R = S->h_out.p;
  const size_t W = (size_t)((n + 3) / 4);
  if (hasH) {
    if (O.scores_h) memcpy(O.scores_h, R, sizeof(float) * (size_t)K);
    if (O.best_h) *O.best_h = (int32_t)R[2 * (size_t)K];
    if (O.best_score_h) memcpy(O.best_score_h, R + 2 * (size_t)K + 2, sizeof(float));
    if (O.inliers_h) memcpy(O.inliers_h, R + 2 * (size_t)K + 4, (size_t)n);
  }
  if (hasF) {
    if (O.scores_f) memcpy(O.scores_f, R + K, sizeof(float) * (size_t)K);
    if (O.best_f) *O.best_f = (int32_t)R[2 * (size_t)K + 1];
    if (O.best_score_f) memcpy(O.best_score_f, R + 2 * (size_t)K + 3, sizeof(float));
    if (O.inliers_f) memcpy(O.inliers_f, R + 2 * (size_t)K + 4 + W, (size_t)n);
  }
  return ORBFE_OK;
}

// No matches: every sum is empty (Initializer.cc:331, :406) and nothing beats the initial score 0 (:137, :188).
void fill_empty(int K, bool hasH, bool hasF, const Outs& O) {
  if (hasH) {
    if (O.scores_h) for (int k = 0; k < K; k++) O.scores_h[k] = 0.f;
    if (O.best_h) *O.best_h = -1;
    if (O.best_score_h) *O.best_score_h = 0.f;
  }
  if (hasF) {
    if (O.scores_f) for (int k = 0; k < K; k++) O.scores_f[k] = 0.f;
    if (O.best_f) *O.best_f = -1;
    if (O.best_score_f) *O.best_score_f = 0.f;
  }
}

// matches12 entries outside [-1, n2) are an error; returns the number of matches (>= 0) or -1
int count_matches(const int32_t* matches12, int n1, int n2) {
  int N = 0;
  for (int i = 0; i < n1; i++) {
    const int32_t v = matches12[i];
    if (v < -1 || v >= n2) { set_err("invalid argument: matches12[%d] = %d is outside [-1, %d)", i, (int)v, n2); return -1; }
    N += v >= 0 ? 1 : 0;
  }
  return N;
}

}  // namespace

extern "C" {

int orbfe_score_init_hypotheses(orbfe_matcher* m, const float* pts, int n, float sigma, int n_hyp, const float* H21, const float* H12,
                                const float* F21, float* scores_h, float* scores_f, int32_t* best_h, int32_t* best_f,
                                float* best_score_h, float* best_score_f, uint8_t* inliers_h, uint8_t* inliers_f) {
  int rc;
  if ((rc = check_common(m, n_hyp, H21, H12, F21))) return rc;
  if (n < 0 || (n > 0 && !pts)) { set_err("invalid argument: n = %d points, pts %s", n, pts ? "given" : "NULL"); return ORBFE_ERR_INVALID; }
  const Outs O{scores_h, scores_f, best_h, best_f, best_score_h, best_score_f, inliers_h, inliers_f};
  if (n == 0) { fill_empty(n_hyp, H21 != nullptr, F21 != nullptr, O); return ORBFE_OK; }
  HIP_TRY(hipSetDevice(m->device));
  InitScratch* S = scratch_in<InitScratch>(m->initscore);
  const size_t pb = sizeof(float) * 4 * (size_t)n;
  if ((rc = stage_hyps(S, n_hyp, pb, H21, H12, F21))) return rc;
  memcpy(S->h_in.p + hyp_bytes(n_hyp), pts, pb);
  HIP_TRY(hipMemcpyAsync(S->d_in.p, S->h_in.p, hyp_bytes(n_hyp) + pb, hipMemcpyHostToDevice, m->stream));
  return score_and_select(m, S, reinterpret_cast<const float4*>(S->d_in.p + hyp_bytes(n_hyp)), n, sigma, n_hyp, H21 != nullptr,
                          F21 != nullptr, O);
}

int orbfe_score_init_hypotheses_kps(orbfe_matcher* m, const OrbfeKeyPoint* kps1_un, int n1, const OrbfeKeyPoint* kps2_un, int n2,
                                    const int32_t* matches12, float sigma, int n_hyp, const float* H21, const float* H12, const float* F21,
                                    float* scores_h, float* scores_f, int32_t* best_h, int32_t* best_f, float* best_score_h,
                                    float* best_score_f, uint8_t* inliers_h, uint8_t* inliers_f, int* n_matches) {
  int rc;
  if ((rc = check_common(m, n_hyp, H21, H12, F21))) return rc;
  if (n1 < 0 || n2 < 0 || (n1 > 0 && (!kps1_un || !matches12)) || (n2 > 0 && !kps2_un)) {
    set_err("invalid argument: keypoint arrays / matches12");
    return ORBFE_ERR_INVALID;
  }
  const int N = count_matches(matches12, n1, n2);
  if (N < 0) return ORBFE_ERR_INVALID;
  const Outs O{scores_h, scores_f, best_h, best_f, best_score_h, best_score_f, inliers_h, inliers_f};
  if (N == 0) { fill_empty(n_hyp, H21 != nullptr, F21 != nullptr, O); if (n_matches) *n_matches = 0; return ORBFE_OK; }
  HIP_TRY(hipSetDevice(m->device));
  InitScratch* S = scratch_in<InitScratch>(m->initscore);
  const size_t pb = sizeof(float) * 4 * (size_t)N;
  if ((rc = stage_hyps(S, n_hyp, pb, H21, H12, F21))) return rc;
  float* p = reinterpret_cast<float*>(S->h_in.p + hyp_bytes(n_hyp));
  for (int i = 0; i < n1; i++) {   // Initializer.cc:54-63
    const int32_t j = matches12[i];
    if (j < 0) continue;
    p[0] = kps1_un[i].x; p[1] = kps1_un[i].y; p[2] = kps2_un[j].x; p[3] = kps2_un[j].y;
    p += 4;
  }
  HIP_TRY(hipMemcpyAsync(S->d_in.p, S->h_in.p, hyp_bytes(n_hyp) + pb, hipMemcpyHostToDevice, m->stream));
  if ((rc = score_and_select(m, S, reinterpret_cast<const float4*>(S->d_in.p + hyp_bytes(n_hyp)), N, sigma, n_hyp, H21 != nullptr,
                             F21 != nullptr, O)))
    return rc;
  if (n_matches) *n_matches = N;
  return ORBFE_OK;
}

int orbfe_score_init_hypotheses_frames(orbfe_matcher* m, orbfe_frame* f1, orbfe_frame* f2, const int32_t* matches12, float sigma,
                                       int n_hyp, const float* H21, const float* H12, const float* F21, float* scores_h, float* scores_f,
                                       int32_t* best_h, int32_t* best_f, float* best_score_h, float* best_score_f, uint8_t* inliers_h,
                                       uint8_t* inliers_f, int* n_matches) {
  int rc;
  if ((rc = check_common(m, n_hyp, H21, H12, F21))) return rc;
  if (!f1 || !f2) { set_err("invalid argument: frame is NULL"); return ORBFE_ERR_INVALID; }
  if (orbfe_frame_device(f1) != m->device || orbfe_frame_device(f2) != m->device) {
    set_err("invalid argument: frames and matcher live on different devices");
    return ORBFE_ERR_INVALID;
  }
  const int n1 = orbfe_frame_size(f1), n2 = orbfe_frame_size(f2);
  if (n1 > 0 && !matches12) { set_err("invalid argument: matches12 is NULL"); return ORBFE_ERR_INVALID; }
  const int N = count_matches(matches12, n1, n2);
  if (N < 0) return ORBFE_ERR_INVALID;
  const Outs O{scores_h, scores_f, best_h, best_f, best_score_h, best_score_f, inliers_h, inliers_f};
  if (N == 0) { fill_empty(n_hyp, H21 != nullptr, F21 != nullptr, O); if (n_matches) *n_matches = 0; return ORBFE_OK; }
  HIP_TRY(hipSetDevice(m->device));
  InitScratch* S = scratch_in<InitScratch>(m->initscore);
  const size_t mb = sizeof(int32_t) * (size_t)n1;
  if ((rc = stage_hyps(S, n_hyp, mb, H21, H12, F21)) || (rc = S->d_pts.ensure((size_t)N))) return rc;
  memcpy(S->h_in.p + hyp_bytes(n_hyp), matches12, mb);
  HIP_TRY(hipMemcpyAsync(S->d_in.p, S->h_in.p, hyp_bytes(n_hyp) + mb, hipMemcpyHostToDevice, m->stream));
  const float *x1, *y1, *x2, *y2;
  orbfe::frame_xy(f1, &x1, &y1);
  orbfe::frame_xy(f2, &x2, &y2);
  orbfe::frame_wait_ready(f1, m->stream);
  orbfe::frame_wait_ready(f2, m->stream);
  hipLaunchKernelGGL(k_init_gather, dim3(1), dim3(kGatherThreads), 0, m->stream,
                     reinterpret_cast<const int32_t*>(S->d_in.p + hyp_bytes(n_hyp)), n1, x1, y1, x2, y2, n2, S->d_pts.p, N);
  HIP_TRY(hipGetLastError());
  if ((rc = score_and_select(m, S, S->d_pts.p, N, sigma, n_hyp, H21 != nullptr, F21 != nullptr, O))) return rc;
  if (n_matches) *n_matches = N;
  return ORBFE_OK;
}

}  // extern "C"
