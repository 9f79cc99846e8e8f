// orbfe_mprefresh.hip -- MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:227-292) and
// MapPoint::UpdateNormalAndDepth (:315-356) for a batch of MapPoints, from the resident keyframes straight into the rows of
// the local map's device table (orbfe_localmap.hip).  C ABI: include/orbfe.h (local-map section).
//
// A MapPoint is named by its table row; its observations are (keyframe slot, keypoint index) pairs.  One wave owns one MapPoint:
// it gathers the 32-byte descriptor rows of the observations in keyframes that are not bad out of the keyframes' resident copies
// (a per-call device array of base pointers) into LDS, finds the descriptor with the least median distance to the others, then
// computes the normal and the depth range and stores all of it into the row.  Per observation 8 bytes go up; no descriptor
// crosses PCIe in either direction.
//
// LDS: the list as [N][8] dwords, 32 bytes per row, nothing else.  In the distance loop every lane reads the SAME row j (a
// broadcast: one address per instruction, no bank conflict whatever the row stride); a lane's own row i is read once into
// registers (two 16-byte reads at a 32-byte lane stride: 2-way on the 64-bank row, once per pass, not worth a padded layout).
// Median: as k_distinctive (orbfe_matcher.hip) -- the element of rank (size_t)(0.5*(N-1)) of row i is the smallest v with
// #{j: d_ij <= v} >= rank+1, found by bisection over 0..256 with the distances recomputed from LDS at each step (nine sweeps of
// N broadcast reads; a stored N x N matrix would not fit beside the list).  Lane i owns rows i, i+64, ... in ascending order
// and keeps its first minimum; the wave reduction orders (median, index) pairs, so the first minimum of the list order wins.
//
// Float rules (this file is built like the rest of the library: no fast-math, -ffp-contract=off, denormals kept):
//   normali = pos - Ow_kf                       float subtraction
//   cv::norm(normali)                           sqrt of the double sum of squares in index order
//   normal = normal + normali/norm              cv::scaleAdd with beta = (float)(1.0/norm): the product is rounded, then added
//   normal/n                                    convertTo with scale: normal*(float)(1.0/n) + 0.0f  (-0 becomes +0)
//   mfMaxDistance = dist*mvScaleFactors[level]  float product
//   mfMinDistance = mfMaxDistance/mvScaleFactors[nLevels-1]   IEEE float division (the compiler's full division sequence)
// The accumulation over the observations is a float sum IN ORDER: the lanes compute the 64 terms of a pass in parallel (the
// double square root and division are the expensive part) and every lane then adds them up in observation order from
// broadcasts, so no tree reduction takes the place of the reference's loop.
#include "orbfe_matcher_internal.h"

#include <atomic>

namespace {

constexpr int kRowBytes = 64;                    // pos[3], normal[3], mfMinDistance, mfMaxDistance, descriptor[32]
constexpr size_t kLdsBudget = 150 * 1024;        // as orbfe_distinctive_descriptors
constexpr unsigned kBadBit = 0x80000000u;        // ORBFE_OBS_KF_BAD travels in bit 31 of the observation's keyframe slot
constexpr int kNoBadLevel = 0x7f7f7f7f;          // what hipMemsetAsync(0x7f) leaves in the report word

struct RefreshParams {
  uint8_t* table;
  const int32_t* rows;             // [n_mp]
  const int32_t* offs;             // [n_mp + 1], offs[0] == 0
  const uint32_t* obsKf;           // [total] slot | kBadBit
  const int32_t* obsKp;            // [total]
  const uint8_t* const* kfDesc;    // [n_kf] descriptor rows of the resident keyframe (null: a slot only bad observations name)
  const int* const* kfOct;         // [n_kf] its octaves
  const float* kfOw;               // [3 * n_kf]
  const int32_t* refKf;            // [n_mp] (NORMAL_DEPTH)
  const int32_t* refKp;
  float sf[32];
  int nlevels;
  int what;
  int32_t* best;                   // [n_mp] outputs in device memory
  float* outRow;                   // [n_mp][5]: normal, min, max as the row holds them after the call
  int* badLevel;                   // first MapPoint whose reference keypoint's octave lies outside [0, nlevels)
};

__global__ __launch_bounds__(64) void k_refresh_map_points(RefreshParams P) {
  extern __shared__ __align__(16) uint32_t dd[];   // [N][8]: the descriptors of the observations whose keyframe is not bad
  const int p = blockIdx.x, lane = threadIdx.x;
  const int o0 = P.offs[p], n = P.offs[p + 1] - o0;
  float* row = reinterpret_cast<float*>(P.table + (size_t)P.rows[p] * kRowBytes);
  const bool doDesc = (P.what & ORBFE_REFRESH_DESCRIPTOR) != 0, doGeom = (P.what & ORBFE_REFRESH_NORMAL_DEPTH) != 0 && n > 0;

  // level = pRefKF->mvKeysUn[observations[pRefKF]].octave: checked before anything is indexed with it or written
  int level = 0;
  if (doGeom) {
    level = P.kfOct[P.refKf[p]][P.refKp[p]];
    if (level < 0 || level >= P.nlevels) {
      if (lane == 0) {
        atomicMin(P.badLevel, p);
        P.best[p] = -1;
        for (int k = 0; k < 5; k++) P.outRow[5 * (size_t)p + k] = row[3 + k];
      }
      return;
    }
  }

  int bestObs = -1;
  if (doDesc && n > 0) {
    // gather, a pass of 64 observations at a time: the ones that count keep their order
    int N = 0;
    for (int b = 0; b < n; b += 64) {
      const int o = b + lane;
      unsigned kf = kBadBit;
      if (o < n) kf = P.obsKf[o0 + o];
      const bool keep = !(kf & kBadBit);
      const unsigned long long mask = __ballot(keep);
      if (keep) {
        const int at = N + __popcll(mask & ((1ull << lane) - 1ull));
        const uint4* src = reinterpret_cast<const uint4*>(P.kfDesc[kf] + (size_t)P.obsKp[o0 + o] * 32);
        const uint4 a = src[0], c = src[1];
        uint4* dst = reinterpret_cast<uint4*>(dd + (size_t)at * 8);
        dst[0] = a;
        dst[1] = c;
      }
      N += __popcll(mask);
    }
    __syncthreads();
    if (N > 0) {
      const int rank = (N - 1) >> 1;   // (size_t)(0.5 * (N - 1))
      int bestMed = 0x7fffffff, bestIdx = 0x7fffffff;
      for (int i = lane; i < N; i += 64) {
        uint32_t qi[8];
#pragma unroll
        for (int w = 0; w < 8; w++) qi[w] = dd[i * 8 + w];
        int lo = 0, hi = 256;   // median in [lo, hi]
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          int cnt = 0;
          for (int j = 0; j < N; j++) {
            int d = 0;
#pragma unroll
            for (int w = 0; w < 8; w++) d += __popc(qi[w] ^ dd[j * 8 + w]);
            cnt += d <= mid;
          }
          if (cnt >= rank + 1) hi = mid; else lo = mid + 1;
        }
        if (lo < bestMed) { bestMed = lo; bestIdx = i; }   // ascending i per lane: first minimum kept
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int om = __shfl_xor(bestMed, o, 64), oi = __shfl_xor(bestIdx, o, 64);
        if (om < bestMed || (om == bestMed && oi < bestIdx)) { bestMed = om; bestIdx = oi; }
      }
      // the winner's place in the full list: the observation with bestIdx kept ones in front of it
      int seen = 0;
      for (int b = 0; b < n; b += 64) {
        const int o = b + lane;
        const bool keep = o < n && !(P.obsKf[o0 + o] & kBadBit);
        const unsigned long long mask = __ballot(keep);
        const int c = __popcll(mask);
        if (bestIdx < seen + c) {
          unsigned long long mm = mask;
          for (int k = seen; k < bestIdx; k++) mm &= mm - 1;   // drop the kept ones in front of it
          bestObs = b + __builtin_ctzll(mm);
          break;
        }
        seen += c;
      }
      if (lane < 8) reinterpret_cast<uint32_t*>(row)[8 + lane] = dd[bestIdx * 8 + lane];   // mDescriptor = vDescriptors[BestIdx]
    }
  }

  float out[5];
  if (doGeom) {
    const float pos[3] = {row[0], row[1], row[2]};
    float normal[3] = {0.0f, 0.0f, 0.0f};
    for (int b = 0; b < n; b += 64) {
      const int o = b + lane;
      float t[3] = {0.0f, 0.0f, 0.0f};
      if (o < n) {
        const float* Ow = P.kfOw + 3 * (size_t)(P.obsKf[o0 + o] & ~kBadBit);
        const float ni[3] = {pos[0] - Ow[0], pos[1] - Ow[1], pos[2] - Ow[2]};   // normali = mWorldPos - Owi
        double s = 0.0;                                                          // cv::norm(normali)
#pragma unroll
        for (int k = 0; k < 3; k++) s += (double)ni[k] * (double)ni[k];
        const float beta = (float)(1.0 / sqrt(s));
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = ni[k] * beta;
      }
      const int cnt = min(64, n - b);
      for (int j = 0; j < cnt; j++) {                                            // normal = normal + normali/norm, in order
#pragma unroll
        for (int k = 0; k < 3; k++) normal[k] = __shfl(t[k], j, 64) + normal[k];
      }
    }
    const float inv = (float)(1.0 / (double)n);                                  // mNormalVector = normal/n
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = normal[k] * inv + 0.0f;
    const float* Or = P.kfOw + 3 * (size_t)P.refKf[p];
    const float PC[3] = {pos[0] - Or[0], pos[1] - Or[1], pos[2] - Or[2]};        // PC = Pos - pRefKF->GetCameraCenter()
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) s += (double)PC[k] * (double)PC[k];
    const float dist = (float)sqrt(s);
    out[4] = dist * P.sf[level];                                                 // mfMaxDistance
    out[3] = out[4] / P.sf[P.nlevels - 1];                                       // mfMinDistance
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 5; k++) row[3 + k] = out[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 5; k++) out[k] = row[3 + k];
  }
  if (lane == 0) {
    P.best[p] = bestObs;
#pragma unroll
    for (int k = 0; k < 5; k++) P.outRow[5 * (size_t)p + k] = out[k];
  }
}

struct RefreshScratch {
  DevBuf<uint8_t> d_in, d_out;
  PinBuf<uint8_t> h_in, h_out;
  hipEvent_t sent = nullptr;       // recorded after the last upload: the staging is free again once it has completed
  std::vector<uint8_t> seen;       // duplicate-row check
  bool ldsAttr = false;
  ~RefreshScratch() {
    if (sent) { (void)hipEventSynchronize(sent); (void)hipEventDestroy(sent); }
    d_in.release(); d_out.release(); h_in.release(); h_out.release();
    (void)hipGetLastError();
  }
};

}  // namespace

extern "C" {

int orbfe_local_map_refresh_rows(orbfe_matcher* m, orbfe_local_map* map, int what, int n_kf, orbfe_frame* const* kf_frames,
                                 const float* kf_Ow, const float* scale_factors, int nlevels, int n_mp, const int32_t* rows,
                                 const int32_t* obs_offsets, const int32_t* obs_kf, const int32_t* obs_kp, const uint8_t* obs_flags,
                                 const int32_t* ref_kf, const int32_t* ref_kp, int32_t* best_obs, float* normal, float* min_raw,
                                 float* max_raw) {
  if (!m || !map || n_mp < 0 || n_kf < 0 || (n_mp && (!rows || !obs_offsets)) || (n_kf && (!kf_frames || !kf_Ow))) {
    set_err("bad argument");
    return ORBFE_ERR_INVALID;
  }
  if (what < 1 || what > (ORBFE_REFRESH_DESCRIPTOR | ORBFE_REFRESH_NORMAL_DEPTH)) {
    set_err("what must be ORBFE_REFRESH_DESCRIPTOR, ORBFE_REFRESH_NORMAL_DEPTH or both");
    return ORBFE_ERR_INVALID;
  }
  orbfe::LocalMapView V;
  orbfe::local_map_view(map, &V);
  if (V.m != m) { set_err("the local map belongs to another matcher (its uploads are ordered on that matcher's stream)"); return ORBFE_ERR_INVALID; }
  if (nlevels < 1 || nlevels > 32) { set_err("nlevels (%d) outside 1..32", nlevels); return ORBFE_ERR_INVALID; }
  const bool geom = (what & ORBFE_REFRESH_NORMAL_DEPTH) != 0;
  if (n_mp == 0) return ORBFE_OK;
  if (geom && (!scale_factors || !ref_kf || !ref_kp)) { set_err("bad argument (NORMAL_DEPTH needs scale_factors, ref_kf and ref_kp)"); return ORBFE_ERR_INVALID; }
  for (int s = 0; s < n_kf; s++)
    if (kf_frames[s] && orbfe_frame_device(kf_frames[s]) != m->device) {
      set_err("keyframe slot %d and matcher live on different devices", s);
      return ORBFE_ERR_INVALID;
    }
  RefreshScratch* S = scratch_in<RefreshScratch>(*V.scratch);
  S->seen.assign((size_t)V.capacity, 0);
  const int base = obs_offsets[0];
  int maxKept = 0;
  bool levelCanFail = false;
  for (int p = 0; p < n_mp; p++) {
    if (rows[p] < 0 || rows[p] >= V.capacity) { set_err("MapPoint %d: row %d outside the local map (%d rows)", p, rows[p], V.capacity); return ORBFE_ERR_INVALID; }
    if (S->seen[rows[p]]) { set_err("row %d named twice", rows[p]); return ORBFE_ERR_INVALID; }
    S->seen[rows[p]] = 1;
    const int a = obs_offsets[p], b = obs_offsets[p + 1];
    if (b < a || a < 0) { set_err("obs_offsets must be non-negative and non-decreasing"); return ORBFE_ERR_INVALID; }
    if (b > a && (!obs_kf || !obs_kp)) { set_err("bad argument (observations without obs_kf / obs_kp)"); return ORBFE_ERR_INVALID; }
    int kept = 0;
    for (int o = a; o < b; o++) {
      const int s = obs_kf[o];
      if (s < 0 || s >= n_kf) { set_err("MapPoint %d: keyframe slot %d outside [0, %d)", p, s, n_kf); return ORBFE_ERR_INVALID; }
      if (obs_flags && (obs_flags[o] & ORBFE_OBS_KF_BAD)) continue;
      if (!kf_frames[s]) { set_err("MapPoint %d: keyframe slot %d is NULL but its observation is not marked bad", p, s); return ORBFE_ERR_INVALID; }
      if (obs_kp[o] < 0 || obs_kp[o] >= orbfe_frame_size(kf_frames[s])) {
        set_err("MapPoint %d: keypoint %d outside keyframe slot %d (%d keypoints)", p, obs_kp[o], s, orbfe_frame_size(kf_frames[s]));
        return ORBFE_ERR_INVALID;
      }
      kept++;
    }
    maxKept = std::max(maxKept, kept);
    if (geom && b > a) {
      const int s = ref_kf[p];
      if (s < 0 || s >= n_kf) { set_err("MapPoint %d: reference keyframe slot %d outside [0, %d)", p, s, n_kf); return ORBFE_ERR_INVALID; }
      if (!kf_frames[s]) { set_err("MapPoint %d: its reference keyframe (slot %d) is NULL", p, s); return ORBFE_ERR_INVALID; }
      if (ref_kp[p] < 0 || ref_kp[p] >= orbfe_frame_size(kf_frames[s])) {
        set_err("MapPoint %d: reference keypoint %d outside keyframe slot %d (%d keypoints)", p, ref_kp[p], s, orbfe_frame_size(kf_frames[s]));
        return ORBFE_ERR_INVALID;
      }
    }
  }
  if ((what & ORBFE_REFRESH_DESCRIPTOR) && (size_t)maxKept * 32 > kLdsBudget) {
    set_err("a MapPoint with %d observations exceeds the LDS budget", maxKept);
    return ORBFE_ERR_INVALID;
  }
  const size_t total = (size_t)(obs_offsets[n_mp] - base);
  HIP_TRY(hipSetDevice(m->device));
  (void)hipGetLastError();

  // one page-locked arena, one copy: per MapPoint row, offset and reference; per observation slot (with the bad bit) and keypoint
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += al(bytes); return at; };
  const size_t c = (size_t)n_mp, k = (size_t)std::max(n_kf, 1);
  const size_t oRows = take(4 * c), oOffs = take(4 * (c + 1)), oRefKf = take(4 * c), oRefKp = take(4 * c), oKf = take(4 * total + 4),
               oKp = take(4 * total + 4), oDesc = take(8 * k), oOct = take(8 * k), oOw = take(12 * k), inBytes = o;
  o = 0;
  const size_t oBad = take(4), oBest = take(4 * c), oOut = take(20 * c), outBytes = o;
  int rc;
  if (S->sent) HIP_TRY(hipEventSynchronize(S->sent));   // the previous call's upload has read the staging
  if ((rc = S->h_in.ensure(inBytes)) || (rc = S->d_in.ensure(inBytes)) || (rc = S->h_out.ensure(outBytes)) || (rc = S->d_out.ensure(outBytes))) return rc;
  if (!S->sent) HIP_TRY(hipEventCreateWithFlags(&S->sent, hipEventDisableTiming));
  uint8_t* H = S->h_in.p;
  memcpy(H + oRows, rows, 4 * c);
  int32_t* ho = (int32_t*)(H + oOffs);
  for (int p = 0; p <= n_mp; p++) ho[p] = obs_offsets[p] - base;
  if (geom) {
    int32_t* hk = (int32_t*)(H + oRefKf);
    int32_t* hp = (int32_t*)(H + oRefKp);
    for (int p = 0; p < n_mp; p++) {
      const bool has = obs_offsets[p + 1] > obs_offsets[p];   // (a MapPoint without observations may carry any reference)
      hk[p] = has ? ref_kf[p] : 0;
      hp[p] = has ? ref_kp[p] : 0;
    }
  }
  uint32_t* hkf = (uint32_t*)(H + oKf);
  for (size_t i = 0; i < total; i++)
    hkf[i] = (uint32_t)obs_kf[base + i] | ((obs_flags && (obs_flags[base + i] & ORBFE_OBS_KF_BAD)) ? kBadBit : 0u);
  if (total) memcpy(H + oKp, obs_kp + base, 4 * total);
  const uint8_t** hd = (const uint8_t**)(H + oDesc);
  const int** hoct = (const int**)(H + oOct);
  for (int s = 0; s < n_kf; s++) {
    hd[s] = nullptr;
    hoct[s] = nullptr;
    if (!kf_frames[s]) continue;
    const float* angle = nullptr;
    int maxOctave = 0;
    orbfe::frame_source_arrays(kf_frames[s], &hoct[s], &angle, &maxOctave);
    hd[s] = orbfe::frame_descriptor_rows(kf_frames[s]);
    if (maxOctave >= nlevels) levelCanFail = true;
    orbfe::frame_wait_ready(kf_frames[s], m->stream);
  }
  if (n_kf) memcpy(H + oOw, kf_Ow, 12 * (size_t)n_kf);
  HIP_TRY(hipMemcpyAsync(S->d_in.p, H, inBytes, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipEventRecord(S->sent, m->stream));
  HIP_TRY(hipMemsetAsync(S->d_out.p + oBad, 0x7f, 4, m->stream));

  RefreshParams P{};
  uint8_t* D = S->d_in.p;
  P.table = V.table;
  P.rows = (const int32_t*)(D + oRows); P.offs = (const int32_t*)(D + oOffs);
  P.obsKf = (const uint32_t*)(D + oKf); P.obsKp = (const int32_t*)(D + oKp);
  P.kfDesc = (const uint8_t* const*)(D + oDesc); P.kfOct = (const int* const*)(D + oOct); P.kfOw = (const float*)(D + oOw);
  P.refKf = (const int32_t*)(D + oRefKf); P.refKp = (const int32_t*)(D + oRefKp);
  if (geom) for (int l = 0; l < nlevels; l++) P.sf[l] = scale_factors[l];
  P.nlevels = nlevels;
  P.what = what;
  P.best = (int32_t*)(S->d_out.p + oBest); P.outRow = (float*)(S->d_out.p + oOut); P.badLevel = (int*)(S->d_out.p + oBad);
  const size_t lds = std::max<size_t>((size_t)maxKept * 32, 32);
  if (lds > 64 * 1024 && !S->ldsAttr) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_refresh_map_points), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
    S->ldsAttr = true;
  }
  hipLaunchKernelGGL(k_refresh_map_points, dim3(n_mp), dim3(64), lds, m->stream, P);
  HIP_TRY(hipGetLastError());
  // Nothing to bring back and no keyframe whose octaves could leave [0, nlevels): the call is enqueued, the stream orders it
  // before the next search.  Otherwise one copy returns the level report and the per-MapPoint results.
  const bool wantOut = best_obs || normal || min_raw || max_raw;
  if (!wantOut && !(geom && levelCanFail)) return ORBFE_OK;
  HIP_TRY(hipMemcpyAsync(S->h_out.p, S->d_out.p, wantOut ? outBytes : al(4), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  const int bad = *(const int*)(S->h_out.p + oBad);
  if (bad != kNoBadLevel) {
    set_err("MapPoint %d: its reference keypoint's octave lies outside [0, %d); its row is left as it was", bad, nlevels);
    return ORBFE_ERR_INVALID;
  }
  if (best_obs) memcpy(best_obs, S->h_out.p + oBest, 4 * c);
  const float* R = (const float*)(S->h_out.p + oOut);
  for (int p = 0; p < n_mp && (normal || min_raw || max_raw); p++) {
    if (normal) memcpy(normal + 3 * (size_t)p, R + 5 * (size_t)p, 12);
    if (min_raw) min_raw[p] = R[5 * (size_t)p + 3];
    if (max_raw) max_raw[p] = R[5 * (size_t)p + 4];
  }
  return ORBFE_OK;
}

int orbfe_local_map_download_rows(orbfe_local_map* map, int n, const int32_t* rows, uint8_t* out) {
  if (!map || n < 0 || (n && (!rows || !out))) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  if (n == 0) return ORBFE_OK;
  orbfe::LocalMapView V;
  orbfe::local_map_view(map, &V);
  for (int i = 0; i < n; i++)
    if (rows[i] < 0 || rows[i] >= V.capacity) { set_err("row %d outside the local map (%d rows)", rows[i], V.capacity); return ORBFE_ERR_INVALID; }
  HIP_TRY(hipSetDevice(V.m->device));
  HIP_TRY(hipStreamSynchronize(V.m->stream));   // every upload and refresh submitted so far has reached the table
  std::vector<uint8_t> all((size_t)V.capacity * kRowBytes);
  HIP_TRY(hipMemcpy(all.data(), V.table, all.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) memcpy(out + (size_t)i * kRowBytes, all.data() + (size_t)rows[i] * kRowBytes, kRowBytes);
  return ORBFE_OK;
}

}  // extern "C"
