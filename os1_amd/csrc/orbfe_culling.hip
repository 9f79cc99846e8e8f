// orbfe_culling.hip -- the counting loop of LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:574-598) for a batch of
// subjects.  C ABI: include/orbfe.h (keyframe culling section); the argument check is in culling_plan.h, the staging of the two CSRs,
// which orbfe_covisibility_counts takes too, in obs_graph_staging.h; what follows the counting
// (the 90 % test, SetBadFlag, the recount after a cull) is include/orbfe/KeyFrameCulling.h.
//
// The CSRs of orbfe_covisibility_counts come up, with a level byte next to every observation and every entry.  The work is all
// entries of all subjects, flattened: one lane per entry, 256 entries per workgroup; the lane finds its subject by bisection of
// subj_offsets.  An observation list of up to kCullingLongList observers is walked by the entry's lane (it stops at th_obs, as the
// reference does); a longer one is handed to the whole wave afterwards, 64 observations per step, counted by ballot and popcount,
// so that a few MapPoints seen from hundreds of keyframes do not hold 63 lanes up.  Subject boundaries fall inside waves: the
// wave peels its subjects off one at a time (ballot of "same subject as the first lane left"), and the first lane of each segment
// adds the two popcounts to the subject's totals with one device atomic each.  The totals are zeroed ahead of the launch.
//
// No float arithmetic anywhere: int32 sums, exact whatever the order of the additions.
#include "orbfe_matcher_internal.h"

#include "culling_plan.h"
#include "obs_graph_staging.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLong = orbfe::kCullingLongList;

struct CullParams {
  const int32_t* obsOffs;      // [n_mp + 1], obsOffs[0] == 0
  const int32_t* obsKf;        // [observations] observer slot
  const uint8_t* obsLevel;     // [observations] octave of the observer's keypoint
  const int32_t* mpNobs;       // [n_mp] MapPoint::Observations()
  const int32_t* subjSelf;     // [n_subj] slot of the subject or -1
  const int32_t* subjOffs;     // [n_subj + 1], subjOffs[0] == 0, subjOffs[n_subj] == nEntries
  const int32_t* subjMp;       // [entries] MapPoint or -1
  const uint8_t* subjLevel;    // [entries] octave of the subject's keypoint
  int nSubj, nEntries, thObs;
  int32_t* outMps;             // [n_subj], zeroed ahead of the launch
  int32_t* outRed;
};

__global__ __launch_bounds__(kThreads) void k_redundant_observations(CullParams P) {
  const int lane = threadIdx.x & 63;
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  int s = 0, p = -1, o0 = 0, o1 = 0, self = -1, top = 0;
  if (e < P.nEntries) {
    int lo = 0, hi = P.nSubj;                      // subjOffs[lo] <= e < subjOffs[hi]: the last subject that starts at or before e
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (P.subjOffs[mid] <= e) lo = mid; else hi = mid;
    }
    s = lo;
    p = P.subjMp[e];
    if (p >= 0 && P.mpNobs[p] > P.thObs) {         // LocalMapping.cc:578
      self = P.subjSelf[s];
      top = (int)P.subjLevel[e] + 1;
      o0 = P.obsOffs[p];
      o1 = P.obsOffs[p + 1];
    }
  }
  const bool valid = p >= 0;                       // LocalMapping.cc:576-577
  const int len = o1 - o0;
  bool red = false;
  if (len > 0 && len <= kLong) {
    int c = 0;
    for (int o = o0; o < o1 && c < P.thObs; o++) c += (P.obsKf[o] != self) & ((int)P.obsLevel[o] <= top);
    red = c >= P.thObs;
  }
  for (unsigned long long todo = __ballot(len > kLong); todo; todo &= todo - 1) {      // wave-uniform
    const int src = __ffsll(todo) - 1;
    const int a0 = __shfl(o0, src, 64), a1 = __shfl(o1, src, 64), sf = __shfl(self, src, 64), tp = __shfl(top, src, 64);
    int c = 0;
    for (int base = a0; base < a1 && c < P.thObs; base += 64) {
      const int o = base + lane;
      const bool q = o < a1 && P.obsKf[o] != sf && (int)P.obsLevel[o] <= tp;
      c += __popcll(__ballot(q));
    }
    if (lane == src) red = c >= P.thObs;
  }
  for (unsigned long long todo = __ballot(valid); todo;) {                             // one round per subject of this wave
    const int first = __ffsll(todo) - 1;
    const int s0 = __shfl(s, first, 64);
    const unsigned long long seg = __ballot(valid && s == s0);
    const int nr = __popcll(__ballot(red && s == s0));
    if (lane == first) {
      atomicAdd(&P.outMps[s0], __popcll(seg));
      if (nr) atomicAdd(&P.outRed[s0], nr);
    }
    todo &= ~seg;
  }
}

}  // namespace

extern "C" {

int orbfe_debug_culling_ms(const orbfe_matcher* m, double out[3]) {
  return orbfe::ObsGraphScratch::lastMs(m ? &m->culling : nullptr, out);
}

int orbfe_redundant_observations(orbfe_matcher* m, int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level,
                                 const int32_t* mp_nobs, int n_subj, const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp,
                                 const uint8_t* subj_level, int th_obs, int32_t* out_n_mps, int32_t* out_n_redundant) {
  const double tEntry = orbfe_matcher::nowMs();
  if (n_kf < 0 || n_mp < 0 || n_subj < 0) {
    set_err("redundant observations: negative size (n_kf %d, n_mp %d, n_subj %d)", n_kf, n_mp, n_subj);
    return ORBFE_ERR_INVALID;
  }
  if (th_obs < 1) { set_err("redundant observations: th_obs = %d is below 1", th_obs); return ORBFE_ERR_INVALID; }
  if (n_subj == 0) {
    if (!m) { set_err("redundant observations: null pointer (matcher)"); return ORBFE_ERR_INVALID; }
    return ORBFE_OK;
  }
  if (!out_n_mps || !out_n_redundant) {
    set_err("redundant observations: null pointer (out_n_mps or out_n_redundant)");
    return ORBFE_ERR_INVALID;
  }
  orbfe::CullingPlan plan;
  if (orbfe::culling_check(n_kf, n_mp, obs_offsets, obs_kf, obs_level, mp_nobs, n_subj, subj_self, subj_offsets, subj_mp, subj_level, th_obs, plan)) {
    set_err("redundant observations: %s", plan.why);
    return ORBFE_ERR_INVALID;
  }
  if (!m) { set_err("redundant observations: null pointer (matcher)"); return ORBFE_ERR_INVALID; }
  HIP_TRY(hipSetDevice(m->device));
  (void)hipGetLastError();
  orbfe::ObsGraphScratch* S = scratch_in<orbfe::ObsGraphScratch>(m->culling);

  // one page-locked arena, one copy up: the graph with its level bytes (obs_graph_stage), then Observations() per MapPoint
  const size_t ns = (size_t)n_subj;
  orbfe::Arena out;
  const size_t oMps = out.take(4 * ns), oRed = out.take(4 * ns), outBytes = out.size;
  orbfe::ObsGraphStaged at;
  int rc;
  if ((rc = orbfe::obs_graph_stage(*S, plan, n_mp, obs_offsets, obs_kf, obs_level, n_subj, subj_self, subj_offsets, subj_mp, subj_level, true,
                                   4 * (size_t)n_mp + 4, outBytes, at)))
    return rc;
  uint8_t* H = S->h_in.p;
  const int32_t* ho = (const int32_t*)(H + at.obsOffs);
  int32_t* hn = (int32_t*)(H + at.extra);
  for (int p = 0; p < n_mp; p++) hn[p] = mp_nobs ? mp_nobs[p] : ho[p + 1] - ho[p];
  const double tStaged = orbfe_matcher::nowMs();
  HIP_TRY(hipMemcpyAsync(S->d_in.p, H, at.bytes, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipMemsetAsync(S->d_out.p, 0, outBytes, m->stream));

  CullParams P{};
  uint8_t* D = S->d_in.p;
  P.obsOffs = (const int32_t*)(D + at.obsOffs); P.obsKf = (const int32_t*)(D + at.obsKf); P.obsLevel = D + at.obsLevel;
  P.mpNobs = (const int32_t*)(D + at.extra);
  P.subjSelf = (const int32_t*)(D + at.self); P.subjOffs = (const int32_t*)(D + at.subjOffs);
  P.subjMp = (const int32_t*)(D + at.subjMp); P.subjLevel = D + at.subjLevel;
  P.nSubj = n_subj; P.nEntries = (int)plan.nEntries; P.thObs = th_obs;
  P.outMps = (int32_t*)(S->d_out.p + oMps); P.outRed = (int32_t*)(S->d_out.p + oRed);
  HIP_TRY(hipEventRecord(S->t0, m->stream));
  if (plan.nEntries) {
    const unsigned blocks = (unsigned)((plan.nEntries + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_redundant_observations, dim3(blocks), dim3(kThreads), 0, m->stream, P);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(S->t1, m->stream));
  HIP_TRY(hipMemcpyAsync(S->h_out.p, S->d_out.p, outBytes, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  float kernelMs = 0.0f;
  HIP_TRY(hipEventElapsedTime(&kernelMs, S->t0, S->t1));
  memcpy(out_n_mps, S->h_out.p + oMps, 4 * ns);
  memcpy(out_n_redundant, S->h_out.p + oRed, 4 * ns);
  S->ms[0] = tStaged - tEntry;
  S->ms[1] = kernelMs;
  S->ms[2] = orbfe_matcher::nowMs() - tEntry;
  return ORBFE_OK;
}

}  // extern "C"
