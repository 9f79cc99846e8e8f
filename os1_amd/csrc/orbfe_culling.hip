// orbfe_culling.hip -- the counting loop of LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:574-598) for a batch of
// subjects.  C ABI: include/orbfe.h (keyframe culling section); the argument check is in culling_plan.h; what follows the counting
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

struct CullingScratch {
  DevBuf<uint8_t> d_in, d_out;
  PinBuf<uint8_t> h_in, h_out;
  hipEvent_t t0 = nullptr, t1 = nullptr;   // around the launch
  double ms[3] = {0, 0, 0};                // check + staging on the host, kernel, the whole call
  ~CullingScratch() {
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    d_in.release(); d_out.release(); h_in.release(); h_out.release();
    (void)hipGetLastError();
  }
};

CullingScratch* scratch_of(orbfe_matcher* m) {
  if (!m->culling) m->culling = std::make_shared<CullingScratch>();
  return static_cast<CullingScratch*>(m->culling.get());
}

}  // namespace

extern "C" {

int orbfe_debug_culling_ms(const orbfe_matcher* m, double out[3]) {
  if (!m || !out) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  const CullingScratch* S = static_cast<const CullingScratch*>(m->culling.get());
  for (int k = 0; k < 3; k++) out[k] = S ? S->ms[k] : 0.0;
  return ORBFE_OK;
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
  CullingScratch* S = scratch_of(m);

  // one page-locked arena, one copy up: the two CSRs rebased to 0, their level bytes, Observations() per MapPoint, self per subject
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += al(bytes); return at; };
  const size_t ns = (size_t)n_subj;
  const size_t oObsOffs = take(4 * ((size_t)n_mp + 1)), oObsKf = take(4 * plan.nObs + 4), oObsLevel = take(plan.nObs + 4), oNobs = take(4 * (size_t)n_mp + 4),
               oSelf = take(4 * ns), oSubjOffs = take(4 * (ns + 1)), oSubjMp = take(4 * plan.nEntries + 4), oSubjLevel = take(plan.nEntries + 4),
               inBytes = o;
  o = 0;
  const size_t oMps = take(4 * ns), oRed = take(4 * ns), outBytes = o;
  int rc;
  if ((rc = S->h_in.ensure(inBytes)) || (rc = S->d_in.ensure(inBytes)) || (rc = S->h_out.ensure(outBytes)) || (rc = S->d_out.ensure(outBytes))) return rc;
  if (!S->t0) {
    HIP_TRY(hipEventCreate(&S->t0));
    HIP_TRY(hipEventCreate(&S->t1));
  }
  uint8_t* H = S->h_in.p;
  int32_t* ho = (int32_t*)(H + oObsOffs);
  for (int p = 0; p <= n_mp; p++) ho[p] = obs_offsets[p] - plan.obsBase;
  if (plan.nObs) {
    memcpy(H + oObsKf, obs_kf + plan.obsBase, 4 * plan.nObs);
    memcpy(H + oObsLevel, obs_level + plan.obsBase, plan.nObs);
  }
  int32_t* hn = (int32_t*)(H + oNobs);
  for (int p = 0; p < n_mp; p++) hn[p] = mp_nobs ? mp_nobs[p] : ho[p + 1] - ho[p];
  memcpy(H + oSelf, subj_self, 4 * ns);
  int32_t* hs = (int32_t*)(H + oSubjOffs);
  for (int s = 0; s <= n_subj; s++) hs[s] = subj_offsets[s] - plan.subjBase;
  if (plan.nEntries) {
    memcpy(H + oSubjMp, subj_mp + plan.subjBase, 4 * plan.nEntries);
    memcpy(H + oSubjLevel, subj_level + plan.subjBase, plan.nEntries);
  }
  const double tStaged = orbfe_matcher::nowMs();
  HIP_TRY(hipMemcpyAsync(S->d_in.p, H, inBytes, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipMemsetAsync(S->d_out.p, 0, outBytes, m->stream));

  CullParams P{};
  uint8_t* D = S->d_in.p;
  P.obsOffs = (const int32_t*)(D + oObsOffs); P.obsKf = (const int32_t*)(D + oObsKf); P.obsLevel = D + oObsLevel;
  P.mpNobs = (const int32_t*)(D + oNobs);
  P.subjSelf = (const int32_t*)(D + oSelf); P.subjOffs = (const int32_t*)(D + oSubjOffs);
  P.subjMp = (const int32_t*)(D + oSubjMp); P.subjLevel = D + oSubjLevel;
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
