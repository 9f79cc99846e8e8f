// orbfe_covis.hip -- the counting loop of KeyFrame::UpdateConnections (reference src/KeyFrame.cc:305-331) and of
// Tracking::UpdateLocalKeyFrames (src/Tracking.cc:862-879) for a batch of subjects.  C ABI: include/orbfe.h (covisibility
// section); the argument check, the output bound and the host-side assembly are in covis_plan.h, the staging of the two CSRs,
// which orbfe_redundant_observations takes too, in obs_graph_staging.h.
//
// Two CSRs of indices come up: MapPoint -> slots of the keyframes that observe it, subject -> MapPoints of its keypoints.  One
// workgroup owns one subject and keeps an int32 histogram over observer slots in LDS.  Its lanes stride over the subject's
// entries; a lane walks the observation run of its MapPoint and adds 1 to the observer's bin (an LDS atomic; the returned old
// value tells whether the bin was empty, so the number of non-zero bins is known when the counting ends, without a sweep).
// The workgroup then reserves that many entries of the output arrays with ONE device-scope atomic on a cursor, and writes the
// non-zero bins there in ascending slot order: 256 bins at a time, a ballot and a prefix count per wave, the waves' totals
// through eight words of LDS, a running base per workgroup.  The sweep leaves the bins zero for the next pass.
//
// More keyframes than bins (kCovisSlotsPerPass): the workgroup makes one pass per slot range over its entries and counts only
// the observers that fall in the range; every pass reserves and writes a piece of its own.
//
// Where a piece lands depends on the order in which the workgroups reach the cursor; the host reads (start, count) of every
// piece and copies them into the caller's CSR in subject and slot order (covis_assemble), so the result does not.  The cursor's
// final value is the number of entries needed whether or not they fitted: a piece that does not fit is not written.
//
// No float arithmetic anywhere.
#include "orbfe_matcher_internal.h"

#include "covis_plan.h"
#include "obs_graph_staging.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kSlots = orbfe::kCovisSlotsPerPass;
constexpr int kHead = 16;   // dwords in front of the bins: [0] non-zero bins of the pass, [1] its base, [8..15] wave totals, two buffers

struct CovisParams {
  const int32_t* obsOffs;      // [n_mp + 1], obsOffs[0] == 0
  const int32_t* obsKf;        // [observations] observer slot
  const int32_t* subjSelf;     // [n_subj] slot of the subject or -1
  const int32_t* subjLimit;    // [n_subj] observers with slot >= limit are not counted
  const int32_t* subjOffs;     // [n_subj + 1], subjOffs[0] == 0
  const int32_t* subjMp;       // [entries] MapPoint or -1
  int nPass;
  int bins;                    // bins of the histogram in LDS: min(n_kf, kSlots), at least 1
  unsigned cap;                // entries outKf / outCount hold
  int32_t* outKf;
  int32_t* outCount;
  uint32_t* pieceStart;        // [n_subj * nPass]
  uint32_t* pieceCount;
  unsigned* cursor;            // entries reserved so far (zeroed ahead of the launch)
};

__global__ __launch_bounds__(kThreads) void k_covisibility(CovisParams P) {
  extern __shared__ __align__(16) int32_t lds[];
  int32_t* head = lds;
  int32_t* hist = lds + kHead;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e0 = P.subjOffs[s], e1 = P.subjOffs[s + 1];
  const int self = P.subjSelf[s], limit = P.subjLimit[s];
  for (int b = tid; b < P.bins; b += kThreads) hist[b] = 0;
  if (tid == 0) head[0] = 0;
  __syncthreads();
  for (int pass = 0; pass < P.nPass; pass++) {
    const size_t piece = (size_t)s * (size_t)P.nPass + (size_t)pass;
    const int lo = pass * P.bins;                 // (nPass > 1 only when bins == kSlots)
    if (lo >= limit) {                            // nothing of this range counts (the same for the whole workgroup)
      if (tid == 0) { P.pieceStart[piece] = 0; P.pieceCount[piece] = 0; }
      continue;
    }
    const int nb = min(limit - lo, P.bins), hi = lo + nb;
    int fresh = 0;                                // bins this lane took from 0 to 1
    for (int e = e0 + tid; e < e1; e += kThreads) {
      const int p = P.subjMp[e];
      if (p < 0) continue;
      const int o1 = P.obsOffs[p + 1];
      for (int o = P.obsOffs[p]; o < o1; o++) {
        const int j = P.obsKf[o];
        if (j >= lo && j < hi && j != self) fresh += atomicAdd(&hist[j - lo], 1) == 0;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fresh += __shfl_xor(fresh, o, 64);
    if (lane == 0 && fresh) atomicAdd(&head[0], fresh);
    __syncthreads();
    if (tid == 0) {
      const int total = head[0];
      const unsigned base = total ? atomicAdd(P.cursor, (unsigned)total) : 0u;
      head[1] = (int32_t)base;
      P.pieceStart[piece] = base;
      P.pieceCount[piece] = (uint32_t)total;
    }
    __syncthreads();
    const int total = head[0];
    unsigned running = (unsigned)head[1];
    if (total > 0) {                              // (no bin was touched otherwise: they are all zero still)
      for (int c = 0, it = 0; c < nb; c += kThreads, it++) {
        const int b = c + tid;
        int v = 0;
        if (b < nb) { v = hist[b]; hist[b] = 0; }
        const unsigned long long mask = __ballot(v != 0);
        int32_t* wt = head + 8 + (it & 1) * kWaves;   // two buffers: one barrier per round is enough
        if (lane == 0) wt[wave] = __popcll(mask);
        __syncthreads();
        unsigned before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
          const unsigned t = (unsigned)wt[w];
          if (w < wave) before += t;
          all += t;
        }
        if (v != 0) {
          const unsigned at = running + before + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
          if (at < P.cap) { P.outKf[at] = lo + b; P.outCount[at] = v; }
        }
        running += all;
      }
    }
    __syncthreads();                              // every lane has read head[0] / head[1]
    if (tid == 0) head[0] = 0;
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int orbfe_debug_covis_slots_per_pass(void) { return kSlots; }

int orbfe_debug_covis_ms(const orbfe_matcher* m, double out[3]) {
  return orbfe::ObsGraphScratch::lastMs(m ? &m->covis : nullptr, out);
}

int orbfe_covisibility_counts(orbfe_matcher* m, int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, int n_subj,
                              const int32_t* subj_self, const int32_t* subj_limit, const int32_t* subj_offsets, const int32_t* subj_mp,
                              int32_t* out_offsets, int32_t* out_kf, int32_t* out_count, int cap, int* n_needed) {
  const double tEntry = orbfe_matcher::nowMs();
  if (n_kf < 0 || n_mp < 0 || n_subj < 0 || cap < 0) {
    set_err("covisibility: negative size (n_kf %d, n_mp %d, n_subj %d, cap %d)", n_kf, n_mp, n_subj, cap);
    return ORBFE_ERR_INVALID;
  }
  if (!out_offsets || !n_needed || (cap > 0 && (!out_kf || !out_count))) {
    set_err("covisibility: null pointer (out_offsets, out_kf, out_count or n_needed)");
    return ORBFE_ERR_INVALID;
  }
  if (n_subj == 0) {
    if (!m) { set_err("covisibility: null pointer (matcher)"); return ORBFE_ERR_INVALID; }
    out_offsets[0] = 0;
    *n_needed = 0;
    return ORBFE_OK;
  }
  orbfe::CovisPlan plan;
  if (orbfe::covis_check(n_kf, n_mp, obs_offsets, obs_kf, n_subj, subj_self, subj_limit, subj_offsets, subj_mp, plan)) {
    set_err("covisibility: %s", plan.why);
    return ORBFE_ERR_INVALID;
  }
  if (!m) { set_err("covisibility: null pointer (matcher)"); return ORBFE_ERR_INVALID; }
  HIP_TRY(hipSetDevice(m->device));
  (void)hipGetLastError();
  orbfe::ObsGraphScratch* S = scratch_in<orbfe::ObsGraphScratch>(m->covis);

  // one page-locked arena, one copy up: the graph (obs_graph_stage), then the limit per subject
  const size_t ns = (size_t)n_subj, pieces = ns * (size_t)plan.nPass;
  const unsigned devCap = (unsigned)std::min<uint64_t>((uint64_t)cap, plan.bound);
  orbfe::Arena out;
  const size_t oCursor = out.take(4), oStart = out.take(4 * pieces), oCount = out.take(4 * pieces), headBytes = out.size,
               oKf = out.take(4 * (size_t)devCap + 4), oCnt = out.take(4 * (size_t)devCap + 4), outBytes = out.size;
  orbfe::ObsGraphStaged at;
  int rc;
  if ((rc = orbfe::obs_graph_stage(*S, plan, n_mp, obs_offsets, obs_kf, nullptr, n_subj, subj_self, subj_offsets, subj_mp, nullptr, false, 4 * ns, outBytes, at)))
    return rc;
  uint8_t* H = S->h_in.p;
  int32_t* hl = (int32_t*)(H + at.extra);
  for (int s = 0; s < n_subj; s++) hl[s] = subj_limit ? subj_limit[s] : n_kf;
  const double tStaged = orbfe_matcher::nowMs();
  HIP_TRY(hipMemcpyAsync(S->d_in.p, H, at.bytes, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipMemsetAsync(S->d_out.p + oCursor, 0, 4, m->stream));

  CovisParams P{};
  uint8_t* D = S->d_in.p;
  P.obsOffs = (const int32_t*)(D + at.obsOffs); P.obsKf = (const int32_t*)(D + at.obsKf);
  P.subjSelf = (const int32_t*)(D + at.self); P.subjLimit = (const int32_t*)(D + at.extra);
  P.subjOffs = (const int32_t*)(D + at.subjOffs); P.subjMp = (const int32_t*)(D + at.subjMp);
  P.nPass = plan.nPass;
  P.bins = std::max(1, std::min(n_kf, kSlots));
  P.cap = devCap;
  P.outKf = (int32_t*)(S->d_out.p + oKf); P.outCount = (int32_t*)(S->d_out.p + oCnt);
  P.pieceStart = (uint32_t*)(S->d_out.p + oStart); P.pieceCount = (uint32_t*)(S->d_out.p + oCount);
  P.cursor = (unsigned*)(S->d_out.p + oCursor);
  const size_t lds = 4 * ((size_t)kHead + (size_t)P.bins);
  if (lds > 64 * 1024 && !S->ldsAttr) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_covisibility), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (kHead + kSlots)));
    S->ldsAttr = true;
  }
  HIP_TRY(hipEventRecord(S->t0, m->stream));
  hipLaunchKernelGGL(k_covisibility, dim3(n_subj), dim3(kThreads), lds, m->stream, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(S->t1, m->stream));
  // down: the cursor and the pieces first, then exactly the entries that were written
  HIP_TRY(hipMemcpyAsync(S->h_out.p, S->d_out.p, headBytes, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  float kernelMs = 0.0f;
  HIP_TRY(hipEventElapsedTime(&kernelMs, S->t0, S->t1));
  const uint32_t needed = *(const uint32_t*)(S->h_out.p + oCursor);
  *n_needed = (int)needed;
  S->ms[0] = tStaged - tEntry;
  S->ms[1] = kernelMs;
  if (needed > (uint32_t)cap) {
    S->ms[2] = orbfe_matcher::nowMs() - tEntry;
    set_err("covisibility: %u entries needed, cap is %d", needed, cap);
    return ORBFE_ERR_OVERFLOW;
  }
  if (needed) {
    HIP_TRY(hipMemcpyAsync(S->h_out.p + oKf, S->d_out.p + oKf, 4 * (size_t)needed, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(S->h_out.p + oCnt, S->d_out.p + oCnt, 4 * (size_t)needed, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  if (orbfe::covis_assemble(n_subj, plan.nPass, (const uint32_t*)(S->h_out.p + oStart), (const uint32_t*)(S->h_out.p + oCount),
                            (const int32_t*)(S->h_out.p + oKf), (const int32_t*)(S->h_out.p + oCnt), needed, out_offsets, out_kf, out_count)) {
    set_err("covisibility: the kernel's pieces do not add up to its cursor (%u)", needed);
    return ORBFE_ERR_HIP;
  }
  S->ms[2] = orbfe_matcher::nowMs() - tEntry;
  return ORBFE_OK;
}

}  // extern "C"
