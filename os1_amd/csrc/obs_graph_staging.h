// obs_graph_staging.h -- what orbfe_covisibility_counts (orbfe_covis.hip) and orbfe_redundant_observations (orbfe_culling.hip) do
// alike between the argument check (obs_graph_plan.h) and the launch: the scratch of a call, and the one page-locked arena that
// takes the observation graph up in one copy.  Each call keeps a scratch of its own on the matcher (m->covis, m->culling), so
// neither's timings nor buffer growth depend on the other.
#pragma once
#include <cstring>
#include <memory>

#include "hip_buffers.h"
#include "obs_graph_plan.h"

namespace orbfe {

// parts of an arena, one after the other, each on a 256-byte boundary
struct Arena {
  size_t size = 0;
  size_t take(size_t bytes) { const size_t at = size; size += al(bytes); return at; }
};

struct ObsGraphScratch {
  DevBuf<uint8_t> d_in, d_out;
  PinBuf<uint8_t> h_in, h_out;
  hipEvent_t t0 = nullptr, t1 = nullptr;   // around the launch
  bool ldsAttr = false;                    // k_covisibility has been allowed its dynamic LDS above 64 KiB
  double ms[3] = {0, 0, 0};                // check + staging on the host, kernel, the whole call
  ~ObsGraphScratch() {
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    d_in.release(); d_out.release(); h_in.release(); h_out.release();
    (void)hipGetLastError();
  }
  static int lastMs(const std::shared_ptr<void>* slot, double out[3]) {      // zeros before the first call; slot is null where the matcher was
    if (!slot || !out) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
    const ObsGraphScratch* S = static_cast<const ObsGraphScratch*>(slot->get());
    for (int k = 0; k < 3; k++) out[k] = S ? S->ms[k] : 0.0;
    return ORBFE_OK;
  }
};

// where the arrays lie in h_in and, after the copy of `bytes`, in d_in; the levels only where asked for, extra for the caller to fill
struct ObsGraphStaged {
  size_t obsOffs = 0, obsKf = 0, obsLevel = 0, self = 0, subjOffs = 0, subjMp = 0, subjLevel = 0, extra = 0, bytes = 0;
};

// Sizes the upload arena (the graph, then extraBytes), grows the four buffers (outBytes for the two of the way down), makes the
// events on first use, and writes the checked graph into h_in: both offset arrays rebased to 0, the payload from its base on.
inline int obs_graph_stage(ObsGraphScratch& S, const ObsGraphPlan& plan, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf,
                           const uint8_t* obs_level, int n_subj, const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp,
                           const uint8_t* subj_level, bool levels, size_t extraBytes, size_t outBytes, ObsGraphStaged& at) {
  Arena in;
  const size_t ns = (size_t)n_subj;
  at.obsOffs = in.take(4 * ((size_t)n_mp + 1));
  at.obsKf = in.take(4 * plan.nObs + 4);
  if (levels) at.obsLevel = in.take(plan.nObs + 4);
  at.self = in.take(4 * ns);
  at.subjOffs = in.take(4 * (ns + 1));
  at.subjMp = in.take(4 * plan.nEntries + 4);
  if (levels) at.subjLevel = in.take(plan.nEntries + 4);
  at.extra = in.take(extraBytes);
  at.bytes = in.size;
  int rc;
  if ((rc = S.h_in.ensure(at.bytes)) || (rc = S.d_in.ensure(at.bytes)) || (rc = S.h_out.ensure(outBytes)) || (rc = S.d_out.ensure(outBytes))) return rc;
  if (!S.t0) {
    HIP_TRY(hipEventCreate(&S.t0));
    HIP_TRY(hipEventCreate(&S.t1));
  }
  uint8_t* H = S.h_in.p;
  int32_t* ho = (int32_t*)(H + at.obsOffs);
  for (int p = 0; p <= n_mp; p++) ho[p] = obs_offsets[p] - plan.obsBase;
  if (plan.nObs) memcpy(H + at.obsKf, obs_kf + plan.obsBase, 4 * plan.nObs);
  if (plan.nObs && levels) memcpy(H + at.obsLevel, obs_level + plan.obsBase, plan.nObs);
  memcpy(H + at.self, subj_self, 4 * ns);
  int32_t* hs = (int32_t*)(H + at.subjOffs);
  for (int s = 0; s <= n_subj; s++) hs[s] = subj_offsets[s] - plan.subjBase;
  if (plan.nEntries) memcpy(H + at.subjMp, subj_mp + plan.subjBase, 4 * plan.nEntries);
  if (plan.nEntries && levels) memcpy(H + at.subjLevel, subj_level + plan.subjBase, plan.nEntries);
  return ORBFE_OK;
}

}  // namespace orbfe
