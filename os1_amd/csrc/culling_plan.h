// culling_plan.h -- the host-side argument check of orbfe_redundant_observations (orbfe_culling.hip), free of HIP so that a plain host
// program can exercise it (tests/cpp/culling_plan_test.cpp, also under the address and undefined-behaviour sanitizers).  The two
// CSRs and their level bytes are obs_graph_plan.h's; th_obs and mp_nobs are this call's own.
#pragma once
#include "obs_graph_plan.h"

namespace orbfe {

// An observation list longer than this is walked by a whole wave, a shorter one by the lane of its entry (k_redundant_observations).
constexpr int kCullingLongList = 64;

typedef ObsGraphPlan CullingPlan;

// Everything the C call refuses with ORBFE_ERR_INVALID, in the order of the header's list: the sizes, th_obs, the graph
// (obs_graph_check), mp_nobs; n_subj == 0 and the output pointers are checked by the caller.  mp_nobs may be null (the CSR's
// length per MapPoint then).
inline int culling_check(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, const int32_t* mp_nobs,
                         int n_subj, const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level,
                         int th_obs, CullingPlan& plan) {
  plan = CullingPlan();
  if (n_kf < 0 || n_mp < 0 || n_subj < 0) return plan_refuse(plan, "negative size (n_kf %lld, n_mp %lld, n_subj %lld)", n_kf, n_mp, n_subj);
  if (th_obs < 1) return plan_refuse(plan, "th_obs = %lld is below 1", th_obs);
  if (obs_graph_check(n_kf, n_mp, obs_offsets, obs_kf, obs_level, n_subj, subj_self, subj_offsets, subj_mp, subj_level, true, plan,
                      [](int) { return kPlanOk; }))
    return kPlanInvalid;
  if (mp_nobs)
    for (int p = 0; p < n_mp; p++)
      if (mp_nobs[p] < 0) return plan_refuse(plan, "mp_nobs[%lld] = %lld is negative", p, mp_nobs[p]);
  return kPlanOk;
}

}  // namespace orbfe
