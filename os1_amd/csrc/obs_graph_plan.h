// obs_graph_plan.h -- the argument check of the observation graph that orbfe_covisibility_counts (covis_plan.h, orbfe_covis.hip) and
// orbfe_redundant_observations (culling_plan.h, orbfe_culling.hip) both take, free of HIP so that a plain host program can
// exercise it (tests/cpp/covis_plan_test.cpp, tests/cpp/culling_plan_test.cpp, also under the address and undefined-behaviour
// sanitizers).  The graph is two CSRs -- MapPoint -> observer slots, subject -> MapPoints, with a `self` slot per subject --
// and, where the call asks for them, a level byte per observation and per entry.  A kernel reads obs_kf, subj_mp and subj_self
// as indices without looking again: every range test on them is here, once.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace orbfe {

constexpr int kPlanOk = 0, kPlanInvalid = -1;   // ORBFE_OK, ORBFE_ERR_INVALID

struct ObsGraphPlan {
  int32_t obsBase = 0, subjBase = 0;   // offsets[0] of the two CSRs (the arrays are sent rebased to 0)
  size_t nObs = 0, nEntries = 0;
  char why[160] = {0};                 // what a kPlanInvalid return objects to
};

inline int plan_refuse(ObsGraphPlan& plan, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
  std::snprintf(plan.why, sizeof plan.why, fmt, a, b, c);
  return kPlanInvalid;
}

// Everything both C calls refuse with ORBFE_ERR_INVALID, in the order of the header's lists, and the bases and lengths the
// staging copies by.  levels: obs_level / subj_level belong to the call and must come with a non-empty CSR.  perSubject(s) runs
// after subj_self[s] has passed and refuses (non-zero, plan.why set) what else the call holds per subject.  The caller resets
// the plan; n_subj == 0 and the output pointers are its business too.
template <class PerSubject>
inline int obs_graph_check(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, int n_subj,
                           const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level, bool levels,
                           ObsGraphPlan& plan, PerSubject&& perSubject) {
  if (!obs_offsets || !subj_self || !subj_offsets) return plan_refuse(plan, "null pointer (obs_offsets, subj_self or subj_offsets)");
  if (obs_offsets[0] < 0) return plan_refuse(plan, "obs_offsets[0] = %lld is negative", obs_offsets[0]);
  for (int p = 0; p < n_mp; p++)
    if (obs_offsets[p + 1] < obs_offsets[p]) return plan_refuse(plan, "obs_offsets decreases at MapPoint %lld (%lld after %lld)", p, obs_offsets[p + 1], obs_offsets[p]);
  plan.obsBase = obs_offsets[0];
  plan.nObs = (size_t)(obs_offsets[n_mp] - obs_offsets[0]);
  if (plan.nObs && (!obs_kf || (levels && !obs_level)))
    return plan_refuse(plan, levels ? "null pointer (obs_kf or obs_level, with %lld observations)" : "null pointer (obs_kf, with %lld observations)", (long long)plan.nObs);
  if (subj_offsets[0] < 0) return plan_refuse(plan, "subj_offsets[0] = %lld is negative", subj_offsets[0]);
  for (int s = 0; s < n_subj; s++)
    if (subj_offsets[s + 1] < subj_offsets[s]) return plan_refuse(plan, "subj_offsets decreases at subject %lld (%lld after %lld)", s, subj_offsets[s + 1], subj_offsets[s]);
  plan.subjBase = subj_offsets[0];
  plan.nEntries = (size_t)(subj_offsets[n_subj] - subj_offsets[0]);
  if (plan.nEntries && (!subj_mp || (levels && !subj_level)))
    return plan_refuse(plan, levels ? "null pointer (subj_mp or subj_level, with %lld entries)" : "null pointer (subj_mp, with %lld entries)", (long long)plan.nEntries);
  for (size_t o = 0; o < plan.nObs; o++) {
    const int32_t j = obs_kf[plan.obsBase + o];
    if (j < 0 || j >= n_kf) return plan_refuse(plan, "obs_kf[%lld] = %lld outside [0, %lld)", (long long)(plan.obsBase + o), j, n_kf);
  }
  for (size_t e = 0; e < plan.nEntries; e++) {
    const int32_t p = subj_mp[plan.subjBase + e];
    if (p < -1 || p >= n_mp) return plan_refuse(plan, "subj_mp[%lld] = %lld outside [-1, %lld)", (long long)(plan.subjBase + e), p, n_mp);
  }
  for (int s = 0; s < n_subj; s++) {
    if (subj_self[s] < -1 || subj_self[s] >= n_kf) return plan_refuse(plan, "subj_self[%lld] = %lld outside [-1, %lld)", s, subj_self[s], n_kf);
    if (perSubject(s)) return kPlanInvalid;
  }
  return kPlanOk;
}

}  // namespace orbfe
