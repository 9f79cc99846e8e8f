// culling_plan.h -- the host-side bookkeeping of orbfe_redundant_observations (orbfe_culling.hip), free of HIP so that a plain host
// program can exercise it (tests/cpp/culling_plan_test.cpp, also under the address and undefined-behaviour sanitizers): the
// argument check of the two CSRs (MapPoint -> observer slots and levels, subject -> MapPoints and levels) before anything is sent,
// and the bases and lengths the staging copies by.  The CSRs are those of covis_plan.h; the level bytes, mp_nobs and th_obs are new.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace orbfe {

constexpr int kCullingOk = 0, kCullingInvalid = -1;   // ORBFE_OK, ORBFE_ERR_INVALID

// An observation list longer than this is walked by a whole wave, a shorter one by the lane of its entry (k_redundant_observations).
constexpr int kCullingLongList = 64;

struct CullingPlan {
  int32_t obsBase = 0, subjBase = 0;   // offsets[0] of the two CSRs (the arrays are sent rebased to 0)
  size_t nObs = 0, nEntries = 0;
  char why[160] = {0};                 // what a kCullingInvalid return objects to
};

inline int culling_refuse(CullingPlan& plan, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
  std::snprintf(plan.why, sizeof plan.why, fmt, a, b, c);
  return kCullingInvalid;
}

// Everything the C call refuses with ORBFE_ERR_INVALID, in the order of the header's list; n_subj == 0 and the output pointers
// are checked by the caller.  mp_nobs may be null (the CSR's length per MapPoint then).
inline int culling_check(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, const int32_t* mp_nobs,
                         int n_subj, const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level,
                         int th_obs, CullingPlan& plan) {
  plan = CullingPlan();
  if (n_kf < 0 || n_mp < 0 || n_subj < 0) return culling_refuse(plan, "negative size (n_kf %lld, n_mp %lld, n_subj %lld)", n_kf, n_mp, n_subj);
  if (th_obs < 1) return culling_refuse(plan, "th_obs = %lld is below 1", th_obs);
  if (!obs_offsets || !subj_self || !subj_offsets) return culling_refuse(plan, "null pointer (obs_offsets, subj_self or subj_offsets)");
  if (obs_offsets[0] < 0) return culling_refuse(plan, "obs_offsets[0] = %lld is negative", obs_offsets[0]);
  for (int p = 0; p < n_mp; p++)
    if (obs_offsets[p + 1] < obs_offsets[p]) return culling_refuse(plan, "obs_offsets decreases at MapPoint %lld (%lld after %lld)", p, obs_offsets[p + 1], obs_offsets[p]);
  plan.obsBase = obs_offsets[0];
  plan.nObs = (size_t)(obs_offsets[n_mp] - obs_offsets[0]);
  if (plan.nObs && (!obs_kf || !obs_level)) return culling_refuse(plan, "null pointer (obs_kf or obs_level, with %lld observations)", (long long)plan.nObs);
  if (subj_offsets[0] < 0) return culling_refuse(plan, "subj_offsets[0] = %lld is negative", subj_offsets[0]);
  for (int s = 0; s < n_subj; s++)
    if (subj_offsets[s + 1] < subj_offsets[s]) return culling_refuse(plan, "subj_offsets decreases at subject %lld (%lld after %lld)", s, subj_offsets[s + 1], subj_offsets[s]);
  plan.subjBase = subj_offsets[0];
  plan.nEntries = (size_t)(subj_offsets[n_subj] - subj_offsets[0]);
  if (plan.nEntries && (!subj_mp || !subj_level)) return culling_refuse(plan, "null pointer (subj_mp or subj_level, with %lld entries)", (long long)plan.nEntries);
  for (size_t o = 0; o < plan.nObs; o++) {
    const int32_t j = obs_kf[plan.obsBase + o];
    if (j < 0 || j >= n_kf) return culling_refuse(plan, "obs_kf[%lld] = %lld outside [0, %lld)", (long long)(plan.obsBase + o), j, n_kf);
  }
  for (size_t e = 0; e < plan.nEntries; e++) {
    const int32_t p = subj_mp[plan.subjBase + e];
    if (p < -1 || p >= n_mp) return culling_refuse(plan, "subj_mp[%lld] = %lld outside [-1, %lld)", (long long)(plan.subjBase + e), p, n_mp);
  }
  for (int s = 0; s < n_subj; s++)
    if (subj_self[s] < -1 || subj_self[s] >= n_kf) return culling_refuse(plan, "subj_self[%lld] = %lld outside [-1, %lld)", s, subj_self[s], n_kf);
  if (mp_nobs)
    for (int p = 0; p < n_mp; p++)
      if (mp_nobs[p] < 0) return culling_refuse(plan, "mp_nobs[%lld] = %lld is negative", p, mp_nobs[p]);
  return kCullingOk;
}

}  // namespace orbfe
