// covis_plan.h -- the host-side bookkeeping of orbfe_covisibility_counts (orbfe_covis.hip), free of HIP so that a plain host
// program can exercise it (tests/cpp/covis_plan_test.cpp, also under the address and undefined-behaviour sanitizers):
//   * the argument check before anything is sent -- the two CSRs are obs_graph_plan.h's, subj_limit and the limits of one call
//     are this call's own -- and the bound on the number of output entries that sizes the device buffers;
//   * how many slot ranges ("passes") k_covisibility walks, and how the host puts the pieces the workgroups wrote -- one per
//     (subject, pass), wherever the workgroup's reservation landed -- into the caller's CSR in subject and slot order.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "obs_graph_plan.h"

namespace orbfe {

// Observer slots one pass of k_covisibility counts: an int32 histogram of 16 384 bins is 64 KiB of the CU's 160 KiB of LDS, so
// two workgroups (64 KiB + 40 bytes of bookkeeping each) are resident per CU whatever n_kf is, and a third does not fit.
// A map of fewer keyframes asks for n_kf bins only.
constexpr int kCovisSlotsPerPass = 16384;
constexpr uint64_t kCovisMaxEntries = 0x7fffffffull;     // n_needed is an int
constexpr uint64_t kCovisMaxPieces = 1ull << 28;         // (subject, pass) records of one call

struct CovisPlan : ObsGraphPlan {
  int nPass = 1;              // slot ranges of kCovisSlotsPerPass the kernel walks (>= 1)
  uint64_t bound = 0;         // sum over the subjects of min(limit, observations reachable): no call needs more entries
};

// Everything the C call refuses with ORBFE_ERR_INVALID, in the order of the header's list: the sizes, the graph with subj_limit[s]
// right after subj_self[s] (obs_graph_check), the two limits of one call.  n_subj == 0 is checked by the caller after the sizes.
// The output pointers are the caller's business too.
inline int covis_check(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, int n_subj, const int32_t* subj_self,
                       const int32_t* subj_limit, const int32_t* subj_offsets, const int32_t* subj_mp, CovisPlan& plan) {
  plan = CovisPlan();
  if (n_kf < 0 || n_mp < 0 || n_subj < 0) return plan_refuse(plan, "negative size (n_kf %lld, n_mp %lld, n_subj %lld)", n_kf, n_mp, n_subj);
  const auto limitOf = [&](int s) {
    if (subj_limit && (subj_limit[s] < 0 || subj_limit[s] > n_kf)) return plan_refuse(plan, "subj_limit[%lld] = %lld outside [0, %lld]", s, subj_limit[s], n_kf);
    return kPlanOk;
  };
  if (obs_graph_check(n_kf, n_mp, obs_offsets, obs_kf, nullptr, n_subj, subj_self, subj_offsets, subj_mp, nullptr, false, plan, limitOf)) return kPlanInvalid;
  plan.nPass = std::max(1, (int)(((int64_t)n_kf + kCovisSlotsPerPass - 1) / kCovisSlotsPerPass));
  if ((uint64_t)n_subj * (uint64_t)plan.nPass > kCovisMaxPieces)
    return plan_refuse(plan, "%lld subjects x %lld slot ranges are more than one call takes", n_subj, plan.nPass);
  uint64_t bound = 0;
  for (int s = 0; s < n_subj; s++) {
    uint64_t reach = 0;
    for (int32_t e = subj_offsets[s]; e < subj_offsets[s + 1]; e++)
      if (subj_mp[e] >= 0) reach += (uint64_t)(obs_offsets[subj_mp[e] + 1] - obs_offsets[subj_mp[e]]);
    bound += std::min<uint64_t>(reach, (uint64_t)(subj_limit ? subj_limit[s] : n_kf));
  }
  if (bound > kCovisMaxEntries) return plan_refuse(plan, "up to %lld output entries are more than one call takes", (long long)bound);
  plan.bound = bound;
  return kPlanOk;
}

// The pieces as the kernel left them -- piece (s, pass) holds pieceCount entries from pieceStart on in devKf / devCount, in
// ascending slot order, and the passes of a subject ascend too -- into the caller's CSR.  nNeeded is the kernel's cursor.
// kPlanInvalid if a piece lies outside [0, nNeeded) or the pieces do not add up to it (a kernel fault, never an argument's).
inline int covis_assemble(int n_subj, int nPass, const uint32_t* pieceStart, const uint32_t* pieceCount, const int32_t* devKf,
                          const int32_t* devCount, uint32_t nNeeded, int32_t* out_offsets, int32_t* out_kf, int32_t* out_count) {
  uint64_t at = 0;
  for (int s = 0; s < n_subj; s++) {
    out_offsets[s] = (int32_t)at;
    for (int q = 0; q < nPass; q++) {
      const size_t r = (size_t)s * (size_t)nPass + (size_t)q;
      const uint64_t c = pieceCount[r], b = pieceStart[r];
      if (c == 0) continue;
      if (b + c > nNeeded || at + c > nNeeded) return kPlanInvalid;
      std::memcpy(out_kf + at, devKf + b, 4 * (size_t)c);
      std::memcpy(out_count + at, devCount + b, 4 * (size_t)c);
      at += c;
    }
  }
  out_offsets[n_subj] = (int32_t)at;
  return at == nNeeded ? kPlanOk : kPlanInvalid;
}

}  // namespace orbfe
