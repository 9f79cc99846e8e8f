// covis_plan.h -- the host-side bookkeeping of orbfe_covisibility_counts (orbfe_covis.hip), free of HIP so that a plain host
// program can exercise it (tests/cpp/covis_plan_test.cpp, also under the address and undefined-behaviour sanitizers):
//   * the argument check of the two CSRs (MapPoint -> observer slots, subject -> MapPoints) before anything is sent, and the
//     bound on the number of output entries that sizes the device buffers;
//   * how many slot ranges ("passes") k_covisibility walks, and how the host puts the pieces the workgroups wrote -- one per
//     (subject, pass), wherever the workgroup's reservation landed -- into the caller's CSR in subject and slot order.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace orbfe {

constexpr int kCovisOk = 0, kCovisInvalid = -1, kCovisOverflow = -5;   // ORBFE_OK, ORBFE_ERR_INVALID, ORBFE_ERR_OVERFLOW

// Observer slots one pass of k_covisibility counts: an int32 histogram of 16 384 bins is 64 KiB of the CU's 160 KiB of LDS, so
// two workgroups (64 KiB + 40 bytes of bookkeeping each) are resident per CU whatever n_kf is, and a third does not fit.
// A map of fewer keyframes asks for n_kf bins only.
constexpr int kCovisSlotsPerPass = 16384;
constexpr uint64_t kCovisMaxEntries = 0x7fffffffull;     // n_needed is an int
constexpr uint64_t kCovisMaxPieces = 1ull << 28;         // (subject, pass) records of one call

struct CovisPlan {
  int nPass = 1;              // slot ranges of kCovisSlotsPerPass the kernel walks (>= 1)
  uint64_t bound = 0;         // sum over the subjects of min(limit, observations reachable): no call needs more entries
  int32_t obsBase = 0, subjBase = 0;   // offsets[0] of the two CSRs (the arrays are sent rebased to 0)
  size_t nObs = 0, nEntries = 0;
  char why[160] = {0};        // what a kCovisInvalid return objects to
};

inline int covis_refuse(CovisPlan& plan, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
  std::snprintf(plan.why, sizeof plan.why, fmt, a, b, c);
  return kCovisInvalid;
}

// Everything the C call refuses with ORBFE_ERR_INVALID, in the order of the header's list; n_subj == 0 is checked by the caller
// after the sizes.  The output pointers are the caller's business too.
inline int covis_check(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, int n_subj, const int32_t* subj_self,
                       const int32_t* subj_limit, const int32_t* subj_offsets, const int32_t* subj_mp, CovisPlan& plan) {
  plan = CovisPlan();
  if (n_kf < 0 || n_mp < 0 || n_subj < 0) return covis_refuse(plan, "negative size (n_kf %lld, n_mp %lld, n_subj %lld)", n_kf, n_mp, n_subj);
  if (!obs_offsets || !subj_self || !subj_offsets) return covis_refuse(plan, "null pointer (obs_offsets, subj_self or subj_offsets)");
  if (obs_offsets[0] < 0) return covis_refuse(plan, "obs_offsets[0] = %lld is negative", obs_offsets[0]);
  for (int p = 0; p < n_mp; p++)
    if (obs_offsets[p + 1] < obs_offsets[p]) return covis_refuse(plan, "obs_offsets decreases at MapPoint %lld (%lld after %lld)", p, obs_offsets[p + 1], obs_offsets[p]);
  plan.obsBase = obs_offsets[0];
  plan.nObs = (size_t)(obs_offsets[n_mp] - obs_offsets[0]);
  if (plan.nObs && !obs_kf) return covis_refuse(plan, "null pointer (obs_kf, with %lld observations)", (long long)plan.nObs);
  if (subj_offsets[0] < 0) return covis_refuse(plan, "subj_offsets[0] = %lld is negative", subj_offsets[0]);
  for (int s = 0; s < n_subj; s++)
    if (subj_offsets[s + 1] < subj_offsets[s]) return covis_refuse(plan, "subj_offsets decreases at subject %lld (%lld after %lld)", s, subj_offsets[s + 1], subj_offsets[s]);
  plan.subjBase = subj_offsets[0];
  plan.nEntries = (size_t)(subj_offsets[n_subj] - subj_offsets[0]);
  if (plan.nEntries && !subj_mp) return covis_refuse(plan, "null pointer (subj_mp, with %lld entries)", (long long)plan.nEntries);
  for (size_t o = 0; o < plan.nObs; o++) {
    const int32_t j = obs_kf[plan.obsBase + o];
    if (j < 0 || j >= n_kf) return covis_refuse(plan, "obs_kf[%lld] = %lld outside [0, %lld)", (long long)(plan.obsBase + o), j, n_kf);
  }
  for (size_t e = 0; e < plan.nEntries; e++) {
    const int32_t p = subj_mp[plan.subjBase + e];
    if (p < -1 || p >= n_mp) return covis_refuse(plan, "subj_mp[%lld] = %lld outside [-1, %lld)", (long long)(plan.subjBase + e), p, n_mp);
  }
  for (int s = 0; s < n_subj; s++) {
    if (subj_self[s] < -1 || subj_self[s] >= n_kf) return covis_refuse(plan, "subj_self[%lld] = %lld outside [-1, %lld)", s, subj_self[s], n_kf);
    if (subj_limit && (subj_limit[s] < 0 || subj_limit[s] > n_kf)) return covis_refuse(plan, "subj_limit[%lld] = %lld outside [0, %lld]", s, subj_limit[s], n_kf);
  }
  plan.nPass = std::max(1, (int)(((int64_t)n_kf + kCovisSlotsPerPass - 1) / kCovisSlotsPerPass));
  if ((uint64_t)n_subj * (uint64_t)plan.nPass > kCovisMaxPieces)
    return covis_refuse(plan, "%lld subjects x %lld slot ranges are more than one call takes", n_subj, plan.nPass);
  uint64_t bound = 0;
  for (int s = 0; s < n_subj; s++) {
    uint64_t reach = 0;
    for (int32_t e = subj_offsets[s]; e < subj_offsets[s + 1]; e++)
      if (subj_mp[e] >= 0) reach += (uint64_t)(obs_offsets[subj_mp[e] + 1] - obs_offsets[subj_mp[e]]);
    bound += std::min<uint64_t>(reach, (uint64_t)(subj_limit ? subj_limit[s] : n_kf));
  }
  if (bound > kCovisMaxEntries) return covis_refuse(plan, "up to %lld output entries are more than one call takes", (long long)bound);
  plan.bound = bound;
  return kCovisOk;
}

// The pieces as the kernel left them -- piece (s, pass) holds pieceCount entries from pieceStart on in devKf / devCount, in
// ascending slot order, and the passes of a subject ascend too -- into the caller's CSR.  nNeeded is the kernel's cursor.
// kCovisInvalid if a piece lies outside [0, nNeeded) or the pieces do not add up to it (a kernel fault, never an argument's).
inline int covis_assemble(int n_subj, int nPass, const uint32_t* pieceStart, const uint32_t* pieceCount, const int32_t* devKf,
                          const int32_t* devCount, uint32_t nNeeded, int32_t* out_offsets, int32_t* out_kf, int32_t* out_count) {
  uint64_t at = 0;
  for (int s = 0; s < n_subj; s++) {
    out_offsets[s] = (int32_t)at;
    for (int q = 0; q < nPass; q++) {
      const size_t r = (size_t)s * (size_t)nPass + (size_t)q;
      const uint64_t c = pieceCount[r], b = pieceStart[r];
      if (c == 0) continue;
      if (b + c > nNeeded || at + c > nNeeded) return kCovisInvalid;
      std::memcpy(out_kf + at, devKf + b, 4 * (size_t)c);
      std::memcpy(out_count + at, devCount + b, 4 * (size_t)c);
      at += c;
    }
  }
  out_offsets[n_subj] = (int32_t)at;
  return at == nNeeded ? kCovisOk : kCovisInvalid;
}

}  // namespace orbfe
