// ransac_plan.h -- the host-side argument check of orbfe_score_sim3_hypotheses / orbfe_score_pnp_hypotheses / orbfe_ransac_mask_words
// (orbfe_ransac.hip), free of HIP so that a plain host program can exercise it (tests/cpp/ransac_plan_test.cpp, also under the
// address and undefined-behaviour sanitizers).  A call scores n_hyp hypotheses that belong to n_seg segments (solvers): segment s
// owns the correspondences [seg_off[s], seg_off[s + 1]) and hypothesis k belongs to segment hyp_seg[k].  The kernel reads hyp_seg,
// the rebased seg_off and the packed word offsets as indices without looking again: every range test on them is here, once.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace orbfe {

constexpr int kRansacOk = 0, kRansacInvalid = -1;     // ORBFE_OK, ORBFE_ERR_INVALID
constexpr int kRansacSim3Row = 12, kRansacPnPRow = 6;   // floats of one correspondence as the caller passes it
constexpr int64_t kRansacMaxCorr = 0x7fffffff / 12;   // correspondences of one call: 12 * N is an int32 index of corr
constexpr int64_t kRansacMaxWords = 0x7fffffff;       // mask words of one call

struct RansacPlan {
  int32_t base = 0;      // seg_off[0]: the arrays are sent rebased to 0
  int64_t nCorr = 0;     // seg_off[n_seg] - seg_off[0]
  int64_t words = 0;     // sum over the hypotheses of ceil(N of its segment / 64)
  char why[160] = {0};   // what a kRansacInvalid return objects to
};

inline int ransac_refuse(RansacPlan& plan, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
  std::snprintf(plan.why, sizeof plan.why, fmt, a, b, c);
  return kRansacInvalid;
}

// mask words of one hypothesis over n correspondences
inline int64_t ransac_words_of(int64_t n) { return (n + 63) / 64; }

// The layout: sizes, seg_off, hyp_seg and the two totals.  Everything orbfe_ransac_mask_words needs and refuses.
inline int ransac_check_layout(int n_seg, const int32_t* seg_off, int n_hyp, const int32_t* hyp_seg, RansacPlan& plan) {
  plan = RansacPlan();
  if (n_seg < 1) return ransac_refuse(plan, "n_seg = %lld (at least one segment)", n_seg);
  if (n_hyp < 1) return ransac_refuse(plan, "n_hyp = %lld (at least one hypothesis)", n_hyp);
  if (!seg_off || !hyp_seg) return ransac_refuse(plan, "null pointer (seg_off or hyp_seg)");
  if (seg_off[0] < 0) return ransac_refuse(plan, "seg_off[0] = %lld is negative", seg_off[0]);
  for (int s = 0; s < n_seg; s++)
    if (seg_off[s + 1] < seg_off[s]) return ransac_refuse(plan, "seg_off decreases at segment %lld (%lld after %lld)", s, seg_off[s + 1], seg_off[s]);
  plan.base = seg_off[0];
  plan.nCorr = (int64_t)seg_off[n_seg] - (int64_t)seg_off[0];
  if (plan.nCorr > kRansacMaxCorr) return ransac_refuse(plan, "%lld correspondences in one call (max %lld)", plan.nCorr, kRansacMaxCorr);
  for (int k = 0; k < n_hyp; k++) {
    const int32_t s = hyp_seg[k];
    if (s < 0 || s >= n_seg) return ransac_refuse(plan, "hyp_seg[%lld] = %lld outside [0, %lld)", k, s, n_seg);
    plan.words += ransac_words_of((int64_t)seg_off[s + 1] - (int64_t)seg_off[s]);
    if (plan.words > kRansacMaxWords) return ransac_refuse(plan, "the hypotheses up to %lld hold more than %lld mask words", k, kRansacMaxWords);
  }
  return kRansacOk;
}

// Everything the two scoring calls refuse with ORBFE_ERR_INVALID, in the order of the header's list; the matcher itself is the
// caller's.  corr / cams / hyp_a / hyp_b: the call's payload arrays (hyp_b only where the model has one, else pass hyp_a twice).
// mask_off may be null (packed); its entries matter only where masks are asked for.
inline int ransac_check(int n_seg, const int32_t* seg_off, const void* corr, const void* cams, int n_hyp, const int32_t* hyp_seg, const void* hyp_a,
                        const void* hyp_b, const int64_t* mask_off, bool wantMasks, RansacPlan& plan) {
  if (ransac_check_layout(n_seg, seg_off, n_hyp, hyp_seg, plan)) return kRansacInvalid;
  if (!cams || !hyp_a || !hyp_b) return ransac_refuse(plan, "null pointer (cameras or hypotheses)");
  if (plan.nCorr && !corr) return ransac_refuse(plan, "null pointer (corr, with %lld correspondences)", plan.nCorr);
  if (wantMasks && mask_off)
    for (int k = 0; k < n_hyp; k++)
      if (mask_off[k] < 0) return ransac_refuse(plan, "mask_off[%lld] = %lld is negative", k, mask_off[k]);
  return kRansacOk;
}

// Where hypothesis k's words start when they are packed one after the other: out[k], k < n_hyp.  After a passed check.
inline void ransac_packed_offsets(const int32_t* seg_off, int n_hyp, const int32_t* hyp_seg, int64_t* out) {
  int64_t at = 0;
  for (int k = 0; k < n_hyp; k++) {
    out[k] = at;
    at += ransac_words_of((int64_t)seg_off[hyp_seg[k] + 1] - (int64_t)seg_off[hyp_seg[k]]);
  }
}

}  // namespace orbfe
