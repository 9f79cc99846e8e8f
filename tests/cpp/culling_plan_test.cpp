// os1_amd/csrc/culling_plan.h as a program of its own (no HIP, no GPU): every refusal of the argument check with its whole message,
// which of two faults is reported, empty and rebased CSRs, and what the check leaves to the caller (n_subj == 0).  Built plainly and with
// -fsanitize=address,undefined by tests/test_keyframe_culling.py: the arrays below are exactly as long as the call may read.
#include <cstdio>
#include <cstring>
#include <vector>

#include "culling_plan.h"

using namespace orbfe;

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

namespace {
struct Args {
  int n_kf = 5, n_mp = 3, n_subj = 3, th_obs = 3;
  std::vector<int32_t> obsOffs{0, 2, 2, 5}, obsKf{0, 4, 1, 2, 3}, nobs{2, 0, 7};      // MapPoint 1 has no observation
  std::vector<uint8_t> obsLevel{0, 255, 1, 2, 3};
  std::vector<int32_t> self{0, -1, 4}, subjOffs{0, 3, 3, 5}, subjMp{0, -1, 2, 2, 2};
  std::vector<uint8_t> subjLevel{0, 0, 7, 255, 1};
  bool withNobs = true;
  int check(CullingPlan& plan) const {
    return culling_check(n_kf, n_mp, obsOffs.data(), obsKf.data(), obsLevel.data(), withNobs ? nobs.data() : nullptr, n_subj, self.data(), subjOffs.data(),
                         subjMp.data(), subjLevel.data(), th_obs, plan);
  }
};
constexpr int kOk = 0, kInvalid = -1;      // ORBFE_OK, ORBFE_ERR_INVALID
bool said(int rc, const CullingPlan& plan, const char* why) {      // the whole message, not a word of it
  if (rc != kInvalid || std::strcmp(plan.why, why)) { std::printf("expected the refusal '%s', got %d '%s'\n", why, rc, plan.why); return false; }
  return true;
}
bool refused(const Args& a, const char* why) {
  CullingPlan plan;
  return said(a.check(plan), plan, why);
}
}  // namespace

int main() {
  CullingPlan plan;
  Args ok;
  CHECK(ok.check(plan) == kOk && plan.why[0] == 0);
  CHECK(plan.nObs == 5 && plan.nEntries == 5 && plan.obsBase == 0 && plan.subjBase == 0);
  ok.withNobs = false;
  CHECK(ok.check(plan) == kOk);
  ok.th_obs = 1;
  CHECK(ok.check(plan) == kOk);

  { Args a; a.n_kf = -1; CHECK(refused(a, "negative size (n_kf -1, n_mp 3, n_subj 3)")); }
  { Args a; a.n_mp = -1; CHECK(refused(a, "negative size (n_kf 5, n_mp -1, n_subj 3)")); }
  { Args a; a.n_subj = -1; CHECK(refused(a, "negative size (n_kf 5, n_mp 3, n_subj -1)")); }
  { Args a; a.th_obs = 0; CHECK(refused(a, "th_obs = 0 is below 1")); }
  { Args a; a.th_obs = -3; CHECK(refused(a, "th_obs = -3 is below 1")); }
  { Args a; a.obsOffs[2] = 1; CHECK(refused(a, "obs_offsets decreases at MapPoint 1 (1 after 2)")); }
  { Args a; a.obsOffs[0] = -1; CHECK(refused(a, "obs_offsets[0] = -1 is negative")); }
  { Args a; a.subjOffs[1] = 4; CHECK(refused(a, "subj_offsets decreases at subject 1 (3 after 4)")); }
  { Args a; a.subjOffs[0] = -1; CHECK(refused(a, "subj_offsets[0] = -1 is negative")); }
  { Args a; a.obsKf[4] = 5; CHECK(refused(a, "obs_kf[4] = 5 outside [0, 5)")); }
  { Args a; a.obsKf[0] = -1; CHECK(refused(a, "obs_kf[0] = -1 outside [0, 5)")); }
  { Args a; a.subjMp[3] = 3; CHECK(refused(a, "subj_mp[3] = 3 outside [-1, 3)")); }
  { Args a; a.subjMp[1] = -2; CHECK(refused(a, "subj_mp[1] = -2 outside [-1, 3)")); }
  { Args a; a.self[2] = 5; CHECK(refused(a, "subj_self[2] = 5 outside [-1, 5)")); }
  { Args a; a.self[1] = -2; CHECK(refused(a, "subj_self[1] = -2 outside [-1, 5)")); }
  { Args a; a.nobs[1] = -1; CHECK(refused(a, "mp_nobs[1] = -1 is negative")); }
  {   // a null pointer; the payload arrays only where their CSR is non-empty
    Args a;
    const int32_t *oo = a.obsOffs.data(), *ok_ = a.obsKf.data(), *ss = a.self.data(), *so = a.subjOffs.data(), *sm = a.subjMp.data();
    const uint8_t *ol = a.obsLevel.data(), *sl = a.subjLevel.data();
    const char *three = "null pointer (obs_offsets, subj_self or subj_offsets)", *obs = "null pointer (obs_kf or obs_level, with 5 observations)",
               *subj = "null pointer (subj_mp or subj_level, with 5 entries)";
    CHECK(said(culling_check(5, 3, nullptr, ok_, ol, nullptr, 3, ss, so, sm, sl, 3, plan), plan, three));
    CHECK(said(culling_check(5, 3, oo, nullptr, ol, nullptr, 3, ss, so, sm, sl, 3, plan), plan, obs));
    CHECK(said(culling_check(5, 3, oo, ok_, nullptr, nullptr, 3, ss, so, sm, sl, 3, plan), plan, obs));
    CHECK(said(culling_check(5, 3, oo, ok_, ol, nullptr, 3, nullptr, so, sm, sl, 3, plan), plan, three));
    CHECK(said(culling_check(5, 3, oo, ok_, ol, nullptr, 3, ss, nullptr, sm, sl, 3, plan), plan, three));
    CHECK(said(culling_check(5, 3, oo, ok_, ol, nullptr, 3, ss, so, nullptr, sl, 3, plan), plan, subj));
    CHECK(said(culling_check(5, 3, oo, ok_, ol, nullptr, 3, ss, so, sm, nullptr, 3, plan), plan, subj));
    // two at once: th_obs comes after the sizes and before the pointers
    CHECK(said(culling_check(5, 3, nullptr, ok_, ol, nullptr, 3, ss, so, sm, sl, 0, plan), plan, "th_obs = 0 is below 1"));
    CHECK(said(culling_check(5, 3, oo, ok_, nullptr, nullptr, 3, ss, so, sm, nullptr, 0, plan), plan, "th_obs = 0 is below 1"));
    CHECK(said(culling_check(5, -2, nullptr, ok_, ol, nullptr, 3, ss, so, sm, sl, 0, plan), plan, "negative size (n_kf 5, n_mp -2, n_subj 3)"));
    a.subjOffs[0] = -1;
    CHECK(said(culling_check(5, 3, oo, ok_, nullptr, nullptr, 3, ss, so, sm, sl, 3, plan), plan, obs));      // before anything about the subjects' CSR
  }
  // two faults at once: which one is reported
  { Args a; a.th_obs = 0; a.n_subj = -1; CHECK(refused(a, "negative size (n_kf 5, n_mp 3, n_subj -1)")); }
  { Args a; a.th_obs = 0; a.obsOffs[0] = -1; CHECK(refused(a, "th_obs = 0 is below 1")); }
  { Args a; a.th_obs = 0; a.nobs[0] = -1; CHECK(refused(a, "th_obs = 0 is below 1")); }
  { Args a; a.nobs[0] = -1; a.self[2] = 5; CHECK(refused(a, "subj_self[2] = 5 outside [-1, 5)")); }        // mp_nobs is tested last
  { Args a; a.nobs[0] = -1; a.subjMp[4] = 3; CHECK(refused(a, "subj_mp[4] = 3 outside [-1, 3)")); }
  { Args a; a.nobs[1] = -4; a.nobs[2] = -1; CHECK(refused(a, "mp_nobs[1] = -4 is negative")); }
  { Args a; a.obsOffs[2] = 1; a.obsKf[0] = 7; CHECK(refused(a, "obs_offsets decreases at MapPoint 1 (1 after 2)")); }
  { Args a; a.subjOffs[1] = 4; a.obsKf[0] = 7; CHECK(refused(a, "subj_offsets decreases at subject 1 (3 after 4)")); }
  { Args a; a.subjMp[3] = 3; a.self[0] = 5; CHECK(refused(a, "subj_mp[3] = 3 outside [-1, 3)")); }
  { Args a; a.obsKf[4] = 5; a.subjMp[0] = -2; CHECK(refused(a, "obs_kf[4] = 5 outside [0, 5)")); }
  { Args a; a.obsKf[1] = 5; a.obsKf[3] = -1; CHECK(refused(a, "obs_kf[1] = 5 outside [0, 5)")); }
  {   // empty CSRs may come without their arrays; offsets that do not start at 0 are rebased
    const int32_t z[2] = {7, 7}, selfs[1] = {-1};
    CHECK(culling_check(0, 0, z, nullptr, nullptr, nullptr, 1, selfs, z, nullptr, nullptr, 3, plan) == kOk);
    CHECK(plan.obsBase == 7 && plan.subjBase == 7 && plan.nObs == 0 && plan.nEntries == 0);
    std::vector<int32_t> obsOffs{2, 4}, obsKf{9, 9, 0, 1}, subjOffs{1, 2}, subjMp{5, 0};
    std::vector<uint8_t> obsLevel{0, 0, 1, 2}, subjLevel{0, 3};
    CHECK(culling_check(2, 1, obsOffs.data(), obsKf.data(), obsLevel.data(), nullptr, 1, selfs, subjOffs.data(), subjMp.data(), subjLevel.data(), 3, plan) ==
          kOk);                                                        // the 9s and the 5 lie outside
    CHECK(plan.obsBase == 2 && plan.subjBase == 1 && plan.nObs == 2 && plan.nEntries == 1);
  }
  {   // n_subj == 0 passes the check with nothing but the MapPoints' offsets: the C call answers ORBFE_OK without a launch
    const int32_t oo[1] = {0}, so[1] = {0}, none[1] = {0};
    CHECK(culling_check(0, 0, oo, nullptr, nullptr, nullptr, 0, none, so, nullptr, nullptr, 3, plan) == kOk && plan.nEntries == 0);
  }
  std::printf("PASS\n");
  return 0;
}
