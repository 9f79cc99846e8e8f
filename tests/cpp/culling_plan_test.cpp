// os1_amd/csrc/culling_plan.h as a program of its own (no HIP, no GPU): every refusal of the argument check with the message that
// names it, empty and rebased CSRs, and what the check leaves to the caller (n_subj == 0).  Built plainly and with
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
bool refused(const Args& a, const char* word) {
  CullingPlan plan;
  const int rc = a.check(plan);
  if (rc != kCullingInvalid || !std::strstr(plan.why, word)) { std::printf("expected a refusal naming '%s', got %d '%s'\n", word, rc, plan.why); return false; }
  return true;
}
}  // namespace

int main() {
  CullingPlan plan;
  Args ok;
  CHECK(ok.check(plan) == kCullingOk && plan.why[0] == 0);
  CHECK(plan.nObs == 5 && plan.nEntries == 5 && plan.obsBase == 0 && plan.subjBase == 0);
  ok.withNobs = false;
  CHECK(ok.check(plan) == kCullingOk);
  ok.th_obs = 1;
  CHECK(ok.check(plan) == kCullingOk);

  { Args a; a.n_kf = -1; CHECK(refused(a, "negative size")); }
  { Args a; a.n_mp = -1; CHECK(refused(a, "negative size")); }
  { Args a; a.n_subj = -1; CHECK(refused(a, "negative size")); }
  { Args a; a.th_obs = 0; CHECK(refused(a, "th_obs = 0")); }
  { Args a; a.th_obs = -3; CHECK(refused(a, "th_obs = -3")); }
  { Args a; a.obsOffs[2] = 1; CHECK(refused(a, "obs_offsets decreases")); }
  { Args a; a.obsOffs[0] = -1; CHECK(refused(a, "obs_offsets[0]")); }
  { Args a; a.subjOffs[1] = 4; CHECK(refused(a, "subj_offsets decreases")); }
  { Args a; a.subjOffs[0] = -1; CHECK(refused(a, "subj_offsets[0]")); }
  { Args a; a.obsKf[4] = 5; CHECK(refused(a, "obs_kf[4] = 5")); }
  { Args a; a.obsKf[0] = -1; CHECK(refused(a, "obs_kf[0] = -1")); }
  { Args a; a.subjMp[3] = 3; CHECK(refused(a, "subj_mp[3] = 3")); }
  { Args a; a.subjMp[1] = -2; CHECK(refused(a, "subj_mp[1] = -2")); }
  { Args a; a.self[2] = 5; CHECK(refused(a, "subj_self[2] = 5")); }
  { Args a; a.self[1] = -2; CHECK(refused(a, "subj_self[1] = -2")); }
  { Args a; a.nobs[1] = -1; CHECK(refused(a, "mp_nobs[1] = -1")); }
  {   // a null pointer where the matching CSR is non-empty
    Args a;
    const int32_t *oo = a.obsOffs.data(), *ok_ = a.obsKf.data(), *ss = a.self.data(), *so = a.subjOffs.data(), *sm = a.subjMp.data();
    const uint8_t *ol = a.obsLevel.data(), *sl = a.subjLevel.data();
    CHECK(culling_check(5, 3, nullptr, ok_, ol, nullptr, 3, ss, so, sm, sl, 3, plan) == kCullingInvalid && std::strstr(plan.why, "null pointer"));
    CHECK(culling_check(5, 3, oo, nullptr, ol, nullptr, 3, ss, so, sm, sl, 3, plan) == kCullingInvalid && std::strstr(plan.why, "obs_kf or obs_level"));
    CHECK(culling_check(5, 3, oo, ok_, nullptr, nullptr, 3, ss, so, sm, sl, 3, plan) == kCullingInvalid && std::strstr(plan.why, "obs_kf or obs_level"));
    CHECK(culling_check(5, 3, oo, ok_, ol, nullptr, 3, nullptr, so, sm, sl, 3, plan) == kCullingInvalid && std::strstr(plan.why, "null pointer"));
    CHECK(culling_check(5, 3, oo, ok_, ol, nullptr, 3, ss, nullptr, sm, sl, 3, plan) == kCullingInvalid && std::strstr(plan.why, "null pointer"));
    CHECK(culling_check(5, 3, oo, ok_, ol, nullptr, 3, ss, so, nullptr, sl, 3, plan) == kCullingInvalid && std::strstr(plan.why, "subj_mp or subj_level"));
    CHECK(culling_check(5, 3, oo, ok_, ol, nullptr, 3, ss, so, sm, nullptr, 3, plan) == kCullingInvalid && std::strstr(plan.why, "subj_mp or subj_level"));
  }
  {   // empty CSRs may come without their arrays; offsets that do not start at 0 are rebased
    const int32_t z[2] = {7, 7}, selfs[1] = {-1};
    CHECK(culling_check(0, 0, z, nullptr, nullptr, nullptr, 1, selfs, z, nullptr, nullptr, 3, plan) == kCullingOk);
    CHECK(plan.obsBase == 7 && plan.subjBase == 7 && plan.nObs == 0 && plan.nEntries == 0);
    std::vector<int32_t> obsOffs{2, 4}, obsKf{9, 9, 0, 1}, subjOffs{1, 2}, subjMp{5, 0};
    std::vector<uint8_t> obsLevel{0, 0, 1, 2}, subjLevel{0, 3};
    CHECK(culling_check(2, 1, obsOffs.data(), obsKf.data(), obsLevel.data(), nullptr, 1, selfs, subjOffs.data(), subjMp.data(), subjLevel.data(), 3, plan) ==
          kCullingOk);                                                        // the 9s and the 5 lie outside
    CHECK(plan.obsBase == 2 && plan.subjBase == 1 && plan.nObs == 2 && plan.nEntries == 1);
  }
  {   // n_subj == 0 passes the check with nothing but the MapPoints' offsets: the C call answers ORBFE_OK without a launch
    const int32_t oo[1] = {0}, so[1] = {0}, none[1] = {0};
    CHECK(culling_check(0, 0, oo, nullptr, nullptr, nullptr, 0, none, so, nullptr, nullptr, 3, plan) == kCullingOk && plan.nEntries == 0);
  }
  std::printf("PASS\n");
  return 0;
}
