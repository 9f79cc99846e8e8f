// os1_amd/csrc/covis_plan.h as a program of its own (no HIP, no GPU): every refusal of the argument check with its whole message,
// which of two faults is reported, the output bound, the pass count at the histogram's capacity, and the assembly of pieces that lie in the device
// arrays in another order than the subjects'.  Built with -fsanitize=address,undefined by tests/test_covisibility.py: the
// arrays below are exactly as long as the call may read.
#include <cstdio>
#include <cstring>
#include <vector>

#include "covis_plan.h"

using namespace orbfe;

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

namespace {
struct Args {
  int n_kf = 5, n_mp = 3, n_subj = 3;
  std::vector<int32_t> obsOffs{0, 2, 2, 5}, obsKf{0, 4, 1, 2, 3};          // MapPoint 1 has no observation
  std::vector<int32_t> self{0, -1, 4}, limit{5, 0, 2}, subjOffs{0, 3, 3, 5}, subjMp{0, -1, 2, 2, 2};
  bool withLimit = true;
  int check(CovisPlan& plan) const {
    return covis_check(n_kf, n_mp, obsOffs.data(), obsKf.data(), n_subj, self.data(), withLimit ? limit.data() : nullptr, subjOffs.data(),
                       subjMp.data(), plan);
  }
};
constexpr int kOk = 0, kInvalid = -1;      // ORBFE_OK, ORBFE_ERR_INVALID
bool said(int rc, const CovisPlan& plan, const char* why) {      // the whole message, not a word of it
  if (rc != kInvalid || std::strcmp(plan.why, why)) { std::printf("expected the refusal '%s', got %d '%s'\n", why, rc, plan.why); return false; }
  return true;
}
bool refused(const Args& a, const char* why) {
  CovisPlan plan;
  return said(a.check(plan), plan, why);
}
}  // namespace

int main() {
  CovisPlan plan;
  Args ok;
  CHECK(ok.check(plan) == kOk && plan.why[0] == 0);
  CHECK(plan.nPass == 1 && plan.nObs == 5 && plan.nEntries == 5 && plan.obsBase == 0 && plan.subjBase == 0);
  CHECK(plan.bound == 5 + 0 + 2);          // min(5, 2 + 3), min(0, 0), min(2, 3 + 3)
  ok.withLimit = false;
  CHECK(ok.check(plan) == kOk && plan.bound == 5 + 0 + 5);

  { Args a; a.n_kf = -1; CHECK(refused(a, "negative size (n_kf -1, n_mp 3, n_subj 3)")); }
  { Args a; a.n_mp = -1; CHECK(refused(a, "negative size (n_kf 5, n_mp -1, n_subj 3)")); }
  { Args a; a.n_subj = -1; CHECK(refused(a, "negative size (n_kf 5, n_mp 3, n_subj -1)")); }
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
  { Args a; a.limit[0] = 6; CHECK(refused(a, "subj_limit[0] = 6 outside [0, 5]")); }
  { Args a; a.limit[2] = -1; CHECK(refused(a, "subj_limit[2] = -1 outside [0, 5]")); }
  {   // a null pointer; the payload arrays only where their CSR is non-empty
    Args a;
    const int32_t *oo = a.obsOffs.data(), *ok_ = a.obsKf.data(), *ss = a.self.data(), *so = a.subjOffs.data(), *sm = a.subjMp.data();
    const char* three = "null pointer (obs_offsets, subj_self or subj_offsets)";
    CHECK(said(covis_check(5, 3, nullptr, ok_, 3, ss, nullptr, so, sm, plan), plan, three));
    CHECK(said(covis_check(5, 3, oo, nullptr, 3, ss, nullptr, so, sm, plan), plan, "null pointer (obs_kf, with 5 observations)"));
    CHECK(said(covis_check(5, 3, oo, ok_, 3, nullptr, nullptr, so, sm, plan), plan, three));
    CHECK(said(covis_check(5, 3, oo, ok_, 3, ss, nullptr, nullptr, sm, plan), plan, three));
    CHECK(said(covis_check(5, 3, oo, ok_, 3, ss, nullptr, so, nullptr, plan), plan, "null pointer (subj_mp, with 5 entries)"));
    // two at once: the sizes before the pointers, obs_kf's absence before anything about the subjects' CSR
    CHECK(said(covis_check(5, -2, nullptr, ok_, 3, ss, nullptr, so, sm, plan), plan, "negative size (n_kf 5, n_mp -2, n_subj 3)"));
    a.subjOffs[1] = 4;
    CHECK(said(covis_check(5, 3, oo, nullptr, 3, ss, nullptr, so, sm, plan), plan, "null pointer (obs_kf, with 5 observations)"));
  }
  // two faults at once: which one is reported
  { Args a; a.limit[0] = 6; a.self[1] = -2; CHECK(refused(a, "subj_limit[0] = 6 outside [0, 5]")); }      // self and limit alternate, subject by subject
  { Args a; a.limit[0] = 6; a.self[0] = 9; CHECK(refused(a, "subj_self[0] = 9 outside [-1, 5)")); }
  { Args a; a.limit[1] = -1; a.self[2] = 5; CHECK(refused(a, "subj_limit[1] = -1 outside [0, 5]")); }
  { Args a; a.obsOffs[2] = 1; a.obsKf[0] = 7; CHECK(refused(a, "obs_offsets decreases at MapPoint 1 (1 after 2)")); }
  { Args a; a.subjOffs[1] = 4; a.obsKf[0] = 7; CHECK(refused(a, "subj_offsets decreases at subject 1 (3 after 4)")); }
  { Args a; a.subjMp[3] = 3; a.self[0] = 5; CHECK(refused(a, "subj_mp[3] = 3 outside [-1, 3)")); }
  { Args a; a.obsKf[4] = 5; a.subjMp[0] = -2; CHECK(refused(a, "obs_kf[4] = 5 outside [0, 5)")); }
  { Args a; a.obsKf[1] = 5; a.obsKf[3] = -1; CHECK(refused(a, "obs_kf[1] = 5 outside [0, 5)")); }
  { Args a; a.subjMp[4] = 3; a.limit[0] = 6; CHECK(refused(a, "subj_mp[4] = 3 outside [-1, 3)")); }
  {   // empty CSRs may come without their arrays; offsets that do not start at 0 are rebased
    const int32_t z[2] = {7, 7}, selfs[1] = {-1};
    CHECK(covis_check(0, 0, z, nullptr, 1, selfs, nullptr, z, nullptr, plan) == kOk);
    CHECK(plan.bound == 0 && plan.nPass == 1 && plan.obsBase == 7 && plan.subjBase == 7 && plan.nObs == 0 && plan.nEntries == 0);
    std::vector<int32_t> obsOffs{2, 4}, obsKf{9, 9, 0, 1}, subjOffs{1, 2}, subjMp{5, 0};
    CHECK(covis_check(2, 1, obsOffs.data(), obsKf.data(), 1, selfs, nullptr, subjOffs.data(), subjMp.data(), plan) == kOk);   // the 9s and the 5 lie outside
    CHECK(plan.obsBase == 2 && plan.subjBase == 1 && plan.nObs == 2 && plan.nEntries == 1 && plan.bound == 2);
  }
  {   // passes at the capacity of the histogram
    const int32_t z[2] = {0, 0}, selfs[1] = {-1};
    for (int d = -1; d <= 1; d++) {
      CHECK(covis_check(kCovisSlotsPerPass + d, 0, z, nullptr, 1, selfs, nullptr, z, nullptr, plan) == kOk);
      CHECK(plan.nPass == (d == 1 ? 2 : 1));
    }
    CHECK(covis_check(3 * kCovisSlotsPerPass, 0, z, nullptr, 1, selfs, nullptr, z, nullptr, plan) == kOk && plan.nPass == 3);
  }
  {   // assembly: 3 subjects x 2 passes, the pieces in the device arrays in the order the workgroups happened to reserve them
    const uint32_t start[6] = {4, 0, 0, 0, 1, 6}, count[6] = {2, 1, 0, 0, 3, 1};
    const int32_t devKf[7] = {20000, 3, 4, 9, 0, 7, 16390}, devCount[7] = {100, 13, 14, 19, 10, 17, 116};
    int32_t offs[4], kf[7], cnt[7];
    CHECK(covis_assemble(3, 2, start, count, devKf, devCount, 7, offs, kf, cnt) == kOk);
    const int32_t wantOffs[4] = {0, 3, 3, 7}, wantKf[7] = {0, 7, 20000, 3, 4, 9, 16390}, wantCnt[7] = {10, 17, 100, 13, 14, 19, 116};
    CHECK(!std::memcmp(offs, wantOffs, sizeof offs) && !std::memcmp(kf, wantKf, sizeof kf) && !std::memcmp(cnt, wantCnt, sizeof cnt));
    CHECK(covis_assemble(3, 2, start, count, devKf, devCount, 6, offs, kf, cnt) == kInvalid);   // a piece past the cursor
    CHECK(covis_assemble(3, 2, start, count, devKf, devCount, 8, offs, kf, cnt) == kInvalid);   // pieces that do not add up
    int32_t o1[1];
    CHECK(covis_assemble(0, 1, nullptr, nullptr, nullptr, nullptr, 0, o1, nullptr, nullptr) == kOk && o1[0] == 0);
  }
  std::printf("PASS\n");
  return 0;
}
