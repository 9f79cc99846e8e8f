// tri_batch_plan_test.cpp -- os1_amd/csrc/tri_batch_plan.h as a program of its own (tests/test_tri_batch_plan.py builds it with
// the address and undefined-behaviour sanitizers): the record list against a brute-force intersection per neighbour, the layout
// of the upload image, the output bound, every refusal (with nothing left in the plan) and the mask step of the finish.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "tri_batch_plan.h"

using namespace orbfe;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Fv {
  std::vector<uint32_t> nodes, offsets{0}, features;
  std::vector<uint8_t> has;
  int n = 0;
};

// a keyframe of n keypoints whose features fall under `nodes` (node id -> how many), indices dealt in a seeded shuffle
static Fv make_fv(int n, const std::vector<std::pair<uint32_t, int>>& nodes, unsigned seed) {
  Fv f;
  f.n = n;
  std::vector<uint32_t> idx((size_t)n);
  for (int i = 0; i < n; i++) idx[i] = (uint32_t)i;
  std::mt19937 g(seed);
  std::shuffle(idx.begin(), idx.end(), g);
  size_t at = 0;
  for (auto& nd : nodes) {
    f.nodes.push_back(nd.first);
    std::vector<uint32_t> part(idx.begin() + at, idx.begin() + at + nd.second);
    std::sort(part.begin(), part.end());
    f.features.insert(f.features.end(), part.begin(), part.end());
    at += (size_t)nd.second;
    f.offsets.push_back((uint32_t)f.features.size());
  }
  f.has.resize((size_t)std::max(n, 1));
  for (int i = 0; i < n; i++) f.has[i] = (uint8_t)(g() & 1u);
  return f;
}

static TriSide side(const Fv& f, int device = 0, int maxOctave = 7, int nlevels = 8) {
  TriSide s;
  s.frame = true; s.device = device; s.n = f.n; s.maxOctave = maxOctave; s.has_mp = f.has.data();
  s.nodes = f.nodes.data(); s.offsets = f.offsets.data(); s.features = f.features.data(); s.n_fv = (int)f.nodes.size();
  s.nlevels = nlevels;
  return s;
}

static void expect_refused(const char* what, int want, int wantNb, const TriSide& s1, std::vector<TriSide> nb, const char* word) {
  TriBatchPlan plan;
  plan.records.push_back(TriRecord{1, 2, 3, 4, 5, 6});   // (a plan that held something: the refusal must leave none of it)
  const int rc = tri_batch_plan(0, s1, (int)nb.size(), nb.data(), 208, plan);
  const bool ok = rc == want && plan.failed == wantNb && plan.records.empty() && plan.bytes == 0 && std::strstr(plan.why, word) &&
                  (wantNb < 0 || std::strstr(plan.why, ("neighbour " + std::to_string(wantNb)).c_str()));
  if (!ok) { std::printf("FAIL refusal '%s': rc %d failed %d why '%s'\n", what, rc, plan.failed, plan.why); fails++; }
}

int main() {
  // ---- records = per-neighbour common nodes, node-major; the image; the bound ----------------------------------------------
  const Fv f1 = make_fv(400, {{2, 30}, {5, 257}, {9, 1}, {11, 0}, {40, 100}, {0xffffffffu, 12}}, 1);
  const std::vector<Fv> f2 = {make_fv(300, {{1, 10}, {5, 100}, {9, 7}, {11, 5}, {0xffffffffu, 100}}, 2),   // shares 5, 9, -1 (11 is empty on side 1)
                              make_fv(350, {{3, 50}, {4, 60}, {41, 70}}, 3),                               // shares nothing
                              make_fv(0, {}, 4),                                                           // an empty keyframe
                              make_fv(380, {{2, 256}, {5, 0}, {40, 124}}, 5)};                             // shares 2, 40 (5 is empty on side 2)
  const TriSide s1 = side(f1);
  std::vector<TriSide> nb;
  for (auto& f : f2) nb.push_back(side(f));
  TriBatchPlan plan;
  CHECK(tri_batch_plan(0, s1, (int)nb.size(), nb.data(), 208, plan) == kTriBatchOk);
  CHECK(plan.failed == -1 && plan.entries == 4ull * 400ull);
  // brute force: for every neighbour, the node ids both sides hold with at least one feature each
  size_t total = 0;
  std::vector<uint32_t> feat2Base(nb.size() + 1, 0);
  for (size_t k = 0; k < nb.size(); k++) feat2Base[k + 1] = feat2Base[k] + (uint32_t)f2[k].features.size();
  for (size_t k = 0; k < nb.size(); k++) {
    std::vector<TriRecord> own, mine;
    tri_common_nodes(s1, nb[k], own);
    for (auto& r : plan.records) if (r.nb == (int)k) mine.push_back(r);
    std::map<uint32_t, std::pair<int, int>> m1, m2;
    for (size_t a = 0; a < f1.nodes.size(); a++) m1[f1.nodes[a]] = {(int)f1.offsets[a], (int)f1.offsets[a + 1]};
    for (size_t b = 0; b < f2[k].nodes.size(); b++) m2[f2[k].nodes[b]] = {(int)f2[k].offsets[b], (int)f2[k].offsets[b + 1]};
    std::vector<TriRecord> brute;
    for (auto& e : m1) {
      auto it = m2.find(e.first);
      if (it == m2.end() || e.second.first == e.second.second || it->second.first == it->second.second) continue;
      brute.push_back(TriRecord{e.second.first, e.second.second, it->second.first, it->second.second, 0, 0});
    }
    CHECK(own.size() == brute.size() && mine.size() == brute.size());
    for (size_t i = 0; i < brute.size() && i < own.size() && i < mine.size(); i++) {
      CHECK(own[i].b1 == brute[i].b1 && own[i].e1 == brute[i].e1 && own[i].b2 == brute[i].b2 && own[i].e2 == brute[i].e2);
      CHECK(mine[i].b1 == own[i].b1 && mine[i].e1 == own[i].e1);
      CHECK(mine[i].b2 == own[i].b2 + (int)feat2Base[k] && mine[i].e2 == own[i].e2 + (int)feat2Base[k]);
      CHECK(mine[i].base1 == (int)k * 400);
    }
    CHECK(plan.flag2[k] == (k == 0 ? 0u : plan.flag2[k - 1] + (uint32_t)f2[k - 1].n) && plan.feat2[k] == feat2Base[k]);
    total += brute.size();
  }
  CHECK(total == 5 && plan.records.size() == total);
  for (size_t i = 1; i < plan.records.size(); i++) {   // node-major, neighbours ascending inside a node
    const TriRecord &p = plan.records[i - 1], &r = plan.records[i];
    CHECK(p.b1 < r.b1 || (p.b1 == r.b1 && p.nb < r.nb));
  }
  for (auto& r : plan.records) {   // the bound: no entry the kernel may write lies outside [0, entries)
    for (int i = r.b1; i < r.e1; i++) CHECK((uint64_t)r.base1 + f1.features[i] < plan.entries);
    CHECK(r.e2 <= (int)plan.nFeat2 && r.e1 <= (int)plan.nFeat1 && r.e2 - r.b2 <= kTriMaxGroup);
  }
  // the image: parts in order, aligned, none overlapping, sized for what goes into them
  CHECK(plan.oTable == 0 && plan.oRecords >= 208 * nb.size() && plan.oFlag1 >= plan.oRecords + sizeof(TriRecord) * plan.records.size());
  CHECK(plan.oFeat1 >= plan.oFlag1 + 400 && plan.oFlag2 >= plan.oFeat1 + 4 * plan.nFeat1 && plan.oFeat2 >= plan.oFlag2 + plan.nFlag2);
  CHECK(plan.bytes >= plan.oFeat2 + 4 * plan.nFeat2 && plan.nFlag2 == 300 + 350 + 0 + 380 && plan.nFeat1 == 400);
  for (size_t o : {plan.oRecords, plan.oFlag1, plan.oFeat1, plan.oFlag2, plan.oFeat2, plan.bytes}) CHECK(o % kTriAlign == 0);
  // n_nb == 0 and a batch of one
  CHECK(tri_batch_plan(0, s1, 0, nullptr, 208, plan) == kTriBatchOk && plan.records.empty() && plan.entries == 0);
  CHECK(tri_batch_plan(0, s1, 1, &nb[3], 208, plan) == kTriBatchOk && plan.records.size() == 2 && plan.entries == 400 && plan.records[1].base1 == 0);

  // ---- refusals: everything is checked before anything is laid out; the message names the neighbour ------------------------
  {
    std::vector<TriSide> bad = nb;
    bad[1].maxOctave = 8;
    expect_refused("octave == nlevels2", kTriBatchInvalid, 1, s1, bad, "octave");
    bad = nb; bad[3].maxOctave = INT_MAX;   // what a resident frame reports for a negative octave
    expect_refused("negative octave", kTriBatchInvalid, 3, s1, bad, "octave");
    bad = nb; bad[2].maxOctave = 99;        // an empty keyframe has no octave to object to
    CHECK(tri_batch_plan(0, s1, (int)bad.size(), bad.data(), 208, plan) == kTriBatchOk);
    bad = nb; bad[0].device = 1;
    expect_refused("neighbour on another device", kTriBatchInvalid, 0, s1, bad, "device");
    TriSide o1 = s1; o1.device = 3;
    expect_refused("frame1 on another device", kTriBatchInvalid, -1, o1, nb, "device");
    for (int lv : {0, -1, 17}) {
      bad = nb; bad[3].nlevels = lv;
      expect_refused("nlevels2", kTriBatchInvalid, 3, s1, bad, "nlevels2");
    }
    bad = nb; bad[0].nlevels = 16; CHECK(tri_batch_plan(0, s1, (int)bad.size(), bad.data(), 208, plan) == kTriBatchOk);
    bad = nb; bad[0].nlevels = 1; bad[0].maxOctave = 0; CHECK(tri_batch_plan(0, s1, (int)bad.size(), bad.data(), 208, plan) == kTriBatchOk);
    Fv g = f2[3];
    g.features[100] = 380;   // == n2
    bad = nb; bad[3] = side(g);
    expect_refused("side-2 feature index == n", kTriBatchInvalid, 3, s1, bad, "feature index");
    Fv h = f1;
    h.features.back() = 400;
    expect_refused("side-1 feature index == n", kTriBatchInvalid, -1, side(h), nb, "feature index");
    g = f2[0]; g.offsets[2] = g.offsets[1] - 1;
    bad = nb; bad[0] = side(g);
    expect_refused("offsets decrease", kTriBatchInvalid, 0, s1, bad, "decrease");
    g = f2[0]; g.nodes[2] = g.nodes[1];
    bad = nb; bad[0] = side(g);
    expect_refused("nodes do not ascend", kTriBatchInvalid, 0, s1, bad, "ascend");
    bad = nb; bad[1].frame = false;
    expect_refused("frame2 NULL", kTriBatchInvalid, 1, s1, bad, "NULL");
    bad = nb; bad[1].has_mp = nullptr;
    expect_refused("has_mp2 NULL", kTriBatchInvalid, 1, s1, bad, "has_mp2");
    bad = nb; bad[3].tables = false;
    expect_refused("tables NULL", kTriBatchInvalid, 3, s1, bad, "scale_factors2");
    // a node of 65 536 features of a neighbour: a position no longer fits a key
    const Fv big = make_fv(kTriMaxGroup + 1, {{5, kTriMaxGroup + 1}}, 7), fits = make_fv(kTriMaxGroup, {{5, kTriMaxGroup}}, 8);
    bad = nb; bad[1] = side(big);
    expect_refused("node of 65 536", kTriBatchOverflow, 1, s1, bad, "65536");
    bad = nb; bad[1] = side(fits);
    CHECK(tri_batch_plan(0, s1, (int)bad.size(), bad.data(), 208, plan) == kTriBatchOk);
  }
  {
    TriBatchPlan p2;
    CHECK(tri_batch_plan(0, s1, -1, nb.data(), 208, p2) == kTriBatchInvalid && p2.records.empty());
  }

  // ---- the mask step of the finish ------------------------------------------------------------------------------------------
  {
    const int32_t raw[6] = {3, -1, 0, 2, -1, 1};
    const uint8_t init[6] = {0, 1, 0, 0, 0, 0}, now[6] = {0, 1, 1, 0, 1, 0}, cleared[6] = {0, 0, 1, 0, 0, 0};
    int32_t row[6] = {9, 9, 9, 9, 9, 9};
    int at = -1;
    CHECK(tri_finish_mask(raw, 6, init, now, 4, row, &at) == kTriBatchOk);
    const int32_t want[6] = {3, -1, -1, 2, -1, 1};
    CHECK(std::memcmp(row, want, sizeof want) == 0);
    int32_t keep[6] = {9, 9, 9, 9, 9, 9};
    CHECK(tri_finish_mask(raw, 6, init, cleared, 4, keep, &at) == kTriFinishStale && at == 1 && keep[0] == 9 && keep[5] == 9);
    CHECK(tri_finish_mask(raw, 6, init, now, 3, keep, &at) == kTriBatchInvalid && at == 0 && keep[0] == 9);
    CHECK(tri_finish_mask(raw, 0, init, now, 0, keep, &at) == kTriBatchOk);
  }
  if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
  std::printf("tri_batch_plan_test ok\n");
  return 0;
}
