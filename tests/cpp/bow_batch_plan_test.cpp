// bow_batch_plan_test.cpp -- the host-side bookkeeping of orbfe_bow_transform_batch and orbfe_kfdb_add_batch
// (os1_amd/csrc/bow_batch_plan.h) without a GPU: the wave-offset table and the search over it, the capacity check that refuses
// the whole call, and the keyframe database's pre-check and placement against a plain simulation of n single adds.
//   build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ios1_amd/csrc tests/cpp/bow_batch_plan_test.cpp
// Prints PASS; exit code 0 iff every check holds.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "bow_batch_plan.h"

#define CHECK(cond)                                                                       \
  do {                                                                                    \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

using namespace orbfe;

namespace {
uint32_t g_state = 2463534242u;
uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 17; g_state ^= g_state << 5; return g_state; }

// n single adds as orbfe_kfdb_add performs them, on numbers only: -> offsets of the batch's keyframes afterwards, or the first
// failing entry
struct SimDb {
  size_t capE, tail, live;
  int capK, nLive;
  std::set<uint64_t> keys;
  std::vector<std::pair<size_t, size_t> > old;   // (offset, count) of the live keyframes already there
};
int simulate(SimDb db, int n, const uint64_t* keys, const int* counts, std::vector<size_t>& off, int* compactions, int* code) {
  std::vector<std::pair<size_t, size_t> > mine;
  *compactions = 0;
  for (int j = 0; j < n; j++) {
    const size_t c = (size_t)counts[j];
    if (db.keys.count(keys[j])) { *code = kBowBatchInvalid; return j; }
    if (db.nLive >= db.capK) { *code = kBowBatchOverflow; return j; }
    if (db.live + c > db.capE) { *code = kBowBatchOverflow; return j; }
    if (db.tail + c > db.capE) {   // compact: live keyframes with entries to the front, in pool order; empty ones to offset 0
      size_t at = 0;
      for (auto& e : db.old) { e.first = e.second ? at : 0; at += e.second; }
      for (auto& e : mine) { e.first = e.second ? at : 0; at += e.second; }
      db.tail = at;
      ++*compactions;
    }
    mine.push_back(std::make_pair(db.tail, c));
    db.keys.insert(keys[j]);
    db.tail += c; db.live += c; db.nLive++;
  }
  off.clear();
  for (auto& e : mine) off.push_back(e.first);
  *code = kBowBatchOk;
  return -1;
}
}  // namespace

int main() {
  // ---- the set-offset table ----
  {
    const int n[7] = {63, 0, 200, 1, 65, 64, 0};
    const int where[7] = {0, 0, 1, 0, 1, 0, 0};
    int cap[7];
    for (int s = 0; s < 7; s++) cap[s] = n[s];
    BowBatchPlan p;
    CHECK(bow_batch_plan(7, n, cap, where, p) == kBowBatchOk && p.failed == -1);
    const uint32_t wantWave[8] = {0, 16, 16, 66, 67, 84, 100, 100}, wantOut[8] = {0, 63, 63, 263, 264, 329, 393, 393};
    const uint32_t wantStage[7] = {0, 63, 63, 63, 64, 64, 128};
    for (int s = 0; s <= 7; s++) CHECK(p.waveStart[s] == wantWave[s] && p.out0[s] == wantOut[s]);
    for (int s = 0; s < 7; s++) CHECK(p.stageRow[s] == wantStage[s]);
    CHECK(p.stagedRows == 128);
    // every wave belongs to exactly one non-empty set, every feature of every set to exactly one (wave, slot)
    std::vector<int> hits(393, 0);
    for (uint32_t w = 0; w < p.waveStart[7]; w++) {
      const int s = bow_batch_set_of_wave(p.waveStart, w);
      CHECK(s >= 0 && s < 7 && n[s] > 0 && p.waveStart[s] <= w && w < p.waveStart[s + 1]);
      for (uint32_t k = 0; k < 4; k++) {
        const uint32_t f = (w - p.waveStart[s]) * 4 + k;
        if (f < (uint32_t)n[s]) hits[p.out0[s] + f]++;
      }
    }
    for (int h : hits) CHECK(h == 1);
    // all-or-nothing: one short on set 3 is the failure that is reported, also when a later set is short too
    cap[3] = 0; cap[5] = 10;
    CHECK(bow_batch_plan(7, n, cap, where, p) == kBowBatchOverflow && p.failed == 3 && p.waveStart.empty());
    cap[3] = 1; cap[5] = 64;
    int neg[7];
    for (int s = 0; s < 7; s++) neg[s] = n[s];
    neg[4] = -1;
    CHECK(bow_batch_plan(7, neg, cap, where, p) == kBowBatchInvalid && p.failed == 4);
    CHECK(bow_batch_plan(0, nullptr, nullptr, nullptr, p) == kBowBatchOk && p.waveStart.size() == 1 && p.waveStart[0] == 0);
    CHECK(bow_batch_plan(2, nullptr, cap, where, p) == kBowBatchInvalid);
    const int big[3] = {1 << 29, 1 << 29, 8}, bw[3] = {1, 1, 1};
    CHECK(bow_batch_plan(3, big, big, bw, p) == kBowBatchOverflow && p.failed == 2);
    // random ragged batches, only empty sets included
    for (int round = 0; round < 200; round++) {
      const int ns = 1 + (int)(rnd() % 40);
      std::vector<int> nn(ns), ww(ns);
      for (int s = 0; s < ns; s++) { nn[s] = (rnd() % 3 == 0 || round == 0) ? 0 : (int)(rnd() % 300); ww[s] = (int)(rnd() & 1); }
      CHECK(bow_batch_plan(ns, nn.data(), nn.data(), ww.data(), p) == kBowBatchOk);
      uint32_t feats = 0;
      for (uint32_t w = 0; w < p.waveStart[ns]; w++) {
        const int s = bow_batch_set_of_wave(p.waveStart, w);
        CHECK(nn[s] > 0 && p.waveStart[s] <= w && w < p.waveStart[s + 1]);
        const uint32_t f0 = (w - p.waveStart[s]) * 4;
        CHECK(f0 < (uint32_t)nn[s]);
        feats += std::min<uint32_t>(4, (uint32_t)nn[s] - f0);
      }
      CHECK(feats == p.out0[ns]);
    }
  }
  // ---- the keyframe database's pre-check and placement, against the simulation of single adds ----
  {
    int withCompaction = 0, refused = 0, accepted = 0;
    for (int round = 0; round < 2000; round++) {
      SimDb db;
      db.capE = 50 + rnd() % 200;
      db.capK = 4 + (int)(rnd() % 12);
      db.nLive = 0; db.live = 0; db.tail = 0;
      // some history: live keyframes and tombstones behind a tail
      const int hist = (int)(rnd() % 5);
      for (int i = 0; i < hist; i++) {
        const size_t c = rnd() % 30;
        if (db.tail + c > db.capE) break;
        if (rnd() & 1) { db.old.push_back(std::make_pair(db.tail, c)); db.keys.insert(100 + (uint64_t)i); db.live += c; db.nLive++; }
        db.tail += c;
      }
      const int n = (int)(rnd() % 10);
      std::vector<uint64_t> keys(n);
      std::vector<int> counts(n);
      std::vector<std::vector<uint32_t> > w(n);
      std::vector<std::vector<double> > v(n);
      std::vector<const uint32_t*> pw(n);
      std::vector<const double*> pv(n);
      for (int j = 0; j < n; j++) {
        keys[j] = (rnd() % 16 == 0) ? 100 + rnd() % 5 : 1000 + (uint64_t)j;
        if (j > 0 && rnd() % 24 == 0) keys[j] = keys[j - 1];
        counts[j] = rnd() % 4 == 0 ? 0 : (int)(rnd() % 40);
        for (int i = 0; i < counts[j]; i++) { w[j].push_back((uint32_t)(3 * i + 1)); v[j].push_back(0.5); }
        pw[j] = w[j].data(); pv[j] = v[j].data();
      }
      std::vector<size_t> want;
      int comp = 0, code = 0;
      const int failAt = simulate(db, n, keys.data(), counts.data(), want, &comp, &code);
      KfdbBatchPlan p;
      const int rc = kfdb_batch_plan(n, keys.data(), pw.data(), pv.data(), counts.data(), 1000u, db.nLive, db.capK, db.live, db.capE, db.tail,
                                     [&](uint64_t k) { return db.keys.count(k) != 0; }, p);
      CHECK(rc == code && p.failed == failAt);
      if (rc) { refused++; continue; }
      accepted++;
      CHECK(comp <= 1 && (comp == 1) == (p.compactAt >= 0));
      withCompaction += comp;
      size_t total = 0;
      for (int j = 0; j < n; j++) { CHECK(p.offset[j] == want[j]); total += (size_t)counts[j]; }
      CHECK(p.total == total);
    }
    CHECK(withCompaction > 20 && refused > 100 && accepted > 500);
    // words: not ascending, out of range -- named by entry
    const uint32_t good[3] = {1, 5, 9}, bad[3] = {1, 9, 9}, high[2] = {4, 1000};
    const double val[3] = {0.1, 0.2, 0.7};
    const uint64_t keys[3] = {1, 2, 3};
    const uint32_t* pw[3] = {good, bad, good};
    const double* pv[3] = {val, val, val};
    const int counts[3] = {3, 3, 3};
    KfdbBatchPlan p;
    auto none = [](uint64_t) { return false; };
    CHECK(kfdb_batch_plan(3, keys, pw, pv, counts, 1000u, 0, 8, 0, 100, 0, none, p) == kBowBatchInvalid && p.failed == 1 && p.why == 1);
    pw[1] = high;
    const int c2[3] = {3, 2, 3};
    CHECK(kfdb_batch_plan(3, keys, pw, pv, c2, 1000u, 0, 8, 0, 100, 0, none, p) == kBowBatchInvalid && p.failed == 1 && p.why == 1);
    CHECK(kfdb_batch_plan(3, keys, pw, pv, c2, 1001u, 0, 8, 0, 100, 0, none, p) == kBowBatchOk && p.total == 8);
    CHECK(kfdb_batch_plan(3, keys, pw, pv, c2, 1001u, 6, 8, 0, 100, 0, none, p) == kBowBatchOverflow && p.failed == 2 && p.why == 3);
    CHECK(kfdb_batch_plan(3, keys, pw, pv, c2, 1001u, 0, 8, 95, 100, 95, none, p) == kBowBatchOverflow && p.failed == 2 && p.why == 4);
    pw[2] = nullptr;
    CHECK(kfdb_batch_plan(3, keys, pw, pv, c2, 1001u, 0, 8, 0, 100, 0, none, p) == kBowBatchInvalid && p.failed == 2 && p.why == 5);
    CHECK(kfdb_batch_plan(0, nullptr, nullptr, nullptr, nullptr, 10u, 0, 8, 0, 100, 0, none, p) == kBowBatchOk && p.total == 0);
  }
  std::printf("PASS\n");
  return 0;
}
