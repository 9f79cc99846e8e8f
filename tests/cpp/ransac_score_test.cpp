// ransac_score_test.cpp -- Sim3RansacWalk / PnPRansacWalk and Sim3Round / PnPRound (include/orbfe/RansacScoring.h) against the
// restated Sim3Solver::iterate / PnPsolver::iterate of tests/cpp/ransac_score_ref.cpp, on the scene files
// tests/ransac_score_util.py writes.  A scene is one round-robin as LoopClosing::ComputeSim3 / Tracking::Relocalization run it:
// several candidates (solvers), iterate(nIterations) on each in turn until each has given a hypothesis or given up.  Per round
// ONE scoring call covers all live candidates as segments; a PnP Refine is an n_hyp = 1 call.  The scoring goes through the C
// ABI (orbfe_score_sim3_hypotheses / orbfe_score_pnp_hypotheses), or with -DRANSAC_SCORE_HOST through the restatement's
// rsr_score_* so that the walks can be checked without a GPU.  Every iterate() prints one line; the last lines are
// "scenes N mismatches M" and PASS / FAIL.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "orbfe/RansacScoring.h"
#include "ransac_score_ref.h"

namespace {

#ifndef RANSAC_SCORE_HOST
orbfe_matcher* g_matcher = nullptr;
const char* last_error() { return orbfe_last_error(); }
#else
const char* last_error() { return "the restatement refused the layout"; }
#endif

int score(orbfe::Sim3Round& r) {
#ifdef RANSAC_SCORE_HOST
  return r.scoreWith(rsr_score_sim3);
#else
  return r.score(g_matcher);
#endif
}
int score(orbfe::PnPRound& r) {
#ifdef RANSAC_SCORE_HOST
  return r.scoreWith(rsr_score_pnp);
#else
  return r.score(g_matcher);
#endif
}

template <class T>
bool readv(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// calls > 0: every candidate gets exactly that many iterate() calls, whatever they return; 0: the round-robin's own rule
struct Header { int32_t model, n_cand, nIter, minInliers, maxIts, minSet; double probability; float epsilon; int32_t calls; };

struct Candidate {
  int32_t N, nFull, K, R;
  std::vector<int> indices;
  std::vector<float> corr, camsF, T12, T21;
  std::vector<double> camsD, Rt, refined;
};

bool same_mask(const std::vector<uint64_t>& words, const std::vector<bool>& bits, int N) {
  if (words.size() != orbfe::RansacWords(N)) return false;
  for (int i = 0; i < N; i++)
    if (orbfe::RansacBit(words.data(), i) != bits[i]) return false;
  for (int i = N; i < (int)(64 * words.size()); i++)
    if (orbfe::RansacBit(words.data(), i)) return false;
  return true;
}

int line(int round, int c, int ret, int want, bool noMore, bool wantNoMore, int nInl, int wantInl, int its, int best, int consumed, bool same) {
  const bool bad = ret != want || noMore != wantNoMore || nInl != wantInl || !same;
  printf("  round %d cand %d ret %d noMore %d nInliers %d its %d best %d consumed %d%s\n", round, c, ret, (int)noMore, nInl, its, best, consumed,
         bad ? " MISMATCH" : "");
  if (bad) printf("    restatement: ret %d noMore %d nInliers %d same-vectors %d\n", want, (int)wantNoMore, wantInl, (int)same);
  return bad;
}

int run_sim3(const Header& H, std::vector<Candidate>& C) {
  const int n = H.n_cand;
  std::vector<std::unique_ptr<orbfe::Sim3RansacWalk>> walk;
  std::vector<std::unique_ptr<RefSim3Solver>> ref;
  for (auto& c : C) {
    walk.emplace_back(new orbfe::Sim3RansacWalk(c.nFull, c.indices));
    ref.emplace_back(new RefSim3Solver(c.nFull, c.indices, c.corr.data(), c.camsF.data(), c.T12.data(), c.T21.data(), c.K));
    walk.back()->SetRansacParameters(H.probability, H.minInliers, H.maxIts);
    ref.back()->SetRansacParameters(H.probability, H.minInliers, H.maxIts);
  }
  std::vector<bool> discarded(n, false);
  std::vector<int> cursor(n, 0);
  int live = n, bad = 0;
  for (int round = 0; live > 0; round++) {
    orbfe::Sim3Round R;
    std::vector<int> firstHyp(n, 0), given(n, 0);
    for (int i = 0; i < n; i++) {
      if (discarded[i]) continue;
      const int need = std::min(walk[i]->hypotheses(H.nIter), C[i].K - cursor[i]);
      const int seg = R.addSegment(C[i].corr.data(), C[i].N, C[i].camsF.data());
      firstHyp[i] = R.hypotheses();
      given[i] = need;
      for (int j = 0; j < need; j++) R.addHypothesis(seg, &C[i].T12[12 * (size_t)(cursor[i] + j)], &C[i].T21[12 * (size_t)(cursor[i] + j)]);
    }
    if (score(R) != ORBFE_OK) { printf("scoring failed: %s\n", last_error()); return 1; }
    for (int i = 0; i < n; i++) {
      if (discarded[i]) continue;
      bool noMore, wantNoMore;
      std::vector<bool> inl, wantInl;
      int nInl, wantN, consumed = 0;
      const int k0 = firstHyp[i];
      const int ret = walk[i]->iterate(H.nIter, R.counts.data() + k0, R.masks.data(), R.maskOff.data() + k0, given[i], cursor[i], noMore, inl, nInl, &consumed);
      const int want = ref[i]->iterate(H.nIter, wantNoMore, wantInl, wantN);
      const bool same = inl == wantInl && walk[i]->mnIterations == ref[i]->mnIterations && walk[i]->mnBestInliers == ref[i]->mnBestInliers &&
                        walk[i]->bestHypothesis == ref[i]->best &&
                        (ref[i]->best < 0 || same_mask(walk[i]->mvbBestInliers, ref[i]->mvbBestInliers, C[i].N));
      bad += line(round, i, ret, want, noMore, wantNoMore, nInl, wantN, walk[i]->mnIterations, walk[i]->bestHypothesis, consumed, same);
      cursor[i] += consumed;
      if (H.calls > 0 ? round + 1 >= H.calls : noMore || ret != -1 || want != -1) { discarded[i] = true; live--; }   // ComputeSim3: vbDiscarded / bMatch
    }
  }
  return bad;
}

int run_pnp(const Header& H, std::vector<Candidate>& C) {
  const int n = H.n_cand;
  std::vector<std::unique_ptr<orbfe::PnPRansacWalk>> walk;
  std::vector<std::unique_ptr<RefPnPSolver>> ref;
  for (auto& c : C) {
    walk.emplace_back(new orbfe::PnPRansacWalk(c.nFull, c.indices));
    ref.emplace_back(new RefPnPSolver(c.nFull, c.indices, c.corr.data(), c.camsD.data(), c.Rt.data(), c.K, c.refined.data(), c.R));
    walk.back()->SetRansacParameters(H.probability, H.minInliers, H.maxIts, H.minSet, H.epsilon);
    ref.back()->SetRansacParameters(H.probability, H.minInliers, H.maxIts, H.minSet, H.epsilon);
  }
  std::vector<bool> discarded(n, false);
  std::vector<int> cursor(n, 0), refCursor(n, 0);
  int live = n, bad = 0;
  for (int round = 0; live > 0; round++) {
    orbfe::PnPRound R;
    std::vector<int> firstHyp(n, 0), given(n, 0);
    for (int i = 0; i < n; i++) {
      if (discarded[i]) continue;
      const int need = std::min(walk[i]->hypotheses(H.nIter), C[i].K - cursor[i]);
      const int seg = R.addSegment(C[i].corr.data(), C[i].N, C[i].camsD.data());
      firstHyp[i] = R.hypotheses();
      given[i] = need;
      for (int j = 0; j < need; j++) R.addHypothesis(seg, &C[i].Rt[12 * (size_t)(cursor[i] + j)]);
    }
    if (score(R) != ORBFE_OK) { printf("scoring failed: %s\n", last_error()); return 1; }
    for (int i = 0; i < n; i++) {
      if (discarded[i]) continue;
      bool noMore, wantNoMore, refineFailed = false;
      std::vector<bool> inl, wantInl;
      int nInl, wantN, consumed = 0;
      const int k0 = firstHyp[i];
      Candidate& c = C[i];
      int& rc = refCursor[i];
      // PnPsolver::Refine: "EPnP on the best inliers" is the next refined hypothesis of the list; its CheckInliers is one more call
      auto refine = [&](const std::vector<uint64_t>& bestMask, int& count, std::vector<uint64_t>& mask) {
        (void)bestMask;
        if (rc >= c.R) { refineFailed = true; return; }
        orbfe::PnPRound one;
        one.addHypothesis(one.addSegment(c.corr.data(), c.N, c.camsD.data()), &c.refined[12 * (size_t)rc++]);
        if (score(one) != ORBFE_OK) { refineFailed = true; return; }
        count = one.counts[0];
        mask = one.masks;
      };
      const int ret = walk[i]->iterate(H.nIter, R.counts.data() + k0, R.masks.data(), R.maskOff.data() + k0, given[i], cursor[i], noMore, inl, nInl, refine,
                                       &consumed);
      const int want = ref[i]->iterate(H.nIter, wantNoMore, wantInl, wantN);
      const bool same = !refineFailed && inl == wantInl && walk[i]->mnIterations == ref[i]->mnIterations &&
                        walk[i]->mnBestInliers == ref[i]->mnBestInliers && walk[i]->bestHypothesis == ref[i]->best &&
                        (size_t)rc == ref[i]->nextRefined && (ref[i]->best < 0 || same_mask(walk[i]->mvbBestInliers, ref[i]->mvbBestInliers, c.N));
      bad += line(round, i, ret, want, noMore, wantNoMore, nInl, wantN, walk[i]->mnIterations, walk[i]->bestHypothesis, consumed, same);
      cursor[i] += consumed;
      if (H.calls > 0 ? round + 1 >= H.calls : noMore || ret != orbfe::kPnPNone || want != -1) { discarded[i] = true; live--; }   // Relocalization: vbDiscarded / bMatch
    }
  }
  return bad;
}

int run(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { printf("cannot open %s\n", path); return 1; }
  Header H;
  bool ok = fread(&H, sizeof H, 1, f) == 1 && (H.model == 0 || H.model == 1) && H.n_cand > 0 && H.n_cand < 1000;
  std::vector<Candidate> C(ok ? H.n_cand : 0);
  for (auto& c : C) {
    int32_t h[4];
    ok = ok && fread(h, 4, 4, f) == 4;
    if (!ok) break;
    c.N = h[0]; c.nFull = h[1]; c.K = h[2]; c.R = h[3];
    ok = c.N >= 0 && c.K >= 0 && c.R >= 0 && readv(f, c.indices, (size_t)c.N);
    if (H.model == 0)
      ok = ok && readv(f, c.corr, 12 * (size_t)c.N) && readv(f, c.camsF, 8) && readv(f, c.T12, 12 * (size_t)c.K) && readv(f, c.T21, 12 * (size_t)c.K);
    else
      ok = ok && readv(f, c.corr, 6 * (size_t)c.N) && readv(f, c.camsD, 4) && readv(f, c.Rt, 12 * (size_t)c.K) && readv(f, c.refined, 12 * (size_t)c.R);
    for (int i : c.indices) ok = ok && i >= 0 && i < c.nFull;
  }
  fclose(f);
  if (!ok) { printf("bad scene file %s\n", path); return 1; }
  printf("%s: model %s candidates %d iterate(%d) minInliers %d maxIts %d\n", path, H.model ? "pnp" : "sim3", H.n_cand, H.nIter, H.minInliers, H.maxIts);
  const int bad = H.model == 0 ? run_sim3(H, C) : run_pnp(H, C);
  printf("%s: %s\n", path, bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}

// the packing helpers: (float)(size_t)(9.210*sigmaSquare) is 13 for sigmaSquare = 1.44f, not 13.26; mvSigma2[i]*th2 is a float product
int pack_check() {
  const float X[3] = {1.f, 2.f, 3.f}, Y[3] = {4.f, 5.f, 6.f}, p[2] = {7.f, 8.f}, q[2] = {9.f, 10.f};
  float row[12], prow[6];
  orbfe::Sim3Row(row, X, Y, p, q, 1.44f, 1.0f);
  orbfe::PnPRow(prow, 1.f, 2.f, 3.f, 4.f, 5.f, 1.44f, 5.991f);
  const float want[12] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f, 9.f, 10.f, 13.f, 9.f};
  const volatile float s2 = 1.44f, th2 = 5.991f;
  const float prod = s2 * th2;
  const bool ok = memcmp(row, want, sizeof want) == 0 && prow[5] == prod && prow[0] == 1.f && prow[4] == 5.f && orbfe::RansacWords(0) == 0 &&
                  orbfe::RansacWords(64) == 1 && orbfe::RansacWords(65) == 2;
  printf("pack: sim3 max %g %g pnp max %.9g %s\n", (double)row[10], (double)row[11], (double)prow[5], ok ? "ok" : "MISMATCH");
  return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
#ifndef RANSAC_SCORE_HOST
  if (orbfe_matcher_create(0, &g_matcher) != ORBFE_OK) { printf("no matcher: %s\nFAIL\n", orbfe_last_error()); return 1; }
#endif
  int bad = pack_check();
  for (int i = 1; i < argc; i++) bad += run(argv[i]);
#ifndef RANSAC_SCORE_HOST
  orbfe_matcher_destroy(g_matcher);
#endif
  printf("scenes %d mismatches %d\n", argc - 1, bad);
  printf(bad ? "FAIL\n" : "PASS\n");
  return bad ? 1 : 0;
}
