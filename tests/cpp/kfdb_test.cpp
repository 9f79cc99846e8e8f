// kfdb_test.cpp -- orbfe::KeyFrameDatabaseT of include/orbfe/orb_shim.hpp (what include/orbfe/KeyFrameDatabase.h binds to the
// reference's types; GPU, through orbfe_kfdb_*) against the reference restatement tests/cpp/kfdb_ref.cpp, on the scenes
// tests/kfdb_util.py writes (argv[1..]: scene files).  The stand-in KeyFrame / Frame expose the member names
// KeyFrameDatabase.cc and LoopClosing.cc:125-140 use.  After EVERY step -- add, erase, clear, DetectLoopCandidates,
// DetectRelocalizationCandidates -- the returned vector and all six members of every keyframe are compared with the
// restatement's.  Where a file <scene file>.expect lies beside a scene file (tests/kfdb_util.py write_expected: the recorded
// outputs of the reference's own compiled KeyFrameDatabase.cc, tests/golden/os1_kfdb_outputs.npz), the returned vector and the
// members are compared with that recording as well.  Prints the restatement's counters and PASS; exit code 0 iff every
// comparison is exact.
//   build: g++ -std=c++17 -O1 -ffp-contract=off -Iinclude tests/cpp/kfdb_test.cpp tests/cpp/kfdb_ref.cpp os1_amd/liborbfe.so
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "orbfe/orb_shim.hpp"

extern "C" {
void* kref_create(int n_words, int scoring);
void kref_destroy(void* h);
int kref_new_kf(void* h, uint64_t mnId, const unsigned* words, const double* values, int n);
void kref_set_connected(void* h, int kf, const int* others, int n);
void kref_set_covisible(void* h, int kf, const int* others, int n);
void kref_set_bad(void* h, int kf, int bad);
void kref_add(void* h, int kf);
void kref_erase(void* h, int kf);
void kref_clear(void* h);
int kref_detect_loop(void* h, int kf, float minScore, int* out, int cap);
int kref_detect_reloc(void* h, uint64_t frame_id, const unsigned* words, const double* values, int n, int* out, int cap);
float kref_min_covisible_score(void* h, int kf);
void kref_members(void* h, int kf, uint64_t* queries, int32_t* words, float* scores);
void kref_counters(void* h, long* out);
}

typedef std::map<unsigned int, double> BowVector;
struct KeyFrame {
  long unsigned int mnId = 0;
  BowVector mBowVec;
  long unsigned int mnLoopQuery = 0;   // KeyFrame.cc:44
  int mnLoopWords = 0;
  float mLoopScore = 0;                // (uninitialised in the reference; 0 here and in the restatement's model)
  long unsigned int mnRelocQuery = 0;
  int mnRelocWords = 0;
  float mRelocScore = 0;
  bool bad = false;
  int index = 0;
  std::set<KeyFrame*> connected;
  std::vector<KeyFrame*> covisible;
  std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return covisible; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    if ((int)covisible.size() < N) return covisible;
    return std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
  }
  bool isBad() { return bad; }
};
struct Frame {
  long unsigned int mnId = 0;
  BowVector mBowVec;
};

static FILE* g_f;
template <class T>
static T rd() {
  T v;
  if (fread(&v, sizeof v, 1, g_f) != 1) { printf("FAIL: short scene file\n"); exit(2); }
  return v;
}
template <class T>
static std::vector<T> rdv(int n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, g_f) != (size_t)n) { printf("FAIL: short scene file\n"); exit(2); }
  return v;
}

static long g_checks = 0, g_refChecks = 0, g_refQueries = 0;

// The recording of the reference object for one scene: per step the candidate count (-1: a mutation) and indices, then
// {mnLoopQuery u64, mnLoopWords i32, mLoopScore bits u32, mnRelocQuery u64, mnRelocWords i32, mRelocScore bits u32} per keyframe.
struct Expected {
  FILE* f = nullptr;
  bool open(const char* scene, int nSteps, int nKf) {
    f = fopen((std::string(scene) + ".expect").c_str(), "rb");
    if (!f) return true;   // no recording beside this scene
    int h[2];
    if (fread(h, 4, 2, f) != 2 || h[0] != nSteps || h[1] != nKf) { printf("FAIL: %s.expect does not belong to the scene\n", scene); return false; }
    return true;
  }
  template <class KF>
  bool step(int s, const char* what, bool isQuery, const std::vector<KF*>& got, const std::vector<KF>& kfs) {
    if (!f) return true;
    int n;
    if (fread(&n, 4, 1, f) != 1) { printf("FAIL: short .expect file\n"); return false; }
    std::vector<int> want(n > 0 ? n : 0);
    if (n > 0 && fread(want.data(), 4, n, f) != (size_t)n) { printf("FAIL: short .expect file\n"); return false; }
    if ((n >= 0) != isQuery) { printf("FAIL: step %d (%s): the recording has another kind of step\n", s, what); return false; }
    if (isQuery) {
      g_refQueries++;
      bool ok = (int)got.size() == n;
      for (int i = 0; ok && i < n; i++) ok = got[i]->index == want[i];
      if (!ok) { printf("FAIL: step %d (%s): %zu candidates vs %d of the reference object\n", s, what, got.size(), n); return false; }
    }
    for (const KF& k : kfs) {
      uint64_t q[2]; int32_t w[2]; uint32_t b[2];
      if (fread(&q[0], 8, 1, f) != 1 || fread(&w[0], 4, 1, f) != 1 || fread(&b[0], 4, 1, f) != 1 || fread(&q[1], 8, 1, f) != 1 ||
          fread(&w[1], 4, 1, f) != 1 || fread(&b[1], 4, 1, f) != 1) { printf("FAIL: short .expect file\n"); return false; }
      g_refChecks++;
      if (q[0] != k.mnLoopQuery || q[1] != k.mnRelocQuery || w[0] != k.mnLoopWords || w[1] != k.mnRelocWords ||
          memcmp(&b[0], &k.mLoopScore, 4) || memcmp(&b[1], &k.mRelocScore, 4)) {
        printf("FAIL: step %d (%s): members of keyframe %d differ from the reference object's: loop %lu/%d/%.9g vs %llu/%d/%08x, reloc "
               "%lu/%d/%.9g vs %llu/%d/%08x\n", s, what, k.index, k.mnLoopQuery, k.mnLoopWords, k.mLoopScore, (unsigned long long)q[0], w[0],
               b[0], k.mnRelocQuery, k.mnRelocWords, k.mRelocScore, (unsigned long long)q[1], w[1], b[1]);
        return false;
      }
    }
    return true;
  }
  ~Expected() { if (f) fclose(f); }
};
static bool same_members(void* ref, std::vector<KeyFrame>& kfs, const char* what, int step) {
  for (KeyFrame& k : kfs) {
    uint64_t q[2]; int32_t w[2]; float s[2];
    kref_members(ref, k.index, q, w, s);
    g_checks++;
    if (q[0] != k.mnLoopQuery || q[1] != k.mnRelocQuery || w[0] != k.mnLoopWords || w[1] != k.mnRelocWords ||
        memcmp(&s[0], &k.mLoopScore, 4) || memcmp(&s[1], &k.mRelocScore, 4)) {
      printf("FAIL: step %d (%s): members of keyframe %d differ: loop %lu/%d/%.9g vs %llu/%d/%.9g, reloc %lu/%d/%.9g vs %llu/%d/%.9g\n",
             step, what, k.index, k.mnLoopQuery, k.mnLoopWords, k.mLoopScore, (unsigned long long)q[0], w[0], s[0], k.mnRelocQuery,
             k.mnRelocWords, k.mRelocScore, (unsigned long long)q[1], w[1], s[1]);
      return false;
    }
  }
  return true;
}

static int run_scene(const char* path, long totals[8]) {
  g_f = fopen(path, "rb");
  if (!g_f) { printf("FAIL: cannot open %s\n", path); return 1; }
  const int nWords = rd<int>(), scoring = rd<int>(), nKf = rd<int>(), nSteps = rd<int>(), capK = rd<int>(), capE = rd<int>();
  void* ref = kref_create(nWords, scoring);
  std::vector<KeyFrame> kfs(nKf);
  std::vector<std::vector<int> > conn(nKf), cov(nKf);
  for (int i = 0; i < nKf; i++) {
    const uint64_t id = rd<uint64_t>();
    const int n = rd<int>(), nc = rd<int>(), nv = rd<int>(), bad = rd<int>();
    std::vector<unsigned> w = rdv<unsigned>(n);
    std::vector<double> v = rdv<double>(n);
    conn[i] = rdv<int>(nc);
    cov[i] = rdv<int>(nv);
    kfs[i].index = i; kfs[i].mnId = (unsigned long)id; kfs[i].bad = bad != 0;
    for (int j = 0; j < n; j++) kfs[i].mBowVec[w[j]] = v[j];
    if (kref_new_kf(ref, id, w.data(), v.data(), n) != i) return 1;
  }
  for (int i = 0; i < nKf; i++) {
    for (int j : conn[i]) kfs[i].connected.insert(&kfs[j]);
    for (int j : cov[i]) kfs[i].covisible.push_back(&kfs[j]);
    kref_set_connected(ref, i, conn[i].data(), (int)conn[i].size());
    kref_set_covisible(ref, i, cov[i].data(), (int)cov[i].size());
    kref_set_bad(ref, i, kfs[i].bad);
  }
  // the scene's own (tight) capacities: the visit of a keyframe that is not in the database makes the facade grow its pool
  orbfe::KeyFrameDatabaseT<KeyFrame> db(0, (size_t)nWords, scoring, capK, capE);
  std::vector<int> want(nKf);
  int queries = 0;
  Expected expected;
  if (!expected.open(path, nSteps, nKf)) return 1;
  for (int s = 0; s < nSteps; s++) {
    const int type = rd<int>(), kf = rd<int>();
    const uint64_t fid = rd<uint64_t>();
    float ms = rd<float>();
    const int hasMs = rd<int>(), n = rd<int>();
    std::vector<unsigned> w = rdv<unsigned>(n);
    std::vector<double> v = rdv<double>(n);
    const char* what = type == 0 ? "add" : type == 1 ? "erase" : type == 2 ? "clear" : type == 3 ? "loop" : "reloc";
    std::vector<KeyFrame*> got;
    int nWant = -1;
    if (type == 0) { db.add(&kfs[kf]); kref_add(ref, kf); }
    else if (type == 1) { db.erase(&kfs[kf]); kref_erase(ref, kf); }
    else if (type == 2) { db.clear(); kref_clear(ref); }
    else if (type == 3) {
      if (!hasMs) {   // LoopClosing.cc:125-140
        ms = db.MinCovisibleScore(&kfs[kf]);
        const float r = kref_min_covisible_score(ref, kf);
        if (memcmp(&ms, &r, 4)) { printf("FAIL: step %d: covisible minimum score %.9g vs %.9g\n", s, ms, r); return 1; }
      }
      got = db.DetectLoopCandidates(&kfs[kf], ms);
      nWant = kref_detect_loop(ref, kf, ms, want.data(), nKf);
    } else {
      Frame F;
      F.mnId = (unsigned long)fid;
      for (int j = 0; j < n; j++) F.mBowVec[w[j]] = v[j];
      got = db.DetectRelocalizationCandidates(&F);
      nWant = kref_detect_reloc(ref, fid, w.data(), v.data(), n, want.data(), nKf);
    }
    if (nWant >= 0) {
      queries++;
      bool ok = (int)got.size() == nWant;
      for (int i = 0; ok && i < nWant; i++) ok = got[i]->index == want[i];
      if (!ok) { printf("FAIL: step %d (%s): %zu candidates vs %d\n", s, what, got.size(), nWant); return 1; }
    }
    if (!same_members(ref, kfs, what, s)) return 1;
    if (!expected.step(s, what, nWant >= 0, got, kfs)) return 1;
  }
  long c[8];
  kref_counters(ref, c);
  for (int i = 0; i < 8; i++) totals[i] += c[i];
  totals[5] += queries;
  kref_destroy(ref);
  fclose(g_f);
  return 0;
}

int main(int argc, char** argv) {
  long totals[8] = {0};
  try {
    for (int i = 1; i < argc; i++)
      if (run_scene(argv[i], totals)) return 1;
  } catch (const std::exception& e) {
    printf("FAIL: %s\n", e.what());
    return 1;
  }
  printf("scenes %d candidates %ld duplicates %ld stale %ld connected_skips %ld best_other %ld queries %ld checks %ld ref_queries %ld "
         "ref_checks %ld\n", argc - 1, totals[0], totals[1], totals[2], totals[3], totals[4], totals[5], g_checks, g_refQueries, g_refChecks);
  printf("PASS\n");
  return 0;
}
