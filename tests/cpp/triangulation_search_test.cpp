// triangulation_search_test.cpp -- drives include/orbfe/TriangulationSearch.h the way LocalMapping::CreateNewMapPoints would
// (LocalMapping.cc:207-364): one keyframe against its neighbours, MapPoints added to the current keyframe between neighbours.
// S.pairs(i, ...) is compared with the existing orbfe::SearchForTriangulation called inside the same loop; the pairs of the
// facade's loop are written out so that tests/test_gpu_triangulation_batch.py compares them with the reference's.
//   usage: triangulation_search_test <dir>     reads <dir>/meta.txt (number of neighbours) and kf0 (current), kf1 .. kfK:
//          kfJ.kps (cv::KeyPoint records), .desc (32-byte rows), .has (1 byte per keypoint), .fv (node, count, features ...),
//          and for J >= 1 .geo (F12[9], ex, ey, scale factors[8], level sigma2[8]); writes <dir>/pairs_ori{0,1}_nb{i}.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "orbfe/TriangulationSearch.h"

struct KeyPoint { float x, y, size, angle, response; int octave, class_id; };  // cv::KeyPoint layout
struct Mat {  // the three public cv::Mat members the shim touches
  unsigned char* data = nullptr;
  size_t step = 0;
  int rows = 0;
};
struct Vec3 {   // GetCameraCenter() / GetTranslation() as far as the epipole lines read them
  float v[3];
  template <class T> T at(int i) const { return v[i]; }
  Vec3 operator+(const Vec3& o) const { return Vec3{{v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]}}; }
};
struct Rot3 {   // GetRotation()
  float m[9];
  Vec3 operator*(const Vec3& x) const {
    return Vec3{{m[0] * x.v[0] + m[1] * x.v[1] + m[2] * x.v[2], m[3] * x.v[0] + m[4] * x.v[1] + m[5] * x.v[2], m[6] * x.v[0] + m[7] * x.v[1] + m[8] * x.v[2]}};
  }
};
struct MapPoint { int dummy = 0; };
typedef std::map<unsigned, double> BowVector;
typedef std::map<unsigned, std::vector<unsigned> > FeatureVector;
struct KeyFrame {
  int N = 0;
  BowVector mBowVec;
  FeatureVector mFeatVec;
  std::vector<KeyPoint> mvKeys, mvKeysUn;
  std::vector<unsigned char> descStore;
  Mat mDescriptors;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<float> mvScaleFactors, mvLevelSigma2;
  static float mnMinX, mnMaxX, mnMinY, mnMaxY;
  float fx = 1.f, fy = 1.f, cx = 0.f, cy = 0.f;
  Vec3 Ow{{0, 0, 0}}, tcw{{0, 0, 1}};
  MapPoint* GetMapPoint(size_t i) { return mvpMapPoints[i]; }
  Vec3 GetCameraCenter() { return Ow; }
  Rot3 GetRotation() { return Rot3{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; }
  Vec3 GetTranslation() { return tcw; }
};
float KeyFrame::mnMinX = 0, KeyFrame::mnMaxX = 640, KeyFrame::mnMinY = 0, KeyFrame::mnMaxY = 480;
struct Mat33f {
  float v[9];
  template <class T> T at(int r, int c) const { return v[3 * r + c]; }
};
typedef std::vector<std::pair<size_t, size_t> > Pairs;

static std::vector<unsigned char> readFile(const std::string& p) {
  FILE* f = fopen(p.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", p.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<unsigned char> v(n);
  if (n && fread(v.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return v;
}

static MapPoint g_point;
static std::vector<std::vector<unsigned char> > g_has;   // the flags at loop entry, per keyframe

static void resetFlags(std::vector<KeyFrame>& kf) {
  for (size_t j = 0; j < kf.size(); j++)
    for (int i = 0; i < kf[j].N; i++) kf[j].mvpMapPoints[i] = g_has[j][i] ? &g_point : nullptr;
}
// which pairs "CreateNewMapPoints" triangulates: a fixed rule the Python side restates
static void addMapPoints(KeyFrame& kf1, const Pairs& p, size_t i) {
  for (auto& pr : p)
    if ((pr.first * 7 + pr.second * 3 + i) % 5 < 3) kf1.mvpMapPoints[pr.first] = &g_point;
}
#define REQUIRE(c, code) do { if (!(c)) { fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); return code; } } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  int K = 0;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%d", &K) != 1) return 2;
    fclose(f);
  }
  std::vector<KeyFrame> kf(K + 1);
  std::vector<Mat33f> vF12(K);
  std::vector<float> wantEx(K), wantEy(K);
  g_has.resize(K + 1);
  for (int j = 0; j <= K; j++) {
    const std::string b = dir + "/kf" + std::to_string(j);
    KeyFrame& k = kf[j];
    std::vector<unsigned char> kp = readFile(b + ".kps");
    k.N = (int)(kp.size() / sizeof(KeyPoint));
    k.mvKeysUn.resize(k.N);
    if (k.N) memcpy(k.mvKeysUn.data(), kp.data(), kp.size());
    k.mvKeys = k.mvKeysUn;
    k.descStore = readFile(b + ".desc");
    k.mDescriptors.data = k.descStore.data(); k.mDescriptors.step = 32; k.mDescriptors.rows = k.N;
    g_has[j] = readFile(b + ".has");
    k.mvpMapPoints.assign(k.N, nullptr);
    std::vector<unsigned char> fv = readFile(b + ".fv");
    const unsigned* w = reinterpret_cast<const unsigned*>(fv.data());
    for (size_t at = 0; at < fv.size() / 4;) {
      const unsigned node = w[at], cnt = w[at + 1];
      k.mFeatVec[node].assign(w + at + 2, w + at + 2 + cnt);
      at += 2 + cnt;
    }
    if (j == 0) continue;
    std::vector<unsigned char> geo = readFile(b + ".geo");
    const float* g = reinterpret_cast<const float*>(geo.data());
    memcpy(vF12[j - 1].v, g, 36);
    wantEx[j - 1] = g[9]; wantEy[j - 1] = g[10];
    k.tcw = Vec3{{g[9], g[10], 1.f}};   // identity rotation, camera 1 at the origin, fx = fy = 1, cx = cy = 0: the epipole IS (tx, ty)
    k.mvScaleFactors.assign(g + 11, g + 19);
    k.mvLevelSigma2.assign(g + 19, g + 27);
  }
  kf[0].mvScaleFactors = kf[1].mvScaleFactors; kf[0].mvLevelSigma2 = kf[1].mvLevelSigma2;
  std::vector<KeyFrame*> vpNeigh;
  for (int j = 1; j <= K; j++) vpNeigh.push_back(&kf[j]);
  orbfe::MatcherContext ctx;
  for (int ori = 0; ori < 2; ori++) {
    // the loop on the existing single search
    resetFlags(kf);
    std::vector<Pairs> want(K);
    std::vector<int> wantN(K);
    for (int i = 0; i < K; i++) {
      wantN[i] = orbfe::SearchForTriangulation(ctx, ori != 0, &kf[0], vpNeigh[i], vF12[i], wantEx[i], wantEy[i], want[i]);
      addMapPoints(kf[0], want[i], i);
    }
    // the same loop on the facade: one call in front, pairs(i) reads the flags as they stand
    resetFlags(kf);
    const size_t uploads0 = ctx.residentUploads(), held0 = ctx.residentFrames();
    REQUIRE(ori != 0 || held0 == 0, 10);             // the single search keeps nothing resident
    orbfe::TriangulationSearch<KeyFrame> S(ctx, ori != 0, &kf[0], vpNeigh, vF12);
    REQUIRE(S.batched() && S.size() == (size_t)K, 11);
    REQUIRE(ctx.residentFrames() == (size_t)K + 1, 12);                                   // made resident on first use ...
    REQUIRE(ori != 0 || ctx.residentUploads() == uploads0 + (size_t)K + 1, 13);
    const size_t uploads1 = ctx.residentUploads();
    size_t total = 0, grown = 0;
    for (int i = 0; i < K; i++) {
      REQUIRE(S.ex(i) == wantEx[i] && S.ey(i) == wantEy[i], 14);
      Pairs got;
      const int n = S.pairs(i, got);
      REQUIRE(n == wantN[i] && got == want[i], 15);
      std::vector<int> flat;
      for (auto& pr : got) { flat.push_back((int)pr.first); flat.push_back((int)pr.second); }
      FILE* f = fopen((dir + "/pairs_ori" + std::to_string(ori) + "_nb" + std::to_string(i) + ".bin").c_str(), "wb");
      if (!flat.empty()) fwrite(flat.data(), 4, flat.size(), f);
      fclose(f);
      addMapPoints(kf[0], got, i);
      total += got.size();
    }
    for (int i = 0; i < kf[0].N; i++) grown += (kf[0].mvpMapPoints[i] != nullptr) != (g_has[0][i] != 0);
    REQUIRE(S.fallbacks() == 0 && total > 20 && grown > 10, 16);
    // a MapPoint taken AWAY from the current keyframe after the call: the raw rows do not cover that keypoint, pairs() searches singly
    resetFlags(kf);
    orbfe::TriangulationSearch<KeyFrame> S2(ctx, ori != 0, &kf[0], vpNeigh, vF12);
    REQUIRE(S2.batched() && ctx.residentUploads() == uploads1 && ctx.residentFrames() == (size_t)K + 1, 24);   // ... and found there the second time
    int cleared = -1;
    for (int i = 0; i < kf[0].N && cleared < 0; i++)
      if (kf[0].mvpMapPoints[i]) { kf[0].mvpMapPoints[i] = nullptr; cleared = i; }
    REQUIRE(cleared >= 0, 17);
    for (int i = 0; i < K; i++) {
      Pairs single, got;
      const int ns = orbfe::SearchForTriangulation(ctx, ori != 0, &kf[0], vpNeigh[i], vF12[i], wantEx[i], wantEy[i], single);
      REQUIRE(S2.pairs(i, got) == ns && got == single, 18);
    }
    REQUIRE(S2.fallbacks() == K, 19);
    // a frame cache that cannot hold the K + 1 keyframes at once: no batch, the single search for every neighbour, same pairs
    resetFlags(kf);
    ctx.setFrameCacheCapacity(2);
    orbfe::TriangulationSearch<KeyFrame> S3(ctx, ori != 0, &kf[0], vpNeigh, vF12);
    REQUIRE(!S3.batched(), 20);
    for (int i = 0; i < K; i++) {
      Pairs got;
      REQUIRE(S3.pairs(i, got) == wantN[i] && got == want[i], 21);
      addMapPoints(kf[0], got, i);
    }
    REQUIRE(S3.fallbacks() == K, 22);
    ctx.setFrameCacheCapacity(48);
  }
  {   // no neighbour at all
    std::vector<KeyFrame*> none;
    std::vector<Mat33f> noF;
    orbfe::TriangulationSearch<KeyFrame> S0(ctx, true, &kf[0], none, noF);
    REQUIRE(S0.size() == 0 && !S0.batched(), 23);
  }
  printf("triangulation_search_test ok\n");
  return 0;
}
