// os1_amd/csrc/extract_plan.h as a program of its own (no HIP, no GPU): the slot layout against the create-time formula it replaces
// (written out below), the hand-over between the GPU and the host quadtree at exactly 4 / 5 roots and 2 044 / 2 045 features on a
// level, the slots of wide strips, and the layout against the keypoint bound the C ABI reports.  Built plainly and with
// -fsanitize=address,undefined by tests/test_extract_plan.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "extract_plan.h"

using namespace orbfe;

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

namespace {
// mnFeaturesPerLevel and the level sizes as the extractor's constructor and ComputePyramid have them (ORBextractor.cc:447-478, :975-976)
struct Geometry {
  int nlevels;
  std::vector<int> nfeat, w, h;
  Geometry(int nfeatures, float scaleFactor, int nlevels_, int cols, int rows) : nlevels(nlevels_), nfeat(nlevels_), w(nlevels_), h(nlevels_) {
    const double scale = scaleFactor;
    std::vector<float> sf(nlevels, 1.0f);
    for (int i = 1; i < nlevels; i++) sf[i] = (float)(sf[i - 1] * scale);
    const float factor = (float)(1.0f / scale);
    float nDesired = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; l++) {
      nfeat[l] = (int)lrintf(nDesired);
      sum += nfeat[l];
      nDesired *= factor;
    }
    nfeat[nlevels - 1] = std::max(nfeatures - sum, 0);
    for (int l = 0; l < nlevels; l++) {
      w[l] = (int)lrintf((float)cols * (1.0f / sf[l]));
      h[l] = (int)lrintf((float)rows * (1.0f / sf[l]));
    }
  }
  int roots(int l) const { return (int)roundf(static_cast<float>(w[l] - 2 * kBorder) / (h[l] - 2 * kBorder)); }   // ORBextractor.cc:574
  ExtractPlan plan(long long candCap = 1 << 20) const { return extract_plan(nlevels, w.data(), h.data(), nfeat.data(), candCap); }
};

// one level of 132 rows: roots = round((w - 32) / 100)
ExtractPlan one_level(int w, int nfeat, long long candCap = 1 << 20) {
  const int h = 132;
  return extract_plan(1, &w, &h, &nfeat, candCap);
}
}  // namespace

int main() {
  const int nfeatures[3] = {200, 1000, 12000};
  const int sizes[4][3] = {{640, 480, 8}, {1920, 1080, 8}, {900, 180, 4}, {1600, 100, 3}};   // cols, rows, levels that still hold a FAST cell
  int inLimit = 0, wide = 0;
  for (int nf : nfeatures)
    for (const auto& s : sizes) {
      const Geometry g(nf, 1.2f, s[2], s[0], s[1]);
      const ExtractPlan p = g.plan();
      bool fewRoots = true, fewFeatures = true;
      for (int l = 0; l < g.nlevels; l++) {
        CHECK(g.roots(l) >= 1 && extract_level_roots(g.w[l], g.h[l]) == g.roots(l));
        fewRoots = fewRoots && g.roots(l) <= 4;
        fewFeatures = fewFeatures && g.nfeat[l] + 4 <= kQtNodeCap;
      }
      CHECK(p.gpuQuadtree == (fewRoots && fewFeatures));
      CHECK(p.selOff[0] == 0 && p.selOff[g.nlevels] == p.selPerFrame);
      if (fewRoots) {   // the layout orbfe_extractor_create used to fix, whatever the image size
        int off = 0;
        for (int l = 0; l < g.nlevels; l++) {
          CHECK(p.selOff[l] == off);
          off += std::max(g.nfeat[l] + 4, 16);
        }
        CHECK(p.selPerFrame == off);
        CHECK(p.selOff[1] - p.selOff[0] == extract_level_slots(g.nfeat[0], kExtractGpuRoots));   // what a match chain is sized by
        inLimit++;
      }
      // the keypoint bounds of the C ABI, as they were written there, and the layout against them
      int any4 = 0, forSize = 0;
      for (int l = 0; l < g.nlevels; l++) {
        any4 += std::max(g.nfeat[l] + 2, 16);
        forSize += std::max(g.nfeat[l] + 2, 4 * g.roots(l));
        const int slots = p.selOff[l + 1] - p.selOff[l];
        CHECK(slots >= std::max(g.nfeat[l] + 2, 4 * g.roots(l)));            // every keypoint the level can return has a slot
        if (4 * g.roots(l) > g.nfeat[l] + 4) { CHECK(slots == 4 * g.roots(l)); wide++; }
      }
      CHECK(extract_max_keypoints(g.nlevels, g.nfeat.data()) == any4);
      CHECK(extract_max_keypoints(g.nlevels, g.nfeat.data(), g.w.data(), g.h.data()) == forSize);
      CHECK(p.selPerFrame >= forSize && p.selPerFrame <= forSize + kExtractSlotSlack * g.nlevels);
    }
  CHECK(inLimit == 6 && wide > 0);   // 640 x 480 and 1920 x 1080 at every nfeatures; both strips have more than 4 roots

  {   // 1600 x 100, nfeatures 200, 3 levels (tests/test_gpu_stream_transitions.py): every level's slots are the first sweep's 4 * roots
    const Geometry g(200, 1.2f, 3, 1600, 100);
    const ExtractPlan p = g.plan();
    CHECK(!p.gpuQuadtree);
    CHECK(g.nfeat[0] == 79 && g.roots(0) == 23);
    for (int l = 0; l < 3; l++) {
      CHECK(g.roots(l) >= 23 && g.roots(l) <= 29 && 4 * g.roots(l) > g.nfeat[l] + 4);
      CHECK(p.selOff[l + 1] - p.selOff[l] == 4 * g.roots(l));
    }
    CHECK(p.selPerFrame == extract_max_keypoints(3, g.nfeat.data(), g.w.data(), g.h.data()));
  }

  // the hand-over: 4 roots GPU, 5 host (round(4.49) = 4, round(4.5) = 5); no root at all is the host's too
  CHECK(one_level(32 + 400, 500).gpuQuadtree && !one_level(32 + 500, 500).gpuQuadtree);
  CHECK(one_level(32 + 449, 500).gpuQuadtree && !one_level(32 + 450, 500).gpuQuadtree);
  CHECK(one_level(32 + 100, 500).gpuQuadtree && !one_level(32 + 49, 500).gpuQuadtree);
  CHECK(one_level(32 + 500, 500).selPerFrame == 504 && one_level(32 + 500, 3).selPerFrame == 20 && one_level(32 + 400, 3).selPerFrame == 16);
  // kQtNodeCap - 4 features on a level GPU, one more host; the layout does not care
  CHECK(kQtNodeCap == 2048);
  CHECK(one_level(432, kQtNodeCap - 4).gpuQuadtree && !one_level(432, kQtNodeCap - 3).gpuQuadtree);
  CHECK(one_level(432, kQtNodeCap - 4).selPerFrame == kQtNodeCap && one_level(432, kQtNodeCap - 3).selPerFrame == kQtNodeCap + 1);
  // a candidate index must fit 24 bits
  CHECK(one_level(432, 500, (1ll << 24) - 1).gpuQuadtree && !one_level(432, 500, 1ll << 24).gpuQuadtree);
  // the slack is reached, and only by the smallest quotas
  CHECK(extract_level_slots(0, 1) - extract_level_keypoints(0, 1) == kExtractSlotSlack);
  for (int n = 0; n < 40; n++)
    for (int r = 1; r < 40; r++) {
      const int d = extract_level_slots(n, r) - extract_level_keypoints(n, r);
      CHECK(d >= 0 && d <= kExtractSlotSlack);
    }
  std::printf("PASS\n");
  return 0;
}
