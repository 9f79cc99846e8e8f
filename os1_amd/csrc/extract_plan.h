// extract_plan.h -- the slot layout of the extractor's result arena and the choice of the selection stage (orbfe_extractor.hip), free of
// HIP so that a plain host program can exercise it (tests/cpp/extract_plan_test.cpp).  Level sizes and per-level quotas in; slot
// offsets, the per-frame slot count and the route out.  One copy of each rule: setGeometry, orbfe_extractor_create (the match chain's
// level-0 capacity) and orbfe_extractor_max_keypoints* all come here.
#pragma once
#include <algorithm>
#include <cmath>

#include "orbfe_internal.h"

namespace orbfe {

// Root nodes of DistributeOctTree on a level of w x h pixels (ORBextractor.cc:574-578); 0 for a level no taller than its border.
inline int extract_level_roots(int w, int h) {
  if (h <= 2 * kBorder) return 0;
  const int roots = (int)roundf(static_cast<float>(w - 2 * kBorder) / (h - 2 * kBorder));
  return roots < 0 ? 0 : roots;
}

// Keypoints a level can return: the first sweep of DistributeOctTree divides every root before any size check (ORBextractor.cc:620-700),
// later ones overshoot the quota N_l by at most 2.
inline int extract_level_keypoints(int nfeat, int roots) { return std::max(nfeat + 2, 4 * roots); }

// Slots the arena keeps for a level: the bound above with a margin of two, and never less than four roots' worth.  For 1..4 roots
// this is max(N_l + 4, 16), whatever the image size; a wider strip's level holds the 4 * roots keypoints of the first sweep.
inline int extract_level_slots(int nfeat, int roots) { return std::max(nfeat + 4, 4 * std::max(roots, 4)); }
// extract_level_slots - extract_level_keypoints is at most this (reached by a one-root level with a quota of 0..2: 16 slots, 4 keypoints)
constexpr int kExtractSlotSlack = 12;

constexpr int kExtractGpuRoots = 4;   // roots k_quadtree3 holds per level

struct ExtractPlan {
  int selOff[kMaxLevels + 1];   // first slot of every level inside a frame's slot region; [nlevels] = selPerFrame
  int selPerFrame;
  bool gpuQuadtree;             // k_quadtree3 holds this geometry; otherwise quadtree.h selects on the host
};

// levW / levH: level sizes in pixels; nfeat: mnFeaturesPerLevel; candCap: candidate capacity per frame (k_quadtree3 packs a candidate
// index into 24 bits).
inline ExtractPlan extract_plan(int nlevels, const int* levW, const int* levH, const int* nfeat, long long candCap) {
  ExtractPlan p{};
  p.gpuQuadtree = candCap < (1ll << 24);
  for (int l = 0; l < nlevels; l++) {
    const int roots = extract_level_roots(levW[l], levH[l]);
    if (roots < 1 || roots > kExtractGpuRoots || nfeat[l] + 4 > kQtNodeCap) p.gpuQuadtree = false;
    p.selOff[l] = p.selPerFrame;
    p.selPerFrame += extract_level_slots(nfeat[l], roots);
  }
  p.selOff[nlevels] = p.selPerFrame;
  return p;
}

// Upper bound on the keypoints of one frame.  levW == nullptr: for any image with at most four roots per level.
inline int extract_max_keypoints(int nlevels, const int* nfeat, const int* levW = nullptr, const int* levH = nullptr) {
  int n = 0;
  for (int l = 0; l < nlevels; l++) n += extract_level_keypoints(nfeat[l], levW ? extract_level_roots(levW[l], levH[l]) : kExtractGpuRoots);
  return n;
}

}  // namespace orbfe
