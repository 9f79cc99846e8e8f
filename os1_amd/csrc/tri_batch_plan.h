// tri_batch_plan.h -- the host-side bookkeeping of orbfe_search_for_triangulation_frames_batch (orbfe_bow.hip), free of HIP so
// that a plain host program can exercise it (tests/cpp/tri_batch_plan_test.cpp, also under the address and undefined-behaviour
// sanitizers):
//   * the argument check of the current keyframe (side 1) and of every neighbour (side 2) before anything is sent;
//   * the common vocabulary nodes of side 1 with each neighbour, as one record list for k_bow_triangulate_batch;
//   * where each part of the call's upload image lies, and how many entries the call writes.
// What crosses the link per keyframe is its feature lists (4 bytes per feature) and its MapPoint flags (1 byte per keypoint);
// keypoints and descriptor rows are read from the resident frames.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace orbfe {

constexpr int kTriBatchOk = 0, kTriBatchInvalid = -1, kTriBatchOverflow = -5;   // ORBFE_OK, ORBFE_ERR_INVALID, ORBFE_ERR_OVERFLOW
constexpr int kTriMaxGroup = 65535;                  // features of one neighbour under one node: a position is 16 bits of a key
constexpr int kTriMaxLevels = 16;                    // entries of the per-neighbour scale / sigma2 tables
constexpr uint64_t kTriMaxEntries = 0x7fffffffull;   // n_nb x n1 entries of matches12_raw, and every offset of the image
constexpr size_t kTriAlign = 256;                    // the parts of the image start on multiples of it

// one keyframe as the plan sees it: what the resident frame says of itself, and the host arrays of the call
struct TriSide {
  bool frame = false;          // the frame handle is not NULL
  int device = -1;             // orbfe_frame_device
  int n = 0;                   // orbfe_frame_size
  int maxOctave = 0;           // the frame's largest octave (INT_MAX if one is negative)
  const uint8_t* has_mp = nullptr;
  const uint32_t *nodes = nullptr, *offsets = nullptr, *features = nullptr;
  int n_fv = 0;
  int nlevels = 1;             // side 2 only
  bool tables = true;          // side 2 only: scale_factors2 and level_sigma2_2 are not NULL
};

// (neighbour, common vocabulary node): [b1, e1) of side 1's feature list, [b2, e2) of the image's side-2 feature part, the first
// entry of the neighbour's row of matches12_raw, the neighbour.  The layout of BowPair (orbfe_bow.hip).
struct TriRecord { int b1, e1, b2, e2, base1, nb; };

struct TriBatchPlan {
  std::vector<TriRecord> records;    // node-major: all neighbours of side 1's first common node, then the next node's, ...
  std::vector<uint32_t> flag2, feat2;   // [n_nb]: where neighbour k's flags / features start inside their parts (bytes / entries)
  size_t oTable = 0, oRecords = 0, oFlag1 = 0, oFeat1 = 0, oFlag2 = 0, oFeat2 = 0, bytes = 0;   // the upload image
  size_t nFeat1 = 0, nFlag2 = 0, nFeat2 = 0;
  uint64_t entries = 0;              // n_nb x n1: what the kernel's output holds, and no index of it is larger
  int failed = -1;                   // the neighbour a non-zero return value names; -1: side 1 or the call
  char why[200] = {0};
};

inline size_t tri_al(size_t b) { return (b + kTriAlign - 1) / kTriAlign * kTriAlign; }

inline int tri_refuse(TriBatchPlan& plan, int code, int nb, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
  char msg[160];
  std::snprintf(msg, sizeof msg, fmt, a, b, c);
  if (nb >= 0) std::snprintf(plan.why, sizeof plan.why, "neighbour %d: %s", nb, msg);
  else std::snprintf(plan.why, sizeof plan.why, "%s", msg);
  plan.failed = nb;
  plan.records.clear();
  return code;
}

// the FeatureVector of one side: offsets ascend from 0, nodes ascend strictly (a std::map's order), every index is a keypoint
inline int tri_check_fv(const TriSide& s, int nb, TriBatchPlan& plan) {
  if (s.n_fv < 0) return tri_refuse(plan, kTriBatchInvalid, nb, "negative number of vocabulary nodes (%lld)", s.n_fv);
  if (s.n_fv == 0) return kTriBatchOk;
  if (!s.nodes || !s.offsets || !s.features) return tri_refuse(plan, kTriBatchInvalid, nb, "null feature-vector pointer");
  if (s.offsets[0] != 0) return tri_refuse(plan, kTriBatchInvalid, nb, "feature-vector offsets start at %lld, not 0", s.offsets[0]);
  for (int a = 0; a < s.n_fv; a++) {
    if (s.offsets[a + 1] < s.offsets[a]) return tri_refuse(plan, kTriBatchInvalid, nb, "feature-vector offsets decrease at node %lld", a);
    if (a > 0 && s.nodes[a] <= s.nodes[a - 1]) return tri_refuse(plan, kTriBatchInvalid, nb, "vocabulary nodes do not ascend at entry %lld", a);
  }
  if ((uint64_t)s.offsets[s.n_fv] > kTriMaxEntries) return tri_refuse(plan, kTriBatchOverflow, nb, "%lld features in one feature vector", s.offsets[s.n_fv]);
  for (uint32_t i = 0; i < s.offsets[s.n_fv]; i++)
    if (s.features[i] >= (uint32_t)s.n) return tri_refuse(plan, kTriBatchInvalid, nb, "feature index %lld is not below the frame's %lld keypoints", s.features[i], s.n);
  return kTriBatchOk;
}

// Common vocabulary nodes of two checked FeatureVectors (the lower_bound zig-zag of ORBmatcher.cc:686-770 visits exactly the
// intersection, in ascending order) as feature ranges into the two sides' own lists; nodes empty on either side are left out.
// node1[i]: the index of record i's node in side 1's FeatureVector.
inline void tri_common_nodes(const TriSide& s1, const TriSide& s2, std::vector<TriRecord>& out, std::vector<int>* node1 = nullptr) {
  out.clear();
  if (node1) node1->clear();
  for (int a = 0, b = 0; a < s1.n_fv && b < s2.n_fv;) {
    if (s1.nodes[a] == s2.nodes[b]) {
      const TriRecord r = {(int)s1.offsets[a], (int)s1.offsets[a + 1], (int)s2.offsets[b], (int)s2.offsets[b + 1], 0, 0};
      if (r.e1 > r.b1 && r.e2 > r.b2) {
        out.push_back(r);
        if (node1) node1->push_back(a);
      }
      a++; b++;
    } else if (s1.nodes[a] < s2.nodes[b]) a++;
    else b++;
  }
}

// Everything the C call refuses, before anything is sent; then the record list and the image's layout.  tableBytes: bytes of
// one entry of the per-neighbour table.  On a non-zero return plan.why says what is wrong and plan.failed which neighbour
// (-1: side 1), and the plan holds no record.
inline int tri_batch_plan(int device, const TriSide& s1, int n_nb, const TriSide* nb, size_t tableBytes, TriBatchPlan& plan) {
  plan = TriBatchPlan();
  if (n_nb < 0 || (n_nb > 0 && !nb)) return tri_refuse(plan, kTriBatchInvalid, -1, "bad neighbour list (n_nb %lld)", n_nb);
  if (!s1.frame) return tri_refuse(plan, kTriBatchInvalid, -1, "frame1 is NULL");
  if (s1.device != device) return tri_refuse(plan, kTriBatchInvalid, -1, "frame1 lives on device %lld, the matcher on device %lld", s1.device, device);
  if (s1.n > 0 && !s1.has_mp) return tri_refuse(plan, kTriBatchInvalid, -1, "has_mp1 is NULL");
  int rc;
  if ((rc = tri_check_fv(s1, -1, plan))) return rc;
  for (int k = 0; k < n_nb; k++) {
    const TriSide& s2 = nb[k];
    if (!s2.frame) return tri_refuse(plan, kTriBatchInvalid, k, "frame2 is NULL");
    if (s2.device != device) return tri_refuse(plan, kTriBatchInvalid, k, "its frame lives on device %lld, the matcher on device %lld", s2.device, device);
    if (s2.nlevels < 1 || s2.nlevels > kTriMaxLevels) return tri_refuse(plan, kTriBatchInvalid, k, "nlevels2 = %lld outside 1..%lld", s2.nlevels, kTriMaxLevels);
    if (!s2.tables) return tri_refuse(plan, kTriBatchInvalid, k, "scale_factors2 or level_sigma2_2 is NULL");
    if (s2.n > 0 && !s2.has_mp) return tri_refuse(plan, kTriBatchInvalid, k, "has_mp2 is NULL");
    if (s2.n > 0 && s2.maxOctave >= s2.nlevels)
      return tri_refuse(plan, kTriBatchInvalid, k, "a keypoint octave lies outside [0, %lld)", s2.nlevels);
    if ((rc = tri_check_fv(s2, k, plan))) return rc;
    for (int b = 0; b < s2.n_fv; b++)
      if (s2.offsets[b + 1] - s2.offsets[b] > (uint32_t)kTriMaxGroup)
        return tri_refuse(plan, kTriBatchOverflow, k, "a vocabulary node holds %lld features (max %lld)", s2.offsets[b + 1] - s2.offsets[b], kTriMaxGroup);
  }
  plan.entries = (uint64_t)n_nb * (uint64_t)s1.n;
  if (plan.entries > kTriMaxEntries) return tri_refuse(plan, kTriBatchOverflow, -1, "%lld neighbours x %lld keypoints are more entries than one call writes", n_nb, s1.n);
  plan.nFeat1 = s1.n_fv ? s1.offsets[s1.n_fv] : 0;
  plan.flag2.assign((size_t)n_nb, 0);
  plan.feat2.assign((size_t)n_nb, 0);
  uint64_t flags = 0, feats = 0;
  for (int k = 0; k < n_nb; k++) {
    plan.flag2[k] = (uint32_t)flags;
    plan.feat2[k] = (uint32_t)feats;
    flags += (uint64_t)nb[k].n;
    feats += nb[k].n_fv ? nb[k].offsets[nb[k].n_fv] : 0;
    if (flags > kTriMaxEntries || feats > kTriMaxEntries) return tri_refuse(plan, kTriBatchOverflow, k, "the neighbours up to this one hold more keypoints than one call takes");
  }
  plan.nFlag2 = (size_t)flags;
  plan.nFeat2 = (size_t)feats;
  // the records, neighbour by neighbour, then node-major: side 1's rows of a node are read by all its neighbours' workgroups
  // at about the same time, so every one after the first finds them in L2
  std::vector<TriRecord> one;
  std::vector<int> node1, key;
  for (int k = 0; k < n_nb; k++) {
    tri_common_nodes(s1, nb[k], one, &node1);
    for (size_t i = 0; i < one.size(); i++) {
      TriRecord r = one[i];
      r.b2 += (int)plan.feat2[k]; r.e2 += (int)plan.feat2[k];
      r.base1 = (int)((uint64_t)k * (uint64_t)s1.n);
      r.nb = k;
      plan.records.push_back(r);
      key.push_back(node1[i]);
    }
  }
  std::vector<size_t> order(plan.records.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return key[a] < key[b]; });   // (stable: neighbours stay ascending)
  std::vector<TriRecord> sorted(plan.records.size());
  for (size_t i = 0; i < order.size(); i++) sorted[i] = plan.records[order[i]];
  plan.records.swap(sorted);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += tri_al(bytes); return at; };
  plan.oTable = take(tableBytes * (size_t)n_nb);
  plan.oRecords = take(sizeof(TriRecord) * plan.records.size());
  plan.oFlag1 = take((size_t)s1.n);
  plan.oFeat1 = take(4 * plan.nFeat1);
  plan.oFlag2 = take(plan.nFlag2);
  plan.oFeat2 = take(4 * plan.nFeat2);
  plan.bytes = o;
  return kTriBatchOk;
}

// ---- the host half: the reference's loop over the neighbours, from one raw row -------------------------------------------------
constexpr int kTriFinishStale = -7;   // ORBFE_ERR_STALE

// Step 1 of orbfe_triangulation_finish.  row[i] = -1 where has_mp1_now[i] is set.  kTriFinishStale (nothing written) if a flag
// that was set when the raw row was computed is clear now: the row lacks that keypoint.  kTriBatchInvalid: an entry outside
// [-1, n2).  *stale_at: the keypoint the refusal is about.
inline int tri_finish_mask(const int32_t* raw, int n1, const uint8_t* initial, const uint8_t* now, int n2, int32_t* row, int* at) {
  for (int i = 0; i < n1; i++) {
    if (initial[i] && !now[i]) { *at = i; return kTriFinishStale; }
    if (raw[i] < -1 || raw[i] >= n2) { *at = i; return kTriBatchInvalid; }
  }
  for (int i = 0; i < n1; i++) row[i] = now[i] ? -1 : raw[i];
  return kTriBatchOk;
}

}  // namespace orbfe
