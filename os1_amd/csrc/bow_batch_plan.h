// bow_batch_plan.h -- the host-side bookkeeping of the two bulk calls of a map load, free of HIP so that a plain host
// program can exercise it (tests/cpp/bow_batch_plan_test.cpp, also under the address and undefined-behaviour sanitizers):
//   * orbfe_bow_transform_batch (orbfe_bow.hip): argument and capacity check, the table of wave offsets that
//     k_bow_descend_batch searches, where each set's rows are read from;
//   * orbfe_kfdb_add_batch (orbfe_kfdb.hip): the check of all n keyframes before anything is sent, and where each keyframe's
//     entries end up so that the pool equals the pool after n single adds.
#pragma once
#include <cstddef>
#include <cstdint>
#include <unordered_set>
#include <vector>

namespace orbfe {

constexpr int kBowBatchOk = 0, kBowBatchInvalid = -1, kBowBatchOverflow = -5;   // ORBFE_OK, ORBFE_ERR_INVALID, ORBFE_ERR_OVERFLOW
constexpr int kBowFeaturesPerWave = 4;       // 16 lanes per descriptor (k_bow_descend*)
constexpr uint32_t kBowBatchMaxFeatures = 1u << 30;   // of one call, padding included: wave and output indices stay below 2^31

// where a set's descriptor rows lie
enum BowRowsWhere { kBowRowsHost = 0, kBowRowsInPlace = 1 };   // copied into the call's upload arena / read where they are

struct BowBatchPlan {
  std::vector<uint32_t> waveStart;   // [n_sets + 1]: set s owns the waves [waveStart[s], waveStart[s + 1]) of the grid
  std::vector<uint32_t> out0;        // [n_sets + 1]: set s owns the outputs [out0[s], out0[s + 1]) -- dense, no padding
  std::vector<uint32_t> stageRow;    // [n_sets]: first row of the set in the upload arena (sets with kBowRowsHost), else unused
  uint32_t stagedRows = 0;           // rows the arena holds
  int failed = -1;                   // the set a non-zero return value names
};

// Sizes and capacities of every set, before anything is computed: a negative size is invalid; capacity[s] < n[s] is an overflow
// (the single call's documented capacity: n entries per output array, n + 1 for fv_offsets).  Then the tables.  Returns
// kBowBatchOk / kBowBatchInvalid / kBowBatchOverflow; on an error plan.failed is the first offending set.
inline int bow_batch_plan(int n_sets, const int* n, const int* capacity, const int* where, BowBatchPlan& plan) {
  plan = BowBatchPlan();
  if (n_sets < 0 || (n_sets > 0 && (!n || !capacity || !where))) return kBowBatchInvalid;
  for (int s = 0; s < n_sets; s++)
    if (n[s] < 0) { plan.failed = s; return kBowBatchInvalid; }
  for (int s = 0; s < n_sets; s++)
    if (capacity[s] < n[s]) { plan.failed = s; return kBowBatchOverflow; }
  plan.waveStart.assign((size_t)n_sets + 1, 0);
  plan.out0.assign((size_t)n_sets + 1, 0);
  plan.stageRow.assign((size_t)n_sets, 0);
  uint64_t waves = 0, outs = 0, staged = 0;
  for (int s = 0; s < n_sets; s++) {
    plan.waveStart[s] = (uint32_t)waves;
    plan.out0[s] = (uint32_t)outs;
    plan.stageRow[s] = (uint32_t)staged;
    waves += ((uint64_t)n[s] + kBowFeaturesPerWave - 1) / kBowFeaturesPerWave;
    outs += (uint64_t)n[s];
    if (where[s] == kBowRowsHost) staged += (uint64_t)n[s];
    if (waves * kBowFeaturesPerWave > kBowBatchMaxFeatures) { plan.failed = s; return kBowBatchOverflow; }
  }
  plan.waveStart[n_sets] = (uint32_t)waves;
  plan.out0[n_sets] = (uint32_t)outs;
  plan.stagedRows = (uint32_t)staged;
  return kBowBatchOk;
}

// The set that owns `wave`: what k_bow_descend_batch's search returns (restated here for the host test).
inline int bow_batch_set_of_wave(const std::vector<uint32_t>& waveStart, uint32_t wave) {
  int lo = 0, hi = (int)waveStart.size() - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (waveStart[mid] <= wave) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- keyframe database -------------------------------------------------------------------------------------------------
struct KfdbBatchPlan {
  int failed = -1;          // the entry a non-zero return value names
  int why = 0;              // 1 words not ascending / out of range, 2 duplicate key, 3 keyframe capacity, 4 entry capacity, 5 bad pointer
  int compactAt = -1;       // the single add (entry index) that would have compacted the pool first; -1: none does
  size_t total = 0;         // entries of the whole batch
  std::vector<size_t> offset;   // [n]: pool offset of entry j's words AFTER the call (see below)
};

// What n single orbfe_kfdb_add calls in index order would decide, without touching anything.  The state of the database comes in
// as numbers (live keyframes / capacity, live entries / capacity, the pool's tail) and a predicate for "key is in the database".
// Checks per entry in the single call's order: words ascending and below n_words, key not present (nor earlier in the batch),
// keyframe capacity, entry capacity.  A single add compacts the pool when its entries do not fit behind the tail; that can
// happen once in a batch at most (afterwards the tail equals the live entries, and those fit).  The pool after the n adds is the
// pool after ONE compaction up front followed by the n keyframes appended in order: the compaction keeps pool order, and the
// batch's earlier keyframes sat behind everything older.  offset[j] is that place; an EMPTY keyframe added before the compaction
// has offset 0 afterwards, as the compaction leaves it.
template <class HasKey>
inline int kfdb_batch_plan(int n, const uint64_t* keys, const uint32_t* const* words, const double* const* values, const int* counts,
                           uint32_t n_words, int nLive, int capK, size_t liveEntries, size_t capE, size_t tail, HasKey has,
                           KfdbBatchPlan& plan) {
  plan = KfdbBatchPlan();
  if (n < 0 || (n > 0 && (!keys || !words || !values || !counts))) { plan.why = 5; return kBowBatchInvalid; }
  std::unordered_set<uint64_t> seen;
  size_t live = liveEntries, simTail = tail;
  plan.offset.assign((size_t)n, 0);
  for (int j = 0; j < n; j++) {
    plan.failed = j;
    const int c = counts[j];
    if (c < 0 || (c > 0 && (!words[j] || !values[j]))) { plan.why = 5; return kBowBatchInvalid; }
    for (int i = 0; i < c; i++)
      if (words[j][i] >= n_words || (i > 0 && words[j][i] <= words[j][i - 1])) { plan.why = 1; return kBowBatchInvalid; }
    if (has(keys[j]) || !seen.insert(keys[j]).second) { plan.why = 2; return kBowBatchInvalid; }
    if (nLive + j >= capK) { plan.why = 3; return kBowBatchOverflow; }
    if (live + (size_t)c > capE) { plan.why = 4; return kBowBatchOverflow; }
    if (simTail + (size_t)c > capE) {
      if (plan.compactAt < 0) plan.compactAt = j;
      simTail = live;
    }
    simTail += (size_t)c;
    live += (size_t)c;
  }
  plan.failed = -1;
  plan.total = live - liveEntries;
  size_t at = plan.compactAt >= 0 ? liveEntries : tail;
  for (int j = 0; j < n; j++) {
    plan.offset[j] = (plan.compactAt >= 0 && j < plan.compactAt && counts[j] == 0) ? 0 : at;
    at += (size_t)counts[j];
  }
  return kBowBatchOk;
}

}  // namespace orbfe
