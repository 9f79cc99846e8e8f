// orbfe_kfdb.hip -- the keyframe bag-of-words database, resident in HBM: what KeyFrameDatabase::DetectLoopCandidates and
// DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:74-334) and the covisible scores of LoopClosing::DetectLoop
// (src/LoopClosing.cc:125-140) need from the inverted file and from mpVoc->score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp).
// C ABI: include/orbfe.h (keyframe database section).
//
// Split of work.  The reference walks the query's words and, per word, the list of keyframes that hold it; what comes out is,
// per keyframe, the number of common words, the place of its first encounter and (for some) a score.  All three are functions
// of ONE keyframe's BowVector and the query's, so one wave takes one keyframe: its lanes look the keyframe's words up in the
// query (binary search, the query staged in LDS), ballots give the count and the first common word, and the score's sum is
// taken over the hits in ascending word order, one double add at a time -- the order of L1Scoring::score's merge walk
// (ScoringObject.cpp:34-59), which is part of the result's bits.  The host then sorts the sharing keyframes by (first common
// word, add order): that IS the first-encounter order of lKFsSharingWords (KeyFrameDatabase.cc:85-104, :207-222), because every
// inverted-file list keeps its keyframes in add order (:42-43 push_back, :56-62 erase keeps the rest in place).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../include/orbfe.h"
#include "bow_batch_plan.h"
#include "hip_buffers.h"

using orbfe::set_err;

namespace {

enum { kL1 = 0, kL2 = 1, kChi = 2, kKL = 3, kBhatta = 4, kDot = 5 };   // DBoW2::ScoringType, BowVector.h:45-53
constexpr int kThreads = 256, kWaves = kThreads / 64;
// Query words staged per block: 12 bytes each, 48 KB at the budget (three blocks per CU keep their copy).  A frame of 2 000
// keypoints has at most 2 000 words; a longer query takes the instantiation that reads it from global memory.
constexpr int kQueryLdsWords = 4096;

struct KfSlot { uint32_t offset, count, alive, add_seq; };          // device mirror of a slot
struct KfResult { uint32_t common, first_word; double score; };     // per item, in page-locked host memory
struct KfMove { uint32_t src, dst, count, pad; };                   // compaction: one keyframe's entries
static_assert(sizeof(KfSlot) == 16 && sizeof(KfResult) == 16, "one 16-byte access each");

__device__ inline double readlane_f64(double x, int l) {   // l wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}

// One wave per item: item i is slot i, or slot slotList[i] (orbfe_kfdb_score).  LDSQ: the query sits in LDS (values first, then
// words); otherwise it is read where the host's copy put it.
template <int SCORING, bool LDSQ>
__global__ __launch_bounds__(kThreads) void k_kfdb_query(const KfSlot* __restrict__ slots, const uint32_t* __restrict__ slotList,
                                                          int nItems, const uint32_t* __restrict__ word,
                                                          const double* __restrict__ value, const double* __restrict__ qv,
                                                          const uint32_t* __restrict__ qw, int nq, KfResult* __restrict__ out) {
  extern __shared__ double s_q[];
  const int tid = threadIdx.x, lane = tid & 63;
  if (LDSQ) {
    uint32_t* sw = reinterpret_cast<uint32_t*>(s_q + nq);
    for (int i = tid; i < nq; i += kThreads) { s_q[i] = qv[i]; sw[i] = qw[i]; }
    __syncthreads();
  }
  const int item = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(tid >> 6);
  if (item >= nItems) return;
  const KfSlot S = slots[slotList ? slotList[item] : (uint32_t)item];
  uint32_t common = 0, first = 0xffffffffu;
  double score = 0;
  const uint32_t count = S.alive ? S.count : 0u;
  for (uint32_t base = 0; base < count; base += 64) {
    const uint32_t i = base + lane;
    const bool in = i < count;
    const uint32_t w = in ? word[(size_t)S.offset + i] : 0u;
    const double wi = in ? value[(size_t)S.offset + i] : 0.0;
    // lower_bound of w among the query's words
    int lo = 0, hi = nq;
    uint32_t found = 0xffffffffu;
    if (LDSQ) {
      const uint32_t* sw = reinterpret_cast<const uint32_t*>(s_q + nq);
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (sw[mid] < w) lo = mid + 1; else hi = mid; }
      if (lo < nq) found = sw[lo];
    } else {
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (qw[mid] < w) lo = mid + 1; else hi = mid; }
      if (lo < nq) found = qw[lo];
    }
    const bool hit = in && found == w;
    double vi = 0.0;   // v1 is the query (KeyFrameDatabase.cc:133, :257: score(pKF->mBowVec, pKFi->mBowVec))
    if (hit) vi = LDSQ ? s_q[lo] : qv[lo];
    double term = 0.0;
    bool adds = hit;
    if (SCORING == kL1) term = fabs(vi - wi) - fabs(vi) - fabs(wi);          // ScoringObject.cpp:41
    else if (SCORING == kChi) { adds = hit && (vi + wi != 0.0); if (adds) term = vi * wi / (vi + wi); }   // :148
    else term = vi * wi;                                                     // :91 (L2), :290 (dot product)
    const unsigned long long hits = __ballot(hit);
    if (hits) {
      if (first == 0xffffffffu) first = (uint32_t)__builtin_amdgcn_readlane((int)w, __builtin_ctzll(hits));
      common += (uint32_t)__builtin_popcountll(hits);
      // the sum in ascending word order, one add at a time: lanes are ascending inside a stride, strides ascending
      unsigned long long m = SCORING == kChi ? __ballot(adds) : hits;
      while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        score += readlane_f64(term, l);
      }
    }
  }
  if (SCORING == kL1) score = -score / 2.0;       // ScoringObject.cpp:65
  else if (SCORING == kChi) score = 2. * score;   // :167   (L2's `1.0 - sqrt(1.0 - score)`, :114-117, is left to the host's sqrt)
  if (lane == 0) {
    KfResult r;
    r.common = common; r.first_word = first; r.score = score;
    out[item] = r;
  }
}

// Pool compaction: block b moves keyframe b's entries from the old pool to the new one.
__global__ __launch_bounds__(kThreads) void k_kfdb_compact(const KfMove* __restrict__ moves, const uint32_t* __restrict__ wordIn,
                                                            const double* __restrict__ valueIn, uint32_t* __restrict__ wordOut,
                                                            double* __restrict__ valueOut) {
  const KfMove M = moves[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < M.count; i += kThreads) {
    wordOut[(size_t)M.dst + i] = wordIn[(size_t)M.src + i];
    valueOut[(size_t)M.dst + i] = valueIn[(size_t)M.src + i];
  }
}

using QueryKernel = void (*)(const KfSlot*, const uint32_t*, int, const uint32_t*, const double*, const double*, const uint32_t*, int,
                             KfResult*);
QueryKernel query_kernel(int scoring, bool lds) {
  switch (scoring) {
    case kL1: return lds ? k_kfdb_query<kL1, true> : k_kfdb_query<kL1, false>;
    case kChi: return lds ? k_kfdb_query<kChi, true> : k_kfdb_query<kChi, false>;
    default: return lds ? k_kfdb_query<kDot, true> : k_kfdb_query<kDot, false>;   // L2 and the dot product: sum of vi * wi
  }
}

struct Slot {
  uint64_t key = 0, add_seq = 0;
  uint32_t offset = 0, count = 0;
  bool alive = false;
};

}  // namespace

struct orbfe_kfdb {
  std::mutex mu;   // like KeyFrameDatabase::mMutex: calls on one handle are serialised
  int device = 0, scoring = 0, capK = 0;
  uint32_t nWords = 0;
  size_t capE = 0, tail = 0, liveEntries = 0;
  int nLive = 0, hiSlot = 0;
  uint64_t addSeq = 0;
  bool slotsDirty = false;
  std::vector<Slot> slots;
  std::vector<int> freeSlots;
  std::unordered_map<uint64_t, int> byKey;
  uint32_t* d_word = nullptr;
  double* d_value = nullptr;
  KfSlot* d_slots = nullptr;
  uint8_t* d_query = nullptr;   // values, words, slot list of the call in flight
  size_t queryCap = 0;
  uint8_t* h_stage = nullptr;   // page-locked: source of the uploads
  size_t stageCap = 0;
  KfResult* h_out = nullptr;    // page-locked, coherent: the kernel writes the results here
  size_t outCap = 0;
  hipStream_t stream = nullptr;
  std::vector<KfSlot> mirror;

  ~orbfe_kfdb() {
    (void)hipSetDevice(device);
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    if (d_word) (void)hipFree(d_word);
    if (d_value) (void)hipFree(d_value);
    if (d_slots) (void)hipFree(d_slots);
    if (d_query) (void)hipFree(d_query);
    if (h_stage) (void)hipHostFree(h_stage);
    if (h_out) (void)hipHostFree(h_out);
  }
};

namespace {

int ensure_stage(orbfe_kfdb* db, size_t bytes) {
  if (bytes <= db->stageCap) return ORBFE_OK;
  if (db->h_stage) (void)hipHostFree(db->h_stage);
  db->h_stage = nullptr; db->stageCap = 0;
  HIP_TRY(hipHostMalloc((void**)&db->h_stage, bytes, hipHostMallocDefault));
  db->stageCap = bytes;
  return ORBFE_OK;
}
int ensure_query(orbfe_kfdb* db, size_t bytes) {
  if (bytes <= db->queryCap) return ORBFE_OK;
  if (db->d_query) (void)hipFree(db->d_query);
  db->d_query = nullptr; db->queryCap = 0;
  HIP_TRY(hipMalloc((void**)&db->d_query, bytes));
  db->queryCap = bytes;
  return ORBFE_OK;
}
int ensure_out(orbfe_kfdb* db, size_t n) {
  if (n <= db->outCap) return ORBFE_OK;
  if (db->h_out) (void)hipHostFree(db->h_out);
  db->h_out = nullptr; db->outCap = 0;
  HIP_TRY(hipHostMalloc((void**)&db->h_out, n * sizeof(KfResult), hipHostMallocCoherent));
  db->outCap = n;
  return ORBFE_OK;
}

// words strictly ascending (a std::map's order) and inside the vocabulary
bool ascending(const uint32_t* w, int n, uint32_t nWords) {
  for (int i = 0; i < n; i++)
    if (w[i] >= nWords || (i > 0 && w[i] <= w[i - 1])) return false;
  return true;
}

// Live keyframes to the front of a fresh pool, in pool order; add_seq, keys and slots stay as they are.
int compact(orbfe_kfdb* db) {
  std::vector<int> order;
  for (int s = 0; s < db->hiSlot; s++) if (db->slots[s].alive && db->slots[s].count) order.push_back(s);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return db->slots[a].offset < db->slots[b].offset; });
  std::vector<KfMove> moves(order.size());
  size_t at = 0;
  for (size_t i = 0; i < order.size(); i++) {
    const Slot& S = db->slots[order[i]];
    moves[i] = KfMove{S.offset, (uint32_t)at, S.count, 0u};
    at += S.count;
  }
  if (!moves.empty()) {
    uint32_t* nw = nullptr;
    double* nv = nullptr;
    KfMove* dm = nullptr;
    HIP_TRY(hipMalloc((void**)&nw, db->capE * sizeof(uint32_t)));
    std::unique_ptr<uint32_t, void (*)(uint32_t*)> gw(nw, [](uint32_t* p) { (void)hipFree(p); });
    HIP_TRY(hipMalloc((void**)&nv, db->capE * sizeof(double)));
    std::unique_ptr<double, void (*)(double*)> gv(nv, [](double* p) { (void)hipFree(p); });
    HIP_TRY(hipMalloc((void**)&dm, moves.size() * sizeof(KfMove)));
    std::unique_ptr<KfMove, void (*)(KfMove*)> gm(dm, [](KfMove* p) { (void)hipFree(p); });
    HIP_TRY(hipMemcpyAsync(dm, moves.data(), moves.size() * sizeof(KfMove), hipMemcpyHostToDevice, db->stream));
    hipLaunchKernelGGL(k_kfdb_compact, dim3((unsigned)moves.size()), dim3(kThreads), 0, db->stream, dm, db->d_word, db->d_value, nw, nv);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(db->stream));
    gw.release(); gv.release();
    (void)hipFree(db->d_word);
    (void)hipFree(db->d_value);
    db->d_word = nw;
    db->d_value = nv;
  }
  for (size_t i = 0; i < order.size(); i++) db->slots[order[i]].offset = moves[i].dst;
  for (int s = 0; s < db->hiSlot; s++) if (!db->slots[s].alive || !db->slots[s].count) db->slots[s].offset = 0;
  db->tail = at;
  db->slotsDirty = true;
  return ORBFE_OK;
}

// The kernel over nItems items (slot list: n entries behind the query in h_stage, or none = every slot below hiSlot); results in h_out.
int run_query(orbfe_kfdb* db, const uint32_t* qw, const double* qv, int nq, const uint32_t* slotList, int nItems) {
  HIP_TRY(hipSetDevice(db->device));
  int rc;
  const size_t offW = sizeof(double) * (size_t)nq, offL = (offW + sizeof(uint32_t) * (size_t)nq + 7) & ~(size_t)7;
  const size_t bytes = offL + sizeof(uint32_t) * (size_t)(slotList ? nItems : 0);
  if ((rc = ensure_stage(db, bytes + 8)) || (rc = ensure_query(db, bytes + 8)) || (rc = ensure_out(db, (size_t)nItems))) return rc;
  if (nq) { memcpy(db->h_stage, qv, sizeof(double) * (size_t)nq); memcpy(db->h_stage + offW, qw, sizeof(uint32_t) * (size_t)nq); }
  if (slotList) memcpy(db->h_stage + offL, slotList, sizeof(uint32_t) * (size_t)nItems);
  if (bytes) HIP_TRY(hipMemcpyAsync(db->d_query, db->h_stage, bytes, hipMemcpyHostToDevice, db->stream));
  if (db->slotsDirty && db->hiSlot > 0) {
    db->mirror.resize(db->hiSlot);
    for (int s = 0; s < db->hiSlot; s++) {
      const Slot& S = db->slots[s];
      db->mirror[s] = KfSlot{S.offset, S.count, S.alive ? 1u : 0u, (uint32_t)S.add_seq};
    }
    // (pageable source: the copy has left db->mirror when the call returns)
    HIP_TRY(hipMemcpyAsync(db->d_slots, db->mirror.data(), sizeof(KfSlot) * (size_t)db->hiSlot, hipMemcpyHostToDevice, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    db->slotsDirty = false;
  }
  const bool lds = nq <= kQueryLdsWords;
  const size_t ldsBytes = lds ? (size_t)nq * 12 : 0;
  hipLaunchKernelGGL(query_kernel(db->scoring, lds), dim3((unsigned)((nItems + kWaves - 1) / kWaves)), dim3(kThreads), ldsBytes,
                     db->stream, db->d_slots, slotList ? (const uint32_t*)(db->d_query + offL) : nullptr, nItems, db->d_word, db->d_value,
                     (const double*)db->d_query, (const uint32_t*)(db->d_query + offW), nq, db->h_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(db->stream));   // the results are in host memory: no copy command follows the kernel
  if (db->scoring == kL2)                      // ScoringObject.cpp:114-117
    for (int i = 0; i < nItems; i++) {
      double& score = db->h_out[i].score;
      if (score >= 1) score = 1.0;
      else score = 1.0 - sqrt(1.0 - score);
    }
  return ORBFE_OK;
}

}  // namespace

extern "C" {

int orbfe_kfdb_create(int device_id, int n_words, int scoring, int capacity_keyframes, int capacity_entries, orbfe_kfdb** out) {
  if (!out || n_words < 1 || capacity_keyframes < 1 || capacity_entries < 1) {
    set_err("bad keyframe database arguments");
    return ORBFE_ERR_INVALID;
  }
  *out = nullptr;
  if (scoring == kKL || scoring == kBhatta) {
    set_err("scoring %d (%s) is not supported: it needs log / sqrt per word with the host library's rounding", scoring,
            scoring == kKL ? "KL" : "BHATTACHARYYA");
    return ORBFE_ERR_INVALID;
  }
  if (scoring < 0 || scoring > kDot) { set_err("unknown scoring %d", scoring); return ORBFE_ERR_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) {
    set_err("no HIP device %d (the keyframe database has no CPU fallback)", device_id);
    return ORBFE_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device_id));
  std::unique_ptr<orbfe_kfdb> db(new orbfe_kfdb);
  db->device = device_id; db->scoring = scoring; db->capK = capacity_keyframes; db->nWords = (uint32_t)n_words;
  db->capE = (size_t)capacity_entries;
  db->slots.resize(capacity_keyframes);
  HIP_TRY(hipMalloc((void**)&db->d_word, db->capE * sizeof(uint32_t)));
  HIP_TRY(hipMalloc((void**)&db->d_value, db->capE * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&db->d_slots, (size_t)capacity_keyframes * sizeof(KfSlot)));
  HIP_TRY(hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking));
  int rc;
  if ((rc = ensure_out(db.get(), (size_t)capacity_keyframes))) return rc;
  *out = db.release();
  return ORBFE_OK;
}

void orbfe_kfdb_destroy(orbfe_kfdb* db) { delete db; }

int orbfe_kfdb_add(orbfe_kfdb* db, uint64_t key, const uint32_t* words, const double* values, int n) {
  if (!db || n < 0 || (n > 0 && (!words || !values))) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  if (!ascending(words, n, db->nWords)) { set_err("words must be ascending and below n_words"); return ORBFE_ERR_INVALID; }
  if (db->byKey.count(key)) { set_err("key %llu is already in the database", (unsigned long long)key); return ORBFE_ERR_INVALID; }
  if (db->nLive >= db->capK) { set_err("keyframe capacity %d exceeded", db->capK); return ORBFE_ERR_OVERFLOW; }
  if (db->liveEntries + (size_t)n > db->capE) {
    set_err("entry capacity %zu exceeded (%zu live + %d)", db->capE, db->liveEntries, n);
    return ORBFE_ERR_OVERFLOW;
  }
  HIP_TRY(hipSetDevice(db->device));
  int rc;
  if (db->tail + (size_t)n > db->capE && (rc = compact(db))) return rc;   // tombstones hold the room: squeeze them out
  if (n > 0) {
    const size_t offW = sizeof(double) * (size_t)n;
    if ((rc = ensure_stage(db, offW + sizeof(uint32_t) * (size_t)n))) return rc;
    memcpy(db->h_stage, values, offW);
    memcpy(db->h_stage + offW, words, sizeof(uint32_t) * (size_t)n);
    HIP_TRY(hipMemcpyAsync(db->d_value + db->tail, db->h_stage, offW, hipMemcpyHostToDevice, db->stream));
    HIP_TRY(hipMemcpyAsync(db->d_word + db->tail, db->h_stage + offW, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
  }
  int s;
  if (!db->freeSlots.empty()) { s = db->freeSlots.back(); db->freeSlots.pop_back(); }
  else s = db->hiSlot++;
  Slot& S = db->slots[s];
  S.key = key; S.add_seq = db->addSeq++; S.offset = (uint32_t)db->tail; S.count = (uint32_t)n; S.alive = true;
  db->byKey[key] = s;
  db->tail += (size_t)n;
  db->liveEntries += (size_t)n;
  db->nLive++;
  db->slotsDirty = true;
  return ORBFE_OK;
}

// orbfe_kfdb_add for n keyframes (the KeyFrameDatabase::add loop of a map load): every check of every keyframe first
// (kfdb_batch_plan, bow_batch_plan.h), then at most one compaction, ONE staging image, one copy per pool array and one wait.
int orbfe_kfdb_add_batch(orbfe_kfdb* db, int n, const uint64_t* keys, const uint32_t* const* words, const double* const* values,
                         const int* n_words) {
  if (!db || n < 0 || (n > 0 && (!keys || !words || !values || !n_words))) { set_err("bad argument"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  orbfe::KfdbBatchPlan plan;
  int rc = orbfe::kfdb_batch_plan(n, keys, words, values, n_words, db->nWords, db->nLive, db->capK, db->liveEntries, db->capE, db->tail,
                                  [&](uint64_t k) { return db->byKey.count(k) != 0; }, plan);
  if (rc) {
    const int j = plan.failed;
    switch (plan.why) {
      case 1: set_err("entry %d: words must be ascending and below n_words", j); break;
      case 2: set_err("entry %d: key %llu is already in the database or named twice", j, (unsigned long long)keys[j]); break;
      case 3: set_err("entry %d: keyframe capacity %d exceeded", j, db->capK); break;
      case 4: set_err("entry %d: entry capacity %zu exceeded", j, db->capE); break;
      default: set_err("bad argument for entry %d", j);
    }
    return rc;
  }
  if (n == 0) return ORBFE_OK;
  HIP_TRY(hipSetDevice(db->device));
  if (plan.compactAt >= 0 && (rc = compact(db))) return rc;   // tombstones hold the room: squeeze them out
  if (plan.total > 0) {
    const size_t offW = sizeof(double) * plan.total;
    if ((rc = ensure_stage(db, offW + sizeof(uint32_t) * plan.total))) return rc;
    size_t at = 0;
    for (int j = 0; j < n; j++) {
      const size_t c = (size_t)n_words[j];
      if (!c) continue;
      memcpy(db->h_stage + sizeof(double) * at, values[j], sizeof(double) * c);
      memcpy(db->h_stage + offW + sizeof(uint32_t) * at, words[j], sizeof(uint32_t) * c);
      at += c;
    }
    HIP_TRY(hipMemcpyAsync(db->d_value + db->tail, db->h_stage, offW, hipMemcpyHostToDevice, db->stream));
    HIP_TRY(hipMemcpyAsync(db->d_word + db->tail, db->h_stage + offW, sizeof(uint32_t) * plan.total, hipMemcpyHostToDevice, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
  }
  for (int j = 0; j < n; j++) {   // the slots, in the order n single adds take them
    int s;
    if (!db->freeSlots.empty()) { s = db->freeSlots.back(); db->freeSlots.pop_back(); }
    else s = db->hiSlot++;
    Slot& S = db->slots[s];
    S.key = keys[j]; S.add_seq = db->addSeq++; S.offset = (uint32_t)plan.offset[j]; S.count = (uint32_t)n_words[j]; S.alive = true;
    db->byKey[keys[j]] = s;
  }
  db->tail += plan.total;
  db->liveEntries += plan.total;
  db->nLive += n;
  db->slotsDirty = true;
  return ORBFE_OK;
}

int orbfe_kfdb_erase(orbfe_kfdb* db, uint64_t key) {
  if (!db) { set_err("database is NULL"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  auto it = db->byKey.find(key);
  if (it == db->byKey.end()) return ORBFE_OK;   // KeyFrameDatabase.cc:46-65 finds nothing to erase
  Slot& S = db->slots[it->second];
  S.alive = false;   // a tombstone: the entries stay where they are until a compaction
  db->liveEntries -= S.count;
  db->nLive--;
  db->freeSlots.push_back(it->second);
  db->byKey.erase(it);
  db->slotsDirty = true;
  return ORBFE_OK;
}

int orbfe_kfdb_clear(orbfe_kfdb* db) {
  if (!db) { set_err("database is NULL"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  for (int s = 0; s < db->hiSlot; s++) db->slots[s] = Slot();
  db->freeSlots.clear();
  db->byKey.clear();
  db->tail = db->liveEntries = 0;
  db->nLive = db->hiSlot = 0;
  db->slotsDirty = true;
  return ORBFE_OK;
}

int orbfe_kfdb_size(orbfe_kfdb* db, int* n_keyframes, int* n_entries) {
  if (!db) { set_err("database is NULL"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  if (n_keyframes) *n_keyframes = db->nLive;
  if (n_entries) *n_entries = (int)db->liveEntries;
  return ORBFE_OK;
}

int orbfe_kfdb_query(orbfe_kfdb* db, const uint32_t* q_words, const double* q_values, int nq, uint64_t* keys, int32_t* common,
                     double* scores, int cap, int* n_out) {
  if (!db || nq < 0 || (nq > 0 && (!q_words || !q_values)) || cap < 0 || !n_out || (cap > 0 && (!keys || !common || !scores))) {
    set_err("bad argument");
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lock(db->mu);
  *n_out = 0;
  if (!ascending(q_words, nq, db->nWords)) { set_err("query words must be ascending and below n_words"); return ORBFE_ERR_INVALID; }
  if (nq == 0 || db->nLive == 0) return ORBFE_OK;
  int rc;
  if ((rc = run_query(db, q_words, q_values, nq, nullptr, db->hiSlot))) return rc;
  struct Rec { uint32_t first; uint64_t seq; int slot; };
  std::vector<Rec> recs;
  for (int s = 0; s < db->hiSlot; s++)
    if (db->slots[s].alive && db->h_out[s].common) recs.push_back(Rec{db->h_out[s].first_word, db->slots[s].add_seq, s});
  std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.first != b.first ? a.first < b.first : a.seq < b.seq; });
  *n_out = (int)recs.size();
  for (int i = 0; i < (int)recs.size() && i < cap; i++) {
    keys[i] = db->slots[recs[i].slot].key;
    common[i] = (int32_t)db->h_out[recs[i].slot].common;
    scores[i] = db->h_out[recs[i].slot].score;
  }
  if ((int)recs.size() > cap) { set_err("%d keyframes share words with the query, capacity %d", (int)recs.size(), cap); return ORBFE_ERR_OVERFLOW; }
  return ORBFE_OK;
}

int orbfe_kfdb_score(orbfe_kfdb* db, const uint32_t* q_words, const double* q_values, int nq, const uint64_t* keys, int n,
                     double* scores) {
  if (!db || nq < 0 || (nq > 0 && (!q_words || !q_values)) || n < 0 || (n > 0 && (!keys || !scores))) {
    set_err("bad argument");
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lock(db->mu);
  if (!ascending(q_words, nq, db->nWords)) { set_err("query words must be ascending and below n_words"); return ORBFE_ERR_INVALID; }
  std::vector<uint32_t> list(n);
  for (int i = 0; i < n; i++) {
    auto it = db->byKey.find(keys[i]);
    if (it == db->byKey.end()) { set_err("key %llu (entry %d) is not in the database", (unsigned long long)keys[i], i); return ORBFE_ERR_INVALID; }
    list[i] = (uint32_t)it->second;
  }
  if (n == 0) return ORBFE_OK;
  int rc;
  if ((rc = run_query(db, q_words, q_values, nq, list.data(), n))) return rc;
  for (int i = 0; i < n; i++) scores[i] = db->h_out[i].score;
  return ORBFE_OK;
}

}  // extern "C"
