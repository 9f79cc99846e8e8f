// orb_shim.hpp -- header-only C++ host side above the C ABI (include/orbfe.h).
//
// Generic (duck-typed) so it compiles with or without OpenCV: the reference's own types
// (cv::KeyPoint, cv::Mat, ORB_SLAM2::Frame, ORB_SLAM2::MapPoint) are template parameters and are
// only touched through the member names the reference uses.  include/orbfe/ORBextractor.h binds the
// extractor part to the exact ORB_SLAM2::ORBextractor signature when OpenCV headers are present;
// INTEGRATION.md shows the three-line bodies that replace the hot ORBmatcher functions.
//
// Error behaviour mirrors the reference: no exceptions for data conditions (empty image => outputs
// untouched, matchers return the match count); a failing GPU call throws std::runtime_error with
// orbfe_last_error() because the reference has no channel to report it and continuing would
// silently corrupt tracking.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../orbfe.h"

namespace orbfe {

inline void check(int rc) {
  if (rc != ORBFE_OK) throw std::runtime_error(std::string("orbfe: ") + orbfe_last_error());
}

namespace detail {
// ORBFE_DEVICE (default 0): the GPU the cv-typed facades use -- extractor AND matcher (include/orbfe/ORBextractor.h,
// ORBmatcher.h), so that an integrated build on GPU != 0 extracts and searches on the same device.
inline int defaultDevice() {
  static const int d = [] { const char* e = std::getenv("ORBFE_DEVICE"); return e ? std::atoi(e) : 0; }();
  return d;
}

// 128-bit content fingerprint (two independently seeded multiply-xorshift lanes over 8-byte words, four interleaved
// chains each for throughput: ~10 bytes per cycle, a 2 000-keypoint frame's 120 KB in 3-4 us).  Used as IDENTITY of a
// frame's searchable content -- not cryptographic, but 2^-128-ish against accidental equality of distinct frames.
struct Hash128 {
  uint64_t a = 0x243F6A8885A308D3ull, b = 0x13198A2E03707344ull;
  bool operator==(const Hash128& o) const { return a == o.a && b == o.b; }
  bool operator!=(const Hash128& o) const { return !(*this == o); }
};
inline uint64_t mix64(uint64_t h, uint64_t v, uint64_t k) {
  h = (h ^ v) * k;
  return h ^ (h >> 29);
}
inline void hashBytes(Hash128& H, const void* p, size_t bytes) {
  const uint64_t K1 = 0x9E3779B97F4A7C15ull, K2 = 0xC2B2AE3D27D4EB4Full;
  const unsigned char* c = static_cast<const unsigned char*>(p);
  uint64_t a[4] = {H.a, H.a ^ K2, H.a + K1, ~H.a}, b[4] = {H.b, H.b ^ K1, H.b + K2, ~H.b};
  size_t i = 0;
  for (; i + 32 <= bytes; i += 32) {
    uint64_t w[4];
    std::memcpy(w, c + i, 32);
    for (int l = 0; l < 4; l++) { a[l] = mix64(a[l], w[l], K1); b[l] = mix64(b[l], w[l] + (uint64_t)l, K2); }
  }
  uint64_t tail[4] = {0, 0, 0, 0};
  if (i < bytes) std::memcpy(tail, c + i, bytes - i);
  for (int l = 0; l < 4; l++) { a[l] = mix64(a[l], tail[l] ^ bytes, K1); b[l] = mix64(b[l], tail[l] + bytes, K2); }
  H.a = mix64(mix64(mix64(a[0], a[1], K2), a[2], K2), a[3], K2);
  H.b = mix64(mix64(mix64(b[0], b[1], K1), b[2], K1), b[3], K1);
}
// the descriptor rows of a CV_8U n x 32 matrix (any step)
template <class MatT>
inline void hashDescriptorRows(Hash128& H, const MatT& m, int n) {
  if (n <= 0) return;
  if ((size_t)m.step == 32) { hashBytes(H, m.data, (size_t)n * 32); return; }
  for (int i = 0; i < n; i++) hashBytes(H, m.data + (size_t)i * m.step, 32);
}
}  // namespace detail

// ORBextractor (reference include/ORBextractor.h:155-373) minus the cv:: types.
//
// Besides extracting, an Extractor remembers WHAT it extracted last (count + fingerprint of the keypoints and descriptor
// rows it returned) while those results still sit in its device arena: the first search of the Frame built from them
// (Frame.cc:100-111: ExtractORB, UndistortKeyPoints, AssignFeaturesToGrid -- no other use of the extractor in between)
// then takes keypoints and descriptors where the kernels left them (MatcherContext::resident ->
// orbfe_frame_create_from_extract) instead of uploading mvKeysUn / mDescriptors again.
class Extractor {
 public:
  Extractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device = 0) : device_(device) {
    check(orbfe_extractor_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device, &h_));
    const int n = orbfe_extractor_levels(h_);
    sf_.resize(n); isf_.resize(n); s2_.resize(n); is2_.resize(n);
    check(orbfe_extractor_scale_tables(h_, sf_.data(), isf_.data(), s2_.data(), is2_.data()));
    cap_ = orbfe_extractor_max_keypoints(h_);
    std::lock_guard<std::mutex> g(registryMutex());
    registry().push_back(this);
  }
  ~Extractor() {
    {
      std::lock_guard<std::mutex> g(registryMutex());
      auto& r = registry();
      r.erase(std::remove(r.begin(), r.end(), this), r.end());
    }
    std::lock_guard<std::mutex> g(mu_);
    orbfe_extractor_destroy(h_);
  }
  Extractor(const Extractor&) = delete;
  Extractor& operator=(const Extractor&) = delete;

  // Which cv::GaussianBlur the descriptors are sampled from (ORBextractor.cc:949-950): ORBFE_GAUSS_ED = OpenCV >= 4.1.1 (default),
  // ORBFE_GAUSS_ROUNDED = OpenCV 4.0.0 - 4.1.0.  The cv-typed facade calls this with the variant of the OpenCV it is compiled against.
  void SetBlurVariant(int variant) {
    std::lock_guard<std::mutex> g(mu_);
    check(orbfe_extractor_set_blur_variant(h_, variant));
  }

  // The camera of the Frames built from this extractor's output (Frame.cc:284-319): with a distorting pinhole model the
  // undistortion runs on the GPU behind the descriptor kernel, extractUndistorted() hands mvKeysUn out with mvKeys, and the
  // resident frame of such a Frame takes its coordinates from the arena (MatcherContext::resident sends none).  camera_mode 1
  // (equidistant) throws: orbfe_extractor_set_camera refuses it; SetEquidistantCamera is the call for such a camera.
  void SetCamera(int camera_mode, float fx, float fy, float cx, float cy, const float* dist, int ndist) {
    std::lock_guard<std::mutex> g(mu_);
    check(orbfe_extractor_set_camera(h_, camera_mode, fx, fy, cx, cy, dist, ndist));
    camActive_ = ndist > 0 && dist[0] != 0.0f;
    lastValid_ = false;
  }

  // The same for os1's equidistant fisheye model (camaraModo == 1, Frame.cc:355-384): orbfe_extractor_set_camera_equidistant.
  // extractUndistorted() then returns what orbfe::UndistortKeyPoints(.., camaraModo 1, ..) computes on the host, bit for bit (the
  // kernel certifies the rounding of every point it can, the library settles the rest with the host's tan before the call returns),
  // and the resident frame takes the coordinates from the arena.  ComputeImageBounds stays the host function.
  void SetEquidistantCamera(float fx, float fy, float cx, float cy) {
    std::lock_guard<std::mutex> g(mu_);
    check(orbfe_extractor_set_camera_equidistant(h_, fx, fy, cx, cy));
    camActive_ = true;
    lastValid_ = false;
  }

  // operator() core: KeyPointT must have cv::KeyPoint's 28-byte layout.
  template <class KeyPointT>
  void extract(const uint8_t* gray, int rows, int cols, size_t step, std::vector<KeyPointT>& keypoints,
               std::vector<uint8_t>& descriptors) {
    extractUndistorted<KeyPointT>(gray, rows, cols, step, keypoints, nullptr, descriptors);
  }

  // extract() plus Frame::UndistortKeyPoints: keypointsUn (may be nullptr) = the records with pt replaced by the undistorted
  // point (Frame.cc:310-316) -- equal to keypoints without a distorting camera (:288-292).
  template <class KeyPointT>
  void extractUndistorted(const uint8_t* gray, int rows, int cols, size_t step, std::vector<KeyPointT>& keypoints,
                          std::vector<KeyPointT>* keypointsUn, std::vector<uint8_t>& descriptors) {
    static_assert(sizeof(KeyPointT) == sizeof(OrbfeKeyPoint), "KeyPointT must match cv::KeyPoint's layout");
    if (!gray || rows == 0 || cols == 0) return;  // reference: silent return, outputs untouched
    std::lock_guard<std::mutex> g(mu_);
    lastValid_ = false;
    cap_ = std::max(cap_, orbfe_extractor_max_keypoints_for_size(h_, rows, cols));   // strips wider than 4.5 : 1
    kp_.resize(cap_);
    desc_.resize((size_t)cap_ * 32);
    int n = 0;
    if (camActive_) {
      xyUn_.resize((size_t)cap_ * 2);
      check(orbfe_extract_undistorted(h_, gray, rows, cols, step, kp_.data(), desc_.data(), cap_, &n, xyUn_.data()));
    } else {
      check(orbfe_extract(h_, gray, rows, cols, step, kp_.data(), desc_.data(), cap_, &n));
    }
    keypoints.clear();
    keypoints.resize(n);
    if (n) std::memcpy(static_cast<void*>(keypoints.data()), kp_.data(), (size_t)n * sizeof(OrbfeKeyPoint));
    if (keypointsUn) {
      *keypointsUn = keypoints;
      if (camActive_)
        for (int i = 0; i < n; i++) std::memcpy(static_cast<void*>(&(*keypointsUn)[i]), &xyUn_[2 * (size_t)i], 8);   // pt = the first two floats
    }
    descriptors.assign(desc_.begin(), desc_.begin() + (size_t)n * 32);
    if (trackLast_ && n > 0) {
      lastN_ = n;
      lastKeys_ = detail::Hash128();
      lastDesc_ = detail::Hash128();
      detail::hashBytes(lastKeys_, kp_.data(), (size_t)n * sizeof(OrbfeKeyPoint));
      detail::hashBytes(lastDesc_, desc_.data(), (size_t)n * 32);
      if (camActive_) {
        lastUn_ = detail::Hash128();
        detail::hashBytes(lastUn_, xyUn_.data(), (size_t)n * 8);
      }
      lastValid_ = true;
    }
  }

  int GetLevels() const { return (int)sf_.size(); }
  float GetScaleFactor() const { return orbfe_extractor_scale_factor(h_); }
  std::vector<float> GetScaleFactors() const { return sf_; }
  std::vector<float> GetInverseScaleFactors() const { return isf_; }
  std::vector<float> GetScaleSigmaSquares() const { return s2_; }
  std::vector<float> GetInverseScaleSigmaSquares() const { return is2_; }
  orbfe_extractor* handle() const { return h_; }
  int capacity() const { return cap_; }
  int device() const { return device_; }
  // false: do not fingerprint the outputs (a caller that never searches Frames through a MatcherContext saves the 3-4 us)
  void setTrackLastOutput(bool on) { std::lock_guard<std::mutex> g(mu_); trackLast_ = on; lastValid_ = false; }

  // A resident frame straight from the arena of whichever live Extractor on `device` produced exactly these outputs last
  // (n keypoints with fingerprint `keys` of the cv::KeyPoint records as returned, `desc` of the rows); xy_un = the
  // undistorted coordinates [2n] when they differ from the extracted ones, else nullptr.  nullptr if there is none.
  // *coord_bytes (optional) receives the bytes of coordinates that had to be sent: 0 when the extractor has no distorting camera
  // and xy_un is nullptr, and 0 when xy_un are the very coordinates its undistortion kernel left in the arena.
  static orbfe_frame* residentFromLastExtract(int device, int n, const detail::Hash128& keys, const detail::Hash128& desc,
                                              const float bounds[4], const float* xy_un, size_t* coord_bytes = nullptr) {
    std::lock_guard<std::mutex> g(registryMutex());
    for (Extractor* e : registry()) {
      if (e->device_ != device) continue;
      std::lock_guard<std::mutex> ge(e->mu_);
      if (!e->lastValid_ || e->lastN_ != n || e->lastKeys_ != keys || e->lastDesc_ != desc) continue;
      orbfe_frame* f = nullptr;
      const float* send = xy_un;
      std::vector<float> raw;
      if (e->camActive_) {
        if (xy_un) {
          detail::Hash128 hu;
          detail::hashBytes(hu, xy_un, (size_t)n * 8);
          if (hu == e->lastUn_) send = nullptr;   // the arena holds exactly these
        } else {   // the Frame kept the extracted coordinates although the arena holds undistorted ones: send the extracted ones
          raw.resize((size_t)n * 2);
          for (int i = 0; i < n; i++) std::memcpy(&raw[2 * (size_t)i], &e->kp_[(size_t)i], 8);
          send = raw.data();
        }
      }
      if (orbfe_frame_create_from_extract(e->h_, 0, bounds, send, &f) == ORBFE_OK && f && orbfe_frame_size(f) == n) {
        if (coord_bytes) *coord_bytes = send ? (size_t)n * 8 : 0;
        return f;
      }
      if (f) orbfe_frame_destroy(f);
    }
    return nullptr;
  }

 private:
  static std::mutex& registryMutex() { static std::mutex m; return m; }
  static std::vector<Extractor*>& registry() { static std::vector<Extractor*> r; return r; }
  orbfe_extractor* h_ = nullptr;
  int cap_ = 0, device_ = 0;
  std::vector<float> sf_, isf_, s2_, is2_;
  std::vector<OrbfeKeyPoint> kp_;
  std::vector<uint8_t> desc_;
  std::mutex mu_;                       // extract() vs. a search thread taking the arena's content
  bool trackLast_ = true, lastValid_ = false, camActive_ = false;
  int lastN_ = 0;
  detail::Hash128 lastKeys_, lastDesc_, lastUn_;
  std::vector<float> xyUn_;
};

// One GPU matcher context per thread that runs searches (Tracking constructs ORBmatcher objects on
// the stack per use, Tracking.cc:383,596,818; the context is the long-lived part).
//
// The context also keeps the DEVICE-RESIDENT copies of the frames it has searched (orbfe_frame): the reference builds a
// frame's grid once (Frame.cc:111, 114-129) and reuses it in every search of that frame -- 2-3 per tracked frame
// (Tracking.cc:608, 614, 824), dozens per keyframe (Fuse, SearchBySim3, relocalisation).
//
// IDENTITY OF A CACHED FRAME = ITS CONTENT.  (kind, mnId, N) is NOT an identity in the reference: Tracking::Reset() sets
// Frame::nNextId and KeyFrame::nNextId back to 0 (Tracking.cc:1159-1160) -- routine after a failed monocular
// initialisation -- and Osmap's map load re-creates KeyFrames with the ids stored in the file (Osmap.cpp:586); N sits in
// 2000-2010 at nFeatures 2000, so a recycled id with an equal N is likely.  An entry is therefore keyed by the keypoint
// count, the image bounds (they position the grid) and a 128-bit fingerprint of ALL of mvKeysUn and of ALL descriptor rows,
// recomputed at every lookup (3-4 us against >= 45 us for the search it precedes).  A Frame, its copies (Frame.cc:39-62)
// and the KeyFrame made from it (KeyFrame.cc:37-60) share content and therefore one resident copy; two different frames
// never do, whatever their ids.  orbfe_resident_invalidate() (Tracking::Reset, map load) additionally empties every
// context's cache at its next lookup -- that frees memory; correctness does not depend on it.
// First use uploads the features once (or takes them from the extractor's arena, Extractor::residentFromLastExtract);
// later searches upload only their queries.  Least-recently-used entries are dropped beyond `capacity` (default 48, at
// least the 2 most recent are always kept: a search uses up to two frames; 0 disables the cache and every search takes the
// host-array call form).
class MatcherContext {
 public:
  explicit MatcherContext(int device = 0, size_t frame_cache_capacity = 48) : device_(device), cap_(frame_cache_capacity) {
    check(orbfe_matcher_create(device, &m_));
    epoch_ = orbfe_resident_epoch();
  }
  ~MatcherContext() {
    invalidate();
    if (table_.pending) orbfe_matcher_synchronize(m_);
    if (table_.rows) orbfe_device_free(device_, table_.rows);
    if (table_.mirror) orbfe_host_free(table_.mirror);
    if (lmap_.map) orbfe_local_map_destroy(lmap_.map);
    orbfe_matcher_destroy(m_);
    for (auto& s : scratch_)
      if (s.p) orbfe_host_free(s.p);
  }
  // Page-locked scratch array `slot` of at least n elements, zero-filled on request: what the per-frame searches marshal their
  // MapPoint snapshots into.  The search kernels read page-locked arrays in place (no copy inside the library), and the
  // arrays are reused from call to call (no allocation per search).  Valid until the next request for the same slot.
  template <class T>
  T* scratch(int slot, size_t n, bool zero) {
    Scratch& s = scratch_[slot];
    const size_t bytes = (n ? n : 1) * sizeof(T);
    if (bytes > s.bytes) {
      if (s.p) orbfe_host_free(s.p);
      s.p = nullptr; s.bytes = 0;
      check(orbfe_host_alloc(bytes + bytes / 2, &s.p));
      s.bytes = bytes + bytes / 2;
    }
    if (zero) std::memset(s.p, 0, bytes);
    return static_cast<T*>(s.p);
  }
  MatcherContext(const MatcherContext&) = delete;
  MatcherContext& operator=(const MatcherContext&) = delete;
  orbfe_matcher* get() const { return m_; }
  int device() const { return device_; }
  void setFrameCacheCapacity(size_t c) { cap_ = c; trim(); }
  size_t frameCacheCapacity() const { return cap_; }           // a call that holds k frames at once needs k of them (TriangulationSearch.h)
  size_t residentFrames() const { return cache_.size(); }
  size_t residentUploads() const { return uploads_; }          // frames whose features crossed PCIe (orbfe_frame_create)
  size_t residentFromExtract() const { return fromExtract_; }  // frames taken from an extractor's arena (no upload)
  size_t residentHits() const { return hits_; }
  size_t residentCoordBytes() const { return coordBytes_; }    // bytes of undistorted coordinates sent for frames taken from an arena
  // drop every cached frame (this context).  Tracking::Reset() / a map load call orbfe_resident_invalidate() instead,
  // which reaches the contexts of all threads.
  void invalidate() {
    for (auto& e : cache_) orbfe_frame_destroy(e.frame);
    cache_.clear();
  }

  // the resident copy of F (a Frame: kind 0, a KeyFrame: kind 1 -- informational, identity is content), created on first
  // use; nullptr when the cache is off
  template <class FrameLike>
  orbfe_frame* resident(const FrameLike& F, int /*kind*/) {
    if (cap_ == 0) return nullptr;
    const unsigned long long ep = orbfe_resident_epoch();
    if (ep != epoch_) { invalidate(); epoch_ = ep; }
    static_assert(sizeof(F.mvKeysUn[0]) == sizeof(OrbfeKeyPoint), "mvKeysUn must hold cv::KeyPoint-layout records");
    const int n = (int)F.mvKeysUn.size();
    const float b[4] = {(float)F.mnMinX, (float)F.mnMaxX, (float)F.mnMinY, (float)F.mnMaxY};
    detail::Hash128 hk, hd;
    detail::hashBytes(hk, F.mvKeysUn.data(), (size_t)n * sizeof(OrbfeKeyPoint));
    detail::hashDescriptorRows(hd, F.mDescriptors, n);
    for (auto it = cache_.begin(); it != cache_.end(); ++it)
      if (it->n == n && it->keys == hk && it->desc == hd && std::memcmp(it->bounds, b, sizeof b) == 0) {
        if (it != cache_.begin()) {   // most recently used first
          Entry e = *it;
          cache_.erase(it);
          cache_.insert(cache_.begin(), e);
        }
        hits_++;
        return cache_.front().frame;
      }
    Entry e;
    e.n = n; e.keys = hk; e.desc = hd;
    std::memcpy(e.bounds, b, sizeof b);
    if (n > 0) e.frame = fromExtractor(F, n, hd, b);
    if (e.frame) fromExtract_++;
    else {
      std::vector<uint8_t> tmp;
      const uint8_t* desc = nullptr;
      if (n) {
        if ((size_t)F.mDescriptors.step == 32) desc = F.mDescriptors.data;
        else {
          tmp.resize((size_t)n * 32);
          for (int i = 0; i < n; i++) std::memcpy(&tmp[(size_t)i * 32], F.mDescriptors.data + (size_t)i * F.mDescriptors.step, 32);
          desc = tmp.data();
        }
      }
      check(orbfe_frame_create(m_, reinterpret_cast<const OrbfeKeyPoint*>(F.mvKeysUn.data()), desc, n, b, &e.frame));
      uploads_++;
    }
    cache_.insert(cache_.begin(), e);
    trim();
    return cache_.front().frame;
  }

  // the resident copy of F if the context HOLDS one (nothing is created, the cache's order stays); nullptr otherwise
  template <class FrameLike>
  orbfe_frame* residentIfHeld(const FrameLike& F) {
    if (cap_ == 0 || cache_.empty() || orbfe_resident_epoch() != epoch_) return nullptr;
    const int n = (int)F.mvKeysUn.size();
    const float b[4] = {(float)F.mnMinX, (float)F.mnMaxX, (float)F.mnMinY, (float)F.mnMaxY};
    detail::Hash128 hk, hd;
    detail::hashBytes(hk, F.mvKeysUn.data(), (size_t)n * sizeof(OrbfeKeyPoint));
    detail::hashDescriptorRows(hd, F.mDescriptors, n);
    for (auto it = cache_.begin(); it != cache_.end(); ++it)
      if (it->n == n && it->keys == hk && it->desc == hd && std::memcmp(it->bounds, b, sizeof b) == 0) return it->frame;
    return nullptr;
  }

  // ---- the local map's descriptors on the device.  Tracking::SearchLocalPoints (Tracking.cc:818-824) sends the same few
  // thousand MapPoints frame after frame; their 32-byte descriptors need not cross PCIe every time.  The context keeps a
  // table of rows keyed by the MapPoint's ADDRESS, in two copies: a page-locked host MIRROR (always complete and current)
  // and the DEVICE rows.  Per search the shim asks for each in-view MapPoint's row:
  //   rowFor(pMP, bytes)   compares GetDescriptor()'s bytes with the mirror row of that MapPoint.  Equal: returns the row
  //                        number -- the kernel reads the device copy.  Different (the descriptor was recomputed,
  //                        MapPoint::ComputeDistinctiveDescriptors, MapPoint.cc:227-292; a new MapPoint; a new object at
  //                        a recycled address): the mirror row is rewritten and the number comes back with bit 31 set --
  //                        the kernel reads THAT row from the mirror, over PCIe, exactly what a search without the table
  //                        does for every row.  The comparison is of the BYTES, so the device copy can never be stale.
  //   tableCommit()        after the search: rows that changed go to the device asynchronously on the matcher's stream
  //                        (runs of neighbouring rows as one copy), ready for the next frame.
  // The local map's order may change from frame to frame (Tracking::UpdateLocalPoints rebuilds the vector): rows belong to
  // MapPoints, not to positions.  Rows of MapPoints that are gone are reclaimed by starting over when the table holds more
  // than 4x the rows one search uses (at least 16 384).
  void tableBegin(size_t nQueries) {
    DescTable& t = table_;
    if (t.pending) { check(orbfe_matcher_synchronize(m_)); t.pending = false; }
    if (t.slotOf.size() > std::max<size_t>(16384, 4 * std::max(nQueries, t.lastQueries))) {
      t.slotOf.clear(); t.used = 0;
      t.dirty.clear();                                     // the rows start over: nothing of the old assignment is owed to the device
      std::fill(t.notOnDevice.begin(), t.notOnDevice.end(), (uint8_t)0);
    }
    t.lastQueries = nQueries;
    // t.dirty is NOT cleared here: rows a previous snapshot rewrote in the mirror and never sent (its search threw before
    // tableCommit) are still owed to the device; until then rowFor hands them out as mirror rows (notOnDevice)
    if (t.cap == 0) growTable(1);
  }
  int32_t rowFor(const void* pMP, const uint8_t* bytes) {
    DescTable& t = table_;
    auto it = t.slotOf.find(pMP);
    uint32_t slot;
    if (it == t.slotOf.end()) {
      slot = (uint32_t)t.used;
      if (t.used + 1 > t.cap) growTable(t.used + 1);
      t.used++;
      t.slotOf.emplace(pMP, slot);
    } else {
      slot = it->second;
      if (std::memcmp(t.mirror + (size_t)slot * 32, bytes, 32) == 0) {
        // equal bytes in the MIRROR say nothing about the device row while an upload of this row has not been enqueued yet: the same
        // MapPoint twice in one vpMapPoints (the reference tolerates that), or a row of a snapshot whose search never committed
        if (t.notOnDevice[slot]) return (int32_t)(slot | 0x80000000u);
        t.rowsFromDevice++;
        return (int32_t)slot;
      }
    }
    std::memcpy(t.mirror + (size_t)slot * 32, bytes, 32);
    if (!t.notOnDevice[slot]) { t.notOnDevice[slot] = 1; t.dirty.push_back(slot); }
    return (int32_t)(slot | 0x80000000u);
  }
  const uint8_t* tableDevice() const { return table_.rows; }
  const uint8_t* tableMirror() const { return table_.mirror; }
  size_t tableRowCapacity() const { return table_.cap; }
  void tableCommit() {
    DescTable& t = table_;
    if (t.dirty.empty()) { t.cleanSearches++; return; }
    std::sort(t.dirty.begin(), t.dirty.end());
    size_t i = 0;
    while (i < t.dirty.size()) {   // runs of changed rows at most 32 rows apart travel as one copy
      size_t j = i;
      while (j + 1 < t.dirty.size() && t.dirty[j + 1] - t.dirty[j] <= 32) j++;
      const size_t lo = t.dirty[i], hi = (size_t)t.dirty[j] + 1;
      t.pending = true;
      if (orbfe_matcher_upload_async(m_, t.rows + lo * 32, t.mirror + lo * 32, (hi - lo) * 32) != ORBFE_OK) {
        t.dirty.erase(t.dirty.begin(), t.dirty.begin() + (std::ptrdiff_t)i);   // rows i.. stay owed (and stay mirror rows)
        check(ORBFE_ERR_HIP);
      }
      for (size_t k = i; k <= j; k++) t.notOnDevice[t.dirty[k]] = 0;   // enqueued on the matcher's stream: in order before the next search
      t.copies++;
      i = j + 1;
    }
    t.rowsChanged += t.dirty.size();
    t.dirty.clear();
  }
  size_t tableRowsChanged() const { return table_.rowsChanged; }        // rows that went to the device (first sight or new bytes)
  size_t tableCleanSearches() const { return table_.cleanSearches; }    // searches that read every descriptor from device memory
  size_t tableRowsFromDevice() const { return table_.rowsFromDevice; }  // descriptor reads served by the device copy
  size_t tableRows() const { return table_.used; }

  // ---- the local map on the device (SearchLocalPoints below): the 64-byte rows of orbfe_local_map (position, normal, raw
  // mfMinDistance / mfMaxDistance, descriptor), keyed by the MapPoint's ADDRESS, with a host mirror.  localMapRow compares a
  // MapPoint's current row with its mirror row BY CONTENT; only rows that differ (a moved MapPoint, a new normal or depth
  // range, a recomputed descriptor, a new MapPoint, a new object at a recycled address) are sent, all of them in one
  // orbfe_local_map_set_rows call by localMapCommit -- asynchronous, ordered before the search on the matcher's stream.
  // Rows of MapPoints that are gone are reclaimed by starting over when the table holds more than 4x the rows one search
  // uses (at least 16 384).
  void localMapBegin(size_t nQueries) {
    LocalMapRows& t = lmap_;
    if (t.rowOf.size() > std::max<size_t>(16384, 4 * std::max(nQueries, t.lastQueries))) {
      t.rowOf.clear(); t.used = 0; t.dirty.clear();   // (every row is new again: none is compared with the mirror)
      std::fill(t.queued.begin(), t.queued.end(), (uint8_t)0);
    }
    t.lastQueries = nQueries;
    if (!t.map) growLocalMap(std::max<size_t>(4096, nQueries + nQueries / 2));
  }
  int32_t localMapRow(const void* pMP, const uint8_t row[64]) {
    LocalMapRows& t = lmap_;
    auto it = t.rowOf.find(pMP);
    int32_t r;
    if (it == t.rowOf.end()) {
      if (t.used + 1 > t.cap) growLocalMap(t.used + 1 + (t.used + 1) / 2);
      r = (int32_t)t.used++;
      t.rowOf.emplace(pMP, r);
    } else {
      r = it->second;
      if (std::memcmp(&t.mirror[(size_t)r * 64], row, 64) == 0) return r;
    }
    if (!t.queued[(size_t)r]) { t.queued[(size_t)r] = 1; t.dirty.push_back(r); }
    std::memcpy(&t.mirror[(size_t)r * 64], row, 64);
    return r;
  }
  void localMapCommit() {
    LocalMapRows& t = lmap_;
    if (t.dirty.empty()) return;
    const size_t n = t.dirty.size();
    std::vector<float> pos(3 * n), nrm(3 * n), dmin(n), dmax(n);
    std::vector<uint8_t> desc(32 * n);
    for (size_t i = 0; i < n; i++) {
      const uint8_t* src = &t.mirror[(size_t)t.dirty[i] * 64];
      std::memcpy(&pos[3 * i], src, 12);
      std::memcpy(&nrm[3 * i], src + 12, 12);
      std::memcpy(&dmin[i], src + 24, 4);
      std::memcpy(&dmax[i], src + 28, 4);
      std::memcpy(&desc[32 * i], src + 32, 32);
    }
    check(orbfe_local_map_set_rows(t.map, (int)n, t.dirty.data(), pos.data(), nrm.data(), dmin.data(), dmax.data(), desc.data()));
    for (int32_t r : t.dirty) t.queued[(size_t)r] = 0;
    t.rowsSent += n;
    t.dirty.clear();
  }
  orbfe_local_map* localMap() const { return lmap_.map; }
  size_t localMapRowsSent() const { return lmap_.rowsSent; }   // rows that went to the device (first sight or new content)
  size_t localMapRows() const { return lmap_.used; }

 private:
  struct Entry { int n = 0; detail::Hash128 keys, desc; float bounds[4] = {0, 0, 0, 0}; orbfe_frame* frame = nullptr; };
  // the extractor route: F.mvKeys are the records some live Extractor of this device returned last (same count, same
  // bytes, same descriptor rows) -> its arena still holds them
  template <class FrameLike>
  orbfe_frame* fromExtractor(const FrameLike& F, int n, const detail::Hash128& hd, const float b[4]) {
    if ((int)F.mvKeys.size() != n) return nullptr;
    detail::Hash128 hraw;
    detail::hashBytes(hraw, F.mvKeys.data(), (size_t)n * sizeof(OrbfeKeyPoint));
    // undistorted coordinates only when they differ from the extracted ones (Frame.cc:288-292: no distortion => mvKeysUn = mvKeys)
    const bool same = std::memcmp(static_cast<const void*>(F.mvKeys.data()), static_cast<const void*>(F.mvKeysUn.data()),
                                  (size_t)n * sizeof(OrbfeKeyPoint)) == 0;
    std::vector<float> xy;
    if (!same) {
      xy.resize((size_t)n * 2);
      for (int i = 0; i < n; i++) std::memcpy(&xy[2 * (size_t)i], &F.mvKeysUn[i], 8);   // pt = the first two floats
      // everything but pt must be what the extractor returned (UndistortKeyPoints copies the record and replaces pt)
      for (int i = 0; i < n; i++)
        if (std::memcmp(reinterpret_cast<const char*>(&F.mvKeys[i]) + 8, reinterpret_cast<const char*>(&F.mvKeysUn[i]) + 8,
                        sizeof(OrbfeKeyPoint) - 8) != 0)
          return nullptr;
    }
    size_t sent = 0;
    orbfe_frame* f = Extractor::residentFromLastExtract(device_, n, hraw, hd, b, same ? nullptr : xy.data(), &sent);
    if (f) coordBytes_ += sent;
    return f;
  }
  void trim() {
    const size_t keep = cap_ == 0 ? 0 : std::max<size_t>(cap_, 2);   // a search uses up to two frames: never evict those
    while (cache_.size() > keep) {
      orbfe_frame_destroy(cache_.back().frame);
      cache_.pop_back();
    }
  }
  orbfe_matcher* m_ = nullptr;
  int device_ = 0;
  size_t cap_ = 48, uploads_ = 0, fromExtract_ = 0, hits_ = 0, coordBytes_ = 0;
  unsigned long long epoch_ = 0;
  std::vector<Entry> cache_;
  struct Scratch { void* p = nullptr; size_t bytes = 0; };
  Scratch scratch_[8];
  struct DescTable {
    uint8_t *rows = nullptr, *mirror = nullptr;   // device rows; page-locked host mirror (complete and current)
    size_t cap = 0, used = 0, lastQueries = 0;
    std::unordered_map<const void*, uint32_t> slotOf;   // MapPoint address -> row
    std::vector<uint32_t> dirty;                  // rows rewritten in the mirror whose upload has not been enqueued yet (each once)
    std::vector<uint8_t> notOnDevice;             // [cap] 1: the row is in `dirty` -- rowFor hands it out as a mirror row whatever the bytes
    size_t rowsChanged = 0, rowsFromDevice = 0, cleanSearches = 0, copies = 0;
    bool pending = false;                         // an upload from the mirror may still be in flight
  };
  void growTable(size_t need) {
    DescTable& t = table_;
    const size_t cap = std::max<size_t>(4096, need + need / 2);
    void *h = nullptr, *d = nullptr;
    check(orbfe_host_alloc(cap * 32, &h));
    if (orbfe_device_malloc(device_, cap * 32, &d) != ORBFE_OK) { orbfe_host_free(h); check(ORBFE_ERR_HIP); }
    if (t.cap) {   // (no upload is in flight here: tableBegin has waited, tableCommit comes after the search)
      std::memcpy(h, t.mirror, t.cap * 32);
      check(orbfe_device_upload(device_, d, t.mirror, t.cap * 32));
      orbfe_device_free(device_, t.rows);
      orbfe_host_free(t.mirror);
    }
    t.mirror = static_cast<uint8_t*>(h);
    t.rows = static_cast<uint8_t*>(d);
    t.cap = cap;
    t.notOnDevice.resize(cap, 0);
  }
  DescTable table_;
  struct LocalMapRows {
    orbfe_local_map* map = nullptr;
    size_t cap = 0, used = 0, lastQueries = 0, rowsSent = 0;
    std::unordered_map<const void*, int32_t> rowOf;   // MapPoint address -> row
    std::vector<uint8_t> mirror;                      // [cap][64] what the device rows hold (or will, once `dirty` is sent)
    std::vector<int32_t> dirty;                       // rows whose new content has not been sent yet (each once)
    std::vector<uint8_t> queued;                      // [cap] 1: the row is in `dirty`
  };
  void growLocalMap(size_t cap) {
    LocalMapRows& t = lmap_;
    orbfe_local_map* m = nullptr;
    check(orbfe_local_map_create(m_, (int)cap, &m));
    if (t.map) {   // the new table starts empty: every row in use is sent again with the next commit
      orbfe_local_map_destroy(t.map);
      for (size_t r = 0; r < t.used; r++)
        if (!t.queued[r]) { t.queued[r] = 1; t.dirty.push_back((int32_t)r); }
    }
    t.map = m;
    t.cap = cap;
    t.mirror.resize(cap * 64, 0);
    t.queued.resize(cap, 0);
  }
  LocalMapRows lmap_;
};

namespace detail {
// rows of a CV_8U N x 32 descriptor matrix -> contiguous bytes (cv::Mat has public data/step/rows)
template <class MatT>
inline const uint8_t* packedDescriptors(const MatT& m, int n, std::vector<uint8_t>& tmp) {
  if (n == 0) return nullptr;
  if ((size_t)m.step == 32) return m.data;
  tmp.resize((size_t)n * 32);
  for (int i = 0; i < n; i++) std::memcpy(&tmp[(size_t)i * 32], m.data + (size_t)i * m.step, 32);
  return tmp.data();
}

// The descriptor rows of F for the bag-of-words searches: its resident copy's rows in device memory when the context's cache
// is on (nothing is copied then), else the packed host rows.
template <class FrameLike>
inline const uint8_t* descriptorRows(MatcherContext& ctx, const FrameLike& F, int kind, int n, std::vector<uint8_t>& tmp) {
  if (n > 0)
    if (orbfe_frame* rf = ctx.resident(F, kind))
      if (const uint8_t* rows = orbfe_frame_descriptors_device(rf)) return rows;
  return packedDescriptors(F.mDescriptors, n, tmp);
}
template <class FrameT>
inline void frameBounds(const FrameT& F, float b[4]) {
  b[0] = F.mnMinX; b[1] = F.mnMaxX; b[2] = F.mnMinY; b[3] = F.mnMaxY;
}
}  // namespace detail

// int ORBmatcher::DescriptorDistance(const cv::Mat& a, const cv::Mat& b)   (ORBmatcher.cc:1605-1621)
template <class MatT>
inline int DescriptorDistance(const MatT& a, const MatT& b) { return orbfe_hamming(a.data, b.data); }

// int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched,
//                                         vector<int>& vnMatches12, int windowSize)   (ORBmatcher.cc:400-515)
template <class FrameT, class Point2fT>
inline int SearchForInitialization(MatcherContext& ctx, float mfNNratio, bool mbCheckOrientation, FrameT& F1,
                                   FrameT& F2, std::vector<Point2fT>& vbPrevMatched, std::vector<int>& vnMatches12,
                                   int windowSize) {
  static_assert(sizeof(Point2fT) == 8, "Point2fT must be two packed floats (cv::Point2f)");
  const int n1 = (int)F1.mvKeysUn.size(), n2 = (int)F2.mvKeysUn.size();
  vnMatches12.assign(n1, -1);
  std::vector<uint8_t> t1, t2;
  float b[4];
  detail::frameBounds(F2, b);
  int nmatches = 0;
  check(orbfe_search_for_initialization(
      ctx.get(), reinterpret_cast<const OrbfeKeyPoint*>(F1.mvKeysUn.data()),
      detail::packedDescriptors(F1.mDescriptors, n1, t1), n1,
      reinterpret_cast<const OrbfeKeyPoint*>(F2.mvKeysUn.data()), detail::packedDescriptors(F2.mDescriptors, n2, t2),
      n2, b, reinterpret_cast<float*>(vbPrevMatched.data()), vnMatches12.data(), windowSize, mfNNratio,
      mbCheckOrientation ? 1 : 0, &nmatches));
  return nmatches;
}

// What the two RANSAC loops of Initializer::Initialize leave behind (Initializer.cc:99-109): FindHomography's and
// FindFundamental's outputs, the iteration each of them kept (-1: no score above 0, the reference's H / F stay empty), and
// currentScore of every iteration.
struct InitializerScores {
  std::vector<bool> vbMatchesInliersH, vbMatchesInliersF;
  float SH = 0.f, SF = 0.f;
  int bestH = -1, bestF = -1;
  std::vector<float> scoresH, scoresF;
};

// float Initializer::CheckHomography / CheckFundamental (Initializer.cc:305-388, :390-468) for every hypothesis, and the
// keep-the-best rule of FindHomography / FindFundamental (:148-171, :199-222), in one GPU call.  keys1 / keys2 = mvKeys1 /
// mvKeys2, matches12 = mvMatches12, sigma = mSigma; H21s[it], H12s[it], F21s[it] = H21i, H12i, F21i of iteration `it`
// (3 x 3, float, read through at<float>(r, c)).  H21s and H12s come together; a model whose vectors are empty is skipped.
template <class KeyPointT, class MatT>
inline void ScoreInitializerHypotheses(MatcherContext& ctx, const std::vector<KeyPointT>& keys1, const std::vector<KeyPointT>& keys2,
                                       const std::vector<std::pair<int, int>>& matches12, float sigma, const std::vector<MatT>& H21s,
                                       const std::vector<MatT>& H12s, const std::vector<MatT>& F21s, InitializerScores& result) {
  const int N = (int)matches12.size();
  const bool hasH = !H21s.empty() || !H12s.empty(), hasF = !F21s.empty();
  const int K = (int)(hasF ? F21s.size() : H21s.size());
  if (hasH && (H21s.size() != (size_t)K || H12s.size() != (size_t)K))
    throw std::runtime_error("orbfe: ScoreInitializerHypotheses needs as many H21 as H12 (and F21) hypotheses");
  std::vector<float> pts((size_t)N * 4), h21, h12, f21;
  for (int i = 0; i < N; i++) {   // Initializer.cc:341-347
    const KeyPointT& kp1 = keys1[matches12[i].first];
    const KeyPointT& kp2 = keys2[matches12[i].second];
    pts[4 * (size_t)i] = kp1.pt.x; pts[4 * (size_t)i + 1] = kp1.pt.y; pts[4 * (size_t)i + 2] = kp2.pt.x; pts[4 * (size_t)i + 3] = kp2.pt.y;
  }
  auto pack = [K](const std::vector<MatT>& ms, std::vector<float>& out) {
    out.resize((size_t)K * 9);
    for (int k = 0; k < K; k++)
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) out[(size_t)k * 9 + 3 * r + c] = ms[k].template at<float>(r, c);
  };
  if (hasH) { pack(H21s, h21); pack(H12s, h12); }
  if (hasF) pack(F21s, f21);
  std::vector<uint8_t> inH((size_t)N + 1), inF((size_t)N + 1);
  result = InitializerScores();
  result.scoresH.assign(hasH ? K : 0, 0.f);
  result.scoresF.assign(hasF ? K : 0, 0.f);
  check(orbfe_score_init_hypotheses(ctx.get(), pts.data(), N, sigma, K, hasH ? h21.data() : nullptr, hasH ? h12.data() : nullptr,
                                    hasF ? f21.data() : nullptr, result.scoresH.data(), result.scoresF.data(), &result.bestH,
                                    &result.bestF, &result.SH, &result.SF, inH.data(), inF.data()));
  result.vbMatchesInliersH.assign(N, false);
  result.vbMatchesInliersF.assign(N, false);
  for (int i = 0; i < N; i++) {
    if (hasH) result.vbMatchesInliersH[i] = inH[i] != 0;
    if (hasF) result.vbMatchesInliersF[i] = inF[i] != 0;
  }
}

// int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th)
// (ORBmatcher.cc:45-124).  MapPoint fields are snapshotted through the reference's own accessors
// (isBad(), GetDescriptor(), Observations() take the MapPoint mutexes, MapPoint.cc:126-129,294-298)
// BEFORE the GPU call; assignments are written back to F.mvpMapPoints afterwards.
template <class FrameT, class MapPointT>
inline int SearchByProjection(MatcherContext& ctx, float mfNNratio, FrameT& F,
                              const std::vector<MapPointT*>& vpMapPoints, const float th) {
  const int n = (int)F.mvKeysUn.size(), nmp = (int)vpMapPoints.size();
  // snapshots go into the context's page-locked arrays (flags and levels zeroed: an absent MapPoint is "not in view", level 0)
  uint8_t* occ = ctx.scratch<uint8_t>(0, n, true);
  uint8_t* flags = ctx.scratch<uint8_t>(1, nmp, true);
  float* xy = ctx.scratch<float>(3, (size_t)nmp * 2, false);
  float* vcos = ctx.scratch<float>(4, nmp, false);
  int32_t* lvl = ctx.scratch<int32_t>(5, nmp, true);
  int32_t* assigned = ctx.scratch<int32_t>(6, n, false);
  float b[4];
  detail::frameBounds(F, b);
  orbfe_frame* rf = ctx.resident(F, 0);
  // With a resident frame the MapPoints' descriptors come from the context's device table (rows keyed by MapPoint, only
  // changed rows cross PCIe); the host-array call form takes plain rows.
  int32_t* drow = rf ? ctx.scratch<int32_t>(2, nmp, true) : nullptr;
  uint8_t* mdesc = rf ? nullptr : ctx.scratch<uint8_t>(2, (size_t)nmp * 32, false);
  if (rf) ctx.tableBegin((size_t)nmp);
  std::vector<uint8_t> tmp;
  for (int i = 0; i < n; i++) assigned[i] = -1;
  for (int i = 0; i < n; i++)
    if (F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0) occ[i] = 1;
  for (int i = 0; i < nmp; i++) {
    MapPointT* p = vpMapPoints[i];
    xy[2 * i] = 0.f; xy[2 * i + 1] = 0.f; vcos[i] = 0.f;
    if (!p->mbTrackInView) continue;
    if (p->isBad()) { flags[i] = ORBFE_MP_IN_VIEW | ORBFE_MP_BAD; continue; }
    flags[i] = ORBFE_MP_IN_VIEW | (p->plCandidato ? ORBFE_MP_CANDIDATO : 0) |
               (p->Observations() > 0 ? ORBFE_MP_OBSERVED : 0);
    xy[2 * i] = p->mTrackProjX;
    xy[2 * i + 1] = p->mTrackProjY;
    lvl[i] = p->mnTrackScaleLevel;
    vcos[i] = p->mTrackViewCos;
    const auto d = p->GetDescriptor();
    if (rf) drow[i] = ctx.rowFor(p, d.data);
    else std::memcpy(&mdesc[(size_t)i * 32], d.data, 32);
  }
  int nmatches = 0;
  if (rf) {
    check(orbfe_search_by_projection_frame_rows(ctx.get(), rf, F.mvScaleFactors.data(), (int)F.mvScaleFactors.size(), occ, xy, lvl,
                                                vcos, flags, ctx.tableDevice(), ctx.tableMirror(), drow, (int)ctx.tableRowCapacity(), nmp, th,
                                                mfNNratio, assigned, &nmatches));
    ctx.tableCommit();
  } else
    check(orbfe_search_by_projection(ctx.get(), reinterpret_cast<const OrbfeKeyPoint*>(F.mvKeysUn.data()),
                                     detail::packedDescriptors(F.mDescriptors, n, tmp), n, b, F.mvScaleFactors.data(),
                                     (int)F.mvScaleFactors.size(), occ, xy, lvl, vcos, flags, mdesc, nmp, th, mfNNratio,
                                     assigned, &nmatches));
  for (int i = 0; i < n; i++)
    if (assigned[i] >= 0) F.mvpMapPoints[i] = vpMapPoints[assigned[i]];
  return nmatches;
}

// ---------------------------------------------------------------------------------------------------------------
// Pose-driven searches.  The reference projects MapPoints with cv::Mat expressions; what those expressions compute
// is OpenCV arithmetic.  RestatedOps restates it (OpenCV 4.x core/src/matmul.simd.hpp small-matrix gemm path,
// matrix_expressions.cpp, norm.cpp; recalled) so that this header needs no OpenCV; a build that
// has OpenCV passes CvOps (include/orbfe/ORBmatcher.h), whose members ARE the reference's expressions.
// ---------------------------------------------------------------------------------------------------------------
namespace detail {
struct RestatedOps {
  // alpha * A(3x3) * b(3x1) + beta * c   -- `Rcw*x3Dw+tcw`, `-sR21*t12` (gemm, flags 0, len 3: float dot, double epilogue)
  static void gemm3(const float A[9], const float b[3], double alpha, const float* c, double beta, float d[3]) {
    for (int i = 0; i < 3; i++) {
      const float t = A[3 * i] * b[0] + A[3 * i + 1] * b[1] + A[3 * i + 2] * b[2];
      d[i] = (float)((double)t * alpha + (double)(c ? c[i] : 0.f) * beta);
    }
  }
  // alpha * A.t() * b   -- `-Rcw.t()*tcw` (gemm with GEMM_1_T: generic path, double accumulation)
  static void gemmT3(const float A[9], const float b[3], double alpha, float d[3]) {
    for (int i = 0; i < 3; i++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += (double)A[3 * k + i] * (double)b[k];
      d[i] = (float)(s * alpha);
    }
  }
  static double norm3(const float v[3]) {   // cv::norm(v)
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
    return std::sqrt(s);
  }
  static double dot3(const float a[3], const float b[3]) {   // a.dot(b)
    double r = 0;
    for (int k = 0; k < 3; k++) r += (double)a[k] * (double)b[k];
    return r;
  }
  static void scale(const float* M, int n, double s, float* out) {   // `s*M` (MatExpr scale -> convertTo with a float factor)
    const float f = (float)s;
    for (int i = 0; i < n; i++) out[i] = M[i] * f;
  }
  static void divide(const float* M, int n, double s, float* out) { scale(M, n, 1.0 / s, out); }   // `M/s` = M * (1./s)
};

template <class MatT>
inline void poseRt(const MatT& T, float R[9], float t[3]) {   // T.rowRange(0,3).colRange(0,3), T.rowRange(0,3).col(3)
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[3 * r + c] = T.template at<float>(r, c);
    t[r] = T.template at<float>(r, 3);
  }
}
template <class MatT>
inline void vec3(const MatT& m, float v[3]) {
  for (int r = 0; r < 3; r++) v[r] = m.template at<float>(r, 0);
}
template <class MatT>
inline void mat33(const MatT& m, float v[9]) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) v[3 * r + c] = m.template at<float>(r, c);
}
// Scw -> Rcw, tcw, Ow   (ORBmatcher.cc:293-298, 949-954)
template <class Ops, class MatT>
inline void decomposeScw(const MatT& Scw, float Rcw[9], float tcw[3], float Ow[3]) {
  float sR[9], st[3];
  poseRt(Scw, sR, st);
  const float scw = (float)std::sqrt(Ops::dot3(sR, sR));
  Ops::divide(sR, 9, (double)scw, Rcw);   // sRcw/scw
  Ops::divide(st, 3, (double)scw, tcw);   // Scw.rowRange(0,3).col(3)/scw
  Ops::gemmT3(Rcw, tcw, -1.0, Ow);
}

// one windowed search of MapPoints projected into a KeyFrame (the loops of SearchByProjection(KF, Scw), Fuse x2, SearchBySim3)
struct ProjectedSources {
  std::vector<float> uv, radius;
  std::vector<int32_t> level, bestIdx, bestDist;
  std::vector<uint8_t> valid, desc;
  explicit ProjectedSources(size_t n) : uv(2 * n, 0.f), radius(n, 0.f), level(n, 0), bestIdx(n, -1), bestDist(n, -1), valid(n, 0), desc(32 * n, 0) {}
};
template <class KeyFrameT>
inline int searchProjected(MatcherContext& ctx, KeyFrameT* pKF, ProjectedSources& S, const uint8_t* kp_skip, int claim,
                           bool chi2, int max_dist) {
  const int n = (int)pKF->mvKeysUn.size(), ns = (int)S.valid.size();
  std::vector<uint8_t> tmp;
  float b[4];
  frameBounds(*pKF, b);
  int nm = 0;
  if (orbfe_frame* rf = ctx.resident(*pKF, 1))
    check(orbfe_search_projected_frame(ctx.get(), rf, ns, S.uv.data(), S.radius.data(), S.level.data(), S.valid.data(), S.desc.data(),
                                       kp_skip, claim, chi2 ? pKF->mvInvLevelSigma2.data() : nullptr,
                                       chi2 ? (int)pKF->mvInvLevelSigma2.size() : 0, 5.99, max_dist, S.bestIdx.data(),
                                       S.bestDist.data(), &nm));
  else
    check(orbfe_search_projected(ctx.get(), reinterpret_cast<const OrbfeKeyPoint*>(pKF->mvKeysUn.data()),
                                 packedDescriptors(pKF->mDescriptors, n, tmp), n, b, ns, S.uv.data(), S.radius.data(),
                                 S.level.data(), S.valid.data(), S.desc.data(), kp_skip, claim,
                                 chi2 ? pKF->mvInvLevelSigma2.data() : nullptr, chi2 ? (int)pKF->mvInvLevelSigma2.size() : 0, 5.99,
                                 max_dist, S.bestIdx.data(), S.bestDist.data(), &nm));
  return nm;
}
// the part of the KeyFrame-side loops between GetWorldPos and GetFeaturesInArea (:322-355, 826-873, 972-1013): fills
// source i and returns whether the point survives the depth / image / distance / viewing-angle tests
template <class Ops, class KeyFrameT, class MapPointT>
inline bool projectIntoKeyFrame(KeyFrameT* pKF, MapPointT* pMP, const float Rcw[9], const float tcw[3], const float Ow[3],
                                float th, bool invzDouble, ProjectedSources& S, size_t i) {
  float p3Dw[3], p3Dc[3];
  vec3(pMP->GetWorldPos(), p3Dw);
  Ops::gemm3(Rcw, p3Dw, 1.0, tcw, 1.0, p3Dc);
  if (p3Dc[2] < 0.0f) return false;
  const float invz = invzDouble ? (float)(1.0 / p3Dc[2]) : 1 / p3Dc[2];
  const float x = p3Dc[0] * invz, y = p3Dc[1] * invz;
  const float u = pKF->fx * x + pKF->cx, v = pKF->fy * y + pKF->cy;
  if (!pKF->IsInImage(u, v)) return false;
  const float maxDistance = pMP->GetMaxDistanceInvariance(), minDistance = pMP->GetMinDistanceInvariance();
  const float PO[3] = {p3Dw[0] - Ow[0], p3Dw[1] - Ow[1], p3Dw[2] - Ow[2]};
  const float dist3D = (float)Ops::norm3(PO);
  if (dist3D < minDistance || dist3D > maxDistance) return false;
  float Pn[3];
  vec3(pMP->GetNormal(), Pn);
  if (Ops::dot3(PO, Pn) < 0.5 * dist3D) return false;
  const int nPredictedLevel = pMP->PredictScale(dist3D, pKF->mfLogScaleFactor);
  S.uv[2 * i] = u; S.uv[2 * i + 1] = v;
  S.level[i] = nPredictedLevel;
  S.radius[i] = th * pKF->mvScaleFactors[nPredictedLevel];
  const auto d = pMP->GetDescriptor();
  std::memcpy(&S.desc[32 * i], d.data, 32);
  S.valid[i] = 1;
  return true;
}
// the row of MapPoint p in the context's local-map table (MatcherContext::localMapRow): what `geometry` hands over, then
// GetDescriptor()
template <class MapPointT, class GeometryFn>
inline int32_t sourceRow(MatcherContext& ctx, MapPointT* p, GeometryFn& geometry) {
  float row[16];
  float& minRaw = row[6];
  float& maxRaw = row[7];
  geometry(p, row, row + 3, minRaw, maxRaw);
  const auto d = p->GetDescriptor();
  std::memcpy(row + 8, d.data, 32);
  return ctx.localMapRow(p, reinterpret_cast<const uint8_t*>(row));
}
}  // namespace detail

// ---------------------------------------------------------------------------------------------------------------
// void Tracking::SearchLocalPoints()  (src/Tracking.cc:798-825), from the projection loop onwards: for every local MapPoint
// that is not skipped (mnLastFrameSeen == F.mnId) and not bad, Frame::isInFrustum(pMP, viewingCosLimit) (src/Frame.cc:151-207),
// IncreaseVisible() for the ones in view, then SearchByProjection(F, vpLocalMapPoints, th) with ORBmatcher(0.8) -- the
// projection and the search in one GPU submission (orbfe_search_local_points_frame).  The caller keeps the loop in front of it
// (Tracking.cc:784-796: MapPoints already matched in F get mnLastFrameSeen = F.mnId and mbTrackInView = false) and chooses th
// (1, or 5 right after a relocalisation, :820-822).
// os1 keeps a MapPoint's mWorldPos, mNormalVector and mfMinDistance / mfMaxDistance protected (include/MapPoint.h): the
// integrator hands them over with `geometry(pMP, pos, normal, minRaw, maxRaw)` (float pos[3], normal[3]; float& minRaw,
// maxRaw = the RAW fields, not the 0.8f / 1.2f invariance bounds), under the MapPoint's position mutex.  The rows go to the
// context's device table (changed rows only, MatcherContext::localMapRow).  Written back, as the reference does:
// mbTrackInView, mTrackProjX / Y, mnTrackScaleLevel, mTrackViewCos of every projected MapPoint (isInFrustum sets
// mbTrackInView = false first and leaves the other fields alone when it returns false), IncreaseVisible(), F.mvpMapPoints.
// Returns the number of matches.  F's pose: Rcw, tcw from F.mTcw (UpdatePoseMatrices' views of it), Ow = F.GetCameraCenter().
template <class FrameT, class MapPointT, class GeometryFn>
inline int SearchLocalPoints(MatcherContext& ctx, FrameT& F, const std::vector<MapPointT*>& vpLocalMapPoints, float th,
                             float viewingCosLimit, GeometryFn geometry) {
  const int n = (int)F.mvKeysUn.size(), nmp = (int)vpLocalMapPoints.size();
  uint8_t* occ = ctx.scratch<uint8_t>(0, n, true);
  uint8_t* flags = ctx.scratch<uint8_t>(1, nmp, true);
  int32_t* rows = ctx.scratch<int32_t>(2, nmp, true);
  uint8_t* inView = ctx.scratch<uint8_t>(3, nmp, false);
  float* xy = ctx.scratch<float>(4, (size_t)nmp * 2, false);
  int32_t* lvl = ctx.scratch<int32_t>(5, nmp, false);
  int32_t* assigned = ctx.scratch<int32_t>(6, n, false);
  float* vcos = ctx.scratch<float>(7, nmp, false);
  OrbfeCamera cam;
  detail::poseRt(F.mTcw, cam.Rcw, cam.tcw);
  detail::vec3(F.GetCameraCenter(), cam.Ow);
  cam.fx = F.fx; cam.fy = F.fy; cam.cx = F.cx; cam.cy = F.cy;
  cam.logScaleFactor = F.mfLogScaleFactor;
  for (int i = 0; i < n; i++)
    if (F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0) occ[i] = 1;
  ctx.localMapBegin((size_t)nmp);
  for (int i = 0; i < nmp; i++) {
    MapPointT* p = vpLocalMapPoints[i];
    if (p->mnLastFrameSeen == F.mnId) { flags[i] = ORBFE_MP_SKIP; continue; }   // Tracking.cc:804-805
    if (p->isBad()) { flags[i] = ORBFE_MP_BAD; continue; }                       // :806-807
    flags[i] = (uint8_t)((p->plCandidato ? ORBFE_MP_CANDIDATO : 0) | (p->Observations() > 0 ? ORBFE_MP_OBSERVED : 0));
    rows[i] = detail::sourceRow(ctx, p, geometry);
  }
  ctx.localMapCommit();
  orbfe_frame* rf = ctx.resident(F, 0);
  orbfe_frame* tmpFrame = nullptr;
  if (!rf) {   // the context's frame cache is off: a frame for this call only
    float b[4];
    detail::frameBounds(F, b);
    std::vector<uint8_t> tmp;
    check(orbfe_frame_create(ctx.get(), reinterpret_cast<const OrbfeKeyPoint*>(F.mvKeysUn.data()),
                             detail::packedDescriptors(F.mDescriptors, n, tmp), n, b, &tmpFrame));
    rf = tmpFrame;
  }
  int nmatches = 0, nInView = 0;
  const int rc = orbfe_search_local_points_frame(ctx.get(), rf, ctx.localMap(), &cam, viewingCosLimit, rows, flags, nmp,
                                                 F.mvScaleFactors.data(), (int)F.mvScaleFactors.size(), occ, th, 0.8f, inView, xy,
                                                 lvl, vcos, assigned, &nmatches, &nInView);
  if (tmpFrame) orbfe_frame_destroy(tmpFrame);
  check(rc);
  for (int i = 0; i < nmp; i++) {
    if (flags[i] & (ORBFE_MP_SKIP | ORBFE_MP_BAD)) continue;
    MapPointT* p = vpLocalMapPoints[i];
    p->mbTrackInView = inView[i] != 0;
    if (!inView[i]) continue;
    p->mTrackProjX = xy[2 * i];
    p->mTrackProjY = xy[2 * i + 1];
    p->mnTrackScaleLevel = lvl[i];
    p->mTrackViewCos = vcos[i];
    p->IncreaseVisible();
  }
  for (int i = 0; i < n; i++)
    if (assigned[i] >= 0) F.mvpMapPoints[i] = vpLocalMapPoints[assigned[i]];
  return nmatches;
}

// ---------------------------------------------------------------------------------------------------------------
// The six pose-driven searches: ONE function per search, TWO middles.
// Each search is written once, as a detail::...Impl that owns everything around the search itself -- the pose set-up, which
// sources are projected (`classify(i)`: 0 = project, else the flag byte ORBFE_MP_SKIP / ORBFE_MP_BAD), the occupancy bytes
// and the bookkeeping that follows -- and takes the middle step as a callable.  The two public forms of a search pass
//   the host middle  (SearchByProjection / Fuse / SearchBySim3, the reference's names): project on the host where classify
//                    allows it, then one windowed search (detail::searchProjectedUv into a Frame, searchProjected into a KeyFrame);
//   the GPU middle   (SearchByProjectionLastFrame / ...KeyFrame / ...Scw, FuseKeyFrame, FuseScw, SearchBySim3Device; last argument
//                    SearchLocalPoints' `geometry` functor): classify's byte and one row number per source (detail::sourceRows)
//                    are all that crosses PCIe, then projection, windows and best match in one call.  The source frame's resident
//                    copy supplies mvKeys[i].octave and mvKeysUn[i].angle (both copies of one record: Frame::UndistortKeyPoints
//                    replaces pt only); positions, normals, depth ranges and descriptors are rows of the context's local-map
//                    table -- SearchLocalPoints' rows, so a MapPoint keeps ONE row and only changed rows are sent.  The fused
//                    keyframe call refuses a valid point whose predicted level lies outside the keyframe's pyramid (the
//                    reference would index mvScaleFactors out of range with it).
// A GPU form first makes its frames resident; when it cannot (frame cache off, sizes that do not line up, a pyramid the fused
// call does not take) it IS the host form, with the caller's Ops.  All twelve take `class Ops = detail::RestatedOps` first;
// SearchByProjectionLastFrame / ...KeyFrame gained it last, and as no call names Ops for these two (their other template
// parameters are deduced) every existing call compiles to what it did.
// ---------------------------------------------------------------------------------------------------------------
namespace detail {
template <class Ops, class FrameT>
inline void currentCamera(const FrameT& F, OrbfeCamera& cam) {
  poseRt(F.mTcw, cam.Rcw, cam.tcw);
  Ops::gemmT3(cam.Rcw, cam.tcw, -1.0, cam.Ow);   // -Rcw.t()*tcw (ORBmatcher.cc:1431; the LastFrame form does not read it)
  cam.fx = F.fx; cam.fy = F.fy; cam.cx = F.cx; cam.cy = F.cy;
  cam.logScaleFactor = F.mfLogScaleFactor;
}
// one windowed search of sources projected on the host into a Frame (the two frame-side host middles), as searchProjected
// is for a KeyFrame
template <class FrameT>
inline int searchProjectedUv(MatcherContext& ctx, FrameT& F, const uint8_t* occ, const float* uv, const int32_t* lvl, const float* ang,
                             const uint8_t* flags, const uint8_t* valid, const uint8_t* sdesc, int ns, float th, int max_dist,
                             int skip_any_occupied, bool checkOrientation, int32_t* assigned) {
  const int n = (int)F.mvKeysUn.size();
  std::vector<uint8_t> tmp;
  float b[4];
  frameBounds(F, b);
  int nmatches = 0;
  if (orbfe_frame* rf = ctx.resident(F, 0))
    check(orbfe_search_by_projection_uv_frame(ctx.get(), rf, F.mvScaleFactors.data(), (int)F.mvScaleFactors.size(), occ, uv, lvl, ang,
                                              flags, valid, sdesc, ns, th, max_dist, skip_any_occupied, checkOrientation ? 1 : 0,
                                              assigned, &nmatches));
  else
    check(orbfe_search_by_projection_uv(ctx.get(), reinterpret_cast<const OrbfeKeyPoint*>(F.mvKeysUn.data()),
                                        packedDescriptors(F.mDescriptors, n, tmp), n, b, F.mvScaleFactors.data(),
                                        (int)F.mvScaleFactors.size(), occ, uv, lvl, ang, flags, valid, sdesc, ns, th, max_dist,
                                        skip_any_occupied, checkOrientation ? 1 : 0, assigned, &nmatches));
  return nmatches;
}
// the source loop of every GPU middle: flags[i] = classify(i), and the local-map row of each source that is projected
template <class PointsT, class Classify, class GeometryFn>
inline void sourceRows(MatcherContext& ctx, const PointsT& pts, int ns, Classify classify, GeometryFn& geometry, uint8_t*& flags,
                       int32_t*& rows) {
  flags = ctx.scratch<uint8_t>(1, ns, true);
  rows = ctx.scratch<int32_t>(2, ns, true);
  ctx.localMapBegin((size_t)ns);
  for (int i = 0; i < ns; i++) {
    flags[i] = classify(i);
    if (!(flags[i] & (ORBFE_MP_SKIP | ORBFE_MP_BAD))) rows[i] = sourceRow(ctx, pts[i], geometry);
  }
  ctx.localMapCommit();
}
// the GPU middle of the two frame-side searches
template <class Ops, class FrameT, class PointsT, class Classify, class GeometryFn>
inline int searchSourcesFrame(MatcherContext& ctx, orbfe_frame* cur, orbfe_frame* src, const FrameT& CurrentFrame, int source_mode,
                              const PointsT& pts, int ns, Classify classify, GeometryFn& geometry, const uint8_t* occ, float th,
                              int max_dist, bool checkOrientation, int32_t* assigned) {
  uint8_t* flags;
  int32_t* rows;
  sourceRows(ctx, pts, ns, classify, geometry, flags, rows);
  OrbfeCamera cam;
  currentCamera<Ops>(CurrentFrame, cam);
  int nmatches = 0, nValid = 0;
  check(orbfe_search_by_projection_sources_frame(ctx.get(), cur, src, ctx.localMap(), &cam, source_mode, rows, flags, ns,
                                                 CurrentFrame.mvScaleFactors.data(), (int)CurrentFrame.mvScaleFactors.size(), occ, th,
                                                 max_dist, checkOrientation ? 1 : 0, nullptr, nullptr, nullptr, assigned, &nmatches,
                                                 &nValid));
  return nmatches;
}
// the write-back of the two frame-side searches: assigned[i] >= 0 is a source index, -2 a match the rotation check took
// away (:1409-1419, :1538-1548)
template <class FrameT, class PointsT>
inline void assignFromSources(FrameT& CurrentFrame, const int32_t* assigned, const PointsT& sources) {
  const int n = (int)CurrentFrame.mvKeysUn.size();
  for (int i = 0; i < n; i++) {
    if (assigned[i] >= 0) CurrentFrame.mvpMapPoints[i] = sources[assigned[i]];
    else if (assigned[i] == -2) CurrentFrame.mvpMapPoints[i] = nullptr;
  }
}

// SearchByProjection(Cur, Last, th).  middle(classify, occ, assigned) -> nmatches.  ORBFE_MP_OBSERVED is not classify's: each
// middle reads Observations() where it does today (the host one after the projection, for the sources that survive it).
template <class FrameT, class Middle>
inline int searchByProjectionLastFrameImpl(MatcherContext& ctx, FrameT& CurrentFrame, const FrameT& LastFrame, Middle middle) {
  const int n = (int)CurrentFrame.mvKeysUn.size();
  // the context's page-locked arrays (see SearchByProjection(F, MapPoints) above)
  uint8_t* occ = ctx.scratch<uint8_t>(0, n, true);
  int32_t* assigned = ctx.scratch<int32_t>(6, n, false);
  for (int i = 0; i < n; i++)
    if (CurrentFrame.mvpMapPoints[i] && CurrentFrame.mvpMapPoints[i]->Observations() > 0) occ[i] = 1;   // :1364-1366
  auto classify = [&](int i) -> uint8_t {                                                                // :1318-1321
    return !LastFrame.mvpMapPoints[i] || LastFrame.mvbOutlier[i] ? (uint8_t)ORBFE_MP_SKIP : (uint8_t)0;
  };
  const int nmatches = middle(classify, occ, assigned);
  assignFromSources(CurrentFrame, assigned, LastFrame.mvpMapPoints);
  return nmatches;
}
// SearchByProjection(Cur, pKF, sAlreadyFound, th, ORBdist).  occ[n] zeroed and assigned[n] are the caller's (std::vector in
// the host form, page-locked in the GPU form); middle(classify) -> nmatches.
template <class FrameT, class PointsT, class SetT, class Middle>
inline int searchByProjectionKeyFrameImpl(FrameT& CurrentFrame, const PointsT& vpMPs, const SetT& sAlreadyFound, uint8_t* occ,
                                          const int32_t* assigned, Middle middle) {
  const int n = (int)CurrentFrame.mvKeysUn.size();
  for (int i = 0; i < n; i++)
    if (CurrentFrame.mvpMapPoints[i]) occ[i] = 1;                         // :1493-1494
  auto classify = [&](int i) -> uint8_t {
    auto* pMP = vpMPs[i];
    if (!pMP) return ORBFE_MP_SKIP;
    if (pMP->isBad()) return ORBFE_MP_BAD;                                // :1447
    return sAlreadyFound.count(pMP) ? (uint8_t)ORBFE_MP_SKIP : (uint8_t)0;
  };
  const int nmatches = middle(classify);
  assignFromSources(CurrentFrame, assigned, vpMPs);
  return nmatches;
}
}  // namespace detail

// int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th)   (ORBmatcher.cc:1292-1423)
template <class Ops = detail::RestatedOps, class FrameT>
inline int SearchByProjection(MatcherContext& ctx, bool mbCheckOrientation, FrameT& CurrentFrame, const FrameT& LastFrame,
                              const float th) {
  return detail::searchByProjectionLastFrameImpl(ctx, CurrentFrame, LastFrame, [&](auto classify, const uint8_t* occ, int32_t* assigned) {
    float Rcw[9], tcw[3];
    detail::poseRt(CurrentFrame.mTcw, Rcw, tcw);
    const int n = (int)CurrentFrame.mvKeysUn.size(), ns = (int)LastFrame.N;
    // page-locked as well; valid / flags / levels zeroed
    float* uv = ctx.scratch<float>(3, (size_t)ns * 2, true);
    float* ang = ctx.scratch<float>(4, ns, true);
    int32_t* lvl = ctx.scratch<int32_t>(5, ns, true);
    uint8_t* valid = ctx.scratch<uint8_t>(7, ns, true);
    uint8_t* flags = ctx.scratch<uint8_t>(1, ns, true);
    uint8_t* sdesc = ctx.scratch<uint8_t>(2, (size_t)ns * 32, false);
    for (int i = 0; i < n; i++) assigned[i] = -1;
    // (locals: the byte stores below could alias what the closure refers to, and every source would load it again)
    const auto fx = CurrentFrame.fx, fy = CurrentFrame.fy, cx = CurrentFrame.cx, cy = CurrentFrame.cy;
    const auto minX = CurrentFrame.mnMinX, maxX = CurrentFrame.mnMaxX, minY = CurrentFrame.mnMinY, maxY = CurrentFrame.mnMaxY;
    for (int i = 0; i < ns; i++) {
      if (classify(i)) continue;
      auto* pMP = LastFrame.mvpMapPoints[i];
      float x3Dw[3], x3Dc[3];
      detail::vec3(pMP->GetWorldPos(), x3Dw);
      Ops::gemm3(Rcw, x3Dw, 1.0, tcw, 1.0, x3Dc);                       // Rcw*x3Dw+tcw
      const float xc = x3Dc[0], yc = x3Dc[1];
      const float invzc = (float)(1.0 / x3Dc[2]);
      if (invzc < 0) continue;
      const float u = fx * xc * invzc + cx;
      const float v = fy * yc * invzc + cy;
      if (u < minX || u > maxX) continue;
      if (v < minY || v > maxY) continue;
      uv[2 * i] = u; uv[2 * i + 1] = v;
      lvl[i] = LastFrame.mvKeys[i].octave;                              // nLastOctave
      ang[i] = LastFrame.mvKeysUn[i].angle;
      flags[i] = pMP->Observations() > 0 ? ORBFE_MP_OBSERVED : 0;
      const auto d = pMP->GetDescriptor();
      std::memcpy(&sdesc[(size_t)i * 32], d.data, 32);
      valid[i] = 1;
    }
    return detail::searchProjectedUv(ctx, CurrentFrame, occ, uv, lvl, ang, flags, valid, sdesc, ns, th, /*TH_HIGH*/ 100,
                                     /*skip_any_occupied*/ 0, mbCheckOrientation, assigned);
  });
}
template <class Ops = detail::RestatedOps, class FrameT, class GeometryFn>
inline int SearchByProjectionLastFrame(MatcherContext& ctx, bool mbCheckOrientation, FrameT& CurrentFrame, const FrameT& LastFrame,
                                       const float th, GeometryFn geometry) {
  const int ns = (int)LastFrame.mvKeysUn.size();
  orbfe_frame* src = ctx.resident(LastFrame, 0);
  orbfe_frame* cur = src ? ctx.resident(CurrentFrame, 0) : nullptr;   // (never evicts src: the two most recent frames stay)
  if (!src || !cur || ns != (int)LastFrame.mvpMapPoints.size()) return SearchByProjection<Ops>(ctx, mbCheckOrientation, CurrentFrame, LastFrame, th);
  return detail::searchByProjectionLastFrameImpl(ctx, CurrentFrame, LastFrame, [&](auto classify, const uint8_t* occ, int32_t* assigned) {
    auto flag = [&](int i) -> uint8_t {
      if (const uint8_t f = classify(i)) return f;
      return LastFrame.mvpMapPoints[i]->Observations() > 0 ? (uint8_t)ORBFE_MP_OBSERVED : (uint8_t)0;
    };
    return detail::searchSourcesFrame<Ops>(ctx, cur, src, CurrentFrame, ORBFE_SRC_LAST_FRAME, LastFrame.mvpMapPoints, ns, flag, geometry,
                                           occ, th, /*TH_HIGH*/ 100, mbCheckOrientation, assigned);
  });
}

// int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound,
//                                    const float th, const int ORBdist)   (ORBmatcher.cc:1425-1552)
template <class Ops = detail::RestatedOps, class FrameT, class KeyFrameT, class SetT>
inline int SearchByProjection(MatcherContext& ctx, bool mbCheckOrientation, FrameT& CurrentFrame, KeyFrameT* pKF,
                              const SetT& sAlreadyFound, const float th, const int ORBdist) {
  float Rcw[9], tcw[3], Ow[3];
  detail::poseRt(CurrentFrame.mTcw, Rcw, tcw);
  Ops::gemmT3(Rcw, tcw, -1.0, Ow);                                       // -Rcw.t()*tcw
  const auto vpMPs = pKF->GetMapPointMatches();
  const int n = (int)CurrentFrame.mvKeysUn.size(), ns = (int)vpMPs.size();
  std::vector<float> uv((size_t)ns * 2, 0.f), ang(ns, 0.f);
  std::vector<int32_t> lvl(ns, 0), assigned(n > 0 ? n : 1, -1);
  std::vector<uint8_t> valid(ns, 0), flags(ns, 0), sdesc((size_t)ns * 32, 0), occ(n > 0 ? n : 1, 0);
  return detail::searchByProjectionKeyFrameImpl(CurrentFrame, vpMPs, sAlreadyFound, occ.data(), assigned.data(), [&](auto classify) {
    for (int i = 0; i < ns; i++) {
      if (classify(i)) continue;
      auto* pMP = vpMPs[i];
      float x3Dw[3], x3Dc[3];
      detail::vec3(pMP->GetWorldPos(), x3Dw);
      Ops::gemm3(Rcw, x3Dw, 1.0, tcw, 1.0, x3Dc);
      const float xc = x3Dc[0], yc = x3Dc[1];
      const float invzc = (float)(1.0 / x3Dc[2]);
      const float u = CurrentFrame.fx * xc * invzc + CurrentFrame.cx;
      const float v = CurrentFrame.fy * yc * invzc + CurrentFrame.cy;
      if (u < CurrentFrame.mnMinX || u > CurrentFrame.mnMaxX) continue;
      if (v < CurrentFrame.mnMinY || v > CurrentFrame.mnMaxY) continue;
      const float PO[3] = {x3Dw[0] - Ow[0], x3Dw[1] - Ow[1], x3Dw[2] - Ow[2]};
      const float dist3D = (float)Ops::norm3(PO);
      const float maxDistance = pMP->GetMaxDistanceInvariance(), minDistance = pMP->GetMinDistanceInvariance();
      if (dist3D < minDistance || dist3D > maxDistance) continue;
      uv[2 * i] = u; uv[2 * i + 1] = v;
      lvl[i] = pMP->PredictScale(dist3D, CurrentFrame.mfLogScaleFactor);
      ang[i] = pKF->mvKeysUn[i].angle;
      const auto d = pMP->GetDescriptor();
      std::memcpy(&sdesc[(size_t)i * 32], d.data, 32);
      valid[i] = 1;
    }
    return detail::searchProjectedUv(ctx, CurrentFrame, occ.data(), uv.data(), lvl.data(), ang.data(), flags.data(), valid.data(),
                                     sdesc.data(), ns, th, ORBdist, /*skip_any_occupied*/ 1, mbCheckOrientation, assigned.data());
  });
}
template <class Ops = detail::RestatedOps, class FrameT, class KeyFrameT, class SetT, class GeometryFn>
inline int SearchByProjectionKeyFrame(MatcherContext& ctx, bool mbCheckOrientation, FrameT& CurrentFrame, KeyFrameT* pKF,
                                      const SetT& sAlreadyFound, const float th, const int ORBdist, GeometryFn geometry) {
  const auto vpMPs = pKF->GetMapPointMatches();
  const int n = (int)CurrentFrame.mvKeysUn.size(), ns = (int)vpMPs.size();
  orbfe_frame* src = ns == (int)pKF->mvKeysUn.size() ? ctx.resident(*pKF, 1) : nullptr;
  orbfe_frame* cur = src ? ctx.resident(CurrentFrame, 0) : nullptr;
  if (!src || !cur) return SearchByProjection<Ops>(ctx, mbCheckOrientation, CurrentFrame, pKF, sAlreadyFound, th, ORBdist);
  uint8_t* occ = ctx.scratch<uint8_t>(0, n, true);
  int32_t* assigned = ctx.scratch<int32_t>(6, n, false);
  return detail::searchByProjectionKeyFrameImpl(CurrentFrame, vpMPs, sAlreadyFound, occ, assigned, [&](auto classify) {
    return detail::searchSourcesFrame<Ops>(ctx, cur, src, CurrentFrame, ORBFE_SRC_KEYFRAME, vpMPs, ns, classify, geometry, occ, th,
                                           ORBdist, mbCheckOrientation, assigned);
  });
}

// ---- the four keyframe-side searches.  Their middles hand back bestIdx[ns]: the keypoint of the keyframe each source
// selected, -1 for none -- and for every source that was not projected.
namespace detail {
template <class KeyFrameT>
inline void keyFrameProjection(KeyFrameT* intr, KeyFrameT* to, const float R[9], const float t[3], const float* Ow,
                               OrbfeKeyFrameProjection& P) {
  std::memset(&P, 0, sizeof P);
  std::memcpy(P.R, R, sizeof P.R);
  std::memcpy(P.t, t, sizeof P.t);
  if (Ow) std::memcpy(P.Ow, Ow, sizeof P.Ow);
  P.fx = intr->fx; P.fy = intr->fy; P.cx = intr->cx; P.cy = intr->cy;
  P.logScaleFactor = to->mfLogScaleFactor;
}
template <class KeyFrameT>
inline bool fusedKeyFrameLevels(KeyFrameT* pKF, bool chi2) {
  const size_t nl = pKF->mvScaleFactors.size();
  return nl >= 1 && nl <= 32 && (!chi2 || pKF->mvInvLevelSigma2.size() == nl);
}
// the GPU middle of the keyframe-side searches: projection + windows + best match of the MapPoints pts into the resident
// keyframe rf; returns bestIdx[pts.size()] (page-locked, valid until the next search through ctx), the matches in *nmatches
template <class KeyFrameT, class PointsT, class Classify, class GeometryFn>
inline const int32_t* searchSourcesKeyFrame(MatcherContext& ctx, orbfe_frame* rf, KeyFrameT* to, const OrbfeKeyFrameProjection& P,
                                            const PointsT& pts, Classify classify, GeometryFn& geometry, float th,
                                            const uint8_t* kp_skip, int claim, bool chi2, int max_dist, int* nmatches = nullptr) {
  const int ns = (int)pts.size();
  uint8_t* flags;
  int32_t* rows;
  sourceRows(ctx, pts, ns, classify, geometry, flags, rows);
  int32_t* bestIdx = ctx.scratch<int32_t>(5, ns, false);
  int nm = 0, nValid = 0;
  check(orbfe_search_projected_keyframe_frame(ctx.get(), rf, ctx.localMap(), &P, rows, flags, ns, to->mvScaleFactors.data(),
                                              (int)to->mvScaleFactors.size(), th, kp_skip, claim,
                                              chi2 ? to->mvInvLevelSigma2.data() : nullptr, 5.99, max_dist, nullptr, nullptr, nullptr,
                                              bestIdx, nullptr, &nm, &nValid));
  if (nmatches) *nmatches = nm;
  return bestIdx;
}

// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th).  middle(classify, Rcw, tcw, Ow, nmatches) -> bestIdx
template <class Ops, class MatT, class MapPointT, class Middle>
inline int searchByProjectionScwImpl(const MatT& Scw, const std::vector<MapPointT*>& vpPoints, std::vector<MapPointT*>& vpMatched,
                                     Middle middle) {
  float Rcw[9], tcw[3], Ow[3];
  decomposeScw<Ops>(Scw, Rcw, tcw, Ow);
  std::vector<MapPointT*> found(vpMatched.begin(), vpMatched.end());     // spAlreadyFound (:301-302)
  std::sort(found.begin(), found.end());
  auto classify = [&](int i) -> uint8_t {
    MapPointT* pMP = vpPoints[i];
    if (pMP->isBad()) return ORBFE_MP_BAD;                                // :312-313
    return std::binary_search(found.begin(), found.end(), pMP) ? (uint8_t)ORBFE_MP_SKIP : (uint8_t)0;
  };
  int nmatches = 0;
  const int32_t* bestIdx = middle(classify, Rcw, tcw, Ow, nmatches);
  for (size_t i = 0; i < vpPoints.size(); i++)
    if (bestIdx[i] >= 0) vpMatched[bestIdx[i]] = vpPoints[i];
  return nmatches;
}

// Fuse(pKF, vpMapPoints, th).  middle(Rcw, tcw, Ow) -> bestIdx.  Which keypoint a MapPoint selects depends only on the
// keyframe's keypoints and the point itself, so all windows are searched in one GPU call; the reference's loop is then
// replayed IN ORDER with its live checks (isBad / IsInKeyFrame change as earlier points are replaced or added).  vpMapPoints
// holds distinct points, as the reference's callers guarantee (LocalMapping::SearchInNeighbors marks candidates with
// mnFuseCandidateForKF).  There is no classify here: the host middle projects every non-null point and leaves isBad /
// IsInKeyFrame to the replay, the GPU middle takes them at entry as well (see FuseKeyFrame).
template <class KeyFrameT, class MapPointT, class Middle>
inline int fuseImpl(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, Middle middle) {
  float Rcw[9], tcw[3], Ow[3];
  mat33(pKF->GetRotation(), Rcw);
  vec3(pKF->GetTranslation(), tcw);
  vec3(pKF->GetCameraCenter(), Ow);
  const int32_t* bestIdx = middle(Rcw, tcw, Ow);
  int nFused = 0;
  for (size_t i = 0; i < vpMapPoints.size(); i++) {
    MapPointT* pMP = vpMapPoints[i];
    if (!pMP) continue;
    if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
    if (bestIdx[i] < 0) continue;   // no keypoint selected, or not projected (a source that is not valid keeps bestIdx == -1)
    const int best = bestIdx[i];
    MapPointT* pMPinKF = pKF->GetMapPoint(best);
    if (pMPinKF) {
      if (!pMPinKF->isBad()) {
        if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
        else pMPinKF->Replace(pMP);
      }
    } else {
      pMP->AddObservation(pKF, best);
      pKF->AddMapPoint(pMP, best);
    }
    nFused++;
  }
  return nFused;
}

// Fuse(pKF, Scw, vpPoints, th, vpReplacePoint).  middle(classify, Rcw, tcw, Ow) -> bestIdx
template <class Ops, class KeyFrameT, class MatT, class MapPointT, class Middle>
inline int fuseScwImpl(KeyFrameT* pKF, const MatT& Scw, const std::vector<MapPointT*>& vpPoints,
                       std::vector<MapPointT*>& vpReplacePoint, Middle middle) {
  float Rcw[9], tcw[3], Ow[3];
  decomposeScw<Ops>(Scw, Rcw, tcw, Ow);
  const auto spAlreadyFound = pKF->GetMapPoints();
  auto classify = [&](int i) -> uint8_t {
    MapPointT* pMP = vpPoints[i];
    if (pMP->isBad()) return ORBFE_MP_BAD;                                // :968-969
    return spAlreadyFound.count(pMP) ? (uint8_t)ORBFE_MP_SKIP : (uint8_t)0;
  };
  const int32_t* bestIdx = middle(classify, Rcw, tcw, Ow);
  int nFused = 0;
  for (size_t i = 0; i < vpPoints.size(); i++) {
    if (bestIdx[i] < 0) continue;   // (as in fuseImpl)
    MapPointT* pMP = vpPoints[i];
    const int best = bestIdx[i];
    MapPointT* pMPinKF = pKF->GetMapPoint(best);     // live: an earlier point of this call may have been added here
    if (pMPinKF) {
      if (!pMPinKF->isBad()) vpReplacePoint[i] = pMPinKF;
    } else {
      pMP->AddObservation(pKF, best);
      pKF->AddMapPoint(pMP, best);
    }
    nFused++;
  }
  return nFused;
}

// SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th).  One direction: the points `pts` of the keyframe with pose
// (Rfw, tfw) through (sR, tt) into `to`; middle(classify, pts, Rfw, tfw, sR, tt, to, vnMatch) fills vnMatch[pts.size()].
template <class Ops, class KeyFrameT, class MatT, class MapPointT, class Middle>
inline int searchBySim3Impl(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12, const float& s12,
                            const MatT& R12m, const MatT& t12m, Middle middle) {
  float R1w[9], t1w[3], R2w[9], t2w[3], R12[9], t12[3], sR12[9], sR21[9], R12t[9], t21[3];
  mat33(pKF1->GetRotation(), R1w); vec3(pKF1->GetTranslation(), t1w);
  mat33(pKF2->GetRotation(), R2w); vec3(pKF2->GetTranslation(), t2w);
  mat33(R12m, R12); vec3(t12m, t12);
  Ops::scale(R12, 9, (double)s12, sR12);                                  // s12*R12
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R12t[3 * r + c] = R12[3 * c + r];
  Ops::scale(R12t, 9, 1.0 / (double)s12, sR21);                           // (1.0/s12)*R12.t()
  Ops::gemm3(sR21, t12, -1.0, nullptr, 0.0, t21);                         // -sR21*t12
  const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
  const int N1 = (int)vpMapPoints1.size(), N2 = (int)vpMapPoints2.size();
  std::vector<bool> vbAlreadyMatched1(N1, false), vbAlreadyMatched2(N2, false);
  for (int i = 0; i < N1; i++) {
    MapPointT* pMP = vpMatches12[i];
    if (pMP) {
      vbAlreadyMatched1[i] = true;
      const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
      if (idx2 >= 0 && idx2 < N2) vbAlreadyMatched2[idx2] = true;
    }
  }
  auto direction = [&](const std::vector<MapPointT*>& pts, const std::vector<bool>& already, const float* Rfw, const float* tfw,
                       const float* sR, const float* tt, KeyFrameT* to, std::vector<int>& vnMatch) {
    auto classify = [&](int i) -> uint8_t {
      MapPointT* pMP = pts[i];
      if (!pMP || already[i]) return ORBFE_MP_SKIP;
      return pMP->isBad() ? (uint8_t)ORBFE_MP_BAD : (uint8_t)0;
    };
    middle(classify, pts, Rfw, tfw, sR, tt, to, vnMatch);
  };
  std::vector<int> vnMatch1, vnMatch2;
  direction(vpMapPoints1, vbAlreadyMatched1, R1w, t1w, sR21, t21, pKF2, vnMatch1);
  direction(vpMapPoints2, vbAlreadyMatched2, R2w, t2w, sR12, t12, pKF1, vnMatch2);
  int nFound = 0;
  for (int i1 = 0; i1 < N1; i1++) {
    const int idx2 = vnMatch1[i1];
    if (idx2 >= 0) {
      const int idx1 = vnMatch2[idx2];
      if (idx1 == i1) { vpMatches12[i1] = vpMapPoints2[idx2]; nFound++; }
    }
  }
  return nFound;
}
}  // namespace detail

// int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
//                                    vector<MapPoint*>& vpMatched, int th)   (ORBmatcher.cc:285-398)
template <class Ops = detail::RestatedOps, class KeyFrameT, class MatT, class MapPointT>
inline int SearchByProjection(MatcherContext& ctx, KeyFrameT* pKF, const MatT& Scw, const std::vector<MapPointT*>& vpPoints,
                              std::vector<MapPointT*>& vpMatched, int th) {
  detail::ProjectedSources S(vpPoints.size());
  std::vector<uint8_t> skip(vpMatched.size() ? vpMatched.size() : 1, 0);
  return detail::searchByProjectionScwImpl<Ops>(Scw, vpPoints, vpMatched, [&](auto classify, const float* Rcw, const float* tcw,
                                                                              const float* Ow, int& nmatches) {
    for (size_t i = 0; i < vpPoints.size(); i++)
      if (!classify((int)i)) detail::projectIntoKeyFrame<Ops>(pKF, vpPoints[i], Rcw, tcw, Ow, (float)th, /*invz = 1/z in float*/ false, S, i);
    for (size_t i = 0; i < vpMatched.size(); i++) skip[i] = vpMatched[i] ? 1 : 0;   // :366-367
    nmatches = detail::searchProjected(ctx, pKF, S, skip.data(), /*claim*/ 1, /*chi2*/ false, /*TH_LOW*/ 50);
    return S.bestIdx.data();
  });
}
template <class Ops = detail::RestatedOps, class KeyFrameT, class MatT, class MapPointT, class GeometryFn>
inline int SearchByProjectionScw(MatcherContext& ctx, KeyFrameT* pKF, const MatT& Scw, const std::vector<MapPointT*>& vpPoints,
                                 std::vector<MapPointT*>& vpMatched, int th, GeometryFn geometry) {
  orbfe_frame* rf = detail::fusedKeyFrameLevels(pKF, false) ? ctx.resident(*pKF, 1) : nullptr;
  if (!rf) return SearchByProjection<Ops>(ctx, pKF, Scw, vpPoints, vpMatched, th);
  return detail::searchByProjectionScwImpl<Ops>(Scw, vpPoints, vpMatched, [&](auto classify, const float* Rcw, const float* tcw,
                                                                              const float* Ow, int& nmatches) {
    uint8_t* skip = ctx.scratch<uint8_t>(0, vpMatched.size(), true);
    for (size_t i = 0; i < vpMatched.size(); i++) skip[i] = vpMatched[i] ? 1 : 0;   // :366-367
    OrbfeKeyFrameProjection P;
    detail::keyFrameProjection(pKF, pKF, Rcw, tcw, Ow, P);
    P.invz_in_double = 0; P.check_viewing_angle = 1;
    return detail::searchSourcesKeyFrame(ctx, rf, pKF, P, vpPoints, classify, geometry, (float)th, skip, /*claim*/ 1, false, /*TH_LOW*/ 50,
                                         &nmatches);
  });
}

// int ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th)   (ORBmatcher.cc:806-939)
template <class Ops = detail::RestatedOps, class KeyFrameT, class MapPointT>
inline int Fuse(MatcherContext& ctx, KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const float th) {
  detail::ProjectedSources S(vpMapPoints.size());
  return detail::fuseImpl(pKF, vpMapPoints, [&](const float* Rcw, const float* tcw, const float* Ow) {
    for (size_t i = 0; i < vpMapPoints.size(); i++)
      if (vpMapPoints[i]) detail::projectIntoKeyFrame<Ops>(pKF, vpMapPoints[i], Rcw, tcw, Ow, th, false, S, i);
    detail::searchProjected(ctx, pKF, S, nullptr, 0, /*chi2 gate :896-903*/ true, /*TH_LOW*/ 50);
    return S.bestIdx.data();
  });
}
// The GPU middle's flags are taken at entry, which is exact: a point that is bad stays bad, and a point that sits in the
// keyframe at entry can only leave it by being Replace()d, which makes it bad -- the reference's live check (:822-823) skips it
// either way.  The replay keeps the live checks for points that change DURING the call.
template <class Ops = detail::RestatedOps, class KeyFrameT, class MapPointT, class GeometryFn>
inline int FuseKeyFrame(MatcherContext& ctx, KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const float th,
                        GeometryFn geometry) {
  orbfe_frame* rf = detail::fusedKeyFrameLevels(pKF, true) ? ctx.resident(*pKF, 1) : nullptr;
  if (!rf) return Fuse<Ops>(ctx, pKF, vpMapPoints, th);
  return detail::fuseImpl(pKF, vpMapPoints, [&](const float* Rcw, const float* tcw, const float* Ow) {
    auto classify = [&](int i) -> uint8_t {
      MapPointT* pMP = vpMapPoints[i];
      if (!pMP) return ORBFE_MP_SKIP;
      if (pMP->isBad()) return ORBFE_MP_BAD;
      return pMP->IsInKeyFrame(pKF) ? (uint8_t)ORBFE_MP_SKIP : (uint8_t)0;
    };
    OrbfeKeyFrameProjection P;
    detail::keyFrameProjection(pKF, pKF, Rcw, tcw, Ow, P);
    P.invz_in_double = 0; P.check_viewing_angle = 1;
    return detail::searchSourcesKeyFrame(ctx, rf, pKF, P, vpMapPoints, classify, geometry, th, nullptr, 0, /*chi2 gate :896-903*/ true,
                                         /*TH_LOW*/ 50);
  });
}

// int ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th,
//                      vector<MapPoint*>& vpReplacePoint)   (ORBmatcher.cc:941-1064)
template <class Ops = detail::RestatedOps, class KeyFrameT, class MatT, class MapPointT>
inline int Fuse(MatcherContext& ctx, KeyFrameT* pKF, const MatT& Scw, const std::vector<MapPointT*>& vpPoints, float th,
                std::vector<MapPointT*>& vpReplacePoint) {
  detail::ProjectedSources S(vpPoints.size());
  return detail::fuseScwImpl<Ops>(pKF, Scw, vpPoints, vpReplacePoint, [&](auto classify, const float* Rcw, const float* tcw, const float* Ow) {
    for (size_t i = 0; i < vpPoints.size(); i++)
      if (!classify((int)i)) detail::projectIntoKeyFrame<Ops>(pKF, vpPoints[i], Rcw, tcw, Ow, th, /*invz = 1.0/z*/ true, S, i);
    detail::searchProjected(ctx, pKF, S, nullptr, 0, false, /*TH_LOW*/ 50);
    return S.bestIdx.data();
  });
}
template <class Ops = detail::RestatedOps, class KeyFrameT, class MatT, class MapPointT, class GeometryFn>
inline int FuseScw(MatcherContext& ctx, KeyFrameT* pKF, const MatT& Scw, const std::vector<MapPointT*>& vpPoints, float th,
                   std::vector<MapPointT*>& vpReplacePoint, GeometryFn geometry) {
  orbfe_frame* rf = detail::fusedKeyFrameLevels(pKF, false) ? ctx.resident(*pKF, 1) : nullptr;
  if (!rf) return Fuse<Ops>(ctx, pKF, Scw, vpPoints, th, vpReplacePoint);
  return detail::fuseScwImpl<Ops>(pKF, Scw, vpPoints, vpReplacePoint, [&](auto classify, const float* Rcw, const float* tcw, const float* Ow) {
    OrbfeKeyFrameProjection P;
    detail::keyFrameProjection(pKF, pKF, Rcw, tcw, Ow, P);
    P.invz_in_double = 1; P.check_viewing_angle = 1;
    return detail::searchSourcesKeyFrame(ctx, rf, pKF, P, vpPoints, classify, geometry, th, nullptr, 0, false, /*TH_LOW*/ 50);
  });
}

// int ORBmatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, const float& s12,
//                              const cv::Mat& R12, const cv::Mat& t12, const float th)   (ORBmatcher.cc:1066-1290):
// one search per direction, then the vnMatch agreement on the host.
template <class Ops = detail::RestatedOps, class KeyFrameT, class MatT, class MapPointT>
inline int SearchBySim3(MatcherContext& ctx, KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12,
                        const float& s12, const MatT& R12m, const MatT& t12m, const float th) {
  const float fx = pKF1->fx, fy = pKF1->fy, cx = pKF1->cx, cy = pKF1->cy;
  return detail::searchBySim3Impl<Ops>(pKF1, pKF2, vpMatches12, s12, R12m, t12m, [&](auto classify, const std::vector<MapPointT*>& pts,
                                                                                     const float* Rfw, const float* tfw, const float* sR,
                                                                                     const float* tt, KeyFrameT* to, std::vector<int>& vnMatch) {
    detail::ProjectedSources S(pts.size());
    for (size_t i = 0; i < pts.size(); i++) {
      if (classify((int)i)) continue;
      MapPointT* pMP = pts[i];
      float p3Dw[3], pa[3], pb[3];
      detail::vec3(pMP->GetWorldPos(), p3Dw);
      Ops::gemm3(Rfw, p3Dw, 1.0, tfw, 1.0, pa);
      Ops::gemm3(sR, pa, 1.0, tt, 1.0, pb);
      if (pb[2] < 0.0) continue;
      const float invz = (float)(1.0 / pb[2]);
      const float x = pb[0] * invz, y = pb[1] * invz;
      const float u = fx * x + cx, v = fy * y + cy;                       // pKF1's intrinsics in both directions (:1069-1072)
      if (!to->IsInImage(u, v)) continue;
      const float maxDistance = pMP->GetMaxDistanceInvariance(), minDistance = pMP->GetMinDistanceInvariance();
      const float dist3D = (float)Ops::norm3(pb);
      if (dist3D < minDistance || dist3D > maxDistance) continue;
      const int nPredictedLevel = pMP->PredictScale(dist3D, to->mfLogScaleFactor);
      S.uv[2 * i] = u; S.uv[2 * i + 1] = v;
      S.level[i] = nPredictedLevel;
      S.radius[i] = th * to->mvScaleFactors[nPredictedLevel];
      const auto d = pMP->GetDescriptor();
      std::memcpy(&S.desc[32 * i], d.data, 32);
      S.valid[i] = 1;
    }
    detail::searchProjected(ctx, to, S, nullptr, 0, false, /*TH_HIGH*/ 100);
    vnMatch.assign(S.bestIdx.begin(), S.bestIdx.end());
  });
}
template <class Ops = detail::RestatedOps, class KeyFrameT, class MatT, class MapPointT, class GeometryFn>
inline int SearchBySim3Device(MatcherContext& ctx, KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12,
                              const float& s12, const MatT& R12m, const MatT& t12m, const float th, GeometryFn geometry) {
  const bool levels = detail::fusedKeyFrameLevels(pKF1, false) && detail::fusedKeyFrameLevels(pKF2, false);
  orbfe_frame* rf2 = levels ? ctx.resident(*pKF2, 1) : nullptr;
  orbfe_frame* rf1 = rf2 ? ctx.resident(*pKF1, 1) : nullptr;   // (never evicts rf2: the two most recent frames stay)
  if (!rf1 || !rf2) return SearchBySim3<Ops>(ctx, pKF1, pKF2, vpMatches12, s12, R12m, t12m, th);
  return detail::searchBySim3Impl<Ops>(pKF1, pKF2, vpMatches12, s12, R12m, t12m, [&](auto classify, const std::vector<MapPointT*>& pts,
                                                                                     const float* Rfw, const float* tfw, const float* sR,
                                                                                     const float* tt, KeyFrameT* to, std::vector<int>& vnMatch) {
    OrbfeKeyFrameProjection P;
    detail::keyFrameProjection(pKF1, to, Rfw, tfw, nullptr, P);           // pKF1's intrinsics in both directions (:1069-1072)
    P.has_second = 1;
    std::memcpy(P.sR, sR, sizeof P.sR);
    std::memcpy(P.t2, tt, sizeof P.t2);
    P.invz_in_double = 1; P.check_viewing_angle = 0; P.distance_from_camera_point = 1;
    const int32_t* bestIdx = detail::searchSourcesKeyFrame(ctx, to == pKF1 ? rf1 : rf2, to, P, pts, classify, geometry, th, nullptr, 0,
                                                           false, /*TH_HIGH*/ 100);
    vnMatch.assign(bestIdx, bestIdx + pts.size());
  });
}

// void Frame::UndistortKeyPoints()   (Frame.cc:286-320) and void Frame::ComputeImageBounds(const cv::Mat& imLeft)
// (:322-353), both camera models (camaraModo 0 = pinhole with mDistCoef through cv::undistortPoints, 1 = os1's
// equidistant fisheye).  K = {fx, fy, cx, cy}; dist = mDistCoef (4, 5 or 8 floats; ignored for mode 1).
template <class KeyPointT>
inline void UndistortKeyPoints(const std::vector<KeyPointT>& mvKeys, std::vector<KeyPointT>& mvKeysUn, int camaraModo, float fx,
                               float fy, float cx, float cy, const float* dist, int ndist) {
  if (camaraModo == 0 && (ndist == 0 || dist[0] == 0.0)) { mvKeysUn = mvKeys; return; }
  static_assert(sizeof(KeyPointT) == sizeof(OrbfeKeyPoint), "KeyPointT must match cv::KeyPoint's layout");
  const int N = (int)mvKeys.size();
  std::vector<float> mat((size_t)N * 2);
  for (int i = 0; i < N; i++) {
    OrbfeKeyPoint k;
    std::memcpy(&k, &mvKeys[i], sizeof k);
    mat[2 * i] = k.x; mat[2 * i + 1] = k.y;
  }
  if (camaraModo) check(orbfe_undistort_equidistant(mat.data(), N, fx, fy, cx, cy));
  else check(orbfe_undistort_pinhole(mat.data(), N, fx, fy, cx, cy, dist, ndist));
  mvKeysUn.resize(N);
  for (int i = 0; i < N; i++) {
    KeyPointT kp = mvKeys[i];
    std::memcpy(static_cast<void*>(&kp), &mat[2 * i], 2 * sizeof(float));   // kp.pt = (x, y): the first two floats of cv::KeyPoint
    mvKeysUn[i] = kp;
  }
}
inline void ComputeImageBounds(int cols, int rows, int camaraModo, float fx, float fy, float cx, float cy, const float* dist,
                               int ndist, float& mnMinX, float& mnMaxX, float& mnMinY, float& mnMaxY) {
  float b[4];
  check(orbfe_compute_image_bounds(cols, rows, camaraModo, fx, fy, cx, cy, dist, ndist, b));
  mnMinX = b[0]; mnMaxX = b[1]; mnMinY = b[2]; mnMaxY = b[3];
}

// ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) as far as the path uses it: loaded from the
// fork's binary vocabulary file (TemplatedVocabulary.h:1563-1640), resident in HBM.
class Vocabulary {
 public:
  explicit Vocabulary(int device = 0) : device_(device) {}
  ~Vocabulary() { orbfe_vocabulary_destroy(v_); }
  Vocabulary(const Vocabulary&) = delete;
  Vocabulary& operator=(const Vocabulary&) = delete;
  // bool loadFromBinaryFile(const std::string& filename)
  bool loadFromBinaryFile(const std::string& filename) {
    FILE* f = std::fopen(filename.c_str(), "rb");
    if (!f) return false;
    std::vector<uint8_t> image;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) image.insert(image.end(), buf, buf + got);
    std::fclose(f);
    orbfe_vocabulary* nv = nullptr;
    if (orbfe_vocabulary_create_from_image(device_, image.data(), image.size(), &nv) != ORBFE_OK) return false;
    orbfe_vocabulary_destroy(v_);
    v_ = nv;
    return true;
  }
  bool empty() const { return v_ == nullptr; }
  orbfe_vocabulary* get() const { return v_; }

  // void transform(const std::vector<TDescriptor>& features, BowVector& v, FeatureVector& fv, int levelsup) const
  // (TemplatedVocabulary.h:1136-1204) on the rows of a CV_8U N x 32 matrix.  BowVectorT / FeatureVectorT are the
  // DBoW2 map types (std::map<WordId, WordValue>, std::map<NodeId, std::vector<unsigned int>>).
  template <class MatT, class BowVectorT, class FeatureVectorT>
  void transform(const MatT& descriptors, int n, BowVectorT& v, FeatureVectorT& fv, int levelsup) {
    v.clear();
    fv.clear();
    if (!v_ || n == 0) return;
    std::vector<uint8_t> tmp;
    ids_.resize(n); vals_.resize(n); nodes_.resize(n); offs_.resize(n + 1); feats_.resize(n);
    int nw = 0, nn = 0;
    check(orbfe_bow_transform(v_, detail::packedDescriptors(descriptors, n, tmp), n, 0, levelsup, ids_.data(),
                              vals_.data(), &nw, nodes_.data(), offs_.data(), feats_.data(), &nn, nullptr, nullptr));
    for (int i = 0; i < nw; i++) v.insert(v.end(), typename BowVectorT::value_type(ids_[i], vals_[i]));
    for (int i = 0; i < nn; i++) {
      auto it = fv.insert(fv.end(), typename FeatureVectorT::value_type(nodes_[i], typename FeatureVectorT::mapped_type()));
      it->second.assign(feats_.begin() + offs_[i], feats_.begin() + offs_[i + 1]);
    }
  }

  // transform() for several descriptor sets in one submission (orbfe_bow_transform_batch): rows[s] = the n[s] packed 32-byte
  // rows of set s (host, page-locked or device memory), bow[s] / fv[s] = where its vectors go.  Each pair of vectors is what
  // transform() gives for that set alone.
  template <class BowVectorT, class FeatureVectorT>
  void transformBatch(const std::vector<const uint8_t*>& rows, const std::vector<int>& n, const std::vector<BowVectorT*>& bow,
                      const std::vector<FeatureVectorT*>& fv, int levelsup) {
    const size_t ns = rows.size();
    for (size_t s = 0; s < ns; s++) { bow[s]->clear(); fv[s]->clear(); }
    if (!v_ || ns == 0) return;
    size_t total = 0;
    for (size_t s = 0; s < ns; s++) total += (size_t)n[s];
    // one block per output array, set s at its prefix (fv_offsets: one entry more per set)
    ids_.resize(total + 1); vals_.resize(total + 1); nodes_.resize(total + 1); offs_.resize(total + ns); feats_.resize(total + 1);
    std::vector<uint32_t*> pi(ns), pn(ns), po(ns), pf(ns);
    std::vector<double*> pv(ns);
    std::vector<int> nw(ns, 0), nn(ns, 0);
    size_t at = 0;
    for (size_t s = 0; s < ns; s++) {
      pi[s] = ids_.data() + at; pv[s] = vals_.data() + at; pn[s] = nodes_.data() + at; pf[s] = feats_.data() + at;
      po[s] = offs_.data() + at + s;
      at += (size_t)n[s];
    }
    check(orbfe_bow_transform_batch(v_, levelsup, (int)ns, rows.data(), n.data(), n.data(), pi.data(), pv.data(), nw.data(), pn.data(),
                                    po.data(), pf.data(), nn.data(), nullptr, nullptr));
    for (size_t s = 0; s < ns; s++) {
      BowVectorT& v = *bow[s];
      FeatureVectorT& f = *fv[s];
      for (int i = 0; i < nw[s]; i++) v.insert(v.end(), typename BowVectorT::value_type(pi[s][i], pv[s][i]));
      for (int i = 0; i < nn[s]; i++) {
        auto it = f.insert(f.end(), typename FeatureVectorT::value_type(pn[s][i], typename FeatureVectorT::mapped_type()));
        it->second.assign(pf[s] + po[s][i], pf[s] + po[s][i + 1]);
      }
    }
  }

 private:
  int device_;
  orbfe_vocabulary* v_ = nullptr;
  std::vector<uint32_t> ids_, nodes_, offs_, feats_;
  std::vector<double> vals_;
};

// void Frame::ComputeBoW()   (Frame.cc:277-284); KeyFrame::ComputeBoW (KeyFrame.cc) is the same call.
template <class FrameT>
inline void ComputeBoW(Vocabulary& voc, FrameT& F) {
  if (F.mBowVec.empty()) voc.transform(F.mDescriptors, (int)F.mDescriptors.rows, F.mBowVec, F.mFeatVec, 4);
}

// KeyFrame::ComputeBoW for every keyframe of a loaded map (the loop of Osmap::rebuild, src/Osmap.cpp) in ONE submission.  The
// reference's guard `if(mBowVec.empty())` holds per keyframe: a keyframe that has its vectors keeps them and sends nothing.
// ctx (optional): a keyframe whose resident copy the context holds passes that copy's device rows; its descriptors do not
// cross PCIe again.  Every keyframe ends up with the vectors the one-keyframe overload gives it.
namespace detail {
template <class KeyFrameT>
inline void computeBoWBatch(Vocabulary& voc, const std::vector<KeyFrameT*>& vpKFs, MatcherContext* ctx) {
  typedef typename std::remove_reference<decltype(vpKFs[0]->mBowVec)>::type BowVectorT;
  typedef typename std::remove_reference<decltype(vpKFs[0]->mFeatVec)>::type FeatureVectorT;
  std::vector<const uint8_t*> rows;
  std::vector<int> n;
  std::vector<BowVectorT*> bow;
  std::vector<FeatureVectorT*> fv;
  std::vector<std::vector<uint8_t> > packed;   // keyframes whose cv::Mat rows are not contiguous
  packed.reserve(vpKFs.size());                // (the pointers handed out below must stay)
  for (KeyFrameT* pKF : vpKFs) {
    if (!pKF || !pKF->mBowVec.empty()) continue;
    const int nk = (int)pKF->mDescriptors.rows;
    const uint8_t* r = nullptr;
    if (nk > 0 && ctx)
      if (orbfe_frame* rf = ctx->residentIfHeld(*pKF)) r = orbfe_frame_descriptors_device(rf);
    if (!r) {
      packed.emplace_back();
      r = detail::packedDescriptors(pKF->mDescriptors, nk, packed.back());
    }
    rows.push_back(r); n.push_back(nk); bow.push_back(&pKF->mBowVec); fv.push_back(&pKF->mFeatVec);
  }
  voc.transformBatch(rows, n, bow, fv, 4);
}
}  // namespace detail
// (two overloads, so that a vector of keyframes never deduces as the FrameT of the one-frame form above)
template <class KeyFrameT>
inline void ComputeBoW(Vocabulary& voc, std::vector<KeyFrameT*>& vpKFs, MatcherContext* ctx = nullptr) {
  detail::computeBoWBatch(voc, vpKFs, ctx);
}
template <class KeyFrameT>
inline void ComputeBoW(Vocabulary& voc, const std::vector<KeyFrameT*>& vpKFs, MatcherContext* ctx = nullptr) {
  detail::computeBoWBatch(voc, vpKFs, ctx);
}

namespace detail {
template <class FeatureVectorT>
inline void flattenFeatureVector(const FeatureVectorT& fv, std::vector<uint32_t>& nodes, std::vector<uint32_t>& offs,
                                 std::vector<uint32_t>& feats) {
  nodes.clear(); offs.clear(); feats.clear();
  for (const auto& e : fv) {
    nodes.push_back((uint32_t)e.first);
    offs.push_back((uint32_t)feats.size());
    feats.insert(feats.end(), e.second.begin(), e.second.end());
  }
  offs.push_back((uint32_t)feats.size());
}
template <class KeyPointT>
inline void angles(const std::vector<KeyPointT>& k, std::vector<float>& a) {
  a.resize(k.size());
  for (size_t i = 0; i < k.size(); i++) a[i] = k[i].angle;
}
template <class MapPointT>
inline void validFlags(const std::vector<MapPointT*>& mps, std::vector<uint8_t>& valid) {
  valid.assign(mps.size(), 0);
  for (size_t i = 0; i < mps.size(); i++)
    if (mps[i] && !mps[i]->isBad()) valid[i] = 1;   // ORBmatcher.cc:191-196 / 553-557
}
}  // namespace detail

// int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)  (ORBmatcher.cc:154-283)
template <class KeyFrameT, class FrameT, class MapPointT>
inline int SearchByBoW(MatcherContext& ctx, float mfNNratio, bool mbCheckOrientation, KeyFrameT* pKF, FrameT& F,
                       std::vector<MapPointT*>& vpMapPointMatches) {
  const std::vector<MapPointT*> vpMapPointsKF = pKF->GetMapPointMatches();
  const int n1 = (int)vpMapPointsKF.size(), n2 = (int)F.N;
  vpMapPointMatches.assign(n2, static_cast<MapPointT*>(nullptr));
  std::vector<uint8_t> valid1, t1, t2;
  std::vector<float> a1, a2;
  std::vector<uint32_t> n1v, o1v, f1v, n2v, o2v, f2v;
  detail::validFlags(vpMapPointsKF, valid1);
  detail::angles(pKF->mvKeysUn, a1);
  detail::angles(F.mvKeys, a2);
  detail::flattenFeatureVector(pKF->mFeatVec, n1v, o1v, f1v);
  detail::flattenFeatureVector(F.mFeatVec, n2v, o2v, f2v);
  std::vector<int32_t> m12(n1 > 0 ? n1 : 1, -1);
  int nmatches = 0;
  check(orbfe_search_by_bow(ctx.get(), detail::descriptorRows(ctx, *pKF, 1, n1, t1), a1.data(), valid1.data(), n1,
                            n1v.data(), o1v.data(), f1v.data(), (int)n1v.size(),
                            detail::descriptorRows(ctx, F, 0, n2, t2), a2.data(), nullptr, n2, n2v.data(),
                            o2v.data(), f2v.data(), (int)n2v.size(), mfNNratio, mbCheckOrientation ? 1 : 0, 0, m12.data(),
                            &nmatches));
  for (int i = 0; i < n1; i++)
    if (m12[i] >= 0) vpMapPointMatches[m12[i]] = vpMapPointsKF[i];
  return nmatches;
}

// The SearchByBoW loop of Tracking::Relocalization (Tracking.cc:1005-1030) as ONE GPU submission: every candidate keyframe
// against the current frame.  vvpMapPointMatches[k] and the returned counts are what the per-keyframe function above gives;
// keyframes for which `skip[k]` is set (pKF->isBad(), :1010-1011) are left out (count 0, matches untouched).  Optional: an
// integration that keeps Tracking.cc unchanged simply keeps calling the per-keyframe member.
template <class KeyFrameT, class FrameT, class MapPointT>
inline std::vector<int> SearchByBoW(MatcherContext& ctx, float mfNNratio, bool mbCheckOrientation, const std::vector<KeyFrameT*>& vpKFs,
                                    const std::vector<bool>& skip, FrameT& F, std::vector<std::vector<MapPointT*> >& vvpMapPointMatches) {
  const int K = (int)vpKFs.size(), n2 = (int)F.N;
  std::vector<int> counts(K, 0);
  vvpMapPointMatches.resize(K);
  struct Side { std::vector<MapPointT*> mps; std::vector<uint8_t> valid, tmp; std::vector<float> ang; std::vector<uint32_t> nodes, offs, feats;
                std::vector<int32_t> m12; const uint8_t* desc = nullptr; };
  std::vector<Side> S(K);
  std::vector<const uint8_t*> d1, v1;
  std::vector<const float*> a1;
  std::vector<const uint32_t*> fn, fo, ff;
  std::vector<int> n1, nf, which;
  std::vector<int32_t*> out;
  for (int k = 0; k < K; k++) {
    if (k < (int)skip.size() && skip[k]) continue;
    Side& s = S[k];
    s.mps = vpKFs[k]->GetMapPointMatches();
    const int n = (int)s.mps.size();
    detail::validFlags(s.mps, s.valid);
    detail::angles(vpKFs[k]->mvKeysUn, s.ang);
    detail::flattenFeatureVector(vpKFs[k]->mFeatVec, s.nodes, s.offs, s.feats);
    s.desc = detail::packedDescriptors(vpKFs[k]->mDescriptors, n, s.tmp);
    s.m12.assign(n > 0 ? n : 1, -1);
    d1.push_back(s.desc); v1.push_back(s.valid.data()); a1.push_back(s.ang.data()); n1.push_back(n);
    fn.push_back(s.nodes.data()); fo.push_back(s.offs.data()); ff.push_back(s.feats.data()); nf.push_back((int)s.nodes.size());
    out.push_back(s.m12.data());
    which.push_back(k);
    vvpMapPointMatches[k].assign(n2, static_cast<MapPointT*>(nullptr));
  }
  if (which.empty()) return counts;
  std::vector<uint8_t> t2;
  std::vector<float> a2;
  std::vector<uint32_t> n2v, o2v, f2v;
  detail::angles(F.mvKeys, a2);
  detail::flattenFeatureVector(F.mFeatVec, n2v, o2v, f2v);
  std::vector<int> nm(which.size(), 0);
  check(orbfe_search_by_bow_batch(ctx.get(), (int)which.size(), d1.data(), a1.data(), v1.data(), n1.data(), fn.data(), fo.data(), ff.data(),
                                  nf.data(), detail::packedDescriptors(F.mDescriptors, n2, t2), a2.data(), nullptr, n2, n2v.data(), o2v.data(),
                                  f2v.data(), (int)n2v.size(), mfNNratio, mbCheckOrientation ? 1 : 0, 0, out.data(), nm.data()));
  for (size_t j = 0; j < which.size(); j++) {
    const int k = which[j];
    counts[k] = nm[j];
    for (int i = 0; i < n1[j]; i++)
      if (S[k].m12[i] >= 0) vvpMapPointMatches[k][S[k].m12[i]] = S[k].mps[i];
  }
  return counts;
}

// int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)  (ORBmatcher.cc:517-650)
template <class KeyFrameT, class MapPointT>
inline int SearchByBoW(MatcherContext& ctx, float mfNNratio, bool mbCheckOrientation, KeyFrameT* pKF1, KeyFrameT* pKF2,
                       std::vector<MapPointT*>& vpMatches12) {
  const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches();
  const std::vector<MapPointT*> vpMapPoints2 = pKF2->GetMapPointMatches();
  const int n1 = (int)vpMapPoints1.size(), n2 = (int)vpMapPoints2.size();
  vpMatches12.assign(n1, static_cast<MapPointT*>(nullptr));
  std::vector<uint8_t> valid1, valid2, t1, t2;
  std::vector<float> a1, a2;
  std::vector<uint32_t> n1v, o1v, f1v, n2v, o2v, f2v;
  detail::validFlags(vpMapPoints1, valid1);
  detail::validFlags(vpMapPoints2, valid2);
  detail::angles(pKF1->mvKeysUn, a1);
  detail::angles(pKF2->mvKeysUn, a2);
  detail::flattenFeatureVector(pKF1->mFeatVec, n1v, o1v, f1v);
  detail::flattenFeatureVector(pKF2->mFeatVec, n2v, o2v, f2v);
  std::vector<int32_t> m12(n1 > 0 ? n1 : 1, -1);
  if (valid2.empty()) valid2.push_back(0);
  int nmatches = 0;
  check(orbfe_search_by_bow(ctx.get(), detail::descriptorRows(ctx, *pKF1, 1, n1, t1), a1.data(), valid1.data(), n1,
                            n1v.data(), o1v.data(), f1v.data(), (int)n1v.size(),
                            detail::descriptorRows(ctx, *pKF2, 1, n2, t2), a2.data(), valid2.data(), n2,
                            n2v.data(), o2v.data(), f2v.data(), (int)n2v.size(), mfNNratio, mbCheckOrientation ? 1 : 0, 1,
                            m12.data(), &nmatches));
  for (int i = 0; i < n1; i++)
    if (m12[i] >= 0) vpMatches12[i] = vpMapPoints2[m12[i]];
  return nmatches;
}

// int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12,
//                                        vector<pair<size_t,size_t>>& vMatchedPairs)   (ORBmatcher.cc:652-804).
// The body keeps the reference's epipole lines (:657-666) and passes (ex, ey); F12 is read through .at<float>(r,c).
template <class KeyFrameT, class MatT>
inline int SearchForTriangulation(MatcherContext& ctx, bool mbCheckOrientation, KeyFrameT* pKF1, KeyFrameT* pKF2,
                                  const MatT& F12, float ex, float ey,
                                  std::vector<std::pair<size_t, size_t> >& vMatchedPairs) {
  const int n1 = (int)pKF1->N, n2 = (int)pKF2->N;
  std::vector<uint8_t> has1(n1 > 0 ? n1 : 1, 0), has2(n2 > 0 ? n2 : 1, 0), t1, t2;
  for (int i = 0; i < n1; i++) has1[i] = pKF1->GetMapPoint(i) ? 1 : 0;   // ORBmatcher.cc:704-709
  for (int i = 0; i < n2; i++) has2[i] = pKF2->GetMapPoint(i) ? 1 : 0;   // :723-727
  std::vector<uint32_t> n1v, o1v, f1v, n2v, o2v, f2v;
  detail::flattenFeatureVector(pKF1->mFeatVec, n1v, o1v, f1v);
  detail::flattenFeatureVector(pKF2->mFeatVec, n2v, o2v, f2v);
  float F[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) F[3 * r + c] = F12.template at<float>(r, c);
  std::vector<int32_t> pairs((size_t)(n1 > 0 ? n1 : 1) * 2, -1);
  int nmatches = 0;
  check(orbfe_search_for_triangulation(
      ctx.get(), reinterpret_cast<const OrbfeKeyPoint*>(pKF1->mvKeysUn.data()), detail::packedDescriptors(pKF1->mDescriptors, n1, t1),
      has1.data(), n1, n1v.data(), o1v.data(), f1v.data(), (int)n1v.size(),
      reinterpret_cast<const OrbfeKeyPoint*>(pKF2->mvKeysUn.data()), detail::packedDescriptors(pKF2->mDescriptors, n2, t2),
      has2.data(), n2, n2v.data(), o2v.data(), f2v.data(), (int)n2v.size(), F, ex, ey, pKF2->mvScaleFactors.data(),
      pKF2->mvLevelSigma2.data(), (int)pKF2->mvScaleFactors.size(), mbCheckOrientation ? 1 : 0, pairs.data(), &nmatches));
  vMatchedPairs.clear();
  vMatchedPairs.reserve(nmatches);
  for (int i = 0; i < nmatches; i++) vMatchedPairs.push_back(std::make_pair((size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]));
  return nmatches;
}

// KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:38-334) over orbfe_kfdb_*: the inverted file and the
// mpVoc->score calls are one GPU query (one wave per keyframe of the map); what the reference does with the result -- the
// member bookkeeping, the 0.8 / 0.75 thresholds, the covisibility accumulation -- is restated here statement for statement.
// KeyFrameT: mnId, mBowVec, mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore,
// GetConnectedKeyFrames(), GetBestCovisibilityKeyFrames(int), GetVectorCovisibleKeyFrames(), isBad().  The key of a keyframe
// is its pointer.  The reference's database has no capacity: this one doubles the device pool when an add does not fit and
// re-adds the live keyframes in their add order (which is their place in every inverted-file list).
template <class KeyFrameT>
class KeyFrameDatabaseT {
 public:
  // n_words = voc.size(), scoring = voc.getScoringType().  The device database is created by the first add: the reference
  // constructs the database before the vocabulary is loaded and calls resizeInvertedFile afterwards (System.cc).
  KeyFrameDatabaseT(int device, size_t n_words, int scoring, int capacity_keyframes = 4096, int capacity_entries = 4096 * 1024)
      : device_(device), scoring_(scoring), nWords_(n_words), capK_(capacity_keyframes), capE_(capacity_entries) {}
  ~KeyFrameDatabaseT() { orbfe_kfdb_destroy(db_); }
  KeyFrameDatabaseT(const KeyFrameDatabaseT&) = delete;
  KeyFrameDatabaseT& operator=(const KeyFrameDatabaseT&) = delete;

  // void KeyFrameDatabase::add(KeyFrame *pKF)   KeyFrameDatabase.cc:38-44
  void add(KeyFrameT* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    addLocked(pKF);
  }
  // add(pKF) for every keyframe of a loaded map, in the vector's order (the loop of Osmap::rebuild, src/Osmap.cpp): one
  // orbfe_kfdb_add_batch.  The database afterwards is the database after the single adds; a keyframe that is already in it, or
  // named twice, throws and nothing is added.
  void add(const std::vector<KeyFrameT*>& vpKFs) {
    std::unique_lock<std::mutex> lock(mMutex);
    if (vpKFs.empty()) return;
    if (!db_) create(capK_, capE_);
    const size_t n = vpKFs.size();
    std::vector<uint64_t> keys(n);
    std::vector<int> counts(n);
    std::vector<size_t> at(n + 1, 0);
    std::set<KeyFrameT*> named;
    for (size_t j = 0; j < n; j++) {
      if (seq_.count(vpKFs[j]) || !named.insert(vpKFs[j]).second)
        throw std::runtime_error("orbfe: KeyFrameDatabase::add of a keyframe that is already in the database");
      keys[j] = key(vpKFs[j]);
      counts[j] = (int)vpKFs[j]->mBowVec.size();
      at[j + 1] = at[j] + (size_t)counts[j];
    }
    std::vector<uint32_t> w(at[n] + 1);
    std::vector<double> v(at[n] + 1);
    std::vector<const uint32_t*> pw(n);
    std::vector<const double*> pv(n);
    for (size_t j = 0; j < n; j++) {
      size_t i = at[j];
      for (auto it = vpKFs[j]->mBowVec.begin(); it != vpKFs[j]->mBowVec.end(); ++it, ++i) { w[i] = (uint32_t)it->first; v[i] = it->second; }
      pw[j] = w.data() + at[j]; pv[j] = v.data() + at[j];
    }
    int rc = orbfe_kfdb_add_batch(db_, (int)n, keys.data(), pw.data(), pv.data(), counts.data());
    if (rc == ORBFE_ERR_OVERFLOW) {   // the reference's database has no capacity: grow the pool, as add(pKF) does
      int nk = 0, ne = 0;
      check(orbfe_kfdb_size(db_, &nk, &ne));
      const long long wantE = (long long)ne + (long long)at[n], wantK = (long long)nk + (long long)n;
      long long capE = capE_, capK = capK_;
      while (capE < wantE) capE *= 2;
      while (capK < wantK) capK *= 2;
      if (capE > 0x7fffffffLL || capK > 0x7fffffffLL) throw std::runtime_error("orbfe: KeyFrameDatabase: more than 2^31 BowVector entries");
      rebuild((int)capK, (int)capE);
      rc = orbfe_kfdb_add_batch(db_, (int)n, keys.data(), pw.data(), pv.data(), counts.data());
    }
    check(rc);
    for (size_t j = 0; j < n; j++) seq_[vpKFs[j]] = next_++;
  }
  // void KeyFrameDatabase::erase(KeyFrame* pKF)   :46-65
  void erase(KeyFrameT* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    eraseLocked(pKF);
  }
  // void KeyFrameDatabase::clear()   :67-71
  void clear() {
    std::unique_lock<std::mutex> lock(mMutex);
    if (db_) check(orbfe_kfdb_clear(db_));
    seq_.clear();
  }
  // void KeyFrameDatabase::resizeInvertedFile(size_t)   :337-339
  void resizeInvertedFile(size_t n) {
    std::unique_lock<std::mutex> lock(mMutex);
    if (n == nWords_) return;
    nWords_ = n;
    if (db_) rebuild(capK_, capE_);
  }
  size_t size() const { return seq_.size(); }

  // The reference minimum score of LoopClosing::DetectLoop (LoopClosing.cc:125-140): the lowest mpORBVocabulary->score to a
  // covisible keyframe that is not bad.  A covisible keyframe that the loop closer has not added yet is scored by a visit
  // (added, scored, erased again: an erased keyframe leaves no trace in any list's order).
  float MinCovisibleScore(KeyFrameT* mpCurrentKF) {
    const std::vector<KeyFrameT*> vpConnectedKeyFrames = mpCurrentKF->GetVectorCovisibleKeyFrames();
    std::unique_lock<std::mutex> lock(mMutex);
    std::vector<uint64_t> keys;
    std::vector<KeyFrameT*> visitors;
    for (size_t i = 0; i < vpConnectedKeyFrames.size(); i++) {
      KeyFrameT* pKF = vpConnectedKeyFrames[i];
      if (pKF->isBad()) continue;
      if (!seq_.count(pKF)) { addLocked(pKF); visitors.push_back(pKF); }
      keys.push_back(key(pKF));
    }
    float minScore = 1;
    if (!keys.empty()) {
      flatten(mpCurrentKF->mBowVec);
      scores_.resize(keys.size());
      const int rc = orbfe_kfdb_score(db_, qw_.data(), qv_.data(), (int)qw_.size(), keys.data(), (int)keys.size(), scores_.data());
      for (KeyFrameT* v : visitors) eraseLocked(v);
      check(rc);
      for (size_t i = 0; i < keys.size(); i++) {
        float score = scores_[i];
        if (score < minScore) minScore = score;
      }
    }
    return minScore;
  }

  // vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore)   KeyFrameDatabase.cc:74-197
  std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore) {
    std::set<KeyFrameT*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    std::list<std::pair<KeyFrameT*, double> > lKFsSharingWords;   // with the score the query computed for each
    {
      std::unique_lock<std::mutex> lock(mMutex);
      // :85-104.  The walk meets keyframe i of the query's result common_[i] times, for the first time in the result's order.
      const int n = query(pKF->mBowVec);
      for (int i = 0; i < n; i++) {
        KeyFrameT* pKFi = reinterpret_cast<KeyFrameT*>((uintptr_t)keys_[i]);
        if (pKFi->mnLoopQuery != pKF->mnId) {
          if (!spConnectedKeyFrames.count(pKFi)) {
            pKFi->mnLoopWords = common_[i];   // reset at the first encounter, counted at each
            pKFi->mnLoopQuery = pKF->mnId;
            lKFsSharingWords.push_back(std::make_pair(pKFi, scores_[i]));
          } else
            pKFi->mnLoopWords = 1;            // connected: mnLoopQuery stays, so EVERY encounter resets; the last leaves 1
        } else
          pKFi->mnLoopWords += common_[i];    // already carries this query's id: never reset, never listed
      }
    }
    if (lKFsSharingWords.empty()) return std::vector<KeyFrameT*>();
    std::list<std::pair<float, KeyFrameT*> > lScoreAndMatch;
    int maxCommonWords = 0;
    for (auto lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      if (lit->first->mnLoopWords > maxCommonWords) maxCommonWords = lit->first->mnLoopWords;
    }
    int minCommonWords = maxCommonWords * 0.8f;
    for (auto lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      KeyFrameT* pKFi = lit->first;
      if (pKFi->mnLoopWords > minCommonWords) {
        float si = lit->second;   // float si = mpVoc->score(pKF->mBowVec,pKFi->mBowVec);
        pKFi->mLoopScore = si;
        if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    if (lScoreAndMatch.empty()) return std::vector<KeyFrameT*>();
    std::list<std::pair<float, KeyFrameT*> > lAccScoreAndMatch;
    float bestAccScore = minScore;
    for (auto it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
      KeyFrameT* pKFi = it->second;
      std::vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = it->first;
      KeyFrameT* pBestKF = pKFi;
      for (auto vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
        KeyFrameT* pKF2 = *vit;
        if (pKF2->mnLoopQuery == pKF->mnId && pKF2->mnLoopWords > minCommonWords) {
          accScore += pKF2->mLoopScore;
          if (pKF2->mLoopScore > bestScore) {
            pBestKF = pKF2;
            bestScore = pKF2->mLoopScore;
          }
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    float minScoreToRetain = 0.75f * bestAccScore;
    std::set<KeyFrameT*> spAlreadyAddedKF;
    std::vector<KeyFrameT*> vpLoopCandidates;
    vpLoopCandidates.reserve(lAccScoreAndMatch.size());
    for (auto it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
      if (it->first > minScoreToRetain) {
        KeyFrameT* pKFi = it->second;
        if (!spAlreadyAddedKF.count(pKFi)) {
          vpLoopCandidates.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        }
      }
    }
    return vpLoopCandidates;
  }

  // vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F)   KeyFrameDatabase.cc:199-334
  template <class FrameT>
  std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F) {
    std::list<std::pair<KeyFrameT*, double> > lKFsSharingWords;
    {
      std::unique_lock<std::mutex> lock(mMutex);
      const int n = query(F->mBowVec);   // :207-222
      for (int i = 0; i < n; i++) {
        KeyFrameT* pKFi = reinterpret_cast<KeyFrameT*>((uintptr_t)keys_[i]);
        if (pKFi->mnRelocQuery != F->mnId) {
          pKFi->mnRelocWords = common_[i];
          pKFi->mnRelocQuery = F->mnId;
          lKFsSharingWords.push_back(std::make_pair(pKFi, scores_[i]));
        } else
          pKFi->mnRelocWords += common_[i];
      }
    }
    if (lKFsSharingWords.empty()) return std::vector<KeyFrameT*>();
    int maxCommonWords = 0;
    for (auto lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      if (lit->first->mnRelocWords > maxCommonWords) maxCommonWords = lit->first->mnRelocWords;
    }
    int minCommonWords = maxCommonWords * 0.8f;
    std::list<std::pair<float, KeyFrameT*> > lScoreAndMatch;
    for (auto lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      KeyFrameT* pKFi = lit->first;
      if (pKFi->mnRelocWords > minCommonWords) {
        float si = lit->second;   // float si = mpVoc->score(F->mBowVec,pKFi->mBowVec);
        pKFi->mRelocScore = si;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    if (lScoreAndMatch.empty()) return std::vector<KeyFrameT*>();
    std::list<std::pair<float, KeyFrameT*> > lAccScoreAndMatch;
    float bestAccScore = 0;
    for (auto it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
      KeyFrameT* pKFi = it->second;
      std::vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = bestScore;
      KeyFrameT* pBestKF = pKFi;
      for (auto vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
        KeyFrameT* pKF2 = *vit;
        if (pKF2->mnRelocQuery != F->mnId) continue;
        accScore += pKF2->mRelocScore;   // (also of a neighbour that this query did not score: its score of an earlier one)
        if (pKF2->mRelocScore > bestScore) {
          pBestKF = pKF2;
          bestScore = pKF2->mRelocScore;
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    float minScoreToRetain = 0.75f * bestAccScore;
    std::set<KeyFrameT*> spAlreadyAddedKF;
    std::vector<KeyFrameT*> vpRelocCandidates;
    vpRelocCandidates.reserve(lAccScoreAndMatch.size());
    for (auto it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
      const float& si = it->first;
      if (si > minScoreToRetain) {
        KeyFrameT* pKFi = it->second;
        if (!spAlreadyAddedKF.count(pKFi)) {
          vpRelocCandidates.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        }
      }
    }
    return vpRelocCandidates;
  }

 private:
  static uint64_t key(KeyFrameT* p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); }
  template <class BowVectorT>
  void flatten(const BowVectorT& v) {
    qw_.clear(); qv_.clear();
    for (auto it = v.begin(); it != v.end(); ++it) { qw_.push_back((uint32_t)it->first); qv_.push_back(it->second); }
  }
  void create(int capK, int capE) {
    orbfe_kfdb* nd = nullptr;
    check(orbfe_kfdb_create(device_, (int)std::max<size_t>(nWords_, 1), scoring_, capK, capE, &nd));
    orbfe_kfdb_destroy(db_);
    db_ = nd; capK_ = capK; capE_ = capE;
  }
  void rebuild(int capK, int capE) {   // a new pool with the live keyframes in their add order
    create(capK, capE);
    std::vector<std::pair<uint64_t, KeyFrameT*> > order;
    for (auto& e : seq_) order.push_back(std::make_pair(e.second, e.first));
    std::sort(order.begin(), order.end());
    for (auto& e : order) {
      flatten(e.second->mBowVec);
      check(orbfe_kfdb_add(db_, key(e.second), qw_.data(), qv_.data(), (int)qw_.size()));
    }
  }
  void addLocked(KeyFrameT* pKF) {
    if (!db_) create(capK_, capE_);
    if (seq_.count(pKF)) throw std::runtime_error("orbfe: KeyFrameDatabase::add of a keyframe that is already in the database");
    flatten(pKF->mBowVec);
    int rc = orbfe_kfdb_add(db_, key(pKF), qw_.data(), qv_.data(), (int)qw_.size());
    if (rc == ORBFE_ERR_OVERFLOW) {
      int nk = 0, ne = 0;
      check(orbfe_kfdb_size(db_, &nk, &ne));
      const std::vector<uint32_t> w = qw_;
      const std::vector<double> v = qv_;
      const long long wantE = (long long)ne + (long long)w.size();
      long long capE = capE_;
      while (capE < wantE) capE *= 2;
      if (capE > 0x7fffffffLL) throw std::runtime_error("orbfe: KeyFrameDatabase: more than 2^31 BowVector entries");
      rebuild(nk + 1 > capK_ ? capK_ * 2 : capK_, (int)capE);
      rc = orbfe_kfdb_add(db_, key(pKF), w.data(), v.data(), (int)w.size());
    }
    check(rc);
    seq_[pKF] = next_++;
  }
  void eraseLocked(KeyFrameT* pKF) {
    if (!seq_.erase(pKF)) return;   // not in any list: the reference's loops find nothing
    check(orbfe_kfdb_erase(db_, key(pKF)));
  }
  template <class BowVectorT>
  int query(const BowVectorT& v) {
    if (!db_ || seq_.empty()) return 0;
    flatten(v);
    const size_t cap = seq_.size();
    keys_.resize(cap); common_.resize(cap); scores_.resize(cap);
    int n = 0;
    check(orbfe_kfdb_query(db_, qw_.data(), qv_.data(), (int)qw_.size(), keys_.data(), common_.data(), scores_.data(), (int)cap, &n));
    return n;
  }

  int device_, scoring_;
  size_t nWords_;
  int capK_, capE_;
  orbfe_kfdb* db_ = nullptr;
  std::mutex mMutex;
  std::unordered_map<KeyFrameT*, uint64_t> seq_;   // the live keyframes and their add order
  uint64_t next_ = 0;
  std::vector<uint32_t> qw_;
  std::vector<double> qv_, scores_;
  std::vector<uint64_t> keys_;
  std::vector<int32_t> common_;
};

}  // namespace orbfe
