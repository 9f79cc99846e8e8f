// orbfe_stream.cpp -- native frame-stream runner on top of the extractor / matcher C ABI.
//
// Role in the reference: the per-frame front end is driven by the Tracking thread, one frame at a
// time (System::TrackMonocular -> Frame::Frame -> ORBextractor, then ORBmatcher).
// For throughput over a stream (BASELINE.json config 4: independent streams, one per GPU) this
// runner keeps the GPU fed without any per-frame host orchestration in the caller's language:
//   push(batch of frames)  ->  [extract thread]  async submit on one of `depth` extractor handles, with
//                              SearchForInitialization of every frame against its predecessor in the
//                              stream chained behind the extraction on the GPU (orbfe_sfi_chain);
//                              collect in order
//   pop()                  ->  results of the oldest finished batch, in push order.
// Everything the GPU computes goes through the extractor / matcher C ABI
// (orbfe_extract_batch_submit_matched/_collect_matched, orbfe_search_for_initialization for a frame 0
// whose predecessor the chain does not hold), so results are identical to calling orbfe_extract_batch
// and orbfe_search_for_initialization frame by frame.
#include <pthread.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/orbfe.h"

namespace orbfe {
void set_err(const char* fmt, ...);
}
int orbfe_concurrent_streams(orbfe_extractor* const* hs, int n);   // orbfe_extractor.hip
using orbfe::set_err;

namespace {
struct Slot {
  std::vector<const uint8_t*> frames;
  int rows = 0, cols = 0;
  size_t stride = 0;
  int onDevice = 1;
  std::vector<OrbfeKeyPoint> kps;
  std::vector<uint8_t> desc;
  std::vector<int> n;
  std::vector<int32_t> m12;
  std::vector<int> nm;
  std::vector<float> prevxy;   // [cap][2] query centres of row 0 (matchFrame0)
  std::vector<uint32_t> bowLeaf, bowNode;   // [batch][cap], with a vocabulary set
  std::vector<float> xyUn, prevXyUn;        // [batch][cap][2] mvKeysUn, and the predecessor's, with a camera set
  bool camera = false;                      // the stream had a camera at push time
  // predecessor of frame 0 (last frame of the previous batch), copied at collect time
  std::vector<OrbfeKeyPoint> prevKps;
  std::vector<uint8_t> prevDesc;
  int prevN = -1;
  long long seq = 0;
  bool done = false;
  bool held = false;        // handed out by orbfe_stream_pop_hold and not released yet
  bool frame0OnHost = false;   // the chain does not hold frame 0's predecessor: the runner matches it on the host (matchFrame0)
  int status = ORBFE_OK;
  std::string err;
  // match parameters of the stream at push time (orbfe_stream_set_matching only works on an idle stream, but the
  // snapshot keeps submit and collect of one batch on the same variant by construction)
  int window = 0, checkOri = 1;
  float nnratio = 0.9f;
  float bounds[4] = {0, 0, 0, 0};
};
}  // namespace

struct orbfe_stream {
  int batch = 0, depth = 0, cap = 0, device = 0;
  int inFlight = 0;   // batches on the GPU at a time: depth, or fewer when the process has fewer hardware queues than that (orbfe_stream_create)
  int window = 100, checkOri = 1;
  float nnratio = 0.9f;
  float bounds[4] = {0, 0, 0, 0};
  std::vector<orbfe_extractor*> ext;
  orbfe_sfi_chain* chain = nullptr;       // GPU-resident matching
  orbfe_matcher* frame0Matcher = nullptr; // frame 0 of a batch whose predecessor the chain does not hold (created when first needed)
  int chainRows = 0, chainCols = 0;       // geometry of the previous batch if the chain matched it (its last frame is the chain's carry), else 0
  bool isolated = false;                  // orbfe_stream_set_isolated_batches: frame 0 of a batch has no predecessor
  std::vector<Slot> slots;
  void growSlots(int nslots) {     // caller holds no batch in flight (or is the constructor)
    const int old = (int)slots.size();
    if (nslots <= old) return;
    slots.resize(nslots);
    for (int i = old; i < nslots; i++) {
      Slot& sl = slots[i];
      sl.frames.resize(batch);
      sl.kps.resize((size_t)batch * cap);
      sl.desc.resize((size_t)batch * cap * 32);
      sl.n.assign(batch, 0);
      sl.m12.assign((size_t)batch * cap, -1);
      sl.nm.assign(batch, 0);
      sl.prevxy.resize((size_t)cap * 2);
      freeQ.push_back(i);
    }
  }

  std::mutex mu;
  std::condition_variable cv;
  std::deque<int> freeQ, extractQ;
  int popped = -1;  // slot handed to the caller by the last pop (returned to freeQ on the next pop)
  int nHeld = 0;     // slots handed out by orbfe_stream_pop_hold and not released
  bool idle() const { return pushSeq == popSeq && nHeld == 0; }   // (caller holds mu)
  // keypoint slots per frame: grow every slot to `need` -- only while idle, the row stride changes (caller holds mu)
  int growCap(int need, int rows, int cols) {
    if (need <= cap) return ORBFE_OK;
    if (!idle()) {
      set_err("frames of %dx%d need %d keypoint slots per frame, the runner holds %d: pop every pushed batch and release every held one "
              "before changing the frame size", cols, rows, need, cap);
      return ORBFE_ERR_INVALID;
    }
    cap = need;
    for (Slot& sl : slots) {
      sl.kps.resize((size_t)batch * need);
      sl.desc.resize((size_t)batch * need * 32);
      sl.m12.assign((size_t)batch * need, -1);
      sl.prevxy.resize((size_t)need * 2);
    }
    return ORBFE_OK;
  }
  bool stop = false;
  std::thread tExtract;
  long long pushSeq = 0, popSeq = 0;
  int channels = 1;   // bytes per pixel of the pushed frames (orbfe_stream_set_input_format)
  bool bow = false;   // orbfe_stream_set_vocabulary
  bool camera = false;   // orbfe_stream_set_camera
  std::vector<float> lastXyUn;

  // last frame of the previous batch (the predecessor of frame 0 of the next one)
  std::vector<OrbfeKeyPoint> lastKps;
  std::vector<uint8_t> lastDesc;
  int lastN = -1;

  // busy time of the extract worker (ms) and batches done, for orbfe_stream_stats
  double busySubmit = 0, busyCollect = 0;
  long long nBatches = 0;
  static double nowMs() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  }

  // frame 0 of a batch whose predecessor (the last frame of the batch before, s.prevKps) the chain does not hold:
  // the host-array search (the same kernels), row 0 overwritten
  int matchFrame0(Slot& s) {
    if (!frame0Matcher) {
      const int rc = orbfe_matcher_create(device, &frame0Matcher);
      if (rc != ORBFE_OK) return rc;
    }
    float* pxy = s.prevxy.data();   // (row 0: prevN <= cap)
    for (int j = 0; j < s.prevN; j++) { pxy[2 * j] = s.prevKps[j].x; pxy[2 * j + 1] = s.prevKps[j].y; }
    int32_t* row = s.m12.data();
    std::fill(row, row + cap, -1);
    if (s.camera) {   // the search runs on mvKeysUn of both frames, vbPrevMatched := F1's mvKeysUn (Tracking.cc:355-357)
      std::vector<OrbfeKeyPoint> k1(s.prevKps.begin(), s.prevKps.begin() + s.prevN), k2(s.kps.begin(), s.kps.begin() + s.n[0]);
      for (int j = 0; j < s.prevN; j++) { k1[j].x = pxy[2 * j] = s.prevXyUn[2 * j]; k1[j].y = pxy[2 * j + 1] = s.prevXyUn[2 * j + 1]; }
      for (int j = 0; j < s.n[0]; j++) { k2[j].x = s.xyUn[2 * j]; k2[j].y = s.xyUn[2 * j + 1]; }
      return orbfe_search_for_initialization(frame0Matcher, k1.data(), s.prevDesc.data(), s.prevN, k2.data(), s.desc.data(), s.n[0],
                                             s.bounds, pxy, row, s.window, s.nnratio, s.checkOri, &s.nm[0]);
    }
    return orbfe_search_for_initialization(frame0Matcher, s.prevKps.data(), s.prevDesc.data(), s.prevN, s.kps.data(), s.desc.data(), s.n[0],
                                           s.bounds, pxy, row, s.window, s.nnratio, s.checkOri, &s.nm[0]);
  }

  void extractLoop() {
    std::deque<std::pair<int, int>> inflight;  // (slot, extractor)
    int nextExt = 0;
    for (;;) {
      int job = -1;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !inflight.empty() || !extractQ.empty(); });
        // on stop, batches that were queued but never submitted are dropped (their frames may already be gone);
        // only batches the GPU is working on are waited for
        if (stop) extractQ.clear();
        if (stop && inflight.empty()) return;
        if (!extractQ.empty() && (int)inflight.size() < inFlight) {
          job = extractQ.front();
          extractQ.pop_front();
        }
      }
      if (job >= 0) {
        Slot& s = slots[job];
        orbfe_extractor* h = ext[nextExt];
        const double ta = nowMs();
        if (s.window > 0) {
          // the chain's carry is frame 0's predecessor only if the chain matched the batch before, on the same geometry (so the same
          // route: the GPU and the host quadtree route keep a carry each); otherwise frame 0 is matched on the host at collect time
          s.frame0OnHost = s.rows != chainRows || s.cols != chainCols;
          if (s.frame0OnHost) (void)orbfe_sfi_chain_restart(chain);
          s.status = orbfe_extract_batch_submit_matched(h, chain, batch, s.frames.data(), s.onDevice, s.rows, s.cols, s.stride,
                                                        s.bounds, s.window, s.nnratio, s.checkOri);
          chainRows = s.status == ORBFE_OK ? s.rows : 0;
          chainCols = s.status == ORBFE_OK ? s.cols : 0;
        } else {
          s.status = orbfe_extract_batch_submit(h, batch, s.frames.data(), s.onDevice, s.rows, s.cols, s.stride);
          chainRows = chainCols = 0;
        }
        {
          std::lock_guard<std::mutex> lk(mu);
          busySubmit += nowMs() - ta;
        }
        if (s.status != ORBFE_OK) s.err = orbfe_last_error();
        inflight.emplace_back(job, nextExt);
        nextExt = (nextExt + 1) % (int)ext.size();
        continue;
      }
      if (inflight.empty()) continue;
      const int slot = inflight.front().first, e = inflight.front().second;
      inflight.pop_front();
      Slot& s = slots[slot];
      if (s.status == ORBFE_OK) {
        const double ta = nowMs();
        if (s.camera) {
          s.xyUn.resize((size_t)batch * cap * 2);
          const bool m = s.window > 0;
          s.status = orbfe_extract_batch_collect_undistorted(ext[e], s.kps.data(), s.desc.data(), cap, s.n.data(), s.xyUn.data(),
                                                             m ? s.m12.data() : nullptr, m ? s.nm.data() : nullptr);
        } else if (s.window > 0)
          s.status = orbfe_extract_batch_collect_matched(ext[e], s.kps.data(), s.desc.data(), cap, s.n.data(), s.m12.data(),
                                                         s.nm.data());
        else
          s.status = orbfe_extract_batch_collect(ext[e], s.kps.data(), s.desc.data(), cap, s.n.data());
        if (s.status == ORBFE_OK && bow) {   // raw (leaf, node) pairs of the batch; vectors are assembled on demand
          s.bowLeaf.resize((size_t)batch * cap);
          s.bowNode.resize((size_t)batch * cap);
          for (int f = 0; f < batch && s.status == ORBFE_OK; f++) {
            int nb = 0;
            s.status = orbfe_extract_bow_raw(ext[e], f, s.bowLeaf.data() + (size_t)f * cap, s.bowNode.data() + (size_t)f * cap, cap, &nb);
          }
        }
        {
          std::lock_guard<std::mutex> lk(mu);
          busyCollect += nowMs() - ta;
        }
        if (s.status != ORBFE_OK) s.err = orbfe_last_error();
      }
      if (s.status == ORBFE_OK) {
        s.prevN = isolated ? -1 : lastN;
        if (s.prevN >= 0) { s.prevKps = lastKps; s.prevDesc = lastDesc; if (s.camera) s.prevXyUn = lastXyUn; }
        if (s.window <= 0) {   // extraction only: no matches
          std::fill(s.nm.begin(), s.nm.end(), 0);
          std::fill(s.m12.begin(), s.m12.end(), -1);
        } else if (s.frame0OnHost && s.prevN >= 0) {
          s.status = matchFrame0(s);
          if (s.status != ORBFE_OK) s.err = orbfe_last_error();
        }
        lastN = s.n[batch - 1];
        lastKps.assign(s.kps.begin() + (size_t)(batch - 1) * cap, s.kps.begin() + (size_t)(batch - 1) * cap + lastN);
        lastDesc.assign(s.desc.begin() + (size_t)(batch - 1) * cap * 32, s.desc.begin() + ((size_t)(batch - 1) * cap + lastN) * 32);
        if (s.camera) lastXyUn.assign(s.xyUn.begin() + (size_t)(batch - 1) * cap * 2, s.xyUn.begin() + ((size_t)(batch - 1) * cap + lastN) * 2);
      }
      {
        std::lock_guard<std::mutex> lk(mu);   // matches (if any) came back with the batch: done
        nBatches++;
        s.done = true;
      }
      cv.notify_all();
    }
  }
};

extern "C" {

int orbfe_stream_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device_id,
                        int batch, int depth, orbfe_stream** out) {
  if (!out || batch < 1 || depth < 1 || depth > 8) { set_err("invalid stream parameters"); return ORBFE_ERR_INVALID; }
  *out = nullptr;
  orbfe_stream* s = new orbfe_stream();
  s->batch = batch;
  s->depth = depth;
  s->device = device_id;
  // depth handles for the batches on the GPU (a spare one for the batch being assembled on the host measured slower: DESIGN_NOTES.md E.5)
  const int nhandles = depth;
  for (int d = 0; d < nhandles; d++) {
    orbfe_extractor* h = nullptr;
    int rc = orbfe_extractor_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device_id, &h);
    if (rc == ORBFE_OK && !getenv("ORBFE_POLL_WAIT_US")) rc = orbfe_extractor_set_wait_mode(h, 50);   // the runner pipelines: do not burn a core on waiting
    if (rc != ORBFE_OK) {
      for (auto* e : s->ext) orbfe_extractor_destroy(e);
      delete s;
      return rc;
    }
    s->ext.push_back(h);
  }
  {
    int rc = orbfe_sfi_chain_create(s->ext[0], &s->chain);
    if (rc != ORBFE_OK) {
      for (auto* e : s->ext) orbfe_extractor_destroy(e);
      delete s;
      return rc;
    }
  }
  // `depth` batches in flight run on `depth` HIP streams, and the HIP runtime folds a process's streams onto GPU_MAX_HW_QUEUES hardware
  // queues (4 unless the variable said otherwise BEFORE the runtime started -- a library cannot set it for the process it is loaded
  // into); two streams on one queue serialise, and a fourth batch that waits behind the first on its queue costs more than it
  // overlaps (87.9 k frames/s at depth 4 on 4 queues against 89.8 k at depth 3; 93.0 k at depth 4 on 8 queues: gpurun r06j,
  // DESIGN.md s6).  So the runner MEASURES how many of its streams run side by side and keeps that many batches in flight.
  s->inFlight = depth;
  if (depth > 1) {
    const int k = orbfe_concurrent_streams(s->ext.data(), depth);
    if (k < 0) {
      for (auto* e : s->ext) orbfe_extractor_destroy(e);
      orbfe_sfi_chain_destroy(s->chain);
      delete s;
      return k;
    }
    s->inFlight = k;
    while ((int)s->ext.size() > k) {   // the handles whose streams share a queue are not used (nor their memory kept)
      orbfe_extractor_destroy(s->ext.back());
      s->ext.pop_back();
    }
    static bool said = false;
    if (k < depth && !said && !getenv("ORBFE_QUIET")) {
      said = true;
      const char* q = getenv("GPU_MAX_HW_QUEUES");
      fprintf(stderr, "liborbfe: orbfe_stream_create(depth = %d): only %d of the runner's streams run side by side in this process (GPU_MAX_HW_QUEUES=%s), "
                      "so %d batches are kept in flight; export GPU_MAX_HW_QUEUES=8 before the process starts for the last 3 %%\n",
              depth, k, q ? q : "unset: 4", k);
    }
  }
  s->cap = orbfe_extractor_max_keypoints(s->ext[0]);
  // result slots: `depth` batches on the GPU, one in the caller's hands, a few queued in front of the worker.  A caller
  // whose own thread can be held up for milliseconds (bench.py's Python driver) asks for a deeper queue with
  // orbfe_stream_set_queue_slots; a slot is host memory only (4 MB at 1080p / 2000 features / 32 frames).
  s->growSlots(depth + 4);
  s->tExtract = std::thread([s] { pthread_setname_np(pthread_self(), "orbfe-runner"); s->extractLoop(); });
  *out = s;
  return ORBFE_OK;
}

void orbfe_stream_destroy(orbfe_stream* s) {
  if (!s) return;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    s->stop = true;
  }
  s->cv.notify_all();
  if (s->tExtract.joinable()) s->tExtract.join();
  for (auto* e : s->ext) orbfe_extractor_destroy(e);
  if (s->frame0Matcher) orbfe_matcher_destroy(s->frame0Matcher);
  orbfe_sfi_chain_destroy(s->chain);
  delete s;
}

int orbfe_stream_set_matching(orbfe_stream* s, const float bounds[4], int window_size, float nnratio,
                              int check_orientation) {
  if (!s || (window_size > 0 && !bounds)) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->idle()) { set_err("batches are still in flight or held"); return ORBFE_ERR_INVALID; }
  if (bounds) memcpy(s->bounds, bounds, sizeof s->bounds);
  s->window = window_size;
  s->nnratio = nnratio;
  s->checkOri = check_orientation;
  return ORBFE_OK;
}

int orbfe_stream_set_isolated_batches(orbfe_stream* s, int isolated) {
  if (!s) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->idle()) { set_err("batches are still in flight or held"); return ORBFE_ERR_INVALID; }
  s->isolated = isolated != 0;
  s->lastN = -1;
  s->chainRows = s->chainCols = 0;
  return orbfe_sfi_chain_set_isolated(s->chain, isolated);
}

int orbfe_stream_set_input_format(orbfe_stream* s, int format, int gray_variant) {
  if (!s) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->idle()) { set_err("batches are still in flight or held"); return ORBFE_ERR_INVALID; }
  for (orbfe_extractor* e : s->ext) {
    const int rc = orbfe_extractor_set_input_format(e, format, gray_variant);
    if (rc) return rc;
  }
  s->channels = format == ORBFE_INPUT_GRAY8 ? 1 : (format == ORBFE_INPUT_RGB8 || format == ORBFE_INPUT_BGR8) ? 3 : 4;
  return ORBFE_OK;
}

int orbfe_stream_set_blur_variant(orbfe_stream* s, int variant) {
  if (!s) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->idle()) { set_err("batches are still in flight or held"); return ORBFE_ERR_INVALID; }
  for (orbfe_extractor* e : s->ext) {
    const int rc = orbfe_extractor_set_blur_variant(e, variant);
    if (rc) return rc;
  }
  return ORBFE_OK;
}

// The camera of every handle of the runner.  The frame pushed next has no predecessor: the one the runner holds was undistorted
// (or not) by the camera before.
int orbfe_stream_set_camera(orbfe_stream* s, int camera_mode, float fx, float fy, float cx, float cy, const float* dist, int ndist) {
  if (!s) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->idle()) { set_err("batches are still in flight or held"); return ORBFE_ERR_INVALID; }
  for (orbfe_extractor* e : s->ext) {
    const int rc = orbfe_extractor_set_camera(e, camera_mode, fx, fy, cx, cy, dist, ndist);   // (a refused model is refused by the first handle)
    if (rc) return rc;
  }
  s->camera = true;
  s->lastN = -1;
  s->chainRows = s->chainCols = 0;
  return orbfe_sfi_chain_restart(s->chain);
}

// The equidistant (fisheye) model for every handle of the runner: as orbfe_stream_set_camera.
int orbfe_stream_set_camera_equidistant(orbfe_stream* s, float fx, float fy, float cx, float cy) {
  if (!s) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->idle()) { set_err("batches are still in flight or held"); return ORBFE_ERR_INVALID; }
  for (orbfe_extractor* e : s->ext) {
    const int rc = orbfe_extractor_set_camera_equidistant(e, fx, fy, cx, cy);
    if (rc) return rc;
  }
  s->camera = true;
  s->lastN = -1;
  s->chainRows = s->chainCols = 0;
  return orbfe_sfi_chain_restart(s->chain);
}

// orbfe_extractor_equidistant_stats summed over the runner's handles (batches popped so far)
int orbfe_stream_equidistant_stats(orbfe_stream* s, long long stats[3]) {
  if (!s || !stats) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  stats[0] = stats[1] = stats[2] = 0;
  for (orbfe_extractor* e : s->ext) {
    long long one[3];
    const int rc = orbfe_extractor_equidistant_stats(e, one);
    if (rc) return rc;
    for (int i = 0; i < 3; i++) stats[i] += one[i];
  }
  return ORBFE_OK;
}

int orbfe_stream_xy_un(orbfe_stream* s, const float** xy_un) {
  if (!s || !xy_un) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  if (s->popped < 0 || !s->slots[s->popped].camera || s->slots[s->popped].xyUn.empty()) {
    set_err("no popped batch with undistorted keypoints (orbfe_stream_set_camera)");
    return ORBFE_ERR_INVALID;
  }
  *xy_un = s->slots[s->popped].xyUn.data();
  return ORBFE_OK;
}

int orbfe_stream_set_vocabulary(orbfe_stream* s, orbfe_vocabulary* v, int levelsup) {
  if (!s) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->idle()) { set_err("batches are still in flight or held"); return ORBFE_ERR_INVALID; }
  for (orbfe_extractor* e : s->ext) {
    const int rc = orbfe_extractor_set_vocabulary(e, v, levelsup);
    if (rc) return rc;
  }
  s->bow = v != nullptr;
  return ORBFE_OK;
}

int orbfe_stream_bow_raw(orbfe_stream* s, int frame, const uint32_t** leaf_node, const uint32_t** level_node, int* n) {
  if (!s || !leaf_node || !level_node || !n || frame < 0 || frame >= s->batch) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  if (s->popped < 0 || !s->bow || s->slots[s->popped].bowLeaf.empty()) {
    set_err("no popped batch with bag-of-words results");
    return ORBFE_ERR_INVALID;
  }
  const Slot& sl = s->slots[s->popped];
  *leaf_node = sl.bowLeaf.data() + (size_t)frame * s->cap;
  *level_node = sl.bowNode.data() + (size_t)frame * s->cap;
  *n = sl.n[frame];
  return ORBFE_OK;
}

int orbfe_stream_capacity(const orbfe_stream* s) { return s ? s->cap : 0; }

// (orbfe_stream_multi.cpp, not in the header) keypoint slots per frame that frames of rows x cols need, and growing to them while idle
int orbfe_stream_capacity_for(const orbfe_stream* s, int rows, int cols) {
  return s ? std::max(s->cap, orbfe_extractor_max_keypoints_for_size(s->ext[0], rows, cols)) : 0;
}
int orbfe_stream_grow_capacity(orbfe_stream* s, int need) {
  if (!s) { set_err("stream is NULL"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  return s->growCap(need, 0, 0);
}
// (orbfe_stream_multi.cpp, not in the header) mvKeysUn of a result held by orbfe_stream_pop_hold; nullptr: pushed without a camera
const float* orbfe_stream_held_xy_un(orbfe_stream* s, int ticket) {
  if (!s || ticket < 0 || ticket >= (int)s->slots.size()) return nullptr;
  const Slot& sl = s->slots[(size_t)ticket];
  return sl.held && sl.camera && !sl.xyUn.empty() ? sl.xyUn.data() : nullptr;
}
int orbfe_stream_batches_in_flight(const orbfe_stream* s) { return s ? s->inFlight : 0; }

int orbfe_stream_set_queue_slots(orbfe_stream* s, int nslots) {
  if (!s) { set_err("stream is NULL"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->idle()) { set_err("orbfe_stream_set_queue_slots: batches in flight or held"); return ORBFE_ERR_INVALID; }
  if (nslots < s->depth + 2 || nslots > 256) { set_err("orbfe_stream_set_queue_slots: need depth+2 <= nslots <= 256"); return ORBFE_ERR_INVALID; }
  s->growSlots(nslots);
  return ORBFE_OK;
}
int orbfe_stream_queue_slots(const orbfe_stream* s) { return s ? (int)s->slots.size() : 0; }

int orbfe_stream_push(orbfe_stream* s, const uint8_t* const* gray, int in_device_memory, int rows, int cols,
                      size_t stride_bytes) {
  if (!s || !gray || rows <= 0 || cols <= 0 || stride_bytes < (size_t)cols * s->channels) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  // matching is on from creation (window 100) but the image bounds are not known until orbfe_stream_set_matching: with empty bounds
  // the match grid's inverse cell size is infinite and the window's cell range leaves the grid
  if (s->window > 0 && !(s->bounds[1] > s->bounds[0] && s->bounds[3] > s->bounds[2])) {
    set_err("matching is on but the image bounds are empty: call orbfe_stream_set_matching (bounds, or window 0) before the first push");
    return ORBFE_ERR_INVALID;
  }
  // a geometry whose levels return more keypoints than the slots hold (strips wider than 4.5 : 1: every root node of a level
  // yields keypoints, ORBextractor.cc:620-700): grow every slot -- only while the pipeline is empty, the row stride changes
  const int need = orbfe_extractor_max_keypoints_for_size(s->ext[0], rows, cols);
  if (need > s->cap) {
    std::lock_guard<std::mutex> lk(s->mu);
    const int rc = s->growCap(need, rows, cols);
    if (rc != ORBFE_OK) return rc;
  }
  int slot;
  {
    std::unique_lock<std::mutex> lk(s->mu);
    s->cv.wait(lk, [&] { return !s->freeQ.empty(); });
    slot = s->freeQ.front();
    s->freeQ.pop_front();
  }
  Slot& sl = s->slots[slot];
  for (int i = 0; i < s->batch; i++) sl.frames[i] = gray[i];
  sl.rows = rows; sl.cols = cols; sl.stride = stride_bytes; sl.onDevice = in_device_memory;
  sl.status = ORBFE_OK;
  sl.done = false;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    sl.window = s->window; sl.checkOri = s->checkOri; sl.nnratio = s->nnratio;
    sl.camera = s->camera;
    memcpy(sl.bounds, s->bounds, sizeof sl.bounds);
    sl.seq = s->pushSeq++;
    s->extractQ.push_back(slot);
  }
  s->cv.notify_all();
  return ORBFE_OK;
}

int orbfe_stream_pop(orbfe_stream* s, const OrbfeKeyPoint** kps, const uint8_t** desc, const int** n_kps,
                     const int32_t** matches12, const int** nmatches) {
  if (!s) { set_err("stream is NULL"); return ORBFE_ERR_INVALID; }
  int slot;
  {
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->nHeld > 0) { set_err("orbfe_stream_pop: %d result(s) of orbfe_stream_pop_hold not released", s->nHeld); return ORBFE_ERR_INVALID; }
    if (s->popped >= 0) {
      s->freeQ.push_back(s->popped);
      s->popped = -1;
      s->cv.notify_all();
    }
    if (s->popSeq == s->pushSeq) { set_err("no batch outstanding (every pushed batch has been popped)"); return ORBFE_ERR_INVALID; }
    auto ready = [&]() -> int {
      for (size_t i = 0; i < s->slots.size(); i++)
        if (s->slots[i].done && s->slots[i].seq == s->popSeq) return (int)i;
      return -1;
    };
    s->cv.wait(lk, [&] { return ready() >= 0; });
    slot = ready();
    s->slots[slot].done = false;
    s->popSeq++;
    s->popped = slot;
  }
  Slot& sl = s->slots[slot];
  if (kps) *kps = sl.kps.data();
  if (desc) *desc = sl.desc.data();
  if (n_kps) *n_kps = sl.n.data();
  if (matches12) *matches12 = sl.m12.data();
  if (nmatches) *nmatches = sl.nm.data();
  if (sl.status != ORBFE_OK) set_err("%s", sl.err.c_str());
  return sl.status;
}

// pop WITHOUT the "valid until the next pop" rule: the result stays where it is until orbfe_stream_release(s, *ticket) -- any number of
// results may be held, each keeps one result slot of the runner busy (orbfe_stream_queue_slots).  For a consumer that hands results on
// to another thread (orbfe_stream_multi's finishers) without copying them.
int orbfe_stream_pop_hold(orbfe_stream* s, const OrbfeKeyPoint** kps, const uint8_t** desc, const int** n_kps, const int32_t** matches12,
                          const int** nmatches, int* ticket) {
  if (!s || !ticket) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  int slot;
  {
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->popped >= 0) {   // (a pop ends the previous pop's result)
      s->freeQ.push_back(s->popped);
      s->popped = -1;
      s->cv.notify_all();
    }
    if (s->popSeq == s->pushSeq) { set_err("no batch outstanding (every pushed batch has been popped)"); return ORBFE_ERR_INVALID; }
    auto ready = [&]() -> int {
      for (size_t i = 0; i < s->slots.size(); i++)
        if (s->slots[i].done && s->slots[i].seq == s->popSeq) return (int)i;
      return -1;
    };
    s->cv.wait(lk, [&] { return ready() >= 0; });
    slot = ready();
    s->slots[slot].done = false;
    s->slots[slot].held = true;
    s->nHeld++;
    s->popSeq++;
  }
  *ticket = slot;
  Slot& sl = s->slots[slot];
  if (kps) *kps = sl.kps.data();
  if (desc) *desc = sl.desc.data();
  if (n_kps) *n_kps = sl.n.data();
  if (matches12) *matches12 = sl.m12.data();
  if (nmatches) *nmatches = sl.nm.data();
  if (sl.status != ORBFE_OK) set_err("%s", sl.err.c_str());
  return sl.status;
}

int orbfe_stream_release(orbfe_stream* s, int ticket) {
  if (!s || ticket < 0) { set_err("invalid arguments"); return ORBFE_ERR_INVALID; }
  {
    std::lock_guard<std::mutex> lk(s->mu);
    if (ticket >= (int)s->slots.size() || !s->slots[(size_t)ticket].held) { set_err("not a held ticket of this runner"); return ORBFE_ERR_INVALID; }
    s->slots[(size_t)ticket].held = false;
    s->nHeld--;
    s->freeQ.push_back(ticket);
  }
  s->cv.notify_all();
  return ORBFE_OK;
}

int orbfe_stream_stats(orbfe_stream* s, double out[4], int reset) {
  if (!s || !out) { set_err("NULL argument"); return ORBFE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(s->mu);
  out[0] = s->busySubmit; out[1] = s->busyCollect; out[2] = 0; out[3] = (double)s->nBatches;   // (out[2]: matching runs inside submit / collect)
  if (reset) { s->busySubmit = s->busyCollect = 0; s->nBatches = 0; }
  return ORBFE_OK;
}

int orbfe_stream_kernel_ms(orbfe_stream* s, double out_ms[5], long long* batches, long long* frames, int reset) {
  if (!s) { set_err("stream is NULL"); return ORBFE_ERR_INVALID; }
  double acc[5] = {0, 0, 0, 0, 0};
  long long b = 0, f = 0;
  for (auto* e : s->ext) {
    double ms[5];
    long long bb = 0, ff = 0;
    orbfe_debug_kernel_ms(e, ms, &bb, &ff, reset);
    for (int i = 0; i < 5; i++) acc[i] += ms[i];
    b += bb;
    f += ff;
  }
  if (out_ms) for (int i = 0; i < 5; i++) out_ms[i] = acc[i];
  if (batches) *batches = b;
  if (frames) *frames = f;
  return ORBFE_OK;
}

}  // extern "C"
