// orbfe_matcher_internal.h -- what the files built on the matcher handle share (orbfe_window.hip, orbfe_matcher.hip,
// orbfe_frame.hip, orbfe_bow.hip, orbfe_localmap.hip, orbfe_initscore.hip, orbfe_mprefresh.hip, orbfe_covis.hip, orbfe_culling.hip,
// orbfe_ransac.hip), none of it a kernel: the window kernel's parameter block and record format (namespace orbfe_match: a file
// that uses them says `using namespace orbfe_match`), the declarations of what these files ask of each other (namespace orbfe),
// and the matcher handle.  Buffer helpers: hip_buffers.h; the window kernel's launch width: window_plan.h.  Reference semantics:
// Frame::GetFeaturesInArea (src/Frame.cc:209-262) over the 64x48 grid (Frame.cc:114-129, 264-274), ORBmatcher.cc:1605-1621.
#pragma once
#include <hip/hip_runtime.h>

#include "orbfe_internal.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/orbfe.h"
#include "hip_buffers.h"
#include "window_plan.h"

using orbfe::set_err;

namespace orbfe_match {

constexpr int kGridCols = 64, kGridRows = 48;  // FRAME_GRID_COLS / FRAME_GRID_ROWS (Frame.h:36-37)
constexpr int TH_HIGH = 100, TH_LOW = 50, HISTO_LENGTH = 30;  // ORBmatcher.cc:37-39

// One "pair" = one train frame (grid-sorted keypoints + descriptors) and a run of queries against it.
struct PairInfo {
  int trainOff;    // first entry of the pair in sx/sy/soct/sidx
  int cellOff;     // first entry of the pair's cellStart table ([64*48+1] ints)
  int tdescOff;    // first descriptor row of the pair's train frame in tdesc
  float minX, minY, invW, invH;
};

struct MatchParams {
  // train frames, keypoints permuted into grid order (cell = ix*48+iy ascending, insertion order inside)
  const float* sx;
  const float* sy;
  const int* soct;
  const int* sidx;        // original keypoint index inside its frame
  const int* cellStart;   // per pair [64*48+1], values relative to the pair's trainOff
  const uint8_t* tdesc;   // descriptor rows in the same grid-sorted order as sx/sy/soct/sidx
  const PairInfo* pairs;
  // queries (all pairs concatenated)
  const int* qpair;       // pair of each query (nullptr: pair 0)
  const float* qx;
  const float* qy;
  const float* qr;        // < 0 : inactive query
  const int* qminL;
  const int* qmaxL;
  const uint8_t* qdesc;   // [nq][32]
  // indexed descriptor rows (a caller-maintained table, orbfe_search_by_projection_frame_rows): query q's descriptor is row
  // (qdescRow[q] & 0x7fffffff) of qdesc (bit 31 clear) or of qdescAlt (bit 31 set: the table's page-locked host mirror, for
  // rows the device copy has not received yet); nullptr: row q of qdesc
  const int* qdescRow = nullptr;
  const uint8_t* qdescAlt = nullptr;
  int nq;
  // outputs
  uint32_t* qcount;       // [nq]
  uint32_t* qoff;         // [nq] offset into pool
  uint32_t* pool;         // entries: idx | dist << 16, reference candidate order per query
  uint32_t poolCap;
  uint32_t* total;        // [1] pool entries claimed (may exceed poolCap: host retries with a larger pool)
  uint32_t* wpool = nullptr;   // wide records (resident-frame searches; sized for the worst case by the host)
  uint32_t* wtotal = nullptr;  // [1] words of it claimed
  // searches on a resident frame (orbfe_frame.hip) filter and annotate the candidates where they are produced, so the
  // bookkeeping kernel needs nothing but the entries themselves (per-candidate tests, independent of order):
  uint32_t* rec = nullptr;            // [nq][4]: {count | decision code << 16, entry 0, entry 1, entry 2}; lists of <= kRecEntries
                                      // live only here.  The decision code (below) tabulates the query's outcome for
                                      // every subset of its candidates being available, so the bookkeeping kernel's rounds are a
                                      // table lookup
  int codeMode = 0;                   // acceptance rule of the search: 0 SearchByProjection(MapPoints), 1 / 2 best <= maxDist
  float nnratio = 0.f;
  int maxDist = 0;
  const float* invSigma2 = nullptr;   // Fuse's gate e2 * mvInvLevelSigma2[octave] > chi2 (ORBmatcher.cc:896-903): dropped
  double chi2 = 0.0;
  int packOctave = 0;                 // entries carry the keypoint's octave in bits 25..30
  uint2* qword = nullptr;             // [nq] the record as the bookkeeping kernel keeps it in LDS: {idx0 | idx1 << 16, idx2 | code << 16};
                                      // lists beyond the record: {offset in the pool (of the wide record for four candidates),
                                      // count | kCodeWide / kCodeLongList << 16}
  // two small byte arrays of the page-locked query arena (claim flags, occupancy) reach the single-block bookkeeping kernel
  // as bit masks in device memory, packed by this kernel's many blocks on the way (64 flags per ballot)
  const uint8_t* bitSrc[2] = {nullptr, nullptr};
  unsigned long long* bitDst[2] = {nullptr, nullptr};
  int bitN[2] = {0, 0};
  uint8_t bitMask[2] = {0xff, 0xff};  // flag = (byte & mask) != 0
  int bitConst[2] = {-1, -1};         // >= 0: no source array, every flag has this value
  // raw queries: the kernel derives window and level range from the caller's own arrays (read in place when they are
  // page-locked) instead of from marshalled qx / qy / qr / qminL / qmaxL
  int rawKind = 0;                    // 0 marshalled; 1 SearchByProjection(F, MapPoints, th) (ORBmatcher.cc:55-73, 126-132);
                                      // 2 SearchByProjection(F, LastFrame / KeyFrame) from the projection on (:1353-1356, :1483-1485);
                                      // 3 the projected loops (radius given)
  const float* rawXY = nullptr;       // [nq][2]
  const int* rawLevel = nullptr;      // [nq]
  const float* rawAux = nullptr;      // kind 1: mTrackViewCos; kind 3: radius
  const uint8_t* rawFlags = nullptr;  // kind 1: ORBFE_MP_* bits; kinds 2, 3: valid
  const float* rawSf = nullptr;       // [32] mvScaleFactors in device memory
  float rawTh = 1.f;
  int rawFactor = 0;                  // kind 1: th != 1.0 (ORBmatcher.cc:49, 67-68)
};

// Decision codes.  Record (up to three candidates): 8 x 2 bits, field p = outcome when exactly the candidates of bit pattern p
// are available (bits beyond the count do not matter).  Wide record (N = four to six candidates): 2^N x 3 bits, eight
// patterns per word (word p >> 3, field p & 7).  Field 0 is always 0 (nothing available: no match).  Written by
// k_window_match (orbfe_window.hip), read by k_resolve (orbfe_frame.hip).
constexpr uint32_t kCodeLongList = 0xffffu;   // (field 0 of a real code is always 0) the list is longer than the record: read the pool
constexpr uint32_t kCodeWide = 0xfffeu;       // four to six candidates: entries in the pool, and in the wide pool a wide record
                                              // {idx0 | idx1 << 16, idx2 | idx3 << 16, idx4 | idx5 << 16, 2^N / 8 code words}
__host__ __device__ constexpr uint32_t wide_words(uint32_t n) { return 3u + (1u << (n - 3u)); }   // 5, 7, 11
constexpr int kRecEntries = 3;
constexpr int kWideMax = 6;

}  // namespace orbfe_match

struct orbfe_frame;
struct orbfe_matcher;
struct orbfe_local_map;
struct orbfe_extractor;

// ---- what the library's files ask of each other (each is defined once, in the file named) -------------------------------
namespace orbfe {
// orbfe_extractor.hip: one frame of the handle's last collected batch
int extractor_view(orbfe_extractor* h, int frame, ExtractView* out);

// orbfe_window.hip: k_window_match for the queries of M on stream `st` of the current device, as wide as the call's widest
// window in grid columns asks for (window_plan.h)
int launch_window_match(const orbfe_match::MatchParams& M, float widestCols, hipStream_t st);

// orbfe_frame.hip.  > 0: the kernels can read p in place (1: page-locked host memory, 2: memory of device `device`); 0: ordinary
// host memory (the caller copies it into a page-locked arena); -1: memory of another device
int gpu_readable(const void* p, int device);
// a resident frame's mnMinX, mnMaxX, mnMinY, mnMaxY; its octaves and angles in keypoint order and its largest octave; its
// undistorted coordinates in keypoint order; its descriptor rows in keypoint order (none of these waits) -- and the stream
// order behind the frame's build, for the kernels that read them
void frame_bounds(const orbfe_frame* f, float out[4]);
void frame_source_arrays(const orbfe_frame* f, const int** oct, const float** angle, int* maxOctave);
void frame_xy(const orbfe_frame* f, const float** x, const float** y);
const uint8_t* frame_descriptor_rows(const orbfe_frame* f);
void frame_wait_ready(orbfe_frame* f, hipStream_t st);
// the host-array searches of orbfe_matcher.hip run on a transient device-resident frame + GPU-side bookkeeping
int sbp_via_frame(orbfe_matcher* m, const OrbfeKeyPoint* kps_un, const uint8_t* desc, int n, const float bounds[4],
                  const float* scale_factors, int nlevels, const uint8_t* kp_occupied, const float* mp_proj_xy,
                  const int32_t* mp_level, const float* mp_viewcos, const uint8_t* mp_flags, const uint8_t* mp_desc, int n_mp,
                  float th, float nnratio, int32_t* kp_assigned, int* nmatches);
int sbp_uv_via_frame(orbfe_matcher* m, const OrbfeKeyPoint* kps_un, const uint8_t* desc, int n, const float bounds[4],
                     const float* scale_factors, int nlevels, const uint8_t* kp_occupied, const float* src_uv,
                     const int32_t* src_level, const float* src_angle, const uint8_t* src_flags, const uint8_t* src_valid,
                     const uint8_t* src_desc, int n_src, float th, int max_dist, int skip_any_occupied, int check_orientation,
                     int32_t* kp_assigned, int* nmatches);
int projected_via_frame(orbfe_matcher* m, const OrbfeKeyPoint* kps_un, const uint8_t* desc, int n, const float bounds[4], int n_src,
                        const float* src_uv, const float* src_radius, const int32_t* src_level, const uint8_t* src_valid,
                        const uint8_t* src_desc, const uint8_t* kp_skip, int claim, const float* inv_level_sigma2, int nlevels,
                        double chi2, int max_dist, int32_t* best_idx, int32_t* best_dist, int* nmatches);
// the three searches on queries that a projection kernel of orbfe_localmap.hip has left in device memory, earlier on the
// matcher's stream (the host reads none of the d_ arrays)
int sbp_frame_device_queries(orbfe_matcher* m, orbfe_frame* f, const float* scale_factors, int nlevels, const uint8_t* kp_occupied,
                             const float* d_xy, const int32_t* d_level, const float* d_viewcos, const uint8_t* d_flags,
                             const uint8_t* d_desc, const int32_t* d_desc_row, int n_mp, float th, float nnratio,
                             int32_t* kp_assigned, int* nmatches);
int sbp_uv_frame_device_queries(orbfe_matcher* m, orbfe_frame* f, const float* scale_factors, int nlevels, const uint8_t* kp_occupied,
                                const float* d_xy, const int32_t* d_level, const float* d_angle, const uint8_t* d_valid,
                                const uint8_t* d_claim, const uint8_t* d_desc, const int32_t* d_desc_row, int n_src, float th,
                                int max_dist, int skip_any_occupied, int check_orientation, int32_t* kp_assigned, int* nmatches);
int search_projected_frame_device_queries(orbfe_matcher* m, orbfe_frame* f, const float* scale_factors, int nlevels, float th,
                                          const float* d_xy, const int32_t* d_level, const float* d_radius, const uint8_t* d_valid,
                                          const uint8_t* d_desc, const int32_t* d_desc_row, int n_src, const uint8_t* kp_skip, int claim,
                                          const float* inv_level_sigma2, double chi2, int max_dist, int32_t* best_idx, int32_t* best_dist,
                                          int* nmatches);

// orbfe_localmap.hip: what orbfe_mprefresh.hip needs of a table -- its matcher, size, rows, and the slot of its own scratch
struct LocalMapView {
  orbfe_matcher* m;
  int capacity;
  uint8_t* table;
  std::shared_ptr<void>* scratch;   // owned by the map, released with it (its device is current then)
};
void local_map_view(orbfe_local_map* map, LocalMapView* v);

// orbfe_matcher.hip: the state of the host-array search (HostSearch::candidates) and the staging buffers of that file's calls
struct HostSearch;
}  // namespace orbfe
using orbfe::gpu_readable;

// The matcher handle: device, stream, what more than one file uses, and one scratch slot per file that keeps device-side
// state of its own (made on first use: scratch_in<T>() of hip_buffers.h, destroyed with the handle).
struct orbfe_matcher {
  int device = 0;
  hipStream_t stream = nullptr;
  std::shared_ptr<void> bow;   // scratch of orbfe_search_by_bow (orbfe_bow.hip)
  std::shared_ptr<void> initscore;   // scratch of orbfe_score_init_hypotheses* (orbfe_initscore.hip)
  std::shared_ptr<void> covis;   // scratch of orbfe_covisibility_counts (orbfe_covis.hip)
  std::shared_ptr<void> culling;   // scratch of orbfe_redundant_observations (orbfe_culling.hip)
  std::shared_ptr<void> ransac;   // scratch of orbfe_score_sim3_hypotheses / orbfe_score_pnp_hypotheses (orbfe_ransac.hip)
  orbfe::HostSearch* host = nullptr;   // orbfe_matcher.hip's; made by orbfe_matcher_create
  // the candidate pool of both kinds of search (host-array: orbfe_matcher.hip, resident frame: orbfe_frame.hip): the size
  // one kind has grown it to is the other's starting size
  DevBuf<uint32_t> d_pool;
  // searches on device-resident frames (orbfe_frame.hip): query arena, result / scratch words, the transient frame of
  // the host-array call forms, rounds the last k_resolve needed (< 0: finished by its serial pass)
  DevBuf<uint8_t> d_q;
  PinBuf<uint8_t> h_q;
  DevBuf<int> d_r;
  PinBuf<int> h_r;
  orbfe_frame* scratch = nullptr;
  int lastRounds = 0, lastResolveRoute = 0;   // route: 2 = tables + entries in LDS, 1 = tables in LDS, 0 = global scratch
  bool resolveAttr[3] = {false, false, false};   // dynamic-LDS attribute set (per matcher: one host thread per handle)
  DevBuf<uint32_t> d_wpool;      // wide records of the frame searches
  DevBuf<float> d_sf;            // raw queries: mvScaleFactors in device memory (and the host copy they were made from)
  float sfHost[32] = {};
  int sfN = -1;
  int seq = 0;                   // number of the last frame search (k_resolve reports it back through page-locked memory)
  // both kinds of search
  double tEntry = 0, tSynced = 0;   // frame searches: clock at the entry of the C call / when the results were seen
  double stageMs[4] = {0, 0, 0, 0};  // arena build, upload+kernel+download, (resolve: filled by callers), total
  static double nowMs() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  }
  ~orbfe_matcher();   // orbfe_matcher.hip
};
