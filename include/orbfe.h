/* orbfe.h -- C ABI of the MI355X-native ORB feature front end (liborbfe.so).
 *
 * Drop-in boundary for the per-frame hot path of AlejandroSilvestri/os1 (ORB-SLAM2 fork):
 * ORBextractor::operator() and the windowed Hamming searches of ORBmatcher.  Each entry point
 * names the reference interface it replaces (paths relative to the reference root).  The C++
 * host side in include/orbfe/ORBextractor.h and include/orbfe/orb_shim.hpp reproduces the ORB_SLAM2:: interfaces
 * on top of this ABI; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C, POD structs, caller-allocated outputs, no exceptions;
 *   - every function returns ORBFE_OK (0) or a negative error code; orbfe_last_error() returns a
 *     thread-local human-readable message for the last failure on the calling thread;
 *   - a handle is single-threaded (like the reference's ORBextractor instance, which mutates
 *     mvImagePyramid and is only ever called from the Tracking thread); use one handle per
 *     GPU / host thread;
 *   - there is NO CPU fallback: if no gfx950 device is usable, create() fails with
 *     ORBFE_ERR_NO_DEVICE.
 */
#ifndef ORBFE_H_
#define ORBFE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBFE_OK 0
#define ORBFE_ERR_INVALID (-1)   /* bad argument (null pointer, non-positive size, cap too small) */
#define ORBFE_ERR_NO_DEVICE (-2) /* no usable HIP device / wrong architecture                      */
#define ORBFE_ERR_HIP (-3)       /* a HIP runtime call failed; see orbfe_last_error()              */
#define ORBFE_ERR_TOO_SMALL (-4) /* image too small: some pyramid level has <1 FAST cell column/row
                                    (the reference divides by zero there, ORBextractor.cc:820-823) */
#define ORBFE_ERR_OVERFLOW (-5)  /* an output capacity was exceeded (outputs truncated)            */
#define ORBFE_ERR_UNSUPPORTED (-6) /* the request is valid but this library has no bit-exact GPU form of it */

/* Same 28-byte layout as cv::KeyPoint: pt.x, pt.y, size, angle, response, octave, class_id. */
typedef struct OrbfeKeyPoint {
  float x, y;      /* pt, in level-0 pixel units (level coords * scale, ORBextractor.cc:959-965) */
  float size;      /* (float)(int)(31 * scale[octave])                    (ORBextractor.cc:879,888) */
  float angle;     /* IC-angle in degrees [0,360)                         (ORBextractor.cc:86-113)  */
  float response;  /* FAST score                                                                    */
  int32_t octave;  /* pyramid level                                                                 */
  int32_t class_id; /* always -1                                                                    */
} OrbfeKeyPoint;

typedef struct orbfe_extractor orbfe_extractor;
typedef struct orbfe_matcher orbfe_matcher;
typedef struct orbfe_vocabulary orbfe_vocabulary;   /* bag-of-words section below */
typedef struct orbfe_kfdb orbfe_kfdb;               /* keyframe database section below */

const char* orbfe_last_error(void);
/* Number of visible HIP devices (0 if none / runtime unusable). Does not create a context. */
int orbfe_device_count(void);

/* Device-memory helpers so a caller without its own HIP code can keep frames resident in HBM
 * (orbfe_extract_batch with in_device_memory != 0).  Plain hipMalloc/hipFree/hipMemcpy/
 * hipDeviceSynchronize on the given device. */
int orbfe_device_malloc(int device_id, size_t bytes, void** out);
int orbfe_device_free(int device_id, void* ptr);
int orbfe_device_upload(int device_id, void* dst_device, const void* src_host, size_t bytes);
int orbfe_device_synchronize(int device_id);
/* Page-locked host memory for frames handed over in HOST memory (in_device_memory == 0): a frame that
 * lives in such a buffer is copied by DMA straight from it while earlier batches compute; a frame in
 * ordinary pageable memory is staged by the HIP runtime first (blocking the caller; 18 k vs 25 k frames/s at
 * 1080p end to end).  hipHostMalloc /
 * hipHostFree.  A cv::Mat can wrap the buffer (Mat(rows, cols, CV_8UC1, ptr, step)) so the camera/decoder
 * writes into it directly. */
int orbfe_host_alloc(size_t bytes, void** out);
int orbfe_host_free(void* ptr);
/* The same for a buffer the caller already owns (a capture ring, a decoder's output, the data of a long-lived cv::Mat): page-locks
 * [ptr, ptr + bytes) and maps it for the GPU (hipHostRegister); frames inside it then take the page-locked route -- for the one-frame
 * call of Frame.cc:133 that is 0.15 ms instead of 0.19 ms at 1080p.  Registering costs hundreds of microseconds: do it once per
 * buffer, not per frame, and unregister BEFORE the memory is freed (a freed-and-reallocated range that is still registered would be
 * read through its old pages). */
int orbfe_host_register(void* ptr, size_t bytes);
int orbfe_host_unregister(void* ptr);
/* NUMA placement for multi-GPU hosts (one process or thread group per GPU): the NUMA node the
 * device hangs off (sysfs numa_node of its PCI function; -1 = unknown), and a helper that restricts the CALLING
 * thread to that node's CPUs (intersected with its current mask).  Threads created and page-locked buffers first
 * touched afterwards -- the stream runner's workers, orbfe_host_alloc memory -- then live next to the GPU.
 * Returns the number of CPUs in the new mask, 0 if nothing was changed (node unknown). */
int orbfe_device_numa_node(int device_id);
int orbfe_bind_thread_to_device(int device_id);
/* Host-to-device link rate seen by `reps` back-to-back copies of `bytes` from `host` (page-locked for a DMA figure),
 * in GB/s: the bound of any caller that hands over host frames (bench.py's pcie_inclusive leg). */
int orbfe_debug_h2d_rate(int device_id, const void* host, size_t bytes, int reps, double* gb_per_s);

/* ---------------------------------------------------------------------------------------------
 * Extractor.  Replaces ORB_SLAM2::ORBextractor (include/ORBextractor.h:155-373).
 * ------------------------------------------------------------------------------------------- */

/* ORBextractor::ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
 * int minThFAST)  (include/ORBextractor.h:164-165, src/ORBextractor.cc:442-502).
 * device_id: HIP device ordinal the handle is bound to. */
int orbfe_extractor_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                           int device_id, orbfe_extractor** out);
void orbfe_extractor_destroy(orbfe_extractor* h);

/* GetLevels / GetScaleFactor (include/ORBextractor.h:194-207). */
int orbfe_extractor_levels(const orbfe_extractor* h);
int orbfe_extractor_device(const orbfe_extractor* h);   /* the device_id given at creation; -1 for NULL */
float orbfe_extractor_scale_factor(const orbfe_extractor* h);
/* GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 * (include/ORBextractor.h:213-239).  Each output has nlevels floats; any may be NULL. */
int orbfe_extractor_scale_tables(const orbfe_extractor* h, float* scale, float* inv_scale, float* sigma2,
                                 float* inv_sigma2);
/* mnFeaturesPerLevel (src/ORBextractor.cc:467-478); nlevels ints. */
int orbfe_extractor_features_per_level(const orbfe_extractor* h, int32_t* out);
/* Upper bound on keypoints one frame can return: sum over levels of max(N_l + 2, 16) -- a level overshoots its quota
 * N_l by at most 2, but DistributeOctTree divides every root node once before it looks at N_l (src/ORBextractor.cc:
 * 620-700), so a level with a tiny quota still returns up to 4 * roots keypoints (roots = round(width/height) <= 4
 * for aspect ratios below 4.5; wider strips are reported with ORBFE_ERR_OVERFLOW if they exceed `cap`).  Equals
 * nfeatures + 2*nlevels whenever every N_l >= 14.  Size `cap` with it. */
int orbfe_extractor_max_keypoints(const orbfe_extractor* h);
/* The same bound for a given image size (exact number of quadtree roots per level): needed only for strips wider
 * than 4.5 : 1 or to size buffers tightly. */
int orbfe_extractor_max_keypoints_for_size(const orbfe_extractor* h, int rows, int cols);

/* How orbfe_extract_batch_collect* (and the blocking calls built on it) wait for the GPU.  poll_us = 0 (default): the
 * runtime's own wait, which spins -- lowest latency, one busy host core per waiting thread.  poll_us > 0: poll the
 * stream and sleep poll_us microseconds between polls; the result arrives up to poll_us later and the core is free in
 * between.  The stream runner (orbfe_stream_*) sets 50 on its handles (ORBFE_POLL_WAIT_US overrides): with several
 * batches in flight the delay is hidden and a rank of a multi-GPU run needs 1.5 instead of 2 host cores.  Not allowed
 * between a submit and its collect. */
int orbfe_extractor_set_wait_mode(orbfe_extractor* h, int poll_us);

/* Colour input (Tracking::GrabImageMonocular, src/Tracking.cc:96-109: cvtColor(RGB2GRAY / BGR2GRAY) on 3- and
 * 4-channel images before the Frame is built).  After this call `gray` in the extract calls points to interleaved
 * 8-bit pixels of the given format (stride in bytes, cols in pixels); the conversion runs on the GPU in front of the
 * pyramid: gray = (R*cr + G*cg + B*cb + half) >> shift, alpha ignored -- OpenCV's 8-bit RGB2Gray with 15-bit
 * coefficients {9798, 19235, 3735} (ORBFE_GRAY_Q15, OpenCV >= 4.1.1) or 14-bit {4899, 9617, 1868}
 * (ORBFE_GRAY_Q14, earlier releases). */
enum { ORBFE_INPUT_GRAY8 = 0, ORBFE_INPUT_RGB8 = 1, ORBFE_INPUT_BGR8 = 2, ORBFE_INPUT_RGBA8 = 3, ORBFE_INPUT_BGRA8 = 4 };
enum { ORBFE_GRAY_Q15 = 0, ORBFE_GRAY_Q14 = 1 };
int orbfe_extractor_set_input_format(orbfe_extractor* h, int format, int gray_variant);

/* Which cv::GaussianBlur(7x7, sigma 2) the descriptors are sampled from (src/ORBextractor.cc:949-950 -- it decides every descriptor
 * bit).  OpenCV's 8-bit path is 8.8 fixed point; the taps depend on the release the reference was BUILT with (nothing in the
 * reference pins it: .cproject:40 names "opencv4", README.md:18 dates the project Feb 2019 = the 4.0.x era):
 *   ORBFE_GAUSS_ED       [18,34,48,56,48,34,18] / 256, rounding error diffused so that the taps add up to 256 -- OpenCV >= 4.1.1
 *                        (and 3.4.7+); the default;
 *   ORBFE_GAUSS_ROUNDED  [18,34,49,55,49,34,18] (sum 257), every tap rounded on its own, and the saturating final cast that
 *                        arithmetic needs: min(255, (sum + 32768) >> 16) -- OpenCV 4.0.0 - 4.1.0 (and 3.4.2 - 3.4.6).
 * Both are restated from upstream from memory (parity unpinned); tests/test_opencv_live.py picks the expected one
 * from cv2.__version__ wherever an OpenCV exists.  The environment variable ORBFE_GAUSS_VARIANT=0|1 presets it for every
 * extractor created afterwards (for a caller that cannot be recompiled). */
enum { ORBFE_GAUSS_ED = 0, ORBFE_GAUSS_ROUNDED = 1 };
int orbfe_extractor_set_blur_variant(orbfe_extractor* h, int variant);

/* void ORBextractor::operator()(InputArray image, InputArray mask, vector<KeyPoint>& keypoints,
 *                               OutputArray descriptors)
 * (include/ORBextractor.h:185-187, src/ORBextractor.cc:907-969).
 *   gray/rows/cols/stride_bytes : CV_8UC1 image in HOST memory (mask is ignored by the reference);
 *   kps  [cap]                  : keypoints, level-major, quadtree list order inside a level;
 *   desc [cap*32]               : descriptors, row i belongs to kps[i] (CV_8U, 32-byte rows);
 *   *n_out                      : number of keypoints produced.
 * rows==0 || cols==0 || gray==NULL: returns ORBFE_OK with *n_out = 0 and outputs untouched
 * (the reference returns silently, ORBextractor.cc:910-911). */
int orbfe_extract(orbfe_extractor* h, const uint8_t* gray, int rows, int cols, size_t stride_bytes,
                  OrbfeKeyPoint* kps, uint8_t* desc, int cap, int* n_out);

/* Batched form of the same call for independent frames of one size (throughput path: one
 * kernel launch sequence for all frames).  gray[i] points to frame i; in_device_memory != 0
 * means the frame pointers are DEVICE pointers on the handle's GPU (frames already resident in
 * HBM).  kps: nframes*cap entries, desc: nframes*cap*32 bytes, n_out: nframes ints.
 * A device frame is read in place, at any byte alignment of pointer and stride (a ROI of a
 * larger device image is fine) and needs no padding: the kernels read whole aligned dwords, so
 * besides the pixels they touch at most the 3 bytes that share a dword with a frame's first
 * pixel and the 3 that share one with the last pixel of its last row, and up to 15 bytes behind
 * the last pixel of every other row (the stride's padding or the next row).  None of those
 * bytes reaches a result. */
int orbfe_extract_batch(orbfe_extractor* h, int nframes, const uint8_t* const* gray, int in_device_memory,
                        int rows, int cols, size_t stride_bytes, OrbfeKeyPoint* kps, uint8_t* desc, int cap,
                        int* n_out);

/* Asynchronous form of orbfe_extract_batch: _submit enqueues the whole extractor for the batch on the
 * handle's stream and returns at once; _collect waits for it and fills the outputs exactly as
 * orbfe_extract_batch does.  One batch may be outstanding per handle; the frames (and, for host input,
 * the host buffers) must stay valid until _collect returns.  Lets a caller overlap the GPU extraction of
 * batch k+1 with the matching of batch k.  (A geometry outside the GPU quadtree's limits -- a strip wider than
 * 4.5 : 1, more than 2 044 features on a level -- is selected by the host quadtree inside _submit, which then
 * returns only when pyramid, FAST and compaction have run: same results and the same calls, less overlap.) */
int orbfe_extract_batch_submit(orbfe_extractor* h, int nframes, const uint8_t* const* gray, int in_device_memory,
                               int rows, int cols, size_t stride_bytes);
int orbfe_extract_batch_collect(orbfe_extractor* h, OrbfeKeyPoint* kps, uint8_t* desc, int cap, int* n_out);
/* Waits until the GPU has finished the submitted batch WITHOUT collecting it: a pipelined caller submits its next batch on another
 * handle between this call and the collect, so that the host-side assembly of the results (0.25 ms for 64 1080p frames) does not
 * leave a gap in the GPU's queue (the stream runner does; orbfe_stream_*).  The collect call that follows returns without waiting. */
int orbfe_extract_batch_wait(orbfe_extractor* h);

/* Extraction + GPU-resident matching for consecutive frames of ONE stream.  A chain carries the predecessor
 * (the previous batch's last frame, kept in HBM) across batches; the batches of a stream may alternate between
 * extractor handles of identical configuration on the same device, but must be submitted in stream order.
 * _submit_matched = orbfe_extract_batch_submit followed, on the GPU, by
 *   ORBmatcher(nnratio, check_orientation).SearchForInitialization(F1 = predecessor, F2 = frame,
 *       vbPrevMatched := F1's keypoints (Tracking.cc:355-357), vnMatches12, window_size)   (ORBmatcher.cc:400-515)
 * for every frame of the batch, reading keypoints, angles and descriptors straight from the extractor's result
 * arena.  _collect_matched additionally returns matches12 [nframes][cap] (row f = vnMatches12 of frame f, indexed
 * by the predecessor's keypoints, -1 = none) and nmatches [nframes] (0 for a stream's very first frame). */
typedef struct orbfe_sfi_chain orbfe_sfi_chain;
int orbfe_sfi_chain_create(const orbfe_extractor* h, orbfe_sfi_chain** out);
void orbfe_sfi_chain_destroy(orbfe_sfi_chain* c);
/* isolated != 0: every batch submitted with this chain stands alone -- its first frame has no predecessor (its match vector is all -1,
 * its count 0) and its last frame is not handed on.  For callers that deal the batches of ONE stream to several devices and match the
 * boundary pairs themselves (orbfe_stream_multi_*). */
int orbfe_sfi_chain_set_isolated(orbfe_sfi_chain* c, int isolated);
/* The next batch submitted with this chain has no predecessor in the chain (its first frame reports no match); its last frame is handed
 * on as usual.  For callers whose stream went on without the chain (a batch extracted unmatched, another geometry or route): they
 * match that first frame themselves. */
int orbfe_sfi_chain_restart(orbfe_sfi_chain* c);
int orbfe_extract_batch_submit_matched(orbfe_extractor* h, orbfe_sfi_chain* chain, int nframes, const uint8_t* const* gray,
                                       int in_device_memory, int rows, int cols, size_t stride_bytes, const float bounds[4],
                                       int window_size, float nnratio, int check_orientation);
int orbfe_extract_batch_collect_matched(orbfe_extractor* h, OrbfeKeyPoint* kps, uint8_t* desc, int cap, int* n_out,
                                        int32_t* matches12, int* nmatches);

/* Frame::UndistortKeyPoints (Frame.cc:284-319) on the GPU: a kernel behind the descriptor kernel restates
 * cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) in IEEE double, bit for bit what orbfe_undistort_pinhole computes on the
 * host, on the level-scaled keypoint positions.  dist = k1 k2 p1 p2 [k3 [k4 k5 k6]], ndist <= 8.
 *   camera_mode 0 with (ndist == 0 or dist[0] == 0): the reference's identity case (Frame.cc:288, whatever the other coefficients
 *     are): the handle behaves exactly like one without a camera -- nothing is launched or allocated, xy_un equals the keypoints.
 *   camera_mode 1 (os1's equidistant fisheye): ORBFE_ERR_UNSUPPORTED, the handle stays as it was.  That model needs the host libm's
 *     double tan bit for bit; orbfe_extractor_set_camera_equidistant (below) is the GPU route for it, orbfe_undistort_equidistant
 *     the host function.
 * With a distorting camera set
 *   - orbfe_extract_undistorted / orbfe_extract_batch_collect_undistorted also return mvKeysUn: xy_un [nframes][cap][2] floats, row f
 *     = frame f in keypoint order (matches12 / nmatches of _collect_undistorted: as _collect_matched, or both NULL);
 *   - orbfe_extract_batch_submit_matched searches on mvKeysUn: PosInGrid, the window's cell range and box test and vbPrevMatched
 *     (:= F1's mvKeysUn) all take the undistorted float coordinates; `bounds` stays the caller's (orbfe_compute_image_bounds).  A
 *     chain whose previous batch was matched without the camera (or the other way round) starts over, as after _chain_restart.
 * May only be called while no batch is submitted.  orbfe_extractor_undistort runs the kernel with the handle's coefficients on n
 * caller points, in place: the batched form of orbfe_undistort_pinhole.  Like that function it is cv::undistortPoints and NOT
 * Frame::UndistortKeyPoints: it ignores the dist[0] == 0 short-cut of Frame.cc:288 and applies k2, p1, ... of an "identity" camera,
 * where the extraction calls of the same handle return xy_un == xy.  A caller that wants the short-cut skips the call. */
int orbfe_extractor_set_camera(orbfe_extractor* h, int camera_mode, float fx, float fy, float cx, float cy, const float* dist,
                               int ndist);
int orbfe_extractor_undistort(orbfe_extractor* h, float* xy, int n);

/* os1's equidistant fisheye model (Frame::antidistorsionarProyeccionEquidistante, Frame.cc:355-384) on the GPU.  The reference's
 * std::tan is not correctly rounded and cannot be restated; its result is rounded to float, though.  The kernel encloses tan with a
 * proved bound and checks whether every double a libm with an error below 1 ULP could return gives the same two floats: it then
 * writes them (bit for bit the reference's on any such libm).  The few points where they differ (measured 7.3e-8 per point, 3.6e-8 per coordinate) are recomputed
 * with orbfe_undistort_equidistant on the host when the call returns or the batch is collected, and patched into the results: xy_un,
 * the arena a resident frame is built from, and -- for a matched batch -- the match rows, which are then searched again on the host.
 * Otherwise the handle behaves as one with a distorting pinhole camera: orbfe_extractor_undistort, orbfe_extract_undistorted,
 * _collect_undistorted, _submit_matched and orbfe_frame_create_from_extract work unchanged.  Only while no batch is submitted.  A match
 * chain whose previous batch was undistorted by another model, or by an equidistant camera with other intrinsics, starts over.
 *   orbfe_extractor_undistort_verdict: the kernel's raw output for n points, nothing settled -- out [n][2]; undecided[i] = 1: the
 *     host would settle point i (out holds the lowest candidate's floats, or the input when theta is outside (1e-8, 1.5]).
 *   orbfe_extractor_equidistant_stats: stats[0] points settled on the host, [1] points whose value changed, [2] match rows redone. */
int orbfe_extractor_set_camera_equidistant(orbfe_extractor* h, float fx, float fy, float cx, float cy);
int orbfe_extractor_undistort_verdict(orbfe_extractor* h, const float* xy, int n, float* out, uint8_t* undecided);
int orbfe_extractor_equidistant_stats(const orbfe_extractor* h, long long stats[3]);
int orbfe_extract_undistorted(orbfe_extractor* h, const uint8_t* gray, int rows, int cols, size_t stride_bytes, OrbfeKeyPoint* kps,
                              uint8_t* desc, int cap, int* n_out, float* xy_un);
int orbfe_extract_batch_collect_undistorted(orbfe_extractor* h, OrbfeKeyPoint* kps, uint8_t* desc, int cap, int* n_out, float* xy_un,
                                            int32_t* matches12, int* nmatches);

/* Stage accessors for the parity tests (state of the LAST extract call, frame index in batch). */
int orbfe_debug_level_size(const orbfe_extractor* h, int level, int* w, int* hgt);
int orbfe_debug_level_copy(orbfe_extractor* h, int frame, int level, uint8_t* out /* w*h, tight */);
/* FAST candidates of one level BEFORE the quadtree, reference order (cell-row-major, row-major in
 * a cell): triples (x, y, score) with x,y relative to (minBorderX,minBorderY) = (16,16) as in
 * vToDistributeKeys (ORBextractor.cc:861-866). */
int orbfe_debug_candidates(orbfe_extractor* h, int frame, int level, int32_t* xys, int cap, int* n_out);
/* Host wall-clock milliseconds of the last collected batch: [0]=enqueue (the submit call), [1]=GPU wait inside the
 * collect call, [2]=host selection -- 0 unless the host quadtree selected the batch (geometries outside the GPU
 * quadtree's limits, ORBFE_HOST_QUADTREE=1): then the wait for pyramid+FAST+compaction, the candidate D2H, the
 * quadtrees and the upload of the selection, all of which happen inside the submit call and are part of [0] too --
 * [3]=output assembly (with the host-side matching of a host-selected batch), [4]=total. */
int orbfe_debug_stage_ms(const orbfe_extractor* h, float out[5]);
/* GPU time (HIP events recorded on the launch stream) accumulated per kernel group since the last
 * reset: out_ms[0]=pyramid (k_resize x (nlevels-1)), [1]=k_fast_tasks, [2]=k_compact,
 * [3]=k_describe, [4]=k_quadtree; *batches = launches of each group, *frames = frames processed. */
int orbfe_debug_kernel_ms(orbfe_extractor* h, double out_ms[5], long long* batches, long long* frames, int reset);
/* k_fast_tasks (the dominant kernel) is timed in every call of MORE than ORBFE_CONE_MAX_FRAMES (default 2) frames;
 * calls with one or two frames take the latency route, which records no events (each costs a dependent-launch gap),
 * so orbfe_debug_kernel_ms reports frames = 0 for them.  enable != 0 also times the other groups, at the price of an
 * event (a few microseconds of stream gap) between them. */
int orbfe_debug_set_profiling(orbfe_extractor* h, int enable);
/* Measurement only: needs a library built with `make EXPERIMENTS=1` (-DORBFE_EXPERIMENTS) and ORBFE_FAST_ABLATE=4 in the environment,
 * which selects an instantiation of the FAST kernel with s_memtime stamps between its phases (a default build returns ORBFE_ERR_INVALID): shader
 * cycles summed over every wave since the last reset -- [0] entry -> geometry known, [1] -> ROI in LDS, [2] -> pre-test done,
 * [3] -> scores done, [4] -> end, [5] = waves counted.  tools/fast_phases.py prints the per-wave averages. */
int orbfe_debug_fast_stamps(orbfe_extractor* h, unsigned long long out[8], int reset);
/* Measurement only (a `make EXPERIMENTS=1` build with ORBFE_SFI_DEBUG=1 in the environment when the process starts; a default build
 * reports no records): one record of 8 ints per pair the GPU-resident
 * SearchForInitialization resolved since the last reset -- frame in its batch, rounds of the fixed point, candidate entries, 1 if
 * the serial finish ran, shader cycles of the block, n1, n2, 1 if the candidate pool fitted LDS (tools/sfi_rounds.py). */
int orbfe_debug_sfi_records(orbfe_extractor* h, int32_t* out, int cap_records, int* n_out, int reset);
/* Device-side restatement of (cosf, sinf)(angle_deg * pi/180) used by the rBRIEF kernel, evaluated
 * on the GPU for n angles (parity test against host libm). */
int orbfe_debug_sincos(orbfe_extractor* h, const float* angle_deg, int n, float* cos_out, float* sin_out);

/* Host-only test hooks (no GPU needed): the product's own quadtree (DistributeOctTree,
 * src/ORBextractor.cc:571-795) on candidate triples (x, y relative to (minX,minY); score), returning
 * the indices of the retained candidates in list order; and the (cosf,sinf) restatement compiled
 * for the host, compared against libm over the float bit patterns [lo_bits, hi_bits] step `step`
 * (returns the number of mismatching values in *mismatches). */
int orbfe_debug_quadtree(const int16_t* x, const int16_t* y, const uint8_t* score, int n, int min_x, int max_x,
                         int min_y, int max_y, int n_target, int32_t* out_idx, int cap, int* n_out);
int orbfe_debug_sincos_host_check(uint32_t lo_bits, uint32_t hi_bits, uint32_t step, long long* mismatches);
/* The device restatement of glibc logf (the one orbfe_project_local_map uses in PredictScale) evaluated on the GPU of
 * matcher m for n inputs, and its host build compared against the host libm over the float bit patterns [lo_bits, hi_bits]
 * step `step` (*mismatches = values whose bits differ). */
int orbfe_debug_logf(orbfe_matcher* m, const float* x, int n, float* out);
int orbfe_debug_logf_host_check(uint32_t lo_bits, uint32_t hi_bits, uint32_t step, long long* mismatches);

/* ---------------------------------------------------------------------------------------------
 * Stream runner (throughput path; no counterpart class in the reference, whose Tracking thread drives
 * ORBextractor / ORBmatcher one frame at a time -- System.cc:115-152, Tracking.cc:92-121,344-419).
 * A stream owns `depth` extractor handles on one GPU and one native worker thread, the extract worker:
 * batches pushed with orbfe_stream_push are extracted (asynchronous submit/collect, `depth` batches in
 * flight) and every frame is matched against its predecessor in the stream with
 * SearchForInitialization (vbPrevMatched := predecessor keypoints, as Tracking.cc:355-357), chained
 * behind the extraction on the GPU; results come back in push order from orbfe_stream_pop.  A frame 0
 * whose predecessor that chain does not hold is matched with orbfe_search_for_initialization on a
 * matcher the stream creates when it first needs one.  Identical results to calling orbfe_extract_batch
 * and orbfe_search_for_initialization frame by frame.
 * ------------------------------------------------------------------------------------------- */
typedef struct orbfe_stream orbfe_stream;
/* PREDECESSOR CONTRACT (orbfe_stream_* and orbfe_stream_multi_*).  Frame 0 of a batch is matched against the last frame pushed before
 * it, whatever that frame's size, whichever route (GPU or host quadtree) either batch took, and whether or not matching was on for that
 * batch.  Three exceptions, where frame 0 reports nmatches 0 and a matches12 row of -1 only: (a) the runner's first batch; (b) every
 * batch pushed while isolated batches are on; (c) the first batch after isolated batches are switched off.  Within a batch, frame i is
 * matched against frame i - 1.  A batch pushed while matching is off reports nmatches 0 and matches12 -1 for every frame.
 * A held result (orbfe_stream_pop_hold) stays valid and unchanged until it is released; while any ticket is held, orbfe_stream_pop,
 * the _set_* calls, orbfe_stream_set_queue_slots and a push that would grow orbfe_stream_capacity return ORBFE_ERR_INVALID, and so
 * does a release of a ticket that is not held.
 * A runner is created with matching on (window 100) and EMPTY image bounds: a push before orbfe_stream_set_matching has given it
 * bounds with maxX > minX and maxY > minY (or a window of 0) returns ORBFE_ERR_INVALID, as does any search handed empty bounds. */
/* batch = frames per push; depth = extraction batches in flight (1..8).
 * HARDWARE QUEUES: each batch in flight has its own HIP stream and the HIP runtime folds a process's streams onto GPU_MAX_HW_QUEUES
 * hardware queues (4 unless the ENVIRONMENT variable said otherwise before the process's first HIP call: the runtime reads it once,
 * a library cannot set it for its host process; bench.py sets 8 before importing torch).  Two streams that share a queue serialise,
 * so the runner measures at creation how many of its streams run side by side (about a millisecond) and keeps that many batches
 * in flight: 3 in a process with the default 4 queues (0.97 of the rate of depth 4 on 8 queues), `depth` where the queues are there.
 * orbfe_stream_batches_in_flight reports the number; a line on stderr says so once (ORBFE_QUIET=1 silences it). */
int orbfe_stream_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device_id,
                        int batch, int depth, orbfe_stream** out);
/* Batches the GPU is working on are waited for; batches still queued are dropped without being submitted.  Frames of
 * submitted batches must stay valid until destroy returns (or pop every batch first). */
void orbfe_stream_destroy(orbfe_stream* s);
/* bounds = {mnMinX, mnMaxX, mnMinY, mnMaxY}; window_size <= 0 disables matching (extract only).  Only while no
 * batch is in flight (every pushed batch popped); each batch carries the parameters in force at its push. */
int orbfe_stream_set_matching(orbfe_stream* s, const float bounds[4], int window_size, float nnratio,
                              int check_orientation);
/* isolated != 0: frame 0 of every pushed batch has no predecessor (orbfe_sfi_chain_set_isolated on the runner's chain); only while
 * no batch is in flight. */
int orbfe_stream_set_isolated_batches(orbfe_stream* s, int isolated);
int orbfe_stream_batches_in_flight(const orbfe_stream* s);
/* orbfe_stream_pop without the "valid until the next pop" rule: the result stays valid until orbfe_stream_release(s, *ticket).  Any
 * number of results may be held; each keeps one of the runner's result slots (orbfe_stream_queue_slots) busy, and a push waits while no
 * slot is free.  Do not mix with orbfe_stream_pop on the same runner (orbfe_stream_pop is refused while a result is held). */
int orbfe_stream_pop_hold(orbfe_stream* s, const OrbfeKeyPoint** kps, const uint8_t** desc, const int** n_kps, const int32_t** matches12,
                          const int** nmatches, int* ticket);
int orbfe_stream_release(orbfe_stream* s, int ticket);
/* orbfe_extractor_set_input_format for every extractor of the runner (only while no batch is in flight). */
int orbfe_stream_set_input_format(orbfe_stream* s, int format, int gray_variant);
/* orbfe_extractor_set_blur_variant for every extractor of the runner (only while no batch is in flight). */
int orbfe_stream_set_blur_variant(orbfe_stream* s, int variant);
/* orbfe_extractor_set_vocabulary for every extractor of the runner (only while no batch is in flight); afterwards
 * orbfe_stream_bow_raw returns, for frame `frame` of the LAST POPPED batch, the per-keypoint (leaf node, level node)
 * pairs (pointers into the runner's buffers, valid until the next pop; feed them to orbfe_bow_assemble). */
int orbfe_stream_set_vocabulary(orbfe_stream* s, orbfe_vocabulary* v, int levelsup);
int orbfe_stream_bow_raw(orbfe_stream* s, int frame, const uint32_t** leaf_node, const uint32_t** level_node, int* n);
/* orbfe_extractor_set_camera for every handle of the runner (only while no batch is in flight or held; an unsupported model changes
 * nothing).  Streamed frames are then matched on mvKeysUn, and the frame pushed next has no predecessor.  orbfe_stream_xy_un returns
 * mvKeysUn of the LAST POPPED batch, [batch][orbfe_stream_capacity][2] floats, valid until the next pop. */
int orbfe_stream_set_camera(orbfe_stream* s, int camera_mode, float fx, float fy, float cx, float cy, const float* dist, int ndist);
/* orbfe_extractor_set_camera_equidistant for every handle of the runner (same rules), and the handles' counters summed. */
int orbfe_stream_set_camera_equidistant(orbfe_stream* s, float fx, float fy, float cx, float cy);
int orbfe_stream_equidistant_stats(orbfe_stream* s, long long stats[3]);
int orbfe_stream_xy_un(orbfe_stream* s, const float** xy_un);
/* Per-frame output capacity (keypoints) of the arrays returned by orbfe_stream_pop = their row stride.  It grows when a
 * push brings frames of a geometry that can return more keypoints (orbfe_extractor_max_keypoints_for_size); such a push
 * is only accepted while no batch is in flight or held. */
int orbfe_stream_capacity(const orbfe_stream* s);
/* Result slots of the runner = batches that can be pushed ahead of the pops before orbfe_stream_push blocks, plus 2
 * (one is in the caller's hands after a pop, one is being filled).  Default depth+4; a caller whose own thread may be
 * held up for milliseconds asks for more (only while no batch is in flight; the number never shrinks;
 * depth+2 <= nslots <= 256).  A caller must never push more than orbfe_stream_queue_slots()-2 batches ahead of its
 * pops from the popping thread: no slot could become free and the push would wait forever. */
int orbfe_stream_set_queue_slots(orbfe_stream* s, int nslots);
int orbfe_stream_queue_slots(const orbfe_stream* s);
/* Enqueue one batch (`batch` frame pointers; device pointers if in_device_memory != 0).  Returns at once unless every
 * result slot is taken (see orbfe_stream_set_queue_slots).  The frames must stay valid until their batch is popped. */
int orbfe_stream_push(orbfe_stream* s, const uint8_t* const* gray, int in_device_memory, int rows, int cols,
                      size_t stride_bytes);
/* Wait for the oldest batch; ORBFE_ERR_INVALID if no pushed batch is outstanding.  Output pointers stay valid until
 * the next pop:
 *   kps [batch][cap], desc [batch][cap][32], n_kps [batch];
 *   matches12 [batch][cap]: row i = vnMatches12 of (F1 = frame i-1 of the stream, F2 = frame i), indexed by
 *   F1's keypoints (first n_kps[i-1] entries valid; row 0 uses the last frame of the previous batch);
 *   nmatches [batch]: return values of the searches (0 for the very first frame of the stream). */
int orbfe_stream_pop(orbfe_stream* s, const OrbfeKeyPoint** kps, const uint8_t** desc, const int** n_kps,
                     const int32_t** matches12, const int** nmatches);
/* Host wall-clock ms the extract worker spent in submit / collect calls (incl. waiting for the GPU), and the number of
 * finished batches, since the last reset: out = {submit, collect, match, batches}.  Matching runs inside submit / collect,
 * so out[2] is always 0 (the slot is kept for ABI compatibility). */
int orbfe_stream_stats(orbfe_stream* s, double out[4], int reset);
/* Sum of orbfe_debug_kernel_ms over the stream's extractor handles. */
int orbfe_stream_kernel_ms(orbfe_stream* s, double out_ms[5], long long* batches, long long* frames, int reset);

/* ---------------------------------------------------------------------------------------------
 * Matcher.  Replaces the hot subset of ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:71-270).
 * ------------------------------------------------------------------------------------------- */

/* static int ORBmatcher::DescriptorDistance(const cv::Mat&, const cv::Mat&)
 * (include/ORBmatcher.h:74, src/ORBmatcher.cc:1605-1621): Hamming distance of two 256-bit rows.
 * Scalar host helper (callers such as MapPoint.cc:266 use it on single pairs). */
int orbfe_hamming(const uint8_t a[32], const uint8_t b[32]);

int orbfe_matcher_create(int device_id, orbfe_matcher** out);
void orbfe_matcher_destroy(orbfe_matcher* m);
int orbfe_matcher_device(const orbfe_matcher* m);       /* the device_id given at creation; -1 for NULL */
/* For callers that keep query-side tables in device memory across searches (the local map's MapPoint descriptors,
 * src/Tracking.cc:818-824 sends the same few thousand every frame; include/orbfe/orb_shim.hpp's MatcherContext does):
 * a host-to-device copy enqueued on the matcher's own stream, i.e. ordered BEFORE the matcher's next search and after its
 * previous one.  Returns at once; `src_host` must be page-locked (orbfe_host_alloc) and unchanged until
 * orbfe_matcher_synchronize(m) or the next search through m has returned. */
int orbfe_matcher_upload_async(orbfe_matcher* m, void* dst_device, const void* src_host, size_t bytes);
int orbfe_matcher_synchronize(orbfe_matcher* m);

/* int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched,
 *                                         vector<int>& vnMatches12, int windowSize)
 * (include/ORBmatcher.h:193, src/ORBmatcher.cc:400-515) with ORBmatcher(nnratio, checkOri).
 *   kps1/desc1/n1   : F1.mvKeysUn, F1.mDescriptors
 *   kps2/desc2/n2   : F2.mvKeysUn, F2.mDescriptors
 *   bounds          : {Frame::mnMinX, mnMaxX, mnMinY, mnMaxY} (static image bounds, Frame.cc:322-353)
 *   prev_xy [2*n1]  : vbPrevMatched, in/out
 *   matches12 [n1]  : vnMatches12, out (-1 = none)
 *   *nmatches       : return value of the reference function */
int orbfe_search_for_initialization(orbfe_matcher* m, const OrbfeKeyPoint* kps1, const uint8_t* desc1, int n1,
                                    const OrbfeKeyPoint* kps2, const uint8_t* desc2, int n2,
                                    const float bounds[4], float* prev_xy, int32_t* matches12, int window_size,
                                    float nnratio, int check_orientation, int* nmatches);

/* Batched form for throughput callers: npairs independent (F1, F2) pairs, one upload + one kernel launch +
 * one download for all of them, bookkeeping of the pairs resolved in parallel on the host.  Arrays of
 * per-pair pointers/sizes; bounds are shared (same camera). nmatches: npairs ints. */
int orbfe_search_for_initialization_batch(orbfe_matcher* m, int npairs, const OrbfeKeyPoint* const* kps1,
                                          const uint8_t* const* desc1, const int* n1,
                                          const OrbfeKeyPoint* const* kps2, const uint8_t* const* desc2,
                                          const int* n2, const float bounds[4], float* const* prev_xy,
                                          int32_t* const* matches12, int window_size, float nnratio,
                                          int check_orientation, int* nmatches);

/* MapPoint flag bits for the searches below. */
#define ORBFE_MP_IN_VIEW 1u    /* MapPoint::mbTrackInView                                   */
#define ORBFE_MP_BAD 2u        /* MapPoint::isBad()                                         */
#define ORBFE_MP_CANDIDATO 4u  /* MapPoint::plCandidato (os1 far-point extension)           */
#define ORBFE_MP_OBSERVED 8u   /* MapPoint::Observations() > 0                              */

/* int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th)
 * (include/ORBmatcher.h:93, src/ORBmatcher.cc:45-132) with ORBmatcher(nnratio).
 * The facade snapshots the MapPoint fields (under the reference's accessors) into flat arrays:
 *   mp_proj_xy [2*n_mp] : mTrackProjX, mTrackProjY       mp_level [n_mp] : mnTrackScaleLevel
 *   mp_viewcos [n_mp]   : mTrackViewCos                  mp_flags [n_mp] : ORBFE_MP_* bits
 *   mp_desc [32*n_mp]   : GetDescriptor()
 *   kp_occupied [n]     : 1 iff F.mvpMapPoints[i] != NULL && ->Observations() > 0 at call time
 *   kp_assigned [n] out : index into vpMapPoints written to F.mvpMapPoints[i] (last writer), -1 = untouched
 *   scale_factors       : F.mvScaleFactors (nlevels floats) */
int orbfe_search_by_projection(orbfe_matcher* m, const OrbfeKeyPoint* kps_un, const uint8_t* desc, int n,
                               const float bounds[4], const float* scale_factors, int nlevels,
                               const uint8_t* kp_occupied, const float* mp_proj_xy, const int32_t* mp_level,
                               const float* mp_viewcos, const uint8_t* mp_flags, const uint8_t* mp_desc, int n_mp,
                               float th, float nnratio, int32_t* kp_assigned, int* nmatches);

/* int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th)
 * (include/ORBmatcher.h:118, src/ORBmatcher.cc:1292-1423) and
 * int ORBmatcher::SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&, const float th, const int ORBdist)
 * (include/ORBmatcher.h:133, src/ORBmatcher.cc:1425-1552), from the projection onwards: the facade
 * projects each source MapPoint exactly as the reference does (float cv::Mat arithmetic,
 * ORBmatcher.cc:1326-1343 / 1451-1477) and passes
 *   src_uv [2*n_src], src_level (nLastOctave resp. nPredictedLevel), src_angle (source keypoint angle),
 *   src_flags (ORBFE_MP_OBSERVED), src_valid (0 = absent / outlier / rejected), src_desc;
 *   max_dist = TH_HIGH (100) resp. ORBdist; skip_any_occupied = 0 (skip kps whose MapPoint has
 *   observations, :1364-1366) resp. 1 (skip kps with any MapPoint, :1493-1494).
 * kp_assigned out: source index per keypoint, -1 untouched, -2 = reset to NULL by the rotation check. */
int orbfe_search_by_projection_uv(orbfe_matcher* m, const OrbfeKeyPoint* kps_un, const uint8_t* desc, int n,
                                  const float bounds[4], const float* scale_factors, int nlevels,
                                  const uint8_t* kp_occupied, const float* src_uv, const int32_t* src_level,
                                  const float* src_angle, const uint8_t* src_flags, const uint8_t* src_valid,
                                  const uint8_t* src_desc, int n_src, float th, int max_dist,
                                  int skip_any_occupied, int check_orientation, int32_t* kp_assigned,
                                  int* nmatches);

/* Host wall-clock ms of the last search call: [0] grid sort + arena build, [1] upload + kernel + download,
 * [2] sequential bookkeeping (resolve). */
int orbfe_debug_matcher_ms(const orbfe_matcher* m, double out[3]);

/* Generic GPU primitive under every windowed search of the reference (Fuse x2
 * ORBmatcher.cc:806-1064, SearchBySim3 :1066-1290, SearchByProjection(KeyFrame*, Scw, ...) :285-398,
 * SearchForTriangulation's window variant): for nq queries (x, y, r, minLevel, maxLevel, 32-byte descriptor)
 * against one frame's keypoints, the candidate lists Frame/KeyFrame::GetFeaturesInArea would return, in
 * reference order, each with its Hamming distance to the query descriptor.  r < 0 marks an inactive query.
 *   counts[nq], offsets[nq] : candidate count and first entry of each query in `pool`
 *   pool[pool_cap]          : entries  index | distance << 16
 *   *pool_used              : entries needed; if > pool_cap the call returns ORBFE_ERR_OVERFLOW (nothing lost:
 *                             call again with a larger pool)
 * The per-function bookkeeping (chi-square gates, best/second-best, occupancy) stays with the caller, exactly
 * like orb_shim.hpp does for the searches above. */
int orbfe_window_candidates(orbfe_matcher* m, const OrbfeKeyPoint* kps_un, const uint8_t* desc, int n,
                            const float bounds[4], int nq, const float* qx, const float* qy, const float* qr,
                            const int32_t* qmin_level, const int32_t* qmax_level, const uint8_t* qdesc,
                            uint32_t* counts, uint32_t* offsets, uint32_t* pool, size_t pool_cap, size_t* pool_used);

/* The projected best-match loop shared by int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const
 * vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th) (src/ORBmatcher.cc:285-398, loop :357-392),
 * int ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, float th) (:806-939, loop :872-936),
 * int ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, ...) (:941-1064, loop :1014-1050) and both directions of
 * int ORBmatcher::SearchBySim3(...) (:1066-1290), from KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:637-676) onwards.
 * The caller keeps the reference's projection code (cv::Mat float arithmetic, depth / viewing-angle / PredictScale
 * checks) and passes, per surviving MapPoint: src_uv, src_radius (= th * mvScaleFactors[nPredictedLevel]), src_level
 * (= nPredictedLevel; keypoints of octave [level-1, level] qualify), src_desc, src_valid (0 = rejected earlier).
 *   kp_skip (n, optional) / claim: vpMatched semantics of SearchByProjection -- a keypoint with kp_skip != 0 is never
 *     taken, and with claim != 0 an accepted keypoint is skipped by later sources (vpMatched[bestIdx] = pMP);
 *   inv_level_sigma2 (nlevels, optional) + chi2: Fuse's reprojection gate e2 * mvInvLevelSigma2[kpLevel] > 5.99;
 *   max_dist: TH_LOW (50) for SearchByProjection / Fuse, TH_HIGH (100) for SearchBySim3.
 * best_idx[i] = accepted keypoint index or -1 (the first minimum in GetFeaturesInArea order), best_dist[i] (optional)
 * its distance; *nmatches = number accepted.  The MapPoint bookkeeping (Replace / AddObservation / vnMatch agreement)
 * stays with the caller. */
int orbfe_search_projected(orbfe_matcher* m, const OrbfeKeyPoint* kps_un, const uint8_t* desc, int n, const float bounds[4],
                           int n_src, const float* src_uv, const float* src_radius, const int32_t* src_level,
                           const uint8_t* src_valid, const uint8_t* src_desc, const uint8_t* kp_skip, int claim,
                           const float* inv_level_sigma2, int nlevels, double chi2, int max_dist, int32_t* best_idx,
                           int32_t* best_dist, int* nmatches);

/* ---------------------------------------------------------------------------------------------
 * Device-resident frames.  The reference builds a frame's grid once (Frame::AssignFeaturesToGrid, src/Frame.cc:114-129,
 * from the constructor :111) and every search of that frame reuses it: 2-3 searches per tracked frame
 * (src/Tracking.cc:608, 614, 824), many more per keyframe.  An orbfe_frame is that object in HBM -- mvKeysUn (x, y,
 * octave, angle), mDescriptors and the cell-sorted table Frame / KeyFrame::GetFeaturesInArea walks (Frame.cc:209-262,
 * KeyFrame.cc:637-676) -- built once; the `_frame` searches below upload only their queries and return only their
 * result vector: candidate lists AND the reference's sequential bookkeeping stay on the GPU.
 * A frame belongs to one device; it may be searched through any matcher of that device, one search at a time.
 * ------------------------------------------------------------------------------------------- */
typedef struct orbfe_frame orbfe_frame;
/* From host arrays (kps_un = mvKeysUn in cv::KeyPoint layout, desc = mDescriptors rows, bounds = mnMinX, mnMaxX, mnMinY,
 * mnMaxY): one upload + the grid build, on the matcher's stream; returns without waiting. */
int orbfe_frame_create(orbfe_matcher* m, const OrbfeKeyPoint* kps_un, const uint8_t* desc, int n, const float bounds[4],
                       orbfe_frame** out);
/* From frame `frame_index` of the extractor's LAST COLLECTED batch (orbfe_extract / _batch / _collect): keypoints and
 * descriptors are taken where the kernels left them -- nothing is uploaded but, optionally, xy_un: the undistorted
 * coordinates [2 * n] of Frame::UndistortKeyPoints (Frame.cc:286-320; NULL = mvKeysUn = mvKeys, the camera without
 * distortion, :288-292 -- or, when the handle has a distorting camera (orbfe_extractor_set_camera), the mvKeysUn the undistortion
 * kernel left in the arena: no coordinate is sent either way).  Keypoint order = the order the extract call returned.  Must be called before the next
 * submit / extract on that handle (its arena is reused); the frame itself then lives on independently. */
int orbfe_frame_create_from_extract(orbfe_extractor* h, int frame_index, const float bounds[4], const float* xy_un,
                                    orbfe_frame** out);
void orbfe_frame_destroy(orbfe_frame* f);
int orbfe_frame_size(const orbfe_frame* f);
int orbfe_frame_device(const orbfe_frame* f);
/* Process-wide generation number of "which host object a resident frame stands for".  A caller that caches orbfe_frame
 * handles per reference object (include/orbfe/orb_shim.hpp does, per Frame / KeyFrame) compares the generation it saw when
 * it filled its cache with the current one and drops the cache when they differ.  orbfe_resident_invalidate() starts a new
 * generation (returns it): call it where the reference recycles identities -- Tracking::Reset() sets Frame::nNextId and
 * KeyFrame::nNextId back to 0 (src/Tracking.cc:1159-1160), Osmap's map load re-creates KeyFrames with the ids stored in the
 * file and rewrites KeyFrame::nNextId (src/Osmap.cpp:586) -- from any thread; every thread's cache notices at its next
 * search.  (The shim's cache is keyed by CONTENT, so a missing call costs memory, not correctness.)  Both are lock-free. */
unsigned long long orbfe_resident_epoch(void);
unsigned long long orbfe_resident_invalidate(void);
/* The frame's descriptor rows [n][32] in DEVICE memory, keypoint order; valid while the frame lives.  Returns when the
 * rows are complete.  Usable as the query descriptor rows of a search on another frame of the same device (a caller that
 * keeps descriptors on the GPU -- its own table of MapPoint descriptors, or a frame's rows -- passes device pointers and no
 * descriptor crosses PCIe).  The call only reads the frame, and so does whoever reads the rows: several threads may use them
 * at once, through any matcher or vocabulary of the device (the wait above is a host wait: no stream has to order itself). */
const uint8_t* orbfe_frame_descriptors_device(orbfe_frame* f);
/* Test / debug: the resident content back on the host -- keypoints (x, y, angle, octave; other fields zeroed) and
 * descriptor rows in keypoint order, the keypoint indices in grid order (capacity n) and the 64*48+1 cell offsets into
 * that order (mGrid flattened: cell = ix * 48 + iy).  Any pointer may be NULL. */
int orbfe_frame_download(orbfe_frame* f, OrbfeKeyPoint* kps_un, uint8_t* desc, int32_t* grid_order, int32_t* cell_start);

/* orbfe_search_by_projection / _uv / orbfe_search_projected on a resident frame: same arguments minus the frame's
 * arrays, same results.  (The host-array forms above run through these with a transient frame owned by the matcher.)
 * WHERE THE INPUT ARRAYS MAY LIVE: the DESCRIPTOR ROWS may lie in ordinary host memory,
 * in page-locked host memory (orbfe_host_alloc) or in the memory of the frame's device (16-byte aligned there, e.g.
 * orbfe_frame_descriptors_device, or a table the caller maintains with orbfe_matcher_upload_async); page-locked and
 * device rows are read by the search kernel in place.  EVERY OTHER per-query array (coordinates, levels, viewing cosines /
 * radii, angles, flags) and kp_occupied / kp_skip must be HOST memory -- the library reads them too (level range, largest
 * radius) -- page-locked ones are read by the kernel in place, ordinary ones are first copied into a page-locked
 * arena (a plain memcpy each -- there is no per-query loop on the host); a device pointer for one of them is refused with
 * ORBFE_ERR_INVALID before anything is read.  ORBFE_FRAME_ZEROCOPY=0: marshal the queries on
 * the host and upload them instead.  The call returns when the kernel's last store -- the call's number, into page-locked
 * memory -- has been seen (or, failing that for 2 ms, when the stream has drained).  Limits: at most 65 535 keypoints per frame,
 * 1 048 574 queries per search, 32 pyramid levels for the in-place route (more: the queries are marshalled on the host). */
int orbfe_search_by_projection_frame(orbfe_matcher* m, orbfe_frame* f, const float* scale_factors, int nlevels,
                                     const uint8_t* kp_occupied, const float* mp_proj_xy, const int32_t* mp_level,
                                     const float* mp_viewcos, const uint8_t* mp_flags, const uint8_t* mp_desc, int n_mp,
                                     float th, float nnratio, int32_t* kp_assigned, int* nmatches);
/* orbfe_search_by_projection_frame with the MapPoints' descriptors in a TABLE THE CALLER KEEPS ON THE DEVICE across searches
 * (Tracking::SearchLocalPoints, src/Tracking.cc:818-824, sends the same few thousand MapPoints frame after frame; their
 * descriptors change only in MapPoint::ComputeDistinctiveDescriptors, src/MapPoint.cc:227-292).  The table has two copies of
 * 32-byte rows: desc_table_device (memory of the frame's device, orbfe_device_malloc) and desc_table_host (page-locked,
 * orbfe_host_alloc; complete and current).  MapPoint i's descriptor is row (mp_desc_row[i] & 0x7fffffff): read from the
 * device copy when bit 31 is clear, from the host copy -- over PCIe, in place -- when it is set (a row the device has not
 * received yet; the caller sends it afterwards with orbfe_matcher_upload_async).  Per MapPoint 4 bytes of index cross PCIe
 * instead of 32 of descriptor.  mp_desc_row is host memory (page-locked: read in place).  n_rows = rows both copies of the table
 * hold: an in-view, not-bad MapPoint whose row index is >= n_rows fails the call with ORBFE_ERR_INVALID (as an out-of-range level
 * does) instead of reading outside the table.  Same results as the plain form. */
int orbfe_search_by_projection_frame_rows(orbfe_matcher* m, orbfe_frame* f, const float* scale_factors, int nlevels,
                                          const uint8_t* kp_occupied, const float* mp_proj_xy, const int32_t* mp_level,
                                          const float* mp_viewcos, const uint8_t* mp_flags, const uint8_t* desc_table_device,
                                          const uint8_t* desc_table_host, const int32_t* mp_desc_row, int n_rows, int n_mp,
                                          float th, float nnratio, int32_t* kp_assigned, int* nmatches);
int orbfe_search_by_projection_uv_frame(orbfe_matcher* m, orbfe_frame* f, const float* scale_factors, int nlevels,
                                        const uint8_t* kp_occupied, const float* src_uv, const int32_t* src_level,
                                        const float* src_angle, const uint8_t* src_flags, const uint8_t* src_valid,
                                        const uint8_t* src_desc, int n_src, float th, int max_dist, int skip_any_occupied,
                                        int check_orientation, int32_t* kp_assigned, int* nmatches);
int orbfe_search_projected_frame(orbfe_matcher* m, orbfe_frame* f, int n_src, const float* src_uv, const float* src_radius,
                                 const int32_t* src_level, const uint8_t* src_valid, const uint8_t* src_desc,
                                 const uint8_t* kp_skip, int claim, const float* inv_level_sigma2, int nlevels, double chi2,
                                 int max_dist, int32_t* best_idx, int32_t* best_dist, int* nmatches);
/* ---------------------------------------------------------------------------------------------
 * Local map on the device.  Tracking::SearchLocalPoints (src/Tracking.cc:798-825) calls Frame::isInFrustum(pMP, 0.5)
 * (src/Frame.cc:151-207) for every local MapPoint and then SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th).  An
 * orbfe_local_map is a table of the MapPoint fields that projection reads, one 64-byte row per MapPoint, in the memory of
 * the matcher's device: pos[3] (GetWorldPos), normal[3] (GetNormal), the RAW mfMinDistance and mfMaxDistance (PredictScale,
 * src/MapPoint.cc:370-379, divides the raw mfMaxDistance; GetMin/MaxDistanceInvariance, :358-368, scale them by 0.8f / 1.2f),
 * then the 32-byte descriptor (GetDescriptor).  The caller keeps the rows current; a search names its MapPoints by row.
 * ------------------------------------------------------------------------------------------- */
typedef struct orbfe_local_map orbfe_local_map;
/* Frame::isInFrustum skips a MapPoint that Tracking::SearchLocalPoints skips: mnLastFrameSeen == mCurrentFrame.mnId
 * (Tracking.cc:804-805; the MapPoints already matched in this frame). */
#define ORBFE_MP_SKIP 16u
/* The camera of the current Frame, as the Frame holds it: mRcw (row-major), mtcw, mOw (passed as it is, nothing is
 * recomputed), fx, fy, cx, cy, mfLogScaleFactor.  The image bounds mnMinX..mnMaxY are the resident frame's. */
typedef struct OrbfeCamera {
  float Rcw[9];
  float tcw[3];
  float Ow[3];
  float fx, fy, cx, cy;
  float logScaleFactor;
} OrbfeCamera;
/* A table of `capacity` rows (zeroed) for searches through matcher m (the table lives on m's device; its uploads are
 * ordered on m's stream). */
int orbfe_local_map_create(orbfe_matcher* m, int capacity, orbfe_local_map** out);
void orbfe_local_map_destroy(orbfe_local_map* map);
int orbfe_local_map_capacity(const orbfe_local_map* map);
/* Writes rows[0..n) of the table: entry i of each array goes to row rows[i] (pos, normal: 3 floats per entry; min_raw,
 * max_raw: 1; desc: 32 bytes).  Any array may be NULL: that field of those rows keeps its value.  Asynchronous: the
 * values are copied into page-locked staging the library owns and sent on the matcher's stream, ordered before its next
 * search; the caller's arrays may be reused when the call returns.  A row outside [0, capacity) or a row named twice
 * fails the call with ORBFE_ERR_INVALID before anything is sent. */
int orbfe_local_map_set_rows(orbfe_local_map* map, int n, const int32_t* rows, const float* pos, const float* normal,
                             const float* min_raw, const float* max_raw, const uint8_t* desc);
/* bool Frame::isInFrustum(MapPoint*, float viewingCosLimit) (src/Frame.cc:151-207) for MapPoint i = table row rows[i],
 * i < n_mp, on the GPU, as Tracking::SearchLocalPoints calls it (Tracking.cc:800-814): a MapPoint whose flags[i] carry
 * ORBFE_MP_BAD or ORBFE_MP_SKIP is not projected (in_view 0); other bits of flags are ignored.  Per MapPoint:
 *   in_view [n_mp]     : the return value (mbTrackInView)
 *   proj_xy [2*n_mp]   : mTrackProjX, mTrackProjY     level [n_mp] : mnTrackScaleLevel (PredictScale, NOT clamped: a
 *   view_cos [n_mp]    : mTrackViewCos                 level outside [0, nlevels) is reported as it is)
 * bit for bit what the reference writes into the MapPoint (float cv::Mat arithmetic, glibc logf); where in_view is 0 the
 * other three hold 0 (the reference leaves the MapPoint's old values).  *n_in_view = MapPoints in view (nToMatch).  Any
 * output array may be NULL.  rows and flags are host memory; a row outside [0, capacity) of a MapPoint that is projected
 * fails the call with ORBFE_ERR_INVALID.  Returns when the outputs are written. */
int orbfe_project_local_map(orbfe_matcher* m, orbfe_frame* f, orbfe_local_map* map, const OrbfeCamera* cam,
                            float view_cos_limit, const int32_t* rows, const uint8_t* flags, int n_mp, uint8_t* in_view,
                            float* proj_xy, int32_t* level, float* view_cos, int* n_in_view);
/* The projection of orbfe_project_local_map followed by int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&
 * vpLocalMapPoints, const float th) (ORBmatcher.cc:45-132, ORBmatcher(nnratio)) in ONE submission on the matcher's stream:
 * the projection kernel leaves the queries in device memory and the search reads them there; no per-MapPoint value
 * crosses PCIe between the two.  flags: ORBFE_MP_BAD / _SKIP as above, ORBFE_MP_CANDIDATO / _OBSERVED as for
 * orbfe_search_by_projection; ORBFE_MP_IN_VIEW is computed, its input value ignored.  kp_occupied, kp_assigned, nmatches,
 * scale_factors (F.mvScaleFactors, 1..32 levels) as for orbfe_search_by_projection_frame.  in_view, proj_xy, level, view_cos:
 * optional outputs (NULL: not returned), as orbfe_project_local_map.  Results are those of orbfe_project_local_map followed
 * by orbfe_search_by_projection_frame_rows on the same inputs.
 * LEVEL CONTRACT: a MapPoint in view whose predicted level lies outside [0, nlevels) fails the call with ORBFE_ERR_INVALID
 * (as an out-of-range level does in the rows form).  The projection kernel finds it and takes it out of the search before
 * anything is indexed with that level; the outputs are then unspecified, and the matcher, frame and table stay usable.
 * f is SEARCHED (one search of a frame at a time); orbfe_project_local_map alone reads nothing of f but its bounds. */
int orbfe_search_local_points_frame(orbfe_matcher* m, orbfe_frame* f, orbfe_local_map* map, const OrbfeCamera* cam,
                                    float view_cos_limit, const int32_t* rows, const uint8_t* flags, int n_mp,
                                    const float* scale_factors, int nlevels, const uint8_t* kp_occupied, float th, float nnratio,
                                    uint8_t* in_view, float* proj_xy, int32_t* level, float* view_cos, int32_t* kp_assigned,
                                    int* nmatches, int* n_in_view);
/* The projection loops of the two frame-rate searches whose sources are the keypoints of ANOTHER frame, on the GPU:
 *   ORBFE_SRC_LAST_FRAME  int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th)
 *                         (src/ORBmatcher.cc:1292-1423; projection :1324-1347)
 *   ORBFE_SRC_KEYFRAME    int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist)
 *                         (:1425-1552; projection :1450-1479)
 * Source i is keypoint i of src_frame (the resident copy of LastFrame / pKF; n_src must equal its size): its octave
 * (mvKeys[i].octave, the window's level in LAST_FRAME mode) and its angle (mvKeysUn[i].angle, the rotation check) are read
 * from that copy.  Its MapPoint is row rows[i] of `map` (position, raw mfMinDistance / mfMaxDistance, descriptor); cam is the
 * CURRENT frame's camera (Ow = -Rcw.t()*tcw as :1431 computes it; read in KEYFRAME mode only), the bounds are cur_frame's.
 * flags[i]: ORBFE_MP_SKIP = no MapPoint / mvbOutlier[i] (LAST_FRAME), no MapPoint / in sAlreadyFound (KEYFRAME);
 * ORBFE_MP_BAD = isBad() (KEYFRAME; ignored in LAST_FRAME mode, whose loop does not ask); ORBFE_MP_OBSERVED =
 * Observations() > 0.  A source that is not projected may carry any row.  Per source:
 *   valid [n_src]  : 1 = the source reaches GetFeaturesInArea (:1349 / :1481)
 *   uv [2*n_src]   : the projection u, v              level [n_src] : nLastOctave resp. nPredictedLevel (PredictScale, NOT
 *                                                                     clamped: reported as it is)
 * bit for bit the reference's values (float cv::Mat arithmetic, the double division of :1329 / :1455, glibc logf); 0
 * where valid is 0.  LAST_FRAME rejects invzc < 0 (:1332), KEYFRAME does not (a point behind the camera that lands inside the
 * bounds stays valid, as in the reference).  A projection that is not finite (z = +-0 with x = y = 0) is invalid: the
 * reference's GetFeaturesInArea finds no cell for it.  *n_valid = valid sources.  Any output may be NULL.  rows and flags are
 * host memory; a row outside [0, capacity) of a source that is projected fails the call with ORBFE_ERR_INVALID.  Returns
 * when the outputs are written. */
#define ORBFE_SRC_LAST_FRAME 0
#define ORBFE_SRC_KEYFRAME 1
int orbfe_project_sources(orbfe_matcher* m, orbfe_frame* cur_frame, orbfe_frame* src_frame, orbfe_local_map* map,
                          const OrbfeCamera* cam, int mode, const int32_t* rows, const uint8_t* flags, int n_src, uint8_t* valid,
                          float* uv, int32_t* level, int* n_valid);
/* The projection of orbfe_project_sources followed by the rest of that search (the windows, best distance <= max_dist, the
 * rotation histogram) in ONE submission on the matcher's stream: the projection kernel leaves the queries in device memory
 * and the search reads them there; per source only rows[i] and flags[i] cross PCIe.  LAST_FRAME: a keypoint is taken once a
 * source with ORBFE_MP_OBSERVED holds it (:1363-1365; orbfe_search_by_projection_uv_frame's skip_any_occupied = 0), max_dist =
 * TH_HIGH; KEYFRAME: once any source holds it (:1493-1494; skip_any_occupied = 1), max_dist = ORBdist.  scale_factors
 * (CurrentFrame.mvScaleFactors, 1..32 levels), kp_occupied, th, check_orientation, kp_assigned (source index, -1, or -2 for a
 * slot the rotation check cleared), nmatches as for orbfe_search_by_projection_uv_frame.  valid, uv, level: optional outputs
 * (NULL: not returned).  Results are those of orbfe_project_sources followed by orbfe_search_by_projection_uv_frame on the
 * same inputs.
 * LEVEL CONTRACT: a valid source whose level lies outside [0, nlevels) fails the call with ORBFE_ERR_INVALID, as in
 * orbfe_search_local_points_frame: the projection kernel takes it out of the search before anything is indexed with that
 * level (LAST_FRAME: refused up front from the source frame's largest octave); the outputs are then unspecified, and the
 * matcher, frames and table stay usable.
 * cur_frame is SEARCHED (one search of a frame at a time).  src_frame is only read (octaves, angles), here and in
 * orbfe_project_sources, behind its build on m's stream: it may serve as the source of several threads' calls at once. */
int orbfe_search_by_projection_sources_frame(orbfe_matcher* m, orbfe_frame* cur_frame, orbfe_frame* src_frame,
                                             orbfe_local_map* map, const OrbfeCamera* cam, int mode, const int32_t* rows,
                                             const uint8_t* flags, int n_src, const float* scale_factors, int nlevels,
                                             const uint8_t* kp_occupied, float th, int max_dist, int check_orientation,
                                             uint8_t* valid, float* uv, int32_t* level, int32_t* kp_assigned, int* nmatches,
                                             int* n_valid);
/* The projection loops of the four KEYFRAME-side searches of LocalMapping and LoopClosing, on the GPU: everything between
 * GetWorldPos() and KeyFrame::GetFeaturesInArea in
 *   int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th)   (src/ORBmatcher.cc:285-398;
 *                                                                                             projection :316-357)
 *   int ORBmatcher::Fuse(KeyFrame* pKF, vpMapPoints, th)                                      (:806-939; :833-873)
 *   int ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint)            (:941-1064; :973-1015)
 *   int ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th), each direction  (:1066-1290; :1122-1155, :1202-1235)
 * OrbfeKeyFrameProjection describes one such loop.  The caller computes every matrix ONCE per call, with the reference's own
 * cv::Mat expressions (Scw's decomposition :293-298, s12*R12, (1.0/s12)*R12.t(), -sR21*t12, GetCameraCenter()); nothing is
 * recomputed on the device.
 *   R, t            : p = R*p3Dw + t (Rcw, tcw; R1w, t1w resp. R2w, t2w for SearchBySim3)
 *   has_second, sR, t2 : SearchBySim3 only: p = sR*p + t2 on the float result of the first (sR21, t21 resp. sR12, t12)
 *   Ow              : the camera centre PO = p3Dw - Ow is taken from (not read when distance_from_camera_point is set)
 *   fx, fy, cx, cy  : the intrinsics u = fx*x + cx, v = fy*y + cy use -- apart from the searched keyframe on purpose:
 *                     SearchBySim3 uses pKF1's in both directions (:1069-1072)
 *   logScaleFactor  : the SEARCHED keyframe's mfLogScaleFactor (PredictScale)
 *   invz_in_double  : 0: `1/p3Dc.at<float>(2)`, a float division (:326, :840); 1: `1.0/...`, a double division rounded to
 *                     float (:983, :1130, :1210)
 *   check_viewing_angle : 1: reject PO.dot(Pn) < 0.5*dist (:349, :865, :1006); SearchBySim3 has no such test
 *   distance_from_camera_point : 0: dist3D = cv::norm(p3Dw - Ow); 1: cv::norm of the transformed point p itself (:1143,
 *                     :1223; not together with check_viewing_angle) */
typedef struct OrbfeKeyFrameProjection {
  float R[9];
  float t[3];
  int has_second;
  float sR[9];
  float t2[3];
  float Ow[3];
  float fx, fy, cx, cy;
  float logScaleFactor;
  int invz_in_double;
  int check_viewing_angle;
  int distance_from_camera_point;
} OrbfeKeyFrameProjection;
/* MapPoint i = row rows[i] of `map`, i < n, projected into the resident keyframe kf_frame (its bounds are the ones
 * KeyFrame::IsInImage, src/KeyFrame.cc:678-681, tests: u >= mnMinX && u < mnMaxX && v >= mnMinY && v < mnMaxY, half-open).
 * flags[i]: ORBFE_MP_BAD = isBad(); ORBFE_MP_SKIP = whatever else keeps the loop from projecting it (in spAlreadyFound, NULL,
 * IsInKeyFrame(pKF), vbAlreadyMatched).  Either bit: not projected, and the point may carry any row.  scale_factors = the
 * searched keyframe's mvScaleFactors (1..32 levels).  Per point:
 *   valid [n]  : 1 = the point reaches GetFeaturesInArea      uv [2*n] : the projection u, v
 *   level [n]  : nPredictedLevel (PredictScale, NOT clamped: reported as it is)
 *   radius [n] : th * scale_factors[level] (0 where the level lies outside [0, nlevels))
 * bit for bit the reference's values (float cv::Mat arithmetic, x = p[0]*invz rounded before the multiplication by fx, glibc
 * logf); 0 where valid is 0.  A projection that is not finite (z = +-0) fails IsInImage by itself.  *n_valid = valid points.
 * Any output may be NULL.  rows and flags are host memory; a row outside [0, capacity) of a point that is projected fails the
 * call with ORBFE_ERR_INVALID.  Returns when the outputs are written. */
int orbfe_project_keyframe(orbfe_matcher* m, orbfe_frame* kf_frame, orbfe_local_map* map, const OrbfeKeyFrameProjection* proj,
                           const int32_t* rows, const uint8_t* flags, int n, const float* scale_factors, int nlevels, float th,
                           uint8_t* valid, float* uv, int32_t* level, float* radius, int* n_valid);
/* The projection of orbfe_project_keyframe followed by the projected best-match loop (orbfe_search_projected_frame: :357-392,
 * :873-936, :1015-1050, :1155-1185 / :1235-1265) in ONE submission on the matcher's stream: the projection kernel leaves uv,
 * level, radius, valid and the descriptor row in device memory and the search reads them there; no copy command runs between
 * the kernels, and per point only rows[i] and flags[i] cross PCIe.  kp_skip, claim, inv_level_sigma2 (nlevels values or NULL)
 * with chi2, max_dist, best_idx [n], best_dist [n] (optional) and nmatches as for orbfe_search_projected_frame.  valid, uv,
 * level: optional outputs (NULL: not returned).  Results are those of orbfe_project_keyframe followed by
 * orbfe_search_projected_frame on the same inputs.  n == 0 or an empty keyframe: ORBFE_OK, every best_idx -1.
 * LEVEL CONTRACT: a valid point whose predicted level lies outside [0, nlevels) fails the call with ORBFE_ERR_INVALID, as in
 * orbfe_search_local_points_frame: the projection kernel takes it out of the search before anything is indexed with that
 * level; the outputs are then unspecified, and the matcher, frame and table stay usable.
 * kf_frame is SEARCHED (one search of a frame at a time); orbfe_project_keyframe alone reads nothing of it but its bounds. */
int orbfe_search_projected_keyframe_frame(orbfe_matcher* m, orbfe_frame* kf_frame, orbfe_local_map* map,
                                          const OrbfeKeyFrameProjection* proj, const int32_t* rows, const uint8_t* flags, int n,
                                          const float* scale_factors, int nlevels, float th, const uint8_t* kp_skip, int claim,
                                          const float* inv_level_sigma2, double chi2, int max_dist, uint8_t* valid, float* uv,
                                          int32_t* level, int32_t* best_idx, int32_t* best_dist, int* nmatches, int* n_valid);

/* void MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cc:227-292) and void MapPoint::UpdateNormalAndDepth()
 * (:315-356) for a batch of MapPoints, from the RESIDENT keyframes straight into the table's rows: the producer of everything
 * the projections above read.  MapPoint p, p < n_mp, is row rows[p]; its observations are entries [obs_offsets[p],
 * obs_offsets[p+1]) of obs_kf / obs_kp / obs_flags in std::map<KeyFrame*,size_t> order: obs_kf = slot of the observing keyframe
 * in kf_frames / kf_Ow (kf_Ow[3*s..] = its GetCameraCenter()), obs_kp = the keypoint index there, obs_flags (NULL: all 0) carries
 * ORBFE_OBS_KF_BAD where pKF->isBad().  `what` selects the function(s):
 *   ORBFE_REFRESH_DESCRIPTOR    the descriptor rows of the observations WITHOUT the bad bit are gathered from the keyframes'
 *                               resident descriptors; the one with the least median distance to the others (median = sorted[
 *                               (size_t)(0.5*(N-1)) ], first minimum wins) goes into the row.  An empty list leaves the row's
 *                               descriptor as it is.
 *   ORBFE_REFRESH_NORMAL_DEPTH  over ALL observations (bad keyframes included, as the reference): normal = mean of
 *                               (pos - Ow)/|pos - Ow|; mfMaxDistance = |pos - Ow_ref| * scale_factors[level], level = octave of
 *                               keypoint ref_kp[p] of the resident keyframe in slot ref_kf[p] (pRefKF, observations[pRefKF]);
 *                               mfMinDistance = mfMaxDistance / scale_factors[nlevels-1].  pos is read from the row (never
 *                               written).  A MapPoint without observations keeps its row (its ref_kf / ref_kp are not read).
 *                               The float chain is restated operation for operation (cv::norm in double, cv::scaleAdd with the
 *                               product rounded before the sum, convertTo's `+ 0`); INTEGRATION.md section 6 names what an
 *                               OpenCV built with fused multiply-add would change.
 * Optional host outputs (NULL: not returned), one entry per MapPoint: best_obs = index of the chosen descriptor's observation
 * inside the MapPoint's own list as passed (bad entries counted), -1 where nothing was chosen or DESCRIPTOR is not selected;
 * normal [3*n_mp], min_raw, max_raw = those fields of the row as they stand after the call.
 * A kf_frames[s] may be NULL if every observation naming slot s carries ORBFE_OBS_KF_BAD and no MapPoint uses it as ref_kf: only
 * its Ow is read.  The call runs on the matcher's stream, after earlier orbfe_local_map_set_rows and before the next search; the
 * keyframes' builds are waited for on the stream.  It returns when the requested host outputs are written; with all four NULL
 * it returns once enqueued (8 bytes per observation went up, nothing comes down) -- unless a keyframe holds an octave >=
 * nlevels, in which case it waits for the kernel's level report (below).  n_mp == 0: ORBFE_OK.
 * ORBFE_ERR_INVALID before anything is sent: a row outside [0, capacity) or named twice; obs_offsets not non-decreasing; a slot
 * outside [0, n_kf); a keypoint index outside its frame's size; a NULL frame named by a non-bad observation or as ref_kf; a frame
 * on another device; nlevels outside 1..32; a list of more non-bad observations than the LDS budget holds (150 KB / 32 bytes, as
 * orbfe_distinctive_descriptors).
 * LEVEL CONTRACT: a MapPoint whose reference keypoint's octave lies outside [0, nlevels) fails the call with ORBFE_ERR_INVALID;
 * the kernel finds it before anything is indexed with that level and leaves that MapPoint's row unwritten (the other rows
 * of the batch are written, the host outputs are not); the matcher, frames and table stay usable.
 * The keyframes are only read (descriptor rows, octaves): calls of other threads that only read them may overlap.  After the
 * enqueue-only return the kernel may still be reading them; orbfe_frame_destroy is safe all the same -- it frees the frame's
 * device memory with hipFree, which waits for the work of every stream of the device before it releases anything. */
#define ORBFE_OBS_KF_BAD 1u              /* pKF->isBad(): not in the descriptor list; still in the normal */
#define ORBFE_REFRESH_DESCRIPTOR   1     /* ComputeDistinctiveDescriptors */
#define ORBFE_REFRESH_NORMAL_DEPTH 2     /* UpdateNormalAndDepth */
int orbfe_local_map_refresh_rows(orbfe_matcher* m, orbfe_local_map* map, int what,
      int n_kf, orbfe_frame* const* kf_frames, const float* kf_Ow /* 3*n_kf */,
      const float* scale_factors, int nlevels,
      int n_mp, const int32_t* rows, const int32_t* obs_offsets /* n_mp+1 */,
      const int32_t* obs_kf /* slot into kf_frames */, const int32_t* obs_kp, const uint8_t* obs_flags,
      const int32_t* ref_kf, const int32_t* ref_kp,          /* per MapPoint; NORMAL_DEPTH only */
      int32_t* best_obs, float* normal, float* min_raw, float* max_raw /* optional host outputs */);
/* test / debug: rows of the table back on the host, 64 bytes each (waits for the matcher's stream first) */
int orbfe_local_map_download_rows(orbfe_local_map* map, int n, const int32_t* rows, uint8_t* out);

/* Rounds the bookkeeping kernel of the last `_frame` search needed -- the most any chunk of 2 048 consecutive queries took
 * (negative: a chunk hit the bound ORBFE_RESOLVE_MAX_ROUNDS, default 48, and a serial pass on the device finished it). */
int orbfe_debug_resolve_rounds(const orbfe_matcher* m);
/* Where that kernel kept its state: 2 = tables and candidate entries in LDS, 1 = tables in LDS, 0 = global scratch (problems
 * beyond 152 KB of tables, or ORBFE_RESOLVE_GENERIC=1). */
int orbfe_debug_resolve_route(const orbfe_matcher* m);
/* Shader-clock readings (low 32 bits) at the kernel's start, after its set-up, after the fixed point, at its end. */
int orbfe_debug_resolve_phases(const orbfe_matcher* m, int out[4]);

/* void MapPoint::ComputeDistinctiveDescriptors()  (src/MapPoint.cc:227-292), from the gathered descriptor list
 * onwards, batched over MapPoints: MapPoint p owns descriptor rows [offsets[p], offsets[p+1]) of `descs`
 * (32-byte rows, the non-bad observations in std::map order); best_idx[p] = index inside its own list of the
 * descriptor with the least median distance to the rest (median = sorted[ (size_t)(0.5*(N-1)) ], first minimum
 * wins), -1 for an empty list.  All-pairs 256-bit Hamming + per-row median on the GPU, one wave per MapPoint. */
int orbfe_distinctive_descriptors(orbfe_matcher* m, int n_mp, const int32_t* offsets, const uint8_t* descs,
                                  int32_t* best_idx);

/* ---------------------------------------------------------------------------------------------
 * Covisibility counts.  The counting loop of KeyFrame::UpdateConnections (src/KeyFrame.cc:305-331) and of
 * Tracking::UpdateLocalKeyFrames (src/Tracking.cc:862-879) for a batch of subjects in one call; what follows the counting (the
 * threshold, AddConnection, the sort, the parent) depends on pointer order and stays with the host (include/orbfe/Covisibility.h).
 *
 * Keyframes are named by slots 0..n_kf-1, MapPoints by indices 0..n_mp-1.  MapPoint p is observed by the keyframes
 * obs_kf[obs_offsets[p] .. obs_offsets[p+1]).  Subject s (a keyframe, or a Frame) holds one entry per keypoint,
 * subj_mp[subj_offsets[s] .. subj_offsets[s+1]): the MapPoint's index, or -1 for whatever the reference skips (null, isBad(),
 * plCandidato, plLejano).  For every entry with p = subj_mp[e] >= 0 and every observation o of p, with j = obs_kf[o]:
 * counter[j]++ unless j == subj_self[s] or j >= subj_limit[s].  A MapPoint named twice by one subject counts twice (the reference
 * walks the vector mvpMapPoints, not a set); observers that are bad keyframes are counted, as in the reference.
 *   subj_self[s]   the subject's own slot (KeyFrame.cc:327), or -1: no exclusion -- Tracking's keyframeCounter
 *   subj_limit     NULL: n_kf for every subject.  Otherwise only observers with slot < subj_limit[s] are counted: with the slots in
 *                  load order, subj_limit[k] = k + 1 gives the counter keyframe k sees in Osmap's rebuild (src/Osmap.cpp:569-579),
 *                  where only keyframes 0..k have added their observations when k calls UpdateConnections.
 * Output: a compact CSR.  Subject s owns [out_offsets[s], out_offsets[s+1]) of out_kf / out_count: its non-zero counters in
 * ascending slot order.  *n_needed = the total number of entries; if it exceeds cap the call returns ORBFE_ERR_OVERFLOW with
 * *n_needed set, the other outputs unspecified and the matcher usable.  No call needs more than the sum over the subjects of
 * min(subj_limit[s], observations reachable from s).
 * ORBFE_ERR_INVALID before anything is sent: a null pointer (out_kf / out_count may be NULL with cap 0, obs_kf / subj_mp where
 * their CSR is empty); a negative size; offsets that decrease; an obs_kf outside [0, n_kf); a subj_mp outside [-1, n_mp); a
 * subj_self outside [-1, n_kf); a subj_limit outside [0, n_kf]; a bound above 2^31 - 1 entries.  n_subj == 0: ORBFE_OK.
 * The call runs on the matcher's stream and returns when the host outputs are written.  It takes no resident frames: only
 * indices cross PCIe.  Integer counting: the result is exact, whatever the order of the additions. */
int orbfe_covisibility_counts(orbfe_matcher* m,
      int n_kf,                                   /* keyframe slots 0..n_kf-1 */
      int n_mp, const int32_t* obs_offsets /* n_mp+1 */, const int32_t* obs_kf /* observer slot per observation */,
      int n_subj, const int32_t* subj_self /* slot of the subject, or -1 for a Frame */,
      const int32_t* subj_limit /* NULL = n_kf for all: only observers with slot < limit are counted */,
      const int32_t* subj_offsets /* n_subj+1 */, const int32_t* subj_mp /* MapPoint index per keypoint entry, -1 = skipped */,
      int32_t* out_offsets /* n_subj+1 */, int32_t* out_kf, int32_t* out_count, int cap, int* n_needed);
/* Observer slots one pass of the kernel counts (the bins of its histogram in LDS); a map of more keyframes takes several passes. */
int orbfe_debug_covis_slots_per_pass(void);
/* The last orbfe_covisibility_counts of this matcher, ms: [0] argument check and staging on the host, [1] the kernel (events on
 * the stream), [2] the whole call. */
int orbfe_debug_covis_ms(const orbfe_matcher* m, double out[3]);

/* ---------------------------------------------------------------------------------------------
 * Keyframe culling.  The counting loop of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:574-598) for a batch of subjects in
 * one call; the 90 % test, SetBadFlag and the recount after a keyframe has gone bad stay with the host
 * (include/orbfe/KeyFrameCulling.h).
 *
 * Slots, MapPoint indices and the two CSRs (obs_offsets / obs_kf, subj_self / subj_offsets / subj_mp) are those of
 * orbfe_covisibility_counts above: a caller that has written them down for that call can pass the same arrays.  Added here:
 *   obs_level[o]   pKFi->mvKeysUn[mit->second].octave of observation o (next to obs_kf[o])
 *   subj_level[e]  pKF->mvKeysUn[i].octave of the subject's entry e (next to subj_mp[e])
 *   mp_nobs[p]     pMP->Observations(); NULL: the length of p's run in the CSR
 *   th_obs         the reference's thObs, 3 there; any value >= 1 here
 * For subject s and every entry e with p = subj_mp[e] >= 0 (-1 stands for whatever the reference skips: null, isBad()):
 * n_mps[s]++; and if nobs(p) > th_obs, with c = the number of observations o of p with obs_kf[o] != subj_self[s] and
 * (int)obs_level[o] <= (int)subj_level[e] + 1: n_redundant[s]++ iff c >= th_obs (the reference's break at thObs is only an early
 * exit).  A MapPoint named twice by one subject counts twice; observers that are bad keyframes count, as in the reference;
 * subj_self[s] == -1 excludes nobody.
 * ORBFE_ERR_INVALID before anything is sent: a null pointer (obs_kf / obs_level and subj_mp / subj_level may be NULL where their
 * CSR is empty, mp_nobs always); a negative size; th_obs < 1; offsets that decrease; an obs_kf outside [0, n_kf); a subj_mp
 * outside [-1, n_mp); a subj_self outside [-1, n_kf); a negative mp_nobs.  n_subj == 0: ORBFE_OK.
 * The call runs on the matcher's stream and returns when the two output arrays are written.  It takes no resident frames: only
 * indices and level bytes cross PCIe.  Integer counting: the result is exact, whatever the order of the additions. */
int orbfe_redundant_observations(orbfe_matcher* m,
      int n_kf,                                   /* keyframe slots 0..n_kf-1 */
      int n_mp, const int32_t* obs_offsets /* n_mp+1 */, const int32_t* obs_kf /* observer slot per observation */,
      const uint8_t* obs_level /* octave per observation */,
      const int32_t* mp_nobs /* n_mp, or NULL = the CSR's length per MapPoint */,
      int n_subj, const int32_t* subj_self /* slot of the subject, or -1 */, const int32_t* subj_offsets /* n_subj+1 */,
      const int32_t* subj_mp /* MapPoint index per keypoint entry, -1 = skipped */, const uint8_t* subj_level /* octave per entry */,
      int th_obs,
      int32_t* out_n_mps /* n_subj */, int32_t* out_n_redundant /* n_subj */);
/* The last orbfe_redundant_observations of this matcher, ms: [0] argument check and staging on the host, [1] the kernel (events
 * on the stream), [2] the whole call. */
int orbfe_debug_culling_ms(const orbfe_matcher* m, double out[3]);

/* ---------------------------------------------------------------------------------------------
 * Bag of words. Replaces the DBoW2 calls on the path: Frame::ComputeBoW (src/Frame.cc:277-284) ->
 * TemplatedVocabulary<FORB>::transform(features, BowVector&, FeatureVector&, levelsup)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1136-1204, descent :1306-1347), and the two
 * ORBmatcher::SearchByBoW overloads (src/ORBmatcher.cc:154-283, 517-650).
 * ------------------------------------------------------------------------------------------- */
/* Vocabulary from the fork's binary file (loadFromBinaryFile, TemplatedVocabulary.h:1563-1640): 4 header bytes
 * {k, L, scoring, weighting} followed by 45-byte node records {int32 parent, u8 isLeaf, u8 descriptor[32],
 * f64 weight} (packed, little endian).  Node ids count from 1 in record order (0 = root), children keep record
 * order, word ids count the isLeaf records.  orbfe_vocabulary_create takes the header fields and the records
 * separately (a loader of the text / yml formats fills the same records); _from_image takes the file contents.
 * scoring: 0 L1_NORM .. 5 DOT_PRODUCT, weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY (BowVector.h:36-53).
 * The tree lives in HBM (k=10, L=6: 1.1 M nodes, about 45 MB). */
int orbfe_vocabulary_create(int device_id, int k, int L, int scoring, int weighting, const void* records, int n_records,
                            orbfe_vocabulary** out);
int orbfe_vocabulary_create_from_image(int device_id, const void* image, size_t bytes, orbfe_vocabulary** out);
void orbfe_vocabulary_destroy(orbfe_vocabulary* v);
int orbfe_vocabulary_info(const orbfe_vocabulary* v, int* k, int* L, int* scoring, int* weighting, int* n_nodes,
                          int* n_words);

/* transform(features, v, fv, levelsup) for n descriptors (32-byte rows; host memory, or device memory when
 * in_device_memory != 0).  BowVector: n_words (word id ascending, value) pairs in bow_ids / bow_values (capacity
 * n).  FeatureVector: n_fv_nodes node ids ascending in fv_nodes (capacity n), fv_offsets[i]..fv_offsets[i+1]
 * (capacity n+1) delimit the node's feature indices in fv_features (capacity n), in push_back order.
 * word_of_feature / node_of_feature (optional, n each): the word id and the node id `levelsup` levels above the
 * leaf that each descriptor reached (stopped words, weight 0, are reported here but left out of both vectors).
 * Values are bit-identical to DBoW2's doubles: weights are summed in feature order, normalised in word order. */
int orbfe_bow_transform(orbfe_vocabulary* v, const uint8_t* desc, int n, int in_device_memory, int levelsup,
                        uint32_t* bow_ids, double* bow_values, int* n_words, uint32_t* fv_nodes, uint32_t* fv_offsets,
                        uint32_t* fv_features, int* n_fv_nodes, uint32_t* word_of_feature, uint32_t* node_of_feature);

/* orbfe_bow_transform for n_sets descriptor sets in ONE submission and ONE wait: the KeyFrame::ComputeBoW loop of a map load
 * (src/Osmap.cpp, Osmap::rebuild).  Set s has n[s] rows (0 is allowed) at desc[s]; WHERE THE ROWS LIE is decided per set:
 * ordinary host memory (copied into one upload), page-locked host memory or 16-byte aligned rows in the memory of the
 * vocabulary's device (orbfe_frame_descriptors_device) -- both read in place.  Every output is an array of n_sets per-set
 * pointers (n_words, n_fv_nodes: n_sets ints), each in the layout and with the bytes orbfe_bow_transform gives for that set
 * alone; word_of_feature / node_of_feature may be NULL, or hold NULL for a set.  capacity[s]: entries the outputs of set s
 * hold (fv_offsets[s]: capacity[s] + 1); capacity[s] < n[s] fails the call with ORBFE_ERR_OVERFLOW, the message names the
 * set, and nothing is written for any set.  One grid covers every (set, feature) pair; at most 2^30 descriptors per call. */
int orbfe_bow_transform_batch(orbfe_vocabulary* v, int levelsup, int n_sets, const uint8_t* const* desc, const int* n,
                              const int* capacity, uint32_t* const* bow_ids, double* const* bow_values, int* n_words,
                              uint32_t* const* fv_nodes, uint32_t* const* fv_offsets, uint32_t* const* fv_features,
                              int* n_fv_nodes, uint32_t* const* word_of_feature, uint32_t* const* node_of_feature);

/* Frame::ComputeBoW fused into the extractor: with a vocabulary set, every extract call also runs the tree descent on
 * the descriptors while they are still in HBM (right behind the descriptor kernel, same stream) and keeps the per-
 * keypoint (word, node) pairs of the last collected batch.  orbfe_extract_bow then returns frame `frame` of that batch
 * in the layout of orbfe_bow_transform -- identical results, no descriptor round trip.  v = NULL switches it off.
 * The vocabulary must outlive the extractor's use of it and live on the same device. */
int orbfe_extractor_set_vocabulary(orbfe_extractor* h, orbfe_vocabulary* v, int levelsup);
int orbfe_extract_bow(orbfe_extractor* h, int frame, uint32_t* bow_ids, double* bow_values, int* n_words, uint32_t* fv_nodes,
                      uint32_t* fv_offsets, uint32_t* fv_features, int* n_fv_nodes, uint32_t* word_of_feature,
                      uint32_t* node_of_feature);

/* The two halves of orbfe_extract_bow, for callers that keep many frames and build the vectors later (the stream runner
 * hands out the raw pairs): per keypoint the leaf node its descriptor reached and the node `levelsup` levels above it
 * (cap entries are written, *n_out = the frame's keypoint count); orbfe_bow_assemble turns such pairs into the BowVector /
 * FeatureVector (host bookkeeping only, no GPU work). */
int orbfe_extract_bow_raw(orbfe_extractor* h, int frame, uint32_t* leaf_node, uint32_t* level_node, int cap, int* n_out);
int orbfe_bow_assemble(orbfe_vocabulary* v, const uint32_t* leaf_node, const uint32_t* level_node, int n, uint32_t* bow_ids,
                       double* bow_values, int* n_words, uint32_t* fv_nodes, uint32_t* fv_offsets, uint32_t* fv_features,
                       int* n_fv_nodes, uint32_t* word_of_feature);

/* int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)  (ORBmatcher.cc:154-283;
 * strict_threshold = 0, valid2 = NULL) and int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2,
 * vector<MapPoint*>& vpMatches12)  (:517-650; strict_threshold = 1: `bestDist1 < TH_LOW`).
 * Side 1 is the keyframe whose MapPoints are searched for: valid1[i] != 0 iff keypoint i has a MapPoint that is
 * not bad; valid2 likewise for side 2 (NULL = every keypoint is a candidate, as for a Frame).  angle1 / angle2: the
 * keypoints' angles (needed when check_orientation).  fvX_*: the FeatureVectors in the layout
 * orbfe_bow_transform writes.  matches12[i1] = matched index on side 2 or -1 (capacity n1); for the Frame overload
 * vpMapPointMatches[matches12[i1]] = vpMapPointsKF[i1].  *nmatches = the function's return value.
 * desc1 / desc2 may point to host memory or to 16-byte aligned rows in the matcher's device memory (a resident frame's
 * descriptors, orbfe_frame_descriptors_device): such a side is not copied anywhere. */
int orbfe_search_by_bow(orbfe_matcher* m, const uint8_t* desc1, const float* angle1, const uint8_t* valid1, int n1,
                        const uint32_t* fv1_nodes, const uint32_t* fv1_offsets, const uint32_t* fv1_features, int n_fv1,
                        const uint8_t* desc2, const float* angle2, const uint8_t* valid2, int n2,
                        const uint32_t* fv2_nodes, const uint32_t* fv2_offsets, const uint32_t* fv2_features, int n_fv2,
                        float nnratio, int check_orientation, int strict_threshold, int32_t* matches12, int* nmatches);

/* The SearchByBoW loop of Tracking::Relocalization (src/Tracking.cc:1005-1030: one SearchByBoW(pKF, mCurrentFrame, ...) per
 * candidate keyframe) as one call: n_kf keyframes (side 1: arrays of per-keyframe pointers / sizes) against ONE frame (side 2),
 * one upload, one kernel launch over every (keyframe, common vocabulary node) pair, one download.  matches12[k] / nmatches[k]
 * are exactly what orbfe_search_by_bow returns for keyframe k. */
int orbfe_search_by_bow_batch(orbfe_matcher* m, int n_kf, const uint8_t* const* desc1, const float* const* angle1,
                              const uint8_t* const* valid1, const int* n1, const uint32_t* const* fv1_nodes,
                              const uint32_t* const* fv1_offsets, const uint32_t* const* fv1_features, const int* n_fv1,
                              const uint8_t* desc2, const float* angle2, const uint8_t* valid2, int n2, const uint32_t* fv2_nodes,
                              const uint32_t* fv2_offsets, const uint32_t* fv2_features, int n_fv2, float nnratio,
                              int check_orientation, int strict_threshold, int32_t* const* matches12, int* nmatches);

/* ---------------------------------------------------------------------------------------------
 * Keyframe database.  Replaces the inverted file of KeyFrameDatabase (src/KeyFrameDatabase.cc:38-334) and the
 * mpVoc->score calls around it (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp; src/LoopClosing.cc:125-140): the
 * BowVectors of the map's keyframes live in HBM, one query compares a BowVector with all of them (one wave per
 * keyframe).  include/orbfe/KeyFrameDatabase.h is the drop-in class on top of it.
 *
 * n_words: the vocabulary's size (word ids are < n_words).  scoring: the vocabulary's DBoW2::ScoringType; 0 L1_NORM,
 * 1 L2_NORM, 2 CHI_SQUARE and 5 DOT_PRODUCT are built, 3 KL and 4 BHATTACHARYYA are refused HERE with ORBFE_ERR_INVALID
 * (they need log / a per-word sqrt with the host library's rounding).  capacity_keyframes / capacity_entries: live keyframes
 * and live (word, value) pairs the pool holds; an add beyond either returns ORBFE_ERR_OVERFLOW and changes nothing.  Erased
 * keyframes leave tombstones in the pool; an add that does not fit behind the last keyframe first compacts the pool on the
 * device.  Calls on one handle are serialised by a mutex inside it (like KeyFrameDatabase::mMutex): unlike the other handles
 * it may be shared by threads.  It depends on no extractor, matcher or vocabulary handle.
 * ------------------------------------------------------------------------------------------- */
int orbfe_kfdb_create(int device_id, int n_words, int scoring, int capacity_keyframes, int capacity_entries, orbfe_kfdb** out);
void orbfe_kfdb_destroy(orbfe_kfdb* db);
/* void KeyFrameDatabase::add(KeyFrame* pKF)  (:38-44).  key: the caller's name for the keyframe (the pointer, or mnId); a key
 * that is already in the database is an error (ORBFE_ERR_INVALID).  words ascending (a BowVector's order), n of them (n * 12
 * bytes are uploaded).  The keyframe goes to the BACK of every word's list, also when the key was there before and erased. */
int orbfe_kfdb_add(orbfe_kfdb* db, uint64_t key, const uint32_t* words, const double* values, int n);
/* orbfe_kfdb_add for n keyframes (the add loop of a map load): keyframe j has key keys[j] and n_words[j] (word, value) pairs
 * at words[j] / values[j].  The database afterwards is the database after n single adds in index order (pool order, tombstones,
 * compaction), so every later query returns the same bytes; the mutex is taken once, the entries go up as one staging image.
 * All n keyframes are checked before anything is sent: words not ascending, a key already present or named twice
 * (ORBFE_ERR_INVALID), a capacity exceeded (ORBFE_ERR_OVERFLOW) at entry j fail the whole call -- the message names j -- and
 * change nothing. */
int orbfe_kfdb_add_batch(orbfe_kfdb* db, int n, const uint64_t* keys, const uint32_t* const* words, const double* const* values,
                         const int* n_words);
/* void KeyFrameDatabase::erase(KeyFrame* pKF)  (:46-65); a key that is not in the database: nothing happens, as there. */
int orbfe_kfdb_erase(orbfe_kfdb* db, uint64_t key);
/* void KeyFrameDatabase::clear()  (:67-71) */
int orbfe_kfdb_clear(orbfe_kfdb* db);
int orbfe_kfdb_size(orbfe_kfdb* db, int* n_keyframes, int* n_entries);
/* The inverted-file walk of DetectLoopCandidates (:85-104) / DetectRelocalizationCandidates (:207-222) and the score of every
 * keyframe it meets: every live keyframe that shares at least one word with the query, in the order of first encounter
 * (query words ascending, each word's list front to back = ascending by (first common word, add order)); common[i] = number
 * of shared words, scores[i] = mpVoc->score(query, keyframe) as DBoW2's double, bit for bit (the sum over the common words in
 * ascending word order); the reference's `float si = ...` is the caller's cast.  No exclusion set and no minCommonWords
 * filter are applied: both act on this sequence and belong to the caller.  *n_out = number of such keyframes; if it exceeds
 * cap, the first cap are written and the call returns ORBFE_ERR_OVERFLOW. */
int orbfe_kfdb_query(orbfe_kfdb* db, const uint32_t* q_words, const double* q_values, int nq, uint64_t* keys, int32_t* common,
                     double* scores, int cap, int* n_out);
/* mpVoc->score(query, keyframe keys[i]) for n given keyframes, whether they share a word or not (src/LoopClosing.cc:125-140).
 * A key that is not in the database fails the call with ORBFE_ERR_INVALID before anything is written. */
int orbfe_kfdb_score(orbfe_kfdb* db, const uint32_t* q_words, const double* q_values, int nq, const uint64_t* keys, int n,
                     double* scores);

/* ---------------------------------------------------------------------------------------------
 * Initialiser.  The scoring passes of Initializer::Initialize (src/Initializer.cc:44-121), the consumer of
 * SearchForInitialization's vnMatches12: CheckHomography (:305-388) and CheckFundamental (:390-468) for all RANSAC
 * hypotheses in one call, and the keep-the-best rule of FindHomography / FindFundamental (:148-171, :199-222).  The
 * hypotheses themselves (Normalize, ComputeH21, ComputeF21: cv::SVD) stay with the caller's OpenCV, like ReconstructH / F,
 * CheckRT and Triangulate.  Scores are the reference's floats bit for bit: the same float expressions without contraction,
 * `1.0/(float)` as a double division rounded to float, and the sum over the matches taken in match order.
 *
 * sigma: mSigma.  H21 / H12 (both or neither) and F21: n_hyp matrices of 9 floats, row-major; a model that is not given is not
 * scored and its outputs are left as they are.  scores_*: n_hyp floats, currentScore of every iteration.  best_*: the iteration
 * whose score replaced the running best last, i.e. the first of the largest scores above 0 (a NaN score never wins), or -1 with
 * best_score_* = 0 and all flags 0 when no score is above 0.  inliers_*: vbMatchesInliers of the winner, one byte per match.
 * NULL outputs are skipped.  ORBFE_ERR_INVALID (nothing is written): n_hyp < 1, only one of H21 / H12, no model at all, a
 * matches12 entry outside [-1, n2), frames on another device than m.
 * ------------------------------------------------------------------------------------------- */
/* Initializer.cc:305-468 for n_hyp hypotheses at once, plus the selection of :148-171 / :199-222.  pts: n x 4 floats
 * (u1 v1 u2 v2) in match order.  n = 0 is valid: scores are 0 and best = -1. */
int orbfe_score_init_hypotheses(orbfe_matcher* m, const float* pts, int n, float sigma, int n_hyp, const float* H21,
                                const float* H12, const float* F21, float* scores_h, float* scores_f, int32_t* best_h,
                                int32_t* best_f, float* best_score_h, float* best_score_f, uint8_t* inliers_h /* n */,
                                uint8_t* inliers_f /* n */);
/* The same, from two keypoint arrays (mvKeys1, mvKeys2 = mvKeysUn of the two frames) and vnMatches12 (n1 entries, -1 =
 * unmatched); the matches are compacted in index order as :54-63 does.  *n_matches receives N; inliers_* hold N entries
 * (n1 bytes always suffice). */
int orbfe_score_init_hypotheses_kps(orbfe_matcher* m, const OrbfeKeyPoint* kps1_un, int n1, const OrbfeKeyPoint* kps2_un, int n2,
                                    const int32_t* matches12, float sigma, int n_hyp, const float* H21, const float* H12,
                                    const float* F21, float* scores_h, float* scores_f, int32_t* best_h, int32_t* best_f,
                                    float* best_score_h, float* best_score_f, uint8_t* inliers_h, uint8_t* inliers_f,
                                    int* n_matches);
/* The same, with both frames resident (orbfe_frame; matches12 has orbfe_frame_size(f1) entries): only matches12 and the
 * hypotheses cross the link, the gather from the frames' undistorted keypoints happens on the device.  Both frames are only
 * read (their keypoint coordinates), behind their builds on m's stream: calls of other threads that only read them may overlap. */
int orbfe_score_init_hypotheses_frames(orbfe_matcher* m, orbfe_frame* f1, orbfe_frame* f2, const int32_t* matches12, float sigma,
                                       int n_hyp, const float* H21, const float* H12, const float* F21, float* scores_h,
                                       float* scores_f, int32_t* best_h, int32_t* best_f, float* best_score_h,
                                       float* best_score_f, uint8_t* inliers_h, uint8_t* inliers_f, int* n_matches);

/* ---------------------------------------------------------------------------------------------
 * RANSAC scoring.  The inlier tests of the two solvers that follow the BoW searches: Sim3Solver::CheckInliers with its two
 * Project calls (src/Sim3Solver.cc:343-367, :385-406; LoopClosing::ComputeSim3) and PnPsolver::CheckInliers
 * (src/PnPsolver.cc:313-344; Tracking::Relocalization), for a flat list of hypotheses in one call.  The minimal-set solvers
 * (Sim3Solver::ComputeSim3 with cv::eigen, EPnP's compute_pose) stay with the caller; what comes here are their results.  The
 * selection among the counts (Sim3Solver::iterate, PnPsolver::iterate) is include/orbfe/RansacScoring.h.
 *
 * A call covers n_seg SEGMENTS.  A segment is one solver -- one loop or relocalisation candidate -- with its own correspondences
 * [seg_off[s], seg_off[s + 1]) of corr and its own camera(s); hypothesis k belongs to segment hyp_seg[k].  N of a segment may be 0.
 * counts[k]: mnInliersi of hypothesis k.  masks: mvbInliersi as 64-bit words, bit (i & 63) of word (i >> 6) for correspondence
 * i of the hypothesis' segment, ceil(N / 64) words per hypothesis (none for N = 0), bits at and above N are 0.  The words of
 * hypothesis k start at masks + mask_off[k]; with mask_off == NULL they follow those of hypothesis k - 1, and
 * orbfe_ransac_mask_words gives the total.  counts and masks may each be NULL.  All arrays are host memory.  Inlier bits are the
 * reference's bit for bit: the same expressions without contraction; a NaN error is an outlier; the sign of z is not tested.
 * ORBFE_ERR_INVALID (nothing is sent, no output is written): a NULL matcher, n_seg < 1, n_hyp < 1, a NULL array, seg_off[0] < 0
 * or a decreasing seg_off, hyp_seg[k] outside [0, n_seg), a negative mask_off[k], more than (2^31 - 1) / 12 correspondences
 * or more than 2^31 - 1 mask words in one call.
 * ------------------------------------------------------------------------------------------- */
/* Sim3Solver.cc:343-367.  corr: 12 floats per correspondence -- mvX3Dc1[i] (3), mvX3Dc2[i] (3), mvP1im1[i] (2), mvP2im2[i] (2),
 * (float)mvnMaxError1[i], (float)mvnMaxError2[i].  cams: fx fy cx cy of mK1, then of mK2, per segment.  T12 / T21: per hypothesis
 * the first 12 floats of mT12i / mT21i, i.e. the top three rows of the 4x4, row-major (r00 r01 r02 t0 r10 ...). */
int orbfe_score_sim3_hypotheses(orbfe_matcher* m, int n_seg, const int32_t* seg_off /* n_seg + 1 */, const float* corr,
                                const float* cams /* 8 * n_seg */, int n_hyp, const int32_t* hyp_seg /* n_hyp */,
                                const float* T12 /* 12 * n_hyp */, const float* T21 /* 12 * n_hyp */, int32_t* counts /* n_hyp */,
                                const int64_t* mask_off /* n_hyp or NULL */, uint64_t* masks);
/* PnPsolver.cc:313-344.  corr: 6 floats per correspondence -- mvP3Dw[i] (3), mvP2D[i] (2), mvMaxError[i].  cams: uc vc fu fv per
 * segment, in double.  Rt: per hypothesis mRi (9, row-major) then mti (3), in double. */
int orbfe_score_pnp_hypotheses(orbfe_matcher* m, int n_seg, const int32_t* seg_off /* n_seg + 1 */, const float* corr,
                               const double* cams /* 4 * n_seg */, int n_hyp, const int32_t* hyp_seg /* n_hyp */,
                               const double* Rt /* 12 * n_hyp */, int32_t* counts /* n_hyp */,
                               const int64_t* mask_off /* n_hyp or NULL */, uint64_t* masks);
/* The number of mask words a packed call writes; 0 (and orbfe_last_error) for a layout the scoring calls refuse. */
size_t orbfe_ransac_mask_words(int n_seg, const int32_t* seg_off, int n_hyp, const int32_t* hyp_seg);

/* int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12, vector<pair<size_t,size_t>>&
 * vMatchedPairs)  (ORBmatcher.cc:652-804, with CheckDistEpipolarLine :135-152), from the epipole onwards: the caller
 * computes (ex, ey) (:657-666) and passes F12 row-major.  has_mpX[i] != 0: the keypoint already has a MapPoint and is
 * skipped (:708, :726).  kpsX_un = mvKeysUn; scale_factors2 / level_sigma2_2 = pKF2->mvScaleFactors / mvLevelSigma2
 * (nlevels2 <= 16).  pairs_out: (idx1, idx2) int32 pairs in ascending idx1, capacity n1 pairs; *nmatches = return
 * value = number of pairs.  (The reference never sets vbMatched2, so a keypoint of pKF2 may appear in several pairs.) */
int orbfe_search_for_triangulation(orbfe_matcher* m, const OrbfeKeyPoint* kps1_un, const uint8_t* desc1,
                                   const uint8_t* has_mp1, int n1, const uint32_t* fv1_nodes, const uint32_t* fv1_offsets,
                                   const uint32_t* fv1_features, int n_fv1, const OrbfeKeyPoint* kps2_un,
                                   const uint8_t* desc2, const uint8_t* has_mp2, int n2, const uint32_t* fv2_nodes,
                                   const uint32_t* fv2_offsets, const uint32_t* fv2_features, int n_fv2, const float F12[9],
                                   float ex, float ey, const float* scale_factors2, const float* level_sigma2_2,
                                   int nlevels2, int check_orientation, int32_t* pairs_out, int* nmatches);

/* The SearchForTriangulation loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-232: mpCurrentKeyFrame against
 * each of up to 20 covisible neighbours) on RESIDENT keyframes, all neighbours in one call.  Keypoints and descriptor rows of
 * every keyframe are read where its orbfe_frame holds them; what crosses the link per keyframe is its FeatureVector's feature
 * list (4 bytes per feature) and its MapPoint flags (1 byte per keypoint).
 *
 * Why one call equals the loop.  Triangulating neighbour i's pairs gives keypoints of the current keyframe a MapPoint, and
 * neighbour i + 1 skips those (ORBmatcher.cc:694-699).  That dependency is a mask and nothing more: each idx1 lies under one
 * vocabulary node, vbMatched2 is never set, so the best idx2 of one idx1 depends on no other idx1 (:686-770).  The RAW row of
 * neighbour k -- matches12 before the orientation histogram, computed with the flags at loop entry -- therefore holds the
 * reference's entry for every idx1 that still has no MapPoint when the loop reaches k; the others only have to be dropped,
 * BEFORE the histogram (:745-791), the one place where matches interact.  orbfe_triangulation_finish does that on the host.
 * The contract: while the loop runs, the current keyframe's flags only grow, and a neighbour's own flags change only in its own
 * iteration, after its search.
 *
 * One OrbfeTriangulationNeighbour per neighbour: its resident frame, has_mp2 [orbfe_frame_size(frame2)], its FeatureVector, F12
 * row-major, the epipole (ex, ey) (:657-666), pKF2->mvScaleFactors / mvLevelSigma2 (nlevels2 in 1..16). */
typedef struct OrbfeTriangulationNeighbour {
  orbfe_frame* frame2;
  const uint8_t* has_mp2;
  const uint32_t *fv2_nodes, *fv2_offsets, *fv2_features;
  int n_fv2;
  float F12[9], ex, ey;
  const float *scale_factors2, *level_sigma2_2;
  int nlevels2;
} OrbfeTriangulationNeighbour;
/* matches12_raw: n_nb rows of n1 = orbfe_frame_size(frame1) entries; row k, entry idx1 = the neighbour's keypoint the search
 * takes for idx1, or -1 where nothing matched or has_mp1[idx1] is set.  One upload, one launch, one download, one wait.
 * n_nb == 0 is valid; a neighbour that shares no vocabulary node with frame1 yields a row of -1.  Everything is checked before
 * anything is sent or written; ORBFE_ERR_INVALID names the neighbour for: a keypoint octave of frame2 outside [0, nlevels2), a
 * feature index that is no keypoint of its frame, a frame on another device than m, nlevels2 outside 1..16.  ORBFE_ERR_OVERFLOW:
 * a vocabulary node with more than 65 535 features of a neighbour.  frame1 and every frame2 are only read (coordinates, octaves,
 * descriptor rows), behind their builds on m's stream, and the call returns after its kernel has finished: calls of other threads
 * that only read these frames may overlap, and a frame may be destroyed as soon as the call has returned. */
int orbfe_search_for_triangulation_frames_batch(orbfe_matcher* m, orbfe_frame* frame1, const uint8_t* has_mp1,
                                                const uint32_t* fv1_nodes, const uint32_t* fv1_offsets, const uint32_t* fv1_features,
                                                int n_fv1, int n_nb, const OrbfeTriangulationNeighbour* neighbours,
                                                int32_t* matches12_raw);
/* Host only: one neighbour's result from its raw row, at the moment the loop reaches it.  In this order: entries whose
 * has_mp1_now is set are dropped; the orientation histogram prunes the rest when check_orientation (kps1_un / kps2_un: the
 * two keyframes' mvKeysUn, read for their angles; may be NULL otherwise); the pairs are written in ascending idx1 (capacity n1
 * pairs) and *nmatches is the reference's return value -- exactly what orbfe_search_for_triangulation gives for has_mp1_now.
 * has_mp1_initial: the flags the raw row was computed with.  If has_mp1_now CLEARS one of them the raw row lacks that keypoint:
 * ORBFE_ERR_STALE, nothing written -- search that neighbour singly. */
#define ORBFE_ERR_STALE (-7)     /* a raw triangulation row does not cover the flags it is finished with */
int orbfe_triangulation_finish(const int32_t* matches12_raw_row, int n1, const uint8_t* has_mp1_initial, const uint8_t* has_mp1_now,
                               int check_orientation, const OrbfeKeyPoint* kps1_un, const OrbfeKeyPoint* kps2_un, int n2,
                               int32_t* pairs_out, int* nmatches);
/* One neighbour: a batch of one, finished with the same flags.  orbfe_search_for_triangulation on resident keyframes. */
int orbfe_search_for_triangulation_frames(orbfe_matcher* m, orbfe_frame* frame1, const uint8_t* has_mp1, const uint32_t* fv1_nodes,
                                          const uint32_t* fv1_offsets, const uint32_t* fv1_features, int n_fv1,
                                          const OrbfeTriangulationNeighbour* neighbour, int check_orientation,
                                          const OrbfeKeyPoint* kps1_un, const OrbfeKeyPoint* kps2_un, int32_t* pairs_out, int* nmatches);

/* void Frame::antidistorsionarProyeccionEquidistante(cv::Mat& puntos)  (src/Frame.cc:355-384): os1's
 * equidistant-fisheye keypoint undistortion (camera `modo: 1`), used by Frame::UndistortKeyPoints (:286-320) and
 * Frame::ComputeImageBounds (:322-353).  Host double-precision math on n (x, y) float pairs, in place; K is the
 * float intrinsic matrix {fx, fy, cx, cy}.  (Microseconds of scalar work per frame: it stays on the host.) */
int orbfe_undistort_equidistant(float* xy, int n, float fx, float fy, float cx, float cy);
/* The pinhole branch of the same two callers: cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK)
 * (src/Frame.cc:307, 339; camera `modo: 0` with Camera.k1 != 0).  dist = mDistCoef: k1 k2 p1 p2 [k3 [k4 k5 k6]]
 * (src/Tracking.cc:1221-1243), ndist 0..8.  Host double-precision math, in place. */
int orbfe_undistort_pinhole(float* xy, int n, float fx, float fy, float cx, float cy, const float* dist, int ndist);
/* void Frame::ComputeImageBounds(const cv::Mat& imLeft)  (src/Frame.cc:322-353): bounds = {mnMinX, mnMaxX, mnMinY,
 * mnMaxY}; camera_mode 0 = pinhole (undistorted corners when dist[0] != 0, else the image rectangle), 1 = os1's
 * equidistant fisheye. */
int orbfe_compute_image_bounds(int cols, int rows, int camera_mode, float fx, float fy, float cx, float cy, const float* dist,
                               int ndist, float bounds[4]);

/* Frame::GetFeaturesInArea (src/Frame.cc:209-262) evaluated by the GPU candidate kernel, for the
 * parity tests: indices in reference order.  out[cap]. */
int orbfe_debug_features_in_area(orbfe_matcher* m, const OrbfeKeyPoint* kps_un, int n, const float bounds[4],
                                 float x, float y, float r, int min_level, int max_level, int32_t* out, int cap,
                                 int* n_out);

/* ---------------------------------------------------------------------------------------------
 * ONE camera stream over several GPUs (the single-stream shape: "round-robin frames over GPUs with an in-order
 * completion queue" -- what the reference itself is: one Video thread, one Tracking thread, frames strictly in order,
 * src/main.cc:113-141, System.cc:115-152).  Batch k of the stream is extracted (and matched inside the batch) on device
 * device_ids[k mod n] by an ordinary single-device runner with `depth` batches in flight; orbfe_stream_multi_pop returns the batches
 * strictly in push order whatever order the devices finish in.  No collective, no device-to-device copy: the predecessor of a
 * batch's FIRST frame (the previous batch's last frame, extracted on another device) takes a host bounce and that one pair per batch
 * is matched by the host-array search on the batch's own device.  Results are identical to one orbfe_stream fed the same frames.
 * A device may appear several times in device_ids (more batches in flight on it).  With in_device_memory != 0 the frames of a
 * push must live on the device that push goes to: orbfe_stream_multi_device_of_next_push.
 * The predecessor contract above orbfe_stream_create holds (there are no isolated batches here).  The runner has one row stride for
 * every batch, orbfe_stream_multi_capacity, the same for every device's runner: a push of frames that need more keypoint slots is only
 * accepted while nothing is in flight (it lets go of the batch the caller holds, as _set_* do) and grows every device's runner at once.
 * Everything else as orbfe_stream_*: pointers returned by _pop stay valid until the next _pop; _set_* only while nothing is in flight;
 * push from one thread, pop from one thread; never push more than `depth` + 2 batches PER DEVICE ahead of the pops (a device's runner
 * has depth + 4 result slots and finished batches wait in them for their turn).
 * ------------------------------------------------------------------------------------------- */
typedef struct orbfe_stream_multi orbfe_stream_multi;
int orbfe_stream_multi_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, const int* device_ids,
                              int n_devices, int batch, int depth, orbfe_stream_multi** out);
void orbfe_stream_multi_destroy(orbfe_stream_multi* s);
int orbfe_stream_multi_devices(const orbfe_stream_multi* s);
int orbfe_stream_multi_capacity(const orbfe_stream_multi* s);
int orbfe_stream_multi_device_of_next_push(const orbfe_stream_multi* s);
int orbfe_stream_multi_set_matching(orbfe_stream_multi* s, const float bounds[4], int window_size, float nnratio, int check_orientation);
int orbfe_stream_multi_set_blur_variant(orbfe_stream_multi* s, int variant);
int orbfe_stream_multi_push(orbfe_stream_multi* s, const uint8_t* const* gray, int in_device_memory, int rows, int cols, size_t stride_bytes);
int orbfe_stream_multi_pop(orbfe_stream_multi* s, const OrbfeKeyPoint** kps, const uint8_t** desc, const int** n_kps, const int32_t** matches12,
                           const int** nmatches);
/* orbfe_stream_set_camera / orbfe_stream_xy_un for ONE stream over several devices: the camera goes to every runner, the boundary pairs (a batch's first frame against
 * the last frame of the batch before, popped on another device) are searched on mvKeysUn too, and _xy_un returns mvKeysUn of the
 * last popped batch, [batch][orbfe_stream_multi_capacity][2] floats, valid until the next pop. */
int orbfe_stream_multi_set_camera(orbfe_stream_multi* s, int camera_mode, float fx, float fy, float cx, float cy, const float* dist,
                                  int ndist);
int orbfe_stream_multi_xy_un(orbfe_stream_multi* s, const float** xy_un);
int orbfe_stream_multi_set_camera_equidistant(orbfe_stream_multi* s, float fx, float fy, float cx, float cy);
int orbfe_stream_multi_equidistant_stats(orbfe_stream_multi* s, long long stats[3]);

#ifdef __cplusplus
}
#endif
#endif /* ORBFE_H_ */
