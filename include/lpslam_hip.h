/*
 * lpslam_hip.h -- C ABI of the MI355X (gfx950) hot path of lpslam: ORB extraction, descriptor matching and
 * SE3 bundle adjustment.  This is the "thin HIP C-ABI layer" beneath the C++ host mirror of the reference's
 * Interface / Tracker plugin surface (lpslam_amd/host/).  Plain pointers and sizes only; every entry point
 * returns an int status (0 = LPSLAM_HIP_OK) and never throws; lpslam_hip_last_error() gives the message.
 *
 * What each group replaces in the reference (paths relative to /root/reference):
 *   context / frames    openvslam::system construction + feed_stereo_frame / feed_monocular_frame
 *                       (src/Trackers/OpenVSLAMTrackerBase.cpp:238-239,
 *                        src/Trackers/OpenVSLAMStereoTracker.cpp:293-295, src/Trackers/OpenVSLAMTracker.cpp:120)
 *   front-end config    the Feature.* block of the generated tracker YAML
 *                       (src/Trackers/OpenVSLAMTrackerBase.cpp:193-198) and Camera.* (:161-190)
 *   keypoint readback   get_frame_state().curr_keypts (src/Trackers/OpenVSLAMStereoTracker.cpp:302-317)
 *   stereo matching     depth_threshold / focal_x_baseline parameters (src/Trackers/OpenVSLAMTrackerBase.cpp:188-201,
 *                       src/Interface/LpSlamTypes.h:219-222)
 *   bundle adjustment   the mapping / global-optimisation threads started by startup()
 *                       (src/Trackers/OpenVSLAMTrackerBase.cpp:239,250-255)
 * The arithmetic itself lives in absent third-party code (OpenVSLAM fork, g2o@691dc51, OpenCV); see DESIGN.md.
 */

/* ---- environment switches ------------------------------------------------------------------------------
 * Every LPSLAM_HIP_* variable the library and the host plugin read, each once per process, with its default.  This list is held to
 * the code by tests/test_abi_cpu.py; what was measured and removed is in DESIGN.md section 20.
 *
 * Behaviour:
 *   LPSLAM_HIP_FLAT_PRIORITIES      0     1: every stream at the default priority (lpslam_hip_set_flat_priorities)
 *   LPSLAM_HIP_NO_QUEUE_SPREAD      unset set: a flat process puts no placeholder streams in front of a context's main stream
 *   LPSLAM_HIP_POOL_SESSIONS        16    sessions a session pool holds (0 .. 64; lpslam_hip_create_session)
 *   LPSLAM_HIP_POOL_CAP_MB          unset bound of a context's cache of released device blocks (unset: 1/32 of the device, <= 16 GB)
 *   LPSLAM_HIP_SHARED_LAUNCHES      2     0 never, 1 always, 2 when two or more sessions are tracking (lpslam_hip_set_shared_launches)
 *   LPSLAM_HIP_SHARE_WINDOW_US      30    a shared matcher / pose request goes out at the latest this long after the oldest one came
 *   LPSLAM_HIP_SHARE_QUIET_US       2     ... or when no matcher request has arrived for this long (sessions without frame hints)
 *   LPSLAM_HIP_CW_MIN_BATCH         40    windows in a batch from which on small dense systems are factored one workgroup each
 *   LPSLAM_HIP_BA_SOLVER            unset "dense": no band plan, every window takes the dense solver
 *   LPSLAM_HIP_BA_GROUP             32    landmarks per group of the band path's Schur kernel (4 .. 64)
 *   LPSLAM_HIP_BA_TWO_LAUNCH_UPDATE 0     1: solve / update and trial / decision as two launches per iteration instead of one
 *   LPSLAM_HIP_BA_GRAPH             unset 1 / 0: graph replay of the solver's launch chain forced on / off (unset: on, except under a profiler)
 * Development traces (set to anything: lines on stderr, no change of behaviour):
 *   LPSLAM_HIP_BA_TRACE             the solver chosen for every problem created
 *   LPSLAM_HIP_MATCH_TRACE          timings of the window matchers' and the vocabulary (bag-of-words) calls
 *   LPSLAM_HIP_PO_TRACE             every pose optimisation: observations, inliers, passes, time
 *   LPSLAM_HIP_SHARE_TRACE          every shared launch, and the role streams chosen
 */
#ifndef LPSLAM_HIP_H
#define LPSLAM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPSLAM_HIP_OK 0
#define LPSLAM_HIP_ERR_INVALID 1      /* bad argument / unsupported configuration */
#define LPSLAM_HIP_ERR_DEVICE 2       /* HIP runtime error (no device, allocation, launch) */
#define LPSLAM_HIP_ERR_CAPACITY 3     /* caller buffer too small / batch exceeds context capacity */

#define LPSLAM_HIP_MAX_LEVELS 16

/* Memory layout of cv::KeyPoint (what get_frame_state().curr_keypts holds). */
typedef struct lpslam_hip_keypoint {
    float x, y;        /* level-0 pixel coordinates                          */
    float size;        /* 31 * scale_factor^octave, truncated                */
    float angle;       /* degrees [0,360)                                    */
    float response;    /* FAST score                                         */
    int32_t octave;
    int32_t class_id;  /* -1                                                 */
} lpslam_hip_keypoint;

/* FAST candidate in border-relative coordinates of its pyramid level (parity/debug readback). */
typedef struct lpslam_hip_corner {
    int32_t x, y, score;
} lpslam_hip_corner;

typedef struct lpslam_hip_frontend_config {
    int32_t width, height;        /* Camera.cols / Camera.rows                               */
    int32_t max_keypoints;        /* Feature.max_num_keypoints  (slamKeypoints)              */
    float   scale_factor;         /* Feature.scale_factor       (1.2)                        */
    int32_t num_levels;           /* Feature.num_levels         (3 generated, 8 in BASELINE) */
    int32_t ini_fast_threshold;   /* Feature.ini_fast_threshold (20)                         */
    int32_t min_fast_threshold;   /* Feature.min_fast_threshold (7)                          */
    int32_t max_images;           /* images resident per batch (a stereo frame is 2 images)  */
    int32_t device;               /* HIP device ordinal                                      */
} lpslam_hip_frontend_config;

typedef struct lpslam_hip_ctx lpslam_hip_ctx;

const char* lpslam_hip_last_error(void);
int lpslam_hip_device_count(int* count);

/* ---- context ------------------------------------------------------------------------------------------- */
/* Accepted configurations: an image of at least 64 x 64; every pyramid level larger than 45 px and smaller than 4134 px on both axes,
 * with fewer than 2048 FAST cells; a per-level keypoint quota of 0 .. 2000; thresholds >= 0 in either order; and, per level, at most
 * 256 quad-tree root columns and 256 root rows (the rounded aspect ratio of the level inside its 19-px border: no level beyond
 * 256 : 1) with fewer than 511 roots in all.  Anything else: LPSLAM_HIP_ERR_INVALID, the message names the level. */
int lpslam_hip_create(const lpslam_hip_frontend_config* cfg, lpslam_hip_ctx** out);
void lpslam_hip_destroy(lpslam_hip_ctx* ctx);
/* hipStream_t all work of this context is enqueued on (for event timing / interop). */
void* lpslam_hip_stream(lpslam_hip_ctx* ctx);
/* Keep `cus_per_xcd` compute units of every XCD free of the front end's kernels (0 = none, the default; at most 16): a bundle
 * adjustment that runs beside the front end -- the reference's mapping thread beside its tracking thread,
 * src/Trackers/OpenVSLAMTrackerBase.cpp:238 (openvslam::system starts both) -- otherwise stands still while front-end workgroups
 * fill every compute unit's LDS.  The context's streams are re-created: call it on an idle context, outside a prefetch section. */
int lpslam_hip_set_mapping_reserve(lpslam_hip_ctx* ctx, int32_t cus_per_xcd);
/* Test hook for the reserve (no reference counterpart): for `microseconds` (<= 50 000) one workgroup holds the whole LDS of every
 * compute unit that is NOT reserved, on a stream of its own; *landed (may be NULL) = how many sit.  Extraction launched meanwhile
 * finds room on the reserved compute units only -- the placement under which it must still complete (tests/test_frontend_gpu.py). */
int lpslam_hip_debug_occupy_unreserved(lpslam_hip_ctx* ctx, int32_t microseconds, int32_t* landed);
/* Process-wide: create the streams of contexts made FROM NOW ON at the default priority (1) or in the three classes (0, the default: main /
 * low-priority prefetch / high-priority solves; -1: back to the environment, LPSLAM_HIP_FLAT_PRIORITIES).  A process that hosts many
 * sessions per GPU (one LpSlamManager per sequence, src/Manager/SlamManager.cpp:54-61) should set 1 FIRST, before anything in it has
 * created a stream: every priority class takes its own set of hardware queues, beyond a few the command processor time-slices them, and
 * one high-priority stream ever created in the process halves the aggregate of the sessions that follow.  In a flat
 * process context k puts k mod 4 placeholder streams in front of its main stream, so that the contexts' main streams spread over the
 * process' four hardware queues (LPSLAM_HIP_NO_QUEUE_SPREAD=1 switches that off: measurements).  Called with 1 AFTER a priority stream has
 * been created in the process it changes nothing, says so on stderr and returns LPSLAM_HIP_ERR_INVALID (the caller must not believe it
 * runs flat); 2 = flat from now on although it is late (tests and measurements of that case). */
int lpslam_hip_set_flat_priorities(int32_t flat);
/* Process-wide: launches shared by the sessions of a process.  The reference runs one manager per sequence, one frame in flight each
 * (src/Manager/SlamManager.cpp:54-61,191-201); N of them on one GPU issue N chains of small latency-bound launches.  With sharing the
 * window matchers' first scan and the pose optimiser of every session that is tracking at that moment go out as ONE launch each
 * (blockIdx = request; per-request result blocks and completion flags as in the unshared call, same device code, same bits).
 * mode 2 (default): when two or more contexts of the device have made such calls within the last few milliseconds; 1: always, a lone
 * session too (tests); 0: never; -1: back to the environment (LPSLAM_HIP_SHARED_LAUNCHES).  LPSLAM_HIP_SHARE_WINDOW_US (30) /
 * LPSLAM_HIP_SHARE_QUIET_US (2) bound how long a request waits for the other sessions'. */
int lpslam_hip_set_shared_launches(int32_t mode);
/* How many shared launches a device has seen and how many requests they carried (measurement / test hook). */
int lpslam_hip_shared_launch_counters(int32_t device, int64_t* batches, int64_t* requests);
/* A context for one SESSION of a process that may host several (what a tracker plugin creates: one per LpSlamManager,
 * src/Manager/SlamManager.cpp:54-61).  Same calls, same results as a context of lpslam_hip_create; its per-image arrays are slices of a
 * pool that the sessions of one device and front-end configuration share (LPSLAM_HIP_POOL_SESSIONS, default 16; max_images <= 8), so
 * that lpslam_hip_front_end can put the frames several sessions have pending through ONE launch chain.  A session beyond the pool's
 * capacity silently gets arrays of its own. */
int lpslam_hip_create_session(const lpslam_hip_frontend_config* cfg, lpslam_hip_ctx** out);
/* One frame's front end behind its uploads, as one asynchronous call: lpslam_hip_extract_range(image, stereo ? 2 : 1), for stereo
 * lpslam_hip_match_stereo(image, image + 1, fxb, baseline), then lpslam_hip_prefetch_frame(image, stereo) -- the per-frame work of
 * feed_stereo_frame / feed_monocular_frame up to the tracking step (src/Trackers/OpenVSLAMStereoTracker.cpp:293-295).  Inside or outside
 * a prefetch section.  With shared launches on and two or more sessions of a pool submitting, their frames are extracted together. */
int lpslam_hip_front_end(lpslam_hip_ctx* ctx, int image, int32_t stereo, float focal_x_baseline, float baseline);
/* The same with the frame itself: lpslam_hip_upload_image of `left` into `image` (and of `right` into image + 1; NULL = monocular),
 * then lpslam_hip_front_end.  A shared front end uploads the frames at the head of its launch chain. */
int lpslam_hip_front_end_images(lpslam_hip_ctx* ctx, int image, const uint8_t* left, const uint8_t* right, int32_t stride,
                                float focal_x_baseline, float baseline);
/* A hint for shared launches: this session will make no more latency-bound requests (window matchers, pose optimisations) for the frame
 * it collected with lpslam_hip_get_frame / _view -- the other sessions' requests stop waiting for it.  Optional; a tracker calls it
 * when the frame's pose is final, before its keyframe work. */
int lpslam_hip_frame_done(lpslam_hip_ctx* ctx);
int lpslam_hip_shared_front_end_counters(int32_t device, int64_t* batches, int64_t* requests);
int lpslam_hip_shared_solve_counters(int32_t device, int64_t* batches, int64_t* requests);
int lpslam_hip_sync(lpslam_hip_ctx* ctx);
/* Geometry derived from the configuration (pyramid sizes, per-level keypoint quota). */
int lpslam_hip_level_info(lpslam_hip_ctx* ctx, int32_t* widths, int32_t* heights, int32_t* pitches,
                          int32_t* quotas, float* scale_factors);
/* Upper bound of keypoints one image can yield (sum of quota+3 over levels). */
int lpslam_hip_max_keypoints_per_image(lpslam_hip_ctx* ctx);

/* Event timers on the context stream (HIP events; used by bench.py to time individual kernels in place). */
#define LPSLAM_HIP_MAX_TIMERS 64
int lpslam_hip_timer_begin(lpslam_hip_ctx* ctx, int slot);
int lpslam_hip_timer_end(lpslam_hip_ctx* ctx, int slot);
/* Waits for the end event of `slot` and returns the elapsed milliseconds. */
int lpslam_hip_timer_read(lpslam_hip_ctx* ctx, int slot, float* ms);

/* ---- frames: images resident in HBM --------------------------------------------------------------------- */
/* Device address and row pitch of level 0 of image slot `image` (write frames there directly, e.g. from a
 * capture DMA or another kernel), or upload from host memory (tightly packed rows of `stride` bytes). */
int lpslam_hip_image_ptr(lpslam_hip_ctx* ctx, int image, void** dev_ptr, int32_t* pitch);
int lpslam_hip_upload_image(lpslam_hip_ctx* ctx, int image, const uint8_t* host, int32_t stride);
/* Page-locked frames and asynchronous uploads.  The reference aliases the caller's 8-bit frame (zero copy, the caller keeps it
 * alive until it is consumed: src/Manager/SlamManager.cpp:1082-1085); the counterpart on a discrete GPU is a frame in page-locked
 * host memory -- lpslam_hip_host_alloc (what a capture layer fills) or the caller's own buffer pinned in place with
 * lpslam_hip_host_register -- copied by the DMA engines on a copy stream of the context while kernels of earlier frames run.
 * lpslam_hip_upload_images_async enqueues the copies of n frames (hosts[i] -> slot first + i; every frame `stride` bytes per row)
 * and returns at once.  Ordering: the copies start after the work enqueued on the context BEFORE this call (it may still read the
 * slots); lpslam_hip_extract* / stage_pyramid of a slot wait for its copy on the device.  The frames must stay valid and unchanged
 * until such an extraction has been synchronised (lpslam_hip_sync, a get_* call).  Frames in pageable memory work but are staged by
 * the runtime inside the call. */
int lpslam_hip_host_alloc(lpslam_hip_ctx* ctx, size_t bytes, void** out);
int lpslam_hip_host_free(lpslam_hip_ctx* ctx, void* p);
int lpslam_hip_host_register(lpslam_hip_ctx* ctx, void* p, size_t bytes);
int lpslam_hip_host_unregister(lpslam_hip_ctx* ctx, void* p);
int lpslam_hip_upload_images_async(lpslam_hip_ctx* ctx, int first, int n, const uint8_t* const* hosts, int32_t stride);
/* On-device undistort / rectify: replaces the per-frame cv::remap(INTER_LINEAR) of ImageProcessing::Undistort::undistort
 * (reference: src/Utils/ImageProcessing.h:245-249; called for both eyes per frame, src/Trackers/OpenVSLAMStereoTracker.cpp:
 * 198-213).  map_x / map_y are the CV_32FC1 maps of one eye (0 = left, 1 = right), width x height floats, as
 * cv::initUndistortRectifyMap / cv::fisheye::initUndistortRectifyMap produce them (the host library builds them from the
 * LpSlamCameraConfiguration pair, lpslam_amd/host/rectify.h).  upload_raw_image copies the distorted frame to HBM and remaps it
 * into level 0 of the image slot, bit-identical to cv::remap with BORDER_CONSTANT 0. */
int lpslam_hip_set_rectify_map(lpslam_hip_ctx* ctx, int32_t eye, const float* map_x, const float* map_y);
int lpslam_hip_upload_raw_image(lpslam_hip_ctx* ctx, int image, int32_t eye, const uint8_t* host, int32_t stride);
/* remaps the raw frame already staged in HBM (the last upload_raw_image) into another slot: the device-side step alone */
int lpslam_hip_remap_staged(lpslam_hip_ctx* ctx, int image, int32_t eye);

/* Intensity adjustment on the device: replaces the per-frame host call of the reference's AdjustIntensity processor
 * (src/Processor/AdjustIntensityProcessor.h:10-41 -> ImageProcessing::imadjust(image, out, nullopt, nullopt, -0.3, 1.4),
 * src/Utils/ImageProcessing.h:258-370; run on both eyes of every frame before the trackers, src/Manager/SlamManager.cpp:114-116).
 * Per image: the histogram of its pixels, the grey levels lo / hi that cut off low_fraction of the pixels at the dark end and
 * 1 - high_fraction at the bright end, and the linear map that sends lo to low_out and hi to high_out (both in units of the full 8-bit
 * range), applied through a 256-entry table in single precision, unfused, rounded half to even and saturated (DESIGN.md section 17
 * has the arithmetic word for word; lo == hi leaves the image unchanged).  The reference's constants are {-0.3, 1.4, 0.01, 0.99}.
 * Needs low_out < high_out (finite), 0 <= low_fraction < high_fraction <= 1 and fewer than 2^24 pixels per image; otherwise
 * LPSLAM_HIP_ERR_INVALID / LPSLAM_HIP_ERR_CAPACITY, and nothing is enqueued.
 *   lpslam_hip_adjust_intensity           image slots [first, first + n) in place on level 0, asynchronous, behind their uploads: two
 *                                         launches for all n images, no host synchronisation; inside or outside a prefetch section.
 *   lpslam_hip_upload_raw_image_adjusted  lpslam_hip_upload_raw_image with the RAW frame adjusted before it is remapped, the order of
 *                                         the reference (SlamManager.cpp:114 runs before OpenVSLAMStereoTracker.cpp:198-213).
 *   lpslam_hip_front_end_images_adjusted  lpslam_hip_front_end_images with the adjustment of the slot (pair) between the uploads and
 *                                         the front end: a tracker's one call per frame stays one call.
 *   lpslam_hip_adjust_intensity_last      test hook, synchronising: lo, hi and the 256 histogram words of the last adjustment of a slot
 *                                         (any of the three outputs may be NULL). */
typedef struct lpslam_hip_adjust_params {
    double low_out, high_out;             /* where lo and hi go, in units of 255 (the reference: -0.3, 1.4) */
    double low_fraction, high_fraction;   /* the quantiles that define lo and hi (the reference: 0.01, 0.99)  */
} lpslam_hip_adjust_params;
int lpslam_hip_adjust_intensity(lpslam_hip_ctx* ctx, int first, int n, const lpslam_hip_adjust_params* params);
int lpslam_hip_upload_raw_image_adjusted(lpslam_hip_ctx* ctx, int image, int32_t eye, const uint8_t* host, int32_t stride,
                                         const lpslam_hip_adjust_params* params);
int lpslam_hip_front_end_images_adjusted(lpslam_hip_ctx* ctx, int image, const uint8_t* left, const uint8_t* right, int32_t stride,
                                         float focal_x_baseline, float baseline, const lpslam_hip_adjust_params* params);
int lpslam_hip_adjust_intensity_last(lpslam_hip_ctx* ctx, int image, int32_t* lo, int32_t* hi, uint32_t* hist256);

/* Colour and YUV frames: the grey conversion of the reference's ingest (cv::cvtColor in src/Manager/SlamManager.cpp:1051-1063,
 * 1190-1260) on the device, behind the upload and in front of everything else: convert, then adjust (SlamManager.cpp:114), then
 * rectify (OpenVSLAMStereoTracker.cpp:198-213).  The arithmetic is integer and exact:
 *   RGB8 / BGR8   3 bytes per pixel; grey = (R 4899 + G 9617 + B 1868 + 8192) >> 14, BGR8 swaps the roles of bytes 0 and 2
 *   NV12          a width x height Y plane at `data` (rows `stride` bytes apart), then height / 2 rows of interleaved U V pairs, one
 *                 pair per 2 x 2 block, at `chroma` (rows `chroma_stride` apart; NULL = right behind the Y plane, at
 *                 data + stride * height, with the Y plane's stride); width and height even
 *   UYVY          bytes U0 Y0 V0 Y1 per pixel pair, 2 width bytes per row; width even
 *   YUV -> RGB    BT.601 limited range, chroma replicated; then the grey formula
 *   GRAY8         1 byte per pixel: the call behaves exactly as the grey call it is the colour form of
 * The frame is copied to page-locked staging and from there to a staging block in HBM (both per slot, up to 3 width height bytes,
 * allocated at the first colour frame of the context: grey-only contexts pay nothing); one kernel launch -- both eyes of a frame in
 * the same launch -- writes level 0 of the slot(s), or the raw-frame block in front of the remap.  Asynchronous, no host
 * synchronisation, inside or outside a prefetch section; a shared front end waits for it as it waits for an adjustment.
 * An unknown format, a null pointer, an odd width / height where the format needs an even one or a stride smaller than a row:
 * LPSLAM_HIP_ERR_INVALID, and nothing is enqueued.
 *   lpslam_hip_upload_pixels      the colour form of lpslam_hip_upload_image
 *   lpslam_hip_upload_raw_pixels  the colour form of lpslam_hip_upload_raw_image (params NULL) / _adjusted (params given)
 *   lpslam_hip_front_end_pixels   the colour form of lpslam_hip_front_end_images (params NULL) / _adjusted (params given); right NULL =
 *                                 monocular */
enum { LPSLAM_HIP_PIXEL_GRAY8 = 0, LPSLAM_HIP_PIXEL_RGB8 = 1, LPSLAM_HIP_PIXEL_BGR8 = 2, LPSLAM_HIP_PIXEL_NV12 = 3, LPSLAM_HIP_PIXEL_UYVY = 4 };
typedef struct lpslam_hip_pixels {
    const uint8_t* data;      /* first row (NV12: of the Y plane) */
    int32_t stride;           /* bytes between rows of `data` */
    const uint8_t* chroma;    /* NV12 only: the interleaved U V rows; NULL = data + stride * height */
    int32_t chroma_stride;    /* NV12 only, with a non-NULL chroma: bytes between its rows */
    int32_t format;           /* LPSLAM_HIP_PIXEL_* */
} lpslam_hip_pixels;
int lpslam_hip_upload_pixels(lpslam_hip_ctx* ctx, int image, const lpslam_hip_pixels* pixels);
int lpslam_hip_upload_raw_pixels(lpslam_hip_ctx* ctx, int image, int32_t eye, const lpslam_hip_pixels* pixels, const lpslam_hip_adjust_params* params);
int lpslam_hip_front_end_pixels(lpslam_hip_ctx* ctx, int image, const lpslam_hip_pixels* left, const lpslam_hip_pixels* right,
                                float focal_x_baseline, float baseline, const lpslam_hip_adjust_params* params);

/* Prefetch: between prefetch_begin and prefetch_end every upload / remap / extract / stereo-match call of this context is enqueued
 * on a second stream, so the front end of the NEXT frame (into image slots nothing else touches) runs on the GPU beside the
 * matching and pose optimisation of the current one; prefetch_join makes the context's main stream wait (on the device, not the
 * host) for the last prefetch section before the first call that reads those slots.  The reference overlaps the same way with
 * its frame queue and worker thread (src/Manager/SlamManager.cpp:54-61: the next frame is decoded while the tracker runs). */
int lpslam_hip_prefetch_begin(lpslam_hip_ctx* ctx);
int lpslam_hip_prefetch_end(lpslam_hip_ctx* ctx);
int lpslam_hip_prefetch_join(lpslam_hip_ctx* ctx);

/* Camera mask of one eye (0 = left: even image slots, 1 = right: odd image slots): a width x height byte image, 0 = masked out,
 * NULL removes it.  Replaces the `mask` argument of feed_stereo_frame / feed_monocular_frame
 * (src/Trackers/OpenVSLAMStereoTracker.cpp:293, masks built by OpenVSLAMTrackerBase::configureMasks, OpenVSLAMTrackerBase.cpp:331-380):
 * [UPSTREAM] orb_extractor skips a FAST cell with a corner in the mask and drops every corner whose own position is masked. */
int lpslam_hip_set_mask(lpslam_hip_ctx* ctx, int32_t eye, const uint8_t* mask, int32_t stride);

/* ---- ORB front end (asynchronous on the context stream) -------------------------------------------------- */
/* pyramid -> FAST (64-px cells, ini/min threshold) -> quad-tree distribution -> orientation + rBRIEF,
 * for image slots [0, n_images). */
int lpslam_hip_extract(lpslam_hip_ctx* ctx, int n_images);
/* Same for image slots [first, first + n_images): lets a tracker keep the previous frame resident (ping-pong). */
int lpslam_hip_extract_range(lpslam_hip_ctx* ctx, int first, int n_images);
/* Individual stages (lpslam_hip_extract = these four in order); exposed for profiling and parity tests. */
int lpslam_hip_stage_pyramid(lpslam_hip_ctx* ctx, int n_images);
int lpslam_hip_stage_fast(lpslam_hip_ctx* ctx, int n_images);
int lpslam_hip_stage_distribute(lpslam_hip_ctx* ctx, int n_images);
int lpslam_hip_stage_describe(lpslam_hip_ctx* ctx, int n_images);

/* ---- fisheye keypoints (monocular tracker) ---------------------------------------------------------------- */
/* The equidistant camera model of a monocular session: the reference hands Camera.model = fisheye with k1 .. k4 to its tracker
 * (src/Trackers/OpenVSLAMTrackerBase.cpp:170-175), which undistorts every keypoint ([UPSTREAM] camera::fisheye::undistort_keypoints =
 * cv::fisheye::undistortPoints with R = I, P = K) and works in undistorted pinhole coordinates from there on.  max_angle in radians:
 * a keypoint whose ray lies further from the axis, or beyond 90 degrees, or whose iteration did not converge, is REMOVED
 * (lpslam_amd/csrc/fisheye_math.h holds the definition, DESIGN.md section 30 the reasons). */
typedef struct lpslam_hip_fisheye {
    double fx, fy, cx, cy;
    double k[4];
    double max_angle;
} lpslam_hip_fisheye;
/* Sets (NULL: clears) the model of every image slot of the context; synchronises the device.  Non-finite values, fx or fy <= 0, or
 * max_angle outside (0, 89 degrees]: LPSLAM_HIP_ERR_INVALID and the context keeps what it had.  With a model set, lpslam_hip_extract,
 * lpslam_hip_extract_range and every lpslam_hip_front_end call run the stage below after the descriptors; lpslam_hip_match_stereo and
 * lpslam_hip_match_stereo_strided answer LPSLAM_HIP_ERR_INVALID (stereo frames are rectified: the stereo tracker sets no model). */
int lpslam_hip_set_keypoint_camera(lpslam_hip_ctx* ctx, const lpslam_hip_fisheye* model);
/* The fifth stage, beside the four above, for image slots [0, n_images): x, y of every keypoint become the undistorted position,
 * invalid keypoints are removed from the keypoint and the descriptor array together (survivors keep their order, every other field
 * its bits) and the slot's count is rewritten.  Without a model: LPSLAM_HIP_OK, nothing is launched. */
int lpslam_hip_stage_undistort(lpslam_hip_ctx* ctx, int n_images);
/* How many keypoints the last run of that stage removed from slot `image` (0 when it has not run); call it once the slot's frame has
 * been collected.  Synchronising. */
int lpslam_hip_undistort_dropped(lpslam_hip_ctx* ctx, int image, int32_t* dropped);
/* The stage's arithmetic on caller points (host memory): xy = n pairs in, xy_out = n pairs out, valid = n bytes (1 / 0; the pair of
 * an invalid point is left as NaN).  The same device function, no compaction.  Synchronising. */
int lpslam_hip_undistort_points(lpslam_hip_ctx* ctx, const lpslam_hip_fisheye* model, const float* xy, int32_t n, float* xy_out, uint8_t* valid);
/* The radial-tangential ("perspective") camera model of a monocular session: the reference hands its configuration file, with
 * Camera.model = perspective and k1, k2, p1, p2, k3, to its tracker unchanged (src/Trackers/OpenVSLAMTrackerBase.cpp:114-123), which
 * undistorts every keypoint ([UPSTREAM] camera::perspective::undistort_keypoints = cv::undistortPoints with R = I, P = K: five
 * fixed-point steps).  A keypoint whose denominator is not positive in one of the steps, or whose result does not map back to within
 * half a pixel of it, is REMOVED (lpslam_amd/csrc/radtan_math.h holds the definition, DESIGN.md section 32 the reasons). */
typedef struct lpslam_hip_radtan {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3;
} lpslam_hip_radtan;
/* As lpslam_hip_set_keypoint_camera, for this model: every image slot of the context, synchronising, the same stage and the same
 * stereo refusals.  Non-finite values or fx, fy <= 0: LPSLAM_HIP_ERR_INVALID and the context keeps what it had.  NULL, or all five
 * coefficients exactly 0, clears the model.  A context has ONE model: either setter replaces whatever the other one set.
 * lpslam_hip_stage_undistort and lpslam_hip_undistort_dropped serve both kinds. */
int lpslam_hip_set_keypoint_camera_radtan(lpslam_hip_ctx* ctx, const lpslam_hip_radtan* model);
/* As lpslam_hip_undistort_points, for this model (zero coefficients are evaluated like any others: the identity). */
int lpslam_hip_undistort_points_radtan(lpslam_hip_ctx* ctx, const lpslam_hip_radtan* model, const float* xy, int32_t n, float* xy_out, uint8_t* valid);

/* Synchronising readbacks (device -> caller memory). */
int lpslam_hip_keypoint_count(lpslam_hip_ctx* ctx, int image, int32_t* count);
int lpslam_hip_get_keypoints(lpslam_hip_ctx* ctx, int image, lpslam_hip_keypoint* kpts, uint8_t* desc32,
                             int32_t capacity, int32_t* count);
/* Everything the tracker reads back per frame in one round trip: keypoints, descriptors and (after lpslam_hip_match_stereo on
 * this slot as the left image) the stereo columns of lpslam_hip_get_stereo.  Any output pointer may be NULL.  What
 * openvslam::data::frame holds after extraction: keypoints, descriptors, stereo_x_right, depths ([UPSTREAM] data/frame.h;
 * reached through feed_stereo_frame, src/Trackers/OpenVSLAMStereoTracker.cpp:293-295).  Not re-entrant per context. */
int lpslam_hip_get_frame(lpslam_hip_ctx* ctx, int image, lpslam_hip_keypoint* kpts, uint8_t* desc32, float* stereo_x_right,
                         float* depths, int32_t capacity, int32_t* count);
/* Queues the read-back of slot `image` behind whatever the calling thread has enqueued for it (inside a prefetch section: behind the
 * next frame's extraction and stereo match): the results are in page-locked memory before lpslam_hip_get_frame(image, ...) asks for
 * them, which then only checks a flag.  Anything that rewrites the slot's results afterwards voids the copy (get_frame then reads
 * back as usual). */
int lpslam_hip_prefetch_frame(lpslam_hip_ctx* ctx, int image, int32_t with_stereo);
/* lpslam_hip_get_frame without the copy out: pointers into the context's page-locked block that holds the slot's results (first
 * *count entries each), valid until the next lpslam_hip_get_frame / _view / lpslam_hip_prefetch_frame call on this context.  The
 * caller copies what it keeps, once, into storage of the right size. */
int lpslam_hip_get_frame_view(lpslam_hip_ctx* ctx, int image, int32_t with_stereo, const lpslam_hip_keypoint** kpts, const uint8_t** desc32,
                              const float** stereo_x_right, const float** depths, int32_t* count);
int lpslam_hip_get_pyramid_level(lpslam_hip_ctx* ctx, int image, int level, uint8_t* out, int32_t out_stride);
int lpslam_hip_get_candidates(lpslam_hip_ctx* ctx, int image, int level, lpslam_hip_corner* out,
                              int32_t capacity, int32_t* count);
/* Device-resident results (valid until the next extract on this context): keypoints [max_per_image],
 * descriptors [max_per_image][32], count (int32). */
int lpslam_hip_keypoint_buffers(lpslam_hip_ctx* ctx, int image, void** kpts_dev, void** desc_dev, void** count_dev);

/* ---- matching -------------------------------------------------------------------------------------------- */
/* Brute-force Hamming 2-NN of the descriptors of image slot `query` against those of slot `train`
 * (first minimum wins).  Results stay on the device until fetched. */
int lpslam_hip_match_bf(lpslam_hip_ctx* ctx, int query, int train);
int lpslam_hip_get_bf_knn2(lpslam_hip_ctx* ctx, int query, int32_t* best_idx, int32_t* best_dist,
                           int32_t* second_dist, int32_t capacity, int32_t* count);
/* knn2 + max distance + Lowe ratio (<= 0 disables) + optional cross check -> (query, train, distance). */
int lpslam_hip_get_bf_matches(lpslam_hip_ctx* ctx, int query, int train, int32_t max_dist, float ratio,
                              int32_t cross_check, int32_t* out_q, int32_t* out_t, int32_t* out_d,
                              int32_t capacity, int32_t* count);
/* The three calls a keyframe comparison makes -- lpslam_hip_set_descriptors(scratch, train_desc32, n_train), lpslam_hip_match_bf(query,
 * scratch), lpslam_hip_get_bf_matches(query, scratch, ...) -- as ONE call with ONE wait: the descriptors go up, both directions are
 * matched, the result arrays are delivered by a kernel into page-locked memory.  Same matches as the three calls; the scratch slot's
 * descriptors and count are overwritten the same way. */
int lpslam_hip_match_bf_descriptors(lpslam_hip_ctx* ctx, int query, int scratch, const uint8_t* train_desc32, int32_t n_train,
                                    int32_t max_dist, float ratio, int32_t cross_check, int32_t* out_q, int32_t* out_t,
                                    int32_t* out_d, int32_t capacity, int32_t* count);
/* Descriptor sets kept on the device under a caller's key -- a tracker's keyframes -- and the comparison of an image slot with MANY
 * of them in one call: one launch matches the slot against every listed set, both directions, one kernel delivers all result arrays,
 * the caller waits once.  out_q / out_t / out_d hold capacity_per_key entries per key (key k's matches start at k * capacity_per_key),
 * counts[k] their number; per key the matches are those of lpslam_hip_match_bf_descriptors against that set.  A loop-candidate search
 * over 48 old keyframes is 48 uploads and 48 waits otherwise.  put replaces an existing key; unknown keys in a match are an error. */
int lpslam_hip_desc_store_put(lpslam_hip_ctx* ctx, int32_t key, const uint8_t* desc32, int32_t n);
int lpslam_hip_desc_store_drop(lpslam_hip_ctx* ctx, int32_t key);
int lpslam_hip_match_bf_stored(lpslam_hip_ctx* ctx, int query, const int32_t* keys, int32_t n_keys, int32_t max_dist, float ratio,
                               int32_t cross_check, int32_t* out_q, int32_t* out_t, int32_t* out_d, int32_t capacity_per_key,
                               int32_t* counts);
/* Per-keypoint mask of a stored set (n must equal the set's count; a set without a mask counts every keypoint).  A put clears it. */
int lpslam_hip_desc_store_mask(lpslam_hip_ctx* ctx, int32_t key, const uint8_t* mask, int32_t n);
/* Ranks stored sets by their votes for image slot `query`; keys == NULL ranks every stored set.  votes(k) = the number of matches
 * lpslam_hip_match_bf_stored(query, {k}, max_dist, ratio, cross_check = 1, ...) reports whose train keypoint t has mask_k[t] != 0.
 * Out: the top_k (1 .. 256) keys with votes >= 1, ordered by votes descending then key ascending, and their votes; *n_out of them.
 * An unknown or duplicate key, or top_k outside 1 .. 256: LPSLAM_HIP_ERR_INVALID.  One launch pair, one wait; only the top_k pairs
 * come back to the host. */
int lpslam_hip_rank_stored(lpslam_hip_ctx* ctx, int query, const int32_t* keys, int32_t n_keys, int32_t max_dist, float ratio,
                           int32_t top_k, int32_t* out_keys, int32_t* out_votes, int32_t* n_out);
/* Batched form: pairs (query0 + i*stride, train0 + i*stride), i in [0, n_pairs), in one launch. */
int lpslam_hip_match_bf_strided(lpslam_hip_ctx* ctx, int query0, int train0, int stride, int n_pairs);
/* Loads a caller-provided descriptor set (host memory, n x 32 bytes) into image slot `image`, replacing the
 * slot's extraction result: matching of descriptors that were produced elsewhere (map points, other frames). */
int lpslam_hip_set_descriptors(lpslam_hip_ctx* ctx, int image, const uint8_t* desc32, int32_t n);

/* Stereo: left slot vs right slot; row-band candidates, Hamming < 75, 11x11 SAD sub-pixel refinement,
 * 2 x median correlation cut.  focal_x_baseline as in LpSlamCameraConfiguration. */
int lpslam_hip_match_stereo(lpslam_hip_ctx* ctx, int left, int right, float focal_x_baseline, float true_baseline);
int lpslam_hip_match_stereo_strided(lpslam_hip_ctx* ctx, int left0, int right0, int stride, int n_pairs,
                                    float focal_x_baseline, float true_baseline);
int lpslam_hip_get_stereo(lpslam_hip_ctx* ctx, int left, float* stereo_x_right, float* depths,
                          int32_t* best_right_idx, int32_t capacity, int32_t* count);

/* ---- bundle adjustment (FP64) ------------------------------------------------------------------------------ */
typedef struct lpslam_hip_ba_obs {
    int32_t pose, point;
    double u, v, ur;          /* ur < 0: monocular edge (2 rows); else stereo (3 rows) */
    double inv_sigma2;        /* information = inv_sigma2 * I (1 / 1.2^(2*octave))      */
} lpslam_hip_ba_obs;

typedef struct lpslam_hip_ba_camera {
    double fx, fy, cx, cy, focal_x_baseline;
    double huber_mono, huber_stereo;   /* sqrt(5.991) / sqrt(7.815); <= 0: no robust kernel */
} lpslam_hip_ba_camera;

typedef struct lpslam_hip_ba_iter_log {
    double chi2_before, chi2_after, lambda;
    int32_t trials, status;            /* status 0 = OK, 1 = terminate */
} lpslam_hip_ba_iter_log;

typedef struct lpslam_hip_ba lpslam_hip_ba;

/* Builds the device-side problem (structure phase = g2o buildStructure): poses n x 7 (qw qx qy qz tx ty tz,
 * world->camera), fixed flags, points n x 3, observations.  One copy takes the inputs to HBM; the index structures (storage
 * order, CSR by landmark, pair lists of the Schur complement) are built there by kernels.  Asynchronous: returns once the work
 * is enqueued on the problem's stream. */
int lpslam_hip_ba_create(lpslam_hip_ctx* ctx, const double* poses, const uint8_t* fixed, int32_t n_poses,
                         const double* points, int32_t n_points, const lpslam_hip_ba_obs* obs, int32_t n_obs,
                         const lpslam_hip_ba_camera* cam, lpslam_hip_ba** out);
/* The same in two halves, for a host that serves many sessions.  lpslam_hip_ba_prepare is the HOST half -- validation, the window's
 * shape, the block carved out of the context's cache, the inputs copied into page-locked staging -- and enqueues nothing: every
 * session's mapping thread prepares its window on its own ([UPSTREAM] mapping_module::run of each session; reached through
 * feed_stereo_frame, src/Trackers/OpenVSLAMStereoTracker.cpp:293-295), thread safe per context.  lpslam_hip_ba_build_batch is the DEVICE
 * half for any number of prepared problems of one device: the structure kernels once for all of them (blockIdx.y = problem, ~16
 * launches whatever n is) on the first problem's stream; the others' streams wait for it on the device.  A prepared problem accepts
 * no other call before it has been built (LPSLAM_HIP_ERR_INVALID).  lpslam_hip_ba_create = prepare + build_batch of one. */
int lpslam_hip_ba_prepare(lpslam_hip_ctx* ctx, const double* poses, const uint8_t* fixed, int32_t n_poses,
                          const double* points, int32_t n_points, const lpslam_hip_ba_obs* obs, int32_t n_obs,
                          const lpslam_hip_ba_camera* cam, lpslam_hip_ba** out);
int lpslam_hip_ba_build_batch(lpslam_hip_ba* const* problems, int32_t n);
void lpslam_hip_ba_destroy(lpslam_hip_ba* ba);
/* Observation activity mask (0 = level 1 / ignored); NULL = all active. */
int lpslam_hip_ba_set_active(lpslam_hip_ba* ba, const uint8_t* active);
/* Levenberg-Marquardt with landmark Schur complement, `iters` outer iterations (g2o semantics: lambda_0 =
 * 1e-5 max diag H, rho-controlled lambda, <= 10 trials).  log may be NULL.  Returns iterations run in *done. */
int lpslam_hip_ba_optimize(lpslam_hip_ba* ba, int32_t robust, int32_t iters, lpslam_hip_ba_iter_log* log,
                           int32_t* done);
/* The same call in two halves.  begin enqueues the work on the problem's own stream and returns at once; end waits
 * for it, runs the extra trials rejected steps need and fetches the log.  Between the two the caller may enqueue
 * front-end work on the context: that is the reference's mapping thread running local BA beside tracking
 * ([UPSTREAM] mapping_module::run; lpslam only sees it through feed_stereo_frame,
 * src/Trackers/OpenVSLAMStereoTracker.cpp:293-295).  No other call on `ba` is allowed in between. */
int lpslam_hip_ba_optimize_begin(lpslam_hip_ba* ba, int32_t robust, int32_t iters);
int lpslam_hip_ba_optimize_end(lpslam_hip_ba* ba, lpslam_hip_ba_iter_log* log, int32_t* done);
/* How many solves of this context were started by replaying a captured launch graph (optimize_begin captures the launch chain
 * of a (stream, launch extents, robust, iters) signature the second time it sees it and replays it from then on, also for OTHER
 * problems with that signature on that stream).  Measurement / test hook; no reference counterpart. */
int64_t lpslam_hip_ba_graph_replays(lpslam_hip_ctx* ctx);
/* Totals over every bundle-adjustment problem this context has solved (the tracker's mapping thread makes a problem per keyframe and
 * destroys it: what happened to them is only visible here).  SIGNATURES: entries of the (stream, signature) cache, bounded at 256 and
 * never evicted -- a signature beyond the bound runs on direct launches; GRAPHS: graphs instantiated; REPLAYS: as
 * lpslam_hip_ba_graph_replays; TIMEOUTS_*: hand-overs between workgroups that timed out (lpslam_hip_ba_timeouts, summed -- any value
 * but 0 means a solve of this context failed).  Writes min(n, LPSLAM_HIP_BA_COUNTERS) values.  Measurement / test hook. */
enum { LPSLAM_HIP_BA_COUNTER_SIGNATURES = 0, LPSLAM_HIP_BA_COUNTER_GRAPHS = 1, LPSLAM_HIP_BA_COUNTER_REPLAYS = 2,
       LPSLAM_HIP_BA_COUNTER_TIMEOUTS_BAND = 3, LPSLAM_HIP_BA_COUNTER_TIMEOUTS_UPDATE = 4, LPSLAM_HIP_BA_COUNTERS = 5 };
int lpslam_hip_ba_counters(lpslam_hip_ctx* ctx, int64_t* out, int32_t n);
/* How many launches of the one-workgroup factorisation (k_chol_wg: batches of LPSLAM_HIP_CW_MIN_BATCH = 40 problems and more) this
 * context has enqueued.  Test hook: proves which of the two factorisations a batch went through.  No reference counterpart. */
int64_t lpslam_hip_ba_wg_factorisations(lpslam_hip_ctx* ctx);
/* Test hook like lpslam_hip_debug_occupy_unreserved (no reference counterpart, no product path calls it): the factor-and-solve of a
 * window on the caller's systems.  `problems`: n built problems on one device; their observations do not matter, they fix
 * dim_i = 6 x free keyframes and the solver.  A[i]: dim_i x dim_i matrix, row major; it stands for S + lambda I and nothing is added to
 * it.  b[i]: dim_i values.  Each reduced buffer is written as the product leaves it in front of a solve and the batch takes the
 * launches an optimize of these n problems takes.
 *   Problems with the dense solver: A[i] full symmetric; alone: the panel-pair chain; 40 problems and more: k_chol_wg for the systems
 *   that fit it, the chain for the others.
 *   Problems on the band solver (lpslam_hip_ba_get_solver: BAND, block half-bandwidth hbw): k_chol_band, launched as a solve launches
 *   it, on what the fused reduction leaves in front of it.  A[i] must be zero below the diagonal further than 6 hbw + 5 from it
 *   (LPSLAM_HIP_ERR_INVALID otherwise: the kernel reads 79 columns left of the diagonal whatever hbw says).  Only the lower triangle is
 *   read; the strict upper triangle is copied as given and may hold anything.  The two hand-over words of the twisted factorisation
 *   (systems of 12 strips of 16 and more) are cleared in front of the launch and must be zero again behind it:
 *   LPSLAM_HIP_ERR_DEVICE otherwise.
 *   A batch may mix the two kinds: both launch families run and each kernel skips the other's problems.
 * x[i] receives dim_i values, pivot_flag[i] (may be NULL) 1 where the factorisation met a pivot <= 0; x[i] is the zero step then, on
 * every kernel (what the replaced pivot left in the factor need not be finite, and none of it reaches x_p).  Finite inputs only (the
 * band kernel's unread upper triangle excepted).
 * The call overwrites the problems' reduced systems and control blocks: lpslam_hip_ba_reset (or reset_batch) each of them before it
 * optimises again. */
int lpslam_hip_ba_debug_solve(lpslam_hip_ba* const* problems, int32_t n, const double* const* A, const double* const* b,
                              double* const* x, int32_t* pivot_flag);
/* Which linear solver a problem takes.  DENSE: Schur complement by pair lists, dense panel-pair Cholesky (any window).  BAND: when
 * no landmark of the window spans more than 10 free keyframes the reduced system is block-banded -- the shape a tracker's windows have,
 * and why the reference's local bundle adjuster solves with g2o's LinearSolverCSparse (SURVEY.md a21;
 * conan-packages/g2o-conan/conanfile.py:117-124) -- and the problem takes the landmark-group Schur complement on the FP64 matrix
 * cores and a band Cholesky in one workgroup (chosen at creation; LPSLAM_HIP_BA_SOLVER=dense in the environment keeps every problem
 * dense).  get_solver reports the solver in use and the block half-bandwidth found at creation (-1: not banded); set_solver
 * switches (BAND on a window that is not banded: LPSLAM_HIP_ERR_INVALID).  Both give the same optimum; their sums differ in order
 * (chi2 agrees to ~1e-12 relative).  The partitioned solve always works on the dense buffer. */
#define LPSLAM_HIP_BA_SOLVER_AUTO 0
#define LPSLAM_HIP_BA_SOLVER_DENSE 1
#define LPSLAM_HIP_BA_SOLVER_BAND 2
int lpslam_hip_ba_get_solver(lpslam_hip_ba* ba, int32_t* solver, int32_t* block_half_bandwidth);
/* The dense path's Schur kernel cuts a window's long pose-block pair lists into parts of `part` terms, one workgroup each.  The
 * build chooses `part` per window: the smallest of 128, 160, 192, 224 whose workgroups still run as one generation on the device
 * (`capacity`: the further parts there is room for), else 256.  `part` depends on the window's own lists and on the device
 * alone: built alone or in a batch, a window gets the same one.  Waits for the problem's stream.  Either pointer may be NULL. */
int lpslam_hip_ba_get_schur_part(lpslam_hip_ba* ba, int32_t* part, int32_t* capacity);
/* Hand-overs between workgroups that timed out on this problem so far: `band` -- the two chains of the twisted band factorisation
 * (k_chol_band), `update` -- the keyframe blocks of the one-launch update waiting for the trial landmarks (k_ba_update).  Both waits
 * are bounded so that a grid always drains; a time-out makes the optimize call that meets it fail with LPSLAM_HIP_ERR_DEVICE (its
 * result is not valid) and is counted here.  Expected: 0, always (asserted by the batch tests).  No reference counterpart. */
int lpslam_hip_ba_timeouts(lpslam_hip_ba* ba, int32_t* band, int32_t* update);
int lpslam_hip_ba_set_solver(lpslam_hip_ba* ba, int32_t solver);
/* Batched solve -- north star: "a batched Levenberg-Marquardt local-BA".  n independent problems (the keyframe windows of
 * several SLAM sessions served by one GPU, [UPSTREAM] mapping_module::run of each session; lpslam reaches it through
 * feed_stereo_frame, src/Trackers/OpenVSLAMStereoTracker.cpp:293-295) are advanced by ONE launch chain: every kernel runs once
 * for the whole batch (blockIdx.y = problem) and each problem follows its own lambda control.  Results are identical to n calls of
 * lpslam_hip_ba_optimize for batches of fewer than 40 problems; from 40 on the reduced systems of local windows are factored by one
 * workgroup each (another summation order: equal within rounding, chi2 to 1e-12 relative).  All problems must live on one device; logs (may be NULL) receives log_stride entries per problem,
 * done (may be NULL) the iterations each problem ran.  reset_batch = lpslam_hip_ba_reset of every problem in one launch. */
int lpslam_hip_ba_optimize_batch(lpslam_hip_ba* const* problems, int32_t n, int32_t robust, int32_t iters,
                                 lpslam_hip_ba_iter_log* logs, int32_t log_stride, int32_t* done);
int lpslam_hip_ba_reset_batch(lpslam_hip_ba* const* problems, int32_t n);
/* lpslam_hip_ba_set_state / lpslam_hip_ba_get for every problem of a batch in one call (poses[i] / points[i] may be NULL as in the
 * single calls): the per-problem kernels are all enqueued before the first wait, and a server that runs its sessions' windows from a
 * scripting language crosses the boundary once per round instead of once per window. */
int lpslam_hip_ba_set_state_batch(lpslam_hip_ba* const* problems, int32_t n, const double* const* poses, const double* const* points);
int lpslam_hip_ba_get_batch(lpslam_hip_ba* const* problems, int32_t n, double* const* poses, double* const* points);
/* lpslam_hip_ba_optimize with a HIP event after every launch of the chain, on the problem's stream: time per kernel, summed over
 * the call (measurement hook of bench.py, like lpslam_hip_timer_*; no reference counterpart). */
#define LPSLAM_HIP_BA_KERNELS 8
#define LPSLAM_HIP_BA_K_LIN 0         /* k_ba_lin       (first unit of a call only; later linearisations ride in k_ba_trial) */
#define LPSLAM_HIP_BA_K_POINT_SUM 1   /* k_ba_point_sum */
#define LPSLAM_HIP_BA_K_SCHUR 2       /* k_ba_schur     */
#define LPSLAM_HIP_BA_K_CHOL 3        /* the factorisation: k_chol_pair x ceil(panels / 2), or k_chol_wg (one launch) */
#define LPSLAM_HIP_BA_K_XSOLVE 4      /* k_chol_xsolve  */
#define LPSLAM_HIP_BA_K_BACKSUB 5     /* k_ba_backsub   */
#define LPSLAM_HIP_BA_K_TRIAL 6       /* k_ba_trial     */
#define LPSLAM_HIP_BA_K_BAND_REDUCE 7 /* k_schur_band_reduce (band path only; there K_SCHUR is k_schur_group and K_CHOL is k_chol_band, one launch) */
typedef struct lpslam_hip_ba_kernel_times {
    float ms[LPSLAM_HIP_BA_KERNELS];                  /* summed over the call                                    */
    int32_t launches[LPSLAM_HIP_BA_KERNELS];          /* marks (= LM trials the kernel ran in)                   */
    int32_t launches_per_mark[LPSLAM_HIP_BA_KERNELS]; /* kernel launches behind one mark (factorisation: several) */
    int32_t iterations, dim;
} lpslam_hip_ba_kernel_times;
int lpslam_hip_ba_optimize_profiled(lpslam_hip_ba* ba, int32_t robust, int32_t iters, lpslam_hip_ba_kernel_times* out);
/* Motion-only mode: landmarks are held fixed (unary edges), only the free poses move. */
int lpslam_hip_ba_set_points_fixed(lpslam_hip_ba* ba, int32_t points_fixed);
/* optimize::pose_optimizer flow on a problem created with ONE free pose: 4 rounds x 10 iterations, outliers
 * (chi2 > 5.991 mono / 7.815 stereo) re-classified after every round, Huber dropped after the third round.
 * outlier may be NULL; *n_inliers receives the number of inlier observations. */
int lpslam_hip_ba_pose_optimize(lpslam_hip_ba* ba, uint8_t* outlier, int32_t* n_inliers);
/* The same flow for the tracker's per-frame call, without a problem object: one launch, one workgroup, the whole 4 x 10
 * iteration flow on the device (pose7 in / out; obs[k].point indexes `points`, obs[k].pose is ignored). */
int lpslam_hip_pose_optimize(lpslam_hip_ctx* ctx, double* pose7, const double* points, int32_t n_points, const lpslam_hip_ba_obs* obs,
                             int32_t n_obs, const lpslam_hip_ba_camera* cam, uint8_t* outlier, int32_t* n_inliers);
/* Diagnostic: passes over the observations the last lpslam_hip_pose_optimize on this context made (one per round + one per
 * Levenberg trial; the call's duration is this number times the latency of a trial). */
int32_t lpslam_hip_pose_optimize_passes(lpslam_hip_ctx* ctx);
/* ---- The covariance of poses the motion-only optimiser returned ---------------------------------------
 * Set i owns observations [set_start[i], set_start[i+1]) of `obs` (7 doubles each: u v ur inv_sigma2 X Y Z, ur < 0 = monocular) and of
 * `active` (1 = use: the optimiser's !outlier), and the pose pose7 + 7 i (qw qx qy qz tx ty tz, world -> camera); cam = fx fy cx cy fxb.
 * Per set: info21 = the upper triangle (row by row) of H = sum w B^T B over the active observations in front of the camera, B the pose
 * Jacobian of the optimiser (rotation first), w = inv_sigma2, no Huber; chi2 = sum w |e|^2; n_used = their number; cov21 = H^-1 in the
 * tangent space of T <- exp(d) T, through the Cholesky factor of D H D, D = diag(H)^-1/2; min_pivot = the smallest pivot of that
 * factorisation; status 0 = a covariance, 1 = fewer than 3 observations used, 2 = refused (a diagonal entry of H not positive or not
 * finite, or a pivot at or below 1e-8) -- on 1 and 2 cov21 is 21 zeros; min_pivot is 0 where the diagonal let no factorisation begin.
 * The arithmetic and the order of every sum are lpslam_amd/csrc/pose_cov_math.h; the results are those of
 * lpslam_pose_covariance_batch_host (liblpslam.so) bit for bit.  lpslam_pose_sigmas_host there turns cov21 into the interface's sigmas.
 * One upload, one launch (one workgroup per set), one wait.
 * A NULL argument, n_sets < 1, a set_start that starts below 0 or does not ascend: LPSLAM_HIP_ERR_INVALID; n_sets above
 * LPSLAM_HIP_POSE_COV_MAX_SETS or more than LPSLAM_HIP_POSE_COV_MAX_OBS observations in all: LPSLAM_HIP_ERR_CAPACITY.  Nothing is
 * allocated or written then. */
#define LPSLAM_HIP_POSE_COV_MAX_SETS 4096
#define LPSLAM_HIP_POSE_COV_MAX_OBS (1 << 18)
int lpslam_hip_pose_covariance_batch(lpslam_hip_ctx* ctx, int32_t n_sets, const int32_t* set_start /* n_sets + 1 */, const double* pose7 /* 7 per set */,
                                     const double* obs /* 7 per observation */, const uint8_t* active /* per observation */, const double* cam /* 5 */,
                                     double* info21 /* 21 per set */, double* cov21 /* 21 per set */, double* chi2, double* min_pivot, int32_t* n_used,
                                     int32_t* status /* each per set */);
/* local_bundle_adjuster flow: first_iters robust, outlier classification, second_iters plain. */
int lpslam_hip_ba_local(lpslam_hip_ba* ba, int32_t first_iters, int32_t second_iters, uint8_t* outlier);
/* A keyframe's local bundle adjustment in ONE call ([UPSTREAM] mapping_module -> optimize::local_bundle_adjuster::optimize, started per
 * keyframe by the mapping thread of startup(), src/Trackers/OpenVSLAMTrackerBase.cpp:239): lpslam_hip_ba_create of the window,
 * lpslam_hip_ba_local, lpslam_hip_ba_get into `poses` / `points` (in: the window's state, out: the solved one), destroy.  When several
 * sessions' mapping threads call it at the same time (shared launches on), their windows are built and solved together. */
int lpslam_hip_ba_local_window(lpslam_hip_ctx* ctx, double* poses, const uint8_t* fixed, int32_t n_poses, double* points, int32_t n_points,
                               const lpslam_hip_ba_obs* obs, int32_t n_obs, const lpslam_hip_ba_camera* cam, int32_t first_iters,
                               int32_t second_iters, uint8_t* outlier);
/* Restores the poses / points / activity mask given at creation (kept in HBM) and clears the LM state. */
int lpslam_hip_ba_reset(lpslam_hip_ba* ba);
/* Replaces the creation-time poses (n_poses x 7) and / or landmarks (n_points x 3) of an existing problem (NULL keeps them) and
 * resets it: the observation graph and its device-built structure stay.  A mapping thread creates the next window while the
 * previous one is being solved (lpslam_hip_ba_create only enqueues) and hands it the state that solve produced
 * ([UPSTREAM] local_bundle_adjuster reads the map after the previous run has written it back). */
int lpslam_hip_ba_set_state(lpslam_hip_ba* ba, const double* poses, const double* points);
int lpslam_hip_ba_get(lpslam_hip_ba* ba, double* poses, double* points);
int lpslam_hip_ba_chi2(lpslam_hip_ba* ba, double* chi2, uint8_t* depth_positive);

/* Partitioned (multi-GPU) global BA: every rank holds a landmark partition (its observations) and all poses.  One LM
 * trial is three device phases with the caller's collectives in between (each phase ends synchronised):
 *   step_begin(robust, first=1)   linearise                -> all-reduce SUM reduced_buffer, MAX scalar_buffer[4]
 *   step_lambda0()                lambda_0 from the reduced diagonals (first trial of an optimisation only)
 *   step_begin(robust, first=0)   (linearise if the state changed) + partial Schur complement -> all-reduce SUM reduced_buffer
 *   step_solve()                  factor, solve, update, trial chi2  -> all-reduce SUM scalar_buffer[1..2]
 *   step_end()                    accept / reject (identical on every rank) */
int lpslam_hip_ba_reduced_buffer(lpslam_hip_ba* ba, void** dev_ptr, int64_t* n_doubles);
int lpslam_hip_ba_scalar_buffer(lpslam_hip_ba* ba, void** dev_ptr, int64_t* n_doubles);
int lpslam_hip_ba_step_begin(lpslam_hip_ba* ba, int32_t robust, int32_t first);
int lpslam_hip_ba_step_lambda0(lpslam_hip_ba* ba);
int lpslam_hip_ba_step_solve(lpslam_hip_ba* ba);
int lpslam_hip_ba_step_end(lpslam_hip_ba* ba, int32_t* accepted, int32_t* iteration_finished);
/* The same partitioned solve driven from C++ with RCCL (ncclAllReduce of the packed triangle of S + b per LM
 * trial, a 2-double all-reduce for the trial chi2): `nccl_comm` is this rank's ncclComm_t, created by the caller
 * (ncclCommInitRank / ncclCommInitAll), one rank per GPU.  All collectives are enqueued on the problem's own stream between the
 * kernels -- no host synchronisation inside a trial; the host looks at the control block once per call (once more per batch of
 * rejected trials).  RCCL is bound at run time (dlopen).  Every rank must call with the same robust / iters. */
int lpslam_hip_ba_optimize_partitioned(lpslam_hip_ba* ba, void* nccl_comm, int32_t robust, int32_t iters,
                                       lpslam_hip_ba_iter_log* log, int32_t* done);
/* The same driver over the caller's own collective (an MPI / shared-memory host, or a test that runs several ranks on one
 * device): `allreduce(user, buf, count, op, stream)` must enqueue an IN-PLACE all-reduce of `count` doubles at device address
 * `buf` on HIP stream `stream` (a hipStream_t), ordered after the work already on that stream, op = LPSLAM_HIP_REDUCE_SUM or
 * LPSLAM_HIP_REDUCE_MAX, and return 0 on success.  Every rank must produce bit-identical results (a fixed summation order):
 * the ranks take their accept / reject decisions separately from the reduced values.  lpslam_hip_ba_optimize_partitioned is
 * this call with ncclAllReduce behind the callback. */
#define LPSLAM_HIP_REDUCE_SUM 0
#define LPSLAM_HIP_REDUCE_MAX 2
typedef int (*lpslam_hip_allreduce_fn)(void* user, void* buf, size_t count, int32_t op, void* stream);
int lpslam_hip_ba_optimize_partitioned_with(lpslam_hip_ba* ba, lpslam_hip_allreduce_fn allreduce, void* user, int32_t robust,
                                            int32_t iters, lpslam_hip_ba_iter_log* log, int32_t* done);
/* Control state after the last optimize / step_end: finished outer iterations, g2o "Terminate", lambda, robust chi2. */
int lpslam_hip_ba_status(lpslam_hip_ba* ba, int32_t* outer_done, int32_t* stopped, double* lambda, double* chi2);

/* ---- bag-of-words vocabulary and match::bow_tree ------------------------------------------------------------------------------
 * [UPSTREAM] DBoW2 TemplatedVocabulary<ORB> (shinsumicco/DBoW2 @ e8cc74d: conan-packages/dbow2-conan/conanfile.py:30-31), which the
 * reference requires at start-up (src/Trackers/OpenVSLAMTrackerBase.cpp:224-227: "Vocab file ... not present" -> start fails;
 * handed to openvslam::system at :238), and [UPSTREAM] openvslam match::bow_tree, which the relocaliser and the loop detector
 * (toggled at :250-255) match keypoints with.
 * lpslam_hip_vocab_create takes the tree as DBoW2 stores it -- nodes 1 .. n_nodes in file order, each naming its parent (0 = the
 * root, which precedes every node), its 32-byte descriptor, its weight and whether it is a leaf (= a word; word ids count the
 * leaves in node order) -- and keeps it in HBM.  A node may have at most 65535 children (LPSLAM_HIP_ERR_CAPACITY otherwise): the tree
 * itself is counted, `k` is only what the file declares.  The file formats are read by the host mirror (lpslam_amd/host/bow.h).
 * lpslam_hip_bow_transform walks the descriptors of an image slot down the tree on the device (TemplatedVocabulary::transform with
 * a FeatureVector: at every level the child at the smallest Hamming distance, the first on ties): per keypoint the word id, the
 * word's weight and the id of the node `levels_up` levels above the leaves (0 = the root when the tree is not that deep).  The
 * result buffers must hold lpslam_hip_max_keypoints_per_image() entries.  _host: the same for descriptors in host memory. */
typedef struct lpslam_hip_vocab lpslam_hip_vocab;
int lpslam_hip_vocab_create(lpslam_hip_ctx* ctx, int32_t k, int32_t L, int32_t n_nodes, const int32_t* parent, const uint8_t* desc32,
                            const float* weight, const uint8_t* is_leaf, lpslam_hip_vocab** out);
void lpslam_hip_vocab_destroy(lpslam_hip_vocab* vocab);
int lpslam_hip_vocab_info(lpslam_hip_vocab* vocab, int32_t* k, int32_t* L, int32_t* n_nodes, int32_t* n_words);
int lpslam_hip_bow_transform(lpslam_hip_ctx* ctx, lpslam_hip_vocab* vocab, int image, int32_t levels_up, int32_t* word_id, float* word_weight,
                             int32_t* node_id, int32_t capacity, int32_t* count);
int lpslam_hip_bow_transform_host(lpslam_hip_ctx* ctx, lpslam_hip_vocab* vocab, const uint8_t* desc32, int32_t n, int32_t levels_up,
                                  int32_t* word_id, float* word_weight, int32_t* node_id);
/* match::bow_tree (match_frame_and_keyframe / match_keyframes): query k (descriptor + the node it falls under, q_node[k] < 0 =
 * not a query, e.g. a keypoint without a landmark) is compared with the targets under the same node.  Queries are served node by
 * node (ascending id) and in keypoint order inside a node; a target matched by an earlier query (or flagged in t_taken, may be
 * NULL) is invisible to later ones; the nearest free target wins (the first on ties), accepted when best <= hamming_thr and
 * best <= lowe_ratio * second (second = 256 when there is no other).  match_idx[k] = target index or -1.  The orientation check
 * of upstream is lpslam_hip_match_orientation_filter on the result. */
int lpslam_hip_match_bow_tree(lpslam_hip_ctx* ctx, const uint8_t* q_desc32, const int32_t* q_node, int32_t nq, const uint8_t* t_desc32,
                              const int32_t* t_node, int32_t nt, const uint8_t* t_taken, int32_t hamming_thr, float lowe_ratio,
                              int32_t* match_idx, int32_t* match_dist, int32_t* n_matches);
/* The same query set against n_sets target sets (a loop-candidate search: the new keyframe against up to eight keyframes,
 * [UPSTREAM] loop_detector -> match::bow_tree::match_keyframes per candidate) in ONE round trip to the device; set i's results in
 * match_idx[i][0 .. nq), match_dist[i] (match_dist or its entries may be NULL), n_matches[i]; t_taken (or its entries) may be NULL.
 * Results are those of n_sets calls of lpslam_hip_match_bow_tree. */
int lpslam_hip_match_bow_tree_multi(lpslam_hip_ctx* ctx, const uint8_t* q_desc32, const int32_t* q_node, int32_t nq, int32_t n_sets,
                                    const uint8_t* const* t_desc32, const int32_t* const* t_node, const int32_t* nt, const uint8_t* const* t_taken,
                                    int32_t hamming_thr, float lowe_ratio, int32_t* const* match_idx, int32_t* const* match_dist, int32_t* n_matches);

/* ---- projection matching ---------------------------------------------------------------------------------------------
 * [UPSTREAM] match::projection::match_frame_and_landmarks (local-map tracking) and match_current_and_last_frames (motion-model
 * tracking), which openvslam::system runs inside feed_stereo_frame / feed_monocular_frame
 * (reference call sites: src/Trackers/OpenVSLAMStereoTracker.cpp:293-295, src/Trackers/OpenVSLAMTracker.cpp:120).
 * Query k = predicted pixel position, predicted right-image x (< 0: none), search radius (margin x scale factor of the
 * predicted level) and level range (-1: open) + its 32-byte descriptor.  Queries are matched IN ORDER against the keypoints of
 * image slot `image`: a keypoint taken by an earlier query (or flagged in `taken`, may be NULL) is invisible to later ones;
 * best distance <= hamming_thr; Lowe ratio only between candidates of the same level.  use_stereo != 0 applies the right-image
 * check against the slot's last stereo match.  match_idx[k] = keypoint index or -1. */
typedef struct lpslam_hip_proj_query {
    float x, y, x_right, radius;
    int32_t min_level, max_level;
} lpslam_hip_proj_query;
int lpslam_hip_match_projection(lpslam_hip_ctx* ctx, int image, const lpslam_hip_proj_query* queries, const uint8_t* q_desc32, int32_t nq,
                                int32_t hamming_thr, float lowe_ratio, const uint8_t* taken, int32_t use_stereo,
                                int32_t* match_idx, int32_t* match_dist, int32_t* n_matches);
/* [UPSTREAM] match::fuse (mapping module: detect / replace duplication): for every landmark projected into a keyframe the best
 * keypoint inside the window whose reprojection error passes the chi-square gate of the keypoint's level (5.99146 / 7.81473 with
 * the right-image x, use_stereo != 0), Hamming distance <= hamming_thr (50).  No exclusivity: what happens to a keypoint that
 * already carries a landmark is the caller's rule. */
int lpslam_hip_match_fuse(lpslam_hip_ctx* ctx, int image, const lpslam_hip_proj_query* queries, const uint8_t* q_desc32, int32_t nq,
                          int32_t hamming_thr, int32_t use_stereo, int32_t* match_idx, int32_t* match_dist, int32_t* n_matches);
/* [UPSTREAM] match::area::match_in_consistent_area (monocular initialiser): queries = level-0 keypoints of frame 1 at the position
 * they were matched to before (radius = margin, levels 0..0), image = frame 2.  A keypoint already matched at an equal or
 * smaller distance is not a candidate; best <= hamming_thr and best < lowe_ratio x second; a better later query takes the
 * keypoint away from the earlier one (whose match_idx becomes -1). */
int lpslam_hip_match_area(lpslam_hip_ctx* ctx, int image, const lpslam_hip_proj_query* queries, const uint8_t* q_desc32, int32_t nq,
                          int32_t hamming_thr, float lowe_ratio, int32_t* match_idx, int32_t* match_dist, int32_t* n_matches);
/* Diagnostic: single-query rescans the last lpslam_hip_match_projection / _fuse / _area call on this context made (a query whose
 * short candidate list earlier queries had used up is scanned again against the current assignment; fuse never rescans). */
int32_t lpslam_hip_window_match_rescans(lpslam_hip_ctx* ctx);
/* match::angle_checker: drops the matches whose angle difference (query - keypoint, degrees) lies outside the three most
 * populated 30-degree bins.  Host-side (a few thousand matches). */
int lpslam_hip_match_orientation_filter(const float* angle_q, const float* angle_t, int32_t* match_idx, int32_t nq, int32_t* n_kept);

/* ---- new landmarks between keyframes ---------------------------------------------------------------------------------
 * [UPSTREAM] mapping_module::create_new_landmarks (match::robust::match_for_triangulation, then the two-view triangulation and its
 * checks), which openvslam::system's mapping thread runs for every keyframe with Mapping.baseline_dist_thr as the reference forwards
 * it (src/Trackers/OpenVSLAMTrackerBase.cpp:72,202).  Upstream is absent from the reference tree: the rule is this project's own,
 * lpslam_amd/csrc/triangulate_math.h holds it and DESIGN.md section 31 the reasons.
 * View 1 is the new keyframe c, whose keypoints, descriptors and last stereo match sit in image slot `image`; each set is a
 * neighbour keyframe n in host memory.  Poses are world -> camera, qw qx qy qz tx ty tz.  A keypoint with depth > 0 under a camera
 * with focal_x_baseline > 0 is a stereo keypoint (focal_x_baseline = 0: a monocular camera, the slot's stereo columns are not read).
 * Keypoint i of c takes part when group1[i] >= 0, keypoint j of n when group[j] >= 0; j is a candidate of i when the groups are equal,
 * the Hamming distance is <= 50, j lies at least 10 sqrt(scale[octave_j]) pixels from the epipole (only when neither is a stereo
 * keypoint and has_epipole != 0) and (l . (x_j, y_j, 1))^2 <= 3.84 scale[octave_j]^2 (l0^2 + l1^2) for l = F (x_i, y_i, 1), l0^2 + l1^2 > 0. */
typedef struct lpslam_hip_tri_camera {
    double fx, fy, cx, cy;
    double focal_x_baseline;      /* fx x the true baseline; 0: monocular */
    double scale_factor;          /* Feature.scale_factor: the distance-ratio check allows 1.5 x this */
} lpslam_hip_tri_camera;
typedef struct lpslam_hip_tri_keypoint {
    float x, y;
    int32_t octave;
    float x_right, depth;         /* depth <= 0: not a stereo keypoint */
} lpslam_hip_tri_keypoint;
typedef struct lpslam_hip_tri_set {
    const lpslam_hip_keypoint* kpts;
    const uint8_t* desc32;
    const int32_t* group;
    const float* x_right;         /* x_right and depth: both NULL = no stereo keypoints */
    const float* depth;
    int32_t n;
    double pose[7];
    double F[9];                  /* row major, pixels: x_n^T F x_c = 0 */
    double epipole[2];            /* c's centre projected into n */
    int32_t has_epipole;          /* 0: that centre has z = 0 in n's frame */
} lpslam_hip_tri_set;
/* Per (set s, query i < *n_queries = the slot's keypoint count) at row s * capacity + i: the eight nearest candidates by (distance,
 * index) -- out_j (-1: none), out_dist (256), out_code (0: no landmark, 1: triangulated, 2 / 3: back-projection of i / of j), out_X
 * (3 doubles, NaN with code 0) -- and out_count, how many candidates passed (it may exceed eight: there is no rescan).  One upload, two
 * launches and one wait.  n_sets > 32, a set above lpslam_hip_max_keypoints_per_image(), capacity below the slot's count or an image
 * slot out of range: LPSLAM_HIP_ERR_CAPACITY; a null argument, an octave outside [0, n_levels), a value that is no number or a slot
 * that has never held an extraction: LPSLAM_HIP_ERR_INVALID.  On a session context the call runs directly (no shared launch). */
int lpslam_hip_triangulate_neighbours(lpslam_hip_ctx* ctx, int image, const int32_t* group1, const double* pose1, const lpslam_hip_tri_camera* cam,
                                      const lpslam_hip_tri_set* sets, int32_t n_sets, const float* scale, int32_t n_levels, int32_t capacity,
                                      int32_t* n_queries, int32_t* out_j, int32_t* out_dist, int32_t* out_code, double* out_X, int32_t* out_count);
/* The same tri_pair on n caller-given pairs (kp1[k] in view pose1, kp2[k] in view pose2): code[k], X[3 k ..] (NaN with code 0).
 * The parity hook of the kernel's arithmetic.  Synchronising. */
int lpslam_hip_triangulate_pairs(lpslam_hip_ctx* ctx, const lpslam_hip_tri_camera* cam, const float* scale, int32_t n_levels, const double* pose1, const double* pose2,
                                 const lpslam_hip_tri_keypoint* kp1, const lpslam_hip_tri_keypoint* kp2, int32_t n, int32_t* code, double* X);

/* ---- PnP RANSAC for a batch of match sets (relocalisation) ---------------------------------------------------------
 * Replaces the loop of LpSlam::pnp_solve_ransac calls (lpslam_amd/host/two_view.h) the relocaliser makes, one per candidate keyframe:
 * [UPSTREAM] solve::pnp_solver -- the pose from landmark / keypoint matches alone, EPnP on 4-match samples inside a RANSAC, then EPnP
 * once more over the inliers of the best sample.  DESIGN.md section 34; the arithmetic is lpslam_amd/csrc/epnp_math.h.
 * Set s holds matches offsets[s] .. offsets[s + 1] of pw (3 doubles each, world), obs (2 doubles, pixels) and inv_sigma2 (1 / scale^2
 * of the keypoint's level); cam4 = fx fy cx cy; every set is sampled with the same seed (xorshift32 from seed ? seed : 1) and
 * `iterations` samples.  Per set: pose7 = qw qx qy qz tx ty tz (world -> camera), n_inliers, the per-match flags in `inlier`
 * (indexed like the matches) and, where best_iteration is not NULL, the winning sample (-1: none).  A set with fewer than four matches,
 * one whose every sample fails (coplanar landmarks) and one whose best sample explains fewer than four matches answer n_inliers 0,
 * flags cleared, best_iteration -1 and the identity pose.  The results are those of pnp_solve_ransac on each set.  One upload, two
 * launches, one wait; the refit calls LpSlam::epnp_solve of liblpslam.so, which must lie beside this library (or be in the process).
 * n_sets == 0: LPSLAM_HIP_OK, nothing done.  n_sets < 0, offsets that start below 0 or do not ascend, iterations outside
 * 1 .. LPSLAM_HIP_PNP_MAX_ITERATIONS, a camera that is no number or NULL where an array is needed (best_iteration alone may be NULL):
 * LPSLAM_HIP_ERR_INVALID with nothing written. */
#define LPSLAM_HIP_PNP_MAX_ITERATIONS 1024
int lpslam_hip_pnp_ransac_batch(lpslam_hip_ctx* ctx, int32_t n_sets, const int32_t* offsets /* n_sets + 1 */, const double* pw, const double* obs,
                                const double* inv_sigma2, const double* cam4, int32_t iterations, uint32_t seed,
                                double* pose7 /* 7 per set */, int32_t* n_inliers /* per set */, uint8_t* inlier /* per match */,
                                int32_t* best_iteration /* per set, may be NULL */);

/* ---- Two-view initialisation: the RANSAC loop and the pose check (monocular) -----------------------------------------
 * Steps 1 and 4 of LpSlam::two_view_initialize (lpslam_amd/host/two_view.h), what openvslam::system does inside
 * feed_monocular_frame until a map exists (reference call site: src/Trackers/OpenVSLAMTracker.cpp:120; parameters
 * src/Trackers/OpenVSLAMTrackerBase.cpp:161-201): [UPSTREAM] initialize::perspective -- solve::homography_solver and
 * solve::fundamental_solver on 8-match samples of Hartley-normalised keypoints, initialize::base::check_triangulated_pts.
 * DESIGN.md section 38; the arithmetic is lpslam_amd/csrc/two_view_math.h, the text the host function runs: the same bits.
 *
 * lpslam_hip_two_view_ransac_batch: set s holds matches offsets[s] .. offsets[s + 1] of p1 (reference image) and p2 (current image),
 * two doubles (pixels) each; every set is sampled with the same seed (xorshift32 from seed ? seed : 1) and `iterations` samples of
 * eight, each giving a homography and a fundamental matrix that are scored over all matches of the set (chi-square at `sigma`, the
 * sum over the matches in index order).  Per set and model (0 = H, 1 = F): best_iteration[2 s + m] (the first sample with the largest
 * score; -1: none), score[2 s + m], model[18 s + 9 m ..] (H21 / F21, reference -> current, pixels, row major) and the per-match
 * inlier flags of the winner in inlier_h / inlier_f (indexed like the matches).  No refit.  A model answers none -- iteration -1,
 * score 0, a zero matrix, flags cleared -- when the set has fewer than eight matches or no sample gives a valid hypothesis (H: a
 * determinant that is not above 1e-300; either: a score that is no number, as with all matches on one point).  One upload, two
 * launches, one wait.  n_sets == 0: LPSLAM_HIP_OK, nothing done.  n_sets < 0, offsets that start below 0 or do not ascend,
 * iterations outside 1 .. LPSLAM_HIP_TWO_VIEW_MAX_ITERATIONS, a sigma that is no positive number or NULL where an array is needed:
 * LPSLAM_HIP_ERR_INVALID with nothing written.
 *
 * lpslam_hip_two_view_check_poses: n_hyp <= LPSLAM_HIP_TWO_VIEW_MAX_POSES motion hypotheses (R 9 doubles row major, t 3 doubles:
 * reference -> current), K4 = fx fy cx cy, the n matches, the chosen model's inlier flags and th2 (squared reprojection bound,
 * pixels).  Per (hypothesis h, match i) at h n + i: code (0: no inlier or rejected, 1: a plausible point, 2: plausible and with
 * enough parallax to become a landmark), X (3 doubles in the reference camera frame; NaN with code 0) and cosp (the cosine of its
 * parallax; 0 with code 0).  Counting, sorting the cosines and the acceptance rules stay with the caller.  One upload, one launch,
 * one wait.  n_hyp == 0 or n == 0: LPSLAM_HIP_OK, nothing done.  n_hyp outside 0 .. 8, n < 0 or NULL where an array is needed:
 * LPSLAM_HIP_ERR_INVALID with nothing written. */
#define LPSLAM_HIP_TWO_VIEW_MAX_ITERATIONS 1024
#define LPSLAM_HIP_TWO_VIEW_MAX_POSES 8
int lpslam_hip_two_view_ransac_batch(lpslam_hip_ctx* ctx, int32_t n_sets, const int32_t* offsets /* n_sets + 1 */, const double* p1, const double* p2,
                                     double sigma, int32_t iterations, uint32_t seed, int32_t* best_iteration /* 2 per set */, double* score /* 2 per set */,
                                     double* model /* 18 per set */, uint8_t* inlier_h /* per match */, uint8_t* inlier_f /* per match */);
int lpslam_hip_two_view_check_poses(lpslam_hip_ctx* ctx, int32_t n_hyp, const double* R /* 9 per hypothesis */, const double* t /* 3 per hypothesis */,
                                    const double* K4, int32_t n, const double* p1, const double* p2, const uint8_t* inlier /* per match */, double th2,
                                    double* X /* 3 per (hypothesis, match) */, double* cosp, uint8_t* code);

/* ---- Sim3 pose graph ---------------------------------------------------------------------------------------------
 * Replaces what openvslam::system runs on its global-optimisation thread after a loop closure while the loop detector
 * is enabled (reference: src/Trackers/OpenVSLAMTrackerBase.cpp:250-255): [UPSTREAM] optimize::graph_optimizer on
 * g2o@691dc51 types_sim3 (VertexSim3Expmap / EdgeSim3, numeric Jacobians, Levenberg, BlockSolver_7_3); SURVEY.md 8(a) a23.
 * A Sim3 is 8 doubles qw qx qy qz tx ty tz s (world -> camera: x_c = s R x_w + t). */
typedef struct lpslam_hip_sim3_edge {
    int32_t i, j;          /* vertices: error = log(meas * S_i * S_j^-1), information = identity */
    double meas[8];
} lpslam_hip_sim3_edge;

typedef struct lpslam_hip_sim3 lpslam_hip_sim3;

/* verts n x 8, fixed flags (NULL = none fixed; the loop keyframe should be), edges; fix_scale != 0 zeroes the scale
 * component of every update (stereo / RGBD).  Copies everything to HBM. */
int lpslam_hip_sim3_create(lpslam_hip_ctx* ctx, const double* verts, const uint8_t* fixed, int32_t n,
                           const lpslam_hip_sim3_edge* edges, int32_t n_edges, int32_t fix_scale, lpslam_hip_sim3** out);
void lpslam_hip_sim3_destroy(lpslam_hip_sim3* graph);
/* `iters` outer Levenberg iterations (graph_optimizer: 50), g2o lambda control; log may be NULL. */
int lpslam_hip_sim3_optimize(lpslam_hip_sim3* graph, int32_t iters, lpslam_hip_ba_iter_log* log, int32_t* done);
int lpslam_hip_sim3_get(lpslam_hip_sim3* graph, double* verts);
/* chi2 (= |error|^2) per edge of the current estimate */
int lpslam_hip_sim3_chi2(lpslam_hip_sim3* graph, double* chi2);

/* Sim3 between two keyframes ([UPSTREAM] optimize::transform_optimizer, called by the loop detector for every loop candidate):
 * matched landmark pairs k = landmark 1 in camera-1 coordinates, landmark 2 in camera-2 coordinates, both keypoints and
 * 1 / sigma^2 of their pyramid levels.  A batch of candidates is solved in one launch (one workgroup each): problem i owns
 * pairs [pair_start[i], pair_start[i+1]) and s12[8 i .. 8 i + 7] (Sim3 camera 2 -> camera 1, in / out).  Flow per problem:
 * 5 Levenberg iterations (Huber sqrt(chi_sq)), pairs with chi2 > chi_sq on either edge dropped, 10 more iterations if any was
 * dropped (else 5); n_inliers[i] = 0 when fewer than 10 pairs survive the first cut.  cam = fx fy cx cy.  inlier may be NULL. */
typedef struct lpslam_hip_sim3_pair {
    double p1c[3], p2c[3];
    double obs1[2], obs2[2];
    double inv_sigma2_1, inv_sigma2_2;
} lpslam_hip_sim3_pair;
int lpslam_hip_sim3_transform_optimize(lpslam_hip_ctx* ctx, int32_t n_problems, double* s12, const lpslam_hip_sim3_pair* pairs,
                                       const int32_t* pair_start, const double* cam1, const double* cam2, double chi_sq,
                                       int32_t fix_scale, uint8_t* inlier, int32_t* n_inliers);

/* ---- Sim3 RANSAC and loop verification for a batch of candidates (loop closing) ---------------------------------------
 * Replaces the loop of LpSlam::sim3_solve_ransac calls (lpslam_amd/host/two_view.h) the loop closer makes, one per candidate keyframe,
 * and the transform-optimiser call behind them: [UPSTREAM] solve::sim3_solver -- the similarity camera 2 -> camera 1 from matched
 * landmark pairs alone, Horn's absolute orientation on 3-pair samples inside a RANSAC over the reprojection error in both images
 * (chi-square 9.210 at the keypoints' levels).  DESIGN.md section 41; the arithmetic is lpslam_amd/csrc/sim3_math.h and horn of
 * lpslam_amd/csrc/epnp_math.h, the text the host solver runs: the same bits.
 * Set i owns pairs [pair_start[i], pair_start[i+1]), the input format of lpslam_hip_sim3_transform_optimize; cam = fx fy cx cy;
 * fix_scale != 0 holds the scale at 1 (stereo / RGBD); every set is sampled with the same seed (xorshift32 from seed ? seed : 1) and
 * `iterations` samples.
 *
 * lpslam_hip_sim3_ransac_batch: per set s12 = qw qx qy qz tx ty tz s of the first sample with the largest count, n_inliers (that
 * count), the per-pair flags in `inlier` (indexed like the pairs) and, where best_iteration is not NULL, the winning sample (-1: none).
 * A set with fewer than three pairs, one whose every sample is refused (coincident points under a free scale) and one whose samples
 * explain no pair answer n_inliers 0, flags cleared, best_iteration -1 and s12 = 1 0 0 0 0 0 0 1.  No refit.  The results are those of
 * lpslam_sim3_ransac_batch_host (liblpslam.so), sim3_solve_ransac on each set.  One upload, two launches, one wait.
 *
 * lpslam_hip_sim3_verify_batch: the same RANSAC, then for every set whose count reaches min_seed_inliers the flow of
 * lpslam_hip_sim3_transform_optimize from that seed at chi_sq, all on the device.  Per set seed_inliers (the RANSAC's count), s12 (the
 * optimised similarity), n_inliers (the optimiser's: 0 when fewer than 10 pairs survive its first cut) and, where `inlier` is not NULL,
 * the optimiser's per-pair flags.  A set below the gate answers n_inliers 0, flags cleared and the RANSAC's seed in s12.  Per set the
 * results are those of the host solver followed by lpslam_hip_sim3_transform_optimize.  One upload, three launches, one wait.
 *
 * n_sets == 0: LPSLAM_HIP_OK, nothing done.  n_sets < 0, a pair_start that starts below 0 or does not ascend, iterations outside
 * 1 .. LPSLAM_HIP_SIM3_RANSAC_MAX_ITERATIONS, a camera that is no number, a chi_sq that is no positive number, min_seed_inliers < 0 or
 * NULL where an array is needed (best_iteration and the verify call's inlier alone may be NULL): LPSLAM_HIP_ERR_INVALID with nothing
 * written. */
#define LPSLAM_HIP_SIM3_RANSAC_MAX_ITERATIONS 1024
int lpslam_hip_sim3_ransac_batch(lpslam_hip_ctx* ctx, int32_t n_sets, const lpslam_hip_sim3_pair* pairs, const int32_t* pair_start /* n_sets + 1 */,
                                 const double* cam1, const double* cam2, int32_t fix_scale, int32_t iterations, uint32_t seed,
                                 double* s12 /* 8 per set */, int32_t* n_inliers /* per set */, uint8_t* inlier /* per pair */,
                                 int32_t* best_iteration /* per set, may be NULL */);
int lpslam_hip_sim3_verify_batch(lpslam_hip_ctx* ctx, int32_t n_sets, const lpslam_hip_sim3_pair* pairs, const int32_t* pair_start /* n_sets + 1 */,
                                 const double* cam1, const double* cam2, int32_t fix_scale, int32_t iterations, uint32_t seed,
                                 int32_t min_seed_inliers, double chi_sq, int32_t* seed_inliers /* per set */, double* s12 /* 8 per set, optimised */,
                                 int32_t* n_inliers /* per set */, uint8_t* inlier /* per pair, may be NULL */);

/* ---- 2-D occupancy grid from laser scans (the reference's map_publisher occupancy_map_export, reached through
 * src/Trackers/OpenVSLAMStereoTracker.cpp:374-400; the grid itself is defined in INTEGRATION.md, "Occupancy grid") ----------
 * Beam directions are uploaded once per scan geometry (cos a, sin a per beam, computed by the caller in double); the ranges of each
 * scan stay on the device under a caller's key (a tracker's keyframes); a build takes one map-plane pose per key and returns the
 * int8 grid (-1 unknown, 0 .. 100 occupied).  All calls of a context that touch the store or build are serialised on the context and
 * run on a stream of their own: a build may come from any thread while the context tracks. */
typedef struct lpslam_hip_scan_pose {
    int32_t key;
    int32_t pad;
    double origin[2];   /* laser position, (world lpslam y, z) */
    double fwd[2];      /* (y, z) of R_world_laser * (0, 0, 1)  */
    double left[2];     /* (y, z) of R_world_laser * (0, -1, 0) */
} lpslam_hip_scan_pose;
typedef struct lpslam_hip_grid_info {
    int64_t x0, y0;              /* global cell of grid cell (0, 0) */
    int32_t width, height;       /* cells; 0 x 0 when no beam counted */
    int64_t rays;                /* beams that were not skipped */
    int64_t cell_visits;         /* hit + miss increments inside the box */
} lpslam_hip_grid_info;
/* A table of n_beams (cos, sin) pairs; *id names it in scan_store_put. */
int lpslam_hip_scan_geometry_put(lpslam_hip_ctx* ctx, const double* cos_sin, int32_t n_beams, int32_t* id);
/* n must equal the geometry's beam count.  put replaces an existing key. */
int lpslam_hip_scan_store_put(lpslam_hip_ctx* ctx, int32_t key, int32_t geometry_id, const float* ranges, int32_t n, float range_min,
                              float range_max, float range_threshold);
int lpslam_hip_scan_store_drop(lpslam_hip_ctx* ctx, int32_t key);
/* The grid of the listed scans at the given poses; res > 0 metres per cell, max_side a positive multiple of 64.  out == NULL: sizing
 * only (info as the full build gives it).  An unknown key, or capacity < width * height with out != NULL: LPSLAM_HIP_ERR_INVALID and
 * nothing is written to out. */
int lpslam_hip_occupancy_build(lpslam_hip_ctx* ctx, const lpslam_hip_scan_pose* poses, int32_t n, double res, int32_t max_side,
                               int8_t* out, int64_t capacity, lpslam_hip_grid_info* info);

/* ---- baseline JPEG encoder (the recorder's cv::imencode(".jpg"), /root/reference/src/Manager/RecordEngine.cpp:93) ----------------
 * A standalone object (no lpslam_hip_ctx: the reference records without a tracker) with its own stream and buffers, sized at creation
 * for max_images images of at most max_width x max_height samples.  One encode call is one launch chain and one wait for the whole
 * batch (both eyes of a stereo frame).  The output of every image is byte for byte what the host encoder writes
 * (LpSlam::encode_jpeg_gray, lpslam_jpeg_encode_gray): one grey component, baseline, Annex K tables scaled for quality, libjpeg's islow
 * FDCT and rounding, no restart markers.  Calls on one encoder are serialised. */
typedef struct lpslam_hip_jpeg lpslam_hip_jpeg;
int lpslam_hip_jpeg_create(int32_t max_width, int32_t max_height, int32_t max_images, lpslam_hip_jpeg** out);
void lpslam_hip_jpeg_destroy(lpslam_hip_jpeg* enc);
/* n images (host samples, row stride in bytes) -> n complete JPEG files in outs[i] (capacity caps[i]).  sizes[i] is always set to the
 * exact length.  If any caps[i] is too small: LPSLAM_HIP_ERR_INVALID, and no output buffer is written.  n outside 1 .. max_images, an
 * image larger than the encoder's maximum, a stride below the width or a quality outside 1 .. 100: LPSLAM_HIP_ERR_INVALID. */
int lpslam_hip_jpeg_encode(lpslam_hip_jpeg* enc, int32_t n, const uint8_t* const* pixels, const int32_t* widths,
                           const int32_t* heights, const int32_t* strides, int32_t quality,
                           uint8_t* const* outs, const int64_t* caps, int64_t* sizes);

/* ---- baseline JPEG decoder: the other direction (replay of a recording, compressed frames handed in by a client) --------------------
 * A standalone object like the encoder (no lpslam_hip_ctx, its own stream and buffers), sized at creation for max_images streams of at
 * most max_width x max_height samples.  One decode call is one upload, one launch chain and one wait for the whole batch (both eyes
 * of a record).  The samples of a decoded image are bit for bit those of the host decoder (LpSlam::decode_jpeg_gray,
 * lpslam_jpeg_decode_gray), which are libjpeg's.  Calls on one decoder are serialised.  Every image gets a status: */
#define LPSLAM_HIP_JPEG_DECODED 0      /* the samples are in outs[i] */
#define LPSLAM_HIP_JPEG_NOT_TAKEN 1    /* a valid file of a class left to the host decoder: three components (see
                                          lpslam_hip_jpeg_dec_create2 for the decoder that takes them), a restart interval (see
                                          lpslam_hip_jpeg_dec_take_restart for the switch that takes those), a 16-bit quantisation table for the first component, larger than the decoder was made for, or more than
                                          4 bytes per sample (12 in a decoder made for colour) + 4096 from the start of the
                                          entropy-coded data to the end of the file (a trailer counts) */
#define LPSLAM_HIP_JPEG_IRREGULAR 2    /* the header does not parse, or the entropy-coded data does not end where the block count says
                                          it must, or (restart intervals) it does not hold ceil(MCUs / Ri) - 1 restart markers, each
                                          byte aligned behind exactly Ri whole MCUs -- fill bytes in front of a marker count as that:
                                          the host decoder gives the verdict */
typedef struct lpslam_hip_jpeg_dec lpslam_hip_jpeg_dec;
int lpslam_hip_jpeg_dec_create(int32_t max_width, int32_t max_height, int32_t max_images, lpslam_hip_jpeg_dec** out);
/* lpslam_hip_jpeg_dec_create is lpslam_hip_jpeg_dec_create2 with flags 0: such a decoder leaves every three-component stream NOT_TAKEN.
 * With LPSLAM_HIP_JPEG_DEC_COLOR the decoder also takes three-component (YCbCr) baseline streams and gives their first component, which
 * is what the host decoder and libjpeg's grey output give: one interleaved scan of all three components in frame order, the first
 * sampled 1 x 1, 2 x 1 or 2 x 2 (4:4:4, 4:2:2, 4:2:0) and the other two 1 x 1, no restart interval, an 8-bit quantisation table for
 * the first component.  Other three-component streams stay NOT_TAKEN.  Such a decoder is sized for 12 bytes of entropy-coded data per
 * sample and for planes of whole 16 x 16 MCUs (about three times the memory of a grey one).  Unknown flag bits:
 * LPSLAM_HIP_ERR_INVALID. */
#define LPSLAM_HIP_JPEG_DEC_COLOR 1u
int lpslam_hip_jpeg_dec_create2(int32_t max_width, int32_t max_height, int32_t max_images, uint32_t flags, lpslam_hip_jpeg_dec** out);
void lpslam_hip_jpeg_dec_destroy(lpslam_hip_jpeg_dec* dec);
/* Off at creation (lpslam_hip_jpeg_dec_create and _create2 alike): every stream whose header sets a restart interval is NOT_TAKEN.
 * on != 0: a stream that is otherwise of a class this decoder takes -- one component, or one interleaved Y/Cb/Cr scan on a decoder
 * made with LPSLAM_HIP_JPEG_DEC_COLOR -- and has a DRI segment is decoded on the device, RSTn markers in the entropy-coded data
 * included (Ri = 0, or Ri of the MCU count or more, means no marker: the path of a stream without DRI).  Non-interleaved and
 * multi-scan files and 16-bit tables for the first component stay NOT_TAKEN.  Holds for the calls that follow; serialised with them. */
int lpslam_hip_jpeg_dec_take_restart(lpslam_hip_jpeg_dec* dec, int32_t on);
/* n complete JPEG files (host memory) -> samples in outs[i], rows out_strides[i] bytes apart, capacity out_caps[i] bytes.  widths[i] /
 * heights[i] are always set from the frame header when there is one (0 otherwise).  If the samples of an image the device takes do
 * not fit its out_caps[i] (or out_strides[i] is below its width): LPSLAM_HIP_ERR_INVALID, the sizes are reported and no output buffer
 * is written.  n outside 1 .. max_images or a null argument: LPSLAM_HIP_ERR_INVALID.  Otherwise LPSLAM_HIP_OK and status[i] says what
 * became of every image; only the buffers of DECODED images are written. */
int lpslam_hip_jpeg_decode(lpslam_hip_jpeg_dec* dec, int32_t n, const uint8_t* const* streams, const int64_t* stream_sizes,
                           uint8_t* const* outs, const int32_t* out_strides, const int64_t* out_caps,
                           int32_t* widths, int32_t* heights, int32_t* status);
/* test hook: per image of the last decode call (n as there) the synchronisation rounds that changed a subsequence state, the
 * subsequences of its entropy-coded data, and the blocks they completed (of all components); zeros for an image the device did not
 * take. */
int lpslam_hip_jpeg_dec_last(lpslam_hip_jpeg_dec* dec, int32_t n, int32_t* rounds, int32_t* subsequences, int32_t* blocks);

#ifdef __cplusplus
}
#endif
#endif /* LPSLAM_HIP_H */
