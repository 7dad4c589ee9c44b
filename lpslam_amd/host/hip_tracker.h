// hip_tracker.h -- tracker plugins "VSLAMStereo" / "VSLAMMono" backed by the MI355X hot path.
//
// Drop-in for the reference's OpenVSLAM adapters (src/Trackers/OpenVSLAMTrackerBase.{h,cpp},
// src/Trackers/OpenVSLAMStereoTracker.{h,cpp}, src/Trackers/OpenVSLAMTracker.{h,cpp}): same type() strings, same JSON
// configuration keys (OpenVSLAMTrackerBase.cpp:31-50), same pose conventions on the way out (createTrackerResult,
// :307-329).  Where the reference holds an openvslam::system, this class holds a lpslam_hip_ctx: per frame it runs the
// HIP front end (ORB on both eyes, stereo match, brute-force match against the previous frame), a motion-only pose
// optimisation, and on keyframes a local bundle adjustment over a sliding window (include/lpslam_hip.h).
#pragma once
#include "core.h"
#include "bow.h"
#include "pose_math.h"
#include "map_file.h"
#include "../csrc/fisheye_math.h"
#include "../csrc/radtan_math.h"
#include "../csrc/triangulate_math.h"
#include "../../include/lpslam_hip.h"

#include <array>
#include <condition_variable>
#include <memory>
#include <thread>
#include <unordered_map>

namespace LpSlam {

enum class TrackerState { NotInitialized, Initializing, Tracking, Lost };     // openvslam::tracker_state_t

class HipVslamTrackerBase : public TrackerBase {
public:
    HipVslamTrackerBase();
    ~HipVslamTrackerBase() override;
    void OnConfigurationUpdate() override;
    bool stop() override;

    // what the manager down-casts for (src/Manager/SlamManager.cpp:1316-1366)
    bool mappingSetMode(bool enableMapping) { m_enableMapping = enableMapping; return true; }
    bool mappingSetFilename(std::string const& filename) { m_mapFilename = filename; m_mapFilenameSet = true; return true; }
    bool mappingExportCSV(std::string csv_filename);
    std::size_t mappingGetFeatures(LpSlamMapBoundary boundary, LpSlamFeatureEntry* entry, std::size_t entry_count, LpSlamMatrix9x9 transform);
    std::size_t mappingGetFeaturesCount(LpSlamMapBoundary boundary);
    std::string lastStatistics() { std::scoped_lock lock(m_slamLock); return m_lastStatistics; }      // "VSLAM statistics: key=value ..." of the last stop(), this tracker's own (the log is process-wide)
    LpSlamStatus getSlamStatus();

    TrackerState state() const { return m_state; }
    void addRequestNavTransformationCallback(RequestNavTransformationCallback_t cb, void* user) override { std::scoped_lock l(m_laserMutex); m_navTransform = cb; m_navTransformData = user; }
    std::array<double, 16> currentCamPose();          // T_cw, row-major 4x4 (get_current_cam_pose)

protected:
    using Pose = LpSlam::Pose;                        // world -> camera (pose_math.h)
    // laser scans (src/Trackers/OpenVSLAMStereoTracker.cpp:232-285,344-371): the latest scan waits in a one-slot buffer; a frame
    // whose ROS time is within maxLaserAge of it takes it along, with the laser's pose in the camera's lpslam frame
    struct LaserScan { std::vector<float> ranges; float range_min = 0, range_max = 0, angle_min = 0, increment = 0, range_threshold = 0; std::optional<LpSlamROSTimestamp> ros; };
    struct ScanAttach { std::shared_ptr<const LaserScan> scan; double R_cl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; double t_cl[3] = {0, 0, 0}; };
public:
    // test hook: the ROS time of every scan the grid is built from and the pose it is built at
    std::vector<std::pair<LpSlamROSTimestamp, lpslam_hip_scan_pose>> occupancyScans();
protected:
    struct FrameData {
        std::optional<ScanAttach> scan;               // the laser scan attached to this frame (stereo only)
        std::vector<lpslam_hip_keypoint> kpts;
        std::vector<uint8_t> desc;                    // 32 bytes per keypoint
        std::vector<float> x_right, depth;
        std::vector<int> landmark;                    // landmark id per keypoint or -1
        Pose pose;
        double sigma[4] = {0, 0, 0, 0};               // poseSigma: x y z (lpslam axes) and orientation sigma of `pose` where poseFromMatches found it, else 0
        int slot = 0;
    };
    // The map ([UPSTREAM] data::map_database): every keyframe ever inserted with its keypoints, descriptors, stereo columns and
    // the landmark of every keypoint; every landmark with the list of its observations.  Covisibility ([UPSTREAM]
    // data::graph_node: keyframes weighted by the landmarks they share) is computed from the observation lists when it is needed.
    struct Keyframe {
        Pose pose;
        std::vector<lpslam_hip_keypoint> kpts; std::vector<uint8_t> desc; std::vector<float> x_right, depth;
        std::vector<int> landmark;                    // per keypoint: landmark id or -1
        int segment = 0;                              // map segment: a re-initialisation after a loss opens a new one
        bool erased = false;                          // culled as redundant: holds no keypoints and no observations any more (the index stays)
        bool desc_on_device = false;                  // lpslam_hip_desc_store_put succeeded: the loop-candidate search may name it in a batched comparison
        BowVector bow;                                // with a vocabulary: the keyframe's BoW vector and, per keypoint, the tree node it falls under
        std::vector<int32_t> node;
        bool has_scan = false;                        // its scan is in the context's scan store under the keyframe index
        double R_cl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t_cl[3] = {0, 0, 0};      // laser pose in the camera's lpslam frame
        LpSlamROSTimestamp scan_ros{};
    };
    struct Landmark {
        double p[3]; 
        // what local-map tracking needs ([UPSTREAM] data::landmark): the descriptor, the viewing direction and the valid
        // distance range of the observation that created it (scale prediction: level = ceil(log(max_valid / d) / log s))
        uint8_t desc[32] = {0};
        double normal[3] = {0, 0, 1};
        double max_valid = 0, min_valid = 0;
        int ref_kf = -1;                              // the keyframe that created it (loop correction moves it with that keyframe)
        // [UPSTREAM] data::landmark num_observable_ / num_observed_ (both start at 1): how often tracking expected to see the landmark
        // and how often it did -- local_map_cleaner::remove_redundant_landmarks drops the ones seen less than 30 % of the time
        int n_observable = 1, n_observed = 1;
        std::vector<std::pair<int, int>> obs;         // (keyframe, keypoint) in insertion order
    };
    struct Statistics {                               // logged at stop() ("VSLAM statistics: ..."): what the tracker did, for logs and tests
        long frames = 0, motion_tracked = 0, bf_tracked = 0, local_map_joined = 0, keyframes = 0, fused_added = 0, fused_merged = 0;
        long culled_landmarks = 0, culled_keyframes = 0;
        long ba_failed = 0;                           // windows whose solve failed on the device (result dropped)
        long local_ba = 0, loops_closed = 0, loop_fused = 0, global_ba = 0, lost = 0, relocalised = 0, reinitialised = 0, nav_priors = 0, prefetched = 0;
        long color_converted = 0;                     // frames whose colour / YUV source was converted to grey on the device
        long pnp_batches = 0, reloc_frames = 0; double t_relocalise = 0;      // relocalisation: solver batches on the device (relocaliseOnDevice), Lost frames that tried, seconds they took
        long sim3_batches = 0, loop_tries = 0; double t_loop_try = 0;      // loop closing: verification batches on the device (verifyLoopsOnDevice), keyframes whose candidates were verified, seconds that took
        long pose_fits = 0, pose_sigmas = 0, pose_sigma_refused = 0; double t_dev_pose_sigma = 0;      // poseFromMatches calls that returned a pose; poseSigma: those whose covariance gave sigmas, those refused (status 1, 2 or a failed call), seconds in the call
        long init_attempts = 0, init_device_calls = 0; double t_init_attempt = 0;      // monocular initialisation: two_view_initialize calls, their steps that ran on the device (initialiseOnDevice), seconds the calls took
        long triangulated = 0, tri_pairs = 0, tri_exhausted = 0;      // triangulateNeighbours: landmarks made, (keyframe, neighbour) pairs served, queries whose eight candidates were all taken while more had passed
        long fisheye_dropped = 0;                     // fisheye session: keypoints the undistort stage removed (beyond the angle limit or 90 degrees, not converged), summed
        long perspective_dropped = 0;                 // radial-tangential session: keypoints the undistort stage removed (a denominator not positive, or the result more than half a pixel off its pixel), summed
        long intensity_adjusted = 0;                  // frames whose intensity adjustment ran on the device (a request the host had applied already does not count)
        // where the frames' time went (seconds, summed): front end (upload, extraction, stereo, read-back), tracking against the
        // previous frame, local-map tracking, keyframe work on the tracking thread (insertion, fusion, loop search, BA set-up / wait)
        double t_front = 0, t_track = 0, t_local = 0, t_keyframe = 0, t_total = 0;
        double t_kf_triangulate = 0;                  // inside t_kf_insert: the triangulation step
        double t_kf_wait = 0, t_kf_apply = 0, t_kf_insert = 0, t_kf_loop = 0, t_kf_prepare = 0, t_map_solve = 0;      // keyframe path: waiting for the previous window's solve, applying it, the new keyframe, the next window's set-up; the mapping thread's solve
        double t_prefetch_wait = 0, t_prefetch_busy = 0;       // this thread waiting for the prefetch thread at the end of a frame / that thread's own time per frame
        double t_dev_match = 0, t_dev_pose = 0, t_dev_upload = 0, t_dev_extract = 0, t_dev_get = 0;      // inside the above: device calls
    };

    bool startContext(bool stereo);
    void warmUpContext(bool stereo);                  // one frame's worth of every per-frame call on blank images: lazily created resources exist before the first frame
    ProcessImageResult trackFrame(CameraQueueEntry& cam, bool stereo, const std::optional<GlobalStateInTime>& navOdom,
                                  std::optional<ScanAttach> scan = std::nullopt);
    TrackerResult createTrackerResult(const Pose& pose_cw, TimeStamp timestamp, const double* sigma4) const;
    bool initializeMap(FrameData& f, const Pose& at);
    bool poseFromMatches(FrameData& cur, const std::vector<int>& cur_idx, const std::vector<int>& lm_ids, const Pose& init, int& n_inliers, int min_inliers = 10);
    void poseSigmas(FrameData& cur, const double* pose7, const std::vector<double>& pts, const std::vector<lpslam_hip_ba_obs>& obs, const std::vector<uint8_t>& outlier);
    // pc = R X + t and its pinhole image (u, v): false when the point is not in front of the camera or falls outside the image
    // (the ONE visibility test of the tracker: nothing else compares against the resolution)
    // (defined here, as projQuery is, so that the per-landmark loops of the query builders keep them inline)
    bool project(const Mat3& R, const double* t, const double* X, double* pc, double& u, double& v) const
    {
        transform(R, t, X, pc);
        if (!(pc[2] > 0)) return false;
        u = m_cam.f_x * pc[0] / pc[2] + m_cam.c_x; v = m_cam.f_y * pc[1] / pc[2] + m_cam.c_y;
        // a fisheye session matches at the pinhole (u, v) -- its keypoints are undistorted -- but what the SENSOR sees decides visibility:
        // inside the angle limit and the distorted pixel inside the image (fisheye_math.h)
        if (m_fisheye) return lpslam_fisheye::visible(m_fisheyeModel, pc[0], pc[1], pc[2], m_cam.resolution_x, m_cam.resolution_y);
        // a radial-tangential session likewise: (u, v) inside the bounds of the undistorted image and the distorted pixel inside the image (radtan_math.h)
        if (m_radtan) return lpslam_radtan::visible(m_radtanModel, m_radtanBounds, pc[0], pc[1], pc[2], m_cam.resolution_x, m_cam.resolution_y);
        return !(u < 0 || v < 0 || u >= m_cam.resolution_x || v >= m_cam.resolution_y);
    }
    lpslam_hip_proj_query projQuery(double u, double v, double z, float radius, int min_level, int max_level, bool stereo) const
    {
        lpslam_hip_proj_query e{};
        e.x = (float)u; e.y = (float)v; e.x_right = stereo ? (float)(u - m_cam.focal_x_baseline / z) : -1.0f;
        e.radius = radius; e.min_level = min_level; e.max_level = max_level;
        return e;
    }
    lpslam_hip_ba_camera baCamera(bool with_baseline) const;
    // descriptor matches (mq[k]: keypoint of the frame, < 0 = none; mt[k]: keypoint of the other side, NULL = k) -> keypoint <-> landmark
    // associations through the other side's landmark list
    void associate(const int32_t* mq, const int32_t* mt, int n, const std::vector<int>& landmark, std::vector<int>& cur_idx, std::vector<int>& lm_ids) const;
    static std::vector<float> keypointAngles(const std::vector<lpslam_hip_keypoint>& kpts);
    bool frameSizeOk(const CameraQueueEntry& cam, bool stereo) const;
    bool predictedPose(Pose& init) const;
    bool navDelta(Pose& v) const;                     // motion of the navigation prior between the last two frames (world -> camera)
    bool trackWithMotionModel(FrameData& cur, int& n_inliers);
    bool trackAgainstPrevious(FrameData& cur, int& n_inliers);
    bool trackLocalMap(FrameData& cur, int& n_inliers);
    bool relocalise(FrameData& cur);
    // monocular: map initialisation from two views ([UPSTREAM] module::initializer + initialize::perspective) and new landmarks
    // by triangulation between consecutive keyframes ([UPSTREAM] mapping_module::create_new_landmarks, previous keyframe only)
    bool monoInitialize(FrameData& cur);
    void monoTriangulate(int prev_kf, Keyframe& kf, FrameData& f);
    // triangulateNeighbours > 0: the keypoints of the keyframe being inserted (id = m_kfs.size(), keypoints in f.slot) that carry no
    // landmark against those of its best covisible keyframes -- candidate lists and tri_pair on the device
    // (lpslam_hip_triangulate_neighbours), ordered replay and orientation filter here
    void triangulateNeighbours(Keyframe& kf, FrameData& f);
    std::vector<int> covisibleOf(const std::vector<int>& landmark, int kf, int top_n, int min_weight) const;      // covisible() of a keyframe that is not stored yet
    bool detectAndCloseLoop(FrameData& cur, int c);
    void initLandmarkView(Landmark& lm, const Pose& pose, const lpslam_hip_keypoint& kp, const uint8_t* desc32) const;
    int insertKeyframe(FrameData& f);
    int resolve(int id) const;                        // follows the replacements of merged landmarks
    std::vector<int> covisible(int kf, int top_n, int min_weight) const;
    // [UPSTREAM] mapping_module::fuse_landmark_duplication / match::fuse: the given landmarks are projected into keyframe `c`
    // (whose keypoints sit in image slot `slot`); a match with a keypoint that has no landmark adds an observation, a match with
    // one that has another landmark merges the two (the one with more observations stays)
    void fuseInto(int c, int slot, const std::vector<int>& landmark_ids, FrameData& f, long& added, long& merged);
    void mergeLandmarks(int keep, int drop, FrameData* f);
    bool keyframeNeeded(int inliers) const;
    // Local bundle adjustment ([UPSTREAM] mapping_module -> optimize::local_bundle_adjuster): the new keyframe and its covisible
    // keyframes are free, every other keyframe that sees their landmarks is held fixed.  As in the reference it runs beside
    // tracking: the problem is copied when a keyframe is inserted, a mapping thread solves it on the GPU (the BA object has its own
    // stream) while the tracking thread takes the next frames, and the result enters the map right before the next keyframe is
    // inserted -- a fixed point of the frame sequence, so a run is reproducible.
    struct MappingJob {
        std::vector<double> poses, pts;
        std::vector<uint8_t> fixed, outlier;
        std::vector<lpslam_hip_ba_obs> obs;
        std::vector<std::pair<int, int>> origin;      // (keyframe, keypoint) of every BA observation
        std::vector<int> ids;                         // landmark id of every BA point
        std::vector<int> kfs;                         // keyframe of every BA pose
        bool global = false;                          // loop-time global BA: plain robust iterations, no outlier pass
        int keyframe = -1;                            // local BA: the keyframe it was started for (redundant-keyframe culling follows it)
        bool solved = false;
    };
    std::unique_ptr<MappingJob> prepareMapping(int c);
    std::unique_ptr<MappingJob> prepareBundle(const std::vector<int>& free_kfs, const std::vector<int>& fixed_kfs);
    void solveMapping(MappingJob& job) const;
    void runGlobalBundle(MappingJob& job, int iterations, const lpslam_hip_ba_camera& cam) const;      // create / optimise / get / destroy
    void applyMapping(const MappingJob& job);
    void startMapping(int c);                         // prepare + solve on the mapping thread (or inline when asyncMapping is off)
    void finishMapping();                             // wait for the mapping thread and apply its result
    void logStatistics();
    std::string m_lastStatistics;                       // the line logStatistics() logged last (kept past stop(): lastStatistics())
    void storeDescriptors(int key, Keyframe& kf);     // keeps the keyframe's descriptors on the device for the batched loop-candidate search
    // map database (src/Trackers/OpenVSLAMTrackerBase.cpp:241-255,287-294): used only when useMapDb is on AND a file name was given
    // (mapFilename in the configuration or mappingSetFilename) -- no implicit map.db in the working directory
    bool mapDbActive() const { return m_useMapDb && (m_mapFilenameGiven || m_mapFilenameSet) && !m_mapFilename.empty(); }
    void loadMap();                                   // startContext: restores the map, or leaves it empty (rejected file: m_mapRejected)
    void saveMap();                                   // stop(): the map into m_mapFilename
    bool m_mapFilenameGiven = false, m_mapFilenameSet = false;
    bool m_mapLoaded = false, m_mapRejected = false;
    bool m_localiseOnly = false;                      // a loaded map with enableMapping off: no keyframes, no loop closing, never re-initialise
    bool m_relocByRank = false;                       // after a load, until the first relocalisation: candidates by lpslam_hip_rank_stored over all keyframes
    bool m_lostSinceUnset = false;
    int sharedRefKf(const FrameData& f) const;          // localisation only: the keyframe that sees most of the frame's landmarks (-1: none)                    // the loss started before the first frame (a loaded map): its first frame starts the clock

    // occupancy grid: scans in, the keyframes' scans into the context's store, the grid out (any thread; device work without m_slamLock)
    void bufferLaserScan(float* ranges, size_t n, float range_min, float range_max, float angle_min, float increment, float range_threshold,
                         const std::optional<LpSlamROSTimestamp>& ros);
    std::optional<ScanAttach> scanForFrame(const CameraQueueEntry& cam);
    void storeScan(int key, const ScanAttach& a);     // m_slamLock held
    bool occupancyBuild(int8_t* out, std::size_t capacity, lpslam_hip_grid_info& info);
    std::vector<lpslam_hip_scan_pose> scanPoses(std::vector<LpSlamROSTimestamp>* stamps);      // m_slamLock held
    std::mutex m_laserMutex;                          // the scan buffer and the transformation callback
    std::mutex m_occMutex;                            // an export in progress (taken before m_slamLock; stop() waits for it before the context goes)
    std::shared_ptr<const LaserScan> m_laserBuffer;
    RequestNavTransformationCallback_t m_navTransform = nullptr; void* m_navTransformData = nullptr;
    std::map<std::pair<int, std::pair<float, float>>, int> m_scanGeometries;      // (beams, (angle_min, increment)) -> geometry id of the context
    double m_occResolution = 0.05; int m_occMaxSide = 4096;

    // configuration (names as in the reference tracker)
    bool m_useLiveView = false, m_useMapDb = true, m_forwardNavState = true, m_forwardImu = true, m_emitMap = false;
    bool m_enableMapping = true, m_waitForNavigation = false, m_forwardHighResNav = false, m_loopClosure = true;
    bool m_useOpenCL = false, m_useCUDA = false, m_relocWithNavigation = true, m_asyncMapping = true, m_prefetch = true;
    int m_mappingReserve = 0;                      // compute units of every XCD the front end leaves to the mapping thread's solves
    std::string m_configFromFile, m_cameraSetup = "monocular", m_vocabFile = "orb_vocab.dbow2", m_mapFilename = "map.db";
    int m_slamKeypoints = 1200, m_viewerFps = 10;
    double m_baselineDistThresh = 0.1, m_maxLaserAge = 1.0;      // baselineDistThresh: read by the triangulateNeighbours step only
    bool m_poseSigma = false;                         // poseFromMatches(): the pose's covariance from the device (lpslam_hip_pose_covariance_batch) into the result's sigmas
    bool m_poseSigmaFailureLogged = false;
    bool m_initialiseOnDevice = false;                // monoInitialize(): the RANSAC loop and the pose check of two_view_initialize on the device (lpslam_hip_two_view_*)
    bool m_verifyLoopsOnDevice = false;               // closeLoop(): solver, gate and optimiser of all candidates in one device call (lpslam_hip_sim3_verify_batch)
    bool m_relocaliseOnDevice = false;                // relocalise(): the candidates' pose solver in one device call (lpslam_hip_pnp_ransac_batch)
    int m_triangulateNeighbours = 0;                  // 0: as before (monocular: the previous keyframe by brute force; stereo: nothing); 1 .. 32: that many covisible keyframes
    // MI355X additions: the generated reference config hard-codes these
    int m_numLevels = 3, m_iniFastThr = 20, m_minFastThr = 7, m_device = 0, m_keyframeInterval = 6, m_localWindow = 10;
    double m_scaleFactor = 1.2;

    std::mutex m_slamLock;
    lpslam_hip_ctx* m_ctx = nullptr;
    LpSlamCameraConfiguration m_cam{};
    bool m_started = false, m_stereo = false, m_rectify = false;
    // monocular fisheye session (src/Trackers/OpenVSLAMTrackerBase.cpp:170-175 hands Camera.model = fisheye, k1 .. k4 to its tracker):
    // the context undistorts and compacts the keypoints (lpslam_hip_set_keypoint_camera), project() tests visibility on the sensor
    bool m_fisheye = false;
    lpslam_fisheye::Model m_fisheyeModel{};
    double m_fisheyeMaxAngleDeg = 70.0;
    // monocular radial-tangential session (a configFromFile with Camera.model = perspective and k1, k2, p1, p2, k3, which the reference
    // hands to its tracker unchanged, OpenVSLAMTrackerBase.cpp:114-123): lpslam_hip_set_keypoint_camera_radtan; the bounds of the
    // undistorted image are computed once at start
    bool m_radtan = false;
    lpslam_radtan::Model m_radtanModel{};
    lpslam_radtan::Bounds m_radtanBounds{};
    MapFileCamera sessionMapCamera() const;           // the camera record a map file of this session carries
    TrackerState m_state = TrackerState::NotInitialized;
    std::optional<TimeStamp> m_firstImageTimestamp;
    uint64_t m_imageTracked = 0;
    // Image slots: a ring of three slot pairs -- the frame being tracked, the previous one (brute-force fallback, scratch for
    // relocalisation / loop candidates once it is no longer needed) and the next one, whose front end is prefetched.
    static int slotOf(uint64_t frame_index) { return (int)(frame_index % 3) * 2; }
    static int previousSlot(int slot) { return ((slot / 2 + 2) % 3) * 2; }
    // map maintenance ([UPSTREAM] module::local_map_cleaner, run by the mapping module around every local BA)
    bool m_mapCulling = true;
    std::vector<int> m_freshLandmarks;                  // landmarks younger than three keyframes
    void cullLandmarks(int cur_kf);
    void cullKeyframes(int cur_kf);
    void eraseLandmark(int id);
    // bag-of-words place recognition ([UPSTREAM] data::bow_vocabulary / bow_database): loaded from vocabFile when that file exists
    lpslam_hip_vocab* m_vocab = nullptr;
    int m_bowLevelsUp = 4;                              // FeatureVector level: 4 levels above the leaves as upstream, less for shallow trees
    BowDatabase m_bowDb;
    void computeBow(Keyframe& kf) const;
    bool frameNodes(const FrameData& f, std::vector<int32_t>& node, BowVector* bow) const;
    struct Prefetched { bool valid = false; bool issued = false /* work may sit on the prefetch stream, valid or not */; const uint8_t* data = nullptr; TimeStamp timestamp{}; int slot = 0; bool stereo = false; std::optional<IntensityAdjust> adjust /* what the prefetch applied on the device */; } m_prefetched;
    void prefetchFrame(CameraQueueEntry const& cam, bool stereo);      // m_slamLock held
    CameraQueueEntry const* m_nextFrame = nullptr;
    void setNextFrame(CameraQueueEntry const* next) override { m_nextFrame = next; }
    bool realisesAdjust() const override { return true; }      // a pending intensity adjustment runs on the device, inside frontEnd
    bool realisesGray() const override { return true; }        // ... and so does a pending colour conversion, in front of it
    bool frontEnd(CameraQueueEntry const& cam, bool stereo, int slot);
    double m_lastFrameSeconds = 0;
    int m_maxKp = 0;
    float m_scales[LPSLAM_HIP_MAX_LEVELS] = {0};
    FrameData m_prev;
    bool m_havePrev = false;
    Pose m_velocity;                                  // last inter-frame motion (constant-velocity prediction)
    bool m_haveVelocity = false;
    int m_framesSinceKeyframe = 0;
    std::vector<Keyframe> m_kfs;                      // the map's keyframes, index = id
    std::vector<std::pair<std::vector<int>, int>> m_loopSets;      // (keyframe set, continuity) of the loop candidates detected at the previous keyframe ([UPSTREAM] cont_detected_keyfrm_sets_)
    std::unordered_map<int, Landmark> m_landmarks;
    // Landmark ids are dense (0 .. m_nextLandmarkId): an index of the map's nodes by id (a node stays where it is until it is erased) and
    // scratch marks by id replace the hash lookups of the per-frame and per-keyframe loops (covisibility, local landmarks, window assembly:
    // 0.10 of a 0.50 ms frame were hash operations)
    std::vector<Landmark*> m_lmIndex;
    Landmark* lm(int id) const { return id >= 0 && (size_t)id < m_lmIndex.size() ? m_lmIndex[(size_t)id] : nullptr; }
    void indexLandmark(int id) { if ((size_t)id >= m_lmIndex.size()) m_lmIndex.resize((size_t)id + 256, nullptr); m_lmIndex[(size_t)id] = &m_landmarks.find(id)->second; }
    void unindexLandmark(int id) { if (id >= 0 && (size_t)id < m_lmIndex.size()) m_lmIndex[(size_t)id] = nullptr; }
    struct IdMarks {                                  // value per id, valid for the current round only (begin() starts a round in O(1))
        std::vector<uint32_t> round; std::vector<int32_t> val; uint32_t cur = 0;
        void begin(size_t n) { if (round.size() < n) { round.resize(n + 256, 0); val.resize(n + 256, 0); } if (++cur == 0) { std::fill(round.begin(), round.end(), 0u); cur = 1; } }
        bool has(int id) const { return id >= 0 && (size_t)id < round.size() && round[(size_t)id] == cur; }
        int32_t& at(int id) { if (round[(size_t)id] != cur) { round[(size_t)id] = cur; val[(size_t)id] = 0; } return val[(size_t)id]; }
        int32_t get(int id) const { return has(id) ? val[(size_t)id] : 0; }
    };
    mutable IdMarks m_marksA, m_marksB, m_marksC, m_marksKf;      // tracking thread only
    std::unordered_map<int, int> m_replaced;          // merged landmark -> the one that took its observations
    int m_nextLandmarkId = 0;
    int m_refKf = -1;                                 // reference keyframe of tracking (the last one inserted)
    int m_refTracked = 0;                             // landmarks the reference keyframe held when it was inserted
    int m_segment = 0, m_segmentStart = 0;            // current map segment and its first keyframe
    // loss and relocalisation (the reference forwards time_to_relocalize = 3.0 s, src/Trackers/OpenVSLAMTrackerBase.cpp:210-211)
    Pose m_lastGoodPose;
    TimeStamp m_lostSince{};
    double m_timeToRelocalize = 3.0;
    // Initializer.num_min_triangulated_pts / parallax_deg_threshold as the reference sets them (src/Trackers/OpenVSLAMTrackerBase.cpp:181-182)
    int m_initMinTriangulated = 40;
    double m_initParallaxDeg = 0.2;
    // navigation prior (src/Trackers/OpenVSLAMStereoTracker.cpp:70-179): camera pose of the odometry, optical axes, world -> camera
    std::optional<Pose> m_navPrev, m_navCur;
    Statistics m_stats;
    FrameData m_monoRef;                              // monocular initialisation: the reference frame ...
    bool m_haveMonoRef = false;
    std::vector<float> m_monoPrevMatched;             // ... and where each of its keypoints was last matched (x, y)
    // the mapping thread (one per tracker, started with the context): a one-slot mailbox each way
    // the prefetch helper: ONE persistent thread (a std::async per frame spawned and joined a thread every frame)
    std::thread m_pfThread;
    std::mutex m_pfMutex;
    std::condition_variable m_pfCv;
    const CameraQueueEntry* m_pfJob = nullptr; bool m_pfStereo = false, m_pfBusy = false, m_pfQuit = false;
    void prefetchLoop();
    void prefetchSubmit(const CameraQueueEntry* next, bool stereo);
    void prefetchWait();
    void stopPrefetchThread();
    std::thread m_mapThread;
    std::mutex m_mapMutex;
    std::condition_variable m_mapCv;
    std::unique_ptr<MappingJob> m_mapIn, m_mapOut;
    bool m_mapBusy = false, m_mapQuit = false;
    void mappingLoop();
    void stopMappingThread();
};

// the keypoint camera of a monocular session and the flat "Section.key" view of an OpenVSLAM YAML file (hip_tracker.cpp; also reached
// through the C shim, for tests without a device)
int resolveFisheyeModel(const LpSlamCameraConfiguration& cam, const std::unordered_map<std::string, std::string>& yaml, double max_angle_deg,
                        lpslam_fisheye::Model* out, std::string* why);
// the radial-tangential model of a monocular session: only from a YAML file (Camera.model = perspective, or no Camera.model and a camera
// that is not a fisheye one) with at least one of Camera.k1, k2, p1, p2, k3 a non-zero number.  1: *out is the model; 0: none (no file,
// another model, all coefficients zero or absent -- a Pinhole camera of the JSON configuration gets none whatever its dist[] holds, as
// in the reference, OpenVSLAMTrackerBase.cpp:161-169); -1: refused, *why says it (names the key that is not a number).
int resolveRadtanModel(const LpSlamCameraConfiguration& cam, const std::unordered_map<std::string, std::string>& yaml, lpslam_radtan::Model* out, std::string* why);
bool loadFlatYaml(const std::string& path, std::unordered_map<std::string, std::string>& yaml, std::string* bad_line);
// the triangulateNeighbours step's host rules (hip_tracker.cpp; also reached through the C shim, for tests without a device):
// the option's range; the neighbour list -- the covisible keyframes in their order, for a monocular session the previous keyframe of the
// segment (prev >= 0) in front when it is absent, cut to n; the median of a keyframe's landmark depths (the lower one of an even count,
// -1 without landmarks)
inline bool triangulateNeighboursOk(int n) { return n >= 0 && n <= lpslam_tri::kMaxSets; }
std::vector<int> triangulationNeighbourList(const std::vector<int>& covisible, int prev, int n);
double medianDepth(std::vector<double> depths);

class HipStereoTracker : public HipVslamTrackerBase {
public:
    ProcessImageResult processImage(CameraQueueEntry& cam, std::optional<GlobalStateInTime> navResultOdom = std::nullopt,
                                    std::optional<GlobalStateInTime> navResultMap = std::nullopt,
                                    std::vector<SensorQueueEntry> const& sensorValues = {}) override;
    bool start(SensorQueue&) override;
    std::string type() override { return "VSLAMStereo"; }       // src/Trackers/OpenVSLAMStereoTracker.h:35-39
    void addLaserScan(GlobalStateInTime origin, float* ranges, size_t n, float range_min, float range_max, float angle_min, float angle_max,
                      float increment, float range_threshold) override;
    std::optional<unsigned long> mappingGetMapRawSize() override;
    std::optional<LpMapInfo> mappingGetMapRaw(int8_t* map, std::size_t capacity) override;
};

class HipMonoTracker : public HipVslamTrackerBase {
public:
    ProcessImageResult processImage(CameraQueueEntry& cam, std::optional<GlobalStateInTime> navResultOdom = std::nullopt,
                                    std::optional<GlobalStateInTime> navResultMap = std::nullopt,
                                    std::vector<SensorQueueEntry> const& sensorValues = {}) override;
    bool start(SensorQueue&) override;
    std::string type() override { return "VSLAMMono"; }
};

}  // namespace LpSlam
