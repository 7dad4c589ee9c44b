// interface.cpp -- LpSlamManager (include/lpslam_manager.h): one-line forwards to LpSlam::SlamManager, like the reference's
// pimpl (/root/reference/src/InterfaceImpl/LpSlamManager.cpp:52-243), plus a plain-C shim of the same calls for
// non-C++ clients and the Python tests.
#include <atomic>
#include "../../include/lpslam_manager.h"
#include "slam_manager.h"
#include "ingest.h"
#include "intensity.h"
#include "jpeg.h"
#include "map_file.h"
#include "occupancy.h"
#include "hip_tracker.h"
#include "../csrc/fisheye_math.h"
#include <cstring>
#include <limits>
#include <unordered_map>
#include <vector>

namespace LpSlam { LpSlamCameraConfiguration defaultCameraConfiguration(); }

LpSlamCameraConfiguration LpSlamConfiguration::createDefaultCameraConfiguration() { return LpSlam::defaultCameraConfiguration(); }

LpSlamManager::LpSlamManager() { m_impl = new LpSlam::SlamManager(); }
LpSlamManager::~LpSlamManager() { delete m_impl; }
void LpSlamManager::logToFile(char const* filename) { m_impl->logToFile(filename ? filename : ""); }
void LpSlamManager::setLogLevel(LpSlamLogLevel l) { m_impl->setLogLevel(l); }
void LpSlamManager::addOnReconstructionCallback(OnReconstructionCallback_t cb, void* ud) { m_impl->addOnReconstructionCallback(cb, ud); }
void LpSlamManager::addRequestNavDataCallback(RequestNavDataCallback_t cb, void* ud) { m_impl->addRequestNavDataCallback(cb, ud); }
void LpSlamManager::addRequestNavTransformation(RequestNavTransformationCallback_t cb, void* ud) { m_impl->addRequestNavTransformation(cb, ud); }
void LpSlamManager::addOnImageCallback(OnImageCallback_t cb, void* ud) { m_impl->addOnImageCallback(cb, ud); }
void LpSlamManager::updateGlobalReferenceState(LpSlamGlobalStateInTime) {}
void LpSlamManager::addImageFromFile(char const*) {}
void LpSlamManager::addStereoImageFromFiles(char const*, char const*) {}
void LpSlamManager::addMarker(LpSlamMarkerIdentifier, LpSlamMarkerState) {}      // no-op in the reference too (SlamManager.cpp:1311-1312)
bool LpSlamManager::addImageFromBuffer(uint32_t n, LpSlamTimestamp t, uint8_t* b, LpSlamImageDescription d) { return m_impl->addImageFromBuffer(n, t, b, d); }
bool LpSlamManager::addStereoImageFromBuffer(uint32_t n, LpSlamTimestamp t, uint8_t* l, uint8_t* r, LpSlamImageDescription d) { return m_impl->addStereoImageFromBuffer(n, t, l, r, d); }
// src/InterfaceImpl/LpSlamManager.cpp:133-152: the buffer is taken as BGRA (Webots), turned grey with cv::cvtColor(COLOR_BGRA2GRAY) -- fixed-point weights
// B 1868, G 9617, R 4899, >> 14 -- and written as cv::imencode(".jpg") writes it: libjpeg, baseline, quality 95 (host/jpeg.cpp; the
// stream is libjpeg's byte for byte).  8UC1 / 8UC3 buffers are taken as what they say they are.  `bufferOut` is as large as the input.
bool LpSlamManager::compressImage(uint8_t* buffer, LpSlamImageDescription desc, uint8_t* bufferOut, uint32_t* bufferOutSize)
{
    if (!buffer || !bufferOut || !bufferOutSize || desc.width == 0 || desc.height == 0) return false;
    LpSlam::GrayImage g; g.width = (int)desc.width; g.height = (int)desc.height;
    const size_t n = (size_t)desc.width * desc.height;
    g.pixels.resize(n);
    size_t in_bytes = 4 * n;
    if (desc.format == LpSlamImageFormat_8UC1) { std::memcpy(g.pixels.data(), buffer, n); in_bytes = n; }
    else if (desc.format == LpSlamImageFormat_8UC3) {
        const int format = desc.image_conversion == LpSlamImageConversion_BGR2RGB ? LPSLAM_HIP_PIXEL_BGR8 : LPSLAM_HIP_PIXEL_RGB8;
        if (!LpSlam::gray_from_pixels_host(g.pixels.data(), desc.width, g.width, g.height, buffer, 3 * (size_t)desc.width, nullptr, 0, format)) return false;
        in_bytes = 3 * n;
    } else {
        for (size_t i = 0; i < n; ++i) g.pixels[i] = (uint8_t)((buffer[4 * i] * 1868 + buffer[4 * i + 1] * 9617 + buffer[4 * i + 2] * 4899 + (1 << 13)) >> 14);
    }
    std::vector<uint8_t> out;
    if (!LpSlam::encode_jpeg_gray(g, 95, out) || out.size() > in_bytes) return false;      // (a stream larger than its image: tiny noise images only)
    std::memcpy(bufferOut, out.data(), out.size());
    *bufferOutSize = (uint32_t)out.size();
    return true;
}
void LpSlamManager::setCameraConfiguration(LpSlamCameraConfiguration c) { m_impl->setCameraConfiguration(c); }
bool LpSlamManager::readConfigurationFile(char const* f) { return m_impl->readConfigurationFile(f ? f : ""); }
bool LpSlamManager::readReplayItems(char const* f) { return m_impl->loadReplayItems(f ? f : ""); }
bool LpSlamManager::addSource(char const* n, char const* c) { return m_impl->addSource(n ? n : "", c ? c : ""); }
bool LpSlamManager::addTracker(char const* n, char const* c) { return m_impl->addTracker(n ? n : "", c ? c : ""); }
bool LpSlamManager::addProcessor(char const* n, char const* c) { return m_impl->addProcessor(n ? n : "", c ? c : ""); }
void LpSlamManager::setShowLiveStream(bool) {}
void LpSlamManager::setWriteImageFiles(bool on) { m_impl->setWriteImageFiles(on); }
void LpSlamManager::setRecord(bool on) { m_impl->setRecord(on); }
void LpSlamManager::setRecordImages(bool on) { m_impl->setRecordImages(on); }
void LpSlamManager::start() { m_impl->start(); }
void LpSlamManager::stop() { m_impl->stop(); }
LpSlamStatus LpSlamManager::getSlamStatus() { return m_impl->getSlamStatus(); }
void LpSlamManager::mappingAddLaserScan(LpSlamGlobalStateInTime o, float* r, size_t n, float r0, float r1, float a0, float a1, float inc, float thr) {
    m_impl->mappingAddLaserScan(LpSlam::conversion::gsInTimeInterfaceToInternal(o), r, n, r0, r1, a0, a1, inc, thr);
}
unsigned long LpSlamManager::mappingGetMapRawSize() { return m_impl->mappingGetMapRawSize(); }
LpMapInfo LpSlamManager::mappingGetMapRaw(int8_t* map, std::size_t capacity) { return m_impl->mappingGetMapRaw(map, capacity); }
std::size_t LpSlamManager::mappingGetFeatures(LpSlamMapBoundary b, LpSlamFeatureEntry* e, std::size_t n, LpSlamMatrix9x9 t) { return m_impl->mappingGetFeatures(b, e, n, t); }
std::size_t LpSlamManager::mappingGetFeaturesCount(LpSlamMapBoundary b) { return m_impl->mappingGetFeaturesCount(b); }
bool LpSlamManager::mappingSetMode(bool e) { return m_impl->mappingSetMode(e); }
bool LpSlamManager::mappingSetFilename(const char* f) { return m_impl->mappingSetFilename(f ? f : ""); }
bool LpSlamManager::mappingExportCSV(const char* f) { return m_impl->mappingExportCSV(f ? f : ""); }

// ---- plain-C shim ----------------------------------------------------------------------------------------------------
extern "C" {
#define LPS_API __attribute__((visibility("default")))
typedef void (*lpslam_c_reconstruction_cb)(const LpSlamGlobalStateInTime* state, void* user);
struct lpslam_c_manager { LpSlamManager mgr; lpslam_c_reconstruction_cb cb = nullptr; void* user = nullptr; std::atomic<uint64_t> n_results{0}, n_valid{0}; LpSlamGlobalState laser_to_camera{}; };
static void c_trampoline(LpSlamGlobalStateInTime const& s, void* p) { auto* m = static_cast<lpslam_c_manager*>(p); if (m->cb) m->cb(&s, m->user); }

LPS_API lpslam_c_manager* lpslam_manager_create(void) { return new lpslam_c_manager(); }
LPS_API void lpslam_manager_destroy(lpslam_c_manager* m) { delete m; }
LPS_API void lpslam_manager_set_log_level(lpslam_c_manager* m, int level) { m->mgr.setLogLevel((LpSlamLogLevel)level); }
LPS_API void lpslam_manager_log_to_file(lpslam_c_manager* m, const char* f) { m->mgr.logToFile(f); }
LPS_API int lpslam_manager_read_configuration_file(lpslam_c_manager* m, const char* f) { return m->mgr.readConfigurationFile(f); }
LPS_API int lpslam_manager_add_tracker(lpslam_c_manager* m, const char* n, const char* c) { return m->mgr.addTracker(n, c); }
LPS_API int lpslam_manager_add_processor(lpslam_c_manager* m, const char* n, const char* c) { return m->mgr.addProcessor(n, c); }
LPS_API int lpslam_manager_add_source(lpslam_c_manager* m, const char* n, const char* c) { return m->mgr.addSource(n, c); }
LPS_API void lpslam_manager_set_camera_configuration(lpslam_c_manager* m, const LpSlamCameraConfiguration* c) { m->mgr.setCameraConfiguration(*c); }
LPS_API void lpslam_manager_default_camera_configuration(LpSlamCameraConfiguration* out) { *out = LpSlamConfiguration().createDefaultCameraConfiguration(); }
LPS_API void lpslam_manager_on_reconstruction(lpslam_c_manager* m, lpslam_c_reconstruction_cb cb, void* user) { m->cb = cb; m->user = user; m->mgr.addOnReconstructionCallback(c_trampoline, m); }
LPS_API void lpslam_manager_on_image(lpslam_c_manager* m, OnImageCallback_t cb, void* user) { m->mgr.addOnImageCallback(cb, user); }
LPS_API void lpslam_manager_request_nav_data(lpslam_c_manager* m, RequestNavDataCallback_t cb, void* user) { m->mgr.addRequestNavDataCallback(cb, user); }
// A compiled RequestNavDataCallback_t that answers every request with a valid identity odometry (what Manager.provide_odometry's
// Python callback answers): for throughput measurements, where a Python callback per frame on the worker thread costs more than the
// tracker's own host work.
static LpSlamRequestNavDataResult identity_odometry(LpSlamROSTimestamp, LpSlamGlobalStateInTime* odom, LpSlamGlobalStateInTime*, void*) {
    odom->state.valid = true;
    odom->state.orientation.w = 1.0;
    return LpSlamRequestNavDataResult_OdomOnly;
}
LPS_API void lpslam_manager_request_identity_nav_data(lpslam_c_manager* m) { m->mgr.addRequestNavDataCallback(identity_odometry, nullptr); }
// A compiled OnReconstructionCallback_t that only counts (results, valid results): sixteen managers at 2000 results per second each are
// 32 000 interpreter entries per second from sixteen notify threads otherwise -- the measurement would be of the interpreter lock.
static void counting_result(LpSlamGlobalStateInTime const& s, void* p) { auto* m = static_cast<lpslam_c_manager*>(p); m->n_results.fetch_add(1); if (s.state.valid) m->n_valid.fetch_add(1); }
LPS_API void lpslam_manager_count_results(lpslam_c_manager* m) { m->n_results = 0; m->n_valid = 0; m->mgr.addOnReconstructionCallback(counting_result, m); }
LPS_API void lpslam_manager_result_counts(lpslam_c_manager* m, uint64_t* results, uint64_t* valid) { if (results) *results = m->n_results.load(); if (valid) *valid = m->n_valid.load(); }
LPS_API int lpslam_manager_add_stereo_image(lpslam_c_manager* m, uint32_t cam, uint64_t ts, uint8_t* l, uint8_t* r, const LpSlamImageDescription* d) { return m->mgr.addStereoImageFromBuffer(cam, ts, l, r, *d); }
LPS_API int lpslam_manager_add_image(lpslam_c_manager* m, uint32_t cam, uint64_t ts, uint8_t* b, const LpSlamImageDescription* d) { return m->mgr.addImageFromBuffer(cam, ts, b, *d); }
LPS_API int lpslam_manager_compress_image(uint8_t* b, const LpSlamImageDescription* d, uint8_t* out, uint32_t* out_size) { return LpSlamManager::compressImage(b, *d, out, out_size); }
LPS_API int lpslam_manager_read_replay_items(lpslam_c_manager* m, const char* f) { return m->mgr.readReplayItems(f); }
LPS_API void lpslam_manager_start(lpslam_c_manager* m) { m->mgr.start(); }
LPS_API void lpslam_manager_stop(lpslam_c_manager* m) { m->mgr.stop(); }
LPS_API void lpslam_manager_status(lpslam_c_manager* m, LpSlamStatus* out) { *out = m->mgr.getSlamStatus(); }
LPS_API size_t lpslam_manager_features(lpslam_c_manager* m, LpSlamFeatureEntry* e, size_t n, const float* t9) {
    LpSlamMatrix9x9 t; for (int i = 0; i < 9; ++i) t[i] = t9[i];
    return m->mgr.mappingGetFeatures(LpSlamMapBoundary{}, e, n, t);
}
// this manager's own tracker statistics (the log file is process-wide: with several managers in a process their lines share it);
// returns the length of the line, copies at most cap - 1 characters
static_assert(sizeof(LpSlamManager) == sizeof(void*), "LpSlamManager holds m_impl and nothing else (src/Interface/LpSlamManager.h:120)");
LPS_API size_t lpslam_manager_tracker_statistics(lpslam_c_manager* m, char* out, size_t cap) {
    LpSlam::SlamManager* impl = *reinterpret_cast<LpSlam::SlamManager**>(&m->mgr);
    const std::string s = impl ? impl->trackerStatistics() : std::string();
    if (out && cap) { const size_t n = std::min(s.size(), cap - 1); memcpy(out, s.data(), n); out[n] = 0; }
    return s.size();
}
// recording (record.h): set before start()
LPS_API void lpslam_manager_set_record(lpslam_c_manager* m, int on) { m->mgr.setRecord(on != 0); }
LPS_API void lpslam_manager_set_record_images(lpslam_c_manager* m, int on) { m->mgr.setRecordImages(on != 0); }
LPS_API void lpslam_manager_set_write_image_files(lpslam_c_manager* m, int on) { m->mgr.setWriteImageFiles(on != 0); }
// test hook: out[4] = images encoded on the device, images encoded on the host, records written, bytes written (this manager's recorder)
LPS_API void lpslam_manager_recorder_counters(lpslam_c_manager* m, uint64_t* out) {
    LpSlam::SlamManager* impl = *reinterpret_cast<LpSlam::SlamManager**>(&m->mgr);
    const LpSlam::RecorderCounters c = impl ? impl->recorderCounters() : LpSlam::RecorderCounters{};
    out[0] = c.device_images; out[1] = c.host_images; out[2] = c.records; out[3] = c.bytes;
}
// test hook: out[3] = compressed images decoded on the device, decoded on the host, refused by both (this manager's replay and ingest)
LPS_API void lpslam_manager_decoder_counters(lpslam_c_manager* m, uint64_t* out) {
    LpSlam::SlamManager* impl = *reinterpret_cast<LpSlam::SlamManager**>(&m->mgr);
    const LpSlam::JpegDecodeCounters c = impl ? impl->decoderCounters() : LpSlam::JpegDecodeCounters{};
    out[0] = c.device_images; out[1] = c.host_images; out[2] = c.refused_images;
}
LPS_API size_t lpslam_manager_features_count(lpslam_c_manager* m) { return m->mgr.mappingGetFeaturesCount(LpSlamMapBoundary{}); }
LPS_API int lpslam_manager_mapping_set_mode(lpslam_c_manager* m, int enable) { return m->mgr.mappingSetMode(enable != 0) ? 1 : 0; }
LPS_API int lpslam_manager_mapping_set_filename(lpslam_c_manager* m, const char* f) { return m->mgr.mappingSetFilename(f ? f : "") ? 1 : 0; }
// the map database file (host/map_file.h) without a tracker: validate a file and report counts[5] = keyframe records, live keyframes,
// landmarks, next landmark id, stereo; 1 = valid, 0 = rejected with the reason in why (at most why_cap - 1 characters)
LPS_API int lpslam_map_file_info(const char* path, int64_t* counts, char* why, size_t why_cap) {
    LpSlam::MapData d; std::string err;
    const bool ok = path && LpSlam::read_map_file(path, d, &err);
    if (why && why_cap) { const size_t n = std::min(err.size(), why_cap - 1); memcpy(why, err.data(), n); why[n] = 0; }
    if (ok && counts) {
        counts[0] = (int64_t)d.kfs.size(); counts[1] = 0;
        for (const auto& k : d.kfs) counts[1] += k.erased ? 0 : 1;
        counts[2] = (int64_t)d.lms.size(); counts[3] = d.next_landmark_id; counts[4] = d.cam.stereo;
    }
    return ok ? 1 : 0;
}
// reads `in` and writes it back to `out` (a valid file comes back byte for byte); 1 = done
LPS_API int lpslam_map_file_rewrite(const char* in, const char* out, char* why, size_t why_cap) {
    LpSlam::MapData d; std::string err;
    const bool ok = in && out && LpSlam::read_map_file(in, d, &err) && LpSlam::write_map_file(out, d, &err);
    if (why && why_cap) { const size_t n = std::min(err.size(), why_cap - 1); memcpy(why, err.data(), n); why[n] = 0; }
    return ok ? 1 : 0;
}
// compares the camera record of a map file with a session's: session = {stereo, width, height, fx, fy, cx, cy, focal_x_baseline,
// num_levels, scale_factor, model (0 / 1 = fisheye / 2 = radial-tangential), k1 .. k4, max_angle in radians -- model 2: k1, k2, p1, p2, k3}.  1: they agree; 0: why = what differs, as the tracker
// logs it ("camera model", ...); -1: the file itself was rejected, why = the reader's reason
LPS_API int lpslam_map_file_camera_check(const char* path, const double* session, char* why, size_t why_cap) {
    LpSlam::MapData d; std::string err;
    int rc = -1;
    if (path && session && LpSlam::read_map_file(path, d, &err)) {
        LpSlam::MapFileCamera s;
        s.stereo = session[0] != 0 ? 1 : 0; s.width = (int32_t)session[1]; s.height = (int32_t)session[2];
        s.fx = session[3]; s.fy = session[4]; s.cx = session[5]; s.cy = session[6]; s.focal_x_baseline = session[7];
        s.num_levels = (int32_t)session[8]; s.scale_factor = session[9]; s.model = (uint32_t)session[10];
        if (s.model == LpSlam::kMapFileModelRadtan) std::copy(session + 11, session + 16, s.d);      // model 2: k1, k2, p1, p2, k3 in the same five places
        else { for (int i = 0; i < 4; ++i) s.k[i] = session[11 + i]; s.max_angle = session[15]; }
        err = LpSlam::map_camera_mismatch(d.cam, s);
        rc = err.empty() ? 1 : 0;
    }
    if (why && why_cap) { const size_t n = std::min(err.size(), why_cap - 1); memcpy(why, err.data(), n); why[n] = 0; }
    return rc;
}
// ---- the fisheye model's host forms (csrc/fisheye_math.h), for tests without a device; model = {fx, fy, cx, cy, k1 .. k4, max_angle} ----
static lpslam_fisheye::Model fisheye_model_of(const double* m) { return lpslam_fisheye::Model{m[0], m[1], m[2], m[3], {m[4], m[5], m[6], m[7]}, m[8]}; }
// n pixels (x, y as doubles) -> out (2 floats each, NaN where invalid), valid (bytes), theta (may be NULL: the angle the iteration ended at)
LPS_API void lpslam_fisheye_undistort(const double* model, const double* xy, size_t n, float* out, uint8_t* valid, double* theta) {
    const lpslam_fisheye::Model m = fisheye_model_of(model);
    for (size_t i = 0; i < n; ++i) {
        float ux = std::numeric_limits<float>::quiet_NaN(), uy = ux; double th = 0;
        valid[i] = lpslam_fisheye::undistort(m, xy[2 * i], xy[2 * i + 1], &ux, &uy, &th) ? 1 : 0;
        out[2 * i] = ux; out[2 * i + 1] = uy;
        if (theta) theta[i] = th;
    }
}
// n camera-frame points (X, Y, Z) -> the sensor pixel, the angle from the axis and the visibility rule of the tracker's projection
LPS_API void lpslam_fisheye_forward(const double* model, const double* xyz, size_t n, int width, int height, double* sensor_xy, double* theta, uint8_t* visible) {
    const lpslam_fisheye::Model m = fisheye_model_of(model);
    for (size_t i = 0; i < n; ++i) {
        lpslam_fisheye::forward(m, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &sensor_xy[2 * i], &sensor_xy[2 * i + 1], &theta[i]);
        visible[i] = lpslam_fisheye::visible(m, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], width, height) ? 1 : 0;
    }
}
// ---- the radial-tangential model's host forms (csrc/radtan_math.h), for tests without a device; model = {fx, fy, cx, cy, k1, k2, p1, p2, k3} ----
static lpslam_radtan::Model radtan_model_of(const double* m) { return lpslam_radtan::Model{m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8]}; }
// n pixels (x, y as doubles) -> out (2 floats each, NaN where invalid), valid (bytes); res2 and min_den (may be NULL): the squared
// residual in pixels and the smallest denominator of the five steps
LPS_API void lpslam_radtan_undistort(const double* model, const double* xy, size_t n, float* out, uint8_t* valid, double* res2, double* min_den) {
    const lpslam_radtan::Model m = radtan_model_of(model);
    for (size_t i = 0; i < n; ++i) {
        float ux = std::numeric_limits<float>::quiet_NaN(), uy = ux; double r = 0, d = 0;
        valid[i] = lpslam_radtan::undistort(m, xy[2 * i], xy[2 * i + 1], &ux, &uy, &r, &d) ? 1 : 0;
        out[2 * i] = ux; out[2 * i + 1] = uy;
        if (res2) res2[i] = r;
        if (min_den) min_den[i] = d;
    }
}
// the bounds of the undistorted width x height image: bounds = {min_x, max_x, min_y, max_y}; invalid_share (may be NULL): the share of
// border pixels without an undistorted position.  0: no border pixel is valid (a start with this model is refused)
LPS_API int lpslam_radtan_bounds(const double* model, int width, int height, double* bounds, double* invalid_share) {
    lpslam_radtan::Bounds b{};
    long bad = 0, all = 0;
    const bool ok = lpslam_radtan::bounds(radtan_model_of(model), width, height, &b, &bad, &all);
    if (invalid_share) *invalid_share = all > 0 ? (double)bad / (double)all : 0.0;
    if (ok) { bounds[0] = b.min_x; bounds[1] = b.max_x; bounds[2] = b.min_y; bounds[3] = b.max_y; }
    return ok ? 1 : 0;
}
// n camera-frame points (X, Y, Z) -> the sensor pixel and the visibility rule of the tracker's projection, given the bounds and the size
LPS_API void lpslam_radtan_forward(const double* model, const double* xyz, size_t n, const double* bounds, int width, int height, double* sensor_xy, uint8_t* visible) {
    const lpslam_radtan::Model m = radtan_model_of(model);
    const lpslam_radtan::Bounds b{bounds[0], bounds[1], bounds[2], bounds[3]};
    for (size_t i = 0; i < n; ++i) {
        lpslam_radtan::forward(m, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &sensor_xy[2 * i], &sensor_xy[2 * i + 1]);
        visible[i] = lpslam_radtan::visible(m, b, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], width, height) ? 1 : 0;
    }
}
// ---- the triangulation step's host forms (csrc/triangulate_math.h), for tests without a device; cam = {fx, fy, cx, cy, focal_x_baseline,
// scale_factor}, poses = qw qx qy qz tx ty tz, keypoints = lpslam_hip_tri_keypoint ----
static lpslam_tri::Camera tri_camera_of(const double* c) { return lpslam_tri::Camera{c[0], c[1], c[2], c[3], c[4], c[5]}; }
static_assert(sizeof(lpslam_hip_tri_keypoint) == sizeof(lpslam_tri::Keypoint), "keypoint layout");
// the candidate lists of n1 queries against one neighbour: keys[8 i + r] = distance << 32 | j (all ones: empty), count[i]
LPS_API void lpslam_tri_candidates_host(const double* cam, const float* scale, const lpslam_hip_tri_keypoint* kp1, const uint8_t* desc1, const int32_t* group1, int n1,
                                        const lpslam_hip_tri_keypoint* kp2, const uint8_t* desc2, const int32_t* group2, int n2, const double* F, const double* epipole,
                                        int has_epipole, unsigned long long* keys, int32_t* count) {
    lpslam_tri::Epipolar e{};
    std::copy(F, F + 9, e.F);
    e.has_epipole = has_epipole ? 1 : 0; e.ex = has_epipole ? epipole[0] : 0.0; e.ey = has_epipole ? epipole[1] : 0.0;
    lpslam_tri::candidates_host(reinterpret_cast<const lpslam_tri::Keypoint*>(kp1), desc1, group1, n1, reinterpret_cast<const lpslam_tri::Keypoint*>(kp2), desc2, group2, n2,
                                tri_camera_of(cam), e, scale, keys, count);
}
// tri_pair on n pairs: code[k], X[3 k ..] (NaN with code 0)
LPS_API void lpslam_tri_pair_host(const double* cam, const float* scale, const double* pose1, const double* pose2, const lpslam_hip_tri_keypoint* kp1,
                                  const lpslam_hip_tri_keypoint* kp2, int n, int32_t* code, double* X) {
    const lpslam_tri::Camera c = tri_camera_of(cam);
    const lpslam_tri::View v1 = lpslam_tri::view_from_pose(pose1), v2 = lpslam_tri::view_from_pose(pose2);
    for (int k = 0; k < n; ++k) {
        double x[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::quiet_NaN()};
        code[k] = lpslam_tri::tri_pair(c, scale, v1, v2, reinterpret_cast<const lpslam_tri::Keypoint*>(kp1)[k], reinterpret_cast<const lpslam_tri::Keypoint*>(kp2)[k], x);
        std::copy(x, x + 3, X + 3 * (size_t)k);
    }
}
// the ordered replay of one neighbour; returns the number of exhausted queries
LPS_API int lpslam_tri_replay_host(const unsigned long long* keys, const int32_t* count, int n1, int n2, const uint8_t* skip, int32_t* match, int32_t* rank) {
    int exhausted = 0;
    lpslam_tri::replay_host(keys, count, n1, n2, skip, match, rank, &exhausted);
    return exhausted;
}
// F (9, row major), the epipole (2) and whether it exists, as the tracker derives them from the two poses
LPS_API int lpslam_tri_epipolar(const double* cam, const double* pose_c, const double* pose_n, double* F, double* epipole) {
    const lpslam_tri::Epipolar e = lpslam_tri::epipolar_from_views(tri_camera_of(cam), lpslam_tri::view_from_pose(pose_c), lpslam_tri::view_from_pose(pose_n));
    std::copy(e.F, e.F + 9, F); epipole[0] = e.ex; epipole[1] = e.ey;
    return e.has_epipole;
}
// the neighbour gate and list of the tracker: the option's range; the covisible keyframes with the previous keyframe (prev >= 0) in front,
// cut to n (returns how many, out holds at most n); the camera-centre test; the median landmark depth
LPS_API int lpslam_tri_option_ok(int n) { return LpSlam::triangulateNeighboursOk(n) ? 1 : 0; }
LPS_API int lpslam_tri_neighbour_list(const int32_t* covisible, int n_covisible, int prev, int n, int32_t* out) {
    const std::vector<int> v = LpSlam::triangulationNeighbourList(std::vector<int>(covisible, covisible + n_covisible), prev, n);
    std::copy(v.begin(), v.end(), out);
    return (int)v.size();
}
LPS_API int lpslam_tri_baseline_accepts(const double* pose_c, const double* pose_n, double min_distance) {
    return lpslam_tri::baseline_accepts(lpslam_tri::view_from_pose(pose_c), lpslam_tri::view_from_pose(pose_n), min_distance) ? 1 : 0;
}
LPS_API double lpslam_tri_median_depth(const double* depths, int n) { return LpSlam::medianDepth(std::vector<double>(depths, depths + n)); }
// the keypoint camera a monocular tracker of this manager would start with: camera 0 of its registry (the configuration file's
// cameras[]), the YAML file of configFromFile (NULL or "": none) and fisheyeMaxAngleDeg.  1: model[9] filled; 0: not a fisheye camera;
// -1: refused (the start would fail), why says it
LPS_API int lpslam_manager_fisheye_session_model(lpslam_c_manager* m, const char* yaml_path, double max_angle_deg, double* model, char* why, size_t why_cap) {
    LpSlam::SlamManager* impl = *reinterpret_cast<LpSlam::SlamManager**>(&m->mgr);
    std::string err;
    int rc = -1;
    std::unordered_map<std::string, std::string> yaml;
    const auto cam = impl ? impl->cameraRegistry().getConfiguration((LpSlamCameraNumber)0) : std::nullopt;
    if (!cam) err = "no camera 0";
    else if (yaml_path && *yaml_path && !LpSlam::loadFlatYaml(yaml_path, yaml, &err)) { if (err.empty()) err = "cannot load the YAML file"; }
    else {
        lpslam_fisheye::Model fm{};
        rc = LpSlam::resolveFisheyeModel(*cam, yaml, max_angle_deg, &fm, &err);
        if (rc == 1) { const double v[9] = {fm.fx, fm.fy, fm.cx, fm.cy, fm.k[0], fm.k[1], fm.k[2], fm.k[3], fm.max_angle}; std::copy(v, v + 9, model); }
    }
    if (why && why_cap) { const size_t n = std::min(err.size(), why_cap - 1); memcpy(why, err.data(), n); why[n] = 0; }
    return rc;
}
// likewise the radial-tangential model a monocular tracker of this manager would start with (a camera that resolves as fisheye gets none:
// the two rules exclude each other).  1: model[9] filled; 0: no model; -1: refused, why says it
LPS_API int lpslam_manager_radtan_session_model(lpslam_c_manager* m, const char* yaml_path, double* model, char* why, size_t why_cap) {
    LpSlam::SlamManager* impl = *reinterpret_cast<LpSlam::SlamManager**>(&m->mgr);
    std::string err;
    int rc = -1;
    std::unordered_map<std::string, std::string> yaml;
    const auto cam = impl ? impl->cameraRegistry().getConfiguration((LpSlamCameraNumber)0) : std::nullopt;
    if (!cam) err = "no camera 0";
    else if (yaml_path && *yaml_path && !LpSlam::loadFlatYaml(yaml_path, yaml, &err)) { if (err.empty()) err = "cannot load the YAML file"; }
    else {
        lpslam_radtan::Model rm{};
        rc = LpSlam::resolveRadtanModel(*cam, yaml, &rm, &err);
        if (rc == 1) { const double v[9] = {rm.fx, rm.fy, rm.cx, rm.cy, rm.k1, rm.k2, rm.p1, rm.p2, rm.k3}; std::copy(v, v + 9, model); }
    }
    if (why && why_cap) { const size_t n = std::min(err.size(), why_cap - 1); memcpy(why, err.data(), n); why[n] = 0; }
    return rc;
}
// laser scans and the occupancy grid.  ros_ts: the scan's ROS time as the frames of lpslam_manager_add_stereo_image carry it.
LPS_API void lpslam_manager_add_laser_scan(lpslam_c_manager* m, const LpSlamROSTimestamp* ros_ts, float* ranges, size_t n, float range_min,
                                           float range_max, float angle_min, float angle_max, float increment, float range_threshold) {
    LpSlamGlobalStateInTime o{};
    if (ros_ts) { o.has_ros_timestamp = 1; o.ros_timestamp = *ros_ts; }
    o.state.orientation.w = 1.0;
    m->mgr.mappingAddLaserScan(o, ranges, n, range_min, range_max, angle_min, angle_max, increment, range_threshold);
}
// a compiled RequestNavTransformationCallback_t that answers Laser -> Camera with the given state (anything else: invalid)
static LpSlamRequestNavTransformation laser_transform(LpSlamROSTimestamp, LpSlamNavDataFrame from, LpSlamNavDataFrame to, void* p) {
    LpSlamRequestNavTransformation r{};
    if (from == LpSlamNavDataFrame_Laser && to == LpSlamNavDataFrame_Camera) r = static_cast<lpslam_c_manager*>(p)->laser_to_camera;
    return r;
}
LPS_API void lpslam_manager_provide_laser_transform(lpslam_c_manager* m, const LpSlamGlobalState* laser_to_camera) {
    m->laser_to_camera = *laser_to_camera;
    m->mgr.addRequestNavTransformation(laser_transform, m);
}
LPS_API unsigned long lpslam_manager_map_raw_size(lpslam_c_manager* m) { return m->mgr.mappingGetMapRawSize(); }
LPS_API void lpslam_manager_map_raw(lpslam_c_manager* m, int8_t* map, size_t capacity, LpMapInfo* info) { *info = m->mgr.mappingGetMapRaw(map, capacity); }
// test hook: the scans the grid is built from (one per keyframe with a scan): ROS time and the pose the grid uses (key, origin, fwd,
// left); returns their number, copies at most cap
LPS_API size_t lpslam_manager_map_scans(lpslam_c_manager* m, LpSlamROSTimestamp* stamps, lpslam_hip_scan_pose* poses, size_t cap) {
    LpSlam::SlamManager* impl = *reinterpret_cast<LpSlam::SlamManager**>(&m->mgr);
    const auto v = impl ? impl->occupancyScans() : std::vector<std::pair<LpSlamROSTimestamp, lpslam_hip_scan_pose>>();
    for (size_t i = 0; i < v.size() && i < cap; ++i) { stamps[i] = v[i].first; poses[i] = v[i].second; }
    return v.size();
}
// the scan pose of a keyframe (CPU): T_cw row-major 4x4 (optical axes) and the laser -> camera state; out = origin[2], fwd[2], left[2]
LPS_API void lpslam_occupancy_scan_pose(const double* T_cw, const LpSlamGlobalState* laser_to_camera, double* out) {
    const double R[9] = {T_cw[0], T_cw[1], T_cw[2], T_cw[4], T_cw[5], T_cw[6], T_cw[8], T_cw[9], T_cw[10]}, t[3] = {T_cw[3], T_cw[7], T_cw[11]};
    double Rcl[9], tcl[3];
    LpSlam::laserToCamera(*laser_to_camera, Rcl, tcl);
    LpSlam::scanPose(R, t, Rcl, tcl, out, out + 2, out + 4);
}
// interface.type_conversion of the reference's tests (src/test/InterfaceTest.cpp:14-33): POD -> internal -> POD
// the host implementation of the AdjustIntensity arithmetic (intensity.h), in place: params = {low_out, high_out, low_fraction,
// high_fraction} (NULL: the reference's constants); out_lo_hi (may be NULL) receives the limits.  0: invalid arguments, nothing written.
LPS_API int lpslam_adjust_intensity(uint8_t* pixels, int width, int height, size_t stride, const double* params, int* out_lo_hi) {
    LpSlam::IntensityAdjust p;
    if (params) { p.low_out = params[0]; p.high_out = params[1]; p.low_fraction = params[2]; p.high_fraction = params[3]; }
    return LpSlam::adjust_intensity_host(pixels, width, height, stride, p, out_lo_hi) ? 1 : 0;
}

// the host implementation of the colour / YUV -> grey conversion (ingest.h); format: LPSLAM_HIP_PIXEL_*.  0: invalid arguments, nothing written.
LPS_API int lpslam_gray_from_pixels(uint8_t* out, size_t out_stride, int width, int height, const uint8_t* data, size_t stride, const uint8_t* chroma,
                                    size_t chroma_stride, int format) {
    return LpSlam::gray_from_pixels_host(out, out_stride, width, height, data, stride, chroma, chroma_stride, format) ? 1 : 0;
}
// test hook: a camera-queue entry with one pending colour source (tightly packed, `format`) and, with params, a pending intensity
// adjustment, taken through realiseGray() and realiseAdjust() as the manager's worker does for a reader of host pixels; out: width *
// height grey bytes.  0: something stayed pending or the image has another size.
LPS_API int lpslam_realise_entry(const uint8_t* data, size_t bytes, size_t stride, int width, int height, int format, const double* params, uint8_t* out) {
    LpSlam::CameraQueueEntry e;
    e.valid = true; e.image.width = width; e.image.height = height;
    e.color.emplace();
    e.color->bytes.assign(data, data + bytes); e.color->format = format; e.color->stride = stride;
    if (params) { e.adjust.emplace(); e.adjust->low_out = params[0]; e.adjust->high_out = params[1]; e.adjust->low_fraction = params[2]; e.adjust->high_fraction = params[3]; }
    LpSlam::realiseGray(e);
    LpSlam::realiseAdjust(e);
    if (e.color || e.adjust || e.image.pixels.size() != (size_t)width * (size_t)height) return 0;
    std::memcpy(out, e.image.pixels.data(), e.image.pixels.size());
    return 1;
}

LPS_API void lpslam_roundtrip_state(const LpSlamGlobalStateInTime* in, LpSlamGlobalStateInTime* out) {
    *out = LpSlam::conversion::gsInTimeInternalToInterface(LpSlam::conversion::gsInTimeInterfaceToInternal(*in));
}
}
