// map_file.h -- the map database of the trackers (useMapDb / mapFilename / mappingSetFilename): a versioned little-endian binary
// file of this project, documented field by field in INTEGRATION.md ("Map database file").  Pure host code: the tracker converts its
// map into MapData and back (hip_tracker.cpp); the C shim exposes validation and rewrite for tests (interface.cpp).
#pragma once
#include "../../include/lpslam_hip.h"

#include <cstdint>
#include <string>
#include <vector>

namespace LpSlam {

struct MapFileCamera {
    uint32_t stereo = 0;                              // 1: stereo, 0: monocular
    int32_t width = 0, height = 0;
    double fx = 0, fy = 0, cx = 0, cy = 0, focal_x_baseline = 0;
    int32_t num_levels = 0;
    double scale_factor = 0;
    // version 2 only (a monocular fisheye session): model = 1 (LpSlamCameraDistortionFunction_Fisheye), k1 .. k4, the angle limit in
    // radians.  model = 0: a version-1 record, which has none of the three.
    uint32_t model = 0;
    double k[4] = {0, 0, 0, 0}, max_angle = 0;
    // version 3 only (a monocular radial-tangential session): model = 2, then k1, k2, p1, p2, k3
    double d[5] = {0, 0, 0, 0, 0};
};

struct MapFileKeyframe {
    uint8_t erased = 0;                               // an erased keyframe is an empty record: the ids stay dense
    double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};     // world -> camera
    int32_t segment = 0;
    std::vector<lpslam_hip_keypoint> kpts;
    std::vector<uint8_t> desc;                        // 32 bytes per keypoint
    std::vector<float> x_right, depth;
    std::vector<int32_t> landmark;                    // landmark id per keypoint or -1
};

struct MapFileLandmark {
    int32_t id = 0;
    double p[3] = {0, 0, 0};
    uint8_t desc[32] = {0};
    double normal[3] = {0, 0, 1};
    double min_valid = 0, max_valid = 0;
    int32_t ref_kf = -1;
    int32_t n_observable = 1, n_observed = 1;
    std::vector<std::pair<int32_t, int32_t>> obs;     // (keyframe, keypoint)
};

struct MapData {
    MapFileCamera cam;
    int32_t next_landmark_id = 0, segment = 0;
    std::vector<MapFileKeyframe> kfs;
    std::vector<MapFileLandmark> lms;
};

constexpr uint32_t kMapFileVersion = 1;              // every session without a keypoint-camera model writes it, byte for byte as before
constexpr uint32_t kMapFileVersionFisheye = 2;       // version 1 with model, k[4], max_angle behind the camera record
constexpr uint32_t kMapFileModelFisheye = 1;
constexpr uint32_t kMapFileVersionRadtan = 3;        // version 1 with model, k1, k2, p1, p2, k3 behind the camera record
constexpr uint32_t kMapFileModelRadtan = 2;

// <path>.tmp, then rename: a crash never leaves half a map under the name.  false + *err on failure.
bool write_map_file(const std::string& path, const MapData& m, std::string* err);
// Checks magic, version, sizes, id ranges and the checksum; false + *err saying which check failed.
bool read_map_file(const std::string& path, MapData& m, std::string* err);
// What differs between the camera a file was made with and the session's ("camera setup", "resolution", "intrinsics",
// "focal_x_baseline", "numLevels / scaleFactor", "camera model"), or an empty string.  A version-1 file in a fisheye session, a
// version-2 file in any other, other coefficients or another angle limit: "camera model".  Likewise a version-1 or version-2 file in a
// radial-tangential session, a version-3 file in any other, other coefficients.
std::string map_camera_mismatch(const MapFileCamera& file, const MapFileCamera& session);

}  // namespace LpSlam
