// map_file.cpp -- reader and writer of the map database file (map_file.h; layout in INTEGRATION.md).
#include "map_file.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <unordered_set>

namespace LpSlam {

namespace {

const char kMagic[8] = {'L', 'P', 'S', 'L', 'M', 'A', 'P', '\0'};

uint64_t fnv1a64(const uint8_t* p, size_t n)      // FNV-1a, 64 bit
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

struct Out {
    std::vector<uint8_t> b;
    void raw(const void* p, size_t n) { const uint8_t* s = (const uint8_t*)p; b.insert(b.end(), s, s + n); }
    template <class T> void v(T x) { raw(&x, sizeof(T)); }      // (little-endian hosts only: static_assert below)
};

struct In {
    const uint8_t* p; size_t n, at = 0;
    bool raw(void* d, size_t k) { if (k > n - at) return false; std::memcpy(d, p + at, k); at += k; return true; }
    template <class T> bool v(T& x) { return raw(&x, sizeof(T)); }
    size_t left() const { return n - at; }
};

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the map file is little-endian and written as the host stores it");
static_assert(sizeof(lpslam_hip_keypoint) == 28, "keypoint record: 5 float + 2 int32");

}  // namespace

bool write_map_file(const std::string& path, const MapData& m, std::string* err)
{
    Out o;
    o.raw(kMagic, 8);
    const bool fisheye = m.cam.model == kMapFileModelFisheye, radtan = m.cam.model == kMapFileModelRadtan;
    if (m.cam.model != 0 && !fisheye && !radtan) { if (err) *err = "camera model " + std::to_string(m.cam.model) + " cannot be written"; return false; }
    o.v<uint32_t>(fisheye ? kMapFileVersionFisheye : radtan ? kMapFileVersionRadtan : kMapFileVersion);
    o.v<uint32_t>(m.cam.stereo); o.v<int32_t>(m.cam.width); o.v<int32_t>(m.cam.height);
    o.v<double>(m.cam.fx); o.v<double>(m.cam.fy); o.v<double>(m.cam.cx); o.v<double>(m.cam.cy); o.v<double>(m.cam.focal_x_baseline);
    o.v<int32_t>(m.cam.num_levels); o.v<double>(m.cam.scale_factor);
    if (fisheye) { o.v<uint32_t>(m.cam.model); for (double x : m.cam.k) o.v<double>(x); o.v<double>(m.cam.max_angle); }
    if (radtan) { o.v<uint32_t>(m.cam.model); for (double x : m.cam.d) o.v<double>(x); }
    o.v<uint32_t>((uint32_t)m.kfs.size()); o.v<uint32_t>((uint32_t)m.lms.size()); o.v<int32_t>(m.next_landmark_id); o.v<int32_t>(m.segment);
    for (const auto& k : m.kfs) {
        o.v<uint8_t>(k.erased ? 1 : 0);
        if (k.erased) continue;
        for (double x : k.q) o.v<double>(x);
        for (double x : k.t) o.v<double>(x);
        o.v<int32_t>(k.segment);
        const uint32_t n = (uint32_t)k.kpts.size();
        o.v<uint32_t>(n);
        o.raw(k.kpts.data(), (size_t)n * sizeof(lpslam_hip_keypoint));
        o.raw(k.desc.data(), (size_t)n * 32);
        o.raw(k.x_right.data(), (size_t)n * 4);
        o.raw(k.depth.data(), (size_t)n * 4);
        o.raw(k.landmark.data(), (size_t)n * 4);
    }
    for (const auto& l : m.lms) {
        o.v<int32_t>(l.id);
        for (double x : l.p) o.v<double>(x);
        o.raw(l.desc, 32);
        for (double x : l.normal) o.v<double>(x);
        o.v<double>(l.min_valid); o.v<double>(l.max_valid);
        o.v<int32_t>(l.ref_kf); o.v<int32_t>(l.n_observable); o.v<int32_t>(l.n_observed);
        o.v<uint32_t>((uint32_t)l.obs.size());
        for (const auto& ob : l.obs) { o.v<int32_t>(ob.first); o.v<int32_t>(ob.second); }
    }
    o.v<uint64_t>(fnv1a64(o.b.data(), o.b.size()));
    const std::string tmp = path + ".tmp";
    {
        std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
        if (!f) { if (err) *err = "cannot open " + tmp + " for writing"; return false; }
        f.write((const char*)o.b.data(), (std::streamsize)o.b.size());
        f.flush();
        if (!f) { if (err) *err = "cannot write " + tmp; std::remove(tmp.c_str()); return false; }
    }
    if (std::rename(tmp.c_str(), path.c_str()) != 0) { if (err) *err = "cannot rename " + tmp + " to " + path; std::remove(tmp.c_str()); return false; }
    return true;
}

bool read_map_file(const std::string& path, MapData& m, std::string* err)
{
    auto fail = [err](const std::string& why) { if (err) *err = why; return false; };
    std::ifstream f(path, std::ios::binary);
    if (!f) return fail("cannot open " + path);
    const std::vector<uint8_t> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    char magic[8];
    if (b.size() < 8) return fail("truncated: no header");
    std::memcpy(magic, b.data(), 8);
    if (std::memcmp(magic, kMagic, 8) != 0) return fail("bad magic: not a map file of this project");
    uint32_t version = 0;
    if (b.size() < 12) return fail("truncated: no version");
    std::memcpy(&version, b.data() + 8, 4);
    if (version != kMapFileVersion && version != kMapFileVersionFisheye && version != kMapFileVersionRadtan)
        return fail("unsupported format version " + std::to_string(version) + " (this build reads " + std::to_string(kMapFileVersion) + ", " + std::to_string(kMapFileVersionFisheye) + " and " + std::to_string(kMapFileVersionRadtan) + ")");
    if (b.size() < 20) return fail("truncated: no checksum");
    // the records first (a file cut short runs out of bytes: "truncated"), the checksum over all of it last
    In in{b.data(), b.size() - 8, 12};
    m = MapData{};
    uint32_t nk = 0, nl = 0;
    bool ok = in.v(m.cam.stereo) && in.v(m.cam.width) && in.v(m.cam.height) && in.v(m.cam.fx) && in.v(m.cam.fy) && in.v(m.cam.cx) && in.v(m.cam.cy) &&
              in.v(m.cam.focal_x_baseline) && in.v(m.cam.num_levels) && in.v(m.cam.scale_factor);
    if (ok && version == kMapFileVersionFisheye) {
        ok = in.v(m.cam.model);
        // version 2 exists for the fisheye model alone: any other value is a format this build does not know
        if (ok && m.cam.model != kMapFileModelFisheye)
            return fail("unsupported format version 2 with camera model " + std::to_string(m.cam.model) + " (this build reads model " + std::to_string(kMapFileModelFisheye) + ", fisheye)");
        ok = ok && in.raw(m.cam.k, sizeof(m.cam.k)) && in.v(m.cam.max_angle);
    }
    if (ok && version == kMapFileVersionRadtan) {
        ok = in.v(m.cam.model);
        // version 3 exists for the radial-tangential model alone
        if (ok && m.cam.model != kMapFileModelRadtan)
            return fail("unsupported format version 3 with camera model " + std::to_string(m.cam.model) + " (this build reads model " + std::to_string(kMapFileModelRadtan) + ", radial-tangential)");
        ok = ok && in.raw(m.cam.d, sizeof(m.cam.d));
    }
    ok = ok && in.v(nk) && in.v(nl) && in.v(m.next_landmark_id) && in.v(m.segment);
    if (!ok) return fail("truncated: header");
    if (m.next_landmark_id < 0 || nl > (uint32_t)m.next_landmark_id) return fail("landmark count " + std::to_string(nl) + " exceeds next landmark id " + std::to_string(m.next_landmark_id));
    if ((size_t)nk > in.left()) return fail("keyframe count " + std::to_string(nk) + " exceeds the file size");
    m.kfs.resize(nk);
    for (uint32_t k = 0; k < nk; ++k) {
        MapFileKeyframe& kf = m.kfs[k];
        if (!in.v(kf.erased)) return fail("truncated: keyframe " + std::to_string(k));
        if (kf.erased > 1) return fail("keyframe " + std::to_string(k) + ": bad erased flag");
        if (kf.erased) continue;
        uint32_t n = 0;
        ok = in.raw(kf.q, sizeof(kf.q)) && in.raw(kf.t, sizeof(kf.t)) && in.v(kf.segment) && in.v(n);
        if (!ok) return fail("truncated: keyframe " + std::to_string(k));
        if ((size_t)n * (sizeof(lpslam_hip_keypoint) + 32 + 12) > in.left()) return fail("keyframe " + std::to_string(k) + ": keypoint count " + std::to_string(n) + " exceeds the file size");
        kf.kpts.resize(n); kf.desc.resize((size_t)n * 32); kf.x_right.resize(n); kf.depth.resize(n); kf.landmark.resize(n);
        in.raw(kf.kpts.data(), (size_t)n * sizeof(lpslam_hip_keypoint)); in.raw(kf.desc.data(), (size_t)n * 32);
        in.raw(kf.x_right.data(), (size_t)n * 4); in.raw(kf.depth.data(), (size_t)n * 4); in.raw(kf.landmark.data(), (size_t)n * 4);
        for (uint32_t i = 0; i < n; ++i)
            if (kf.landmark[i] < -1 || kf.landmark[i] >= m.next_landmark_id) return fail("keyframe " + std::to_string(k) + ": landmark id " + std::to_string(kf.landmark[i]) + " out of range");
    }
    if ((size_t)nl > in.left()) return fail("landmark count " + std::to_string(nl) + " exceeds the file size");
    m.lms.resize(nl);
    std::unordered_set<int32_t> seen;
    for (uint32_t j = 0; j < nl; ++j) {
        MapFileLandmark& l = m.lms[j];
        uint32_t no = 0;
        ok = in.v(l.id) && in.raw(l.p, sizeof(l.p)) && in.raw(l.desc, 32) && in.raw(l.normal, sizeof(l.normal)) && in.v(l.min_valid) && in.v(l.max_valid) &&
             in.v(l.ref_kf) && in.v(l.n_observable) && in.v(l.n_observed) && in.v(no);
        if (!ok) return fail("truncated: landmark record " + std::to_string(j));
        if (l.id < 0 || l.id >= m.next_landmark_id) return fail("landmark id " + std::to_string(l.id) + " out of range");
        if (!seen.insert(l.id).second) return fail("landmark id " + std::to_string(l.id) + " stored twice");
        if (l.ref_kf < -1 || l.ref_kf >= (int32_t)nk) return fail("landmark " + std::to_string(l.id) + ": reference keyframe out of range");
        if ((size_t)no * 8 > in.left()) return fail("landmark " + std::to_string(l.id) + ": observation count exceeds the file size");
        l.obs.resize(no);
        for (uint32_t o = 0; o < no; ++o) {
            int32_t kk = 0, kp = 0;
            in.v(kk); in.v(kp);
            if (kk < 0 || kk >= (int32_t)nk || m.kfs[(size_t)kk].erased || kp < 0 || (size_t)kp >= m.kfs[(size_t)kk].kpts.size())
                return fail("landmark " + std::to_string(l.id) + ": observation (" + std::to_string(kk) + ", " + std::to_string(kp) + ") out of range");
            l.obs[o] = {kk, kp};
        }
    }
    if (in.left() != 0) return fail("trailing bytes after the landmark records");
    uint64_t stored = 0;
    std::memcpy(&stored, b.data() + b.size() - 8, 8);
    if (fnv1a64(b.data(), b.size() - 8) != stored) return fail("checksum mismatch: the file is damaged");
    return true;
}

static bool close_to(double a, double b) { return std::fabs(a - b) <= 1e-6 * std::max(1.0, std::max(std::fabs(a), std::fabs(b))); }

std::string map_camera_mismatch(const MapFileCamera& c, const MapFileCamera& s)
{
    if ((c.stereo != 0) != (s.stereo != 0)) return "camera setup";
    if (c.width != s.width || c.height != s.height) return "resolution";
    if (!close_to(c.fx, s.fx) || !close_to(c.fy, s.fy) || !close_to(c.cx, s.cx) || !close_to(c.cy, s.cy)) return "intrinsics";
    if (s.stereo && !close_to(c.focal_x_baseline, s.focal_x_baseline)) return "focal_x_baseline";
    if (c.num_levels != s.num_levels || !close_to(c.scale_factor, s.scale_factor)) return "numLevels / scaleFactor";
    if (c.model != s.model) return "camera model";
    for (int i = 0; i < 5; ++i) if (!close_to(c.d[i], s.d[i])) return "camera model";      // (all zero but in a radial-tangential record)
    if (c.model != 0 && !(close_to(c.k[0], s.k[0]) && close_to(c.k[1], s.k[1]) && close_to(c.k[2], s.k[2]) && close_to(c.k[3], s.k[3]) && close_to(c.max_angle, s.max_angle))) return "camera model";
    return std::string();
}

}  // namespace LpSlam
