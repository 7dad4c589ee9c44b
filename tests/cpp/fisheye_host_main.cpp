// fisheye_host_main.cpp -- stand-alone sanitizer check of the fisheye model's host forms (lpslam_amd/csrc/fisheye_math.h) and of the
// map-file reader with the version-2 camera record (lpslam_amd/host/map_file.cpp).  tests/test_fisheye_cpu.py writes the cases, builds
// this with -fsanitize=address,undefined and runs it; by hand, from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -o fisheye_host_check tests/cpp/fisheye_host_main.cpp lpslam_amd/host/map_file.cpp
//   ./fisheye_host_check cases.txt version1.lpsmap version2.lpsmap cut.lpsmap
// cases.txt: n, the nine numbers of the model, then n lines "x y valid bits(ux) bits(uy)" (the float32 results as int32 bit patterns).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../lpslam_amd/csrc/fisheye_math.h"
#include "../../lpslam_amd/host/map_file.h"

static long ulps(float a, int32_t want_bits)
{
    int32_t ia; std::memcpy(&ia, &a, 4);
    return std::labs((long)ia - (long)want_bits);      // (valid results here are positive or share their sign: same-sign bit patterns are ordered)
}

int main(int argc, char** argv)
{
    if (argc != 5) { std::printf("usage: %s cases.txt version1.lpsmap version2.lpsmap cut.lpsmap\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int n = 0; double v[9];
    if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 2;
    for (double& d : v) if (std::fscanf(f, "%lf", &d) != 1) return 2;
    const lpslam_fisheye::Model m{v[0], v[1], v[2], v[3], {v[4], v[5], v[6], v[7]}, v[8]};
    if (!lpslam_fisheye::model_ok(m)) { std::printf("model refused\n"); return 1; }
    int bad = 0;
    // heap blocks of exactly one result each: a write past them stops the run
    for (int i = 0; i < n; ++i) {
        double x, y; int valid; int bx, by;
        if (std::fscanf(f, "%lf %lf %d %d %d", &x, &y, &valid, &bx, &by) != 5) { std::printf("case %d: cannot parse\n", i); return 2; }
        std::vector<float> out(2, -1.0f);
        double theta = 0;
        const bool ok = lpslam_fisheye::undistort(m, x, y, &out[0], &out[1], &theta);
        if (ok != (valid != 0)) { std::printf("case %d (%.17g, %.17g): valid %d, expected %d\n", i, x, y, (int)ok, valid); ++bad; continue; }
        if (!ok) { if (out[0] != -1.0f || out[1] != -1.0f) { std::printf("case %d: an invalid point was written\n", i); ++bad; } continue; }
        if (ulps(out[0], bx) > 1 || ulps(out[1], by) > 1) { std::printf("case %d: (%.9g, %.9g) is more than 1 ulp from the reference\n", i, out[0], out[1]); ++bad; }
        // forward of the undistorted ray comes back to the pixel (Newton's 1e-8 rad and the float32 rounding of the position, see the Python test)
        double sx, sy, th;
        lpslam_fisheye::forward(m, ((double)out[0] - m.cx) / m.fx, ((double)out[1] - m.cy) / m.fy, 1.0, &sx, &sy, &th);
        if (std::fabs(sx - x) > 1e-3 || std::fabs(sy - y) > 1e-3 || std::fabs(th - theta) > 1e-6) { std::printf("case %d: forward gives (%.9g, %.9g), pixel (%.9g, %.9g)\n", i, sx, sy, x, y); ++bad; }
        if (!lpslam_fisheye::visible(m, ((double)out[0] - m.cx) / m.fx, ((double)out[1] - m.cy) / m.fy, 1.0, 1 << 20, 1 << 20) && x >= 0 && y >= 0 && th < m.max_angle - 1e-6) { std::printf("case %d: not visible\n", i); ++bad; }
    }
    std::fclose(f);
    lpslam_fisheye::Model refused = m; refused.max_angle = 1.56;
    if (lpslam_fisheye::model_ok(refused)) { std::printf("an angle limit beyond 89 degrees was accepted\n"); ++bad; }
    if (lpslam_fisheye::visible(m, 0.1, 0.1, -1.0, 100, 100)) { std::printf("a point behind the camera is visible\n"); ++bad; }
    if (bad) { std::printf("points: %d failed\n", bad); return 1; }
    std::printf("points ok %d\n", n);

    LpSlam::MapData d1, d2, d3; std::string err;
    if (!LpSlam::read_map_file(argv[2], d1, &err)) { std::printf("version-1 file rejected: %s\n", err.c_str()); return 1; }
    if (!LpSlam::read_map_file(argv[3], d2, &err)) { std::printf("version-2 file rejected: %s\n", err.c_str()); return 1; }
    if (d1.cam.model != 0 || d2.cam.model != LpSlam::kMapFileModelFisheye || !(d2.cam.max_angle > 0) || d2.kfs.size() != d1.kfs.size() || d2.lms.size() != d1.lms.size()) { std::printf("camera records or counts are wrong\n"); return 1; }
    if (LpSlam::map_camera_mismatch(d2.cam, d2.cam) != "" || LpSlam::map_camera_mismatch(d1.cam, d1.cam) != "") { std::printf("a record differs from itself\n"); return 1; }
    LpSlam::MapFileCamera as_v2 = d1.cam; as_v2.model = d2.cam.model; std::memcpy(as_v2.k, d2.cam.k, sizeof(as_v2.k)); as_v2.max_angle = d2.cam.max_angle;
    if (LpSlam::map_camera_mismatch(d1.cam, as_v2) != "camera model") { std::printf("a version-1 file passed in a fisheye session\n"); return 1; }
    if (LpSlam::read_map_file(argv[4], d3, &err) || err.find("truncated") == std::string::npos) { std::printf("the cut file: %s\n", err.c_str()); return 1; }
    // every prefix of the version-2 file is rejected without reading past its bytes
    std::vector<unsigned char> whole;
    { std::FILE* g = std::fopen(argv[3], "rb"); int ch; while (g && (ch = std::fgetc(g)) != EOF) whole.push_back((unsigned char)ch); if (g) std::fclose(g); }
    const std::string tmp = std::string(argv[4]) + ".prefix";
    for (size_t len = 0; len < whole.size(); len += (len < 160 ? 1 : 97)) {
        std::FILE* g = std::fopen(tmp.c_str(), "wb");
        if (!g) return 2;
        if (len) std::fwrite(whole.data(), 1, len, g);
        std::fclose(g);
        LpSlam::MapData dp;
        if (LpSlam::read_map_file(tmp, dp, &err)) { std::printf("a prefix of %zu bytes was accepted\n", len); return 1; }
    }
    std::remove(tmp.c_str());
    std::printf("maps ok\n");
    return 0;
}
