// radtan_host_main.cpp -- stand-alone sanitizer check of the radial-tangential model's host forms (lpslam_amd/csrc/radtan_math.h) and of
// the map-file reader with the version-3 camera record (lpslam_amd/host/map_file.cpp).  tests/test_radtan_cpu.py writes the cases, builds
// this with -fsanitize=address,undefined and runs it; by hand, from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -o radtan_host_check tests/cpp/radtan_host_main.cpp lpslam_amd/host/map_file.cpp
//   ./radtan_host_check cases.txt version1.lpsmap version3.lpsmap cut.lpsmap
// cases.txt: n, width, height, the nine numbers of the model, then n lines "x y valid bits(ux) bits(uy)" (the float32 results as int32
// bit patterns).  Prints one line "point i valid bits bits" per case for the test to compare, then its own verdicts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../lpslam_amd/csrc/radtan_math.h"
#include "../../lpslam_amd/host/map_file.h"

static int32_t bits(float a) { int32_t i; std::memcpy(&i, &a, 4); return i; }
static long ulps(float a, int32_t want_bits)
{
    auto ordered = [](int32_t i) { return i < 0 ? -(long)(i & 0x7fffffff) : (long)i; };
    return std::labs(ordered(bits(a)) - ordered(want_bits));
}

int main(int argc, char** argv)
{
    if (argc != 5) { std::printf("usage: %s cases.txt version1.lpsmap version3.lpsmap cut.lpsmap\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int n = 0, width = 0, height = 0; double v[9];
    if (std::fscanf(f, "%d %d %d", &n, &width, &height) != 3 || n < 0) return 2;
    for (double& d : v) if (std::fscanf(f, "%lf", &d) != 1) return 2;
    const lpslam_radtan::Model m{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
    if (!lpslam_radtan::model_ok(m) || lpslam_radtan::is_identity(m)) { std::printf("model refused\n"); return 1; }
    int bad = 0;
    // heap blocks of exactly one result each: a write past them stops the run
    for (int i = 0; i < n; ++i) {
        double x, y; int valid; int bx, by;
        if (std::fscanf(f, "%lf %lf %d %d %d", &x, &y, &valid, &bx, &by) != 5) { std::printf("case %d: cannot parse\n", i); return 2; }
        std::vector<float> out(2, -1.0f);
        std::vector<double> extra(2, 0.0);
        const bool ok = lpslam_radtan::undistort(m, x, y, &out[0], &out[1], &extra[0], &extra[1]);
        std::printf("point %d %d %d %d\n", i, (int)ok, ok ? bits(out[0]) : 0, ok ? bits(out[1]) : 0);
        if (ok != (valid != 0)) { std::printf("case %d (%.17g, %.17g): valid %d, expected %d\n", i, x, y, (int)ok, valid); ++bad; continue; }
        if (!ok) { if (out[0] != -1.0f || out[1] != -1.0f) { std::printf("case %d: an invalid point was written\n", i); ++bad; } continue; }
        if (ulps(out[0], bx) > 1 || ulps(out[1], by) > 1) { std::printf("case %d: (%.9g, %.9g) is more than 1 ulp from the reference\n", i, out[0], out[1]); ++bad; }
        // the validity rule itself: forward of the result lies within half a pixel (plus the float32 rounding of the position)
        double sx, sy;
        lpslam_radtan::forward(m, ((double)out[0] - m.cx) / m.fx, ((double)out[1] - m.cy) / m.fy, 1.0, &sx, &sy);
        if (!(std::hypot(sx - x, sy - y) <= 0.5 + 1e-3) || !(extra[0] <= lpslam_radtan::kMaxResidual2) || !(extra[1] > 0.0)) { std::printf("case %d: forward gives (%.9g, %.9g), pixel (%.9g, %.9g)\n", i, sx, sy, x, y); ++bad; }
    }
    std::fclose(f);
    lpslam_radtan::Bounds b{};
    long n_bad = 0, n_all = 0;
    const bool has_bounds = lpslam_radtan::bounds(m, width, height, &b, &n_bad, &n_all);
    std::printf("bounds %d %.17g %.17g %.17g %.17g %ld %ld\n", (int)has_bounds, b.min_x, b.max_x, b.min_y, b.max_y, n_bad, n_all);
    if (n_all != 2L * width + 2L * (height - 2)) { std::printf("border pixel count %ld\n", n_all); ++bad; }
    if (has_bounds && lpslam_radtan::visible(m, b, 0.1, 0.1, -1.0, width, height)) { std::printf("a point behind the camera is visible\n"); ++bad; }
    if (has_bounds && !lpslam_radtan::visible(m, b, 0.0, 0.0, 1.0, width, height)) { std::printf("the axis is not visible\n"); ++bad; }
    lpslam_radtan::Model refused = m; refused.fx = 0.0;
    if (lpslam_radtan::model_ok(refused)) { std::printf("fx = 0 was accepted\n"); ++bad; }
    refused = m; refused.k2 = NAN;
    if (lpslam_radtan::model_ok(refused)) { std::printf("a NaN coefficient was accepted\n"); ++bad; }
    if (bad) { std::printf("points: %d failed\n", bad); return 1; }
    std::printf("points ok %d\n", n);

    LpSlam::MapData d1, d3, dc; std::string err;
    if (!LpSlam::read_map_file(argv[2], d1, &err)) { std::printf("version-1 file rejected: %s\n", err.c_str()); return 1; }
    if (!LpSlam::read_map_file(argv[3], d3, &err)) { std::printf("version-3 file rejected: %s\n", err.c_str()); return 1; }
    if (d1.cam.model != 0 || d3.cam.model != LpSlam::kMapFileModelRadtan || d3.cam.d[0] == 0.0 || d3.kfs.size() != d1.kfs.size() || d3.lms.size() != d1.lms.size()) { std::printf("camera records or counts are wrong\n"); return 1; }
    if (LpSlam::map_camera_mismatch(d3.cam, d3.cam) != "" || LpSlam::map_camera_mismatch(d1.cam, d1.cam) != "") { std::printf("a record differs from itself\n"); return 1; }
    LpSlam::MapFileCamera as_v3 = d1.cam; as_v3.model = d3.cam.model; std::memcpy(as_v3.d, d3.cam.d, sizeof(as_v3.d));
    if (LpSlam::map_camera_mismatch(d1.cam, as_v3) != "camera model") { std::printf("a version-1 file passed in a radial-tangential session\n"); return 1; }
    if (LpSlam::read_map_file(argv[4], dc, &err) || err.find("truncated") == std::string::npos) { std::printf("the cut file: %s\n", err.c_str()); return 1; }
    // every prefix of the version-3 file is rejected without reading past its bytes
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
