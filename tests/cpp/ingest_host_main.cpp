// ingest_host_main.cpp -- stand-alone sanitizer check of the host colour / YUV -> grey conversion (lpslam_amd/host/ingest.cpp) on the odd
// and minimal shapes: every buffer is a heap block of exactly the bytes the call may touch, so a read or write beyond them stops the run.
// Not part of the suite.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -o ingest_host_check tests/cpp/ingest_host_main.cpp lpslam_amd/host/ingest.cpp && ./ingest_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/lpslam_hip.h"
#include "../../lpslam_amd/host/ingest.h"

namespace LpSlam { void logMessage(LpSlamLogLevel, const std::string& msg) { std::fprintf(stderr, "%s\n", msg.c_str()); } }

static int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
static int grey_rgb(int r, int g, int b) { return (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14; }
static int grey_yuv(int Y, int U, int V)
{
    const int y = (Y > 16 ? Y - 16 : 0) * 1220542, u = U - 128, v = V - 128;
    return grey_rgb(sat8((y + 1673527 * v + (1 << 19)) >> 20), sat8((y - 852492 * v - 409993 * u + (1 << 19)) >> 20), sat8((y + 2116026 * u + (1 << 19)) >> 20));
}

static int check(int fmt, int w, int h, size_t extra)
{
    const size_t row = fmt == LPSLAM_HIP_PIXEL_NV12 ? (size_t)w : fmt == LPSLAM_HIP_PIXEL_UYVY ? 2 * (size_t)w : 3 * (size_t)w;
    const size_t stride = row + extra, rows = fmt == LPSLAM_HIP_PIXEL_NV12 ? (size_t)h + h / 2 : (size_t)h;
    std::vector<uint8_t> src(stride * (rows - 1) + row);      // the last row ends with its last pixel
    unsigned s = 12345u + (unsigned)(fmt * 7919 + w * 31 + h);
    for (auto& b : src) { s = s * 1664525u + 1013904223u; b = (uint8_t)(s >> 24); }
    const size_t ostride = (size_t)w + extra;
    std::vector<uint8_t> out(ostride * (size_t)(h - 1) + (size_t)w, 0xA5);
    if (!LpSlam::gray_from_pixels_host(out.data(), ostride, w, h, src.data(), stride, nullptr, 0, fmt)) { std::printf("format %d %d x %d: refused\n", fmt, w, h); return 1; }
    int bad = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int want;
            const uint8_t* p = src.data() + (size_t)y * stride;
            if (fmt == LPSLAM_HIP_PIXEL_RGB8) want = grey_rgb(p[3 * x], p[3 * x + 1], p[3 * x + 2]);
            else if (fmt == LPSLAM_HIP_PIXEL_BGR8) want = grey_rgb(p[3 * x + 2], p[3 * x + 1], p[3 * x]);
            else if (fmt == LPSLAM_HIP_PIXEL_UYVY) want = grey_yuv(p[2 * x + 1], p[4 * (x / 2)], p[4 * (x / 2) + 2]);
            else { const uint8_t* c = src.data() + ((size_t)h + y / 2) * stride; want = grey_yuv(p[x], c[x & ~1], c[(x & ~1) + 1]); }
            bad += out[(size_t)y * ostride + x] != want;
        }
    for (int y = 0; y + 1 < h; ++y) for (size_t k = (size_t)w; k < ostride; ++k) bad += out[(size_t)y * ostride + k] != 0xA5;
    // a pending source through realiseGray: tightly packed, as the manager stores it
    LpSlam::CameraQueueEntry e;
    e.image.width = w; e.image.height = h;
    e.color.emplace();
    e.color->format = fmt; e.color->stride = row; e.color->bytes.resize(row * rows);
    for (size_t r = 0; r < rows; ++r) std::copy(src.begin() + r * stride, src.begin() + r * stride + row, e.color->bytes.begin() + r * row);
    LpSlam::realiseGray(e);
    if (e.color || e.image.pixels.size() != (size_t)w * h) ++bad;
    else for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) bad += e.image.pixels[(size_t)y * w + x] != out[(size_t)y * ostride + x];
    if (bad) std::printf("format %d %d x %d stride +%zu: %d mismatches\n", fmt, w, h, extra, bad);
    return bad ? 1 : 0;
}

int main()
{
    int fails = 0, n = 0;
    const int rgb[][2] = {{1, 1}, {3, 2}, {65, 64}, {333, 77}, {64, 64}}, yuv[][2] = {{2, 2}, {66, 64}, {322, 64}, {64, 64}}, uyvy_odd_h[][2] = {{2, 1}, {322, 63}};
    for (size_t extra : {(size_t)0, (size_t)5}) {
        for (auto& s : rgb) for (int f : {LPSLAM_HIP_PIXEL_RGB8, LPSLAM_HIP_PIXEL_BGR8}) { fails += check(f, s[0], s[1], extra); ++n; }
        for (auto& s : yuv) for (int f : {LPSLAM_HIP_PIXEL_NV12, LPSLAM_HIP_PIXEL_UYVY}) { fails += check(f, s[0], s[1], extra); ++n; }
        for (auto& s : uyvy_odd_h) { fails += check(LPSLAM_HIP_PIXEL_UYVY, s[0], s[1], extra); ++n; }
    }
    std::printf("%d shapes, %d failed\n", n, fails);
    return fails ? 1 : 0;
}
