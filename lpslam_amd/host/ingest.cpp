// ingest.cpp -- see ingest.h.
#include "ingest.h"

#include <algorithm>

#include "../../include/lpslam_hip.h"
#include "../csrc/ingest_math.h"

namespace LpSlam {

bool gray_from_pixels_host(uint8_t* out, size_t out_stride, int width, int height, const uint8_t* data, size_t stride,
                           const uint8_t* chroma, size_t chroma_stride, int format)
{
    using namespace lpslam_ingest;
    if (!out || !data || width < 1 || height < 1 || out_stride < (size_t)width) return false;
    const size_t w = (size_t)width;
    switch (format) {
    case LPSLAM_HIP_PIXEL_GRAY8:
        if (stride < w) return false;
        for (int y = 0; y < height; ++y) std::copy(data + (size_t)y * stride, data + (size_t)y * stride + w, out + (size_t)y * out_stride);
        return true;
    case LPSLAM_HIP_PIXEL_RGB8: case LPSLAM_HIP_PIXEL_BGR8: {
        if (stride < 3 * w) return false;
        const int ir = format == LPSLAM_HIP_PIXEL_BGR8 ? 2 : 0, ib = 2 - ir;
        for (int y = 0; y < height; ++y) {
            const uint8_t* p = data + (size_t)y * stride;
            uint8_t* q = out + (size_t)y * out_stride;
            for (size_t x = 0; x < w; ++x) q[x] = (uint8_t)grey_of_rgb(p[3 * x + ir], p[3 * x + 1], p[3 * x + ib]);
        }
        return true;
    }
    case LPSLAM_HIP_PIXEL_NV12: {
        if (((width | height) & 1) || stride < w || (chroma && chroma_stride < w)) return false;
        const uint8_t* uv = chroma ? chroma : data + stride * (size_t)height;
        const size_t uvs = chroma ? chroma_stride : stride;
        for (int y = 0; y < height; ++y) {
            const uint8_t* p = data + (size_t)y * stride;
            const uint8_t* c = uv + (size_t)(y >> 1) * uvs;
            uint8_t* q = out + (size_t)y * out_stride;
            for (size_t x = 0; x < w; ++x) q[x] = (uint8_t)grey_of_yuv(p[x], c[x & ~(size_t)1], c[(x & ~(size_t)1) + 1]);
        }
        return true;
    }
    case LPSLAM_HIP_PIXEL_UYVY:
        if ((width & 1) || stride < 2 * w) return false;
        for (int y = 0; y < height; ++y) {
            const uint8_t* p = data + (size_t)y * stride;
            uint8_t* q = out + (size_t)y * out_stride;
            for (size_t x = 0; x < w; ++x) { const uint8_t* pair = p + 4 * (x >> 1); q[x] = (uint8_t)grey_of_yuv(pair[1 + 2 * (x & 1)], pair[0], pair[2]); }
        }
        return true;
    default: return false;
    }
}

static void realise_eye(GrayImage& img, std::optional<ColorSource>& col)
{
    if (!col) return;
    const ColorSource src = std::move(*col);
    col.reset();
    img.pixels.resize((size_t)img.width * (size_t)img.height);
    if (!gray_from_pixels_host(img.pixels.data(), (size_t)img.width, img.width, img.height, src.bytes.data(), src.stride, nullptr, 0, src.format)) {
        logMessage(LpSlamLogLevel_Error, "Colour frame of " + std::to_string(img.width) + " x " + std::to_string(img.height) + " pixels not converted");
        std::fill(img.pixels.begin(), img.pixels.end(), (uint8_t)0);
    }
}

void realiseGray(CameraQueueEntry& cam)
{
    realise_eye(cam.image, cam.color);
    if (cam.image_second) realise_eye(*cam.image_second, cam.color_second);
}

}  // namespace LpSlam
