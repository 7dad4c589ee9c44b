// ingest_math.h -- the grey value of a colour or YUV pixel, once, for the device kernel (ingest.hip) and the
// host function (lpslam_amd/host/ingest.cpp): integer arithmetic, the same bytes on either side.
//   RGB -> grey   cv::cvtColor's fixed-point weights: (R 4899 + G 9617 + B 1868 + 2^13) >> 14
//   YUV -> RGB    [UPSTREAM] OpenCV's BT.601 limited-range 8-bit path (color_yuv), written down from memory and not checked against
//                 OpenCV itself: y = max(0, Y - 16) 1220542, u = U - 128, v = V - 128, 20 fractional bits, arithmetic shift, saturated
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LP_INGEST_FN __host__ __device__ __forceinline__
#else
#define LP_INGEST_FN inline
#endif

namespace lpslam_ingest {

LP_INGEST_FN int grey_of_rgb(int r, int g, int b) { return (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14; }
LP_INGEST_FN int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// every sum stays inside int32: |y| <= 239 * 1220542, |2116026 u| <= 128 * 2116026, |852492 v + 409993 u| <= 128 * 1262485
LP_INGEST_FN int grey_of_yuv(int Y, int U, int V)
{
    const int y = (Y > 16 ? Y - 16 : 0) * 1220542, u = U - 128, v = V - 128;
    const int r = sat8((y + 1673527 * v + (1 << 19)) >> 20);
    const int g = sat8((y - 852492 * v - 409993 * u + (1 << 19)) >> 20);
    const int b = sat8((y + 2116026 * u + (1 << 19)) >> 20);
    return grey_of_rgb(r, g, b);
}

}  // namespace lpslam_ingest
