// ingest.hip -- colour and YUV frames at ingest: the grey conversion on the device, one pointwise kernel from the staged frame in HBM into
// a pitched 8-bit destination -- level 0 of an image slot, or the raw-frame block in front of the remap (gfx950).
//
// Replaces the cv::cvtColor calls of the reference's ingest (src/Manager/SlamManager.cpp:1051-1063 for 8UC3, :1190-1260 for NV12 and
// YUV16), which run on the caller's thread.  The arithmetic is ingest_math.h's, the same functions the host
// implementation (lpslam_amd/host/ingest.cpp) is compiled from.
//
// k_ingest: a lane produces four neighbouring output pixels and stores them as one dword (blockIdx.y = image: both eyes of a frame in
// one launch).  What it reads for them:
//   RGB8 / BGR8   three dwords (12 bytes)
//   UYVY          two dwords (U0 Y0 V0 Y1  U1 Y2 V1 Y3)
//   NV12          TWO rows per lane: a dword of each Y row and the one chroma dword (U0 V0 U1 V1) both rows share, read once
// The last group of a row whose width is no multiple of four goes pixel by pixel, so neither a byte behind a source row is read nor a
// byte of the destination's row padding written.  Rows whose base or stride is not dword aligned (a raw-frame block of odd width) move
// byte by byte as well.  The kernel is bandwidth bound: 3 bytes in, 1 byte out per pixel for RGB.
#include "internal.h"
#include "ingest_math.h"

using namespace lpslam;
using namespace lpslam_ingest;

namespace {

struct IngImage { const uint8_t* src; uint8_t* dst; int fmt; };
// src_stride: bytes between the staged rows (NV12: of both planes; its chroma rows start at src + chroma_off)
struct IngArgs { IngImage img[2]; int w, h, dst_pitch, dst_vec; int src_stride[2]; unsigned chroma_off[2]; };

__device__ __forceinline__ uint32_t ing_ld32(const uint8_t* p, bool vec)
{
    if (vec) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ void ing_st32(uint8_t* p, uint32_t v, bool vec)
{
    if (vec) { *reinterpret_cast<uint32_t*>(p) = v; return; }
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
__device__ __forceinline__ int ing_byte(uint32_t w, int k) { return (int)((w >> (8 * k)) & 255u); }

__global__ __launch_bounds__(256) void k_ingest(IngArgs a)
{
    const IngImage im = a.img[blockIdx.y];
    const int stride = a.src_stride[blockIdx.y];
    const bool src_vec = (stride & 3) == 0 && ((uintptr_t)im.src & 3) == 0, dst_vec = a.dst_vec != 0;
    const int groups = (a.w + 3) >> 2;          // four-pixel groups per row, the last one may be short
    const bool nv12 = im.fmt == LPSLAM_HIP_PIXEL_NV12;
    const int rows = nv12 ? a.h >> 1 : a.h;     // NV12: a lane works on rows 2 r and 2 r + 1
    const int total = rows * groups;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int r = i / groups, x = (i - r * groups) * 4, np = min(4, a.w - x);
        if (im.fmt == LPSLAM_HIP_PIXEL_RGB8 || im.fmt == LPSLAM_HIP_PIXEL_BGR8) {
            const int ir = im.fmt == LPSLAM_HIP_PIXEL_BGR8 ? 2 : 0, ib = 2 - ir;
            const uint8_t* p = im.src + (size_t)r * stride + (size_t)x * 3;
            uint8_t* q = im.dst + (size_t)r * a.dst_pitch + x;
            if (np == 4) {
                const uint32_t w[3] = {ing_ld32(p, src_vec), ing_ld32(p + 4, src_vec), ing_ld32(p + 8, src_vec)};
                uint32_t out = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {       // (constant indices once unrolled: the three words stay in registers)
                    const int b0 = ing_byte(w[(3 * k) >> 2], (3 * k) & 3), b1 = ing_byte(w[(3 * k + 1) >> 2], (3 * k + 1) & 3), b2 = ing_byte(w[(3 * k + 2) >> 2], (3 * k + 2) & 3);
                    out |= (uint32_t)grey_of_rgb(ir ? b2 : b0, b1, ir ? b0 : b2) << (8 * k);
                }
                ing_st32(q, out, dst_vec);
            } else {
                for (int k = 0; k < np; ++k) q[k] = (uint8_t)grey_of_rgb(p[3 * k + ir], p[3 * k + 1], p[3 * k + ib]);
            }
        } else if (im.fmt == LPSLAM_HIP_PIXEL_UYVY) {
            const uint8_t* p = im.src + (size_t)r * stride + (size_t)x * 2;       // x is even: a pixel pair starts here
            uint8_t* q = im.dst + (size_t)r * a.dst_pitch + x;
            if (np == 4) {
                const uint32_t w0 = ing_ld32(p, src_vec), w1 = ing_ld32(p + 4, src_vec);
                const uint32_t out = (uint32_t)grey_of_yuv(ing_byte(w0, 1), ing_byte(w0, 0), ing_byte(w0, 2)) |
                                     ((uint32_t)grey_of_yuv(ing_byte(w0, 3), ing_byte(w0, 0), ing_byte(w0, 2)) << 8) |
                                     ((uint32_t)grey_of_yuv(ing_byte(w1, 1), ing_byte(w1, 0), ing_byte(w1, 2)) << 16) |
                                     ((uint32_t)grey_of_yuv(ing_byte(w1, 3), ing_byte(w1, 0), ing_byte(w1, 2)) << 24);
                ing_st32(q, out, dst_vec);
            } else {
                for (int k = 0; k < np; ++k) { const uint8_t* pair = p + 4 * (k >> 1); q[k] = (uint8_t)grey_of_yuv(pair[1 + 2 * (k & 1)], pair[0], pair[2]); }
            }
        } else {        // NV12
            const uint8_t* y0 = im.src + (size_t)(2 * r) * stride + x;
            const uint8_t* y1 = y0 + stride;
            const uint8_t* uv = im.src + a.chroma_off[blockIdx.y] + (size_t)r * stride + x;      // x is even: a U V pair starts here
            uint8_t* q0 = im.dst + (size_t)(2 * r) * a.dst_pitch + x;
            uint8_t* q1 = q0 + a.dst_pitch;
            if (np == 4) {
                const uint32_t a0 = ing_ld32(y0, src_vec), a1 = ing_ld32(y1, src_vec), c = ing_ld32(uv, src_vec);
                uint32_t o0 = 0, o1 = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int u = ing_byte(c, k & 2), v = ing_byte(c, (k & 2) + 1);
                    o0 |= (uint32_t)grey_of_yuv(ing_byte(a0, k), u, v) << (8 * k);
                    o1 |= (uint32_t)grey_of_yuv(ing_byte(a1, k), u, v) << (8 * k);
                }
                ing_st32(q0, o0, dst_vec); ing_st32(q1, o1, dst_vec);
            } else {
                for (int k = 0; k < np; ++k) {
                    const int u = uv[k & 2], v = uv[(k & 2) + 1];
                    q0[k] = (uint8_t)grey_of_yuv(y0[k], u, v); q1[k] = (uint8_t)grey_of_yuv(y1[k], u, v);
                }
            }
        }
    }
}

// bytes between the staged rows of a format: the row itself, rounded up to a dword
int staged_stride(int fmt, int w) { return ((fmt == LPSLAM_HIP_PIXEL_NV12 ? w : fmt == LPSLAM_HIP_PIXEL_UYVY ? 2 * w : 3 * w) + 3) & ~3; }
int row_bytes(int fmt, int w) { return fmt == LPSLAM_HIP_PIXEL_NV12 ? w : fmt == LPSLAM_HIP_PIXEL_UYVY ? 2 * w : 3 * w; }
// one slot's staging: the largest staged frame (RGB)
size_t staging_bytes(const lpslam_hip_ctx* c) { return (size_t)staged_stride(LPSLAM_HIP_PIXEL_RGB8, c->lt.w[0]) * (size_t)c->lt.h[0]; }

int ensure_staging(lpslam_hip_ctx* c, int image)
{
    std::lock_guard<std::mutex> lock(c->pool_mutex);       // (a tracking thread and its prefetch thread may both arrive here first)
    if (c->h_color.size() < (size_t)c->cfg.max_images) { c->h_color.resize((size_t)c->cfg.max_images, nullptr); c->d_color.resize((size_t)c->cfg.max_images, nullptr); }
    const size_t n = staging_bytes(c);
    if (!c->h_color[(size_t)image] && hipHostMalloc((void**)&c->h_color[(size_t)image], n, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); c->h_color[(size_t)image] = nullptr; set_error("page-locked colour staging of %zu bytes failed", n); return LPSLAM_HIP_ERR_DEVICE;
    }
    if (!c->d_color[(size_t)image] && hipMalloc((void**)&c->d_color[(size_t)image], n) != hipSuccess) {
        (void)hipGetLastError(); c->d_color[(size_t)image] = nullptr; set_error("device colour staging of %zu bytes failed", n); return LPSLAM_HIP_ERR_DEVICE;
    }
    return LPSLAM_HIP_OK;
}

}  // namespace

int lp_ingest_check(lpslam_hip_ctx* c, const lpslam_hip_pixels* px)
{
    if (!c || !px) { set_error("null argument"); return LPSLAM_HIP_ERR_INVALID; }
    const int w = c->lt.w[0], h = c->lt.h[0];
    if (px->format == LPSLAM_HIP_PIXEL_GRAY8) {        // (the check and the words of the grey calls)
        if (!px->data || px->stride < w) { set_error("bad host image (stride %d < width %d)", px->stride, w); return LPSLAM_HIP_ERR_INVALID; }
        return LPSLAM_HIP_OK;
    }
    if (!px->data) { set_error("null argument"); return LPSLAM_HIP_ERR_INVALID; }
    switch (px->format) {
    case LPSLAM_HIP_PIXEL_RGB8: case LPSLAM_HIP_PIXEL_BGR8: break;
    case LPSLAM_HIP_PIXEL_NV12:
        if ((w | h) & 1) { set_error("NV12 needs an even width and height (%d x %d)", w, h); return LPSLAM_HIP_ERR_INVALID; }
        if (px->chroma && px->chroma_stride < w) { set_error("bad host image (chroma stride %d < width %d)", px->chroma_stride, w); return LPSLAM_HIP_ERR_INVALID; }
        break;
    case LPSLAM_HIP_PIXEL_UYVY:
        if (w & 1) { set_error("UYVY needs an even width (%d)", w); return LPSLAM_HIP_ERR_INVALID; }
        break;
    default: set_error("unknown pixel format %d", px->format); return LPSLAM_HIP_ERR_INVALID;
    }
    const int need = row_bytes(px->format, w);
    if (px->stride < need) { set_error("bad host image (stride %d < row of %d bytes)", px->stride, need); return LPSLAM_HIP_ERR_INVALID; }
    return LPSLAM_HIP_OK;
}

int lp_ingest_stage(lpslam_hip_ctx* c, int image, const lpslam_hip_pixels* px, hipStream_t us)
{
    int rc = ensure_staging(c, image); if (rc) return rc;
    const int w = c->lt.w[0], h = c->lt.h[0], fmt = px->format;
    const size_t rb = (size_t)row_bytes(fmt, w), ss = (size_t)staged_stride(fmt, w);
    uint8_t* buf = c->h_color[(size_t)image];
    auto rows = [&](uint8_t* to, const uint8_t* from, size_t stride, int n) {
        if (stride == ss) memcpy(to, from, ss * (size_t)(n - 1) + rb);
        else for (int r = 0; r < n; ++r) memcpy(to + (size_t)r * ss, from + (size_t)r * stride, rb);
    };
    size_t total = ss * (size_t)h;
    rows(buf, px->data, (size_t)px->stride, h);
    if (fmt == LPSLAM_HIP_PIXEL_NV12) {
        const uint8_t* chroma = px->chroma ? px->chroma : px->data + (size_t)px->stride * (size_t)h;
        rows(buf + total, chroma, (size_t)(px->chroma ? px->chroma_stride : px->stride), h / 2);
        total += ss * (size_t)(h / 2);
    }
    LP_HIP(hipMemcpyAsync(c->d_color[(size_t)image], buf, total, hipMemcpyHostToDevice, us));
    return LPSLAM_HIP_OK;
}

int lp_ingest_launch(lpslam_hip_ctx* c, hipStream_t s, int n, const int* images, const int32_t* formats, uint8_t* const* dst, int dst_pitch)
{
    if (n < 1 || n > 2) { set_error("ingest: %d images in one launch", n); return LPSLAM_HIP_ERR_INVALID; }
    IngArgs a{};
    a.w = c->lt.w[0]; a.h = c->lt.h[0]; a.dst_pitch = dst_pitch;
    a.dst_vec = (dst_pitch & 3) == 0 ? 1 : 0;
    for (int k = 0; k < n; ++k) {
        a.img[k] = IngImage{c->d_color[(size_t)images[k]], dst[k], formats[k]};
        a.src_stride[k] = staged_stride(formats[k], a.w);
        a.chroma_off[k] = (unsigned)((size_t)a.src_stride[k] * (size_t)a.h);
        if ((uintptr_t)dst[k] & 3) a.dst_vec = 0;
    }
    // four pixels (NV12: eight) per lane and pass; enough workgroups to fill the chip, the rest in the grid-stride loop
    const int lanes = ((a.w + 3) / 4) * a.h;
    const int blocks = std::max(1, std::min(2048, (lanes + 255) / 256));
    hipLaunchKernelGGL(k_ingest, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, s, a);
    LP_HIP(hipGetLastError());
    return LPSLAM_HIP_OK;
}

void lp_ingest_free(lpslam_hip_ctx* c)
{
    for (uint8_t* b : c->h_color) if (b) (void)hipHostFree(b);
    for (uint8_t* b : c->d_color) if (b) (void)hipFree(b);
    c->h_color.clear(); c->d_color.clear();
}
