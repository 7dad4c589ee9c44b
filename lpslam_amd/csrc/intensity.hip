// intensity.hip -- the AdjustIntensity processor on the device: histogram, limits, look-up table and point transform of the images of
// one frame, in place on what the front end reads next (gfx950).
//
// Replaces the per-frame host call of the reference's AdjustIntensityProcessor (src/Processor/AdjustIntensityProcessor.h:10-41), i.e.
// ImageProcessing::imadjust(image, out, nullopt, nullopt, -0.3, 1.4) on each eye (src/Utils/ImageProcessing.h:258-370).  The arithmetic
// is the one DESIGN.md section 17 states, bit for bit that of the host implementation (lpslam_amd/host/intensity.cpp):
//   hist[256] over the pixels; low_count = (uint32)(low_fraction * N), high_count = (uint32)((1 - high_fraction) * N), in double;
//   lo = the first i (ascending) whose exclusive prefix sum is >= low_count (none: 0), hi = the first i (descending) whose exclusive
//   suffix sum is >= high_count (none: 1); alpha = (high_out - low_out) / (hi / 255 - lo / 255), beta = (high_out - hi / 255 * alpha) * 255
//   in double; out = saturate_u8(round_half_even((float)x * (float)alpha + (float)beta)), product and sum unfused; lo == hi: unchanged.
//
// Two launches per frame, every image of the frame in each (blockIdx.y = image):
//   k_adj_hist   per-wavefront histograms in LDS (32-bit counters), merged into 256 words per image with one vector atomic per non-empty
//                bin and workgroup.  Integer counts: the order of the atomics does not matter, the result is reproducible.
//   k_adj_apply  every workgroup redoes the 256-step walk (a scan over the 256 words) and the table in LDS, then maps its share of the
//                pixels, 16 per load / store.  The kernel boundary is what makes the histogram words visible on every XCD.
// The histogram words of a slot exist twice: an adjustment counts into one set and its k_adj_apply zeroes the OTHER set, which the
// slot's next adjustment counts into -- cleared on the stream, never by the host, and never while a workgroup may still read them.  The
// set of the last adjustment stays readable for lpslam_hip_adjust_intensity_last.
#include "internal.h"

#include <cmath>

using namespace lpslam;

namespace {

constexpr int kAdjBatch = 64;          // images per launch (one bit each in the `sets` word)

// One image = `rows` rows of `row_bytes` pixels, `pitch` bytes apart; a contiguous image is one row of width * height bytes.  A row is
// cut into 16-byte chunks; `vec`: the chunks are 16-byte aligned (base, slab and pitch are), whole chunks move as one dwordx4.
struct AdjGeom { int rows, row_bytes, pitch, chunks_per_row, vec; unsigned long long slab; };

__device__ __forceinline__ void adj_count_word(uint32_t* h, uint32_t w)
{
    const uint32_t b0 = w & 255u;
    if (w == b0 * 0x01010101u) { atomicAdd(&h[b0], 4u); return; }       // flat areas: one LDS atomic per dword
    atomicAdd(&h[b0], 1u); atomicAdd(&h[(w >> 8) & 255u], 1u); atomicAdd(&h[(w >> 16) & 255u], 1u); atomicAdd(&h[w >> 24], 1u);
}

__global__ __launch_bounds__(256) void k_adj_hist(const uint8_t* __restrict__ base, AdjGeom g, uint32_t* __restrict__ hist, int slot0,
                                                  unsigned long long sets)
{
    __shared__ uint32_t s_h[4][256];
    const int t = threadIdx.x, img = blockIdx.y;
    for (int k = 0; k < 4; ++k) s_h[k][t] = 0;
    __syncthreads();
    uint32_t* h = s_h[t >> 6];
    const uint8_t* p = base + (size_t)img * g.slab;
    const int total = g.rows * g.chunks_per_row;
    for (int i = blockIdx.x * 256 + t; i < total; i += gridDim.x * 256) {
        const int row = i / g.chunks_per_row, c = i - row * g.chunks_per_row;
        const uint8_t* q = p + (size_t)row * g.pitch + (size_t)c * 16;
        const int nb = min(16, g.row_bytes - c * 16);
        if (nb == 16 && g.vec) {
            const uint4 v = *reinterpret_cast<const uint4*>(q);
            adj_count_word(h, v.x); adj_count_word(h, v.y); adj_count_word(h, v.z); adj_count_word(h, v.w);
        } else {
            for (int k = 0; k < nb; ++k) atomicAdd(&h[q[k]], 1u);
        }
    }
    __syncthreads();
    const uint32_t n = s_h[0][t] + s_h[1][t] + s_h[2][t] + s_h[3][t];
    if (n) atomicAdd(&hist[((size_t)(slot0 + img) * 2 + ((sets >> img) & 1ull)) * 256 + t], n);
}

__global__ __launch_bounds__(256) void k_adj_apply(uint8_t* __restrict__ base, AdjGeom g, uint32_t* __restrict__ hist, int32_t* __restrict__ lohi,
                                                   int slot0, unsigned long long sets, uint32_t low_count, uint32_t high_count, double low_out,
                                                   double high_out)
{
    __shared__ uint32_t s_sum[256];
    __shared__ int s_lo, s_hi;
    __shared__ uint8_t s_tab[256];
    const int t = threadIdx.x, img = blockIdx.y, slot = slot0 + img;
    const int set = (int)((sets >> img) & 1ull);
    const uint32_t mine = hist[((size_t)slot * 2 + set) * 256 + t];
    if (blockIdx.x == 0) hist[((size_t)slot * 2 + (set ^ 1)) * 256 + t] = 0;      // the set the slot's NEXT adjustment counts into
    if (t == 0) { s_lo = 256; s_hi = -1; }
    s_sum[t] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {        // inclusive scan of the 256 bins
        const uint32_t v = s_sum[t] + (t >= off ? s_sum[t - off] : 0u);
        __syncthreads();
        s_sum[t] = v;
        __syncthreads();
    }
    const uint32_t incl = s_sum[t], total = s_sum[255];
    // the walks test before they add: bin t is reached with the sum of the bins before it (after it, for the descending walk)
    if (incl - mine >= low_count) atomicMin(&s_lo, t);
    if (total - incl >= high_count) atomicMax(&s_hi, t);
    __syncthreads();
    const int lo = s_lo == 256 ? 0 : s_lo, hi = s_hi < 0 ? 1 : s_hi;
    if (lo == hi) s_tab[t] = (uint8_t)t;             // alpha would be infinite: the image stays as it is
    else {
        const double lo_n = (double)lo / 255.0, hi_n = (double)hi / 255.0;
        const double alpha = __ddiv_rn(__dsub_rn(high_out, low_out), __dsub_rn(hi_n, lo_n));
        const double beta = __dmul_rn(__dsub_rn(high_out, __dmul_rn(hi_n, alpha)), 255.0);
        const float v = rintf(__fadd_rn(__fmul_rn((float)t, (float)alpha), (float)beta));      // unfused, round half to even
        s_tab[t] = (uint8_t)(v > 0.0f ? (v >= 255.0f ? 255.0f : v) : 0.0f);      // (a NaN -- outputs beyond the double range -- gives 0)
    }
    if (blockIdx.x == 0 && t == 0) { lohi[slot * 2] = lo; lohi[slot * 2 + 1] = hi; }
    __syncthreads();
    uint8_t* p = base + (size_t)img * g.slab;
    const int n_chunks = g.rows * g.chunks_per_row;
    for (int i = blockIdx.x * 256 + t; i < n_chunks; i += gridDim.x * 256) {
        const int row = i / g.chunks_per_row, c = i - row * g.chunks_per_row;
        uint8_t* q = p + (size_t)row * g.pitch + (size_t)c * 16;
        const int nb = min(16, g.row_bytes - c * 16);
        if (nb == 16 && g.vec) {
            uint4 v = *reinterpret_cast<const uint4*>(q);
            auto map4 = [&](uint32_t w) -> uint32_t {
                return (uint32_t)s_tab[w & 255u] | ((uint32_t)s_tab[(w >> 8) & 255u] << 8) | ((uint32_t)s_tab[(w >> 16) & 255u] << 16) | ((uint32_t)s_tab[w >> 24] << 24);
            };
            v.x = map4(v.x); v.y = map4(v.y); v.z = map4(v.z); v.w = map4(v.w);
            *reinterpret_cast<uint4*>(q) = v;
        } else {
            for (int k = 0; k < nb; ++k) q[k] = s_tab[q[k]];
        }
    }
}

// the histogram sets and limits of every slot of the context; made at the first adjustment (zeroed before any stream can use them)
int adj_state(lpslam_hip_ctx* c)
{
    std::lock_guard<std::mutex> lock(c->pool_mutex);
    if (c->d_adj_hist) return LPSLAM_HIP_OK;
    const size_t B = (size_t)c->cfg.max_images;
    uint32_t* hist = nullptr; int32_t* lohi = nullptr;
    LP_HIP(hipMalloc((void**)&hist, B * 2 * 256 * sizeof(uint32_t)));
    if (hipMalloc((void**)&lohi, B * 2 * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(hist); set_error("device memory for the intensity limits"); return LPSLAM_HIP_ERR_DEVICE; }
    // (the context's streams do not synchronise with the null stream: the zeroes must be there before any of them runs a kernel)
    if (hipMemset(hist, 0, B * 2 * 256 * sizeof(uint32_t)) != hipSuccess || hipMemset(lohi, 0, B * 2 * sizeof(int32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(hist); (void)hipFree(lohi); set_error("clearing the intensity histograms failed"); return LPSLAM_HIP_ERR_DEVICE;
    }
    c->adj_set.assign(B, 0); c->adj_seen.assign(B, 0);
    c->d_adj_lohi = lohi; c->d_adj_hist = hist;
    return LPSLAM_HIP_OK;
}

}  // namespace

int lp_adjust_check(lpslam_hip_ctx* c, const lpslam_hip_adjust_params* p)
{
    if (!c || !p) { set_error("null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (!std::isfinite(p->low_out) || !std::isfinite(p->high_out) || !(p->low_out < p->high_out)) { set_error("adjust intensity: low_out %g must be below high_out %g", p->low_out, p->high_out); return LPSLAM_HIP_ERR_INVALID; }
    if (!(p->low_fraction >= 0.0) || !(p->low_fraction < p->high_fraction) || !(p->high_fraction <= 1.0)) {
        set_error("adjust intensity: fractions must satisfy 0 <= low (%g) < high (%g) <= 1", p->low_fraction, p->high_fraction); return LPSLAM_HIP_ERR_INVALID;
    }
    if ((size_t)c->lt.w[0] * (size_t)c->lt.h[0] >= ((size_t)1 << 24)) { set_error("adjust intensity: images of 2^24 pixels and more are not supported (%d x %d)", c->lt.w[0], c->lt.h[0]); return LPSLAM_HIP_ERR_CAPACITY; }
    return LPSLAM_HIP_OK;
}

// Adjusts n images in place on stream `s`: image k starts at base + k * slab and belongs to slot first + k (whose histogram words and
// limits it uses); rows of `width` pixels `pitch` bytes apart.  Arguments checked by the caller (lp_adjust_check, slot range).
int lp_adjust_launch(lpslam_hip_ctx* c, hipStream_t s, uint8_t* base, size_t slab, int pitch, int first, int n, const lpslam_hip_adjust_params* p)
{
    int rc = adj_state(c); if (rc) return rc;
    const int w = c->lt.w[0], h = c->lt.h[0];
    const size_t N = (size_t)w * (size_t)h;
    AdjGeom g{};
    if (pitch == w) { g.rows = 1; g.row_bytes = (int)N; g.pitch = (int)N; }
    else { g.rows = h; g.row_bytes = w; g.pitch = pitch; }
    g.chunks_per_row = (g.row_bytes + 15) / 16;
    g.slab = slab;
    g.vec = ((uintptr_t)base % 16 == 0 && (n == 1 || slab % 16 == 0) && (g.rows == 1 || pitch % 16 == 0)) ? 1 : 0;
    const uint32_t low_count = (uint32_t)(p->low_fraction * (double)N), high_count = (uint32_t)((1.0 - p->high_fraction) * (double)N);
    // two chunks (32 pixels) per thread and pass, at most one workgroup per compute unit and image
    const int blocks = std::max(1, std::min(256, (g.rows * g.chunks_per_row + 511) / 512));
    for (int k0 = 0; k0 < n; k0 += kAdjBatch) {
        const int m = std::min(n - k0, kAdjBatch);
        unsigned long long sets = 0;
        for (int k = 0; k < m; ++k) {
            uint8_t& set = c->adj_set[(size_t)(first + k0 + k)];
            if (set) sets |= 1ull << k;
            set ^= 1;
            c->adj_seen[(size_t)(first + k0 + k)] = 1;
        }
        uint8_t* b = base + (size_t)k0 * slab;
        hipLaunchKernelGGL(k_adj_hist, dim3((unsigned)blocks, (unsigned)m), dim3(256), 0, s, (const uint8_t*)b, g, c->d_adj_hist, first + k0, sets);
        LP_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_adj_apply, dim3((unsigned)blocks, (unsigned)m), dim3(256), 0, s, b, g, c->d_adj_hist, c->d_adj_lohi, first + k0, sets,
                           low_count, high_count, p->low_out, p->high_out);
        LP_HIP(hipGetLastError());
    }
    return LPSLAM_HIP_OK;
}

void lp_adjust_free(lpslam_hip_ctx* c)
{
    if (c->d_adj_hist) (void)hipFree(c->d_adj_hist);
    if (c->d_adj_lohi) (void)hipFree(c->d_adj_lohi);
    c->d_adj_hist = nullptr; c->d_adj_lohi = nullptr;
}

extern "C" {

int lpslam_hip_adjust_intensity_last(lpslam_hip_ctx* c, int image, int32_t* lo, int32_t* hi, uint32_t* hist256)
{
    if (!c) { set_error("null context"); return LPSLAM_HIP_ERR_INVALID; }
    if (image < 0 || image >= c->cfg.max_images) { set_error("image slot %d exceeds the context capacity %d", image, c->cfg.max_images); return LPSLAM_HIP_ERR_CAPACITY; }
    if (!c->d_adj_hist || !c->adj_seen[(size_t)image]) { set_error("image slot %d has not been adjusted", image); return LPSLAM_HIP_ERR_INVALID; }
    LP_HIP(hipSetDevice(c->cfg.device));
    LP_HIP(hipStreamSynchronize(c->stream));
    if (c->fe_stream) LP_HIP(hipStreamSynchronize(c->fe_stream));
    int32_t lh[2] = {0, 0};
    LP_HIP(hipMemcpy(lh, c->d_adj_lohi + (size_t)image * 2, sizeof(lh), hipMemcpyDeviceToHost));
    if (lo) *lo = lh[0];
    if (hi) *hi = lh[1];
    const int last = c->adj_set[(size_t)image] ^ 1;       // adj_set names the set of the NEXT adjustment
    if (hist256) LP_HIP(hipMemcpy(hist256, c->d_adj_hist + ((size_t)image * 2 + (size_t)last) * 256, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return LPSLAM_HIP_OK;
}

}  // extern "C"
