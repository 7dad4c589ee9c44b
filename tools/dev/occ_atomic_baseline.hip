// occ_atomic_baseline.hip -- micro-benchmark for tools/time_occupancy.py, not part of the library: the occupancy traversal done the
// plain way, one lane per ray walking every cell of its ray with one global atomic per cell visit into uint32 hit / miss grids in
// HBM, then one pass to int8.  Input: the ray records and the box of a library build (same traversal as lpslam_amd/csrc/occupancy.hip),
// so its grid must equal the library's byte for byte.  Built as a shared library: hipcc --offload-arch=gfx950 -O3 -shared -fPIC.
#include <hip/hip_runtime.h>
#include <cstdint>

__global__ void k_walk(const int4* rays, const uint8_t* flags, int n, long long x0, long long y0, int W, int H, unsigned* hits, unsigned* misses)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const int4 r = rays[i];
    const int dx = abs(r.z - r.x), dy = abs(r.w - r.y);
    const int sx = (r.z > r.x) - (r.z < r.x), sy = (r.w > r.y) - (r.w < r.y);
    const bool xm = dx >= dy;
    const int da = xm ? dx : dy, db = xm ? dy : dx, sa = xm ? sx : sy, sb = xm ? sy : sx;
    int a = xm ? r.x : r.y, b = xm ? r.y : r.x, rem = da, q2 = 2 * da;
    for (int k = 0; k <= da; ++k) {
        const long long cx = xm ? a : b, cy = xm ? b : a;
        if (cx >= x0 && cx < x0 + W && cy >= y0 && cy < y0 + H) {
            const size_t c = (size_t)(cy - y0) * W + (size_t)(cx - x0);
            atomicAdd((k == da && (flags[i] & 2)) ? &hits[c] : &misses[c], 1u);
        }
        a += sa; rem += 2 * db;
        if (rem >= q2) { rem -= q2; b += sb; }
    }
}

__global__ void k_final(const unsigned* hits, const unsigned* misses, long long cells, int8_t* out)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cells) return;
    const unsigned long long h = hits[c], n = h + misses[c];
    out[c] = n == 0 ? (int8_t)-1 : (int8_t)((100 * h + n / 2) / n);
}

extern "C" int occ_atomic_build(const int* rays4, const uint8_t* flags, int n, long long x0, long long y0, int W, int H, int reps,
                                int8_t* out, float* kernel_ms)
{
    int4* d_r = nullptr; uint8_t* d_f = nullptr; unsigned* d_c = nullptr; int8_t* d_o = nullptr;
    const long long cells = (long long)W * H;
    if (hipMalloc(&d_r, sizeof(int4) * (size_t)n) || hipMalloc(&d_f, (size_t)n) || hipMalloc(&d_c, sizeof(unsigned) * 2 * (size_t)cells) ||
        hipMalloc(&d_o, (size_t)cells)) return 1;
    hipMemcpy(d_r, rays4, sizeof(int4) * (size_t)n, hipMemcpyHostToDevice);
    hipMemcpy(d_f, flags, (size_t)n, hipMemcpyHostToDevice);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int r = 0; r < reps; ++r) {
        hipMemset(d_c, 0, sizeof(unsigned) * 2 * (size_t)cells);
        hipEventRecord(e0, 0);
        k_walk<<<(n + 255) / 256, 256>>>(d_r, d_f, n, x0, y0, W, H, d_c, d_c + cells);
        k_final<<<(unsigned)((cells + 255) / 256), 256>>>(d_c, d_c + cells, cells, d_o);
        hipEventRecord(e1, 0); hipEventSynchronize(e1);
        hipEventElapsedTime(&kernel_ms[r], e0, e1);
    }
    hipMemcpy(out, d_o, (size_t)cells, hipMemcpyDeviceToHost);
    const int rc = hipGetLastError() != hipSuccess;
    hipFree(d_r); hipFree(d_f); hipFree(d_c); hipFree(d_o); hipEventDestroy(e0); hipEventDestroy(e1);
    return rc;
}
