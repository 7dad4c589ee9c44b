// occupancy.hip -- 2-D occupancy grid from laser scans on gfx950: the scan store and the grid build.
//
// [UPSTREAM] map_publisher::occupancy_map_export of LP-Research's OpenVSLAM fork (absent), reached from the reference through
// src/Trackers/OpenVSLAMStereoTracker.cpp:374-400.  The grid is defined exactly in INTEGRATION.md ("Occupancy grid"); this file
// computes that definition.  A build is four launches on the context's occupancy stream:
//   k_occ_rays   one workgroup per scan: end points in FP64, the ray records (origin cell, end cell, hit), the box (LDS min/max,
//                one global atomic per workgroup and field)
//   k_occ_bin    one lane per ray, twice: the 64 x 64-cell tiles of the box each ray crosses, with the first and last step of the
//                ray in each from the closed form -- first counted, then (after k_occ_scan) scattered into a (tile -> segment)
//                list.  Lanes of a wavefront that land in the same tile share one atomic.
//   k_occ_tiles  one workgroup per tile (a tile with many segments: several, see kChunkSegs) walks its segments incrementally and
//                counts hits and misses in LDS; the owner writes the tile's int8 cells with plain stores (no count grid in HBM, no
//                global atomics per cell visit); a split tile leaves partial counts that k_occ_merge adds up.
// Every count is an integer sum, so the grid does not depend on launch or scheduling order.
#include "internal.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

using namespace lpslam;

namespace {

constexpr int kTile = 64;                       // tile side in cells (box and tiles are aligned to 64 in global cell coordinates)
constexpr int kTileCells = kTile * kTile;
constexpr double kCellLimit = 268435456.0;      // 2^28: a beam whose origin or end cell is not inside (-2^28, 2^28) is skipped
constexpr long long kChunkSegs = 16384;         // segments one tile workgroup walks; a tile with more is split into chunks
constexpr int kMaxSide = 65536;

struct OccScan {            // one pose of a build (device table)
    const float* ranges;
    const double2* cs;
    long long ray0;
    int n, pad;
    double rmin, rmax, rthr;
    double ox, oy, fx, fy, lx, ly;
};
struct OccRay { int gx0, gy0, gx1, gy1; };
struct OccSeg { int ray, kb, ke; };
struct OccWork { int tile, partial; long long s0, s1; };      // partial < 0: this workgroup owns the tile's cells
struct OccMerge { int tile, first, count, pad; };
struct OccBox { int min_x, min_y, max_x, max_y; unsigned long long rays, visits; };
struct OccGrid { long long x0, y0; int tiles_x, tiles_y, width; };

// ---- the traversal of INTEGRATION.md in major / minor form: cell k = (a0 + sa k, b0 + sb q(k)), q(k) = (2 k db + da) div (2 da)
struct Walk { int a0, b0, sa, sb, da, db, n; bool xmajor; };

__device__ __forceinline__ Walk make_walk(const OccRay& r)
{
    Walk w;
    const int dx = abs(r.gx1 - r.gx0), dy = abs(r.gy1 - r.gy0);
    const int sx = (r.gx1 > r.gx0) - (r.gx1 < r.gx0), sy = (r.gy1 > r.gy0) - (r.gy1 < r.gy0);
    w.xmajor = dx >= dy;
    if (w.xmajor) { w.a0 = r.gx0; w.b0 = r.gy0; w.sa = sx; w.sb = sy; w.da = dx; w.db = dy; }
    else          { w.a0 = r.gy0; w.b0 = r.gx0; w.sa = sy; w.sb = sx; w.da = dy; w.db = dx; }
    w.n = w.da;
    return w;
}

// smallest k >= 0 with q(k) >= m (db > 0)
__device__ __forceinline__ long long kmin_q(long long m, long long da, long long db)
{
    const long long num = 2 * da * m - da;
    return num <= 0 ? 0 : (num + 2 * db - 1) / (2 * db);
}

// the steps of the ray inside the box [Alo, Ahi) x [Blo, Bhi) (major, minor): an interval, both coordinates being monotonic
__device__ __forceinline__ bool clip_walk(const Walk& w, long long Alo, long long Ahi, long long Blo, long long Bhi, long long& klo, long long& khi)
{
    klo = 0; khi = w.n;
    if (w.sa > 0) { klo = max(klo, Alo - w.a0); khi = min(khi, Ahi - 1 - w.a0); }
    else if (w.sa < 0) { klo = max(klo, w.a0 - (Ahi - 1)); khi = min(khi, w.a0 - Alo); }
    else if (w.a0 < Alo || w.a0 >= Ahi) return false;
    if (w.sb == 0) {
        if (w.b0 < Blo || w.b0 >= Bhi) return false;
    } else {
        const long long qlo = w.sb > 0 ? Blo - w.b0 : w.b0 - (Bhi - 1);
        const long long qhi = w.sb > 0 ? Bhi - 1 - w.b0 : w.b0 - Blo;
        if (qhi < 0) return false;
        klo = max(klo, kmin_q(qlo, w.da, w.db));
        khi = min(khi, kmin_q(qhi + 1, w.da, w.db) - 1);
    }
    return klo <= khi;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- kernel 1: ray records and the box ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_occ_rays(const OccScan* __restrict__ scans, OccRay* __restrict__ rays, uint8_t* __restrict__ flags,
                                                  OccBox* box, double inv_res)
{
    __shared__ int s_box[4];
    __shared__ unsigned s_rays;
    if (threadIdx.x == 0) { s_box[0] = INT_MAX; s_box[1] = INT_MAX; s_box[2] = INT_MIN; s_box[3] = INT_MIN; s_rays = 0; }
    __syncthreads();
    const OccScan s = scans[blockIdx.x];
    const double oxc = s.ox * inv_res, oyc = s.oy * inv_res;
    const bool origin_ok = fabs(oxc) < kCellLimit && fabs(oyc) < kCellLimit;
    const int gx0 = origin_ok ? (int)floor(oxc) : 0, gy0 = origin_ok ? (int)floor(oyc) : 0;
    int mnx = INT_MAX, mny = INT_MAX, mxx = INT_MIN, mxy = INT_MIN;
    unsigned cnt = 0;
    for (int i = threadIdx.x; i < s.n; i += blockDim.x) {
        const double r = (double)s.ranges[i];
        OccRay rec{gx0, gy0, gx0, gy0};
        uint8_t f = 0;
        if (origin_ok && isfinite(r) && !(r < s.rmin)) {
            const bool hit = r < s.rthr && r <= s.rmax;
            const double L = hit ? r : (s.rthr < s.rmax ? s.rthr : s.rmax);
            const double2 cs = s.cs[i];
            const double ex = s.ox + L * (cs.x * s.fx + cs.y * s.lx);
            const double ey = s.oy + L * (cs.x * s.fy + cs.y * s.ly);
            const double exc = ex * inv_res, eyc = ey * inv_res;
            if (fabs(exc) < kCellLimit && fabs(eyc) < kCellLimit) {
                rec.gx1 = (int)floor(exc); rec.gy1 = (int)floor(eyc);
                f = hit ? 3 : 1;
                mnx = min(mnx, min(gx0, rec.gx1)); mxx = max(mxx, max(gx0, rec.gx1));
                mny = min(mny, min(gy0, rec.gy1)); mxy = max(mxy, max(gy0, rec.gy1));
                ++cnt;
            }
        }
        rays[s.ray0 + i] = rec;
        flags[s.ray0 + i] = f;
    }
    if (cnt) {
        atomicMin(&s_box[0], mnx); atomicMin(&s_box[1], mny); atomicMax(&s_box[2], mxx); atomicMax(&s_box[3], mxy);
        atomicAdd(&s_rays, cnt);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_rays) {
        atomicMin(&box->min_x, s_box[0]); atomicMin(&box->min_y, s_box[1]); atomicMax(&box->max_x, s_box[2]); atomicMax(&box->max_y, s_box[3]);
        atomicAdd(&box->rays, (unsigned long long)s_rays);
    }
}

// ---- kernel 2: (tile -> segment) binning: count (segs == nullptr) or scatter ------------------------------------------------
__global__ __launch_bounds__(256) void k_occ_bin(const OccRay* __restrict__ rays, const uint8_t* __restrict__ flags, long long n_rays, OccGrid g,
                                                 unsigned* __restrict__ tile_count, unsigned long long* __restrict__ cursor,
                                                 OccSeg* __restrict__ segs, unsigned long long* visits)
{
    const int lane = __lane_id();
    const long long Xlo = g.x0, Xhi = g.x0 + (long long)g.tiles_x * kTile, Ylo = g.y0, Yhi = g.y0 + (long long)g.tiles_y * kTile;
    const int max_iter = g.tiles_x + g.tiles_y + 2;      // a ray crosses at most this many tiles of the box
    unsigned long long my_visits = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = (long long)blockIdx.x * blockDim.x; base < n_rays; base += stride) {      // (uniform per wavefront)
        const long long i = base + threadIdx.x;
        bool live = false;
        Walk w{};
        long long k = 0, khi = -1;
        long long Alo = 0, Blo = 0;
        if (i < n_rays && flags[i]) {
            w = make_walk(rays[i]);
            Alo = w.xmajor ? Xlo : Ylo; Blo = w.xmajor ? Ylo : Xlo;
            const long long Ahi = w.xmajor ? Xhi : Yhi, Bhi = w.xmajor ? Yhi : Xhi;
            live = clip_walk(w, Alo, Ahi, Blo, Bhi, k, khi);
        }
        for (int it = 0; it < max_iter; ++it) {
            const bool has = live && k <= khi;
            if (!__ballot(has)) break;
            int tile = -1;
            long long kend = 0;
            if (has) {
                const long long a = w.a0 + (long long)w.sa * k;
                const long long q = w.da ? (2 * k * w.db + w.da) / (2 * (long long)w.da) : 0;
                const long long b = w.b0 + (long long)w.sb * q;
                const long long ta = (a - Alo) >> 6, tb = (b - Blo) >> 6;
                kend = khi;
                if (w.sa > 0) kend = min(kend, Alo + (ta + 1) * kTile - w.a0 - 1);
                else if (w.sa < 0) kend = min(kend, w.a0 - (Alo + ta * kTile - 1) - 1);
                if (w.sb > 0) kend = min(kend, kmin_q(Blo + (tb + 1) * kTile - w.b0, w.da, w.db) - 1);
                else if (w.sb < 0) kend = min(kend, kmin_q(w.b0 - (Blo + tb * kTile - 1), w.da, w.db) - 1);
                tile = w.xmajor ? (int)(tb * g.tiles_x + ta) : (int)(ta * g.tiles_x + tb);
                my_visits += (unsigned long long)(kend - k + 1);
            }
            // one atomic per distinct tile of the wavefront
            unsigned long long pend = __ballot(has);
            while (pend) {
                const int leader = __ffsll((long long)pend) - 1;
                const int t0 = __shfl(tile, leader);
                const bool mine = has && tile == t0;
                const unsigned long long m = __ballot(mine);
                if (!segs) {
                    if (lane == leader) atomicAdd(&tile_count[t0], (unsigned)__popcll(m));
                } else {
                    unsigned long long slot = 0;
                    if (lane == leader) slot = atomicAdd(&cursor[t0], (unsigned long long)__popcll(m));
                    slot = __shfl(slot, leader);
                    if (mine) {
                        slot += (unsigned long long)__popcll(m & ((1ull << lane) - 1));
                        segs[slot] = OccSeg{(int)i, (int)k, (int)kend};
                    }
                }
                pend &= ~m;
            }
            if (has) k = kend + 1;
        }
    }
    if (!segs) {
        const unsigned long long v = wave_sum(my_visits);
        if (lane == 0 && v) atomicAdd(visits, v);
    }
}

// ---- exclusive prefix of the tile counts (one workgroup): offsets[t], offsets[n] = total; cursor = offsets -------------------
__global__ __launch_bounds__(1024) void k_occ_scan(const unsigned* __restrict__ count, int n, unsigned long long* __restrict__ offsets,
                                                   unsigned long long* __restrict__ cursor)
{
    __shared__ unsigned long long part[1024];
    const int per = (n + (int)blockDim.x - 1) / (int)blockDim.x;
    const int b = (int)threadIdx.x * per, e = min(n, b + per);
    unsigned long long sum = 0;
    for (int t = b; t < e; ++t) sum += count[t];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < (int)blockDim.x; o <<= 1) {      // Hillis-Steele over the per-thread sums
        const unsigned long long v = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = part[threadIdx.x] - sum;
    for (int t = b; t < e; ++t) { offsets[t] = run; cursor[t] = run; run += count[t]; }
    if (threadIdx.x == blockDim.x - 1) offsets[n] = part[threadIdx.x];
}

__device__ __forceinline__ int8_t occ_value(unsigned long long h, unsigned long long m)
{
    const unsigned long long n = h + m;
    return n == 0 ? (int8_t)-1 : (int8_t)((100 * h + n / 2) / n);
}

// ---- kernel 3: tile owner ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_occ_tiles(const OccWork* __restrict__ work, const OccSeg* __restrict__ segs, const OccRay* __restrict__ rays,
                                                   const uint8_t* __restrict__ flags, OccGrid g, int8_t* __restrict__ grid, unsigned* __restrict__ partials)
{
    __shared__ unsigned cnt[2][kTileCells];      // [0] misses, [1] hits
    for (int c = threadIdx.x; c < 2 * kTileCells; c += blockDim.x) (&cnt[0][0])[c] = 0;
    __syncthreads();
    const OccWork wk = work[blockIdx.x];
    const int tx = wk.tile % g.tiles_x, ty = wk.tile / g.tiles_x;
    const int cx0 = (int)(g.x0 + (long long)tx * kTile), cy0 = (int)(g.y0 + (long long)ty * kTile);
    const int lane = __lane_id();
    long long s = wk.s0 + threadIdx.x;
    // per lane: the segment being walked -- cell (a, b), remainder r of q(k), steps left
    int a = 0, b = 0, sa = 0, sb = 0, r = 0, da2 = 0, db2 = 0, left = 0, hit_at = -1, k = 0;
    bool xmajor = true;
    for (;;) {
        while (left <= 0 && s < wk.s1) {
            const OccSeg sg = segs[s];
            s += blockDim.x;
            const Walk w = make_walk(rays[sg.ray]);
            const long long N = 2LL * sg.kb * w.db + w.da;
            const long long q = w.da ? N / (2LL * w.da) : 0;
            r = w.da ? (int)(N - q * 2LL * w.da) : 0;
            a = w.a0 + w.sa * sg.kb; b = w.b0 + w.sb * (int)q;
            sa = w.sa; sb = w.sb; da2 = 2 * w.da; db2 = 2 * w.db; xmajor = w.xmajor;
            k = sg.kb; left = sg.ke - sg.kb + 1;
            hit_at = (flags[sg.ray] & 2) ? w.n : -1;
        }
        const bool active = left > 0;
        const unsigned long long act = __ballot(active);
        if (!act) break;
        int code = -1;
        if (active) {
            const int lx = (xmajor ? a : b) - cx0, ly = (xmajor ? b : a) - cy0;
            code = ((ly * kTile + lx) << 1) | (k == hit_at ? 1 : 0);
        }
        // lanes on one cell (every beam of a scan near its origin): one LDS atomic for the wavefront
        const int leader = __ffsll((long long)act) - 1;
        const int c0 = __shfl(code, leader);
        const unsigned long long same = __ballot(code == c0);
        if (same == act) {
            if (lane == leader) atomicAdd(&cnt[c0 & 1][c0 >> 1], (unsigned)__popcll(act));
        } else if (active) {
            atomicAdd(&cnt[code & 1][code >> 1], 1u);
        }
        if (active) {
            ++k; --left; a += sa; r += db2;
            if (r >= da2) { r -= da2; b += sb; }
        }
    }
    __syncthreads();
    if (wk.partial < 0) {
        // 16 cells per thread: row t / 4, columns 16 (t % 4) ..
        const int row = threadIdx.x >> 2, col = (threadIdx.x & 3) * 16;
        union { int8_t v[16]; uint4 u; } pk;
        for (int j = 0; j < 16; ++j) pk.v[j] = occ_value(cnt[1][row * kTile + col + j], cnt[0][row * kTile + col + j]);
        *reinterpret_cast<uint4*>(grid + (size_t)(ty * kTile + row) * g.width + (size_t)tx * kTile + col) = pk.u;
    } else {
        unsigned* p = partials + (size_t)wk.partial * 2 * kTileCells;
        for (int c = threadIdx.x; c < 2 * kTileCells; c += blockDim.x) p[c] = (&cnt[0][0])[c];
    }
}

// ---- a split tile: sum of its chunks' partial counts; block = (tile, row), thread = column ----------------------------------
__global__ __launch_bounds__(64) void k_occ_merge(const OccMerge* __restrict__ merges, const unsigned* __restrict__ partials, OccGrid g,
                                                  int8_t* __restrict__ grid)
{
    const OccMerge mg = merges[blockIdx.x];
    const int row = blockIdx.y, col = threadIdx.x, c = row * kTile + col;
    unsigned long long h = 0, m = 0;
    for (int p = 0; p < mg.count; ++p) {
        const unsigned* q = partials + (size_t)(mg.first + p) * 2 * kTileCells;
        m += q[c]; h += q[kTileCells + c];
    }
    const int tx = mg.tile % g.tiles_x, ty = mg.tile / g.tiles_x;
    grid[(size_t)(ty * kTile + row) * g.width + (size_t)tx * kTile + col] = occ_value(h, m);
}

long long floor64(long long v) { return v >= 0 ? v / 64 * 64 : -((-v + 63) / 64) * 64; }

}  // namespace

struct LpOccupancy {
    hipStream_t stream = nullptr;
    struct Geometry { double2* d = nullptr; int n = 0; };
    std::vector<Geometry> geometries;
    struct Scan { float* d = nullptr; int cap = 0, n = 0, geometry = -1; float rmin = 0, rmax = 0, rthr = 0; };
    std::map<int, Scan> scans;
    // build buffers, grown as needed (every build ends with a stream synchronisation, so a buffer is idle when it is replaced)
    struct Buf { void* p = nullptr; size_t cap = 0; };
    Buf table, rays, flags, tile_count, offsets, cursor, segs, work, merges, partials, grid, box;
    OccBox* h_box = nullptr;
};

namespace {

int grow(LpOccupancy::Buf& b, size_t bytes)
{
    if (b.cap >= bytes) return LPSLAM_HIP_OK;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t cap = std::max<size_t>(bytes + bytes / 4, 4096);
    LP_HIP(hipMalloc(&b.p, cap));
    b.cap = cap;
    return LPSLAM_HIP_OK;
}

int occ_state(lpslam_hip_ctx* c, LpOccupancy** out)
{
    if (!c->occ) {
        LP_HIP(hipSetDevice(c->cfg.device));
        auto* o = new LpOccupancy();
        if (hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking) != hipSuccess ||
            hipHostMalloc((void**)&o->h_box, sizeof(OccBox)) != hipSuccess) {
            const hipError_t e = hipGetLastError();
            if (o->stream) (void)hipStreamDestroy(o->stream);
            delete o;
            return hip_fail(e == hipSuccess ? hipErrorOutOfMemory : e, "occupancy stream / staging");
        }
        c->occ = o;
    }
    *out = c->occ;
    return LPSLAM_HIP_OK;
}

}  // namespace

void lp_occupancy_free(lpslam_hip_ctx* c)
{
    std::lock_guard<std::mutex> lock(c->occ_mutex);
    LpOccupancy* o = c->occ;
    if (!o) return;
    (void)hipStreamSynchronize(o->stream);
    for (auto& g : o->geometries) if (g.d) (void)hipFree(g.d);
    for (auto& kv : o->scans) if (kv.second.d) (void)hipFree(kv.second.d);
    for (LpOccupancy::Buf* b : {&o->table, &o->rays, &o->flags, &o->tile_count, &o->offsets, &o->cursor, &o->segs, &o->work, &o->merges, &o->partials, &o->grid, &o->box})
        if (b->p) (void)hipFree(b->p);
    if (o->h_box) (void)hipHostFree(o->h_box);
    (void)hipStreamDestroy(o->stream);
    delete o;
    c->occ = nullptr;
}

extern "C" {

int lpslam_hip_scan_geometry_put(lpslam_hip_ctx* c, const double* cos_sin, int32_t n_beams, int32_t* id)
{
    if (!c || !cos_sin || !id || n_beams <= 0) { set_error("bad scan_geometry_put arguments"); return LPSLAM_HIP_ERR_INVALID; }
    std::lock_guard<std::mutex> lock(c->occ_mutex);
    LpOccupancy* o = nullptr;
    if (const int rc = occ_state(c, &o)) return rc;
    LP_HIP(hipSetDevice(c->cfg.device));
    LpOccupancy::Geometry g;
    g.n = n_beams;
    LP_HIP(hipMalloc((void**)&g.d, sizeof(double2) * (size_t)n_beams));
    const hipError_t e = hipMemcpy(g.d, cos_sin, sizeof(double2) * (size_t)n_beams, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(g.d); return hip_fail(e, "hipMemcpy scan geometry"); }
    *id = (int32_t)o->geometries.size();
    o->geometries.push_back(g);
    return LPSLAM_HIP_OK;
}

int lpslam_hip_scan_store_put(lpslam_hip_ctx* c, int32_t key, int32_t geometry_id, const float* ranges, int32_t n, float range_min,
                              float range_max, float range_threshold)
{
    if (!c || !ranges || n <= 0) { set_error("bad scan_store_put arguments"); return LPSLAM_HIP_ERR_INVALID; }
    std::lock_guard<std::mutex> lock(c->occ_mutex);
    LpOccupancy* o = nullptr;
    if (const int rc = occ_state(c, &o)) return rc;
    if (geometry_id < 0 || geometry_id >= (int)o->geometries.size() || o->geometries[(size_t)geometry_id].n != n) {
        set_error("scan_store_put: geometry %d does not exist or has not %d beams", geometry_id, n);
        return LPSLAM_HIP_ERR_INVALID;
    }
    LP_HIP(hipSetDevice(c->cfg.device));
    LpOccupancy::Scan& s = o->scans[key];
    if (s.cap < n) {
        if (s.d) { (void)hipFree(s.d); s.d = nullptr; s.cap = 0; }
        if (hipMalloc((void**)&s.d, sizeof(float) * (size_t)n) != hipSuccess) { o->scans.erase(key); return hip_fail(hipGetLastError(), "hipMalloc scan"); }
        s.cap = n;
    }
    s.n = n; s.geometry = geometry_id; s.rmin = range_min; s.rmax = range_max; s.rthr = range_threshold;
    LP_HIP(hipMemcpyAsync(s.d, ranges, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, o->stream));
    LP_HIP(hipStreamSynchronize(o->stream));      // (the caller's buffer is free when the call returns)
    return LPSLAM_HIP_OK;
}

int lpslam_hip_scan_store_drop(lpslam_hip_ctx* c, int32_t key)
{
    if (!c) { set_error("null context"); return LPSLAM_HIP_ERR_INVALID; }
    std::lock_guard<std::mutex> lock(c->occ_mutex);
    LpOccupancy* o = c->occ;
    if (!o) return LPSLAM_HIP_OK;
    auto it = o->scans.find(key);
    if (it == o->scans.end()) return LPSLAM_HIP_OK;
    if (it->second.d) { (void)hipSetDevice(c->cfg.device); (void)hipFree(it->second.d); }
    o->scans.erase(it);
    return LPSLAM_HIP_OK;
}

int lpslam_hip_occupancy_build(lpslam_hip_ctx* c, const lpslam_hip_scan_pose* poses, int32_t n, double res, int32_t max_side,
                               int8_t* out, int64_t capacity, lpslam_hip_grid_info* info)
{
    if (!c || !info || n < 0 || (n > 0 && !poses) || !(res > 0) || !std::isfinite(res) || max_side <= 0 || max_side % kTile || max_side > kMaxSide) {
        set_error("bad occupancy_build arguments (res > 0, max_side a multiple of 64 in 64 .. %d)", kMaxSide);
        return LPSLAM_HIP_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lock(c->occ_mutex);
    LpOccupancy* o = nullptr;
    if (const int rc = occ_state(c, &o)) return rc;
    LP_HIP(hipSetDevice(c->cfg.device));
    const double inv_res = 1.0 / res;
    // the scan table: every key must be stored
    std::vector<OccScan> table((size_t)n);
    long long n_rays = 0;
    for (int i = 0; i < n; ++i) {
        auto it = o->scans.find(poses[i].key);
        if (it == o->scans.end()) { set_error("occupancy_build: no scan stored under key %d", poses[i].key); return LPSLAM_HIP_ERR_INVALID; }
        const LpOccupancy::Scan& s = it->second;
        OccScan& t = table[(size_t)i];
        t.ranges = s.d; t.cs = o->geometries[(size_t)s.geometry].d; t.ray0 = n_rays; t.n = s.n; t.pad = 0;
        t.rmin = s.rmin; t.rmax = s.rmax; t.rthr = s.rthr;
        t.ox = poses[i].origin[0]; t.oy = poses[i].origin[1]; t.fx = poses[i].fwd[0]; t.fy = poses[i].fwd[1]; t.lx = poses[i].left[0]; t.ly = poses[i].left[1];
        n_rays += s.n;
    }
    if (n_rays >= INT_MAX) { set_error("occupancy_build: %lld beams exceed the supported 2^31", n_rays); return LPSLAM_HIP_ERR_CAPACITY; }
    *info = lpslam_hip_grid_info{};
    if (n == 0) return LPSLAM_HIP_OK;
    hipStream_t st = o->stream;
    if (int rc = grow(o->table, sizeof(OccScan) * (size_t)n)) return rc;
    if (int rc = grow(o->rays, sizeof(OccRay) * (size_t)n_rays)) return rc;
    if (int rc = grow(o->flags, (size_t)n_rays)) return rc;
    if (int rc = grow(o->box, sizeof(OccBox))) return rc;
    *o->h_box = OccBox{INT_MAX, INT_MAX, INT_MIN, INT_MIN, 0, 0};
    LP_HIP(hipMemcpyAsync(o->table.p, table.data(), sizeof(OccScan) * (size_t)n, hipMemcpyHostToDevice, st));
    LP_HIP(hipMemcpyAsync(o->box.p, o->h_box, sizeof(OccBox), hipMemcpyHostToDevice, st));
    OccBox* d_box = (OccBox*)o->box.p;
    k_occ_rays<<<n, 256, 0, st>>>((const OccScan*)o->table.p, (OccRay*)o->rays.p, (uint8_t*)o->flags.p, d_box, inv_res);
    LP_HIP(hipGetLastError());
    LP_HIP(hipMemcpyAsync(o->h_box, d_box, sizeof(OccBox), hipMemcpyDeviceToHost, st));
    LP_HIP(hipStreamSynchronize(st));
    const OccBox bx = *o->h_box;
    if (bx.rays == 0) return LPSLAM_HIP_OK;
    // the box: origin and end cells, snapped outward to 64; a side longer than max_side is re-centred on the last pose's origin cell
    long long lo[2] = {floor64(bx.min_x), floor64(bx.min_y)}, hi[2] = {floor64(bx.max_x) + kTile, floor64(bx.max_y) + kTile};
    const double last[2] = {poses[n - 1].origin[0] * inv_res, poses[n - 1].origin[1] * inv_res};
    for (int a = 0; a < 2; ++a) {
        if (hi[a] - lo[a] <= max_side) continue;
        const long long cc = std::isfinite(last[a]) ? (long long)std::floor(std::max(-kCellLimit, std::min(kCellLimit, last[a]))) : 0;
        lo[a] = floor64(cc - max_side / 2); hi[a] = lo[a] + max_side;
    }
    OccGrid g;
    g.x0 = lo[0]; g.y0 = lo[1];
    g.tiles_x = (int)((hi[0] - lo[0]) / kTile); g.tiles_y = (int)((hi[1] - lo[1]) / kTile);
    g.width = g.tiles_x * kTile;
    const int height = g.tiles_y * kTile;
    const long long cells = (long long)g.width * height;
    if (out && capacity < cells) { set_error("occupancy_build: capacity %lld < %d x %d cells", (long long)capacity, g.width, height); return LPSLAM_HIP_ERR_INVALID; }
    const int n_tiles = g.tiles_x * g.tiles_y;
    if (int rc = grow(o->tile_count, sizeof(unsigned) * (size_t)n_tiles)) return rc;
    if (int rc = grow(o->offsets, sizeof(unsigned long long) * ((size_t)n_tiles + 1))) return rc;
    if (int rc = grow(o->cursor, sizeof(unsigned long long) * (size_t)n_tiles)) return rc;
    LP_HIP(hipMemsetAsync(o->tile_count.p, 0, sizeof(unsigned) * (size_t)n_tiles, st));
    const int bin_blocks = (int)std::min<long long>((n_rays + 255) / 256, 16384);
    k_occ_bin<<<bin_blocks, 256, 0, st>>>((const OccRay*)o->rays.p, (const uint8_t*)o->flags.p, n_rays, g, (unsigned*)o->tile_count.p,
                                          (unsigned long long*)o->cursor.p, nullptr, &d_box->visits);
    LP_HIP(hipGetLastError());
    k_occ_scan<<<1, 1024, 0, st>>>((const unsigned*)o->tile_count.p, n_tiles, (unsigned long long*)o->offsets.p, (unsigned long long*)o->cursor.p);
    LP_HIP(hipGetLastError());
    std::vector<unsigned long long> off((size_t)n_tiles + 1);
    LP_HIP(hipMemcpyAsync(off.data(), o->offsets.p, sizeof(unsigned long long) * off.size(), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemcpyAsync(o->h_box, d_box, sizeof(OccBox), hipMemcpyDeviceToHost, st));
    LP_HIP(hipStreamSynchronize(st));
    info->x0 = g.x0; info->y0 = g.y0; info->width = g.width; info->height = height;
    info->rays = (int64_t)bx.rays; info->cell_visits = (int64_t)o->h_box->visits;
    if (!out) return LPSLAM_HIP_OK;
    // segments, then the work list: one workgroup per tile, kChunkSegs segments at most each; a split tile is merged afterwards
    const unsigned long long n_segs = off[(size_t)n_tiles];
    if (n_segs >= (1ull << 34)) { set_error("occupancy_build: %llu ray segments exceed the supported count", n_segs); return LPSLAM_HIP_ERR_CAPACITY; }
    std::vector<OccWork> work; work.reserve((size_t)n_tiles);
    std::vector<OccMerge> merges;
    int n_partials = 0;
    for (int t = 0; t < n_tiles; ++t) {
        const long long s0 = (long long)off[(size_t)t], s1 = (long long)off[(size_t)t + 1];
        if (s1 - s0 <= kChunkSegs) { work.push_back(OccWork{t, -1, s0, s1}); continue; }
        const int chunks = (int)((s1 - s0 + kChunkSegs - 1) / kChunkSegs);
        merges.push_back(OccMerge{t, n_partials, chunks, 0});
        for (int k = 0; k < chunks; ++k) work.push_back(OccWork{t, n_partials + k, s0 + k * kChunkSegs, std::min(s1, s0 + (k + 1) * kChunkSegs)});
        n_partials += chunks;
    }
    if (int rc = grow(o->segs, sizeof(OccSeg) * std::max<size_t>((size_t)n_segs, 1))) return rc;
    if (int rc = grow(o->work, sizeof(OccWork) * work.size())) return rc;
    if (int rc = grow(o->grid, (size_t)cells)) return rc;
    if (!merges.empty()) {
        if (int rc = grow(o->merges, sizeof(OccMerge) * merges.size())) return rc;
        if (int rc = grow(o->partials, sizeof(unsigned) * 2 * kTileCells * (size_t)n_partials)) return rc;
        LP_HIP(hipMemcpyAsync(o->merges.p, merges.data(), sizeof(OccMerge) * merges.size(), hipMemcpyHostToDevice, st));
    }
    LP_HIP(hipMemcpyAsync(o->work.p, work.data(), sizeof(OccWork) * work.size(), hipMemcpyHostToDevice, st));
    k_occ_bin<<<bin_blocks, 256, 0, st>>>((const OccRay*)o->rays.p, (const uint8_t*)o->flags.p, n_rays, g, (unsigned*)o->tile_count.p,
                                          (unsigned long long*)o->cursor.p, (OccSeg*)o->segs.p, nullptr);
    LP_HIP(hipGetLastError());
    k_occ_tiles<<<(unsigned)work.size(), 256, 0, st>>>((const OccWork*)o->work.p, (const OccSeg*)o->segs.p, (const OccRay*)o->rays.p,
                                                       (const uint8_t*)o->flags.p, g, (int8_t*)o->grid.p, (unsigned*)o->partials.p);
    LP_HIP(hipGetLastError());
    if (!merges.empty()) {
        k_occ_merge<<<dim3((unsigned)merges.size(), kTile), kTile, 0, st>>>((const OccMerge*)o->merges.p, (const unsigned*)o->partials.p, g, (int8_t*)o->grid.p);
        LP_HIP(hipGetLastError());
    }
    LP_HIP(hipMemcpyAsync(out, o->grid.p, (size_t)cells, hipMemcpyDeviceToHost, st));
    LP_HIP(hipStreamSynchronize(st));
    return LPSLAM_HIP_OK;
}

}  // extern "C"
