// pose_opt.hip -- motion-only pose optimisation on gfx950 (FP64), the whole flow in one workgroup.
//
// [UPSTREAM] optimize::pose_optimizer: one SE3 vertex, unary reprojection edges to fixed landmarks, 4 rounds of 10 Levenberg
// iterations (g2o lambda control), after every round the observations with chi2 > 5.991 (mono) / 7.815 (stereo) become
// outliers (and may come back), Huber is dropped after the third round, the flow stops when fewer than 5 inliers remain.
// The tracker needs this once per frame: instead of ~600 launches through the general BA machinery the 6x6 system lives in
// LDS and one launch returns the pose (one workgroup; several frames / candidates could share a launch, one workgroup each).
#include "internal.h"
#include "ba_common.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#pragma clang fp contract(off)

using namespace lpslam;

namespace {

struct PoShared {
    double pose[7];
    double red[8];                     // the wavefronts' partial sums of po_block_sum
    double sums[28];                   // a pass's 28 sums (upper triangle of H, b, chi2)
};

// The kernel is one workgroup and a chain of 50 - 65 dependent Levenberg trials; a trial is ~3 us of latency, not of arithmetic
// (round 4, in-kernel cycle stamps: pass over the observations ~2000 cycles, the 28-value reduction ~1700, decision + 6x6 solve +
// pose update ~3500).  Four wavefronts, one per SIMD: the reduction's register step costs every SIMD half of what it costs with
// eight, the passes are issue-bound either way, and the serial section between two passes is executed by EVERY thread on
// replicated registers (a SIMD runs one lane as fast as 64), so nothing is published and no barrier follows it.  In the
// per-observation arithmetic, reciprocals and reciprocal square roots come from v_rcp_f64 / v_rsq_f64 plus one cubic correction
// step (1.4e-16 relative error, measured) where IEEE division and sqrt cost ~30 instructions each.  Products and sums are contracted
// to fused multiply-adds in these functions (the rest of the file is compiled without contraction): the Cholesky solve alone went
// from 107 multiplications + 73 additions to half as many instructions on the serial section's critical path.
#ifndef LPSLAM_PO_T
#define LPSLAM_PO_T 256
#endif
constexpr int PO_T = LPSLAM_PO_T;
static_assert(PO_T >= 128 && PO_T % 64 == 0, "k_pose_optimize: the 27-value reduction needs at least two wavefronts (one wavefront faulted on the device, round 4)");
constexpr int PO_W = PO_T / 64;
__device__ __forceinline__ double po_rcp(double d) { return fast_rcp(d); }
__device__ __forceinline__ double po_block_sum(double v, PoShared& sh)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh.red[0];
#pragma unroll
    for (int w = 1; w < PO_W; ++w) s += sh.red[w];
    return s;
}
__device__ __forceinline__ void po_quat_to_rot(const double* q, double* R)
{
#pragma clang fp contract(fast)
    const double rn = po_rsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * rn, x = q[1] * rn, y = q[2] * rn, z = q[3] * rn;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}
// the same for a quaternion of unit length (what po_oplus returns): no normalisation on the chain between two passes
__device__ __forceinline__ void po_unit_quat_to_rot(const double* q, double* R)
{
#pragma clang fp contract(fast)
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}
__device__ __forceinline__ void po_huber(double e2, double delta, double* rho0, double* rho1)
{
#pragma clang fp contract(fast)
    const double dsqr = delta * delta;
    if (e2 <= dsqr) { *rho0 = e2; *rho1 = 1.0; }
    else { const double rs = po_rsqrt(e2); *rho0 = 2 * (e2 * rs) * delta - dsqr; *rho1 = delta * rs; }
}
// pose half of ba_jacobians (the landmark is a constant here), with one reciprocal
__device__ __forceinline__ void po_jacobian(const BaCam& c, const double* pc, double iz, int D, double B[3][6])
{
#pragma clang fp contract(fast)
    const double x = pc[0], y = pc[1], iz2 = iz * iz;
    B[0][0] = x * y * iz2 * c.fx;          B[0][1] = -(1.0 + (x * x * iz2)) * c.fx; B[0][2] = y * iz * c.fx;
    B[0][3] = -iz * c.fx;                  B[0][4] = 0.0;                            B[0][5] = x * iz2 * c.fx;
    B[1][0] = (1.0 + y * y * iz2) * c.fy;  B[1][1] = -x * y * iz2 * c.fy;            B[1][2] = -x * iz * c.fy;
    B[1][3] = 0.0;                         B[1][4] = -iz * c.fy;                     B[1][5] = y * iz2 * c.fy;
    B[2][0] = B[0][0] - c.fxb * y * iz2;   B[2][1] = B[0][1] + c.fxb * x * iz2;      B[2][2] = B[0][2];
    B[2][3] = B[0][3];                     B[2][4] = 0.0;                            B[2][5] = B[0][5] - c.fxb * iz2;
    if (D == 2) {
#pragma unroll
        for (int k = 0; k < 6; ++k) B[2][k] = 0.0;
    }
}
// residual of observation k at pose p7; returns the dimension (2 / 3)
__device__ __forceinline__ int po_residual(const BaCam& cam, const double* R, const double* t, const double* X, const lpslam_hip_ba_obs& o, double* e, double* pc, double* iz_out = nullptr)
{
#pragma clang fp contract(fast)
#pragma unroll
    for (int i = 0; i < 3; ++i) pc[i] = R[i * 3] * X[0] + R[i * 3 + 1] * X[1] + R[i * 3 + 2] * X[2] + t[i];
    const double iz = po_rcp(pc[2]);
    if (iz_out) *iz_out = iz;
    const double u = cam.fx * pc[0] * iz + cam.cx, vv = cam.fy * pc[1] * iz + cam.cy;
    e[0] = o.u - u; e[1] = o.v - vv;
    if (o.ur < 0) { e[2] = 0; return 2; }
    e[2] = o.ur - (u - cam.fxb * iz);
    return 3;
}
// One observation as the kernel keeps it in LDS: measurement, weight and the landmark it sees (56 bytes); the first `cache_n`
// observations live there, the rest (only very large n) is read from global memory like before.
struct PoObs { double u, v, ur, w, X[3]; };

template <bool ALL_CACHED>
struct PoData {
    const double* pts; const lpslam_hip_ba_obs* obs; const PoObs* cache; const uint8_t* act; int n, cache_n;
    __device__ __forceinline__ void get(int k, lpslam_hip_ba_obs& o, double* X) const
    {
        // (ALL_CACHED is a compile-time fact on purpose: with both sources in one function the compiler merges them into generic
        // pointers and every LDS read becomes a flat load)
        if (ALL_CACHED || k < cache_n) {
            const PoObs c = cache[k];
            o.pose = 0; o.point = 0; o.u = c.u; o.v = c.v; o.ur = c.ur; o.inv_sigma2 = c.w;
            X[0] = c.X[0]; X[1] = c.X[1]; X[2] = c.X[2];
        } else {
            o = obs[k];
            const double* p = pts + 3 * (size_t)o.point;
            X[0] = p[0]; X[1] = p[1]; X[2] = p[2];
        }
    }
};

// The 28 sums of a pass (upper triangle of H, b, chi2) over the PO_T threads: first over each quad of lanes in registers (two DPP
// exchanges per value), then one lane of four stores its 28 partials transposed into LDS, PO_T / 32 lanes per value add eight of
// them each (interleaved: neighbouring lanes read neighbouring words) and finish inside their DPP row.
template <int CTRL>
__device__ __forceinline__ double quad_swap(double v)     // DPP exchange inside a row (a shuffle would go through the LDS crossbar)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
constexpr int PO_NV = 28;                  // values per pass
constexpr int PO_Q = PO_T / 4;             // partials per value after the quad step
constexpr int PO_TR = PO_Q + 8;            // padded row of the transposed reduction buffer [PO_NV][PO_Q]: the second step's lanes read (value q, partial j + 8 i) --
                                           // q 72 + j puts the eight values of a wavefront's read on different banks (with + 1 they met four to a bank)
constexpr int PO_LPV = PO_T / 32;          // lanes per value in the second step (16 = one DPP row at 512 threads)
static_assert(PO_NV * PO_LPV <= PO_T && PO_Q == 8 * PO_LPV && (PO_LPV == 16 || PO_LPV == 8 || PO_LPV == 4), "po_reduce28 layout");
__device__ __forceinline__ void po_reduce28(double (&acc)[PO_NV], double* tr, double* out, int lane_stride)
{
    const int tid = threadIdx.x;
    // (lane_stride: observations sit in every lane / every second / every fourth -- po_pass: the register step shrinks with them)
    if (lane_stride == 1) {
#pragma unroll
        for (int q = 0; q < PO_NV; ++q) acc[q] += quad_swap<0xB1>(acc[q]);           // lanes 0<->1, 2<->3
    }
    if (lane_stride <= 2) {
#pragma unroll
        for (int q = 0; q < PO_NV; ++q) acc[q] += quad_swap<0x4E>(acc[q]);           // lanes 0<->2, 1<->3
    }
    if ((tid & 3) == 0) {
#pragma unroll
        for (int q = 0; q < PO_NV; ++q) tr[q * PO_TR + (tid >> 2)] = acc[q];
    }
    __syncthreads();
    const int q = tid / PO_LPV, j = tid % PO_LPV;
    double s = 0;
    if (q < PO_NV) {
        const double* row = tr + q * PO_TR + j;
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = row[i * PO_LPV];
        s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    s += quad_swap<0xB1>(s);
    s += quad_swap<0x4E>(s);
    if (PO_LPV >= 8) s += quad_swap<0x141>(s);           // row_half_mirror: the other quad of the eight
    if (PO_LPV >= 16) s += quad_swap<0x140>(s);          // row_mirror: the other half of the row
    if (q < PO_NV && j == 0) out[q] = s;
    __syncthreads();
}

#ifdef LPSLAM_PO_STAMPS
__device__ double g_po_stamps[16];
#define PO_STAMP(k) do { if (threadIdx.x == 0) { const double now_ = (double)clock64(); po_acc[k] += now_ - po_last; po_last = now_; } } while (0)
#define PO_ST_PARAM , double (&po_acc)[16], double& po_last
#define PO_ST_ARG , po_acc, po_last
#else
#define PO_STAMP(k) do {} while (0)
#define PO_ST_PARAM
#define PO_ST_ARG
#endif

// One observation's share of the 28 sums (upper triangle of H, b, robustified chi2) at the pose (R, t)
__device__ __forceinline__ void po_accumulate(const BaCam& cam, const double (&R)[9], const double (&t)[3], const lpslam_hip_ba_obs& o, const double (&X)[3], int robust, double (&acc)[PO_NV])
{
#pragma clang fp contract(fast)
    double e[3], pc[3], B[3][6], iz;
    const int D = po_residual(cam, R, t, X, o, e, pc, &iz);
    const double om = o.inv_sigma2;
    const double chi = om * (e[0] * e[0] + e[1] * e[1] + (D == 3 ? e[2] * e[2] : 0.0));
    const double delta = D == 3 ? cam.hub_stereo : cam.hub_mono;
    double w = om, c = chi;
    if (robust && delta > 0) { double r0, r1; po_huber(chi, delta, &r0, &r1); w *= r1; c = r0; }
    acc[27] += c;
    po_jacobian(cam, pc, iz, D, B);
    // w B once (18 products), then every entry is three fused multiply-adds onto its running sum; the columns that
    // are structurally zero (B[0][4], B[1][3], B[2][4]) are skipped by hand -- the compiler may not drop x * 0
    double wB[3][6], we[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        we[r] = -w * e[r];
#pragma unroll
        for (int a = 0; a < 6; ++a) wB[r][a] = w * B[r][a];
    }
    int idx = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int c2 = a; c2 < 6; ++c2) {
            double s2 = acc[idx];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const bool zero = (r == 0 && (a == 4 || c2 == 4)) || (r == 1 && (a == 3 || c2 == 3)) || (r == 2 && (a == 4 || c2 == 4));
                if (!zero) s2 = fma(wB[r][a], B[r][c2], s2);
            }
            acc[idx++] = s2;
        }
        double s3 = acc[21 + a];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const bool zero = (r == 0 && a == 4) || (r == 1 && a == 3) || (r == 2 && a == 4);
            if (!zero) s3 = fma(B[r][a], we[r], s3);
        }
        acc[21 + a] = s3;
    }
}

// One pass over the active observations at pose p7: the 27 sums of the linearised system (upper triangle of H, then b) and the
// (robustified) chi2 as the 28th, into sh.sums (valid until the next pass).  A trial's chi2 and the NEXT iteration's linearisation are the same
// pass: the trial is accepted nearly always, and then its pose is the pose to linearise at (one reduction less per Levenberg
// iteration; a rejected trial wastes the 27 sums).
template <bool ALL_CACHED>
__device__ __forceinline__ void po_pass(const BaCam& cam, const double (&p7)[7], const PoData<ALL_CACHED>& d, int robust, double* tr, PoShared& sh PO_ST_PARAM)
{
#pragma clang fp contract(fast)
    const int tid = threadIdx.x;
    double R[9];
    po_quat_to_rot(p7, R);
    const double t[3] = {p7[4], p7[5], p7[6]};
    double acc[PO_NV];
#pragma unroll
    for (int q = 0; q < PO_NV; ++q) acc[q] = 0;
    // few observations are spread out, one per quad of lanes (up to PO_T / 4) or one per pair: the reduction's first step adds the
    // four lanes of a quad in registers, 168 instructions when every lane carries sums -- none when only one lane of four does
    const int lane_stride = d.n <= PO_T / 4 ? 4 : d.n <= PO_T / 2 ? 2 : 1;
    for (int k = (tid % lane_stride) ? d.n : tid / lane_stride; k < d.n; k += PO_T / lane_stride) {
        if (!d.act[k]) continue;
        double X[3];
        lpslam_hip_ba_obs o;
        d.get(k, o, X);
        po_accumulate(cam, R, t, o, X, robust, acc);
    }
    PO_STAMP(1);
    po_reduce28(acc, tr, sh.sums, lane_stride);
    PO_STAMP(2);
#ifdef LPSLAM_PO_STAMPS
    if (tid == 0) po_acc[15] += 1;
#endif
}

// (H + lambda I) x = b by a 6x6 Cholesky factorisation and two substitutions, fully unrolled with constant indices (the matrix
// stays in registers), then the trial pose; every thread computes its own copy.  Returns 0 when the matrix is not positive definite
// (the trial is then the pose itself and x is not meaningful).
__device__ __forceinline__ int po_solve_trial(const double (&sys)[PO_NV], double lam, const double (&pose)[7], double (&x)[6], double (&trial)[7] PO_ST_PARAM)
{
#pragma clang fp contract(fast)
    double A[36];
    {
        int idx = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c, ++idx) { A[a * 6 + c] = sys[idx]; A[c * 6 + a] = sys[idx]; }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) A[j * 7] += lam;
    int ok = 1;
    double inv[6];                                     // 1 / L_jj: six divisions per solve instead of twenty-seven
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d2 = A[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d2 -= A[j * 6 + k] * A[j * 6 + k];
        if (!(d2 > 0.0)) { ok = 0; d2 = 1.0; }         // keep going on harmless numbers; the result is discarded
        inv[j] = po_rsqrt(d2);
        A[j * 6 + j] = d2 * inv[j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s2 = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s2 -= A[i * 6 + k] * A[j * 6 + k];
            A[i * 6 + j] = s2 * inv[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s2 = sys[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s2 -= A[i * 6 + k] * x[k];
        x[i] = s2 * inv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s2 = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s2 -= A[k * 6 + i] * x[k];
        x[i] = s2 * inv[i];
    }
    PO_STAMP(4);
    double moved[7];
    po_oplus(pose, x, moved);
#pragma unroll
    for (int i = 0; i < 7; ++i) trial[i] = ok ? moved[i] : pose[i];
    PO_STAMP(5);
    return ok;
}

// ALL_CACHED (every tracker-sized call): pose7 / packed / outlier / n_inliers / done_flag are page-locked HOST memory -- the workgroup
// reads its inputs over PCIe in the prologue and writes the results straight back, then releases `seq` into *done_flag, which the
// calling thread polls (no copy-engine packet on either side, no wait for the end-of-kernel cache flush).
template <bool ALL_CACHED>
__global__ __launch_bounds__(PO_T) void k_pose_optimize(double* pose7, const double* pts, const lpslam_hip_ba_obs* obs, const PoObs* packed, int n, BaCam cam,
                                                       uint8_t* outlier, int* n_inliers, int cache_n, int* done_flag, int seq)
{
#pragma clang fp contract(fast)
    __shared__ PoShared sh;
    extern __shared__ double po_dyn[];
    double* tr = po_dyn;
    PoObs* cache = reinterpret_cast<PoObs*>(po_dyn + PO_NV * PO_TR);
    uint8_t* active = reinterpret_cast<uint8_t*>(cache + cache_n);
    const int tid = threadIdx.x;
#ifdef LPSLAM_PO_STAMPS
    double po_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, po_last = (double)clock64();
#endif
    if (tid < 7) sh.pose[tid] = pose7[tid];
    if (ALL_CACHED) {
        static_assert(sizeof(PoObs) == 7 * sizeof(double), "PoObs is copied as doubles");
        for (int i = tid; i < 7 * n; i += PO_T) reinterpret_cast<double*>(cache)[i] = reinterpret_cast<const double*>(packed)[i];
    }
    for (int k = tid; k < n; k += PO_T) {
        active[k] = 1;
        if (!ALL_CACHED && k < cache_n) {
            const lpslam_hip_ba_obs o = obs[k];
            const double* p = pts + 3 * (size_t)o.point;
            PoObs c; c.u = o.u; c.v = o.v; c.ur = o.ur; c.w = o.inv_sigma2; c.X[0] = p[0]; c.X[1] = p[1]; c.X[2] = p[2];
            cache[k] = c;
        }
    }
    __syncthreads();
    const PoData<ALL_CACHED> d{pts, obs, cache, active, n, cache_n};
    // from here on every thread holds the optimiser's state (pose, trial, system, lambda control) in its own registers
    double pose[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) pose[i] = sh.pose[i];
    int robust = 1, n_bad_last = 0, passes = 0;
    PO_STAMP(0);
    for (int round = 0; round < 4; ++round) {
        // chi2 and linearisation at the round's starting pose (the kernel / the active set may have changed), then trial after
        // trial: every pass evaluates the trial in flight AND linearises at it; g2o's Levenberg control runs between the passes:
        // up to ten iterations, each with up to ten trials of growing lambda.
        double sys[PO_NV], x[6], trial[7];
        po_pass(cam, pose, d, robust, tr, sh PO_ST_ARG);
#pragma unroll
        for (int q = 0; q < PO_NV; ++q) sys[q] = sh.sums[q];
        ++passes;
        double lambda = 1e-5 * fmax(fmax(fmax(fabs(sys[0]), fabs(sys[6])), fmax(fabs(sys[11]), fabs(sys[15]))), fmax(fabs(sys[18]), fabs(sys[20])));
        double ni = 2, current_chi = sys[27];
        int it = 0, qmax = 1;
        PO_STAMP(3);
        int ok = po_solve_trial(sys, lambda, pose, x, trial PO_ST_ARG);
        for (;;) {
            po_pass(cam, trial, d, robust, tr, sh PO_ST_ARG);
            ++passes;
            const double temp = ok ? sh.sums[27] : DBL_MAX;
            double rho = current_chi - temp, scale = 0;
            if (ok) {
#pragma unroll
                for (int j = 0; j < 6; ++j) scale += x[j] * (lambda * x[j] + sys[21 + j]);
            }
            scale += 1e-3;
            rho *= po_rcp(scale);
            if (rho > 0 && isfinite(temp)) {
                const double t3 = 2 * rho - 1;
                double alpha = 1. - t3 * t3 * t3;
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                current_chi = temp;
#pragma unroll
                for (int i = 0; i < 7; ++i) pose[i] = trial[i];
#pragma unroll
                for (int q = 0; q < PO_NV - 1; ++q) sys[q] = sh.sums[q];     // the pass just made linearised at the accepted pose
            } else {
                lambda *= ni; ni *= 2;
            }
            if (rho < 0 && qmax < 10) ++qmax;                                // another trial of this iteration
            else {
                ++it;
                if (qmax == 10 || rho == 0 || it == 10) break;
                qmax = 1;
            }
            PO_STAMP(3);
            ok = po_solve_trial(sys, lambda, pose, x, trial PO_ST_ARG);
        }
        // classification with the plain chi2 of this round's pose
        double R[9];
        po_quat_to_rot(pose, R);
        int bad = 0;
        for (int k = tid; k < n; k += PO_T) {
            double e[3], pc[3], X[3];
            lpslam_hip_ba_obs o;
            d.get(k, o, X);
            const int D = po_residual(cam, R, pose + 4, X, o, e, pc);
            const double chi = o.inv_sigma2 * (e[0] * e[0] + e[1] * e[1] + (D == 3 ? e[2] * e[2] : 0.0));
            const double thr = D == 3 ? 7.81473 : 5.99146;
            const int out = thr < chi ? 1 : 0;
            active[k] = (uint8_t)!out;
            bad += out;
        }
        n_bad_last = (int)po_block_sum((double)bad, sh);
        if (round == 2) robust = 0;
        __syncthreads();
        PO_STAMP(8);
        if (n - n_bad_last < 5) break;
    }
#ifdef LPSLAM_PO_STAMPS
    if (tid == 0) for (int k = 0; k < 16; ++k) g_po_stamps[k] = po_acc[k];
#endif
    for (int k = tid; k < n; k += PO_T) outlier[k] = active[k] ? 0 : 1;       // the last classification made
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 7; ++i) pose7[i] = pose[i];
        n_inliers[0] = n - n_bad_last;
        n_inliers[1] = passes;
    }
    if (done_flag) lp_signal_done_of(nullptr, done_flag, seq, 1u);
}

// ---- the same flow with ONE observation per lane, for up to 256 observations (what a tracked frame has) ---------------------------------
// k_pose_optimize's trial is 2.45 us, of which the 28-value reduction across its wavefronts is 0.8-1.0 (quad step in registers, LDS
// transposition, row reductions).  Here W = 1, 2 or 4 wavefronts carry one observation per lane (n <= 64 W): a pass is bound by the
// FP64 issue rate of a SIMD -- ~350 instructions per observation AND LANE, 1650 cycles whether 1 or 64 lanes are busy -- so a second
// observation per lane costs a second 1650 cycles (round 5's first version: 2.05 us per pass at <= 64 observations, 2.6 at 65-128),
// a second wavefront on the next SIMD costs two workgroup barriers.  Every lane writes its 28 partial sums into a [28][66 W] LDS
// array (consecutive lanes, consecutive words), 2 W lanes per value add 32 partials each in a fixed tree and meet their partners by DPP
// exchanges inside a row, the 28 totals come back to every lane by broadcast reads.  The serial section (lambda control, 6 x 6 solve,
// pose update) is the four-wavefront kernel's code on replicated registers, identical in every wavefront.  The sums' order differs from
// the four-wavefront kernel's (results move in the last bits); which kernel runs depends on the observation count alone.
#define PO_WN_ROW(W) (66 * (W))
template <int W>
__device__ __forceinline__ void po_reduce28_wn(const double (&acc)[PO_NV], double* tr, double* out, double (&sums)[PO_NV])
{
    // column c of a row sits at word c + c / 32 and a row is 66 W words: the 2 W lanes of a value read their 32 partials from chunks that
    // start 33 words apart and neighbouring values 2 W words (mod 32) apart, so the 16 lanes the LDS serves together touch 16 different
    // bank pairs (with rows of 64 W + 1 words the lanes of a value met on ONE bank: W = 2 / 4 measured 2.5 / 3.9 us per pass against 2.1)
    constexpr int ROW = PO_WN_ROW(W);
    constexpr int LPV = 2 * W;                             // lanes per value: neighbours inside a DPP row
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < PO_NV; ++q) tr[q * ROW + tid + (tid >> 5)] = acc[q];
    __syncthreads();                                       // (W = 1: an ordering point for the compiler and the LDS queue, not a wait)
    const int q = tid / LPV, j = tid % LPV;
    double s = 0;
    if (q < PO_NV) {
        const double* row = tr + q * ROW + 33 * j;
        double v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = row[i];
#pragma unroll
        for (int w = 16; w >= 1; w >>= 1)
#pragma unroll
            for (int i = 0; i < w; ++i) v[i] = v[2 * i] + v[2 * i + 1];
        s = v[0];
    }
    s += quad_swap<0xB1>(s);                               // lanes 0<->1, 2<->3
    if (LPV >= 4) s += quad_swap<0x4E>(s);                 // lanes 0<->2, 1<->3
    if (LPV >= 8) s += quad_swap<0x141>(s);                // row_half_mirror: the other quad of the eight
    if (q < PO_NV && j == 0) out[q] = s;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PO_NV; ++i) sums[i] = out[i];
}

// (a device function: the launch is k_pose_optimize_req below -- one workgroup per request of a batch, the same code whether the batch
// holds one tracker's frame or the pending frames of every session of the process, so shared and unshared results are the same bits)
template <int W>
__device__ __forceinline__ void po_wn_body(double* pose7, const PoObs* packed, int n, const BaCam& cam, uint8_t* outlier, int* n_inliers, int* done_flag, int seq,
                                           double* tr, double* out28, PoObs* cache, int (*s_bad)[4])
{
#pragma clang fp contract(fast)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    static_assert(sizeof(PoObs) == 7 * sizeof(double), "PoObs is copied as doubles");
    for (int i = tid; i < 7 * n; i += 64 * W) reinterpret_cast<double*>(cache)[i] = reinterpret_cast<const double*>(packed)[i];      // page-locked host memory, over PCIe
    double pose[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) pose[i] = pose7[i];
    {   // unit quaternion from here on: every pose the passes see is this one or a po_oplus result (normalised there)
        const double rn = po_rsqrt(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2] + pose[3] * pose[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) pose[i] *= rn;
    }
    __syncthreads();
    bool act = tid < n;                                    // this lane's observation is an inlier of the last classification
    // the lane's observation stays in registers for the whole call (the compiler cannot keep it there itself: the reduction writes LDS
    // between two passes)
    lpslam_hip_ba_obs o;
    double X[3];
    {
        const PoObs c = cache[tid < n ? tid : 0];
        o.pose = 0; o.point = 0; o.u = c.u; o.v = c.v; o.ur = c.ur; o.inv_sigma2 = c.w;
        X[0] = c.X[0]; X[1] = c.X[1]; X[2] = c.X[2];
    }
#ifdef LPSLAM_PO_STAMPS
    double po_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, po_last = (double)clock64();
#endif
    auto pass = [&](const double (&p7)[7], int robust, double (&sums)[PO_NV]) __attribute__((always_inline)) {
        double R[9];
        po_unit_quat_to_rot(p7, R);
        const double t[3] = {p7[4], p7[5], p7[6]};
        double acc[PO_NV];
#pragma unroll
        for (int q = 0; q < PO_NV; ++q) acc[q] = 0;
        if (act) po_accumulate(cam, R, t, o, X, robust, acc);
        PO_STAMP(1);
        po_reduce28_wn<W>(acc, tr, out28, sums);
        PO_STAMP(2);
#ifdef LPSLAM_PO_STAMPS
        if (tid == 0) po_acc[15] += 1;
#endif
    };
    int robust = 1, n_bad_last = 0, passes = 0;
    double sys[PO_NV];
    double chi_kept = 0;                                   // the (robustified) chi2 at `pose` the previous round ended with
    bool reuse = false;                                    // the round starts from the sums the previous one ended with
    for (int round = 0; round < 4; ++round) {
        // (the control flow of k_pose_optimize: g2o's Levenberg between the passes, up to ten iterations of up to ten trials; every
        // wavefront takes the same decisions from the same sums, so the barriers inside the passes match)
        double got[PO_NV], x[6], trial[7];
        // A round opens with chi2 and the linearisation at its starting pose.  When the classification changed nothing and the kernel is
        // the same, that is what the previous round ended with -- sys holds the sums at `pose` (an accepted trial's pass, or the ones the
        // rejected trials left standing), chi_kept its chi2: the same numbers a pass would produce, so the pass is not made.
        if (reuse) sys[27] = chi_kept;
        else { pass(pose, robust, sys); ++passes; }
        double lambda = 1e-5 * fmax(fmax(fmax(fabs(sys[0]), fabs(sys[6])), fmax(fabs(sys[11]), fabs(sys[15]))), fmax(fabs(sys[18]), fabs(sys[20])));
        double ni = 2, current_chi = sys[27];
        int it = 0, qmax = 1;
        PO_STAMP(3);
        int ok = po_solve_trial(sys, lambda, pose, x, trial PO_ST_ARG);
        for (;;) {
            pass(trial, robust, got);
            ++passes;
            const double temp = ok ? got[27] : DBL_MAX;
            double rho = current_chi - temp, scale = 0;
            if (ok) {
#pragma unroll
                for (int j = 0; j < 6; ++j) scale += x[j] * (lambda * x[j] + sys[21 + j]);
            }
            scale += 1e-3;
            rho *= po_rcp(scale);
            if (rho > 0 && isfinite(temp)) {
                const double t3 = 2 * rho - 1;
                double alpha = 1. - t3 * t3 * t3;
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                current_chi = temp;
#pragma unroll
                for (int i = 0; i < 7; ++i) pose[i] = trial[i];
#pragma unroll
                for (int q = 0; q < PO_NV - 1; ++q) sys[q] = got[q];         // the pass just made linearised at the accepted pose
            } else {
                lambda *= ni; ni *= 2;
            }
            if (rho < 0 && qmax < 10) ++qmax;                                // another trial of this iteration
            else {
                ++it;
                if (qmax == 10 || rho == 0 || it == 10) break;
                qmax = 1;
            }
            PO_STAMP(3);
            ok = po_solve_trial(sys, lambda, pose, x, trial PO_ST_ARG);
        }
        PO_STAMP(3);
        // classification with the plain chi2 of this round's pose
        double R[9];
        po_unit_quat_to_rot(pose, R);
        int is_out = 0;
        if (tid < n) {
            double e[3], pc[3];
            const int D = po_residual(cam, R, pose + 4, X, o, e, pc);
            const double chi = o.inv_sigma2 * (e[0] * e[0] + e[1] * e[1] + (D == 3 ? e[2] * e[2] : 0.0));
            const double thr = D == 3 ? 7.81473 : 5.99146;
            is_out = thr < chi ? 1 : 0;
        }
        const bool act_new = tid < n && !is_out;
        int bad = __popcll(__ballot(is_out)) | (__ballot(act_new != act) ? 1 << 16 : 0);       // outliers | "some lane changed sides"
        act = act_new;
        if (W > 1) {
            if (lane == 0) s_bad[round & 1][wave] = bad;
            __syncthreads();
            bad = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) { const int b2 = s_bad[round & 1][w]; bad = ((bad & 0xffff) + (b2 & 0xffff)) | ((bad | b2) & (1 << 16)); }
        }
        n_bad_last = bad & 0xffff;
        chi_kept = current_chi;
        reuse = !(bad >> 16) && round != 2;                // (after round 2 the kernel changes: plain chi2)
        if (round == 2) robust = 0;
        PO_STAMP(8);
        if (n - n_bad_last < 5) break;
    }
#ifdef LPSLAM_PO_STAMPS
    if (tid == 0) for (int k = 0; k < 16; ++k) g_po_stamps[k] = po_acc[k];
#endif
    if (tid < n) outlier[tid] = act ? 0 : 1;               // the last classification made
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 7; ++i) pose7[i] = pose[i];
        n_inliers[0] = n - n_bad_last;
        n_inliers[1] = passes;
    }
    if (done_flag) lp_signal_done_of(nullptr, done_flag, seq, 1u);
}

// One workgroup per request.  A request is a page-locked block of the caller: pose (in / out) at 0, inlier count and passes at 56 / 60,
// the done flag at 64, the camera at 72, the packed observations at 128, the outlier bytes behind them (lpslam_hip_pose_optimize lays
// it out).  Block pointer, observation count and sequence number come by value; W = 1, 2 or 4 wavefronts work on a request
// (n <= 64 W), the others of the workgroup leave at once -- a barrier counts the wavefronts that are left.
constexpr int PO_MAX_BATCH = 32;
struct PoBatch { uint8_t* blk[PO_MAX_BATCH]; int n[PO_MAX_BATCH]; int seq[PO_MAX_BATCH]; };
constexpr size_t PO_BLK_INLIERS = 56, PO_BLK_FLAG = 64, PO_BLK_CAM = 72, PO_BLK_PACKED = 128;
static_assert(PO_BLK_CAM + sizeof(BaCam) <= PO_BLK_PACKED, "pose-optimiser block header");
__global__ __launch_bounds__(256) void k_pose_optimize_req(PoBatch b)
{
    // LDS by the launch (po_lds_bytes of the largest request of the batch): the transposition array [28][66 W], the 28 totals, the
    // observations, the wavefronts' outlier counts.  A workgroup that asks for the four-wavefront layout (74 KB) whatever it needs found
    // no compute unit to start on while an extraction kernel's workgroups held theirs (8 x 13 KB of 160): requests of <= 128
    // observations -- 92 % of a tracker's -- now ask for 37 KB or 19.
    extern __shared__ __attribute__((aligned(16))) double po_lds[];
    const int wmax = (int)blockDim.x >> 6;
    double* tr = po_lds;
    double* out28 = tr + PO_NV * 66 * wmax;
    PoObs* cache = reinterpret_cast<PoObs*>(out28 + 32);
    int (*s_bad)[4] = reinterpret_cast<int (*)[4]>(cache + 64 * wmax);      // outliers per wavefront, double-buffered over the rounds
    const int r = blockIdx.x, n = b.n[r];
    uint8_t* blk = b.blk[r];
    const int W = n <= 64 ? 1 : (n <= 128 ? 2 : 4);
    if ((int)threadIdx.x >= 64 * W) return;
    BaCam cam;
    {
        const double* cp = reinterpret_cast<const double*>(blk + PO_BLK_CAM);
        cam.fx = cp[0]; cam.fy = cp[1]; cam.cx = cp[2]; cam.cy = cp[3]; cam.fxb = cp[4]; cam.hub_mono = cp[5]; cam.hub_stereo = cp[6];
    }
    double* pose7 = reinterpret_cast<double*>(blk);
    const PoObs* packed = reinterpret_cast<const PoObs*>(blk + PO_BLK_PACKED);
    uint8_t* outlier = blk + PO_BLK_PACKED + (size_t)(n > 0 ? n : 1) * sizeof(PoObs);
    int* n_inliers = reinterpret_cast<int*>(blk + PO_BLK_INLIERS);
    int* flag = reinterpret_cast<int*>(blk + PO_BLK_FLAG);
    if (W == 1) po_wn_body<1>(pose7, packed, n, cam, outlier, n_inliers, flag, b.seq[r], tr, out28, cache, s_bad);
    else if (W == 2) po_wn_body<2>(pose7, packed, n, cam, outlier, n_inliers, flag, b.seq[r], tr, out28, cache, s_bad);
    else po_wn_body<4>(pose7, packed, n, cam, outlier, n_inliers, flag, b.seq[r], tr, out28, cache, s_bad);
}

}  // namespace

int lp_launch_pose_batch(hipStream_t s, const LpPoseReq* reqs, int n)
{
    for (int i0 = 0; i0 < n; i0 += PO_MAX_BATCH) {
        const int m = std::min(n - i0, (int)PO_MAX_BATCH);
        PoBatch b{};
        int n_max = 0;
        for (int i = 0; i < m; ++i) { b.blk[i] = reqs[i0 + i].blk; b.n[i] = reqs[i0 + i].n; b.seq[i] = reqs[i0 + i].seq; n_max = std::max(n_max, reqs[i0 + i].n); }
        const int threads = n_max <= 64 ? 64 : (n_max <= 128 ? 128 : 256), wmax = threads / 64;
        const size_t lds = (size_t)(PO_NV * 66 * wmax + 32) * sizeof(double) + (size_t)64 * wmax * sizeof(PoObs) + 64;
        {
            static std::atomic<bool> attr_set[64];
            int dev = 0; (void)hipGetDevice(&dev);
            if (dev >= 0 && dev < 64 && !attr_set[dev].load()) { (void)hipFuncSetAttribute((const void*)k_pose_optimize_req, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); attr_set[dev].store(true); }
        }
        hipLaunchKernelGGL(k_pose_optimize_req, dim3((unsigned)m), dim3((unsigned)threads), lds, s, b);
        LP_HIP(hipGetLastError());
    }
    return LPSLAM_HIP_OK;
}

extern "C" {

int lpslam_hip_pose_optimize(lpslam_hip_ctx* ctx, double* pose7, const double* points, int32_t n_points, const lpslam_hip_ba_obs* obs, int32_t n_obs,
                             const lpslam_hip_ba_camera* cam, uint8_t* outlier, int32_t* n_inliers)
{
    if (!ctx || !pose7 || !cam || n_obs < 0 || n_points < 0 || (n_obs > 0 && (!points || !obs))) { set_error("invalid pose-optimiser arguments"); return LPSLAM_HIP_ERR_INVALID; }
    for (int k = 0; k < n_obs; ++k) if (obs[k].point < 0 || obs[k].point >= n_points) { set_error("observation %d references point %d out of range", k, obs[k].point); return LPSLAM_HIP_ERR_INVALID; }
    LP_HIP(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    const BaCam c{cam->fx, cam->fy, cam->cx, cam->cy, cam->focal_x_baseline, cam->huber_mono, cam->huber_stereo};
    const size_t no = (size_t)std::max(n_obs, 1), np = (size_t)std::max(n_points, 1);
    // dynamic LDS: transposed reduction buffer + as many observations as fit beside it + one activity byte per observation
    constexpr size_t kPoLdsBudget = 150 * 1024;
    const size_t fixed_lds = PO_NV * PO_TR * sizeof(double) + no + 64;
    const int cache_n = (int)std::min<size_t>((size_t)n_obs, fixed_lds < kPoLdsBudget ? (kPoLdsBudget - fixed_lds) / sizeof(PoObs) : 0);
    const size_t lds = PO_NV * PO_TR * sizeof(double) + (size_t)cache_n * sizeof(PoObs) + no + 64;
    if (lds > kPoLdsBudget + 4096) { set_error("pose optimiser: %d observations exceed the LDS activity array", n_obs); return LPSLAM_HIP_ERR_CAPACITY; }
    {
        static std::atomic<bool> po_attr[64];
        int dev = 0; (void)hipGetDevice(&dev);
        if (dev >= 0 && dev < 64 && !po_attr[dev].load()) {
            (void)hipFuncSetAttribute((const void*)k_pose_optimize<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kPoLdsBudget + 4096));
            (void)hipFuncSetAttribute((const void*)k_pose_optimize<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kPoLdsBudget + 4096));
            po_attr[dev].store(true);
        }
    }
    const bool all_cached = cache_n == n_obs;
    // page-locked block: pose (in and out) | inlier count | done flag | then either the packed observations and the outlier bytes
    // (all_cached: the kernel works on this block directly) or a mirror of the device block below
    const size_t off_pts = 128, off_obs = off_pts + 3 * np * sizeof(double), off_out = off_obs + no * sizeof(lpslam_hip_ba_obs);
    const size_t off_packed = 128, off_flags = off_packed + no * sizeof(PoObs);
    const size_t need = all_cached ? off_flags + no : off_out + no;
    uint8_t* hb = lp_match_staging(ctx, need, need * 2, s);
    if (!hb) return LPSLAM_HIP_ERR_DEVICE;
    memcpy(hb, pose7, 7 * sizeof(double));
    int32_t inl = 0;
    if (all_cached) {
        PoObs* packed = (PoObs*)(hb + off_packed);
        for (int k = 0; k < n_obs; ++k) {
            const lpslam_hip_ba_obs& o = obs[k];
            const double* p = points + 3 * (size_t)o.point;
            packed[k] = PoObs{o.u, o.v, o.ur, o.inv_sigma2, {p[0], p[1], p[2]}};
        }
        // (no arrival counter: one workgroup signals.  The block is shared with the matchers' staging -- whatever they left in the flag is
        // not a sequence number -- and the flag counts on its own, po_seq)
        LpDone done{};
        { const int rc = lp_done_arm(ctx, LP_NO_COUNTER, (int*)(hb + PO_BLK_FLAG), ctx->po_seq, &done); if (rc) return rc; }
        bool delivered = false;
        if (n_obs <= 256) {
            // a tracked frame: one observation per lane on 1, 2 or 4 wavefronts (k_pose_optimize_req); the camera travels in the block
            memcpy(hb + PO_BLK_CAM, &c, sizeof(BaCam));
            const LpPoseReq req{hb, n_obs, done.seq};
            // several sessions tracking at once: the request joins the others' in one launch (share.hip) and comes back delivered
            const int shared = lp_share_pose(ctx, req, done.flag);
            if (shared < 0) return -shared;
            if (shared == LP_SHARE_DONE) delivered = true;
            else { const int rc = lp_launch_pose_batch(s, &req, 1); if (rc) return rc; }
        } else
        hipLaunchKernelGGL(k_pose_optimize<true>, dim3(1), dim3(PO_T), lds, s, (double*)hb, (const double*)nullptr, (const lpslam_hip_ba_obs*)nullptr, packed, n_obs, c,
                           hb + off_flags, (int*)(hb + 56), cache_n, done.flag, done.seq);
        LP_HIP(hipGetLastError());
        // the kernel's last store releases `seq`: poll it (a few hundred microseconds at most), fall back to the stream when it does not come
        const auto t0 = std::chrono::steady_clock::now();
        if (!delivered && lp_done_wait(ctx, done, s)) { set_error("pose optimiser: the kernel did not complete"); return LPSLAM_HIP_ERR_DEVICE; }
        memcpy(pose7, hb, 7 * sizeof(double));
        memcpy(&inl, hb + 56, sizeof(int));
        memcpy(&ctx->po_passes, hb + 60, sizeof(int));
        {
            static const bool trace = getenv("LPSLAM_HIP_PO_TRACE") != nullptr;
            if (trace) fprintf(stderr, "pose_optimize: %d observations, %d inliers, %d passes, %.1f us\n", n_obs, inl, ctx->po_passes,
                               1e-3 * (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
        }
        if (outlier && n_obs) memcpy(outlier, hb + off_flags, (size_t)n_obs);
        if (n_inliers) *n_inliers = inl;
        return LPSLAM_HIP_OK;
    }
    // more observations than the LDS holds: one block of the context's cache, pose | n_inliers | points | observations | outlier
    LpPoolBlock blk(ctx);
    { const int rc = blk.alloc(off_out + no); if (rc) return rc; }
    uint8_t* base = (uint8_t*)blk.ptr;
    double* d_pose = (double*)base; int* d_n = (int*)(base + 64); double* d_pts = (double*)(base + off_pts);
    lpslam_hip_ba_obs* d_obs = (lpslam_hip_ba_obs*)(base + off_obs); uint8_t* d_out = base + off_out;
    if (n_points) memcpy(hb + off_pts, points, 3 * (size_t)n_points * sizeof(double));
    if (n_obs) memcpy(hb + off_obs, obs, (size_t)n_obs * sizeof(lpslam_hip_ba_obs));
    LP_HIP(hipMemcpyAsync(base, hb, off_out, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pose_optimize<false>, dim3(1), dim3(PO_T), lds, s, d_pose, d_pts, d_obs, (const PoObs*)nullptr, n_obs, c, d_out, d_n, cache_n, (int*)nullptr, 0);
    LP_HIP(hipGetLastError());
    LP_HIP(hipMemcpyAsync(hb, base, 128, hipMemcpyDeviceToHost, s));                    // pose and inlier count
    if (outlier && n_obs) LP_HIP(hipMemcpyAsync(hb + off_out, d_out, (size_t)n_obs, hipMemcpyDeviceToHost, s));
    LP_HIP(hipStreamSynchronize(s));
    memcpy(pose7, hb, 7 * sizeof(double));
    memcpy(&inl, hb + 64, sizeof(int));
    memcpy(&ctx->po_passes, hb + 68, sizeof(int));
    if (outlier && n_obs) memcpy(outlier, hb + off_out, (size_t)n_obs);
    if (n_inliers) *n_inliers = inl;
    return LPSLAM_HIP_OK;
}
int32_t lpslam_hip_pose_optimize_passes(lpslam_hip_ctx* c) { return c ? c->po_passes : 0; }

}  // extern "C"

#ifdef LPSLAM_PO_STAMPS
extern "C" __attribute__((visibility("default"))) int lpslam_hip_debug_po_stamps(double* out16) { return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_po_stamps), 16 * sizeof(double)); }
#endif
