// pose_cov_math.h -- the covariance of a pose the motion-only optimiser returned, once, for the device kernel
// (pose_cov.hip), the host library (lpslam_amd/host/pose_cov_batch.cpp) and the CPU tests: FP64 throughout, + - * / sqrt only, IEEE
// division and square root, so that -- every side built with -ffp-contract=off -- all of them return the same bits.
//   obs_add        one observation's share of the 22 sums: the upper triangle of H = sum w B^T B (row by row, the order of the pose
//                  optimiser's po_accumulate) and chi2 = sum w |e|^2, at the pose (R, t); residual and Jacobian rows are those of
//                  po_residual / po_jacobian (pose_opt.hip), weight w = inv_sigma2, no Huber
//   fold           the fixed binary tree over the kLanes partial sums of one value
//   set_sums       the sums of one set in the stated order (what the host runs; the kernel does the same additions on 256 lanes)
//   invert         Sigma = H^-1 through the Cholesky factor of the diagonally scaled matrix, with the status rules
//   pose_sigmas    Sigma -> the interface's x_sigma, y_sigma, z_sigma (lpslam axes) and orientation sigma (radians)
// The order of the sums: lane l of kLanes adds the active observations k = l, l + kLanes, ... of its set in ascending k onto 0.0; the
// kLanes partial sums are folded with strides kLanes / 2, ..., 1, v[l] += v[l + stride].  No heap, no state.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "jacobi_math.h"

#if defined(__HIPCC__)
#define LP_PCOV_FN __host__ __device__ inline
#define LP_PCOV_PRAGMA(x) _Pragma(#x)
#define LP_PCOV_UNROLL LP_PCOV_PRAGMA(unroll)       // constant indices: the 6 x 6 matrices stay in registers on the device
#else
#define LP_PCOV_FN inline
#define LP_PCOV_UNROLL
#endif

namespace lpslam_pose_cov {

constexpr int kLanes = 256;                // partial sums per value
constexpr int kSums = 22;                  // 21 entries of H (upper triangle, row by row), chi2
constexpr int kObsDoubles = 7;             // u v ur inv_sigma2 X Y Z
constexpr int kMaxSets = 4096;
constexpr int kMaxObs = 1 << 18;
constexpr double kMinPivot = 1e-8;         // a pivot of the scaled factorisation at or below this refuses the set
enum { kOk = 0, kTooFew = 1, kRefused = 2 };
enum { kArgsOk = 0, kArgsInvalid = 1, kArgsCapacity = 3 };      // LPSLAM_HIP_OK, LPSLAM_HIP_ERR_INVALID, LPSLAM_HIP_ERR_CAPACITY

// The argument rules of both batch calls, in front of any allocation; *why names the rule that refused.
inline int check_args(int32_t n_sets, const int32_t* set_start, const void* pose7, const void* obs, const void* active, const void* cam, const void* info21,
                      const void* cov21, const void* chi2, const void* min_pivot, const void* n_used, const void* status, int* first, int* total, const char** why)
{
    *first = 0; *total = 0; *why = "";
    if (!set_start || !pose7 || !cam || !info21 || !cov21 || !chi2 || !min_pivot || !n_used || !status) { *why = "null argument"; return kArgsInvalid; }
    if (n_sets < 1) { *why = "fewer than one set"; return kArgsInvalid; }
    if (n_sets > kMaxSets) { *why = "more than 4096 sets"; return kArgsCapacity; }
    if (set_start[0] < 0) { *why = "set_start begins below 0"; return kArgsInvalid; }
    for (int i = 0; i < n_sets; ++i) if (set_start[i + 1] < set_start[i]) { *why = "set_start does not ascend"; return kArgsInvalid; }
    const int64_t n = (int64_t)set_start[n_sets] - (int64_t)set_start[0];
    if (n > kMaxObs) { *why = "more than 1 << 18 observations"; return kArgsCapacity; }
    if (n > 0 && (!obs || !active)) { *why = "null argument"; return kArgsInvalid; }
    *first = set_start[0]; *total = (int)n;
    return kArgsOk;
}

// rotation matrix (row major) of the normalised quaternion q = w x y z
LP_PCOV_FN void quat_to_rot(const double* q, double* R)
{
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// One observation o = u v ur inv_sigma2 X Y Z at the pose (R, t), cam = fx fy cx cy fxb: acc[i] += its i-th term.  false: the point is
// not in front of the camera (pc_z not above 0), nothing added and the observation does not count.
LP_PCOV_FN bool obs_add(const double* R, const double* t, const double* cam, const double* o, double* acc)
{
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], fxb = cam[4];
    const double* X = o + 4;
    double pc[3];
    LP_PCOV_UNROLL
    for (int i = 0; i < 3; ++i) pc[i] = R[i * 3] * X[0] + R[i * 3 + 1] * X[1] + R[i * 3 + 2] * X[2] + t[i];
    if (!(pc[2] > 0.0)) return false;
    const double x = pc[0], y = pc[1], iz = 1.0 / pc[2], iz2 = iz * iz;
    const double u = fx * x * iz + cx, v = fy * y * iz + cy;
    const bool stereo = !(o[2] < 0.0);
    double e[3];
    e[0] = o[0] - u; e[1] = o[1] - v; e[2] = stereo ? o[2] - (u - fxb * iz) : 0.0;
    double B[3][6];
    B[0][0] = x * y * iz2 * fx;           B[0][1] = -(1.0 + x * x * iz2) * fx;   B[0][2] = y * iz * fx;
    B[0][3] = -iz * fx;                   B[0][4] = 0.0;                          B[0][5] = x * iz2 * fx;
    B[1][0] = (1.0 + y * y * iz2) * fy;   B[1][1] = -(x * y * iz2) * fy;          B[1][2] = -(x * iz) * fy;
    B[1][3] = 0.0;                        B[1][4] = -iz * fy;                     B[1][5] = y * iz2 * fy;
    if (stereo) {
        B[2][0] = B[0][0] - fxb * y * iz2; B[2][1] = B[0][1] + fxb * x * iz2;     B[2][2] = B[0][2];
        B[2][3] = B[0][3];                 B[2][4] = 0.0;                          B[2][5] = B[0][5] - fxb * iz2;
    } else {
        LP_PCOV_UNROLL
        for (int k = 0; k < 6; ++k) B[2][k] = 0.0;
    }
    const double w = o[3];
    double wB[3][6];
    LP_PCOV_UNROLL
    for (int r = 0; r < 3; ++r) {
        LP_PCOV_UNROLL
        for (int a = 0; a < 6; ++a) wB[r][a] = w * B[r][a];
    }
    int idx = 0;
    LP_PCOV_UNROLL
    for (int a = 0; a < 6; ++a) {
        LP_PCOV_UNROLL
        for (int c = a; c < 6; ++c) {
            const double term = wB[0][a] * B[0][c] + wB[1][a] * B[1][c] + wB[2][a] * B[2][c];
            acc[idx] = acc[idx] + term;
            ++idx;
        }
    }
    acc[21] = acc[21] + w * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    return true;
}

// the fixed tree over kLanes values `stride` doubles apart: the total ends in v[0]
LP_PCOV_FN void fold(double* v, int stride)
{
    for (int s = kLanes / 2; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) v[(size_t)l * stride] += v[(size_t)(l + s) * stride];
}

// The 22 sums and the number of observations used of one set of n observations (obs: 7 doubles each, active: 1 = use) at pose7.
// partial: kLanes x kSums doubles of the caller's.
LP_PCOV_FN int set_sums(const double* pose7, const double* cam, const double* obs, const uint8_t* active, int n, double* partial, double* sums)
{
    double R[9];
    quat_to_rot(pose7, R);
    int used = 0;
    for (int l = 0; l < kLanes; ++l) {
        double* acc = partial + (size_t)l * kSums;
        for (int q = 0; q < kSums; ++q) acc[q] = 0.0;
        for (int k = l; k < n; k += kLanes)
            if (active[k] == 1 && obs_add(R, pose7 + 4, cam, obs + (size_t)kObsDoubles * k, acc)) ++used;
    }
    for (int q = 0; q < kSums; ++q) { fold(partial + q, kSums); sums[q] = partial[q]; }
    return used;
}

// Sigma = H^-1 of the 21 sums h (upper triangle, row by row) of n_used observations: A = D H D with D = diag(H)^-1/2, A = L L^T,
// A^-1 = L^-T L^-1, Sigma = D A^-1 D -- cov receives its upper triangle in the same order, *min_pivot the smallest pivot (L_jj^2, in
// (0, 1] for a positive definite H) met.  Returns kTooFew (n_used < 3, whatever else holds); kRefused (a diagonal entry of H not positive
// or not finite, or a pivot not above kMinPivot); else kOk.  Anything but kOk: cov = 21 zeros.  *min_pivot is defined wherever the
// diagonal let the factorisation begin -- at a refusing pivot it is that pivot -- and 0 otherwise.
LP_PCOV_FN int invert(const double* h, int n_used, double* cov, double* min_pivot)
{
    LP_PCOV_UNROLL
    for (int i = 0; i < 21; ++i) cov[i] = 0.0;
    *min_pivot = 0.0;
    const bool few = n_used < 3;
    double A[6][6], d[6];
    {
        int idx = 0;
        LP_PCOV_UNROLL
        for (int a = 0; a < 6; ++a) {
            LP_PCOV_UNROLL
            for (int c = a; c < 6; ++c) { A[a][c] = h[idx]; A[c][a] = h[idx]; ++idx; }
        }
    }
    bool good = true;
    LP_PCOV_UNROLL
    for (int i = 0; i < 6; ++i) {
        const double v = A[i][i];
        if (!(v > 0.0) || !(v <= 1.7976931348623157e308)) good = false;
        d[i] = 1.0 / sqrt(v);
    }
    if (!good) return few ? kTooFew : kRefused;
    LP_PCOV_UNROLL
    for (int i = 0; i < 6; ++i) {
        LP_PCOV_UNROLL
        for (int j = 0; j < 6; ++j) A[i][j] = d[i] * A[i][j] * d[j];
    }
    // Cholesky, column by column: L in the lower triangle of A
    double piv_min = 2.0;
    LP_PCOV_UNROLL
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        LP_PCOV_UNROLL
        for (int k = 0; k < j; ++k) s = s - A[j][k] * A[j][k];
        if (good && (s < piv_min || !(s == s))) piv_min = s;
        if (!(s > kMinPivot)) good = false;
        const double l = sqrt(s);
        A[j][j] = l;
        LP_PCOV_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            LP_PCOV_UNROLL
            for (int k = 0; k < j; ++k) v = v - A[i][k] * A[j][k];
            A[i][j] = v / l;
        }
    }
    *min_pivot = piv_min;
    if (few) return kTooFew;
    if (!good) return kRefused;
    // M = L^-1 (lower triangle)
    double M[6][6];
    LP_PCOV_UNROLL
    for (int j = 0; j < 6; ++j) {
        M[j][j] = 1.0 / A[j][j];
        LP_PCOV_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double v = 0.0;
            LP_PCOV_UNROLL
            for (int k = j; k < i; ++k) v = v + A[i][k] * M[k][j];
            M[i][j] = -v / A[i][i];
        }
    }
    // Sigma = D (M^T M) D
    int idx = 0;
    LP_PCOV_UNROLL
    for (int a = 0; a < 6; ++a) {
        LP_PCOV_UNROLL
        for (int c = a; c < 6; ++c) {
            double v = 0.0;
            LP_PCOV_UNROLL
            for (int k = c; k < 6; ++k) v = v + M[k][a] * M[k][c];
            cov[idx] = d[a] * v * d[c];
            ++idx;
        }
    }
    return kOk;
}

// entry (a, c) of the symmetric 6 x 6 matrix kept as its upper triangle row by row
LP_PCOV_FN double sym6(const double* m21, int a, int c)
{
    const int lo = a < c ? a : c, hi = a < c ? c : a;
    return m21[lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)];
}

// cov21 (tangent space of T <- exp(d) T, d = (omega, upsilon)) -> out4 = x_sigma, y_sigma, z_sigma, orientation sigma.  The camera
// centre C = -R^T t moves by -R^T upsilon to first order, so Sigma_C = R^T Sigma_uu R; in lpslam axes (position = (-C_y, C_x, C_z))
// x_sigma = sqrt(Sigma_C[1][1]), y_sigma = sqrt(Sigma_C[0][0]), z_sigma = sqrt(Sigma_C[2][2]).  The orientation sigma is the square root
// of the largest eigenvalue of Sigma_ww (radians; the shared Jacobi solver).  A variance that is not above 0 gives sigma 0.
LP_PCOV_FN void pose_sigmas(const double* pose7, const double* cov21, double* out4)
{
    double R[9], var[3];
    quat_to_rot(pose7, R);
    for (int i = 0; i < 3; ++i) {
        double s = 0.0;
        for (int a = 0; a < 3; ++a) {
            double tmp = 0.0;
            for (int b = 0; b < 3; ++b) tmp = tmp + sym6(cov21, 3 + a, 3 + b) * R[b * 3 + i];
            s = s + R[a * 3 + i] * tmp;
        }
        var[i] = s;
    }
    out4[0] = var[1] > 0.0 ? sqrt(var[1]) : 0.0;
    out4[1] = var[0] > 0.0 ? sqrt(var[0]) : 0.0;
    out4[2] = var[2] > 0.0 ? sqrt(var[2]) : 0.0;
    double a[9], v[9];
    int order[3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) a[i * 3 + j] = sym6(cov21, i, j);
    lpslam_jacobi::jacobi<3, 3>(a, v, 1, order);
    const double top = a[order[2] * 3 + order[2]];
    out4[3] = top > 0.0 ? sqrt(top) : 0.0;
}

}  // namespace lpslam_pose_cov
