// two_view_math.h -- the arithmetic of the monocular two-view initialiser, once, for the device kernels
// (two_view.hip), the host library (lpslam_amd/host/two_view.cpp, two_view_batch.cpp) and the CPU tests: FP64 throughout, + - * / sqrt
// and comparisons only, so that -- every side built with -ffp-contract=off -- all of them return the same bits.
//   M3, mul, transpose, det, inverse       3 x 3 matrices, row major
//   homography_from_matches<N>              DLT on N matches (N = 8: a RANSAC sample; N = 0: a run-time count, the refit)
//   fundamental_from_matches<N>             eight-point algorithm + rank 2
//   homography_terms / fundamental_terms    one match's two score terms and its inlier flag
//   pose_setup / pose_point                 one match under one motion hypothesis: X, the cosine of its parallax, a code
//   host only: normalize_points (Hartley); the 8-match samples are sample_table<kSample> of ransac_sample.h
// No heap: every array is of fixed size or the caller's.  The 9 x 9 matrix A^T A and its eigenvectors (162 doubles) live in a
// workspace of the caller: element e of it is ws[e * stride].  On the device sixteen lanes of a wave estimate one model together:
// they share the workspace (LDS), divide the 81 sums of A^T A and the independent elements of each Jacobi rotation among them
// (jacobi_math.h); everything else each of them computes for itself, with the same result.
// [UPSTREAM] initialize::perspective, solve::homography_solver, solve::fundamental_solver, initialize::base (see host/two_view.h).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "jacobi_math.h"
#include "triangulate_math.h"

#if defined(__HIPCC__)
#define LP_TV_FN __host__ __device__ inline
#define LP_TV_UNROLL(n) LP_JACOBI_UNROLL(n)
#else
#define LP_TV_FN inline
#define LP_TV_UNROLL(n)
#endif

namespace lpslam_tv {

constexpr int kWorkspace = 162;       // doubles of workspace per model: A^T A, then its eigenvectors
constexpr int kSample = 8;            // matches of a RANSAC sample

struct M3 { double m[9]; };

LP_TV_FN M3 mul(const M3& a, const M3& b)
{
    M3 r;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r.m[i * 3 + j] = a.m[i * 3] * b.m[j] + a.m[i * 3 + 1] * b.m[3 + j] + a.m[i * 3 + 2] * b.m[6 + j];
    return r;
}
LP_TV_FN M3 transpose(const M3& a) { M3 r; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r.m[i * 3 + j] = a.m[j * 3 + i]; return r; }
LP_TV_FN double det(const M3& a)
{
    return a.m[0] * (a.m[4] * a.m[8] - a.m[5] * a.m[7]) - a.m[1] * (a.m[3] * a.m[8] - a.m[5] * a.m[6]) + a.m[2] * (a.m[3] * a.m[7] - a.m[4] * a.m[6]);
}
LP_TV_FN M3 inverse(const M3& a)
{
    const double d = det(a), id = 1.0 / d;
    M3 r;
    r.m[0] = (a.m[4] * a.m[8] - a.m[5] * a.m[7]) * id; r.m[1] = (a.m[2] * a.m[7] - a.m[1] * a.m[8]) * id; r.m[2] = (a.m[1] * a.m[5] - a.m[2] * a.m[4]) * id;
    r.m[3] = (a.m[5] * a.m[6] - a.m[3] * a.m[8]) * id; r.m[4] = (a.m[0] * a.m[8] - a.m[2] * a.m[6]) * id; r.m[5] = (a.m[2] * a.m[3] - a.m[0] * a.m[5]) * id;
    r.m[6] = (a.m[3] * a.m[7] - a.m[4] * a.m[6]) * id; r.m[7] = (a.m[1] * a.m[6] - a.m[0] * a.m[7]) * id; r.m[8] = (a.m[0] * a.m[4] - a.m[1] * a.m[3]) * id;
    return r;
}

// r[k] of a nine-element row held in registers: on the device a chain of selects (a variable index would send the row to scratch)
LP_TV_FN double pick9(const double* r, int k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    double x = r[0];
    LP_TV_UNROLL(8)
    for (int j = 1; j < 9; ++j) x = k == j ? r[j] : x;
    return x;
#else
    return r[k];
#endif
}

// DLT of x2 ~ H x1 on (already normalised) matches: H = the eigenvector of the smallest eigenvalue of A^T A, two rows a match.
// N: the match count when it is a constant of the caller (8), 0: the argument n_run.  ws: kWorkspace doubles at `stride`.
// ln, nl: lane ln of nl lanes of one wave that call this together on one shared ws (jacobi_math.h): the 81 sums are divided among
// them (entry e = ln, ln + nl, ...), each summed over the matches in index order.  Every lane receives H.
template <int N>
LP_TV_FN void homography_from_matches(const double* x1, const double* x2, int n_run, double* ws, int stride, double* H, int ln = 0, int nl = 1)
{
    const int n = N > 0 ? N : n_run;
    double* AtA = ws;
    double* evec = ws + 81 * stride;
    for (int e = ln; e < 81; e += nl) AtA[e * stride] = 0;
    for (int i = 0; i < n; ++i) {
        const double u1 = x1[2 * i], v1 = x1[2 * i + 1], u2 = x2[2 * i], v2 = x2[2 * i + 1];
        const double r1[9] = {0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2};
        const double r2[9] = {u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2};
        for (int e = ln; e < 81; e += nl) {             // (a lane's entries are its own)
            const int a = e / 9, b = e - 9 * a;
            AtA[e * stride] += pick9(r1, a) * pick9(r1, b) + pick9(r2, a) * pick9(r2, b);
        }
    }
    LP_JACOBI_LANES_SYNC();
    int order[9];
    lpslam_jacobi::jacobi<9, 1>(AtA, evec, stride, order, ln, nl);       // ascending
    for (int k = 0; k < 9; ++k) H[k] = evec[(k * 9 + order[0]) * stride];
}

// Eight-point algorithm of x2^T F x1 = 0 on (already normalised) matches, then rank 2: F <- F (I - v3 v3^T), v3 the right singular
// vector of the smallest singular value.  Arguments as above.
template <int N>
LP_TV_FN void fundamental_from_matches(const double* x1, const double* x2, int n_run, double* ws, int stride, double* F, int ln = 0, int nl = 1)
{
    const int n = N > 0 ? N : n_run;
    double* AtA = ws;
    double* evec = ws + 81 * stride;
    for (int e = ln; e < 81; e += nl) AtA[e * stride] = 0;
    for (int i = 0; i < n; ++i) {
        const double u1 = x1[2 * i], v1 = x1[2 * i + 1], u2 = x2[2 * i], v2 = x2[2 * i + 1];
        const double r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1};
        for (int e = ln; e < 81; e += nl) {
            const int a = e / 9, b = e - 9 * a;
            AtA[e * stride] += pick9(r, a) * pick9(r, b);
        }
    }
    LP_JACOBI_LANES_SYNC();
    int order[9];
    lpslam_jacobi::jacobi<9, 1>(AtA, evec, stride, order, ln, nl);
    M3 Fp;
    for (int k = 0; k < 9; ++k) Fp.m[k] = evec[(k * 9 + order[0]) * stride];
    M3 FtF = mul(transpose(Fp), Fp);
    double v3[9];
    int ord3[3];
    lpslam_jacobi::jacobi<3, 3>(FtF.m, v3, 1, ord3);                      // (registers of the lane: every lane for itself)
    double v[3] = {v3[0], v3[3], v3[6]};
    LP_TV_UNROLL(2)
    for (int c = 1; c < 3; ++c) if (ord3[0] == c) { v[0] = v3[c]; v[1] = v3[3 + c]; v[2] = v3[6 + c]; }
    for (int r = 0; r < 3; ++r) {
        const double fv = Fp.m[r * 3] * v[0] + Fp.m[r * 3 + 1] * v[1] + Fp.m[r * 3 + 2] * v[2];
        for (int c = 0; c < 3; ++c) F[r * 3 + c] = Fp.m[r * 3 + c] - fv * v[c];
    }
}

// One match's part of a model's score: the caller adds t1 when add1, then t2 when add2 -- over the matches in index order, the first
// direction before the second: the order of that floating sum is part of the definition.
struct MatchTerms { double t1, t2; int add1, add2, inlier; };

// symmetric transfer error under H21 (reference -> current) and H12 = inverse(H21), chi-square 5.991 at sigma
LP_TV_FN MatchTerms homography_terms(const double* H21, const double* H12, double u1, double v1, double u2, double v2, double inv_s2)
{
    const double th = 5.991;
    MatchTerms r{0, 0, 0, 0, 0};
    bool in = true;
    {   // second image point into the first
        const double w = 1.0 / (H12[6] * u2 + H12[7] * v2 + H12[8]);
        const double x = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w, y = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w;
        const double c = ((u1 - x) * (u1 - x) + (v1 - y) * (v1 - y)) * inv_s2;
        if (c > th) in = false; else { r.t1 = th - c; r.add1 = 1; }
    }
    {   // first image point into the second
        const double w = 1.0 / (H21[6] * u1 + H21[7] * v1 + H21[8]);
        const double x = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w, y = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w;
        const double c = ((u2 - x) * (u2 - x) + (v2 - y) * (v2 - y)) * inv_s2;
        if (c > th) in = false; else { r.t2 = th - c; r.add2 = 1; }
    }
    r.inlier = in ? 1 : 0;
    return r;
}

// distance to the epipolar lines under F21, chi-square 3.841 at sigma (scored against 5.991, as ORB-SLAM does)
LP_TV_FN MatchTerms fundamental_terms(const double* F21, double u1, double v1, double u2, double v2, double inv_s2)
{
    const double th = 3.841, th_score = 5.991;
    MatchTerms r{0, 0, 0, 0, 0};
    bool in = true;
    {   // epipolar line of x1 in the second image: l2 = F21 x1
        const double a = F21[0] * u1 + F21[1] * v1 + F21[2], b = F21[3] * u1 + F21[4] * v1 + F21[5], c = F21[6] * u1 + F21[7] * v1 + F21[8];
        const double num = a * u2 + b * v2 + c;
        const double chi = num * num / (a * a + b * b) * inv_s2;
        if (chi > th) in = false; else { r.t1 = th_score - chi; r.add1 = 1; }
    }
    {   // epipolar line of x2 in the first image: l1 = F21^T x2
        const double a = F21[0] * u2 + F21[3] * v2 + F21[6], b = F21[1] * u2 + F21[4] * v2 + F21[7], c = F21[2] * u2 + F21[5] * v2 + F21[8];
        const double num = a * u1 + b * v1 + c;
        const double chi = num * num / (a * a + b * b) * inv_s2;
        if (chi > th) in = false; else { r.t2 = th_score - chi; r.add2 = 1; }
    }
    r.inlier = in ? 1 : 0;
    return r;
}

// A motion hypothesis (R row major, t: reference -> current) with the camera K = (fx, fy, cx, cy): the two projections, the second centre
struct PoseSetup { double P1[12], P2[12], O2[3]; };
LP_TV_FN void pose_setup(const double* R, const double* t, const double* K, PoseSetup& s)
{
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    const double P1[12] = {fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0};
    for (int k = 0; k < 12; ++k) s.P1[k] = P1[k];
    for (int c = 0; c < 3; ++c) {
        s.P2[c] = fx * R[c] + cx * R[6 + c]; s.P2[4 + c] = fy * R[3 + c] + cy * R[6 + c]; s.P2[8 + c] = R[6 + c];
    }
    s.P2[3] = fx * t[0] + cx * t[2]; s.P2[7] = fy * t[1] + cy * t[2]; s.P2[11] = t[2];
    s.O2[0] = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]); s.O2[1] = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]);
    s.O2[2] = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
}

// One inlier match under the hypothesis (ORB-SLAM CheckRT / OpenVSLAM check_triangulated_pts): 0 = rejected, 1 = counted (X is a
// plausible point, its cosine enters the parallax), 2 = counted and good (enough parallax to become a landmark).  X and *cosp are
// the caller's to use when the code is not 0.
enum { kPoseRejected = 0, kPoseCounted = 1, kPoseGood = 2 };
LP_TV_FN int pose_point(const PoseSetup& s, const double* R, const double* t, const double* K, const double* x1, const double* x2, double th2, double* X, double* cosp_out)
{
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    if (!lpslam_tri::triangulate_linear(s.P1, s.P2, x1[0], x1[1], x2[0], x2[1], X)) return kPoseRejected;
    if (!__builtin_isfinite(X[0]) || !__builtin_isfinite(X[1]) || !__builtin_isfinite(X[2])) return kPoseRejected;
    const double n1 = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    const double d2[3] = {X[0] - s.O2[0], X[1] - s.O2[1], X[2] - s.O2[2]};
    const double n2 = sqrt(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]);
    const double cosp = (X[0] * d2[0] + X[1] * d2[1] + X[2] * d2[2]) / (n1 * n2);
    *cosp_out = cosp;
    if (X[2] <= 0 && cosp < 0.99998) return kPoseRejected;
    const double X2[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1],
                          R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]};
    if (X2[2] <= 0 && cosp < 0.99998) return kPoseRejected;
    const double e1x = fx * X[0] / X[2] + cx - x1[0], e1y = fy * X[1] / X[2] + cy - x1[1];
    if (e1x * e1x + e1y * e1y > th2) return kPoseRejected;
    const double e2x = fx * X2[0] / X2[2] + cx - x2[0], e2y = fy * X2[1] / X2[2] + cy - x2[1];
    if (e2x * e2x + e2y * e2y > th2) return kPoseRejected;
    return cosp < 0.99998 ? kPoseGood : kPoseCounted;
}

// ---- host only from here on (plain inline functions) ---------------------------------------------------------------------------
// Hartley normalisation as ORB-SLAM / OpenVSLAM do it: centroid to the origin, mean absolute deviation 1 per axis (sequential sums).
// in, out: n x 2
inline void normalize_points(const double* in, size_t n, double* out, M3& T)
{
    double mx = 0, my = 0;
    for (size_t i = 0; i < n; ++i) { mx += in[2 * i]; my += in[2 * i + 1]; }
    mx /= (double)n; my /= (double)n;
    double dx = 0, dy = 0;
    for (size_t i = 0; i < n; ++i) { out[2 * i] = in[2 * i] - mx; out[2 * i + 1] = in[2 * i + 1] - my; dx += fabs(out[2 * i]); dy += fabs(out[2 * i + 1]); }
    dx /= (double)n; dy /= (double)n;
    const double sx = 1.0 / dx, sy = 1.0 / dy;
    for (size_t i = 0; i < n; ++i) { out[2 * i] *= sx; out[2 * i + 1] *= sy; }
    T = M3{{sx, 0, -mx * sx, 0, sy, -my * sy, 0, 0, 1}};
}

}  // namespace lpslam_tv
