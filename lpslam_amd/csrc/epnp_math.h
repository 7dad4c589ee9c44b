// epnp_math.h -- the pose of a camera from landmark / keypoint matches (DESIGN.md sections 34 and 35), once, for the device kernels
// (pnp.hip), the host library (lpslam_amd/host/two_view.cpp, pnp_batch.cpp) and the CPU tests: FP64 throughout, + - * / sqrt only, so
// that -- every side built with -ffp-contract=off -- all of them return the same bits.
//   epnp           EPnP on n >= 4 matches; epnp<4> is its instance at n = 4 with the per-match arrays as locals (the device's form)
//   horn           Horn's absolute orientation of n >= 3 matched points, with or without a free scale
//   lsq_small      the small least-squares solves of EPnP's betas
//   pnp_inlier     the scoring rule of the RANSAC around EPnP, pnp_score its count over a set
//   host only:     pnp_solve_sample (one sample's hypothesis) and pnp_refit (EPnP once more over the winner's inliers); the 4-match
//                  samples of LpSlam::pnp_solve_ransac are sample_table<4> of ransac_sample.h
// No heap: every array is of fixed size or the caller's.  The 12 x 12 matrix M^T M and its eigenvectors (288 doubles) live in a
// workspace of the caller: element e of it is ws[e * stride].  On the device sixteen lanes of a wave solve one hypothesis together:
// they share the workspace (LDS) and divide the independent elements of each Jacobi rotation of the 12 x 12 matrix among them
// (jacobi_math.h); everything else each of them computes for itself, with the same result.
//
// [UPSTREAM] solve::pnp_solver (relocalisation without a pose prior).
// EPnP (Lepetit, Moreno-Noguer, Fua: "EPnP: An Accurate O(n) Solution to the PnP Problem", IJCV 2009) inside a RANSAC over 4-match
// samples, then a refit on the inliers of the best sample -- the structure of OpenVSLAM's solver (which follows ORB-SLAM's PnPsolver,
// itself the authors' reference implementation).  The algorithm, as published:
//   1. four control points in the world: the centroid and the centroid plus the principal directions scaled by sqrt(eigenvalue / n);
//   2. every landmark as a barycentric combination of them (alphas, they sum to one);
//   3. the projection equations are linear in the 12 camera-frame coordinates of the control points: M x = 0 (2 n x 12); the solution is
//      a combination x = sum beta_k v_k of the eigenvectors of M^T M with the four smallest eigenvalues;
//   4. the betas from the six pairwise distances of the control points, which the camera frame must preserve (L_6x10 beta_ij = rho):
//      three linearised guesses (N = 1 .. 3 null vectors: approx_1 / _2 / _3), each refined by five Gauss-Newton steps;
//   5. per guess the camera-frame landmarks, the sign that puts them in front of the camera, the rigid motion world -> camera (Horn's
//      absolute orientation here; the reference implementation takes the SVD form), and its mean reprojection error: the best wins.
// Inliers are counted by the reprojection error (chi-square 5.991 at the keypoint's level).  The pose optimiser on the device refines
// the result, as upstream refines EPnP's.  The linear algebra is the Jacobi eigen-solver of jacobi_math.h and small Gaussian
// eliminations, written so that the tests' numpy restatement can follow it operation by operation (both sides then test the same
// hypotheses).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "jacobi_math.h"

#if defined(__HIPCC__)
#define LP_EPNP_FN __host__ __device__ inline
#define LP_EPNP_UNROLL(n) LP_JACOBI_UNROLL(n)
#else
#define LP_EPNP_FN inline
#define LP_EPNP_UNROLL(n)
#endif

namespace lpslam_epnp {

constexpr int kWorkspace = 288;       // doubles of workspace per hypothesis: M^T M, then its eigenvectors

LP_EPNP_FN bool finite(double x) { return __builtin_isfinite(x); }

// least squares A x = b (m x k, k <= 5) by the normal equations and Gaussian elimination with partial pivoting; false when singular
LP_EPNP_FN bool lsq_small(const double* A, const double* b, int m, int k, double* x)
{
    double N[5 * 6];
    for (int i = 0; i < k; ++i) {
        for (int j = 0; j < k; ++j) { double s = 0; for (int r = 0; r < m; ++r) s += A[r * k + i] * A[r * k + j]; N[i * (k + 1) + j] = s; }
        double s = 0;
        for (int r = 0; r < m; ++r) s += A[r * k + i] * b[r];
        N[i * (k + 1) + k] = s;
    }
    for (int c = 0; c < k; ++c) {
        int piv = c;
        for (int r = c + 1; r < k; ++r) if (fabs(N[r * (k + 1) + c]) > fabs(N[piv * (k + 1) + c])) piv = r;
        if (!(fabs(N[piv * (k + 1) + c]) > 1e-300)) return false;
        if (piv != c) for (int j = 0; j <= k; ++j) { const double tmp = N[c * (k + 1) + j]; N[c * (k + 1) + j] = N[piv * (k + 1) + j]; N[piv * (k + 1) + j] = tmp; }
        for (int r = c + 1; r < k; ++r) {
            const double f = N[r * (k + 1) + c] / N[c * (k + 1) + c];
            for (int j = c; j <= k; ++j) N[r * (k + 1) + j] -= f * N[c * (k + 1) + j];
        }
    }
    for (int i = k - 1; i >= 0; --i) {
        double s2 = N[i * (k + 1) + k];
        for (int j = i + 1; j < k; ++j) s2 -= N[i * (k + 1) + j] * x[j];
        x[i] = s2 / N[i * (k + 1) + i];
    }
    return true;
}

// Horn's absolute orientation of n >= 3 matched points: x1 = s R x2 + t (R row major; fix_scale: s = 1).  false: fewer than three
// points, no rotation, or no positive scale -- nothing is written then.  NFIX: the number of points when it is a constant of the
// caller (epnp<4>), 0: it is the argument n_points.
template <int NFIX = 0>
LP_EPNP_FN bool horn(const double* x1, const double* x2, int n_points, bool fix_scale, double* R, double* t, double* s_out)
{
    const int n = NFIX > 0 ? NFIX : n_points;
    if (n < 3) return false;
    double o1[3] = {0, 0, 0}, o2[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) { o1[a] += x1[3 * i + a]; o2[a] += x2[3 * i + a]; }
    for (int a = 0; a < 3; ++a) { o1[a] /= n; o2[a] /= n; }
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};           // M[a][b] = sum (x2 - o2)[a] (x1 - o1)[b]
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) M[a * 3 + b] += (x2[3 * i + a] - o2[a]) * (x1[3 * i + b] - o1[b]);
    double N[16] = {M[0] + M[4] + M[8], M[5] - M[7], M[6] - M[2], M[1] - M[3],
                    M[5] - M[7], M[0] - M[4] - M[8], M[1] + M[3], M[6] + M[2],
                    M[6] - M[2], M[1] + M[3], -M[0] + M[4] - M[8], M[5] + M[7],
                    M[1] - M[3], M[6] + M[2], M[5] + M[7], -M[0] - M[4] + M[8]};
    double evec[16];
    int top;                                                           // the column of the largest eigenvalue
    if constexpr (NFIX == 3) {
        // a lane of the Sim3 kernel holds the 4 x 4 in registers: no index list with its variable indices (they put the matrix into
        // scratch), the last column of the ascending order found directly -- the largest eigenvalue, the later one among equal ones
        lpslam_jacobi::jacobi_sweeps<4, 4, false>(N, evec, 1);
        top = 0;
        double dtop = N[0];
        if (!(N[5] < dtop)) { top = 1; dtop = N[5]; }
        if (!(N[10] < dtop)) { top = 2; dtop = N[10]; }
        if (!(N[15] < dtop)) { top = 3; dtop = N[15]; }
    } else {
        int order[4];
        lpslam_jacobi::jacobi<4, 4>(N, evec, 1, order);                // ascending: the last column belongs to the largest eigenvalue
        top = order[3];
    }
    double q[4];
    q[0] = evec[0]; q[1] = evec[4]; q[2] = evec[8]; q[3] = evec[12];
    LP_EPNP_UNROLL(3)
    for (int c = 1; c < 4; ++c) if (top == c) { q[0] = evec[c]; q[1] = evec[4 + c]; q[2] = evec[8 + c]; q[3] = evec[12 + c]; }
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(qn > 0)) return false;
    for (int k = 0; k < 4; ++k) q[k] /= qn;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double Rm[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                          2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                          2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    double sc = 1.0;
    if (!fix_scale) {
        double nom = 0, den = 0;
        for (int i = 0; i < n; ++i) {
            double p3[3];
            for (int r = 0; r < 3; ++r) p3[r] = Rm[r * 3] * (x2[3 * i] - o2[0]) + Rm[r * 3 + 1] * (x2[3 * i + 1] - o2[1]) + Rm[r * 3 + 2] * (x2[3 * i + 2] - o2[2]);
            for (int r = 0; r < 3; ++r) { nom += (x1[3 * i + r] - o1[r]) * p3[r]; den += p3[r] * p3[r]; }
        }
        if (!(den > 0) || !(nom > 0)) return false;
        sc = nom / den;
    }
    for (int k = 0; k < 9; ++k) R[k] = Rm[k];
    for (int r = 0; r < 3; ++r) t[r] = o1[r] - sc * (Rm[r * 3] * o2[0] + Rm[r * 3 + 1] * o2[1] + Rm[r * 3 + 2] * o2[2]);
    *s_out = sc;
    return true;
}

LP_EPNP_FN double dot3(const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// EPnP (the steps in the comment at the top).  pw: n x 3 landmarks (world), uv: n x 2 keypoints (pixels), cam: fx fy cx cy; ws:
// kWorkspace doubles, element e at ws[e * stride].  true: R (row major, world -> camera) and t are written; false: fewer than four
// matches or degenerate input.
// NFIX: the number of matches when it is a constant of the caller -- the RANSAC's 4, on the device and on the host -- 0: it is the
// argument n_matches.  The per-match arrays, the alphas al (4 n doubles) and the camera-frame landmarks pc (3 n), are locals at a
// constant n (al and pc are not read, pass null) and the caller's scratch otherwise.  (The kernel calls epnp<4> itself, and the
// arrays are declared here, because k_pnp_hypotheses was found to keep its code only so: a wrapper in between, or arrays handed in,
// moved its register allocation.)
// ln, nl: as for jacobi_sweeps (jacobi_math.h) -- nl lanes of a wave call this together with the same arguments and one workspace; each
// returns the result.
template <int NFIX = 0>
LP_EPNP_FN bool epnp(const double* pw, const double* uv, int n_matches, const double* cam, double* al, double* pc, double* ws, int stride, double* R, double* t,
                     int ln = 0, int nl = 1)
{
    const int n = NFIX > 0 ? NFIX : n_matches;
    double al_fixed[NFIX > 0 ? 4 * NFIX : 1], pc_fixed[NFIX > 0 ? 3 * NFIX : 1];
    if (NFIX > 0) { al = al_fixed; pc = pc_fixed; }
    if (n < 4) return false;
    const double fu = cam[0], fv = cam[1], uc = cam[2], vc = cam[3];
    // 1. control points
    double cws[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) cws[0][a] += pw[3 * i + a];
    for (int a = 0; a < 3; ++a) cws[0][a] /= n;
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) for (int b2 = 0; b2 < 3; ++b2) C[a * 3 + b2] += (pw[3 * i + a] - cws[0][a]) * (pw[3 * i + b2] - cws[0][b2]);
    double evec[9];
    int ord3[3];
    lpslam_jacobi::jacobi<3, 3>(C, evec, 1, ord3);                       // ascending; the principal direction first, as the published code orders them
    for (int j = 1; j <= 3; ++j) {
        const int col = ord3[3 - j];
        const double e = C[col * 4];
        const double k = sqrt((e < 0.0 ? 0.0 : e) / n);
        for (int a = 0; a < 3; ++a) cws[j][a] = cws[0][a] + k * evec[a * 3 + col];
    }
    // 2. barycentric coordinates: [c1 - c0, c2 - c0, c3 - c0] a = p - c0
    double CC[9], CI[9];
    for (int a = 0; a < 3; ++a) for (int j = 1; j <= 3; ++j) CC[a * 3 + (j - 1)] = cws[j][a] - cws[0][a];
    const double det = CC[0] * (CC[4] * CC[8] - CC[5] * CC[7]) - CC[1] * (CC[3] * CC[8] - CC[5] * CC[6]) + CC[2] * (CC[3] * CC[7] - CC[4] * CC[6]);
    if (!(fabs(det) > 1e-300)) return false;                // landmarks in a plane or on a line: no volume to span
    CI[0] = (CC[4] * CC[8] - CC[5] * CC[7]) / det; CI[1] = (CC[2] * CC[7] - CC[1] * CC[8]) / det; CI[2] = (CC[1] * CC[5] - CC[2] * CC[4]) / det;
    CI[3] = (CC[5] * CC[6] - CC[3] * CC[8]) / det; CI[4] = (CC[0] * CC[8] - CC[2] * CC[6]) / det; CI[5] = (CC[2] * CC[3] - CC[0] * CC[5]) / det;
    CI[6] = (CC[3] * CC[7] - CC[4] * CC[6]) / det; CI[7] = (CC[1] * CC[6] - CC[0] * CC[7]) / det; CI[8] = (CC[0] * CC[4] - CC[1] * CC[3]) / det;
    for (int i = 0; i < n; ++i) {
        const double d0 = pw[3 * i] - cws[0][0], d1 = pw[3 * i + 1] - cws[0][1], d2 = pw[3 * i + 2] - cws[0][2];
        for (int j = 0; j < 3; ++j) al[4 * i + 1 + j] = CI[j * 3] * d0 + CI[j * 3 + 1] * d1 + CI[j * 3 + 2] * d2;
        al[4 * i] = 1.0 - al[4 * i + 1] - al[4 * i + 2] - al[4 * i + 3];
    }
    // 3. M^T M, accumulated row pair by row pair
    double* MtM = ws;
    double* mvec = ws + 144 * stride;
    for (int e = ln; e < 144; e += nl) MtM[e * stride] = 0;
    LP_JACOBI_LANES_SYNC();
    for (int i = 0; i < n; ++i) {
        double r1[12], r2[12];
        for (int j = 0; j < 4; ++j) {
            const double a = al[4 * i + j];
            r1[3 * j] = a * fu; r1[3 * j + 1] = 0.0;    r1[3 * j + 2] = a * (uc - uv[2 * i]);
            r2[3 * j] = 0.0;    r2[3 * j + 1] = a * fv; r2[3 * j + 2] = a * (vc - uv[2 * i + 1]);
        }
        for (int a = ln; a < 12; a += nl) for (int b2 = 0; b2 < 12; ++b2) MtM[(a * 12 + b2) * stride] += r1[a] * r1[b2] + r2[a] * r2[b2];      // (a lane's rows are its own)
    }
    LP_JACOBI_LANES_SYNC();
    int ord12[12];
    lpslam_jacobi::jacobi<12, 1>(MtM, mvec, stride, ord12, ln, nl);       // ascending: columns 0 .. 3 span the (approximate) null space
    double v[4][12];
    for (int k = 0; k < 4; ++k) for (int a = 0; a < 12; ++a) v[k][a] = mvec[(a * 12 + ord12[k]) * stride];
    // 4. distance constraints
    const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
    double dv[4][6][3], L[60], rho[6];
    for (int k = 0; k < 4; ++k) for (int p = 0; p < 6; ++p) for (int a = 0; a < 3; ++a) dv[k][p][a] = v[k][3 * pa[p] + a] - v[k][3 * pb[p] + a];
    for (int p = 0; p < 6; ++p) {
        double* row = L + 10 * p;
        row[0] = dot3(dv[0][p], dv[0][p]); row[1] = 2.0 * dot3(dv[0][p], dv[1][p]); row[2] = dot3(dv[1][p], dv[1][p]);
        row[3] = 2.0 * dot3(dv[0][p], dv[2][p]); row[4] = 2.0 * dot3(dv[1][p], dv[2][p]); row[5] = dot3(dv[2][p], dv[2][p]);
        row[6] = 2.0 * dot3(dv[0][p], dv[3][p]); row[7] = 2.0 * dot3(dv[1][p], dv[3][p]); row[8] = 2.0 * dot3(dv[2][p], dv[3][p]);
        row[9] = dot3(dv[3][p], dv[3][p]);
        double d2 = 0;
        for (int a = 0; a < 3; ++a) { const double d = cws[pa[p]][a] - cws[pb[p]][a]; d2 += d * d; }
        rho[p] = d2;
    }
    double best_err = 1e300;
    bool found = false;
    for (int guess = 0; guess < 3; ++guess) {
        double be[4] = {0, 0, 0, 0};
        if (guess == 0) {                                   // betas 11 12 13 14 (columns 0, 1, 3, 6): N = 4 with the cross terms of beta_1 only
            double A[24], x4[4];
            for (int p = 0; p < 6; ++p) { A[4 * p] = L[10 * p]; A[4 * p + 1] = L[10 * p + 1]; A[4 * p + 2] = L[10 * p + 3]; A[4 * p + 3] = L[10 * p + 6]; }
            if (!lsq_small(A, rho, 6, 4, x4)) continue;
            if (x4[0] < 0) { be[0] = sqrt(-x4[0]); be[1] = -x4[1] / be[0]; be[2] = -x4[2] / be[0]; be[3] = -x4[3] / be[0]; }
            else { be[0] = sqrt(x4[0]); be[1] = x4[1] / be[0]; be[2] = x4[2] / be[0]; be[3] = x4[3] / be[0]; }
        } else if (guess == 1) {                            // betas 11 12 22 (columns 0, 1, 2): N = 2
            double A[18], x3[3];
            for (int p = 0; p < 6; ++p) { A[3 * p] = L[10 * p]; A[3 * p + 1] = L[10 * p + 1]; A[3 * p + 2] = L[10 * p + 2]; }
            if (!lsq_small(A, rho, 6, 3, x3)) continue;
            if (x3[0] < 0) { be[0] = sqrt(-x3[0]); be[1] = x3[2] < 0 ? sqrt(-x3[2]) : 0.0; }
            else { be[0] = sqrt(x3[0]); be[1] = x3[2] > 0 ? sqrt(x3[2]) : 0.0; }
            if (x3[1] < 0) be[0] = -be[0];
        } else {                                            // betas 11 12 22 13 23 (columns 0 .. 4): N = 3
            double A[30], x5[5];
            for (int p = 0; p < 6; ++p) for (int c = 0; c < 5; ++c) A[5 * p + c] = L[10 * p + c];
            if (!lsq_small(A, rho, 6, 5, x5)) continue;
            if (x5[0] < 0) { be[0] = sqrt(-x5[0]); be[1] = x5[2] < 0 ? sqrt(-x5[2]) : 0.0; }
            else { be[0] = sqrt(x5[0]); be[1] = x5[2] > 0 ? sqrt(x5[2]) : 0.0; }
            if (x5[1] < 0) be[0] = -be[0];
            be[2] = x5[3] / be[0];
        }
        if (!(be[0] == be[0]) || !finite(be[0]) || !finite(be[1]) || !finite(be[2]) || !finite(be[3])) continue;
        bool gn_ok = true;
        for (int it = 0; it < 5 && gn_ok; ++it) {           // Gauss-Newton on the six distance equations
            double A[24], r6[6], dx[4];
            for (int p = 0; p < 6; ++p) {
                const double* l = L + 10 * p;
                A[4 * p] = 2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
                A[4 * p + 1] = l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
                A[4 * p + 2] = l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3];
                A[4 * p + 3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3];
                r6[p] = rho[p] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] +
                                  l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
            }
            if (!lsq_small(A, r6, 6, 4, dx)) { gn_ok = false; break; }
            for (int k = 0; k < 4; ++k) be[k] += dx[k];
        }
        if (!gn_ok || !finite(be[0]) || !finite(be[1]) || !finite(be[2]) || !finite(be[3])) continue;
        // 5. camera-frame control points and landmarks, sign, rigid motion, reprojection error
        double ccs[4][3];
        for (int j = 0; j < 4; ++j) for (int a = 0; a < 3; ++a) ccs[j][a] = be[0] * v[0][3 * j + a] + be[1] * v[1][3 * j + a] + be[2] * v[2][3 * j + a] + be[3] * v[3][3 * j + a];
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) pc[3 * i + a] = al[4 * i] * ccs[0][a] + al[4 * i + 1] * ccs[1][a] + al[4 * i + 2] * ccs[2][a] + al[4 * i + 3] * ccs[3][a];
        if (pc[2] < 0) for (int k = 0; k < 3 * n; ++k) pc[k] = -pc[k];      // the first landmark in front of the camera
        double Rg[9], tg[3], unit;
        if (!horn<NFIX>(pc, pw, n, true, Rg, tg, &unit)) continue;
        double err = 0;
        bool fin = true;
        for (int i = 0; i < n; ++i) {
            const double* X = pw + 3 * i;
            const double xc = Rg[0] * X[0] + Rg[1] * X[1] + Rg[2] * X[2] + tg[0], yc = Rg[3] * X[0] + Rg[4] * X[1] + Rg[5] * X[2] + tg[1], zc = Rg[6] * X[0] + Rg[7] * X[1] + Rg[8] * X[2] + tg[2];
            const double du = uc + fu * xc / zc - uv[2 * i], dv2 = vc + fv * yc / zc - uv[2 * i + 1];
            const double e = sqrt(du * du + dv2 * dv2);
            if (!finite(e)) { fin = false; break; }
            err += e;
        }
        if (!fin) continue;
        err /= n;
        if (err < best_err) { best_err = err; found = true; for (int k = 0; k < 9; ++k) R[k] = Rg[k]; for (int k = 0; k < 3; ++k) t[k] = tg[k]; }
    }
    return found;
}

// The RANSAC's inlier rule for one match: landmark X, keypoint (u, v) with weight inv_sigma2 = 1 / scale^2 of its level
LP_EPNP_FN bool pnp_inlier(const double* R, const double* t, const double* cam, const double* X, double u, double v, double inv_sigma2)
{
    const double xc = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], yc = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    const double du = cam[0] * xc / z + cam[2] - u, dv = cam[1] * yc / z + cam[3] - v;
    return z > 0 && (du * du + dv * dv) * inv_sigma2 < 5.991;
}

// ---- host only from here on (plain inline functions) ---------------------------------------------------------------------------
// The hypothesis of one sample: EPnP on the four matches idx names
inline bool pnp_solve_sample(const double* pw, const double* obs, const int32_t* idx, const double* cam, double* R, double* t)
{
    double p4[12], u4[8], ws[kWorkspace];
    for (int k = 0; k < 4; ++k) { const size_t m = (size_t)idx[k]; for (int a = 0; a < 3; ++a) p4[3 * k + a] = pw[3 * m + a]; u4[2 * k] = obs[2 * m]; u4[2 * k + 1] = obs[2 * m + 1]; }
    return epnp<4>(p4, u4, 4, cam, nullptr, nullptr, ws, 1, R, t);
}

// The inliers of a pose among n matches: their number, flags[i] = 1 for each
inline int pnp_score(const double* R, const double* t, const double* cam, const double* pw, const double* obs, const double* inv_sigma2, int n, uint8_t* flags)
{
    int count = 0;
    for (int i = 0; i < n; ++i) { flags[i] = pnp_inlier(R, t, cam, pw + 3 * (size_t)i, obs[2 * (size_t)i], obs[2 * (size_t)i + 1], inv_sigma2[i]) ? 1 : 0; count += flags[i]; }
    return count;
}

// The refit on the inliers of the best sample ([UPSTREAM] refine): EPnP over all of them, kept when it explains at least as many
// matches as the sample's `best` -- then inlier, R and t are replaced and the new count is returned; `best` otherwise.
// scratch: 12 n doubles (the inliers' landmarks and keypoints, EPnP's alphas and camera-frame landmarks), cur: n flags.
inline int pnp_refit(const double* pw, const double* obs, const double* inv_sigma2, int n, const double* cam, int best, uint8_t* inlier, double* R, double* t,
                     double* scratch, uint8_t* cur)
{
    double* pi = scratch; double* ui = pi + 3 * (size_t)n; double* al = ui + 2 * (size_t)n; double* pc = al + 4 * (size_t)n;
    int m = 0;
    for (int i = 0; i < n; ++i) if (inlier[i]) { for (int a = 0; a < 3; ++a) pi[3 * (size_t)m + a] = pw[3 * (size_t)i + a]; ui[2 * (size_t)m] = obs[2 * (size_t)i]; ui[2 * (size_t)m + 1] = obs[2 * (size_t)i + 1]; ++m; }
    double ws[kWorkspace], Rr[9], tr[3];
    if (!epnp(pi, ui, m, cam, al, pc, ws, 1, Rr, tr)) return best;
    const int count = pnp_score(Rr, tr, cam, pw, obs, inv_sigma2, n, cur);
    if (count < best) return best;
    for (int i = 0; i < n; ++i) inlier[i] = cur[i];
    for (int k = 0; k < 9; ++k) R[k] = Rr[k];
    for (int k = 0; k < 3; ++k) t[k] = tr[k];
    return count;
}

}  // namespace lpslam_epnp
