// epnp_math.h -- the pose of a camera from exactly four landmark / keypoint matches, once, for the device
// kernels (pnp.hip), the host shims (lpslam_amd/host/pnp_batch.cpp) and the CPU tests: FP64 throughout.
//   epnp4          the fixed-size form of LpSlam::epnp_solve (lpslam_amd/host/two_view.cpp) at n = 4: the same operations in the same
//                  order with the same thresholds, so that -- both sides built with -ffp-contract=off, + - * / sqrt correctly
//                  rounded on both -- its R, t and return value are those of epnp_solve to the last bit
//   pnp_inlier     the scoring rule of pnp_solve_ransac's count_inliers
//   sample_table   the 4-match samples pnp_solve_ransac draws (host only: the draw is sequential by definition)
// [UPSTREAM] solve::pnp_solver; EPnP: Lepetit, Moreno-Noguer, Fua, IJCV 2009 (see the comment in front of epnp_solve).
// No heap, every array of fixed size, every loop with the host's own fixed bound.  The 12 x 12 matrix M^T M and its eigenvectors
// (288 doubles) live in a workspace of the caller: element e of it is ws[e * stride] -- stride 1 on the host, the number of
// workspace's element stride on the device.  There sixteen lanes of a wave solve one hypothesis together: they share the workspace (LDS)
// and divide the independent elements of each Jacobi rotation of the 12 x 12 matrix among them (jacobi, below); everything else each
// of them computes for itself, with the same result.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LP_EPNP_FN __host__ __device__ inline
#define LP_EPNP_PRAGMA(x) _Pragma(#x)
#define LP_EPNP_UNROLL(n) LP_EPNP_PRAGMA(unroll n)      // constant indices: the small matrices stay in registers on the device
#else
#define LP_EPNP_FN inline
#define LP_EPNP_UNROLL(n)
#endif
// Lanes of one wave that work on one workspace together (below): what a lane wrote to it is read by its neighbours from here on.  A
// wave's LDS instructions execute in their order; this keeps the compiler from moving or caching accesses across the point.
#if defined(__HIP_DEVICE_COMPILE__)
#define LP_EPNP_LANES_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#else
#define LP_EPNP_LANES_SYNC() do { } while (0)
#endif

namespace lpslam_epnp {

constexpr int kWorkspace = 288;       // doubles of workspace per hypothesis: M^T M, then its eigenvectors

LP_EPNP_FN bool finite(double x) { return __builtin_isfinite(x); }

// sym_eigen_jacobi of lpslam_amd/host/two_view.cpp on an N x N matrix, in place: a (row major, element (i, j) at a[(i * N + j) * st])
// ends with the eigenvalues on its diagonal, v receives the eigenvectors as columns; at most 64 sweeps.  order[c] = the column of the
// c-th smallest eigenvalue: the host sorts with std::sort, which for 16 elements or fewer is libstdc++'s insertion sort -- the first
// among equal eigenvalues stays first -- and that sort is written out here comparison by comparison.
// UNROLL: the loop bodies are expanded so that every index is a constant (N = 3, 4); the 12 x 12 matrix keeps its loops.
// ln, nl: lane ln of nl lanes of one wave that call this together on one (shared) a and v with the same values: the elements of a
// rotation -- independent of each other -- are divided among them (k = ln, ln + nl, ...), everything else every lane computes for
// itself.  Each element is computed by the same operations either way; the host and the small matrices run with one lane.
template <int N, int UNROLL>
LP_EPNP_FN void jacobi(double* a, double* v, int st, int* order, int ln = 0, int nl = 1)
{
    for (int i = ln; i < N * N; i += nl) v[i * st] = 0.0;
    LP_EPNP_LANES_SYNC();
    for (int i = ln; i < N; i += nl) v[(i * N + i) * st] = 1.0;
    LP_EPNP_LANES_SYNC();
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0, diag = 0;
        LP_EPNP_UNROLL(UNROLL)
        for (int i = 0; i < N; ++i)
            LP_EPNP_UNROLL(UNROLL)
            for (int j = 0; j < N; ++j) { const double x = a[(i * N + j) * st]; if (i == j) diag += x * x; else off += x * x; }
        if (off <= 1e-30 * (diag + 1e-300)) break;
        LP_EPNP_UNROLL(UNROLL)
        for (int p = 0; p < N - 1; ++p)
            LP_EPNP_UNROLL(UNROLL)
            for (int q = p + 1; q < N; ++q) {
                const double apq = a[(p * N + q) * st];
                if (apq == 0.0) continue;
                const double theta = (a[(q * N + q) * st] - a[(p * N + p) * st]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                LP_EPNP_LANES_SYNC();                           // (every lane has read a_pp, a_qq, a_pq)
                LP_EPNP_UNROLL(UNROLL)
                for (int k = ln; k < N; k += nl) {              // columns p, q
                    const double akp = a[(k * N + p) * st], akq = a[(k * N + q) * st];
                    a[(k * N + p) * st] = c * akp - s * akq; a[(k * N + q) * st] = s * akp + c * akq;
                }
                LP_EPNP_LANES_SYNC();
                LP_EPNP_UNROLL(UNROLL)
                for (int k = ln; k < N; k += nl) {              // rows p, q
                    const double apk = a[(p * N + k) * st], aqk = a[(q * N + k) * st];
                    a[(p * N + k) * st] = c * apk - s * aqk; a[(q * N + k) * st] = s * apk + c * aqk;
                }
                LP_EPNP_UNROLL(UNROLL)
                for (int k = ln; k < N; k += nl) {
                    const double vkp = v[(k * N + p) * st], vkq = v[(k * N + q) * st];
                    v[(k * N + p) * st] = c * vkp - s * vkq; v[(k * N + q) * st] = s * vkp + c * vkq;
                }
                LP_EPNP_LANES_SYNC();
            }
    }
    for (int i = 0; i < N; ++i) order[i] = i;
    for (int i = 1; i < N; ++i) {
        const int val = order[i];
        const double dv = a[(val * N + val) * st];
        if (dv < a[(order[0] * N + order[0]) * st]) {
            for (int j = i; j > 0; --j) order[j] = order[j - 1];
            order[0] = val;
        } else {
            int j = i;
            while (dv < a[(order[j - 1] * N + order[j - 1]) * st]) { order[j] = order[j - 1]; --j; }      // (stops at j = 1 at the latest: the test above failed)
            order[j] = val;
        }
    }
}

// lsq_small of two_view.cpp: least squares A x = b (m x k, k <= 5) by the normal equations and Gaussian elimination with partial
// pivoting; false when singular
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

// horn_absolute_orientation of two_view.cpp for four points and a fixed scale: x1 = R x2 + t
LP_EPNP_FN bool horn4(const double* x1, const double* x2, double* R, double* t)
{
    const int n = 4;
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
    int order[4];
    jacobi<4, 4>(N, evec, 1, order);                     // ascending: the last column belongs to the largest eigenvalue
    double q[4];
    q[0] = evec[0]; q[1] = evec[4]; q[2] = evec[8]; q[3] = evec[12];
    LP_EPNP_UNROLL(3)
    for (int c = 1; c < 4; ++c) if (order[3] == c) { q[0] = evec[c]; q[1] = evec[4 + c]; q[2] = evec[8 + c]; q[3] = evec[12 + c]; }
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(qn > 0)) return false;
    for (int k = 0; k < 4; ++k) q[k] /= qn;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double Rm[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                          2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                          2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    const double sc = 1.0;
    for (int k = 0; k < 9; ++k) R[k] = Rm[k];
    for (int r = 0; r < 3; ++r) t[r] = o1[r] - sc * (Rm[r * 3] * o2[0] + Rm[r * 3 + 1] * o2[1] + Rm[r * 3 + 2] * o2[2]);
    return true;
}

LP_EPNP_FN double dot3(const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// epnp_solve of two_view.cpp (lines 587-717) for n = 4.  pw: 4 x 3 landmarks (world), uv: 4 x 2 keypoints (pixels), cam: fx fy cx cy;
// ws: kWorkspace doubles, element e at ws[e * stride].  true: R (row major, world -> camera) and t are written.
// ln, nl: as for jacobi -- nl lanes of a wave call this together with the same arguments and one workspace; each returns the result.
LP_EPNP_FN bool epnp4(const double* pw, const double* uv, const double* cam, double* ws, int stride, double* R, double* t, int ln = 0, int nl = 1)
{
    const int n = 4;
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
    jacobi<3, 3>(C, evec, 1, ord3);                         // ascending; the principal direction first, as the published code orders them
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
    double al[16];
    for (int i = 0; i < n; ++i) {
        const double d0 = pw[3 * i] - cws[0][0], d1 = pw[3 * i + 1] - cws[0][1], d2 = pw[3 * i + 2] - cws[0][2];
        for (int j = 0; j < 3; ++j) al[4 * i + 1 + j] = CI[j * 3] * d0 + CI[j * 3 + 1] * d1 + CI[j * 3 + 2] * d2;
        al[4 * i] = 1.0 - al[4 * i + 1] - al[4 * i + 2] - al[4 * i + 3];
    }
    // 3. M^T M, accumulated row pair by row pair
    double* MtM = ws;
    double* mvec = ws + 144 * stride;
    for (int e = ln; e < 144; e += nl) MtM[e * stride] = 0;
    LP_EPNP_LANES_SYNC();
    for (int i = 0; i < n; ++i) {
        double r1[12], r2[12];
        for (int j = 0; j < 4; ++j) {
            const double a = al[4 * i + j];
            r1[3 * j] = a * fu; r1[3 * j + 1] = 0.0;    r1[3 * j + 2] = a * (uc - uv[2 * i]);
            r2[3 * j] = 0.0;    r2[3 * j + 1] = a * fv; r2[3 * j + 2] = a * (vc - uv[2 * i + 1]);
        }
        for (int a = ln; a < 12; a += nl) for (int b2 = 0; b2 < 12; ++b2) MtM[(a * 12 + b2) * stride] += r1[a] * r1[b2] + r2[a] * r2[b2];      // (a lane's rows are its own)
    }
    LP_EPNP_LANES_SYNC();
    int ord12[12];
    jacobi<12, 1>(MtM, mvec, stride, ord12, ln, nl);        // ascending: columns 0 .. 3 span the (approximate) null space
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
    double pc[12];
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
        if (pc[2] < 0) for (int k = 0; k < 12; ++k) pc[k] = -pc[k];      // the first landmark in front of the camera
        double Rg[9], tg[3];
        if (!horn4(pc, pw, Rg, tg)) continue;
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

// count_inliers of pnp_solve_ransac for one match: landmark X, keypoint (u, v) with weight inv_sigma2 = 1 / scale^2 of its level
LP_EPNP_FN bool pnp_inlier(const double* R, const double* t, const double* cam, const double* X, double u, double v, double inv_sigma2)
{
    const double xc = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], yc = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    const double du = cam[0] * xc / z + cam[2] - u, dv = cam[1] * yc / z + cam[3] - v;
    return z > 0 && (du * du + dv * dv) * inv_sigma2 < 5.991;
}

// ---- host only from here on (a plain inline function) ---------------------------------------------------------------------------
// The samples of pnp_solve_ransac for a set of n >= 4 matches: xorshift32 from seed ? seed : 1, four draws per iteration (whether
// or not the solve succeeds), each a step of a partial Fisher-Yates over avail[0 .. n) that is rebuilt every iteration.  table
// receives iterations x 4 match indices; avail is n ints of scratch.
inline void sample_table(int n, int iterations, uint32_t seed, int32_t* table, int* avail)
{
    uint32_t s = seed ? seed : 1u;
    for (int it = 0; it < iterations; ++it) {
        for (int i = 0; i < n; ++i) avail[i] = i;
        int left = n;
        for (int k = 0; k < 4; ++k) {
            s ^= s << 13; s ^= s >> 17; s ^= s << 5;
            const int r = (int)(s % (uint32_t)left);
            table[4 * it + k] = avail[r]; avail[r] = avail[left - 1]; --left;
        }
    }
}

}  // namespace lpslam_epnp
