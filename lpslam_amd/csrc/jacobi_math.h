// jacobi_math.h -- the cyclic Jacobi eigen-solver of a small symmetric matrix, once, for the device kernels
// (pnp.hip through epnp_math.h, triangulate.hip through triangulate_math.h) and the host library (LpSlam::sym_eigen_jacobi of
// lpslam_amd/host/two_view.cpp): FP64, + - * / sqrt only, so that -- every side built with -ffp-contract=off -- all of them return the
// same bits.  No heap; the matrices are the caller's.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LP_JACOBI_FN __host__ __device__ __forceinline__      // (inlined: a caller's constant n, stride and lanes stay constants)
#define LP_JACOBI_PRAGMA(x) _Pragma(#x)
#define LP_JACOBI_UNROLL(n) LP_JACOBI_PRAGMA(unroll n)     // constant indices: the small matrices stay in registers on the device
#else
#define LP_JACOBI_FN inline
#define LP_JACOBI_UNROLL(n)
#endif
// Lanes of one wave that work on one matrix together (below): what a lane wrote to it is read by its neighbours from here on.  A
// wave's LDS instructions execute in their order; this keeps the compiler from moving or caching accesses across the point.
#if defined(__HIP_DEVICE_COMPILE__)
#define LP_JACOBI_LANES_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#else
#define LP_JACOBI_LANES_SYNC() do { } while (0)
#endif

namespace lpslam_jacobi {

// The rotations of the cyclic Jacobi method on a symmetric n x n matrix, in place: a (row major, element (i, j) at a[(i * n + j) * st])
// ends with the eigenvalues on its diagonal, v receives the eigenvectors as columns; at most 64 sweeps.
// N: the size when it is a constant of the caller (every index of the small matrices is then a constant: registers on the device);
// 0: the size is the argument n_run (the host's sym_eigen_jacobi).
// UNROLL: the loop bodies are expanded so that every index is a constant (N = 3, 4); the 12 x 12 matrix and the host keep their loops.
// ln, nl: lane ln of nl lanes of one wave that call this together on one (shared) a and v with the same values: the elements of a
// rotation -- independent of each other -- are divided among them (k = ln, ln + nl, ...), everything else every lane computes for
// itself.  Each element is computed by the same operations either way; the host and the small matrices run with one lane.
// SYNC: the points at which the lanes wait for each other's writes.  false leaves them out for a caller whose lanes each hold their
// own matrix in registers (triangulate.hip); the PnP kernel keeps them at all three of its matrices, as it was measured.
template <int N, int UNROLL, bool SYNC = true>
LP_JACOBI_FN void jacobi_sweeps(double* a, double* v, int st, int ln = 0, int nl = 1, int n_run = N)
{
    const int n = N > 0 ? N : n_run;
    for (int i = ln; i < n * n; i += nl) v[i * st] = 0.0;
    if (SYNC) LP_JACOBI_LANES_SYNC();
    for (int i = ln; i < n; i += nl) v[(i * n + i) * st] = 1.0;
    if (SYNC) LP_JACOBI_LANES_SYNC();
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0, diag = 0;
        LP_JACOBI_UNROLL(UNROLL)
        for (int i = 0; i < n; ++i)
            LP_JACOBI_UNROLL(UNROLL)
            for (int j = 0; j < n; ++j) { const double x = a[(i * n + j) * st]; if (i == j) diag += x * x; else off += x * x; }
        if (off <= 1e-30 * (diag + 1e-300)) break;
        LP_JACOBI_UNROLL(UNROLL)
        for (int p = 0; p < n - 1; ++p)
            LP_JACOBI_UNROLL(UNROLL)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(p * n + q) * st];
                if (apq == 0.0) continue;
                const double theta = (a[(q * n + q) * st] - a[(p * n + p) * st]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                if (SYNC) LP_JACOBI_LANES_SYNC();                         // (every lane has read a_pp, a_qq, a_pq)
                LP_JACOBI_UNROLL(UNROLL)
                for (int k = ln; k < n; k += nl) {              // columns p, q
                    const double akp = a[(k * n + p) * st], akq = a[(k * n + q) * st];
                    a[(k * n + p) * st] = c * akp - s * akq; a[(k * n + q) * st] = s * akp + c * akq;
                }
                if (SYNC) LP_JACOBI_LANES_SYNC();
                LP_JACOBI_UNROLL(UNROLL)
                for (int k = ln; k < n; k += nl) {              // rows p, q
                    const double apk = a[(p * n + k) * st], aqk = a[(q * n + k) * st];
                    a[(p * n + k) * st] = c * apk - s * aqk; a[(q * n + k) * st] = s * apk + c * aqk;
                }
                LP_JACOBI_UNROLL(UNROLL)
                for (int k = ln; k < n; k += nl) {
                    const double vkp = v[(k * n + p) * st], vkq = v[(k * n + q) * st];
                    v[(k * n + p) * st] = c * vkp - s * vkq; v[(k * n + q) * st] = s * vkp + c * vkq;
                }
                if (SYNC) LP_JACOBI_LANES_SYNC();
            }
    }
}

// order[c] = the column of the c-th smallest eigenvalue after jacobi_sweeps: an insertion sort in which the first among equal
// eigenvalues stays first, written out comparison by comparison as libstdc++'s std::sort performs it on 16 elements or fewer (the
// order LpSlam::sym_eigen_jacobi has always returned).
template <int N>
LP_JACOBI_FN void jacobi_order(const double* a, int st, int* order, int n_run = N)
{
    const int n = N > 0 ? N : n_run;
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 1; i < n; ++i) {
        const int val = order[i];
        const double dv = a[(val * n + val) * st];
        if (dv < a[(order[0] * n + order[0]) * st]) {
            for (int j = i; j > 0; --j) order[j] = order[j - 1];
            order[0] = val;
        } else {
            int j = i;
            while (dv < a[(order[j - 1] * n + order[j - 1]) * st]) { order[j] = order[j - 1]; --j; }      // (stops at j = 1 at the latest: the test above failed)
            order[j] = val;
        }
    }
}

// Both.  (Size, stride and unrolling are template or literal arguments at every device call: the kernels were found to compile to the
// same code as with their own copies only when each of these functions sees its constants before it is inlined.)
template <int N, int UNROLL>
LP_JACOBI_FN void jacobi(double* a, double* v, int st, int* order, int ln = 0, int nl = 1)
{
    jacobi_sweeps<N, UNROLL>(a, v, st, ln, nl);
    jacobi_order<N>(a, st, order);
}

}  // namespace lpslam_jacobi
