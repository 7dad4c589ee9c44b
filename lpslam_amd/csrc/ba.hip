// ba.hip -- SE3 bundle adjustment on gfx950 (FP64): g2o-style Levenberg-Marquardt with landmark Schur complement.
//
// [UPSTREAM] g2o@691dc51 OptimizationAlgorithmLevenberg + BlockSolver<6,3> (buildSystem / Schur / solve) and the
// OpenVSLAM reprojection edges, which the reference runs on its mapping / global-optimisation threads
// (/root/reference/src/Trackers/OpenVSLAMTrackerBase.cpp:239,250-255; pin conan-packages/g2o-conan/conanfile.py:6).
//
// The whole LM loop is device driven: lambda, nu, the accepted-state index and the accept / reject decision live in a
// small control block in HBM, every kernel reads it, and the host only enqueues "trial units" and looks at the control
// block once per optimize() call.  A unit = [linearise if the state changed] + one LM trial:
//   linearise   k_ba_lin (observation side: thread / observation, W = B^T w A and shares of H_ll, b_l; pose side: 8
//               wavefronts / keyframe, H_pp, b_p, chi2; both in one launch), k_ba_point_sum (H_ll, b_l; its last workgroup
//               combines the pose partials in fixed order and computes lambda_0)
//   trial       k_ba_schur (wavefront / pose-block pair over a pair list; Y = W (H_ll + lambda)^-1 formed per term),
//               k_chol_pair x nb/2 (32-wide panels, two per launch, block products on the f64 matrix cores; the rhs is carried as an extra
//               row and L^-T as extra row blocks, so no triangular substitution is needed), k_chol_xsolve (x_p = L^-T y),
//               k_ba_backsub (landmarks, trial poses), k_ba_trial (trial chi2; its last workgroup runs g2o's lambda control)
// All sums are fixed-order segmented reductions (no float atomics): results are reproducible run to run.
// The reduced system [S | rhs | b_p | diag H_pp | chi2] is one contiguous buffer, so a landmark-partitioned multi-GPU
// solve needs one sum all-reduce of it per trial (lpslam_hip_ba_step_*).
#include "internal.h"
#include "ba_common.h"
#include <chrono>
#include <cmath>
#include <cstring>
#include <cstddef>
#include <cfloat>
#include <algorithm>
#include <atomic>
#include <map>
#include <string>
#include <dlfcn.h>

#pragma clang fp contract(off)

using namespace lpslam;

namespace {

constexpr int SCH_PV = 42;            // values a part of a pose-block pair's list hands over in k_ba_schur: the 6 x 6 sum + the 6 of the keyframe's rhs (diagonal blocks)
// How many workgroups of k_ba_schur share a pose-block pair's list: lists longer than `part` terms are cut into interleaved parts
// (32-term chunks round-robin), so that the longest list -- a keyframe's diagonal block, one term per observation -- does not set the
// kernel's duration; the part that finishes last adds the parts up in order (fixed summation order).
// `part` is chosen per window when its lists are built (k_bs_blkscan): the smallest of 128, 160, 192, 224 (at most
// SCH_MAXP parts) whose further parts still fit beside the launch's other workgroups in ONE generation of resident wavefronts, else
// SCH_PART with at most SCH_MAXP_WIDE parts -- the cut every window had before.
// (The earlier note here, "8 parts of ~100 terms measured: 23.0 us against 22.2", blamed the surplus workgroups of the larger table.
// The arithmetic says otherwise: 128-term parts make ~2300 workgroups of the benchmark's window, the chip holds 2048 wavefronts of this
// kernel, and the launch ran a second generation.)
constexpr int SCH_MAXP = 8, SCH_PART = 256, SCH_MAXP_WIDE = 4, SCH_PART_MIN = 128, SCH_PART_STEP = 32;
__host__ __device__ inline int schur_parts(int n_terms, int part)
{
    if (n_terms <= part) return 1;
    const int p = (n_terms + part - 1) / part, cap = part >= SCH_PART ? SCH_MAXP_WIDE : SCH_MAXP;
    return p < cap ? p : cap;
}
// head word of the table of further parts (behind the tickets): items in the low 24 bits (at most 1 << 18), part / 32 above them
__host__ __device__ inline int schur_head(int count, int part) { return count | ((part / SCH_PART_STEP) << 24); }
__host__ __device__ inline int schur_head_count(int head) { return head & 0xFFFFFF; }
__host__ __device__ inline int schur_head_part(int head) { const int p = (head >> 24) * SCH_PART_STEP; return p >= SCH_PART_MIN && p < SCH_PART ? p : SCH_PART; }
constexpr int SPLIT = 8;              // wavefronts per keyframe in the pose pass
constexpr int PV = 28;                // partial-row stride per wavefront: 21 (H_pp upper) + 6 (b_p) (+1 pad; chi2 is kept apart)

// Which problems take the one-launch update behind the fused solve (k_ba_update, ba_update.inl), decided per PROBLEM so that a problem
// is solved by the same kernels -- to the same bytes -- alone or inside a mixed batch; the two-launch form (k_ba_backsub, k_ba_trial)
// skips those problems when it runs beside it.
constexpr int UPD_MAXP = 320;               // keyframes whose trial poses fit the landmark blocks' LDS (config 5: 200)
__host__ __device__ inline bool upd_takes(int n_points, int n_free, int n_poses) { return n_points >= 1 && n_free >= 1 && n_poses <= UPD_MAXP; }

// A batch of problems (grid.y = problems) with every problem's workgroups on ONE XCD: workgroups go to the eight XCDs round robin
// in dispatch order (x fastest), so workgroup L of the launch is given to problem L % 8 (+ 8 per full round of a problem's
// workgroups).  What a problem's workgroups read again and again -- the W rows in the Schur kernel, 8 times each -- then comes out
// of one L2 instead of being fetched into all eight (a 16-window batch: 444 MB of FETCH_SIZE per Schur launch against the 93 MB
// the batch holds; 4.24 -> 4.05 ms per batch of 16 x 10 iterations).  Speed only: the mapping is a bijection whatever the
// placement is.  Needs grid.y to be a multiple of 8.
struct BaWg { int x, y; };
__device__ __forceinline__ BaWg ba_wg_xcd()
{
    int x = blockIdx.x, y = blockIdx.y;
    const int ny = gridDim.y, nx = gridDim.x;
    if (ny >= 8 && (ny & 7) == 0) {
        const unsigned L = (unsigned)y * (unsigned)nx + (unsigned)x, slot = L >> 3;
        y = (int)(L & 7u) + 8 * (int)(slot / (unsigned)nx);
        x = (int)(slot % (unsigned)nx);
    }
    return BaWg{x, y};
}
#define BA_VIEW_XCD(v, bx) const BaWg wg_ = ba_wg_xcd(); BaView v = views[wg_.y]; const int bx = wg_.x
// The members a kernel needs before its first branch, made live together: one scalar round trip for the extents AND the control
// block pointer (left alone the compiler loads the pointer only behind the extent test, one round trip later).
#define BA_VIEW_HEAD(...) asm volatile("" :: __VA_ARGS__)

// What the kernels read of the control block, fetched in ONE round trip (straight-line loads, no branch between them): written as
// `if (ba_idle(ctl) || !ctl->need_lin) return; idx = ctl->cur;` every member was a dependent round trip of its own in front of the
// kernel's real work.
struct BaFlags {
    double lambda; int cur, need_lin, outer_done, max_outer, stopped, cur_launch, spec;
    __device__ __forceinline__ bool idle() const { return (stopped != 0) | (outer_done >= max_outer); }
};
__device__ __forceinline__ BaFlags ba_flags(const BaCtl* c)
{
    BaFlags f;
    f.lambda = c->lambda; f.cur = c->cur; f.need_lin = c->need_lin; f.outer_done = c->outer_done; f.max_outer = c->max_outer;
    f.stopped = c->stopped; f.cur_launch = c->cur_launch; f.spec = c->spec;
    return f;
}
// Member [idx] of a two-element pointer array of the view, by ARITHMETIC on its two constant-index members: a select between two
// members (or a dynamic index) can end up as an indexed load from a copy of the whole view in scratch memory -- it did when the
// view grew (552 bytes of scratch per lane, every member access a scratch load, trial launch 14 -> 41 us).
template <class P> __device__ __forceinline__ P sel2(P a0, P a1, int idx) { return a0 + (ptrdiff_t)idx * (a1 - a0); }
// selects the evaluated state: the accepted one (trial = 0) or the trial one
__device__ __forceinline__ void ba_select(BaView& v, int trial)
{
    const int s = v.ctl->cur ^ trial;
    v.poses = sel2(v.poses_buf[0], v.poses_buf[1], s); v.points = sel2(v.points_buf[0], v.points_buf[1], s);
}
// state buffer and linearisation set by explicit index (kernels that must not follow a `cur` flipping under them)
__device__ __forceinline__ void ba_select_idx(BaView& v, int idx)
{
    v.poses = sel2(v.poses_buf[0], v.poses_buf[1], idx); v.points = sel2(v.points_buf[0], v.points_buf[1], idx);
}
// offsets (in doubles, multiples of 32 = 256 bytes) of the sub-arrays of a linearisation set's two blocks and of the CSR copies
struct SetOff { size_t loc, z_total, bl, Hpp, W, hl, d_total; };
__host__ __device__ inline size_t al32(size_t x) { return (x + 31) & ~(size_t)31; }
__host__ __device__ inline SetOff set_offsets(int n_poses, int n_points, int n_obs, int n_free, int dim_pad)
{
    const size_t np = (size_t)n_poses, npt = (size_t)(n_points > 1 ? n_points : 1), no = (size_t)(n_obs > 1 ? n_obs : 1), nf = (size_t)(n_free > 1 ? n_free : 1);
    SetOff o;
    o.loc = al32(np * SPLIT * (PV + 1)); o.z_total = o.loc + al32(2 * (size_t)dim_pad + 8);
    o.bl = al32(6 * npt); o.Hpp = o.bl + al32(3 * npt); o.W = o.Hpp + al32(36 * nf); o.hl = o.W + al32(18 * no); o.d_total = o.hl + al32(9 * no);
    return o;
}
__host__ __device__ inline size_t csr_stride(int n_obs) { return al32((size_t)(n_obs > 1 ? n_obs : 1)); }
__device__ __forceinline__ void ba_lin_set(BaView& v, int idx)
{
    GPTR(double) z = sel2(v.set_z[0], v.set_z[1], idx);
    GPTR(double) d = sel2(v.set_d[0], v.set_d[1], idx);
    const SetOff o = set_offsets(v.n_poses, v.n_points, v.n_obs, v.n_free, v.dim_pad);
    v.partial = z;
    GPTR(double) loc = z + o.loc;
    v.bp_loc = loc; v.hppdiag_loc = loc + v.dim_pad; v.chi_loc = loc + 2 * v.dim_pad;
    v.Hll = d; v.bl = d + o.bl; v.Hpp = d + o.Hpp; v.W = d + o.W; v.hl_obs = d + o.hl;
}

__device__ __forceinline__ void quat_to_rot(const double* q, double* R)
{
    const double rn = fast_rsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * rn, x = q[1] * rn, y = q[2] * rn, z = q[3] * rn;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}

// residual e = obs - projection, camera-frame point pc; returns 2 (mono) or 3 (stereo).  The camera travels BY VALUE through these
// helpers: handed on as a reference into the by-value view, the compiler kept the whole view in scratch memory (552 bytes per lane).
__device__ __forceinline__ int ba_residual_vals(const BaCam cam, double ou, double ov, double ur, const double* R, const double* t, const double* X,
                                                double* e, double* pc)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) pc[i] = R[i * 3] * X[0] + R[i * 3 + 1] * X[1] + R[i * 3 + 2] * X[2] + t[i];
    const double iz = fast_rcp(pc[2]);
    const double u = cam.fx * pc[0] * iz + cam.cx;
    const double vv = cam.fy * pc[1] * iz + cam.cy;
    e[0] = ou - u; e[1] = ov - vv;
    if (ur < 0) { e[2] = 0; return 2; }
    e[2] = ur - (u - cam.fxb * iz);
    return 3;
}
__device__ __forceinline__ int ba_residual(const BaView& v, int k, const double* R, const double* t, const double* X,
                                           double* e, double* pc)
{
    return ba_residual_vals(v.cam, v.o_u[k], v.o_v[k], v.o_ur[k], R, t, X, e, pc);
}

// Jacobians of the reprojection error: A (D x 3, landmark), B (D x 6, pose, rotation first)
__device__ __forceinline__ void ba_jacobians(const BaCam c, const double* R, const double* pc, int D, double A[3][3], double B[3][6])
{
    const double x = pc[0], y = pc[1], iz = fast_rcp(pc[2]), iz2 = iz * iz;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[0][k] = -c.fx * R[k] * iz + c.fx * x * R[6 + k] * iz2;
        A[1][k] = -c.fy * R[3 + k] * iz + c.fy * y * R[6 + k] * iz2;
        A[2][k] = A[0][k] - c.fxb * R[6 + k] * iz2;
    }
    B[0][0] = x * y * iz2 * c.fx;          B[0][1] = -(1.0 + (x * x * iz2)) * c.fx; B[0][2] = y * iz * c.fx;
    B[0][3] = -iz * c.fx;                  B[0][4] = 0.0;                            B[0][5] = x * iz2 * c.fx;
    B[1][0] = (1.0 + y * y * iz2) * c.fy;  B[1][1] = -x * y * iz2 * c.fy;            B[1][2] = -x * iz * c.fy;
    B[1][3] = 0.0;                         B[1][4] = -iz * c.fy;                     B[1][5] = y * iz2 * c.fy;
    B[2][0] = B[0][0] - c.fxb * y * iz2;   B[2][1] = B[0][1] + c.fxb * x * iz2;      B[2][2] = B[0][2];
    B[2][3] = B[0][3];                     B[2][4] = 0.0;                            B[2][5] = B[0][5] - c.fxb * iz2;
    if (D == 2) {      // monocular edge: the third row does not exist; zero rows keep every sum exact and loops unrolled
#pragma unroll
        for (int k = 0; k < 3; ++k) A[2][k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) B[2][k] = 0.0;
    }
}

// weight (rho1 * inv_sigma2) and robustified chi2 of one observation
__device__ __forceinline__ double ba_weight_vals(const BaCam cam, double om, int D, const double* e, int robust, double* rho0)
{
    const double chi = om * (e[0] * e[0] + e[1] * e[1] + (D == 3 ? e[2] * e[2] : 0.0));
    const double delta = D == 3 ? cam.hub_stereo : cam.hub_mono;
    double w = om;
    *rho0 = chi;
    if (robust && delta > 0) { double r1; huber(chi, delta, rho0, &r1); w *= r1; }
    return w;
}
__device__ __forceinline__ double ba_weight(const BaView& v, int k, int D, const double* e, int robust, double* rho0)
{
    return ba_weight_vals(v.cam, v.o_w[k], D, e, robust, rho0);
}

// The last-workgroup hand-over (ba_last_block, ba_common.h) without cache maintenance: every byte the last workgroup reads from the others
// is stored write-through (st_sc1) and read L1-bypassing (ld_sc1); each storing wavefront drains its stores, the workgroup
// meets at a barrier and one lane takes a relaxed agent-scope ticket (MI355X_MICROARCH, valid forms: one unsharded counter, the
// consumer is the workgroup whose add came last).  An acquire-release pair here would cost a buffer_wbl2 + buffer_inv, ~3.5 us.
__device__ __forceinline__ void st_sc1(double* p, double x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_sc1(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void st_sc1(GPTR(double) p, double x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }      // global_, not flat_
__device__ __forceinline__ double ld_sc1(GPTR(const double) p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_sc1(GPTR(double) p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif
__device__ __forceinline__ bool ba_last_block_sc1(int* ticket, int total)
{
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wavefront drains its own stores (a barrier alone does not)
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == total - 1);
        if (s_last) *ticket = 0;
    }
    __syncthreads();
    return s_last != 0;
}
__device__ __forceinline__ bool ba_last_block_sc1(BaCtl* c, int total) { return ba_last_block_sc1(&c->ticket, total); }

// (H_ll + lambda I)^-1 of one landmark, symmetric 3x3 stored as 6 (zero when singular)
__device__ __forceinline__ void point_hinv(const double* hl, double lambda, double* ho)
{
    const double a = hl[0] + lambda, b = hl[1], c = hl[2], d = hl[3] + lambda, e = hl[4], f = hl[5] + lambda;
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double det = a * c00 + b * c01 + c * c02;
    if (fabs(det) > 0) {
        const double id = fast_rcp(det);
        ho[0] = c00 * id; ho[1] = c01 * id; ho[2] = c02 * id;
        ho[3] = (a * f - c * c) * id; ho[4] = (b * c - a * e) * id; ho[5] = (a * d - b * b) * id;
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) ho[i] = 0;
    }
}

// ---- linearisation, observation side: one thread per observation: W = B^T w A and the observation's share of H_ll, b_l --
__device__ __forceinline__ void obs_lin_body(BaView& v, int bid, int robust, int points_fixed, int set)
{
    ba_select_idx(v, set); ba_lin_set(v, set);
    const int k = bid * 256 + threadIdx.x;
    if (k >= v.n_obs) return;
    double* Wk = v.W + 18 * (size_t)k;
    double* ho = v.hl_obs + 9 * (size_t)k;
    const int p = v.o_pose[k];
    const int slot = v.pose_slot[p];
    if (!v.o_active[k] || points_fixed) {       // inactive edge, or motion-only mode (landmarks are constants: x_l = 0)
#pragma unroll
        for (int i = 0; i < 18; ++i) Wk[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) ho[i] = 0.0;
        return;
    }
    const int j = v.o_point[k];
    const double X[3] = {v.points[3 * j], v.points[3 * j + 1], v.points[3 * j + 2]};
    double R[9], e[3], pc[3], A[3][3], B[3][6], rho0;
    quat_to_rot(v.poses + 7 * p, R);
    const int D = ba_residual(v, k, R, v.poses + 7 * p + 4, X, e, pc);
    ba_jacobians(v.cam, R, pc, D, A, B);
    const double w = ba_weight(v, k, D, e, robust, &rho0);
    int idx = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = a; c < 3; ++c) {
            double s2 = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r) s2 += A[r][a] * w * A[r][c];
            ho[idx++] = s2;
        }
        double s3 = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) s3 += A[r][a] * (-w * e[r]);
        ho[6 + a] = s3;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double s2 = 0;
            if (slot >= 0) {
#pragma unroll
                for (int r = 0; r < 3; ++r) s2 += B[r][a] * w * A[r][c];
            }
            Wk[a * 3 + c] = s2;
        }
}

// ---- linearisation, observation side, LANDMARK-MAJOR: what obs_lin_body + the landmark sums of k_ba_point_sum compute, in one pass.
//      A workgroup owns LAND_B consecutive landmarks and walks their observations in CSR order (= the order k_ba_point_sum adds
//      them in), 256 at a time: thread = observation -> W (to the observation's storage slot) and its 9 shares of (H_ll, b_l) into
//      LDS; then thread (landmark l, component c) adds the shares of its landmark's segment of the chunk in ascending order -- the
//      same sums, bit for bit, without the 72 bytes per observation going to memory and coming back in a launch of their own.
//      The observation constants are read from their CSR-ordered copies (c_*), coalesced.
constexpr int LAND_B = 32;
__device__ __forceinline__ void land_lin_body(BaView& v, int bid, int robust, int points_fixed, int set)
{
    ba_select_idx(v, set); ba_lin_set(v, set);
    __shared__ double sh[256 * 9];
    __shared__ int s_start[LAND_B + 1];
    const int tid = threadIdx.x;
    const int j0 = v.land_start[2 * bid], j1 = v.land_start[2 * bid + 2];
    if (tid <= LAND_B) s_start[tid] = v.pt_start[min(j0 + tid, j1)];
    __syncthreads();
    const int s_lo = s_start[0], s_hi = s_start[j1 - j0];
    const size_t cs = csr_stride(v.n_obs);
    GPTR(const double) c_u = v.csr; GPTR(const double) c_v = v.csr + cs; GPTR(const double) c_ur = v.csr + 2 * cs; GPTR(const double) c_w = v.csr + 3 * cs;
    GPTR(const int) c_pose = (GPTR(const int))(v.csr + 4 * cs); GPTR(const int) c_point = c_pose + cs;
    const int l = tid >> 3, c = tid & 7;                   // the sums: landmark j0 + l, components c (and 8 with c == 0)
    const int seg_lo = s_start[min(l, j1 - j0)], seg_hi = s_start[min(l + 1, j1 - j0)];
    double acc = 0, acc8 = 0;
    for (int chunk = s_lo; chunk < s_hi; chunk += 256) {
        const int s = chunk + tid;
        double hs[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (s < s_hi) {
            const int k = v.pt_obs[s];
            const int p = c_pose[s];
            const int slot = v.pose_slot[p];
            double* Wk = v.W + 18 * (size_t)k;
            if (!v.o_active[k] || points_fixed) {
#pragma unroll
                for (int i = 0; i < 18; ++i) Wk[i] = 0.0;
            } else {
                const int j = c_point[s];
                const double X[3] = {v.points[3 * j], v.points[3 * j + 1], v.points[3 * j + 2]};
                double R[9], e[3], pc[3], A[3][3], B[3][6], rho0;
                quat_to_rot(v.poses + 7 * p, R);
                const int D = ba_residual_vals(v.cam, c_u[s], c_v[s], c_ur[s], R, v.poses + 7 * p + 4, X, e, pc);
                ba_jacobians(v.cam, R, pc, D, A, B);
                const double w = ba_weight_vals(v.cam, c_w[s], D, e, robust, &rho0);
                int idx = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
#pragma unroll
                    for (int cc = a; cc < 3; ++cc) {
                        double s2 = 0;
#pragma unroll
                        for (int r = 0; r < 3; ++r) s2 += A[r][a] * w * A[r][cc];
                        hs[idx++] = s2;
                    }
                    double s3 = 0;
#pragma unroll
                    for (int r = 0; r < 3; ++r) s3 += A[r][a] * (-w * e[r]);
                    hs[6 + a] = s3;
                }
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) {
                        double s2 = 0;
                        if (slot >= 0) {
#pragma unroll
                            for (int r = 0; r < 3; ++r) s2 += B[r][a] * w * A[r][cc];
                        }
                        Wk[a * 3 + cc] = s2;
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) sh[tid * 9 + i] = hs[i];
        __syncthreads();
        const int a0 = max(seg_lo, chunk), a1 = min(seg_hi, chunk + 256);
        for (int t = a0; t < a1; ++t) {
            acc += sh[(t - chunk) * 9 + c];
            if (c == 0) acc8 += sh[(t - chunk) * 9 + 8];
        }
        __syncthreads();
    }
    const int j = j0 + l;
    if (j < j1) {
        if (c < 6) v.Hll[6 * (size_t)j + c] = acc; else v.bl[3 * (size_t)j + (c - 6)] = acc;
        if (c == 0) v.bl[3 * (size_t)j + 2] = acc8;
    }
}

// ---- linearisation 2/2: H_ll, b_l per landmark = fixed-order sum over its observations; block maxima of diag H_ll.  The
//      One extra workgroup combines the pose partials of the linearisation (pose_combine_body, defined below); the workgroup
//      that finishes last starts the outer iteration.
__device__ __forceinline__ void pose_combine_body(BaView& v, int mode, int part_n, int fused);
__global__ __launch_bounds__(256) void k_ba_point_sum(const BaView* __restrict__ views, int fused)
{
    BA_VIEW(v);
    BA_VIEW_HEAD("s"(v.point_blocks), "s"(v.ctl));
    const int part_n = v.point_blocks;                     // landmark workgroups of this problem; workgroup part_n combines the pose partials
    if ((int)blockIdx.x > part_n) return;
    const BaFlags fl = ba_flags(v.ctl);
    if (fl.idle() || !fl.need_lin) return;
    ba_lin_set(v, fl.cur);
    __shared__ double sm[4];
    if ((int)blockIdx.x == part_n) {
        // the extra workgroup: the pose partials of the linearisation are complete before this launch, so they are combined
        // here, beside the landmark sums, instead of on the critical path of the workgroup that finishes last
        pose_combine_body(v, 0, part_n, 0);
    } else {
        const int j = blockIdx.x * 256 + threadIdx.x;
        double m = 0;
        if (j < v.n_points) {
            double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            // four observations at a time: their index loads together, then their 36 doubles together, then the sums in the fixed
            // order (one observation per pass meant two dependent round trips each: the kernel was their latency)
            const int s_end = v.pt_start[j + 1];
            for (int s = v.pt_start[j]; s < s_end; s += 4) {
                int kk[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) kk[u] = v.pt_obs[min(s + u, s_end - 1)];
                double hv[4][9];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double* ho = v.hl_obs + 9 * (size_t)kk[u];
#pragma unroll
                    for (int i = 0; i < 9; ++i) hv[u][i] = ho[i];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (s + u < s_end) {
#pragma unroll
                        for (int i = 0; i < 9; ++i) acc[i] += hv[u][i];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) v.Hll[6 * (size_t)j + i] = acc[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) v.bl[3 * (size_t)j + i] = acc[6 + i];
            m = fmax(fabs(acc[0]), fmax(fabs(acc[3]), fabs(acc[5])));
        }
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0 && (int)blockIdx.x < part_n) st_sc1(&v.part[blockIdx.x], fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3])));
    }
    if (!ba_last_block_sc1(v.ctl, part_n + 1)) return;
    // last workgroup: max diag H_ll over the block maxima, then the start of the outer iteration (lambda_0)
    if (threadIdx.x < 64) {
        double acc = 0;
        for (int i = threadIdx.x; i < part_n; i += 64) acc = fmax(acc, ld_sc1(&v.part[i]));
        acc = wave_max(acc);
        if (threadIdx.x == 0) {
            v.scal[4] = acc;
            const double chi = ld_sc1(&v.scal[6]), max_pp = ld_sc1(&v.scal[7]);
            *v.chi_cur = chi; *v.chi_loc = chi;
            if (fused) lm_begin(v, max_pp, acc, chi);
        }
    }
}

// ---- linearisation, pose side (mode 0) and trial chi2 (mode 1): SPLIT wavefronts per keyframe over slices of its
//      observations
__device__ __forceinline__ void pose_part_body(BaView& v, int bid, int robust, int mode, int set)
{
    ba_select_idx(v, set); ba_lin_set(v, set);
    double* chi_out = mode == 0 ? v.partial + (size_t)v.n_poses * SPLIT * PV : v.partial_trial;
    const int lane = threadIdx.x & 63;
    const int wv = bid * 4 + (threadIdx.x >> 6);
    const int p = wv / SPLIT, sp = wv - p * SPLIT;
    if (p >= v.n_poses) return;
    double R[9];
    quat_to_rot(v.poses + 7 * p, R);
    const double* t = v.poses + 7 * p + 4;
    const int slot = v.pose_slot[p];
    double h[21], b[6], chi = 0;
#pragma unroll
    for (int i = 0; i < 21; ++i) h[i] = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = 0;
    const bool full = mode == 0 && slot >= 0;
    for (int s = v.ps_start[p] + sp * 64 + lane; s < v.ps_start[p + 1]; s += 64 * SPLIT) {
        const int k = s;                        // observations are stored keyframe by keyframe
        if (!v.o_active[k]) continue;
        const int j = v.o_point[k];
        const double X[3] = {v.points[3 * j], v.points[3 * j + 1], v.points[3 * j + 2]};
        double e[3], pc[3], rho0;
        const int D = ba_residual(v, k, R, t, X, e, pc);
        const double w = ba_weight(v, k, D, e, robust, &rho0);
        chi += rho0;
        if (!full) continue;
        double A[3][3], B[3][6];
        ba_jacobians(v.cam, R, pc, D, A, B);
        int idx = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int c = a; c < 6; ++c) {
                double s2 = 0;
#pragma unroll
                for (int r = 0; r < 3; ++r) s2 += B[r][a] * w * B[r][c];
                h[idx++] += s2;
            }
            double s3 = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r) s3 += B[r][a] * (-w * e[r]);
            b[a] += s3;
        }
    }
    // partials: chi2 per (keyframe, slice) in the tail of v.partial, H_pp / b_p per (free-pose slot, slice) in its head,
    // so the combine addresses both without an index lookup
    chi = wave_sum(chi);
    if (lane == 0) st_sc1(&chi_out[(size_t)p * SPLIT + sp], chi);       // mode 1: read by the last workgroup of this launch
    if (!full) return;
    double* out = v.partial + ((size_t)slot * SPLIT + sp) * PV;
#pragma unroll
    for (int i = 0; i < 21; ++i) h[i] = wave_sum(h[i]);
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = wave_sum(b[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 21; ++i) out[i] = h[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) out[21 + i] = b[i];
    }
}

// ---- after the linearisation (mode 0) and the trial chi2 (mode 1): one workgroup (the last one of the pass that produced
//      the partials, see ba_last_block) combines the SPLIT partials in order, totals
//      chi2, reduces the landmark-side block partials in v.part (max diag H_ll / scale terms) and, in the single-GPU
//      ("fused") solve, runs the lambda control.  The partitioned solve runs k_lm_begin / k_lm_decide after its all-reduce.
__device__ __forceinline__ void pose_combine_body(BaView& v, int mode, int part_n, int fused)
{
    __shared__ double s_val[3];            // chi2, landmark-side term (max diag H_ll / scale term), max diag H_pp
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (wave == 0) {                       // chi2 = sum over keyframes (64-strided, then butterfly) of the in-order sum of its SPLIT partials
        double acc = 0;
        for (int p = lane; p < v.n_poses; p += 64) {
            double s = 0;
            const double* chi_in = mode == 0 ? v.partial + (size_t)v.n_poses * SPLIT * PV : v.partial_trial;
            for (int sp = 0; sp < SPLIT; ++sp) s += mode == 1 ? ld_sc1(&chi_in[(size_t)p * SPLIT + sp]) : chi_in[(size_t)p * SPLIT + sp];
            v.chi_pose[p] = s;
            acc += s;
        }
        acc = wave_sum(acc);
        if (lane == 0) s_val[0] = acc;
    } else if (wave == 1 && mode == 1) {
        double acc = 0;
        for (int i = lane; i < part_n; i += 64) acc += v.part[i];
        acc = wave_sum(acc);
        if (lane == 0) s_val[1] = acc;
    } else if (wave == 2 && mode == 0) {   // max |diag H_pp| straight from the partials (same sums as the loop below)
        double m = 0;
        for (int i = lane; i < v.dim; i += 64) {
            const int slot = i / 6, a = i - 6 * slot;
            const int q = 6 * a - a * (a - 1) / 2;          // (a, a) in the row-major upper triangle
            double s = 0;
            for (int sp = 0; sp < SPLIT; ++sp) s += v.partial[((size_t)slot * SPLIT + sp) * PV + q];
            m = fmax(m, fabs(s));
        }
        m = wave_max(m);
        if (lane == 0) s_val[2] = m;
    }
    if (mode == 0) {
        // H_pp (21) and b_p (6) per free pose: in-order sums of the SPLIT partials; three items per thread and pass so that
        // their 24 loads are in flight together
        const int items = v.n_free * 27;
        for (int i0 = tid; i0 < items; i0 += 3 * 256) {
            double sum[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int i = i0 + u * 256;
                sum[u] = 0;
                if (i < items) {
                    const int slot = i / 27, q = i - slot * 27;
                    for (int sp = 0; sp < SPLIT; ++sp) sum[u] += v.partial[((size_t)slot * SPLIT + sp) * PV + q];
                }
            }
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int i = i0 + u * 256;
                if (i >= items) continue;
                const int slot = i / 27, q = i - slot * 27;
                const double sv = sum[u];
                if (q >= 21) { v.bp[6 * slot + (q - 21)] = sv; v.bp_loc[6 * slot + (q - 21)] = sv; }
                else {
                    int a = 0, rem = q;                    // upper-triangle index q -> (a, c)
                    while (rem >= 6 - a) { rem -= 6 - a; ++a; }
                    const int c = a + rem;
                    double* H = v.Hpp + 36 * (size_t)slot;
                    H[a * 6 + c] = sv; H[c * 6 + a] = sv;
                    if (a == c) { v.hppdiag[6 * slot + a] = sv; v.hppdiag_loc[6 * slot + a] = sv; }
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (mode == 0) {
            st_sc1(&v.scal[6], s_val[0]); st_sc1(&v.scal[7], s_val[2]);        // chi2 and max diag H_pp for the last workgroup of k_ba_point_sum
        } else {
            const double fail = v.scal[5], scale_p = v.scal[3];
            v.scal[1] = s_val[0]; v.scal[2] = s_val[1];
            if (fused) lm_decide(v, s_val[0], fail, s_val[1], scale_p, fused == 2);
        }
    }
}

// ---- linearisation 1/2: the observation side (blocks [0, obs_blocks)) and the pose side (the rest) of the accepted state in one
//      launch: both only read the state, so they run side by side.  Skipped when the previous trial launch already linearised
//      this state on speculation (ctl->spec).
__global__ __launch_bounds__(256) void k_ba_lin(const BaView* __restrict__ views, int robust, int points_fixed)
{
    BA_VIEW(v);
    BA_VIEW_HEAD("s"(v.obs_blocks), "s"(v.pose_blocks), "s"(v.ctl));
    const int obs_blocks = v.obs_blocks;
    if ((int)blockIdx.x >= obs_blocks + v.pose_blocks) return;
    const BaFlags fl = ba_flags(v.ctl);
    if (fl.idle() || !fl.need_lin || fl.spec) return;
    const int idx = fl.cur;
    if ((int)blockIdx.x < obs_blocks) obs_lin_body(v, blockIdx.x, robust, points_fixed, idx);
    else pose_part_body(v, (int)blockIdx.x - obs_blocks, robust, 0, idx);
}

// ---- chi2 of the trial state per keyframe (blocks [0, trial_blocks)); the last of them totals it and (fused) runs the lambda
//      control.  With spec != 0 the rest of the grid linearises the TRIAL state into the other linearisation set beside it: a
//      trial is accepted far more often than not, and then the next iteration starts with its linearisation done (the sets are
//      double buffered like the states, a rejected trial leaves the accepted state's set untouched).  These workgroups read
//      ctl->cur_launch, not ctl->cur, which the decision may flip while they run.
__global__ __launch_bounds__(256) void k_ba_trial(const BaView* __restrict__ views, int robust, int fused, int points_fixed, int spec, int skip_one_pass)
{
    BA_VIEW(v);
    BA_VIEW_HEAD("s"(v.part_n), "s"(v.pose_blocks), "s"(v.land_blocks), "s"(v.ctl));
    const int part_n = v.part_n, trial_blocks = v.pose_blocks, land_blocks = v.land_blocks;
    if ((int)blockIdx.x >= trial_blocks + (spec ? land_blocks + trial_blocks : 0)) return;
    if (skip_one_pass && upd_takes(v.n_points, v.n_free, v.n_poses)) return;      // that problem's trial ran in k_ba_update
    const BaFlags fl = ba_flags(v.ctl);
    if (fl.idle()) return;
    const int idx = fl.cur_launch ^ 1;
    int combine = -1;
    if ((int)blockIdx.x >= trial_blocks) {
        // the complete linearisation of the trial state into the other set: observations landmark-major with the landmark sums
        // (land_lin_body), the pose side per keyframe and slice (its partial sums are added up by their readers in k_ba_schur)
        const int bid = (int)blockIdx.x - trial_blocks;
        if (bid < land_blocks) land_lin_body(v, bid, robust, points_fixed, idx);
        else pose_part_body(v, bid - land_blocks, robust, 0, idx);
        return;                          // read by the next launch only (k_ba_schur adds the pose partials up itself): no hand-over
    } else {
        pose_part_body(v, blockIdx.x, robust, 1, idx);
        if (ba_last_block_sc1(v.ctl, trial_blocks)) combine = 1;
    }
    if (combine < 0) return;
    pose_combine_body(v, 1, part_n, fused ? (spec ? 2 : 1) : 0);
}

// partitioned solve: lambda control on the all-reduced quantities
__global__ __launch_bounds__(64) void k_lm_begin(const BaView* __restrict__ views)
{
    BA_VIEW(v);
    if (ba_idle(v.ctl) || !v.ctl->need_lin) return;
    double m = 0;
    for (int i = threadIdx.x; i < v.dim; i += 64) m = fmax(m, fabs(v.hppdiag[i]));
    m = wave_max(m);
    if (threadIdx.x == 0) lm_begin(v, m, v.scal[4], *v.chi_cur);
}
__global__ void k_lm_decide(const BaView* __restrict__ views)
{
    BA_VIEW(v);
    if (ba_idle(v.ctl)) return;
    if (threadIdx.x == 0 && blockIdx.x == 0) lm_decide(v, v.scal[1], v.scal[5], v.scal[2], v.scal[3]);
}

// Y = W (H_ll + lambda I)^-1 of one observation (6x3 times symmetric 3x3), in the operation order every user shares
__device__ __forceinline__ void obs_y_row(const double* h, double w0, double w1, double w2, double& y0, double& y1, double& y2)
{
    y0 = w0 * h[0] + w1 * h[1] + w2 * h[2];
    y1 = w0 * h[1] + w1 * h[3] + w2 * h[4];
    y2 = w0 * h[2] + w1 * h[4] + w2 * h[5];
}

// ---- per trial: Schur complement; Y = W (H_ll + lambda I)^-1 is formed per term from W and the landmark's 3x3 block (a launch
//      and the 18 doubles per observation it wrote and this kernel read back are gone).  One wavefront per pose-block pair (i <= k)
//      or part of one, over the pair's term list (observation of i, observation of k, landmark), 32 terms per round, two lanes per
//      term with 18 accumulators each; partials are summed in lane order through LDS (fixed summation order).
//      Round 6, in-kernel stamps (tools/dev_schur_stamps.py): 3675 of the 5349 workgroups of the first form were surplus parts that
//      left at once, and dispatching them kept the last real ones (the rhs blocks) waiting for 8-12 us of a 24 us launch; a workgroup's
//      own chain was five dependent round trips before its first row and then a round trip per round.  Now the grid holds the parts
//      that exist (table built with the lists, ba_build.inl), a workgroup's item record and the control flags come in one round trip,
//      and a round's 64 rows (144 bytes each) are fetched by the wavefront TOGETHER, nine lanes to a row, sixteen bytes a lane, a round
//      AHEAD of their use (registers -> LDS -> the lanes of the term).  What bounds a workgroup since is its instruction count: ~115
//      FP64 instructions (4 cycles each) + ~100 others per round of 32 terms, two wavefronts to a SIMD (1.3 us per round measured; with
//      every load hitting the L1 still 0.9).  Measured and dropped: four lanes per term with two or three rounds in flight (128- and
//      64-thread workgroups; 28.5 / 31 us: more instructions per term, or more wavefronts than the chip holds).
//      What sets the launch's duration is its longest chain of rounds (3.1 us before the first row, then 1.3-1.8 us a round), as long as
//      all workgroups are resident at once: 2048 wavefronts of this kernel (two to a SIMD).  The part size that cuts the lists is
//      therefore chosen per window, the smallest whose workgroups still fit in one generation (k_bs_blkscan).
//      The rhs of keyframe i, b_p,i - sum Y b_l over its observations, rides on the diagonal block (i, i), whose list has a term per
//      observation: no workgroups of its own and no second pass over W.
//      fused != 0 (single-GPU solve): lambda goes onto the pose diagonal, rhs straight into row `dim` of S and the failure
//      flag / rhs pivot are reset here, so no separate preparation launch is needed.
#ifdef LPSLAM_SCHUR_STAMPS
// development: (start, end, wait start) of every workgroup of the last k_ba_schur launch, 100 MHz clock (tools/dev_schur_stamps.py)
__device__ unsigned long long g_schur_stamps[8 * 8192];
#define SCHUR_STAMP(k) do { if (threadIdx.x == 0 && bx0 < 8192) g_schur_stamps[8 * bx0 + (k)] = wall_clock64(); } while (0)
#else
#define SCHUR_STAMP(k) do {} while (0)
#endif
typedef double dbl2 __attribute__((ext_vector_type(2)));      // (a plain vector type: registers, where the HIP class type ended up in scratch memory)
// a round's rows, landmark blocks and rhs vectors -> registers (term records in `ab`: lane l holds term l & 31 of the round).
// Straight-line code: every lane loads in every slot (the last slots of the landmark blocks fetch a duplicate that is never stored) --
// with a condition around a load the compiler ends each one with a full wait, the eleven lane exchanges and loads ran one after the
// other and a round cost 0.9 us of issue alone.
__device__ __forceinline__ void schur_fetch(const BaView& v, const int4& ab, int lane, bool diag, dbl2 (&wq)[9], dbl2 (&hq)[2], double (&bq)[2], int& same)
{
    const int mine = lane < 32 ? ab.x : ab.y;
    int o[9], lm[2];
#pragma unroll
    for (int j = 0; j < 9; ++j) o[j] = __shfl(mine, (j * 64 + lane) / 9);
#pragma unroll
    for (int j = 0; j < 2; ++j) lm[j] = __shfl(ab.z, min((j * 64 + lane) / 3, 31));
    same = __shfl((int)(ab.x == ab.y), lane >> 1);
    // (byte offsets in 32 bits: base in scalar registers + one vector offset per load instead of a 64-bit multiply-add each)
    GPTR(const char) Wc = reinterpret_cast<GPTR(const char)>(v.W);
    GPTR(const char) Hc = reinterpret_cast<GPTR(const char)>(v.Hll);
    GPTR(const char) Bc = reinterpret_cast<GPTR(const char)>(v.bl);
#pragma unroll
    for (int j = 0; j < 9; ++j) { const int idx = j * 64 + lane, u = idx - 9 * (idx / 9); wq[j] = *reinterpret_cast<GPTR(const dbl2)>(Wc + (144u * (unsigned)o[j] + 16u * (unsigned)u)); }
#pragma unroll
    for (int j = 0; j < 2; ++j) { const int idx = j * 64 + lane, u = idx - 3 * (idx / 3); hq[j] = *reinterpret_cast<GPTR(const dbl2)>(Hc + (48u * (unsigned)lm[j] + 16u * (unsigned)u)); }
    if (diag) {
#pragma unroll
        for (int j = 0; j < 2; ++j) { const int idx = j * 64 + lane, u = idx - 3 * (idx / 3); bq[j] = *reinterpret_cast<GPTR(const double)>(Bc + (24u * (unsigned)lm[j] + 8u * (unsigned)u)); }
    }
}
template <int UPD_PB> __device__ __forceinline__ void ba_pose_side_wave(BaView& v, int p, int sp, int robust, int cur, bool publish);
__device__ __forceinline__ void ba_pose_side_wait(const BaView& v);
__global__ __launch_bounds__(64) void k_ba_schur(const BaView* __restrict__ views, int fused, int robust)
{
    BA_VIEW_XCD(v, bx0);
    // workgroups: [pose side of an accepted state's linearisation (ba_update.inl) | further parts, first stretch | part 0 of every
    // block | further parts, the rest]
    const int lead = v.n_poses * SPLIT;
    const int nblk = v.n_blocks, ecap = v.extra_pack >> 12, efirst = v.extra_pack & 4095;
    if (bx0 >= lead + ecap + nblk || v.band_hbw >= 0) return;      // banded windows: k_schur_group / k_schur_band_reduce (ba_band.inl)
    // the item's record and the control block's flags in ONE round trip (both addresses follow from the view alone)
    const int bx = bx0 - lead;
    const bool further = bx >= 0 && (bx < efirst || bx >= efirst + nblk);
    GPTR(const int) ex = v.blk_ticket + nblk;              // [items | block * SCH_MAXP + part ...], written with the lists and constant since
    const int e = bx < efirst ? bx : bx - nblk;
    const int head = ex[0];                                // items of the table and the window's part size (schur_head)
    const int count = schur_head_count(head);
    const int item = bx < 0 ? 0 : (further ? ex[1 + min(max(e, 0), max(ecap - 1, 0))] : SCH_MAXP * v.blk_perm[bx - efirst]);
    const BaFlags fl = ba_flags(v.ctl);
    if (fl.idle()) return;
    const int pending = fused ? ba_sync_words(v)[3] : 0;   // raised by k_ba_update's decision: H_pp, b_p of state `cur` are this launch's to compute
    SCHUR_STAMP(0); SCHUR_STAMP(2);
    if (bx < 0) { if (pending) ba_pose_side_wave<2>(v, bx0 / SPLIT, bx0 % SPLIT, robust, fl.cur, true); SCHUR_STAMP(1); return; }
    if (further && e >= count) return;
    const int blk = item / SCH_MAXP, part_id = item % SCH_MAXP;
    const double lambda = fl.lambda;
    ba_lin_set(v, fl.cur);
    const int lane = threadIdx.x;
    const int n = v.dim_pad;
    const int t_begin = v.blk_start[blk], t_end = v.blk_start[blk + 1];
    const int parts = schur_parts(t_end - t_begin, schur_head_part(head));
    SCHUR_STAMP(3);
    // block -> (i, k), i <= k, blocks numbered row by row: row i starts at i N - i (i - 1) / 2
    int i;
    {
        const int N = v.n_free;
        const float h = (float)(2 * N + 1);
        i = (int)((h - sqrtf(fmaxf(h * h - 8.0f * (float)blk, 0.0f))) * 0.5f);
        i = max(0, min(i, N - 1));
        while (i > 0 && i * N - i * (i - 1) / 2 > blk) --i;
        while (i + 1 < N && (i + 1) * N - (i + 1) * i / 2 <= blk) ++i;
    }
    const int k = i + (blk - (i * v.n_free - i * (i - 1) / 2));
    const bool diag = i == k;
    // LDS: a round's rows [64][18] (0 .. 31 the terms' rows of keyframe i, 32 .. 63 of keyframe k), landmark blocks [32][6] and rhs
    // vectors [32][3]; afterwards the lanes' partial sums [32][43]
    __shared__ __attribute__((aligned(16))) double s_buf[64 * 18 + 2 * 128 + 128];      // (every lane stores in every slot: the blocks' and vectors' sections are rounded up to 128 lanes)
    double* s_h = s_buf + 64 * 18;
    double* s_b = s_h + 2 * 128;
    const int tl = lane >> 1, hp = lane & 1;
    double acc[18], r3[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < 18; ++q) acc[q] = 0;
    const int stride = 32 * parts;
    int t0 = t_begin + part_id * 32;
    // registers of the round being fetched
    dbl2 wq[9], hq[2];
    double bq[2] = {0, 0};
    int4 ab = make_int4(0, 0, 0, 0), ab_next = make_int4(0, 0, 0, 0);
    int same_next = 0;
    if (t0 < t_end) {
        ab = v.blk_terms[min(t0 + (lane & 31), t_end - 1)];
        if (t0 + stride < t_end) ab_next = v.blk_terms[min(t0 + stride + (lane & 31), t_end - 1)];
        schur_fetch(v, ab, lane, diag, wq, hq, bq, same_next);
    }
    SCHUR_STAMP(4);
    bool first_round = true;
    while (t0 < t_end) {
#pragma unroll
        for (int j = 0; j < 9; ++j) *reinterpret_cast<dbl2*>(s_buf + 2 * (j * 64 + lane)) = wq[j];
        *reinterpret_cast<dbl2*>(s_h + 2 * lane) = hq[0];
        *reinterpret_cast<dbl2*>(s_h + 2 * (64 + lane)) = hq[1];
        if (diag) { s_b[lane] = bq[0]; s_b[64 + lane] = bq[1]; }
        const bool valid = t0 + tl < t_end;
        const bool same = same_next != 0;
        __syncthreads();
        if (first_round) { SCHUR_STAMP(5); first_round = false; }
        t0 += stride;
        if (t0 < t_end) {
            ab = ab_next;
            schur_fetch(v, ab, lane, diag, wq, hq, bq, same_next);
            if (t0 + stride < t_end) ab_next = v.blk_terms[min(t0 + stride + (lane & 31), t_end - 1)];
        }
        if (valid) {
            double hraw[6], y[9], w[18];
            const double* ya = s_buf + 18 * tl + 9 * hp;
            const dbl2* wb = reinterpret_cast<const dbl2*>(s_buf + 18 * (32 + tl));
#pragma unroll
            for (int q = 0; q < 6; ++q) hraw[q] = s_h[6 * tl + q];
#pragma unroll
            for (int q = 0; q < 9; ++q) y[q] = ya[q];
#pragma unroll
            for (int q = 0; q < 9; ++q) { const dbl2 b2 = wb[q]; w[2 * q] = b2.x; w[2 * q + 1] = b2.y; }
            double h[6];
            point_hinv(hraw, lambda, h);
#pragma unroll
            for (int r = 0; r < 3; ++r) {                  // Y = W (H_ll + lambda I)^-1, row r of this lane's half
                const double w0 = y[r * 3], w1 = y[r * 3 + 1], w2 = y[r * 3 + 2];
                y[r * 3] = __builtin_fma(w2, h[2], __builtin_fma(w1, h[1], w0 * h[0]));
                y[r * 3 + 1] = __builtin_fma(w2, h[4], __builtin_fma(w1, h[3], w0 * h[1]));
                y[r * 3 + 2] = __builtin_fma(w2, h[5], __builtin_fma(w1, h[4], w0 * h[2]));
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    acc[r * 6 + c] = __builtin_fma(y[r * 3 + 2], w[c * 3 + 2], __builtin_fma(y[r * 3 + 1], w[c * 3 + 1], __builtin_fma(y[r * 3], w[c * 3], acc[r * 6 + c])));      // (fused: the kernel is bound by its vector instructions, 4 cycles each)
            if (diag && same) {                            // the observation's share of the keyframe's rhs (a keyframe that sees a landmark twice has cross terms in its list: not those)
                const double b0 = s_b[3 * tl], b1 = s_b[3 * tl + 1], b2 = s_b[3 * tl + 2];
#pragma unroll
                for (int r = 0; r < 3; ++r) r3[r] = __builtin_fma(y[r * 3 + 2], b2, __builtin_fma(y[r * 3 + 1], b1, __builtin_fma(y[r * 3], b0, r3[r])));
            }
        }
        __syncthreads();
    }
    SCHUR_STAMP(6);
    // the lanes' sums in lane order: per term-lane pair [row half 0: 18 + 3 | row half 1: 18 + 3], stride 43
    double* part = s_buf;
#pragma unroll
    for (int q = 0; q < 18; ++q) part[tl * 43 + 21 * hp + q] = acc[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) part[tl * 43 + 21 * hp + 18 + q] = r3[q];
    __syncthreads();
    // lanes 0 .. 35: entry (r, c) of the 6 x 6 sum; lanes 36 .. 41: row lane - 36 of the keyframe's rhs sum (diagonal blocks)
    const int er = lane < 36 ? lane / 6 : lane - 36, ec = lane < 36 ? lane - 6 * er : 0;
    const int slot = 21 * (er / 3) + (lane < 36 ? 6 * (er % 3) + ec : 18 + er % 3);
    double sum = 0;
    if (lane < SCH_PV) for (int l = 0; l < 32; ++l) sum += part[l * 43 + slot];
    SCHUR_STAMP(7);
    if (parts > 1) {
        // hand-over without cache maintenance: the partial sums are stored write-through (sc1) and read back L1-bypassing (sc1),
        // the ticket is a relaxed agent-scope add made after this (single) wavefront's stores have drained -- no buffer_wbl2 /
        // buffer_inv, which cost more than the part they guard (MI355X_MICROARCH: valid forms, one unsharded counter)
        double* mine = v.blk_part + (size_t)(SCH_MAXP * blk + part_id) * SCH_PV;
        if (lane < SCH_PV) __hip_atomic_store(&mine[lane], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __shared__ int s_last;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            const int tk = __hip_atomic_fetch_add(&v.blk_ticket[blk], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (tk == parts - 1);
            if (s_last) v.blk_ticket[blk] = 0;
        }
        __syncthreads();
        if (!s_last) { SCHUR_STAMP(1); return; }
        sum = 0;
        if (lane < SCH_PV) for (int p = 0; p < parts; ++p) sum += __hip_atomic_load(&v.blk_part[(size_t)(SCH_MAXP * blk + p) * SCH_PV + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    SCHUR_STAMP(2);
    if (diag && pending) ba_pose_side_wait(v);             // the leading workgroups of this launch have stored the pose side (write-through)
    SCHUR_STAMP(1);
    if (lane < 36) {
        const int r = er, c = ec;
        if (diag) {
            const int ra = min(r, c), rc = max(r, c);
            const int q = 6 * ra - ra * (ra - 1) / 2 + (rc - ra);      // H_pp(r, c) in the row-major upper triangle of the pose partials
            double hpp = 0;
            for (int sp = 0; sp < SPLIT; ++sp) { const double* pr = v.partial + ((size_t)i * SPLIT + sp) * PV + q; hpp += pending ? ld_sc1(pr) : *pr; }
            double val = hpp - sum;
            if (fused && r == c) val += lambda;
            v.S[(size_t)(6 * i + r) * n + 6 * i + c] = val;
        } else {
            v.S[(size_t)(6 * i + r) * n + 6 * k + c] = -sum;
            v.S[(size_t)(6 * k + c) * n + 6 * i + r] = -sum;
        }
    } else if (diag && lane < SCH_PV) {
        // b_p and diag H_pp of keyframe i: the SPLIT partial sums of the set's pose-side linearisation, added in order (what
        // pose_combine_body does after an explicit linearisation; a linearisation made beside a trial has no combine of its own)
        const int q = er;
        const int qd = 6 * q - q * (q - 1) / 2;              // (q, q) in the row-major upper triangle
        double bsum = 0, dsum = 0;
        for (int sp = 0; sp < SPLIT; ++sp) { const double* pr = v.partial + ((size_t)i * SPLIT + sp) * PV; bsum += pending ? ld_sc1(pr + 21 + q) : pr[21 + q]; dsum += pending ? ld_sc1(pr + qd) : pr[qd]; }
        const double val = bsum - sum;
        v.rhs[6 * i + q] = val;
        if (fused) v.S[(size_t)v.dim * n + 6 * i + q] = val;
        v.bp[6 * i + q] = bsum; v.hppdiag[6 * i + q] = dsum;      // the solved set's sums (partitioned: fresh partials for the all-reduce)
    } else if (diag && i == 0) {
        if (!fused && lane == 62) *v.chi_cur = *v.chi_loc;
        if (fused && lane == 63) { v.S[(size_t)v.dim * n + v.dim] = 1e200; v.scal[5] = 0.0; }
    }
}

// preparation for the partitioned (all-reduced) solve: lambda on the diagonal, rhs row, flag / pivot reset
__global__ __launch_bounds__(256) void k_chol_prep(const BaView* __restrict__ views)
{
    BA_VIEW(v);
    if (ba_idle(v.ctl)) return;
    const double lambda = v.ctl->lambda;
    const int n = v.dim_pad, dim = v.dim;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { v.scal[5] = 0.0; v.S[(size_t)dim * n + dim] = 1e200; }
    if (i < dim) { v.S[(size_t)i * n + i] += lambda; v.S[(size_t)dim * n + i] = v.rhs[i]; }
    else if (i < n && i > dim) v.S[(size_t)i * n + i] = 1.0;      // the all-reduce summed the identity padding
}

__device__ __forceinline__ void pose_oplus(const double* pose, const double* d, double* out)
{
    const double wx = d[0], wy = d[1], wz = d[2];
    const double theta2 = wx * wx + wy * wy + wz * wz;
    const double theta = sqrt(theta2);
    double a, b, c, qe[4];
    if (theta < 0.00001) {
        a = 1.0; b = 0.5; c = 1.0 / 6.0;
        qe[0] = 1.0; qe[1] = 0.5 * wx; qe[2] = 0.5 * wy; qe[3] = 0.5 * wz;
    } else {
        a = sin(theta) / theta;
        b = (1 - cos(theta)) / theta2;
        c = (theta - sin(theta)) / (theta2 * theta);
        const double sh = sin(0.5 * theta) / theta;
        qe[0] = cos(0.5 * theta); qe[1] = sh * wx; qe[2] = sh * wy; qe[3] = sh * wz;
    }
    const double Wm[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double W2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += Wm[i * 3 + k] * Wm[k * 3 + j]; W2[i * 3 + j] = s; }
    double Re[9], V[9];
    for (int i = 0; i < 9; ++i) { const double I = (i % 4 == 0) ? 1.0 : 0.0; Re[i] = I + a * Wm[i] + b * W2[i]; V[i] = I + b * Wm[i] + c * W2[i]; }
    const double* t = pose + 4;
    double tn[3];
    for (int i = 0; i < 3; ++i)
        tn[i] = V[i * 3] * d[3] + V[i * 3 + 1] * d[4] + V[i * 3 + 2] * d[5] + Re[i * 3] * t[0] + Re[i * 3 + 1] * t[1] + Re[i * 3 + 2] * t[2];
    const double* q = pose;
    double qn[4];
    qn[0] = qe[0] * q[0] - qe[1] * q[1] - qe[2] * q[2] - qe[3] * q[3];
    qn[1] = qe[0] * q[1] + qe[1] * q[0] + qe[2] * q[3] - qe[3] * q[2];
    qn[2] = qe[0] * q[2] - qe[1] * q[3] + qe[2] * q[0] + qe[3] * q[1];
    qn[3] = qe[0] * q[3] + qe[1] * q[2] - qe[2] * q[1] + qe[3] * q[0];
    const double nn = sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
    for (int i = 0; i < 4; ++i) out[i] = qn[i] / nn;
    for (int i = 0; i < 3; ++i) out[4 + i] = tn[i];
}


// ---- blocked Cholesky of S (+ lambda I), 32-wide panel columns, two per launch ------------------------------------------------
//   Two kinds of extra rows ride along so that no triangular substitution is ever run:
//     row `dim` of S carries the rhs            -> after the last panel it holds y = L^-1 rhs,
//     Minv starts as the identity (synthesised) -> its row blocks become L^-T; block (e, .) only exists from column e on.
//   A panel is factored by ONE wavefront in two 16-column strips (chol_panel_dpp, chol_panel.inl): the diagonal block replicated in every
//   16-lane DPP row, the rows that ride along one per lane; the same rank-1 updates factor D and solve B L_jj^T = B.  The
//   diagonal block is factored redundantly by every panel workgroup, which removes every dependence between workgroups of a launch.
//   All working workgroups run on one XCD: the grid is launched 8x oversized and only every 8th workgroup works (workgroups go
//   round-robin to the 8 XCDs), so the panel written by one launch is an L2 hit for the next (measured: -1 us per launch).
// Explicit FMAs are used here (the contraction pragma only governs implicit fusing): the factor's bits are not a parity quantity.
// What the factor-and-solve must deliver is x_p itself: a forward error within n kappa_2 2^-53 of the exact solution and within the
// measured margin of a float64 Cholesky solve on the host -- the accuracy table of DESIGN.md 36 (profiles/solve_accuracy.txt),
// held by tests/test_ba_solve_gpu.py through lpslam_hip_ba_debug_solve.  The LM trajectory (chi2 / poses, tolerances in DESIGN.md)
// sees an error of the step only to second order.
// Launch m factors panel columns j = 2m and j1 = 2m + 1 and applies the previous pair (kb0 = 2m - 2, kb1 = 2m - 1) to the rest of
// the trailing matrix: one kernel boundary per two panels on the critical path.  A panel workgroup (row block i, or
// Minv row block e) keeps its five blocks  D_j, X = A_j1,j, D_j1, B0 = A_i,j, B1 = A_i,j1  in LDS:
//   1. lookahead with the previous pair (K = 64, matrix cores): the LEFT halves of D_j, X, B0 on all four wavefronts;
//   2. wavefront 0 factors [D_j; X] -> L_jj, L_j1,j and wavefront 1 [D_j; B0] -> L_i,j in registers, while
//      wavefronts 2 and 3 finish the right halves, announce them, and go on with the lookahead of D_j1 and B1;
//   3. D_j1 -= L_j1,j L_j1,j^T, B1 -= L_i,j L_j1,j^T (matrix cores), left halves;
//   4. wavefront 0 factors [D_j1; B1] -> L_j1,j1, L_i,j1 while wavefronts 1-3 finish the right halves, announce them and store
//      step 2's blocks.
// A panel starts strip A on the left halves alone and takes the right ones behind the announcement (chol_panel_split).
// D_j, X and D_j1 are factored redundantly by every panel workgroup; nobody overwrites them in S during the launch, and no later
// launch needs L_jj, L_j1,j or L_j1,j1.  Their one reader is k_chol_xsolve, which takes the rhs row out of the system's LAST panel
// column: the diagonal workgroup publishes the rhs row of that column's diagonal block into Ldiag and, when it is the second column of a
// pair, L_j1,j into Lsub -- in the system's last launch and in no other.  In every other launch the diagonal workgroup
// only raises the pivot flag.  With an odd number of panels the last launch is `single`: only column j, factored by wavefront 0 alone.
// The LAST panel column of a system (step 4 of its last launch, or step 2 of a `single` one) stops after its dim - 32 (nb - 1) real
// columns (chol_panel_trim): what follows them -- the rhs row's diagonal, the identity padding -- is read by nobody.
constexpr int CP_BLK = NB * (NB + 1);                  // one padded 32x32 block in LDS
// 11 blocks + the factor scratch of two wavefronts + the two announcement counters (chol_panel_split)
constexpr int CP_LDS_BYTES = (11 * CP_BLK + 2 * (64 * 17 + 64 * 17) + 2) * (int)sizeof(double);

constexpr int CH_SCR = 64 * 17 + 64 * 17;              // doubles of scratch per factoring wavefront: L1 [64][17] and U [64][17]
// the strips, the panel [D; B] in registers and the 32-wide tile product: shared with tools/dev/panel_bench.hip
#include "chol_panel.inl"

#ifdef LPSLAM_PAIR_STAMPS
// development: shader-clock stamps of the diagonal workgroup, the first row workgroup and the first Minv workgroup of launches
// m = 0 .. 7 of view 0, 24 slots each (tools/dev/pair_stamps.py names them)
__device__ unsigned long long g_pair_stamps[8 * 3 * 24];
#define PAIR_STAMP(k, cond) do { if (stamp_kind >= 0 && (cond) && lane == 0) g_pair_stamps[(m * 3 + stamp_kind) * 24 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
// wait start, wait end (chol_panel_split) and panel written out
#define PAIR_PANEL_STAMPS(k, p) do { if (stamp_kind >= 0 && lane == 0) { unsigned long long* g = g_pair_stamps + (m * 3 + stamp_kind) * 24 + (k); \
        g[0] = (p).clk[0]; g[1] = (p).clk[1]; g[2] = __builtin_amdgcn_s_memtime(); } } while (0)
#else
#define PAIR_STAMP(k, cond) do {} while (0)
#define PAIR_PANEL_STAMPS(k, p) do {} while (0)
#endif

__global__ __launch_bounds__(256, 2) void k_chol_pair(const BaView* __restrict__ views, int m, int pin, int skip_small)
{
    if (pin && (blockIdx.x & 7)) return;                 // small launches: XCD 0 only (see above); large ones use the whole chip
#ifdef LPSLAM_PAIR_STAMPS
    const unsigned long long t_entry = __builtin_amdgcn_s_memtime();
#endif
    // Everything this kernel reads of its view, fetched in ONE round trip: left to itself the compiler loads each member where it
    // is first used, and the prologue becomes a chain of dependent round trips (measured: 3 us of an 18 us launch went into ten
    // of them -- arguments, sizes, control block, pointers, four passes of block loads).
    const BaView& vw = views[blockIdx.y];
    const int dim = vw.dim, n = vw.dim_pad, band = vw.band_hbw;
    GPTR(double) S = vw.S; GPTR(double) M = vw.Minv; GPTR(double) Ldiag = vw.Ldiag; GPTR(double) Lsub = vw.Lsub; GPTR(double) scal = vw.scal;
    GPTR(BaCtl) ctl = vw.ctl;
    asm volatile("" :: "s"(dim), "s"(n), "s"(S), "s"(M), "s"(Ldiag), "s"(Lsub), "s"(scal), "s"(ctl), "s"(band));
    const int nb = n / NB;
    if (2 * m >= nb || dim == 0 || band >= 0 || (skip_small && cw_fits(dim))) return;   // a batch runs the panel pairs of its largest system; small systems may be k_chol_wg's
    const int bid = pin ? blockIdx.x >> 3 : blockIdx.x;
    {
        const int ncol0 = (2 * m + 1 < nb) ? 2 : 1, T0 = nb - 2 * m - ncol0;
        if (bid >= 1 + T0 + 2 * m + ncol0 + (m > 0 ? T0 * (T0 + 1) / 2 + 2 * m * T0 : 0)) return;
    }
    // the control block travels with the block loads below (no short circuit: one round trip, awaited after they are issued)
    const int c_stopped = ctl->stopped, c_done = ctl->outer_done, c_max = ctl->max_outer;
    extern __shared__ double cp_lds[];
    const int j = 2 * m, j1 = j + 1;
    const bool single = j1 >= nb;
    const bool prev = m > 0;
    const int kb0 = j - 2, kb1 = j - 1;
    const int ncol = single ? 1 : 2;
    const int n_rows = nb - j - ncol;                    // square row blocks below the pair
    const int n_extra = j + ncol;                        // Minv row blocks 0 .. j (j1)
    const int n_panel = 1 + n_rows + n_extra;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tr = (wave >> 1) * 16, tc = (wave & 1) * 16, lr = tid & 15, lk = lane >> 4;
    // A block of the matrix on its way into LDS: mode 0 copy from memory, 1 zero, 2 identity.  Every block is LOADED, whatever
    // its mode (blocks that are not read point at the pair's own diagonal block, which always exists): with the loads
    // unconditional all of them -- 44 per thread in a panel workgroup -- are in flight together, one round trip.
    struct Blk { const double* p; int mode; };
    auto blk = [&](const double* src, size_t r0, size_t c0, int mode) -> Blk {
        return mode == 0 ? Blk{src + r0 * n + c0, 0} : Blk{S + (size_t)j * NB * n + (size_t)j * NB, mode};
    };
    auto fill = [&](int mode, double ld, int r, int c) -> double { return mode == 0 ? ld : (mode == 2 && r == c ? 1.0 : 0.0); };
    if (bid >= n_panel) {
        // ---- trailing update of block (i2, j2), j2 >= j + ncol, with the previous pair
        const int T = nb - j - ncol;
        int u = bid - n_panel;
        const int n_sq_upd = T * (T + 1) / 2;
        double* dst; const double* srcI; size_t ri, rj; bool overwrite = false; int e = -1;
        if (u < n_sq_upd) {
            int bi = 0;
            while (u > bi) { u -= bi + 1; ++bi; }
            ri = (size_t)(j + ncol + bi) * NB; rj = (size_t)(j + ncol + u) * NB; dst = S; srcI = S;
        } else {
            u -= n_sq_upd;
            e = u / T;
            ri = (size_t)e * NB; rj = (size_t)(j + ncol + (u - e * T)) * NB; dst = M; srcI = M;
            overwrite = e >= kb0;                        // first contribution to this block: it holds no value yet
        }
        double* Li0 = cp_lds; double* Li1 = cp_lds + CP_BLK; double* Lj0 = cp_lds + 2 * CP_BLK; double* Lj1 = cp_lds + 3 * CP_BLK;
        // Minv block (e, k) is structurally zero for k < e
        const Blk bk[4] = {blk(srcI, ri, (size_t)kb0 * NB, e > kb0 ? 1 : 0), blk(srcI, ri, (size_t)kb1 * NB, e > kb1 ? 1 : 0),
                           blk(S, rj, (size_t)kb0 * NB, 0), blk(S, rj, (size_t)kb1 * NB, 0)};
        f64x2 ld[2][4];                                  // two adjacent columns per lane: 16-byte loads, 16 lanes to a 256-byte row
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int t = 2 * tid + it * 512, r = t / NB, c = t % NB;
#pragma unroll
            for (int q = 0; q < 4; ++q) ld[it][q] = *reinterpret_cast<const f64x2*>(bk[q].p + (size_t)r * n + c);
        }
        double old[4];
        if (!overwrite) {
#pragma unroll
            for (int q = 0; q < 4; ++q) old[q] = dst[(ri + tr + lk + 4 * q) * n + rj + tc + lr];
        }
        if (c_stopped | (c_done >= c_max)) return;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int t = 2 * tid + it * 512, r = t / NB, c = t % NB, o = r * (NB + 1) + c;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                Li0[o + h] = fill(bk[0].mode, ld[it][0][h], r, c + h); Li1[o + h] = fill(bk[1].mode, ld[it][1][h], r, c + h);
                Lj0[o + h] = ld[it][2][h]; Lj1[o + h] = ld[it][3][h];
            }
        }
        __syncthreads();
        f64x4 acc = {0, 0, 0, 0};
        acc = mfma_tile32(Li0, Lj0, tr, tc, lr, lk, acc);
        acc = mfma_tile32(Li1, Lj1, tr, tc, lr, lk, acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[(ri + tr + lk + 4 * q) * n + rj + tc + lr] = overwrite ? -acc[q] : old[q] - acc[q];
        return;
    }
    // ---- panel workgroup
    const bool diag = bid == 0;
    const bool extra = bid > n_rows;
    const int i = diag ? j : (extra ? bid - 1 - n_rows : j + ncol + bid - 1);       // row block (extra: Minv row e)
    const size_t rj = (size_t)j * NB, rj1 = (size_t)j1 * NB, ri = (size_t)i * NB;
    const bool has_b = !diag;
    const double* Bsrc = extra ? M : S;
#ifdef LPSLAM_PAIR_STAMPS
    const int stamp_kind = (blockIdx.y != 0 || m >= 8) ? -1 : (diag ? 0 : (bid == 1 && n_rows > 0 ? 1 : (bid == n_rows + 1 ? 2 : -1)));
    if (stamp_kind >= 0 && tid == 0) g_pair_stamps[(m * 3 + stamp_kind) * 24] = t_entry;
#endif
    double* Dj = cp_lds;               double* X = cp_lds + CP_BLK;        double* Dj1 = cp_lds + 2 * CP_BLK;
    double* B0 = cp_lds + 3 * CP_BLK;  double* B1 = cp_lds + 4 * CP_BLK;
    double* Ljk0 = cp_lds + 5 * CP_BLK; double* Ljk1 = cp_lds + 6 * CP_BLK;      // row j of the previous pair (later: L_j1,j and L_i,j)
    double* Lj1k0 = cp_lds + 7 * CP_BLK; double* Lj1k1 = cp_lds + 8 * CP_BLK;
    double* Lik0 = cp_lds + 9 * CP_BLK; double* Lik1 = cp_lds + 10 * CP_BLK;
    // Minv row e: block (e, e) starts as the identity, blocks left of it are zero, blocks right of it hold a value only once a
    // trailing update of an earlier launch has written them (e < kb0)
    const int mode0 = !has_b ? 1 : (!extra ? 0 : (i == j ? 2 : (i > j || i >= kb0 ? 1 : 0)));
    const int mode1 = (!has_b || single) ? 1 : (!extra ? 0 : (i == j1 ? 2 : (i >= kb0 ? 1 : 0)));
    const int ms = single ? 1 : 0;                                             // second-column blocks do not exist
    const int mp = prev ? 0 : 1, mps = (prev && !single) ? 0 : 1;
    const int mi0 = (!prev || !has_b || (extra && i > kb0)) ? 1 : 0, mi1 = (!prev || !has_b || (extra && i > kb1)) ? 1 : 0;
    const size_t c0 = (size_t)(prev ? kb0 : 0) * NB, c1 = (size_t)(prev ? kb1 : 0) * NB;
    // in the order of the LDS blocks: Dj X Dj1 B0 B1 Ljk0 Ljk1 Lj1k0 Lj1k1 Lik0 Lik1
    const Blk bk[11] = {blk(S, rj, rj, 0), blk(S, rj1, rj, ms), blk(S, rj1, rj1, ms), blk(Bsrc, ri, rj, mode0), blk(Bsrc, ri, rj1, mode1),
                        blk(S, rj, c0, mp), blk(S, rj, c1, mp), blk(S, rj1, c0, mps), blk(S, rj1, c1, mps), blk(Bsrc, ri, c0, mi0), blk(Bsrc, ri, c1, mi1)};
    {
        f64x2 ld[2][11];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int t = 2 * tid + it * 512, r = t / NB, c = t % NB;
#pragma unroll
            for (int q = 0; q < 11; ++q) ld[it][q] = *reinterpret_cast<const f64x2*>(bk[q].p + (size_t)r * n + c);
        }
        if (c_stopped | (c_done >= c_max)) return;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int t = 2 * tid + it * 512, r = t / NB, c = t % NB, o = r * (NB + 1) + c;
#pragma unroll
            for (int q = 0; q < 11; ++q) {
                cp_lds[q * CP_BLK + o] = fill(bk[q].mode, ld[it][q][0], r, c);
                cp_lds[q * CP_BLK + o + 1] = fill(bk[q].mode, ld[it][q][1], r, c + 1);
            }
        }
    }
    // the announcements of the right halves (chol_panel_split): [0] step 1's, two wavefronts; [1] step 3's, three
    int* const gate = reinterpret_cast<int*>(cp_lds + 11 * CP_BLK + 2 * CH_SCR);
    if (tid == 0) { gate[0] = 0; gate[1] = 0; }
    PAIR_STAMP(1, wave == 0);
    __syncthreads();
    // One 16x16 tile (r, c) of a block, D -= A0 Bk0^T + A1 Bk1^T (K = 64) or D -= A0 Bk0^T (K = 32): a chain of mfma_tile32 calls of
    // its own, so its bits do not depend on the wavefront that runs it or on when.  Tile (0, 1) of D_j and D_j1 is never computed:
    // panel loads read the lower triangle of a diagonal block, and the factored block is not written back.
    auto tile64 = [&](double* D, const double* A0, const double* A1, const double* Bk0, const double* Bk1, int r, int c) __attribute__((always_inline)) {
        f64x4 acc = {0, 0, 0, 0};
        acc = mfma_tile32(A0, Bk0, 16 * r, 16 * c, lr, lk, acc); acc = mfma_tile32(A1, Bk1, 16 * r, 16 * c, lr, lk, acc);
        tile_sub(D, 16 * r, 16 * c, lr, lk, acc);
    };
    auto tile32 = [&](double* D, const double* A0, const double* Bk0, int r, int c) __attribute__((always_inline)) {
        f64x4 acc = {0, 0, 0, 0};
        acc = mfma_tile32(A0, Bk0, 16 * r, 16 * c, lr, lk, acc);
        tile_sub(D, 16 * r, 16 * c, lr, lk, acc);
    };
    // 1. lookahead of the blocks the first factorisations need, LEFT halves first (strip A of a panel reads columns 0-15 only):
    //      round 1   D_j (0,0) | D_j (1,0) | X (0,0) | X (1,0)          round 2   B0 (0,0) | B0 (1,0) | D_j (1,1) | X (0,1)
    //    The right halves that remain -- X (1,1) on wavefront 2, B0 (0,1) and (1,1) on wavefront 3 -- run beside strip A (step 2).
    if (prev) {
        if (wave < 2) tile64(Dj, Ljk0, Ljk1, Ljk0, Ljk1, wave, 0);
        else if (!single) tile64(X, Lj1k0, Lj1k1, Ljk0, Ljk1, wave - 2, 0);
        if (wave < 2) { if (has_b) tile64(B0, Lik0, Lik1, Ljk0, Ljk1, wave, 0); }
        else if (wave == 2) tile64(Dj, Ljk0, Ljk1, Ljk0, Ljk1, 1, 1);
        else if (!single) tile64(X, Lj1k0, Lj1k1, Ljk0, Ljk1, 0, 1);
    }
    __syncthreads();
    PAIR_STAMP(2, wave == 0);
    const int want1 = prev ? 2 : 0;                      // wavefronts 2 and 3 announce step 1's right halves
    bool fail = false;
    const int need = min(max(dim - NB * (nb - 1), 0), NB);       // real columns of the system's last panel column (chol_panel_trim)
    // Ldiag and Lsub have one reader, k_chol_xsolve, and it reads the blocks of the system's last panel column alone (the rhs row lives
    // there): a `single` launch's column is that one, a pair's first column never is, its second column is in the system's last launch.
    // From the view's own size, as `need`: in a batch the chain goes on behind a shorter system's last launch.
    const bool last1 = j1 == nb - 1;
    // The factored row blocks leave the registers through LDS (every lane owns a ROW there): the workgroup then stores them to memory
    // 32 lanes to a row, where a lane-per-row store touched one cache line per lane (2.4k cycles of the factoring wavefront).
    // L_j1,j goes into Ljk0's place, L_i,j into Ljk1's, L_i,j1 into B1's.  The factored diagonal block stays in the registers.
    auto panel_to_lds = [&](const PanelRegs& p, double* Lb) {
        if (lane >= 16 && lane < 48 && Lb) {
#pragma unroll
            for (int c = 0; c < 16; ++c) { Lb[(lane - 16) * (NB + 1) + c] = p.x[c]; Lb[(lane - 16) * (NB + 1) + 16 + c] = p.y[c]; }
        }
    };
    // Of the last column's diagonal block k_chol_xsolve reads ONE row: row `need`, the rhs row, columns < need.  The lane that holds it
    // (rows 0-15 of the block: dA; rows 16-31: x | dB) stores it from its registers, two columns a store: at most 16 stores of one
    // lane, where the whole block went through LDS (64 ds_write_b64 of the factoring wavefront) and then to memory.  With an odd `need`
    // the last pair reaches column `need` itself, which nobody reads.  Nothing else of Ldiag is written.
    auto rhs_row_to_memory = [&](const PanelRegs& p, double* blk) {                // wavefront 0
        if (lane == (need & 15)) {
            f64x2* dst = reinterpret_cast<f64x2*>(blk + (size_t)need * NB);
            if (need < 16) {
#pragma unroll
                for (int c = 0; c < 16; c += 2) if (c < need) dst[c / 2] = f64x2{p.dA[c], p.dA[c + 1]};
            } else {
#pragma unroll
                for (int c = 0; c < 16; c += 2) {
                    dst[c / 2] = f64x2{p.x[c], p.x[c + 1]};
                    if (16 + c < need) dst[8 + c / 2] = f64x2{p.dB[c], p.dB[c + 1]};
                }
            }
        }
    };
    auto block_to_memory = [&](const double* L, double* dst, size_t pitch) {       // all four wavefronts
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int t = tid + it * 256, r = t / NB, c = t % NB;
            dst[(size_t)r * pitch + c] = L[r * (NB + 1) + c];
        }
    };
    auto block_to_memory3 = [&](const double* L, double* dst, size_t pitch) {      // wavefronts 1-3, six rows a pass
#pragma unroll
        for (int it = 0; it < 6; ++it) {
            const int t = tid - 64 + it * 192, r = t / NB, c = t % NB;
            if (t < NB * NB) dst[(size_t)r * pitch + c] = L[r * (NB + 1) + c];
        }
    };
    // Every factoring wavefront passes the announcement before it writes its panel out (panel_to_lds overwrites Ljk0 and Ljk1,
    // which the right-half tiles read): chol_panel_split waits in all of its paths.
    if (wave == 0) {
        PanelRegs p;
        PAIR_STAMP(3, true);
        if (single) {                                    // 2. the system's last panel column alone: [D_j; B0] -> L_jj / L_i,j, cut short
            fail = chol_panel_split<true>(p, Dj, has_b ? B0 : nullptr, lane, cp_lds + 11 * CP_BLK, gate, want1, need);
            panel_to_lds(p, has_b ? Ljk1 : nullptr);
            if (diag) rhs_row_to_memory(p, Ldiag + (size_t)j * NB * NB);
        } else {                                         // 2a. [D_j; X] -> L_jj, L_j1,j
            fail = chol_panel_split<false>(p, Dj, X, lane, cp_lds + 11 * CP_BLK, gate, want1, NB);
            panel_to_lds(p, Ljk0);                                                     // L_j1,j for step 3
        }
        PAIR_PANEL_STAMPS(4, p);
        if (diag && fail && lane == 0) scal[5] = 1.0;
    } else if (wave == 1) {
        if (!single && has_b) {                          // 2b. [D_j; B0] -> L_i,j
            PanelRegs p;
            PAIR_STAMP(7, true);
            chol_panel_split<false>(p, Dj, B0, lane, cp_lds + 11 * CP_BLK + CH_SCR, gate, want1, NB);
            panel_to_lds(p, Ljk1);
            PAIR_PANEL_STAMPS(8, p);
        }
    } else if (prev) {
        // the right halves step 1 left over, then 2c, the rest of the lookahead: D_j1 (0,0) (1,0) (1,1) and B1 (0,0) on wavefront 2,
        // B1 (0,1) (1,0) (1,1) on wavefront 3 -- five tiles each behind step 1's barrier, 80 MFMAs against the ~118 a panel has room for
        if (wave == 2) { if (!single) tile64(X, Lj1k0, Lj1k1, Ljk0, Ljk1, 1, 1); }
        else if (has_b) { tile64(B0, Lik0, Lik1, Ljk0, Ljk1, 0, 1); tile64(B0, Lik0, Lik1, Ljk0, Ljk1, 1, 1); }
        panel_gate_open(gate, lane);
        PAIR_STAMP(15 + wave, true);
        if (!single) {
            for (int t4 = 0; t4 < 4; ++t4) {
                const bool d = wave == 2 && t4 < 3;      // a tile of D_j1
                if (!d && (!has_b || (wave == 3 && t4 == 0))) continue;
                const int r2 = d ? (t4 + 1) >> 1 : (wave == 2 ? 0 : t4 >> 1), c2 = d ? t4 >> 1 : (wave == 2 ? 0 : t4 & 1);
                tile64(d ? Dj1 : B1, d ? Lj1k0 : Lik0, d ? Lj1k1 : Lik1, Lj1k0, Lj1k1, r2, c2);
            }
        }
        PAIR_STAMP(17 + wave, true);
    }
    __syncthreads();
    PAIR_STAMP(11, wave == 0);
    if (single) {
        if (!diag) block_to_memory(Ljk1, (extra ? M : S) + ri * n + rj, n);
        PAIR_STAMP(23, wave == 0);
        return;
    }
    // 3. the second column sees the first (K = 32), left halves first:  D_j1 (0,0) | D_j1 (1,0) | B1 (0,0) | B1 (1,0)
    if (wave < 2) tile32(Dj1, Ljk0, Ljk0, wave, 0);
    else if (has_b) tile32(B1, Ljk1, Ljk0, wave - 2, 0);
    __syncthreads();
    PAIR_STAMP(12, wave == 0);
    if (wave == 0) {                                     // 4. [D_j1; B1] -> L_j1,j1, L_i,j1
        PanelRegs p;
        PAIR_STAMP(13, true);
        fail = last1 ? chol_panel_split<true>(p, Dj1, has_b ? B1 : nullptr, lane, cp_lds + 11 * CP_BLK, gate + 1, 3, need)
                            : chol_panel_split<false>(p, Dj1, has_b ? B1 : nullptr, lane, cp_lds + 11 * CP_BLK, gate + 1, 3, NB);
        panel_to_lds(p, has_b ? B1 : nullptr);
        if (diag && last1) rhs_row_to_memory(p, Ldiag + (size_t)j1 * NB * NB);
        PAIR_PANEL_STAMPS(14, p);
        if (diag && fail && lane == 0) scal[5] = 1.0;
    } else {
        // beside strip A: D_j1 (1,1) | B1 (0,1) | B1 (1,1), announced; then step 2's blocks leave for memory in the panel's shadow
        // (step 4 touches none of X, Ljk0, Ljk1)
        if (wave == 1) tile32(Dj1, Ljk0, Ljk0, 1, 1);
        else if (has_b) tile32(B1, Ljk1, Ljk0, wave - 2, 1);
        panel_gate_open(gate + 1, lane);
        if (diag) {
            // L_j1,j for k_chol_xsolve: the rhs row lives in block j1.  Not into S: the other panel workgroups read A_j1,j.
            if (last1) block_to_memory3(Ljk0, Lsub + (size_t)j1 * NB * NB, NB);
        } else {
            block_to_memory3(Ljk1, (extra ? M : S) + ri * n + rj, n);
        }
        PAIR_STAMP(21, wave == 1);
    }
    __syncthreads();
    if (!diag) block_to_memory(B1, (extra ? M : S) + ri * n + rj1, n);
    PAIR_STAMP(23, wave == 0);
}

// the whole factorisation + L^-T rows: ceil(nb / 2) launches
// nb = panels of the (largest) system, count = problems (grid.y; every problem reads its own size from its view)
void enqueue_cholesky(hipStream_t s, const BaView* d_views, int count, int nb, int skip_small = 0, bool spread = false)
{
    // the attribute belongs to the (function, device) pair: once per device this process uses
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && !attr_set[dev].load()) {
        (void)hipFuncSetAttribute((const void*)k_chol_pair, hipFuncAttributeMaxDynamicSharedMemorySize, CP_LDS_BYTES);
        attr_set[dev].store(true);
    }
    for (int m = 0; 2 * m < nb; ++m) {
        const int j = 2 * m, ncol = (j + 1 < nb) ? 2 : 1;
        const int T = nb - j - ncol;
        const int n_panel = 1 + (nb - j - ncol) + (j + ncol);
        const int n_update = m > 0 ? T * (T + 1) / 2 + j * T : 0;
        // 32 CUs of one XCD hold a latency-bound launch of one problem; a throughput-bound one (or a batch) needs all 256
        // (spread: the front end keeps a few CUs of EVERY XCD free for this chain -- lpslam_hip_set_mapping_reserve -- so its workgroups go there)
        const int pin = (!spread && count == 1 && (n_panel + n_update) <= 96) ? 1 : 0;
        hipLaunchKernelGGL(k_chol_pair, dim3((n_panel + n_update) * (pin ? 8 : 1), count), dim3(256), CP_LDS_BYTES, s, d_views, m, pin, skip_small);
    }
}
// x_p = L^-T y with y = L[dim][0..dim): one wavefront per row of the (upper triangular) L^-T, butterfly sum
__global__ __launch_bounds__(256) void k_chol_xsolve(const BaView* __restrict__ views, int pin, int skip_small)
{
    if (pin && (blockIdx.x & 7)) return;  // XCD 0 only, like k_chol_pair: its inputs sit in that L2
    BA_VIEW(v);
    BA_VIEW_HEAD("s"(v.dim), "s"(v.dim_pad), "s"(v.ctl), "s"(v.S), "s"(v.Ldiag), "s"(v.Lsub), "s"(v.Minv), "s"(v.xp), "s"(v.scal), "s"(v.band_hbw));
    if (v.band_hbw >= 0 || ba_flags(v.ctl).idle() || (skip_small && cw_fits(v.dim))) return;
    // a flagged factorisation (a pivot <= 0 was replaced; the launches behind it may have grown that into infinities) gives the zero
    // step: the trial is rejected on the flag, and nothing that is not finite reaches the update
    const double flagged = v.scal[5];
    const int lane = threadIdx.x & 63;
    const int i = (pin ? blockIdx.x >> 3 : blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= v.dim) return;
    const int n = v.dim_pad;
    // y = L^-1 rhs is row `dim` of L: off-diagonal blocks live in S, the part inside the row's own diagonal block in Ldiag
    const int yb = v.dim / NB;
    const double* y = v.S + (size_t)v.dim * n;
    const double* yd = v.Ldiag + ((size_t)yb * NB + (v.dim - yb * NB)) * NB - (size_t)yb * NB;
    // an odd block is the second column of a panel pair: its block left of the diagonal went to Lsub (see k_chol_pair)
    const int ys0 = (yb & 1) ? (yb - 1) * NB : yb * NB;
    const double* ys = v.Lsub + ((size_t)yb * NB + (v.dim - yb * NB)) * NB - (size_t)ys0;
    const double* m = v.Minv + (size_t)i * n;
    double acc = 0;
    for (int c = (i / NB) * NB + lane; c < v.dim; c += 64) acc += m[c] * (c < ys0 ? y[c] : (c < yb * NB ? ys[c] : yd[c]));     // blocks left of the diagonal are empty
    acc = wave_sum(acc);
    if (lane == 0) v.xp[i] = flagged != 0.0 ? 0.0 : acc;
}

void enqueue_xsolve(hipStream_t s, const BaView* d_views, int count, int dim, int skip_small = 0, bool spread = false)
{
    const int pin = (!spread && count == 1) ? 1 : 0;
    hipLaunchKernelGGL(k_chol_xsolve, dim3((dim + 3) / 4 * (pin ? 8 : 1), count), dim3(256), 0, s, d_views, pin, skip_small);
}

#include "ba_solve.inl"
#include "ba_band.inl"

// factorisation + solve of `count` reduced systems.  `wg`: the systems that fit one compute unit go to k_chol_wg (one workgroup
// each, one launch), the others through the panel-pair chain and k_chol_xsolve (each kernel skips the problems of the other
// kind).  Measured (MI355X, 295 x 295, 10 LM iterations per problem, round 3): batches of 4 / 16 / 32 / 48 / 64 / 96 windows take
// 1.78 / 4.10 / 7.96 / 11.8 / 15.2 / 22.4 ms through the chain and 2.65 / 4.97 / 7.99 / 10.9 / 13.8 / 19.6 ms through k_chol_wg: the
// chain spreads one problem's trailing updates and L^-T rows over 20-60 workgroups, which only stops paying once the batch alone
// fills the chip.  (Factoring k_chol_wg's diagonal blocks with the DPP strips of the chain instead of the readlane form -- 2 x 2.8 k
// cycles against 2 x 10 k -- changed none of these numbers: that wavefront works beside the seven that update tiles.)
constexpr int CW_MIN_BATCH = 40;
// LPSLAM_HIP_CW_MIN_BATCH overrides the threshold (measurements)
int cw_min_batch()
{
    static const int v = [] { const char* e = getenv("LPSLAM_HIP_CW_MIN_BATCH"); return e ? atoi(e) : CW_MIN_BATCH; }();
    return v;
}
}  // namespace

void lp_enqueue_factor_solve(hipStream_t s, const void* views, int count, int nb_max, int dim_max, bool wg, bool any_small, bool any_large, bool spread)
{
    const BaView* d_views = (const BaView*)views;
    if (!wg) { any_large = any_large || any_small; any_small = false; }
    if (any_small) {
        static std::atomic<bool> attr_set[64];
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev >= 0 && dev < 64 && !attr_set[dev].load()) {
            (void)hipFuncSetAttribute((const void*)k_chol_wg, hipFuncAttributeMaxDynamicSharedMemorySize, CW_LDS_BYTES);
            attr_set[dev].store(true);
        }
        hipLaunchKernelGGL(k_chol_wg, dim3(1, count), dim3(CW_THREADS), CW_LDS_BYTES, s, d_views);
    }
    if (any_large) {
        enqueue_cholesky(s, d_views, count, nb_max, any_small ? 1 : 0, spread);
        enqueue_xsolve(s, d_views, count, dim_max, any_small ? 1 : 0, spread);
    }
}

namespace {

// ---- landmark back substitution and update (4 lanes per landmark); the last block applies x_p to the poses -------------------
__global__ __launch_bounds__(256) void k_ba_backsub(const BaView* __restrict__ views, int skip_one_pass)
{
    BA_VIEW(v);
    BA_VIEW_HEAD("s"(v.part_n), "s"(v.ctl));
    const int point_blocks = v.part_n;
    if ((int)blockIdx.x > point_blocks) return;
    if (skip_one_pass && upd_takes(v.n_points, v.n_free, v.n_poses)) return;      // that problem's update ran in k_ba_update
    const BaFlags fl = ba_flags(v.ctl);
    if (fl.idle()) return;
    const double lambda = fl.lambda;
    ba_select_idx(v, fl.cur); ba_lin_set(v, fl.cur);
    GPTR(double) poses_out = sel2(v.poses_buf[0], v.poses_buf[1], fl.cur ^ 1);
    GPTR(double) points_out = sel2(v.points_buf[0], v.points_buf[1], fl.cur ^ 1);
    if ((int)blockIdx.x == point_blocks) {
        // trial poses = exp(x_p) * poses; scal[3] = sum x_p (lambda x_p + b_p) (fixed order, one wavefront)
        if (threadIdx.x == 0) v.ctl->cur_launch = fl.cur;          // what the trial launch reads while the decision flips `cur`
        if (threadIdx.x >= 64) return;
        double sc = 0;
        for (int p = threadIdx.x; p < v.n_poses; p += 64) {
            const int slot = v.pose_slot[p];
            if (slot < 0) { for (int i = 0; i < 7; ++i) poses_out[7 * p + i] = v.poses[7 * p + i]; continue; }
            pose_oplus(v.poses + 7 * p, v.xp + 6 * slot, poses_out + 7 * p);
            for (int a = 0; a < 6; ++a) { const double x = v.xp[6 * slot + a]; sc += x * (lambda * x + v.bp[6 * slot + a]); }
        }
        sc = wave_sum(sc);
        if (threadIdx.x == 0) v.scal[3] = sc;
        return;
    }
    const int g = blockIdx.x * 64 + (threadIdx.x >> 2), sub = threadIdx.x & 3;
    double sc = 0;
    double r[3] = {0, 0, 0};
    if (g < v.n_points) {
        // two observations of the lane at a time, their index / slot / W / x_p load chains side by side (same order of the sums)
        const int s_end = v.pt_start[g + 1];
        for (int s = v.pt_start[g] + sub; s < s_end; s += 8) {
            int kk[2], slot[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) kk[u] = v.pt_obs[min(s + 4 * u, s_end - 1)];
#pragma unroll
            for (int u = 0; u < 2; ++u) slot[u] = v.pose_slot[v.o_pose[kk[u]]];
            double wv[2][18], xv[2][6];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const double* Wk = v.W + 18 * (size_t)kk[u];
                const double* x = v.xp + 6 * (size_t)max(slot[u], 0);
#pragma unroll
                for (int i = 0; i < 18; ++i) wv[u][i] = Wk[i];
#pragma unroll
                for (int i = 0; i < 6; ++i) xv[u][i] = x[i];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (s + 4 * u < s_end && slot[u] >= 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int rr = 0; rr < 6; ++rr) r[c] += wv[u][rr * 3 + c] * xv[u][rr];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a1 = __shfl_xor(r[c], 1);
        const double lo = (sub & 1) ? a1 + r[c] : r[c] + a1;      // (s0 + s1) and (s2 + s3), same order in both lanes
        const double a2 = __shfl_xor(lo, 2);
        r[c] = (sub & 2) ? a2 + lo : lo + a2;                     // (s0 + s1) + (s2 + s3)
    }
    if (g < v.n_points && sub == 0) {
        const double b0 = v.bl[3 * (size_t)g], b1 = v.bl[3 * (size_t)g + 1], b2 = v.bl[3 * (size_t)g + 2];
        const double q0 = b0 - r[0], q1 = b1 - r[1], q2 = b2 - r[2];
        double h[6];
        point_hinv(v.Hll + 6 * (size_t)g, lambda, h);
        const double x0 = h[0] * q0 + h[1] * q1 + h[2] * q2;
        const double x1 = h[1] * q0 + h[3] * q1 + h[4] * q2;
        const double x2 = h[2] * q0 + h[4] * q1 + h[5] * q2;
        points_out[3 * (size_t)g] = v.points[3 * (size_t)g] + x0;
        points_out[3 * (size_t)g + 1] = v.points[3 * (size_t)g + 1] + x1;
        points_out[3 * (size_t)g + 2] = v.points[3 * (size_t)g + 2] + x2;
        sc = x0 * (lambda * x0 + b0) + x1 * (lambda * x1 + b1) + x2 * (lambda * x2 + b2);
    }
    __shared__ double sm[4];
    sc = wave_sum(sc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = sc;
    __syncthreads();
    if (threadIdx.x == 0) v.part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// per-observation chi2 (non robust) and depth sign of the accepted state
__global__ __launch_bounds__(256) void k_ba_obs_chi2(const BaView* __restrict__ views, double* chi2, uint8_t* depth_pos)
{
    BA_VIEW(v);
    ba_select(v, 0);
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= v.n_obs) return;
    const int p = v.o_pose[k], j = v.o_point[k];
    double R[9], e[3], pc[3];
    quat_to_rot(v.poses + 7 * p, R);
    const double X[3] = {v.points[3 * j], v.points[3 * j + 1], v.points[3 * j + 2]};
    const int D = ba_residual(v, k, R, v.poses + 7 * p + 4, X, e, pc);
    const int ko = v.o_orig[k];                 // the caller's observation index
    chi2[ko] = v.o_w[k] * (e[0] * e[0] + e[1] * e[1] + (D == 3 ? e[2] * e[2] : 0.0));
    depth_pos[ko] = pc[2] > 0 ? 1 : 0;
}

#include "ba_update.inl"
#include "ba_build.inl"

}  // namespace

#include "ba_host.inl"
#include "ba_partitioned.inl"

#ifdef LPSLAM_SCHUR_STAMPS
extern "C" __attribute__((visibility("default"))) int lpslam_hip_debug_schur_stamps(unsigned long long* out, int n) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_schur_stamps), (size_t)n * sizeof(unsigned long long)); }
#endif
#ifdef LPSLAM_PAIR_STAMPS
extern "C" __attribute__((visibility("default"))) int lpslam_hip_debug_pair_stamps(unsigned long long* out, int n) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pair_stamps), (size_t)n * sizeof(unsigned long long)); }
#endif
#ifdef LPSLAM_UPD_STAMPS
extern "C" __attribute__((visibility("default"))) int lpslam_hip_debug_upd_stamps(double* out32) { return (int)hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_upd_stamps), 32 * sizeof(double)); }
#endif
