// ba_common.h -- what the bundle adjuster (ba.hip), the motion-only pose optimiser (pose_opt.hip) and the Sim3 pose graph and transform
// optimiser (sim3.hip) have in common: the device-driven Levenberg control block and its two steps, the view of a problem the Cholesky
// kernels take, the last-workgroup hand-over, the wavefront reductions and the fast reciprocals.  Everything here is used by more than
// one of the three units; what only the bundle adjuster needs (Schur constants, the linearisation sets' layout) stays in ba.hip.
// Definitions sit in an anonymous namespace: every unit compiles its own copy, only lp_enqueue_factor_solve crosses units.
#pragma once
#include "internal.h"
#include <cfloat>
#include <cmath>

// Parity with the CPU definition forbids FMA contraction ("Numerics"); the functions that want fused multiply-adds say
// contract(fast) themselves.
#pragma clang fp contract(off)

namespace {

constexpr int NB = 32;                // Cholesky panel width
constexpr int MAX_LOG = 64;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct BaCam { double fx, fy, cx, cy, fxb, hub_mono, hub_stereo; };

struct BaCtl {                        // device-resident LM state (g2o OptimizationAlgorithmLevenberg)
    double lambda, ni, current_chi, chi_before, rho;
    int cur;                          // buffer index of the accepted state
    int need_lin;                     // the next unit must linearise first
    int first;                        // lambda_0 not yet computed in this optimize() call
    int qmax;                         // trials of the running outer iteration
    int outer_done, max_outer;
    int stopped;                      // g2o "Terminate"
    int last_accepted;
    int ticket;                       // workgroups of the running pass that have published their partials (last one combines)
    int cur_launch;                   // copy of `cur` that stays put while a trial launch runs (the decision flips `cur` inside it)
    int spec;                         // linearisation set [cur] already holds the linearisation of state cur (speculated beside the trial)
    int faults_band, faults_update;   // host copy only (k_ba_collect fills them from ba_sync_words): hand-overs that timed out, cumulative
};

// Pointer members of the view are typed as global-address-space pointers in the device pass: a view is read from device memory
// (views[blockIdx.y], scalar loads), and a pointer that comes out of memory is a generic ("flat") pointer to the compiler --
// flat loads count on both vmcnt and lgkmcnt and return out of order, so every wait on them is a full drain.  With the address
// space in the type every access through the view is a global_load / global_store with counted waits, as with by-value kernel
// arguments.  The host pass sees plain pointers of the same size and layout.
#if defined(__HIP_DEVICE_COMPILE__)
#define GPTR(T) __attribute__((address_space(1))) T*
#else
#define GPTR(T) T*
#endif
template <class D, class S> inline void vset(D& d, S* s) { d = (D)s; }       // host side: generic pointer into a view member

struct BaView {                       // one problem, resident in device memory (kernels index an array of them by blockIdx.y)
    int n_poses, n_points, n_obs, n_free, dim, dim_pad;
    // launch extents of this problem (a batch launches the maximum over its problems; surplus workgroups exit at once)
    int obs_blocks;                   // ceil(n_obs / 256): observation-side linearisation
    int pose_blocks;                  // ceil(n_poses * SPLIT / 4): pose-side linearisation / trial chi2
    int point_blocks;                 // ceil(n_points / 256): k_ba_point_sum
    int part_n;                       // max(ceil(n_points / 64), 1): k_ba_backsub landmark blocks = entries of `part`
    int n_blocks;                     // pose-block pairs (n_free (n_free + 1) / 2)
    int land_blocks;                  // ceil(n_points / LAND_B): landmark-major linearisation beside a trial (land_lin_body)
    GPTR(double) poses_buf[2]; GPTR(double) points_buf[2];
    GPTR(const double) poses; GPTR(const double) points;        // set by the kernel prologue (state being evaluated)
    GPTR(const double) poses0; GPTR(const double) points0;      // state given at creation (reset)
    GPTR(const int) pose_slot; GPTR(const int) free_pose;
    GPTR(const int) o_pose; GPTR(const int) o_point;
    GPTR(const double) o_u; GPTR(const double) o_v; GPTR(const double) o_ur; GPTR(const double) o_w;
    GPTR(uint8_t) o_active;
    GPTR(const int) pt_start; GPTR(const int) pt_obs; GPTR(const int) ps_start; GPTR(const int) o_orig;
    GPTR(double) W; GPTR(double) Hll; GPTR(double) bl; GPTR(double) Hpp; GPTR(double) hl_obs; GPTR(double) partial;   // linearisation set in use (ba_lin_set)
    // Both linearisation sets (indexed like the state buffers), each as TWO blocks whose sub-arrays sit at offsets that follow from
    // the problem's sizes (SetOff): set_z = [partial | b_p, diag H_pp, chi2] (zero-initialised), set_d = [H_ll | b_l | H_pp | W | hl].
    // One pointer pair per set instead of seven keeps the by-value view small enough to live in scalar registers (at 672 bytes the
    // compiler kept a copy in scratch memory and every member access became a scratch load: trial launch 14 -> 41 us).
    GPTR(double) set_z[2]; GPTR(double) set_d[2]; GPTR(double) partial_trial;     // + trial chi2 partials
    GPTR(const double) csr;            // observation constants once more in CSR (landmark-major) order [u | v | ur | w | pose, point (int) | pose slot (int)]
    GPTR(const int) land_start;        // landmark blocks of the landmark-major passes: (first landmark, first CSR entry) per block + a closing pair; <= LAND_B landmarks and -- unless one landmark alone has more -- <= 256 entries each, cut on the host at creation
    GPTR(double) S; GPTR(double) rhs; GPTR(double) bp; GPTR(double) hppdiag; GPTR(double) chi_cur;   // reduced buffer sections (all-reduced when partitioned)
    GPTR(double) bp_loc; GPTR(double) hppdiag_loc; GPTR(double) chi_loc;                    // this rank's own sums (equal to the above on one GPU)
    GPTR(double) Minv;                                                            // L^-T row blocks (dim_pad x dim_pad)
    GPTR(double) Ldiag;                                                           // [nb][32][32]; only row dim - 32 (nb - 1) of block nb - 1 is written: the rhs row inside L's last diagonal block
    GPTR(double) Lsub;                                                            // [nb][32][32]; block nb - 1 alone, for an even nb: L_j1,j of the last pair
    GPTR(double) xp; GPTR(double) chi_pose; GPTR(double) part; GPTR(double) scal;
    GPTR(const int) blk_start; GPTR(const int4) blk_terms;        // Schur pair lists: (observation a, observation b, their landmark, -)
    GPTR(double) blk_part; GPTR(int) blk_ticket;                  // Schur partial sums [block][SCH_MAXP][SCH_PV], per-block tickets (+ the table of further parts, ba_build.inl)
    GPTR(int) blk_perm;                                           // k_ba_schur: which pose-block pair work item w takes (XCD tiles, see lpslam_hip_ba_prepare)
    GPTR(BaCtl) ctl; GPTR(lpslam_hip_ba_iter_log) log;
    BaCam cam;
    // block-banded windows (ba_band.inl): block half-bandwidth of the reduced system when the problem takes the band path (-1: pair
    // lists + dense chain), landmark groups, [group records | first / last candidate group per free slot], entry table, group partials
    int band_hbw, band_groups, band_groups_cap;
    int extra_pack;                   // k_ba_schur: workgroups for the further parts of long pair lists (table behind blk_ticket[n_blocks]: head word = items + the window's part size, then the items):
                                      // (cap << 12) | first -- the table holds at most `cap` items, `first` of them get workgroups in FRONT of the pairs'
                                      // part 0 (what the host expects: the diagonal blocks' parts), the rest behind them (one int: the view's size matters)
    GPTR(const int) band_tab; GPTR(const int) band_ent; GPTR(double) band_part;
};

// Words beside the eight scalars of v.scal that are NOT part of the control block (lm_begin / lm_decide rewrite that as a whole):
// [0] hand-overs of the twisted band factorisation that timed out, [1] keyframe blocks of k_ba_update that timed out (both stay 0;
// lpslam_hip_ba_timeouts; [1] also counts k_ba_schur blocks whose wait for the pose side timed out), [2] unused (it keeps its slot: the layout is the host's too), [3] "pose side
// pending": the accepted state's H_pp, b_p are the next Schur launch's to compute (set by k_ba_update's decision, ba_update.inl),
// [4] wavefronts of that launch that have stored theirs.
__device__ __forceinline__ int* ba_sync_words(const BaView& v) { return (int*)(double*)(v.scal + 8); }

// The view of problem blockIdx.y.  `views` is const __restrict__ and read before any store of the kernel: scalar loads.
#define BA_VIEW(v) BaView v = views[blockIdx.y]

__device__ __forceinline__ bool ba_idle(const BaCtl* c) { return c->stopped || c->outer_done >= c->max_outer; }

// Reciprocal and reciprocal square root for the per-observation arithmetic: v_rcp_f64 / v_rsq_f64 (2^-24, measured) plus ONE cubic
// correction step -- five instructions and 1.4e-16 maximum relative error (4M samples, tools/dev/rsq_acc.hip) where IEEE division
// and sqrt are ~30 instructions each.  A reprojection Jacobian held thirteen divisions: across a window's 39 k observations and
// their three passes per LM iteration that was most of the arithmetic of the linearising kernels.  Not correctly rounded: results
// move in the last bits against a libm evaluation (tests: chi2 trajectories 1e-9 relative, poses 1e-4 rad / 1e-3 m).
__device__ __forceinline__ double fast_rcp(double d)       // 1 / d
{
    const double y0 = __builtin_amdgcn_rcp(d);
    const double e = fma(-d, y0, 1.0);
    return fma(y0, fma(e, e, e), y0);                   // y0 (1 + e + e^2)
}
__device__ __forceinline__ double fast_rsqrt(double d)     // 1 / sqrt(d), d > 0
{
    const double y0 = __builtin_amdgcn_rsq(d);
    const double e = fma(-(d * y0), y0, 1.0);
    return fma(y0 * e, fma(0.375, e, 0.5), y0);         // y0 (1 + e / 2 + 3 e^2 / 8)
}

__device__ __forceinline__ void huber(double e2, double delta, double* rho0, double* rho1)
{
    const double dsqr = delta * delta;
    if (e2 <= dsqr) { *rho0 = e2; *rho1 = 1.0; }
    else { const double rs = fast_rsqrt(e2); *rho0 = 2 * (e2 * rs) * delta - dsqr; *rho1 = delta * rs; }
}

// "Last workgroup done" hand-over: every workgroup of a pass calls this after its partials are stored.  Returns true in
// exactly one workgroup -- the one that arrives last -- with all other workgroups' stores visible (producer: every wavefront
// drains its stores, barrier, one lane's agent-scope release + ticket; consumer: agent-scope acquire by that lane, its wait,
// barrier, plain loads -- MI355X_MICROARCH.md, inter-workgroup visibility); that workgroup then runs the single-workgroup
// combine, which saves a launch.  No spinning, so the grid always drains.
// The general form (any plain stores before it are visible to the last workgroup's plain loads after it): agent-scope
// acquire-release on the ticket, i.e. an L2 write-back and an L1 invalidate per workgroup.  Used where the handed-over data
// are not confined to a few words (sim3.hip).
__device__ __forceinline__ bool ba_last_block(BaCtl* c, int total)
{
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wavefront drains its own stores (a barrier alone does not)
    __syncthreads();
    if (threadIdx.x == 0) {
        // release: the workgroup's stores leave this XCD's L2; acquire (only the last arrival needs it): stale lines are dropped
        const int t = __hip_atomic_fetch_add(&c->ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == total - 1);
        if (s_last) c->ticket = 0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // holds the barrier below until the invalidate has completed
    }
    __syncthreads();
    return s_last != 0;
}

__device__ __forceinline__ double wave_sum(double x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ double wave_max(double x)
{
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
    return x;
}

// ---- g2o's lambda control (one thread) ----------------------------------------------------------------------------------
// start of an outer iteration / after a linearisation: lambda_0 = tau * max diag(H) on the first one, chi2 bookkeeping
__device__ __forceinline__ void lm_begin(BaView& v, double max_diag_pp, double max_diag_ll, double chi_cur)
{
    BaCtl c = *v.ctl;                                      // one batch of loads, one batch of stores
    if (c.first) {
        const double maxd = fmax(v.n_points ? max_diag_ll : 0.0, max_diag_pp);
        c.lambda = 1e-5 * maxd;
        c.ni = 2;
        c.first = 0;
    }
    c.current_chi = chi_cur;
    if (c.qmax == 0) c.chi_before = chi_cur;
    c.need_lin = 0;
    c.spec = 0;
    *v.ctl = c;
}
// after a trial: rho, accept / reject, lambda update, iteration and termination bookkeeping
__device__ __forceinline__ int lm_decide(BaView& v, double temp_chi, double chol_failed, double scale_l, double scale_p, bool spec_ran = false, const BaCtl* preloaded = nullptr)      // returns "accepted"
{
    BaCtl c = preloaded ? *preloaded : *v.ctl;             // (preloaded: the caller fetched the block beside its other loads -- one round trip less on the chain)
    // factorisation failed: g2o's ok = 0 branch -- no step was taken, computeScale is not run (the scale is its 1e-3 alone), so rho < 0
    // and the iteration goes on to its next trial with a larger lambda.  The scale terms of a flagged solve must not get a say: they
    // come from whatever the factorisation left (tests/test_ba_solve_gpu.py).
    if (chol_failed != 0.0) { temp_chi = DBL_MAX; scale_l = 0.0; scale_p = 0.0; }
    double rho = c.current_chi - temp_chi;
    const double scale = (scale_l + scale_p) + 1e-3;
    rho /= scale;
    const bool accepted = rho > 0 && isfinite(temp_chi);
    if (accepted) {
        const double t = 2 * rho - 1;
        double alpha = 1. - t * t * t;
        alpha = fmin(alpha, 2. / 3.);
        const double sf = fmax(1. / 3., alpha);
        c.lambda *= sf;
        c.ni = 2;
        c.current_chi = temp_chi;
        c.cur ^= 1;                                        // discardTop: the trial state becomes the accepted one
        c.spec = spec_ran ? 1 : 0;                         // ... and its linearisation is already in its set
    } else {
        c.lambda *= c.ni;
        c.ni *= 2;                                         // pop: the accepted state stays
    }
    c.rho = rho;
    c.last_accepted = accepted ? 1 : 0;
    c.qmax++;
    const bool finished = !(rho < 0 && c.qmax < 10);
    if (finished) {
        const int terminate = (c.qmax == 10 || rho == 0) ? 1 : 0;
        if (c.outer_done < MAX_LOG) {
            lpslam_hip_ba_iter_log* l = v.log + c.outer_done;
            l->chi2_before = c.chi_before; l->chi2_after = c.current_chi; l->lambda = c.lambda; l->trials = c.qmax; l->status = terminate;
        }
        c.outer_done++;
        c.qmax = 0;
        if (accepted && spec_ran) {
            // the trial launch linearised the accepted state completely (W, landmark and pose sums, combined by its last workgroup):
            // the next outer iteration starts at the Schur complement.  What lm_begin would do: chi2 bookkeeping of a fresh iteration
            c.need_lin = 0; c.spec = 0; c.chi_before = c.current_chi;
        } else c.need_lin = 1;
        if (terminate) c.stopped = 1;
    } else {
        c.need_lin = 0;
    }
    *v.ctl = c;
    return c.last_accepted;
}

// ---- the pose update of the pose optimiser (pose_opt.hip), which the bundle adjuster's one-launch update applies too (k_ba_update,
//      ba_update.inl) --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double po_rsqrt(double d) { return fast_rsqrt(d); }
// sin and cos of a half angle up to 0.5 rad (every Levenberg step of a tracked frame) from their Taylor polynomials -- two
// interleaved Horner chains of eight terms, truncation below 1e-18 -- instead of the library's ~130 instructions of argument
// reduction; larger angles take the library call
__device__ __forceinline__ void po_sincos_half(double h, double* sn, double* cs)
{
    if (h <= 0.5) {
        const double z = h * h;
        double ps = 1.0 / 355687428096000.0, pc = 1.0 / 20922789888000.0;     // 1 / 17!, 1 / 16!
        ps = fma(ps, -z, 1.0 / 1307674368000.0);  pc = fma(pc, -z, 1.0 / 87178291200.0);       // 1 / 15!, 1 / 14!
        ps = fma(ps, -z, 1.0 / 6227020800.0);     pc = fma(pc, -z, 1.0 / 479001600.0);         // 1 / 13!, 1 / 12!
        ps = fma(ps, -z, 1.0 / 39916800.0);       pc = fma(pc, -z, 1.0 / 3628800.0);           // 1 / 11!, 1 / 10!
        ps = fma(ps, -z, 1.0 / 362880.0);         pc = fma(pc, -z, 1.0 / 40320.0);             // 1 / 9!, 1 / 8!
        ps = fma(ps, -z, 1.0 / 5040.0);           pc = fma(pc, -z, 1.0 / 720.0);               // 1 / 7!, 1 / 6!
        ps = fma(ps, -z, 1.0 / 120.0);            pc = fma(pc, -z, 1.0 / 24.0);                // 1 / 5!, 1 / 4!
        ps = fma(ps, -z, 1.0 / 6.0);              pc = fma(pc, -z, 0.5);                       // 1 / 3!, 1 / 2!
        *sn = fma(h * z, -ps, h);                                                              // h - h^3 (1/3! - ...)
        *cs = fma(z, -pc, 1.0);                                                                // 1 - h^2 (1/2! - ...)
    } else {
        sincos(h, sn, cs);
    }
}
// pose_oplus: exp(d) * pose with one sincos of the half angle and the fast reciprocals.  The increment's rotation and its V matrix
// are applied as Rodrigues sums (v + a w x v + b w x (w x v)), not as 3x3 matrices: 40 instructions where forming W^2, R and V took
// 80 (this runs between two passes, on every thread's own registers).
__device__ __forceinline__ void po_oplus(const double* pose, const double* d, double* out)
{
#pragma clang fp contract(fast)
    const double wx = d[0], wy = d[1], wz = d[2];
    const double theta2 = wx * wx + wy * wy + wz * wz;
    double a, b, c, qe[4];
    if (theta2 < 1e-10) {
        a = 1.0; b = 0.5; c = 1.0 / 6.0;
        qe[0] = 1.0; qe[1] = 0.5 * wx; qe[2] = 0.5 * wy; qe[3] = 0.5 * wz;
    } else {
        const double rt = po_rsqrt(theta2), theta = theta2 * rt, rt2 = rt * rt;
        double sh2, ch2;
        po_sincos_half(0.5 * theta, &sh2, &ch2);
        const double st = 2.0 * sh2 * ch2, omc = 2.0 * sh2 * sh2;        // sin(theta), 1 - cos(theta)
        a = st * rt;
        b = omc * rt2;
        c = (theta - st) * (rt2 * rt);
        const double shq = sh2 * rt;
        qe[0] = ch2; qe[1] = shq * wx; qe[2] = shq * wy; qe[3] = shq * wz;
    }
    const double* t = pose + 4;
    // w x t, w x (w x t), w x u, w x (w x u) with u the translation part of the increment
    const double c1[3] = {wy * t[2] - wz * t[1], wz * t[0] - wx * t[2], wx * t[1] - wy * t[0]};
    const double c2[3] = {wy * c1[2] - wz * c1[1], wz * c1[0] - wx * c1[2], wx * c1[1] - wy * c1[0]};
    const double u1[3] = {wy * d[5] - wz * d[4], wz * d[3] - wx * d[5], wx * d[4] - wy * d[3]};
    const double u2[3] = {wy * u1[2] - wz * u1[1], wz * u1[0] - wx * u1[2], wx * u1[1] - wy * u1[0]};
    double tn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) tn[i] = fma(c, u2[i], fma(b, u1[i], d[3 + i])) + fma(b, c2[i], fma(a, c1[i], t[i]));
    const double* q = pose;
    double qn[4];
    qn[0] = qe[0] * q[0] - qe[1] * q[1] - qe[2] * q[2] - qe[3] * q[3];
    qn[1] = qe[0] * q[1] + qe[1] * q[0] + qe[2] * q[3] - qe[3] * q[2];
    qn[2] = qe[0] * q[2] - qe[1] * q[3] + qe[2] * q[0] + qe[3] * q[1];
    qn[3] = qe[0] * q[3] + qe[1] * q[2] - qe[2] * q[1] + qe[3] * q[0];
    const double rn = po_rsqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = qn[i] * rn;
#pragma unroll
    for (int i = 0; i < 3; ++i) out[4 + i] = tn[i];
}

// the system fits the single-workgroup factorisation (k_chol_wg, ba_solve.inl): 16-row tile rows held, dim + 1 <= 304
constexpr int CW_MAXT = 19;
__host__ __device__ inline bool cw_fits(int dim) { return dim > 0 && dim + 1 <= 16 * CW_MAXT; }

}  // namespace

// Factorisation + solve of `count` systems whose views (BaView) sit in the device array d_views, enqueued on s (ba.hip, where the
// Cholesky kernels live; the parameters are described there).  The views cross as void*: BaView belongs to each unit's own
// anonymous namespace, and a function that names it in its signature would be local to its unit too.
void lp_enqueue_factor_solve(hipStream_t s, const void* d_views, int count, int nb_max, int dim_max, bool wg, bool any_small, bool any_large, bool spread = false);
