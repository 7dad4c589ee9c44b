// pnp.hip -- the relocaliser's pose solver for a batch of match sets ([UPSTREAM] solve::pnp_solver, the host
// form is LpSlam::pnp_solve_ransac in lpslam_amd/host/two_view.cpp).  One call takes S sets of landmark / keypoint matches:
//   host            the sample table (the 4-match samples pnp_solve_ransac would draw, ransac_sample.h) and ONE upload of it with the matches
//   k_pnp_hypotheses  sixteen lanes per (set, iteration): EPnP on the four sampled matches (epnp<4> of epnp_math.h, the function the host
//                   solver calls); the 12 x 12 matrix and its eigenvectors live in LDS (2.3 KB a hypothesis, four a wave) and
//                   the lanes divide each Jacobi rotation's elements among them
//   k_pnp_score     one workgroup per set, a wave per hypothesis in turn: inliers counted with the host's expression, the winner by the
//                   key count << 32 | ~iteration (the lowest iteration among equal counts, the host's `count > best`), its flags and
//                   pose written to page-locked memory, then the done flag (internal.h)
//   host            one wait; per set the refit of pnp_solve_ransac (pnp_refit of epnp_math.h): EPnP over the winner's inliers
// The round trip -- page-locked block, device block, done flag, what becomes of them when a stream is late or dead -- is LpStagedCall
// (internal.h).
#include "internal.h"
#include "epnp_math.h"
#include "ransac_sample.h"
#include "../host/pose_math.h"
#include <cmath>

using namespace lpslam;
namespace ep = lpslam_epnp;

namespace {

constexpr int kHypLanes = 16;          // lanes that solve one hypothesis together (12 of them carry a row / column of the 12 x 12 matrix)
constexpr int kHypPerWg = 64 / kHypLanes;      // one wave per workgroup
constexpr int kHypLds = ep::kWorkspace + 2;    // doubles of LDS per hypothesis: the four workspaces of a wave start on different banks

struct PnpHead { double cam[4]; int32_t n_sets, iterations; uint32_t o_offsets, o_table, o_pw, o_obs, o_w, pad; };
struct PnpResult { int32_t best_iteration, count; double R[9], t[3]; };
static_assert(sizeof(PnpResult) == 104, "result record");

__global__ __launch_bounds__(64) void k_pnp_hypotheses(const uint8_t* __restrict__ base, double* __restrict__ hyp, int* __restrict__ valid)
{
    __shared__ double ws[kHypLds * kHypPerWg];
    const PnpHead& head = *(const PnpHead*)base;
    const int group = threadIdx.x / kHypLanes, ln = threadIdx.x % kHypLanes;
    const int h = blockIdx.x * kHypPerWg + group;
    if (h >= head.n_sets * head.iterations) return;           // (the sixteen lanes of a hypothesis together; no workgroup barrier in this kernel)
    const int s = h / head.iterations;
    const int32_t* off = (const int32_t*)(base + head.o_offsets);
    const int o = off[s], n = off[s + 1] - o;
    if (n < 4) { if (ln == 0) valid[h] = 0; return; }
    const int32_t* idx = (const int32_t*)(base + head.o_table) + 4 * (size_t)h;
    const double* pw = (const double*)(base + head.o_pw);
    const double* obs = (const double*)(base + head.o_obs);
    double p4[12], u4[8], cam[4], R[9], t[3];
    for (int k = 0; k < 4; ++k) {
        const size_t m = (size_t)o + (size_t)min(max(idx[k], 0), n - 1);
        for (int a = 0; a < 3; ++a) p4[3 * k + a] = pw[3 * m + a];
        u4[2 * k] = obs[2 * m]; u4[2 * k + 1] = obs[2 * m + 1];
    }
    for (int k = 0; k < 4; ++k) cam[k] = head.cam[k];
    const bool ok = ep::epnp<4>(p4, u4, 4, cam, nullptr, nullptr, ws + kHypLds * group, 1, R, t, ln, kHypLanes);
    if (ln != 0) return;
    valid[h] = ok ? 1 : 0;
    if (ok) { for (int k = 0; k < 9; ++k) hyp[12 * (size_t)h + k] = R[k]; for (int k = 0; k < 3; ++k) hyp[12 * (size_t)h + 9 + k] = t[k]; }
}

__global__ __launch_bounds__(256) void k_pnp_score(const uint8_t* __restrict__ base, const double* __restrict__ hyp, const int* __restrict__ valid,
                                                   PnpResult* __restrict__ res, uint8_t* __restrict__ flags, unsigned* counter, int* flag, int seq)
{
    __shared__ unsigned long long wkey[4];
    const PnpHead& head = *(const PnpHead*)base;
    const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* off = (const int32_t*)(base + head.o_offsets);
    const int o = off[s], n = off[s + 1] - o;
    const double* pw = (const double*)(base + head.o_pw) + 3 * (size_t)o;
    const double* obs = (const double*)(base + head.o_obs) + 2 * (size_t)o;
    const double* w = (const double*)(base + head.o_w) + (size_t)o;
    double cam[4];
    for (int k = 0; k < 4; ++k) cam[k] = head.cam[k];
    unsigned long long best = 0;
    if (n >= 4)
        for (int it = wave; it < head.iterations; it += 4) {              // the same for every lane of a wave
            const size_t h = (size_t)s * (size_t)head.iterations + (size_t)it;
            if (!valid[h]) continue;
            double Rt[12];
            for (int k = 0; k < 12; ++k) Rt[k] = hyp[12 * h + k];
            int count = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                const bool in = i < n && ep::pnp_inlier(Rt, Rt + 9, cam, pw + 3 * (size_t)i, obs[2 * (size_t)i], obs[2 * (size_t)i + 1], w[i]);
                count += __popcll(__ballot(in));
            }
            const unsigned long long key = (unsigned long long)count << 32 | (unsigned long long)(~(uint32_t)it);
            if (count > 0 && key > best) best = key;
        }
    if (lane == 0) wkey[wave] = best;
    __syncthreads();
    best = wkey[0];
    for (int k = 1; k < 4; ++k) if (wkey[k] > best) best = wkey[k];
    const int count = (int)(best >> 32);
    const int it = (int)(~(uint32_t)(best & 0xffffffffu));
    uint8_t* fl = flags + o;
    if (count < 4) {                                                      // the host's `best < 4`: no pose, the flags cleared
        for (int i = threadIdx.x; i < n; i += 256) fl[i] = 0;
        if (threadIdx.x == 0) {
            PnpResult r{};
            r.best_iteration = -1; r.count = 0; r.R[0] = r.R[4] = r.R[8] = 1.0;
            res[s] = r;
        }
    } else {
        const size_t h = (size_t)s * (size_t)head.iterations + (size_t)it;
        double Rt[12];
        for (int k = 0; k < 12; ++k) Rt[k] = hyp[12 * h + k];
        for (int i = threadIdx.x; i < n; i += 256)
            fl[i] = ep::pnp_inlier(Rt, Rt + 9, cam, pw + 3 * (size_t)i, obs[2 * (size_t)i], obs[2 * (size_t)i + 1], w[i]) ? 1 : 0;
        if (threadIdx.x == 0) {
            PnpResult r{};
            r.best_iteration = it; r.count = count;
            for (int k = 0; k < 9; ++k) r.R[k] = Rt[k];
            for (int k = 0; k < 3; ++k) r.t[k] = Rt[9 + k];
            res[s] = r;
        }
    }
    lp_signal_done(counter, flag, seq);
}

}  // namespace

extern "C" {

int lpslam_hip_pnp_ransac_batch(lpslam_hip_ctx* c, int32_t n_sets, const int32_t* offsets, const double* pw, const double* obs, const double* inv_sigma2,
                                const double* cam4, int32_t iterations, uint32_t seed, double* pose7, int32_t* n_inliers, uint8_t* inlier, int32_t* best_iteration)
{
    if (!c) { set_error("null context"); return LPSLAM_HIP_ERR_INVALID; }
    int first = 0, total = 0;
    if (const char* why = lpslam_ransac::check_offsets(n_sets, offsets, &first, &total)) { set_error("pnp_ransac_batch: %s", why); return LPSLAM_HIP_ERR_INVALID; }
    if (iterations < 1 || iterations > LPSLAM_HIP_PNP_MAX_ITERATIONS) { set_error("pnp_ransac_batch: %d iterations outside 1 .. %d", iterations, LPSLAM_HIP_PNP_MAX_ITERATIONS); return LPSLAM_HIP_ERR_INVALID; }
    if (!cam4 || (n_sets > 0 && (!pose7 || !n_inliers))) { set_error("pnp_ransac_batch: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (total > 0 && (!pw || !obs || !inv_sigma2 || !inlier)) { set_error("pnp_ransac_batch: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    for (int k = 0; k < 4; ++k) if (!std::isfinite(cam4[k])) { set_error("pnp_ransac_batch: the camera is no number"); return LPSLAM_HIP_ERR_INVALID; }
    if (n_sets == 0) return LPSLAM_HIP_OK;
    const size_t n_hyp = (size_t)n_sets * (size_t)iterations;
    if (n_hyp > (size_t)0x7fffffff / 4) { set_error("pnp_ransac_batch: %d sets x %d iterations do not fit one launch", n_sets, iterations); return LPSLAM_HIP_ERR_CAPACITY; }
    LP_HIP(hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    const LpMatchTrace tr;
    // page-locked block: flag | input (head, offsets rebased to 0, sample table, landmarks, keypoints, weights) | results (a record per
    // set, a flag per match); device block: the input, then the hypotheses (R, t) and their valid flags
    const size_t o_in = 64, tot1 = (size_t)std::max(total, 1);
    LpLayout dev;
    dev.take(sizeof(PnpHead));
    const size_t o_offsets = dev.take((size_t)(n_sets + 1) * 4), o_table = dev.take(n_hyp * 16);
    const size_t o_pw = dev.take(tot1 * 24), o_obs = dev.take(tot1 * 16), o_w = dev.take(tot1 * 8);
    const size_t in_bytes = dev.at;
    const size_t d_hyp = dev.take(n_hyp * 96), d_valid = dev.take(n_hyp * 4);
    LpLayout host{o_in + in_bytes};
    const size_t h_res = host.take((size_t)n_sets * sizeof(PnpResult)), h_flags = host.take(tot1);
    LpStagedCall call{c, s, "pnp_ransac_batch"};
    if (int rc = call.open(host.at, dev.at, LP_DONE_PNP)) return rc;
    uint8_t *hb = call.host, *base = call.dev(), *in = hb + o_in;
    PnpHead head{};
    for (int k = 0; k < 4; ++k) head.cam[k] = cam4[k];
    head.n_sets = n_sets; head.iterations = iterations;
    head.o_offsets = (uint32_t)o_offsets; head.o_table = (uint32_t)o_table; head.o_pw = (uint32_t)o_pw; head.o_obs = (uint32_t)o_obs; head.o_w = (uint32_t)o_w;
    memcpy(in, &head, sizeof head);
    int32_t* off0 = (int32_t*)(in + o_offsets);
    for (int i = 0; i <= n_sets; ++i) off0[i] = offsets[i] - first;
    lpslam_ransac::batch_tables<4>(n_sets, off0, iterations, seed, (int32_t*)(in + o_table));
    if (total > 0) {
        memcpy(in + o_pw, pw + 3 * (size_t)first, (size_t)total * 24);
        memcpy(in + o_obs, obs + 2 * (size_t)first, (size_t)total * 16);
        memcpy(in + o_w, inv_sigma2 + (size_t)first, (size_t)total * 8);
    }
    const double tr_staged = tr.us();
    if (int rc = call.upload(o_in, in_bytes)) return rc;
    double* hyp = (double*)(base + d_hyp); int* valid = (int*)(base + d_valid);
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3((unsigned)((n_hyp + kHypPerWg - 1) / kHypPerWg)), dim3(64), 0, s, (const uint8_t*)base, hyp, valid);
    hipLaunchKernelGGL(k_pnp_score, dim3((unsigned)n_sets), dim3(256), 0, s, (const uint8_t*)base, (const double*)hyp, (const int*)valid,
                       (PnpResult*)(hb + h_res), hb + h_flags, call.done.counter, call.done.flag, call.done.seq);
    if (int rc = call.finish()) return rc;
    const double tr_back = tr.us();
    // the refit of pnp_solve_ransac, per set (pnp_refit of epnp_math.h): EPnP over the winner's inliers, kept when it explains at least as many
    const PnpResult* res = (const PnpResult*)(hb + h_res);
    const uint8_t* fl = hb + h_flags;
    std::vector<double> scratch;
    std::vector<uint8_t> cur;
    for (int i = 0; i < n_sets; ++i) {
        const int o = off0[i], n = off0[i + 1] - o;
        const double* spw = pw + 3 * (size_t)(first + o); const double* sob = obs + 2 * (size_t)(first + o); const double* sw = inv_sigma2 + (size_t)(first + o);
        uint8_t* out_fl = inlier + (size_t)(first + o);
        double* p7 = pose7 + 7 * (size_t)i;
        int best = res[i].count;
        if (best_iteration) best_iteration[i] = best >= 4 ? res[i].best_iteration : -1;
        if (best < 4) {
            for (int k = 0; k < n; ++k) out_fl[k] = 0;
            n_inliers[i] = 0;
            p7[0] = 1; for (int k = 1; k < 7; ++k) p7[k] = 0;
            continue;
        }
        double bestR[9], bestT[3];
        for (int k = 0; k < 9; ++k) bestR[k] = res[i].R[k];
        for (int k = 0; k < 3; ++k) bestT[k] = res[i].t[k];
        for (int k = 0; k < n; ++k) out_fl[k] = fl[o + k];
        scratch.resize((size_t)12 * n); cur.resize((size_t)n);
        best = ep::pnp_refit(spw, sob, sw, n, cam4, best, out_fl, bestR, bestT, scratch.data(), cur.data());
        double q[4];
        LpSlam::rotToQuat(bestR, q);
        for (int k = 0; k < 4; ++k) p7[k] = q[k];
        for (int k = 0; k < 3; ++k) p7[4 + k] = bestT[k];
        n_inliers[i] = best;
    }
    if (tr.on()) fprintf(stderr, "pnp_ransac_batch: %d sets, %d matches, %d iterations; us: staged %.1f, results back %.1f, refitted %.1f\n", n_sets, total, iterations, tr_staged, tr_back, tr.us());
    return LPSLAM_HIP_OK;
}

}  // extern "C"
