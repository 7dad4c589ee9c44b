// two_view.hip -- steps 1 and 4 of the monocular two-view initialiser for the device ([UPSTREAM]
// initialize::perspective, the host form is LpSlam::two_view_initialize in lpslam_amd/host/two_view.cpp).  The arithmetic is
// two_view_math.h, the text the host runs.
// lpslam_hip_two_view_ransac_batch, S sets of pixel matches:
//   host          Hartley normalisation of each set, the sample table (the 8-match samples two_view_initialize would draw) and ONE
//                 upload of both with the matches
//   k_tv_models   sixteen lanes per (set, iteration, model): the homography or the fundamental matrix of the eight sampled matches;
//                 the 9 x 9 matrix and its eigenvectors live in LDS (1.3 KB a unit, four units a wave), the lanes divide the 81 sums
//                 and each Jacobi rotation's elements among them; de-normalised to pixels, for H also det and the inverse
//   k_tv_score    one workgroup per (set, model), a wave per hypothesis in turn: the lanes compute the terms of 64 matches, then the
//                 wave adds them in index order, each read from its lane's register (the order of that sum is part of the definition:
//                 no tree, no reduction across lanes); the winner by (valid, score bits, ~iteration), its flags and record written
//                 to page-locked memory, then the done flag
//   host          one wait
// lpslam_hip_two_view_check_poses, P <= 8 motion hypotheses over n matches:
//   k_tv_pose     one lane per (hypothesis, match): X, the cosine of the parallax and the code, to page-locked memory; one wait
// The round trip of either call -- page-locked block, device block, done flag, what becomes of them when a stream is late or dead --
// is LpStagedCall (internal.h).
#include "internal.h"
#include "two_view_math.h"
#include "ransac_sample.h"
#include <cmath>

using namespace lpslam;
namespace tv = lpslam_tv;

namespace {

constexpr int kUnitLanes = 16;         // lanes that estimate one model together
constexpr int kUnitsPerWg = 64 / kUnitLanes;   // one wave per workgroup
constexpr int kUnitLds = tv::kWorkspace + 2;   // doubles of LDS per unit: the four workspaces of a wave start on different banks
constexpr int kScoreWaves = 16;        // waves of a scoring workgroup: hypotheses in flight per (set, model)

struct TvHead { double inv_s2; int32_t n_sets, iterations; uint32_t o_offsets, o_table, o_norm, o_p1, o_p2, o_n1, o_n2, pad; };
struct TvResult { int32_t best_iteration, pad; double score, M[9]; };
static_assert(sizeof(TvResult) == 88, "result record");
constexpr int kHypDoubles = 27;        // per (set, iteration): H21, inverse(H21), F21

__global__ __launch_bounds__(64) void k_tv_models(const uint8_t* __restrict__ base, double* __restrict__ hyp, int* __restrict__ valid)
{
    __shared__ double ws[kUnitLds * kUnitsPerWg];
    const TvHead& head = *(const TvHead*)base;
    const int group = threadIdx.x / kUnitLanes, ln = threadIdx.x % kUnitLanes;
    const long long u = (long long)blockIdx.x * kUnitsPerWg + group;
    if (u >= 2ll * head.n_sets * head.iterations) return;      // (the sixteen lanes of a unit together; no workgroup barrier in this kernel)
    const size_t h = (size_t)(u >> 1);
    const int model = (int)(u & 1);
    const int s = (int)(h / (size_t)head.iterations);
    const int32_t* off = (const int32_t*)(base + head.o_offsets);
    const int o = off[s], n = off[s + 1] - o;
    if (n < tv::kSample) { if (ln == 0) valid[u] = 0; return; }
    const int32_t* idx = (const int32_t*)(base + head.o_table) + tv::kSample * h;
    const double* n1 = (const double*)(base + head.o_n1);
    const double* n2 = (const double*)(base + head.o_n2);
    const double* nm = (const double*)(base + head.o_norm) + 27 * (size_t)s;      // T1, inverse(T2), transpose(T2)
    double s1[16], s2[16];
    for (int k = 0; k < tv::kSample; ++k) {
        const size_t m = (size_t)o + (size_t)min(max(idx[k], 0), n - 1);
        s1[2 * k] = n1[2 * m]; s1[2 * k + 1] = n1[2 * m + 1]; s2[2 * k] = n2[2 * m]; s2[2 * k + 1] = n2[2 * m + 1];
    }
    tv::M3 T1, Tl, Mn;
    for (int k = 0; k < 9; ++k) { T1.m[k] = nm[k]; Tl.m[k] = nm[(model ? 18 : 9) + k]; }
    if (model == 0) tv::homography_from_matches<8>(s1, s2, 8, ws + kUnitLds * group, 1, Mn.m, ln, kUnitLanes);
    else tv::fundamental_from_matches<8>(s1, s2, 8, ws + kUnitLds * group, 1, Mn.m, ln, kUnitLanes);
    if (ln != 0) return;
    const tv::M3 M21 = tv::mul(tv::mul(Tl, Mn), T1);
    double* out = hyp + kHypDoubles * h;
    if (model == 0) {
        const bool ok = fabs(tv::det(M21)) > 1e-300;
        valid[u] = ok ? 1 : 0;
        if (ok) { const tv::M3 M12 = tv::inverse(M21); for (int k = 0; k < 9; ++k) { out[k] = M21.m[k]; out[9 + k] = M12.m[k]; } }
    } else {
        valid[u] = 1;
        for (int k = 0; k < 9; ++k) out[18 + k] = M21.m[k];
    }
}

// x of lane k, k the same for the whole wave
__device__ __forceinline__ double lane_value(double x, int k)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), k), hi = __builtin_amdgcn_readlane(__double2hiint(x), k);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(64 * kScoreWaves) void k_tv_score(const uint8_t* __restrict__ base, const double* __restrict__ hyp, const int* __restrict__ valid,
                                                               TvResult* __restrict__ res, uint8_t* __restrict__ flags_h, uint8_t* __restrict__ flags_f,
                                                               unsigned* counter, int* flag, int seq)
{
    __shared__ unsigned long long wbits[kScoreWaves];
    __shared__ int wit[kScoreWaves];
    const TvHead& head = *(const TvHead*)base;
    const int s = blockIdx.x >> 1, model = blockIdx.x & 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* off = (const int32_t*)(base + head.o_offsets);
    const int o = off[s], n = off[s + 1] - o;
    const double* p1 = (const double*)(base + head.o_p1) + 2 * (size_t)o;
    const double* p2 = (const double*)(base + head.o_p2) + 2 * (size_t)o;
    const double inv_s2 = head.inv_s2;
    // the host's `s > best` from -1: the largest score, the lowest iteration among equal ones, never a NaN; a score of 0.0 does win
    // over none -- (valid, score bits, ~iteration) in that order, a non-negative finite double orders like its bit pattern
    int best_it = -1;
    unsigned long long best_bits = 0;
    if (n >= tv::kSample)
        for (int it = wave; it < head.iterations; it += kScoreWaves) {      // the same for every lane of a wave
            const size_t h = (size_t)s * (size_t)head.iterations + (size_t)it;
            if (!valid[2 * h + model]) continue;
            double M[18];
            for (int k = 0; k < 18; ++k) M[k] = model == 0 ? hyp[kHypDoubles * h + k] : (k < 9 ? hyp[kHypDoubles * h + 18 + k] : 0.0);
            double score = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                tv::MatchTerms m{0, 0, 0, 0, 0};
                if (i < n) {
                    const double u1 = p1[2 * (size_t)i], v1 = p1[2 * (size_t)i + 1], u2 = p2[2 * (size_t)i], v2 = p2[2 * (size_t)i + 1];
                    m = model == 0 ? tv::homography_terms(M, M + 9, u1, v1, u2, v2, inv_s2) : tv::fundamental_terms(M, u1, v1, u2, v2, inv_s2);
                }
                // every lane adds the 64 matches' terms in index order, first direction then second, read from the lane that holds them
                // (a uniform lane index: a register read, no LDS); the score is the same in all lanes
                const unsigned long long m1 = __ballot(m.add1 != 0), m2 = __ballot(m.add2 != 0);
                const int cnt = min(64, n - i0);
                for (int k = 0; k < cnt; ++k) {
                    if ((m1 >> k) & 1) score += lane_value(m.t1, k);
                    if ((m2 >> k) & 1) score += lane_value(m.t2, k);
                }
            }
            if (lane == 0 && score == score) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(score);
                if (best_it < 0 || bits > best_bits) { best_bits = bits; best_it = it; }      // (a wave's iterations ascend)
            }
        }
    if (lane == 0) { wbits[wave] = best_bits; wit[wave] = best_it; }
    __syncthreads();
    best_it = wit[0]; best_bits = wbits[0];
    for (int k = 1; k < kScoreWaves; ++k) {
        const int it = wit[k];
        if (it < 0) continue;
        if (best_it < 0 || wbits[k] > best_bits || (wbits[k] == best_bits && it < best_it)) { best_bits = wbits[k]; best_it = it; }
    }
    uint8_t* fl = (model == 0 ? flags_h : flags_f) + o;
    if (best_it < 0) {                                                    // none: fewer than eight matches or no valid hypothesis
        for (int i = threadIdx.x; i < n; i += blockDim.x) fl[i] = 0;
        if (threadIdx.x == 0) {
            TvResult r{};
            r.best_iteration = -1;
            res[2 * s + model] = r;
        }
    } else {
        const size_t h = (size_t)s * (size_t)head.iterations + (size_t)best_it;
        double M[18];
        for (int k = 0; k < 18; ++k) M[k] = model == 0 ? hyp[kHypDoubles * h + k] : (k < 9 ? hyp[kHypDoubles * h + 18 + k] : 0.0);
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const double u1 = p1[2 * (size_t)i], v1 = p1[2 * (size_t)i + 1], u2 = p2[2 * (size_t)i], v2 = p2[2 * (size_t)i + 1];
            const tv::MatchTerms m = model == 0 ? tv::homography_terms(M, M + 9, u1, v1, u2, v2, inv_s2) : tv::fundamental_terms(M, u1, v1, u2, v2, inv_s2);
            fl[i] = (uint8_t)m.inlier;
        }
        if (threadIdx.x == 0) {
            TvResult r{};
            r.best_iteration = best_it; r.score = __longlong_as_double((long long)best_bits);
            for (int k = 0; k < 9; ++k) r.M[k] = M[k];
            res[2 * s + model] = r;
        }
    }
    lp_signal_done(counter, flag, seq);
}

struct PoseHead { double R[72], t[24], K[4], th2; int32_t n_hyp, n; };

__global__ __launch_bounds__(256) void k_tv_pose(PoseHead head, const double* __restrict__ p1, const double* __restrict__ p2, const uint8_t* __restrict__ inl,
                                                 double* __restrict__ X, double* __restrict__ cosp, uint8_t* __restrict__ code, unsigned* counter, int* flag, int seq)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < (long long)head.n_hyp * head.n) {
        const int h = (int)(idx / head.n), i = (int)(idx - (long long)h * head.n);
        double R[9], t[3], K[4];
        for (int k = 0; k < 9; ++k) R[k] = head.R[9 * h + k];
        for (int k = 0; k < 3; ++k) t[k] = head.t[3 * h + k];
        for (int k = 0; k < 4; ++k) K[k] = head.K[k];
        double x[3] = {0, 0, 0}, c = 0;
        int k = tv::kPoseRejected;
        if (inl[i]) {
            tv::PoseSetup ps;
            tv::pose_setup(R, t, K, ps);
            const double x1[2] = {p1[2 * (size_t)i], p1[2 * (size_t)i + 1]}, x2[2] = {p2[2 * (size_t)i], p2[2 * (size_t)i + 1]};
            k = tv::pose_point(ps, R, t, K, x1, x2, head.th2, x, &c);
        }
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        code[idx] = (uint8_t)k;
        cosp[idx] = k ? c : 0.0;
        for (int a = 0; a < 3; ++a) X[3 * idx + a] = k ? x[a] : nan;
    }
    lp_signal_done(counter, flag, seq);
}

}  // namespace

extern "C" {

int lpslam_hip_two_view_ransac_batch(lpslam_hip_ctx* c, int32_t n_sets, const int32_t* offsets, const double* p1, const double* p2, double sigma, int32_t iterations,
                                     uint32_t seed, int32_t* best_iteration, double* score, double* model, uint8_t* inlier_h, uint8_t* inlier_f)
{
    if (!c) { set_error("null context"); return LPSLAM_HIP_ERR_INVALID; }
    int first = 0, total = 0;
    if (const char* why = lpslam_ransac::check_offsets(n_sets, offsets, &first, &total)) { set_error("two_view_ransac_batch: %s", why); return LPSLAM_HIP_ERR_INVALID; }
    if (iterations < 1 || iterations > LPSLAM_HIP_TWO_VIEW_MAX_ITERATIONS) { set_error("two_view_ransac_batch: %d iterations outside 1 .. %d", iterations, LPSLAM_HIP_TWO_VIEW_MAX_ITERATIONS); return LPSLAM_HIP_ERR_INVALID; }
    if (!(sigma > 0) || !std::isfinite(sigma)) { set_error("two_view_ransac_batch: sigma is no positive number"); return LPSLAM_HIP_ERR_INVALID; }
    if (n_sets > 0 && (!best_iteration || !score || !model)) { set_error("two_view_ransac_batch: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (total > 0 && (!p1 || !p2 || !inlier_h || !inlier_f)) { set_error("two_view_ransac_batch: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (n_sets == 0) return LPSLAM_HIP_OK;
    const size_t n_hyp = (size_t)n_sets * (size_t)iterations;
    if (n_hyp > (size_t)0x7fffffff / 8) { set_error("two_view_ransac_batch: %d sets x %d iterations do not fit one launch", n_sets, iterations); return LPSLAM_HIP_ERR_CAPACITY; }
    LP_HIP(hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    const LpMatchTrace tr;
    // page-locked block: flag | input (head, offsets rebased to 0, sample table, the sets' normalisations, the matches in pixels and
    // normalised) | results (two records per set, two flags per match); device block: the input, then the hypotheses and their valid flags
    const size_t o_in = 64, tot1 = (size_t)std::max(total, 1);
    LpLayout dev;
    dev.take(sizeof(TvHead));
    const size_t o_offsets = dev.take((size_t)(n_sets + 1) * 4), o_table = dev.take(n_hyp * 32), o_norm = dev.take((size_t)n_sets * 27 * 8);
    const size_t o_p1 = dev.take(tot1 * 16), o_p2 = dev.take(tot1 * 16), o_n1 = dev.take(tot1 * 16), o_n2 = dev.take(tot1 * 16);
    const size_t in_bytes = dev.at;
    const size_t d_hyp = dev.take(n_hyp * kHypDoubles * 8), d_valid = dev.take(n_hyp * 2 * 4);
    LpLayout host{o_in + in_bytes};
    const size_t h_res = host.take((size_t)n_sets * 2 * sizeof(TvResult)), h_fh = host.take(tot1), h_ff = host.take(tot1);
    LpStagedCall call{c, s, "two_view_ransac_batch"};
    if (int rc = call.open(host.at, dev.at, LP_DONE_TWO_VIEW)) return rc;
    uint8_t *hb = call.host, *base = call.dev(), *in = hb + o_in;
    TvHead head{};
    head.inv_s2 = 1.0 / (sigma * sigma);
    head.n_sets = n_sets; head.iterations = iterations;
    head.o_offsets = (uint32_t)o_offsets; head.o_table = (uint32_t)o_table; head.o_norm = (uint32_t)o_norm;
    head.o_p1 = (uint32_t)o_p1; head.o_p2 = (uint32_t)o_p2; head.o_n1 = (uint32_t)o_n1; head.o_n2 = (uint32_t)o_n2;
    memcpy(in, &head, sizeof head);
    int32_t* off0 = (int32_t*)(in + o_offsets);
    for (int i = 0; i <= n_sets; ++i) off0[i] = offsets[i] - first;
    if (total > 0) {
        memcpy(in + o_p1, p1 + 2 * (size_t)first, (size_t)total * 16);
        memcpy(in + o_p2, p2 + 2 * (size_t)first, (size_t)total * 16);
    }
    lpslam_ransac::batch_tables<tv::kSample>(n_sets, off0, iterations, seed, (int32_t*)(in + o_table));
    for (int i = 0; i < n_sets; ++i) {
        const int o = off0[i], n = off0[i + 1] - o;
        double* nm = (double*)(in + o_norm) + 27 * (size_t)i;
        if (n < tv::kSample) { memset(nm, 0, 27 * 8); continue; }
        tv::M3 T1, T2;
        tv::normalize_points((const double*)(in + o_p1) + 2 * (size_t)o, (size_t)n, (double*)(in + o_n1) + 2 * (size_t)o, T1);
        tv::normalize_points((const double*)(in + o_p2) + 2 * (size_t)o, (size_t)n, (double*)(in + o_n2) + 2 * (size_t)o, T2);
        const tv::M3 T2inv = tv::inverse(T2), T2t = tv::transpose(T2);
        memcpy(nm, T1.m, 72); memcpy(nm + 9, T2inv.m, 72); memcpy(nm + 18, T2t.m, 72);
    }
    const double tr_staged = tr.us();
    if (int rc = call.upload(o_in, in_bytes)) return rc;
    double* hyp = (double*)(base + d_hyp); int* valid = (int*)(base + d_valid);
    const size_t n_units = 2 * n_hyp;
    hipLaunchKernelGGL(k_tv_models, dim3((unsigned)((n_units + kUnitsPerWg - 1) / kUnitsPerWg)), dim3(64), 0, s, (const uint8_t*)base, hyp, valid);
    hipLaunchKernelGGL(k_tv_score, dim3((unsigned)(2 * n_sets)), dim3(64 * kScoreWaves), 0, s, (const uint8_t*)base, (const double*)hyp, (const int*)valid,
                       (TvResult*)(hb + h_res), hb + h_fh, hb + h_ff, call.done.counter, call.done.flag, call.done.seq);
    if (int rc = call.finish()) return rc;
    const TvResult* res = (const TvResult*)(hb + h_res);
    for (int i = 0; i < n_sets; ++i) {
        const int o = off0[i], n = off0[i + 1] - o;
        for (int m = 0; m < 2; ++m) {
            const TvResult& r = res[2 * i + m];
            best_iteration[2 * i + m] = r.best_iteration; score[2 * i + m] = r.score;
            memcpy(model + 18 * (size_t)i + 9 * (size_t)m, r.M, 72);
        }
        if (n > 0) { memcpy(inlier_h + (size_t)(first + o), hb + h_fh + o, (size_t)n); memcpy(inlier_f + (size_t)(first + o), hb + h_ff + o, (size_t)n); }
    }
    if (tr.on()) fprintf(stderr, "two_view_ransac_batch: %d sets, %d matches, %d iterations; us: staged %.1f, results back %.1f\n", n_sets, total, iterations, tr_staged, tr.us());
    return LPSLAM_HIP_OK;
}

int lpslam_hip_two_view_check_poses(lpslam_hip_ctx* c, int32_t n_hyp, const double* R, const double* t, const double* K4, int32_t n, const double* p1, const double* p2,
                                    const uint8_t* inlier, double th2, double* X, double* cosp, uint8_t* code)
{
    if (!c) { set_error("null context"); return LPSLAM_HIP_ERR_INVALID; }
    if (n_hyp < 0 || n_hyp > LPSLAM_HIP_TWO_VIEW_MAX_POSES) { set_error("two_view_check_poses: %d hypotheses outside 0 .. %d", n_hyp, LPSLAM_HIP_TWO_VIEW_MAX_POSES); return LPSLAM_HIP_ERR_INVALID; }
    if (n < 0) { set_error("two_view_check_poses: %d matches", n); return LPSLAM_HIP_ERR_INVALID; }
    if (!K4 || (n_hyp > 0 && (!R || !t))) { set_error("two_view_check_poses: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (n_hyp > 0 && n > 0 && (!p1 || !p2 || !inlier || !X || !cosp || !code)) { set_error("two_view_check_poses: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (n_hyp == 0 || n == 0) return LPSLAM_HIP_OK;
    LP_HIP(hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    const size_t pn = (size_t)n_hyp * (size_t)n;
    // page-locked block: flag | input (the matches, their flags) | results (X, cosines, codes); device block: the input
    const size_t o_in = 64;
    LpLayout dev;
    const size_t o_p1 = dev.take((size_t)n * 16), o_p2 = dev.take((size_t)n * 16), o_fl = dev.take((size_t)n);
    const size_t in_bytes = dev.at;
    LpLayout host{o_in + in_bytes};
    const size_t h_x = host.take(pn * 24), h_cos = host.take(pn * 8), h_code = host.take(pn);
    LpStagedCall call{c, s, "two_view_check_poses"};
    if (int rc = call.open(host.at, in_bytes, LP_DONE_TWO_VIEW)) return rc;
    uint8_t *hb = call.host, *base = call.dev(), *in = hb + o_in;
    memcpy(in + o_p1, p1, (size_t)n * 16); memcpy(in + o_p2, p2, (size_t)n * 16); memcpy(in + o_fl, inlier, (size_t)n);
    PoseHead head{};
    memcpy(head.R, R, (size_t)n_hyp * 72); memcpy(head.t, t, (size_t)n_hyp * 24); memcpy(head.K, K4, 32);
    head.th2 = th2; head.n_hyp = n_hyp; head.n = n;
    if (int rc = call.upload(o_in, in_bytes)) return rc;
    hipLaunchKernelGGL(k_tv_pose, dim3((unsigned)((pn + 255) / 256)), dim3(256), 0, s, head, (const double*)(base + o_p1), (const double*)(base + o_p2),
                       (const uint8_t*)(base + o_fl), (double*)(hb + h_x), (double*)(hb + h_cos), hb + h_code, call.done.counter, call.done.flag, call.done.seq);
    if (int rc = call.finish()) return rc;
    memcpy(X, hb + h_x, pn * 24); memcpy(cosp, hb + h_cos, pn * 8); memcpy(code, hb + h_code, pn);
    return LPSLAM_HIP_OK;
}

}  // extern "C"
