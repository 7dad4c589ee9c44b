// two_view_batch.cpp -- the CPU side of the two-view initialiser's device steps: C shims for the tests and the timing tool.
//   lpslam_two_view_sample_table        the 8-match samples two_view_initialize draws for a set of n matches (csrc/ransac_sample.h)
//   lpslam_two_view_models8_host        the header's two estimators at 8 on the host (the instance the RANSAC loop and the kernel run)
//   lpslam_two_view_ransac_batch_host   lpslam_hip_two_view_ransac_batch without the context: step 1 of two_view_initialize on each set
//   lpslam_two_view_check_poses_host    lpslam_hip_two_view_check_poses without the context: the per-match part of step 4
//   lpslam_two_view_initialize_steps    two_view_initialize with steps 1 and 4 taken through the hook from the two host forms above
//   lpslam_two_view_initialize_with     ... or from the caller's functions (the device entry points), with the seconds each step took
#include "two_view.h"
#include "../csrc/two_view_math.h"
#include "../csrc/ransac_sample.h"
#include <cstring>
#include <vector>

#define LP_EXPORT extern "C" __attribute__((visibility("default")))

// 1: table holds iterations x 8 indices; 0: n < 8 or iterations < 1, table untouched
LP_EXPORT int lpslam_two_view_sample_table(int n, int iterations, uint32_t seed, int32_t* table)
{
    if (n < 8 || iterations < 1 || !table) return 0;
    std::vector<int> avail((size_t)n);
    lpslam_ransac::sample_table<lpslam_tv::kSample>(n, iterations, seed, table, avail.data());
    return 1;
}

// x1, x2: eight (normalised) matches; H9, F9: the models in those coordinates
LP_EXPORT void lpslam_two_view_models8_host(const double* x1, const double* x2, double* H9, double* F9)
{
    double ws[lpslam_tv::kWorkspace];
    lpslam_tv::homography_from_matches<8>(x1, x2, 8, ws, 1, H9);
    lpslam_tv::fundamental_from_matches<8>(x1, x2, 8, ws, 1, F9);
}

// LpSlam::homography_from_matches / fundamental_from_matches (the header's estimators at a run-time count: the refit's instance)
LP_EXPORT void lpslam_two_view_models_host(const double* x1, const double* x2, int n, double* H9, double* F9)
{
    LpSlam::homography_from_matches(x1, x2, n, H9);
    LpSlam::fundamental_from_matches(x1, x2, n, F9);
}

// 0: done; 1: refused (the argument rules of lpslam_hip_two_view_ransac_batch), nothing written
LP_EXPORT int lpslam_two_view_ransac_batch_host(int32_t n_sets, const int32_t* offsets, const double* p1, const double* p2, double sigma, int32_t iterations, uint32_t seed,
                                                int32_t* best_iteration, double* score, double* model, uint8_t* inlier_h, uint8_t* inlier_f)
{
    int first = 0, total = 0;
    if (lpslam_ransac::check_offsets(n_sets, offsets, &first, &total) || iterations < 1 || iterations > 1024 || !(sigma > 0) || !__builtin_isfinite(sigma)) return 1;
    if ((n_sets > 0 && (!best_iteration || !score || !model)) || (total > 0 && (!p1 || !p2 || !inlier_h || !inlier_f))) return 1;
    LpSlam::TwoViewModels w;
    for (int s = 0; s < n_sets; ++s) {
        const size_t o = (size_t)offsets[s];
        const int n = offsets[s + 1] - offsets[s];
        LpSlam::two_view_ransac(p1 + 2 * o, p2 + 2 * o, n, sigma, iterations, seed, w);
        best_iteration[2 * s] = w.it_h; best_iteration[2 * s + 1] = w.it_f;
        score[2 * s] = w.score_h; score[2 * s + 1] = w.score_f;
        std::memcpy(model + 18 * (size_t)s, w.H, sizeof(w.H)); std::memcpy(model + 18 * (size_t)s + 9, w.F, sizeof(w.F));
        for (int i = 0; i < n; ++i) { inlier_h[o + (size_t)i] = w.inl_h[(size_t)i]; inlier_f[o + (size_t)i] = w.inl_f[(size_t)i]; }
    }
    return 0;
}

// 0: done; 1: refused (the argument rules of lpslam_hip_two_view_check_poses), nothing written
LP_EXPORT int lpslam_two_view_check_poses_host(int32_t n_hyp, const double* R, const double* t, const double* K4, int32_t n, const double* p1, const double* p2,
                                               const uint8_t* inlier, double th2, double* X, double* cosp, uint8_t* code)
{
    if (n_hyp < 0 || n_hyp > 8 || n < 0 || !K4 || (n_hyp > 0 && (!R || !t))) return 1;
    if (n_hyp > 0 && n > 0 && (!p1 || !p2 || !inlier || !X || !cosp || !code)) return 1;
    LpSlam::two_view_check_poses(n_hyp, R, t, K4, n, p1, p2, inlier, th2, X, cosp, code);
    return 0;
}

LP_EXPORT int lpslam_two_view_initialize_with(void* ctx, void* ransac_fn, void* poses_fn, const double* K, const float* kp_ref, const float* kp_cur, const int32_t* matches,
                                              int n_matches, double sigma, int ransac_iters, uint32_t seed, double* R9, double* t3, double* H9, double* F9, double* scores2,
                                              double* parallax_deg, int32_t* model, uint8_t* inlier, uint8_t* triangulated, double* points3, int32_t* calls2, double* seconds4);

namespace {
int ransac_hook(void*, int32_t n_sets, const int32_t* offsets, const double* p1, const double* p2, double sigma, int32_t iterations, uint32_t seed,
                int32_t* best_iteration, double* score, double* model, uint8_t* inlier_h, uint8_t* inlier_f)
{
    return lpslam_two_view_ransac_batch_host(n_sets, offsets, p1, p2, sigma, iterations, seed, best_iteration, score, model, inlier_h, inlier_f);
}
int poses_hook(void*, int32_t n_hyp, const double* R, const double* t, const double* K4, int32_t n, const double* p1, const double* p2, const uint8_t* inlier, double th2,
               double* X, double* cosp, uint8_t* code)
{
    return lpslam_two_view_check_poses_host(n_hyp, R, t, K4, n, p1, p2, inlier, th2, X, cosp, code);
}
}  // namespace

// lpslam_two_view_initialize (two_view.cpp) with steps 1 and 4 handed in through TwoViewSteps, as the tracker hands in the device calls;
// calls2 (may be null) receives how many step calls were made and how many failed
LP_EXPORT int lpslam_two_view_initialize_steps(const double* K, const float* kp_ref, const float* kp_cur, const int32_t* matches, int n_matches, double sigma,
                                               int ransac_iters, uint32_t seed, double* R9, double* t3, double* H9, double* F9, double* scores2, double* parallax_deg,
                                               int32_t* model, uint8_t* inlier, uint8_t* triangulated, double* points3, int32_t* calls2)
{
    return lpslam_two_view_initialize_with(nullptr, nullptr, nullptr, K, kp_ref, kp_cur, matches, n_matches, sigma, ransac_iters, seed, R9, t3, H9, F9, scores2, parallax_deg,
                                           model, inlier, triangulated, points3, calls2, nullptr);
}

// The same with the steps of the caller's choice (the timing tool): ransac_fn / poses_fn are the addresses of lpslam_hip_two_view_ransac_batch /
// lpslam_hip_two_view_check_poses and ctx their context, or null for the host forms; seconds4 (may be null) receives the seconds of the four steps
LP_EXPORT int lpslam_two_view_initialize_with(void* ctx, void* ransac_fn, void* poses_fn, const double* K, const float* kp_ref, const float* kp_cur, const int32_t* matches,
                                              int n_matches, double sigma, int ransac_iters, uint32_t seed, double* R9, double* t3, double* H9, double* F9, double* scores2,
                                              double* parallax_deg, int32_t* model, uint8_t* inlier, uint8_t* triangulated, double* points3, int32_t* calls2, double* seconds4)
{
    LpSlam::TwoViewParams prm;
    prm.sigma = sigma; prm.ransac_iters = ransac_iters; prm.seed = seed;
    LpSlam::TwoViewResult res;
    LpSlam::TwoViewSteps st;
    st.ctx = ctx;
    st.ransac = ransac_fn ? (decltype(st.ransac))ransac_fn : ransac_hook;
    st.check_poses = poses_fn ? (decltype(st.check_poses))poses_fn : poses_hook;
    const bool ok = LpSlam::two_view_initialize(K, kp_ref, kp_cur, matches, n_matches, prm, res, &st);
    if (R9) std::memcpy(R9, res.R, sizeof(res.R));
    if (t3) std::memcpy(t3, res.t, sizeof(res.t));
    if (H9) std::memcpy(H9, res.H, sizeof(res.H));
    if (F9) std::memcpy(F9, res.F, sizeof(res.F));
    if (scores2) { scores2[0] = res.score_h; scores2[1] = res.score_f; }
    if (parallax_deg) *parallax_deg = res.parallax_deg;
    if (model) *model = res.model;
    for (int i = 0; i < n_matches; ++i) {
        if (inlier) inlier[i] = res.inlier.size() > (size_t)i ? res.inlier[(size_t)i] : 0;
        if (triangulated) triangulated[i] = res.triangulated.size() > (size_t)i ? res.triangulated[(size_t)i] : 0;
        if (points3) for (int c = 0; c < 3; ++c) points3[3 * i + c] = res.points.size() > (size_t)(3 * i + c) ? res.points[(size_t)(3 * i + c)] : 0.0;
    }
    if (calls2) { calls2[0] = st.calls; calls2[1] = st.failed; }
    if (seconds4) { seconds4[0] = st.t_ransac; seconds4[1] = st.t_refit; seconds4[2] = st.t_decompose; seconds4[3] = st.t_pose; }
    return ok ? 1 : 0;
}
