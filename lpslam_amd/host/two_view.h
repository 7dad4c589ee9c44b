// two_view.h -- monocular map initialisation from two views (host, init only).
// What openvslam::system does inside feed_monocular_frame until a map exists (reference call site:
// /root/reference/src/Trackers/OpenVSLAMTracker.cpp:120; parameters of the generated configuration,
// src/Trackers/OpenVSLAMTrackerBase.cpp:161-201): [UPSTREAM] initialize::perspective -- homography and fundamental matrix by
// RANSAC over 8-match samples on Hartley-normalised keypoints (solve::homography_solver / solve::fundamental_solver), model
// choice by the score ratio (H if S_H / (S_H + S_F) > 0.40), motion hypotheses from the chosen model (4 from E = K^T F K, 8 from
// H by Faugeras' decomposition), linear triangulation of the inlier matches and the plausibility test of
// initialize::base::find_most_plausible_pose (positive depth, reprojection error, parallax, one clear winner).
// The upstream sources are absent from the reference tree; this restates the published algorithm (ORB-SLAM's Initializer, which
// OpenVSLAM follows) in FP64 with a deterministic sampler.
#pragma once
#include <cstdint>
#include <vector>

namespace LpSlam {

struct TwoViewParams {
    double sigma = 1.0;                  // keypoint standard deviation in pixels (level 0)
    int ransac_iters = 100;              // Initializer.num_ransac_iterations
    int min_triangulated = 50;           // Initializer.num_min_triangulated_pts
    double parallax_deg_thr = 1.0;       // Initializer.parallax_deg_threshold
    double reproj_err_thr = 4.0;         // Initializer.reprojection_error_threshold
    uint32_t seed = 0x9E3779B9u;         // sampler (xorshift32); upstream seeds from std::random_device
};

struct TwoViewResult {
    bool ok = false;
    int model = -1;                      // 0 = homography, 1 = fundamental matrix
    double score_h = 0, score_f = 0;
    double H[9] = {0}, F[9] = {0};       // reference -> current, row-major
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};     // reference -> current (|t| = 1)
    double parallax_deg = 0;
    int n_inliers = 0, n_valid = 0;
    std::vector<uint8_t> inlier;         // per match: inlier of the chosen model
    std::vector<uint8_t> triangulated;   // per match: landmark accepted
    std::vector<double> points;          // per match: X Y Z in the reference camera frame (valid where triangulated)
};

// The function is four steps: 1 the RANSAC loop over 8-match samples, 2 the refit of both winners and the
// model choice, 3 the decomposition into motion hypotheses, 4 the pose check of every hypothesis and the acceptance rules.  Steps 1
// and 4 exist on the device too (lpslam_hip_two_view_ransac_batch, lpslam_hip_two_view_check_poses: the same arithmetic,
// csrc/two_view_math.h, the same bits); a caller hands them in through TwoViewSteps.
// The winners of step 1 for one set of matches: per model the winning iteration (-1: none; then score 0, a zero matrix, flags cleared),
// its score, the matrix in pixel coordinates (reference -> current) and the per-match inlier flags.
struct TwoViewModels {
    int it_h = -1, it_f = -1;
    double score_h = 0, score_f = 0;
    double H[9] = {0}, F[9] = {0};
    std::vector<uint8_t> inl_h, inl_f;
};
// Steps 1 and 4 as a caller provides them (arguments of the two device entry points without the context, see include/lpslam_hip.h;
// 0 = done).  A step that is null or fails runs on the host; `calls` and `failed` count what happened.
struct TwoViewSteps {
    void* ctx = nullptr;
    int (*ransac)(void* ctx, int32_t n_sets, const int32_t* offsets, const double* p1, const double* p2, double sigma, int32_t iterations, uint32_t seed,
                  int32_t* best_iteration, double* score, double* model, uint8_t* inlier_h, uint8_t* inlier_f) = nullptr;
    int (*check_poses)(void* ctx, int32_t n_hyp, const double* R, const double* t, const double* K4, int32_t n, const double* p1, const double* p2,
                       const uint8_t* inlier, double th2, double* X, double* cosp, uint8_t* code) = nullptr;
    int calls = 0, failed = 0;
    double t_ransac = 0, t_refit = 0, t_decompose = 0, t_pose = 0;      // seconds of steps 1 .. 4 (the normalisation counts to none)
};

// K = (fx, fy, cx, cy), shared by both views; keypoints (x, y) in pixels; matches = (index in ref, index in cur) pairs
bool two_view_initialize(const double* K, const float* kp_ref, const float* kp_cur, const int32_t* matches, int n_matches,
                         const TwoViewParams& prm, TwoViewResult& out, TwoViewSteps* steps = nullptr);

// step 1 on the host: p1, p2 are n x 2 pixel coordinates (reference, current)
void two_view_ransac(const double* p1, const double* p2, int n, double sigma, int iterations, uint32_t seed, TwoViewModels& out);
// step 4's per-match part on the host, for n_hyp hypotheses (R: n_hyp x 9, t: n_hyp x 3): X (n_hyp x n x 3; NaN where the code is 0),
// cosp (n_hyp x n; 0 where the code is 0), code (n_hyp x n: 0 rejected or no inlier, 1 counted, 2 counted and good)
void two_view_check_poses(int n_hyp, const double* R, const double* t, const double* K4, int n, const double* p1, const double* p2,
                          const uint8_t* inlier, double th2, double* X, double* cosp, uint8_t* code);

// building blocks (exposed for the tests)
void sym_eigen_jacobi(const double* A, int n, double* eigval, double* eigvec);        // A symmetric n x n; eigvec columns, ascending eigval
void homography_from_matches(const double* x1, const double* x2, int n, double* H);   // DLT, x2 ~ H x1 (already normalised points)
void fundamental_from_matches(const double* x1, const double* x2, int n, double* F);  // 8-point + rank 2, x2^T F x1 = 0
bool triangulate_point(const double* P1, const double* P2, const double* x1, const double* x2, double* X);

// [UPSTREAM] solve::sim3_solver (ORB-SLAM Sim3Solver): the similarity (or rigid, fix_scale) transform between two keyframes from
// matched landmarks given in each keyframe's camera frame -- x1 = s R x2 + t -- by Horn's closed-form absolute orientation on
// 3-match samples (RANSAC, xorshift32 sampler as in two_view_initialize), scored by the reprojection error in BOTH images
// (chi-square 9.210 x the keypoint's level sigma^2).  This is what gives a loop candidate a transform WITHOUT trusting the current
// (drifted) pose estimates; the Sim3 optimiser on the device refines it.  p1c / p2c: n x 3, obs1 / obs2: n x 2 pixels,
// inv_sigma2_*: n.  Returns the number of inliers of the best hypothesis (0: none found); s12 = (qw qx qy qz tx ty tz s).
int sim3_solve_ransac(const double* p1c, const double* p2c, const double* obs1, const double* obs2, const double* inv_sigma2_1, const double* inv_sigma2_2,
                      int n, const double* cam1 /* fx fy cx cy */, const double* cam2, bool fix_scale, int iterations, uint32_t seed, double* s12, uint8_t* inlier);
// EPnP (Lepetit, Moreno-Noguer, Fua 2009): world -> camera (R row major, t) from n >= 4 landmark / pixel matches; false for degenerate input
bool epnp_solve(const double* pw, const double* uv, int n, const double* cam /* fx fy cx cy */, double* R, double* t);
// [UPSTREAM] solve::pnp_solver: world -> camera pose from n >= 4 landmark / keypoint matches, no prior: EPnP on 4-match samples (RANSAC),
// inliers by reprojection error (chi-square 5.991 at the keypoint's level), then EPnP once more over the inliers of the best sample.
// pw: n x 3 world points, obs: n x 2 pixels.  Returns the inlier count of the result (0: none); pose7 = qw qx qy qz tx ty tz.
int pnp_solve_ransac(const double* pw, const double* obs, const double* inv_sigma2, int n, const double* cam /* fx fy cx cy */, int iterations, uint32_t seed,
                     double* pose7, uint8_t* inlier);
// Horn's absolute orientation of n >= 3 matched points: x1 = s R x2 + t (R row major)
bool horn_absolute_orientation(const double* x1, const double* x2, int n, bool fix_scale, double* R, double* t, double* s);

}  // namespace LpSlam
