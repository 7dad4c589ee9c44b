// two_view.cpp -- see two_view.h
#include "two_view.h"
#include "pose_math.h"
#include "../csrc/epnp_math.h"
#include "../csrc/ransac_sample.h"
#include "../csrc/sim3_math.h"
#include "../csrc/triangulate_math.h"
#include "../csrc/two_view_math.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstring>
#include <limits>

namespace LpSlam {

namespace {

using lpslam_tv::M3; using lpslam_tv::mul; using lpslam_tv::transpose; using lpslam_tv::det; using lpslam_tv::inverse;      // csrc/two_view_math.h

// M = U diag(s) V^T, s descending; U, V proper or improper as they come (callers fix signs)
void svd3(const M3& M, M3& U, double* s, M3& V)
{
    const M3 MtM = mul(transpose(M), M);
    double ev[3], evec[9];
    sym_eigen_jacobi(MtM.m, 3, ev, evec);                       // ascending
    for (int c = 0; c < 3; ++c) {
        const int src = 2 - c;
        s[c] = std::sqrt(std::max(ev[src], 0.0));
        for (int r = 0; r < 3; ++r) V.m[r * 3 + c] = evec[r * 3 + src];
    }
    for (int c = 0; c < 2; ++c) {
        double u[3] = {0, 0, 0};
        for (int r = 0; r < 3; ++r) u[r] = M.m[r * 3] * V.m[c] + M.m[r * 3 + 1] * V.m[3 + c] + M.m[r * 3 + 2] * V.m[6 + c];
        const double n = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        for (int r = 0; r < 3; ++r) U.m[r * 3 + c] = n > 0 ? u[r] / n : (r == c ? 1.0 : 0.0);
    }
    // second column re-orthogonalised against the first, third = first x second (valid for rank 2 and rank 3 alike up to sign)
    double d01 = U.m[0] * U.m[1] + U.m[3] * U.m[4] + U.m[6] * U.m[7];
    for (int r = 0; r < 3; ++r) U.m[r * 3 + 1] -= d01 * U.m[r * 3];
    double n1 = std::sqrt(U.m[1] * U.m[1] + U.m[4] * U.m[4] + U.m[7] * U.m[7]);
    for (int r = 0; r < 3; ++r) U.m[r * 3 + 1] /= n1;
    U.m[2] = U.m[3] * U.m[7] - U.m[6] * U.m[4];
    U.m[5] = U.m[6] * U.m[1] - U.m[0] * U.m[7];
    U.m[8] = U.m[0] * U.m[4] - U.m[3] * U.m[1];
    // sign of the third column such that M v3 = s3 u3 where s3 is not negligible
    double mv[3];
    for (int r = 0; r < 3; ++r) mv[r] = M.m[r * 3] * V.m[2] + M.m[r * 3 + 1] * V.m[5] + M.m[r * 3 + 2] * V.m[8];
    if (mv[0] * U.m[2] + mv[1] * U.m[5] + mv[2] * U.m[8] < 0) for (int r = 0; r < 3; ++r) U.m[r * 3 + 2] = -U.m[r * 3 + 2];
}

void normalize_points(const std::vector<double>& in, std::vector<double>& out, M3& T)
{
    out.resize(in.size());
    lpslam_tv::normalize_points(in.data(), in.size() / 2, out.data(), T);
}

// the score of a model over all matches: the terms of csrc/two_view_math.h added in index order, first direction then second
double check_homography(const M3& H21, const M3& H12, const double* p1, const double* p2, size_t n, double sigma, std::vector<uint8_t>& inl)
{
    const double inv_s2 = 1.0 / (sigma * sigma);
    double score = 0;
    inl.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const lpslam_tv::MatchTerms m = lpslam_tv::homography_terms(H21.m, H12.m, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1], inv_s2);
        if (m.add1) score += m.t1;
        if (m.add2) score += m.t2;
        inl[i] = (uint8_t)m.inlier;
    }
    return score;
}

double check_fundamental(const M3& F21, const double* p1, const double* p2, size_t n, double sigma, std::vector<uint8_t>& inl)
{
    const double inv_s2 = 1.0 / (sigma * sigma);
    double score = 0;
    inl.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const lpslam_tv::MatchTerms m = lpslam_tv::fundamental_terms(F21.m, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1], inv_s2);
        if (m.add1) score += m.t1;
        if (m.add2) score += m.t2;
        inl[i] = (uint8_t)m.inlier;
    }
    return score;
}

struct Hypothesis { M3 R; double t[3]; };

// what check_pose does after its loop over the matches (ORB-SLAM CheckRT / OpenVSLAM check_triangulated_pts): the plausible points
// counted, their cosines in match order sorted, the parallax from the 51st
int pose_tally(const double* X, const double* cosp, const uint8_t* code, size_t n, std::vector<double>& pts, std::vector<uint8_t>& good, double& parallax_deg)
{
    pts.assign(3 * n, std::numeric_limits<double>::quiet_NaN());
    good.assign(n, 0);
    std::vector<double> cosines;
    int n_good = 0;
    for (size_t i = 0; i < n; ++i) {
        if (code[i] == lpslam_tv::kPoseRejected) continue;
        cosines.push_back(cosp[i]);
        pts[3 * i] = X[3 * i]; pts[3 * i + 1] = X[3 * i + 1]; pts[3 * i + 2] = X[3 * i + 2];
        ++n_good;
        if (code[i] == lpslam_tv::kPoseGood) good[i] = 1;
    }
    parallax_deg = 0;
    if (!cosines.empty()) {
        std::sort(cosines.begin(), cosines.end());
        const size_t idx = std::min<size_t>(50, cosines.size() - 1);
        parallax_deg = std::acos(std::min(1.0, std::max(-1.0, cosines[idx]))) * 180.0 / M_PI;
    }
    return n_good;
}

void hypotheses_from_fundamental(const M3& F21, const double* K, std::vector<Hypothesis>& out)
{
    const M3 Km{{K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1}};
    const M3 E = mul(mul(transpose(Km), F21), Km);
    M3 U, V; double s[3];
    svd3(E, U, s, V);
    if (det(U) < 0) for (int r = 0; r < 3; ++r) U.m[r * 3 + 2] = -U.m[r * 3 + 2];
    if (det(V) < 0) for (int r = 0; r < 3; ++r) V.m[r * 3 + 2] = -V.m[r * 3 + 2];
    const M3 W{{0, -1, 0, 1, 0, 0, 0, 0, 1}};
    M3 R1 = mul(mul(U, W), transpose(V)), R2 = mul(mul(U, transpose(W)), transpose(V));
    if (det(R1) < 0) for (double& v : R1.m) v = -v;
    if (det(R2) < 0) for (double& v : R2.m) v = -v;
    double t[3] = {U.m[2], U.m[5], U.m[8]};
    const double nt = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (double& v : t) v /= nt;
    out.clear();
    out.push_back({R1, {t[0], t[1], t[2]}}); out.push_back({R2, {t[0], t[1], t[2]}});
    out.push_back({R1, {-t[0], -t[1], -t[2]}}); out.push_back({R2, {-t[0], -t[1], -t[2]}});
}

// Faugeras & Lustman, "Motion and structure from motion in a piecewise planar environment" (1988): 8 motion hypotheses
bool hypotheses_from_homography(const M3& H21, const double* K, std::vector<Hypothesis>& out)
{
    const M3 Km{{K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1}};
    const M3 A = mul(mul(inverse(Km), H21), Km);
    M3 U, V; double w[3];
    svd3(A, U, w, V);
    const double s = det(U) * det(V);
    const double d1 = w[0], d2 = w[1], d3 = w[2];
    out.clear();
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return false;
    const double aux1 = std::sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = std::sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const double x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
    {   // d' = d2
        const double aux_s = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
        const double ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
        const double st[4] = {aux_s, -aux_s, -aux_s, aux_s};
        for (int i = 0; i < 4; ++i) {
            const M3 Rp{{ct, 0, -st[i], 0, 1, 0, st[i], 0, ct}};
            M3 R = mul(mul(U, Rp), transpose(V));
            for (double& v : R.m) v *= s;
            const double tp[3] = {x1[i] * (d1 - d3), 0, -x3[i] * (d1 - d3)};
            double t[3];
            for (int r = 0; r < 3; ++r) t[r] = U.m[r * 3] * tp[0] + U.m[r * 3 + 1] * tp[1] + U.m[r * 3 + 2] * tp[2];
            const double nt = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
            out.push_back({R, {t[0] / nt, t[1] / nt, t[2] / nt}});
        }
    }
    {   // d' = -d2
        const double aux_s = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
        const double cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
        const double sp[4] = {aux_s, -aux_s, -aux_s, aux_s};
        for (int i = 0; i < 4; ++i) {
            const M3 Rp{{cp, 0, sp[i], 0, -1, 0, sp[i], 0, -cp}};
            M3 R = mul(mul(U, Rp), transpose(V));
            for (double& v : R.m) v *= s;
            const double tp[3] = {x1[i] * (d1 + d3), 0, x3[i] * (d1 + d3)};
            double t[3];
            for (int r = 0; r < 3; ++r) t[r] = U.m[r * 3] * tp[0] + U.m[r * 3 + 1] * tp[1] + U.m[r * 3 + 2] * tp[2];
            const double nt = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
            out.push_back({R, {t[0] / nt, t[1] / nt, t[2] / nt}});
        }
    }
    return true;
}

}  // namespace

// the shared solver (csrc/jacobi_math.h) on a copy of A, its columns read through the order it returns
void sym_eigen_jacobi(const double* A, int n, double* eigval, double* eigvec)
{
    std::vector<double> a(A, A + n * n), v((size_t)n * n);
    std::vector<int> order(n);
    lpslam_jacobi::jacobi_sweeps<0, 1>(a.data(), v.data(), 1, 0, 1, n);
    if (n <= 16) lpslam_jacobi::jacobi_order<0>(a.data(), 1, order.data(), n);
    else {                                                   // (no caller: beyond 16 elements std::sort is no insertion sort, and equal eigenvalues get the order it gives them)
        for (int i = 0; i < n; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * n + x] < a[(size_t)y * n + y]; });
    }
    for (int c = 0; c < n; ++c) {
        eigval[c] = a[(size_t)order[c] * n + order[c]];
        for (int r = 0; r < n; ++r) eigvec[(size_t)r * n + c] = v[(size_t)r * n + order[c]];
    }
}

void homography_from_matches(const double* x1, const double* x2, int n, double* H)
{
    double ws[lpslam_tv::kWorkspace];
    lpslam_tv::homography_from_matches<0>(x1, x2, n, ws, 1, H);
}

void fundamental_from_matches(const double* x1, const double* x2, int n, double* F)
{
    double ws[lpslam_tv::kWorkspace];
    lpslam_tv::fundamental_from_matches<0>(x1, x2, n, ws, 1, F);
}

bool triangulate_point(const double* P1, const double* P2, const double* x1, const double* x2, double* X)
{
    return lpslam_tri::triangulate_linear(P1, P2, x1[0], x1[1], x2[0], x2[1], X);
}

namespace {

// the matches of one pair of views, Hartley-normalised: what steps 1 and 2 work on
struct Normalised { std::vector<double> n1, n2; M3 T1, T2inv, T2t; };

void normalise_pair(const std::vector<double>& p1, const std::vector<double>& p2, Normalised& nm)
{
    M3 T2;
    normalize_points(p1, nm.n1, nm.T1);
    normalize_points(p2, nm.n2, T2);
    nm.T2inv = inverse(T2); nm.T2t = transpose(T2);
}

// ---- step 1: the RANSAC loop.  The same 8-match samples serve both models (ORB-SLAM draws them once); sampling without replacement
void ransac_loop(const Normalised& nm, const double* p1, const double* p2, size_t n, double sigma, int iterations, uint32_t seed, TwoViewModels& out)
{
    out = TwoViewModels();
    out.inl_h.assign(n, 0); out.inl_f.assign(n, 0);
    if (n < 8 || iterations < 1) return;
    std::vector<int> avail(n);
    std::vector<int32_t> table((size_t)lpslam_tv::kSample * (size_t)iterations);
    lpslam_ransac::sample_table<lpslam_tv::kSample>((int)n, iterations, seed, table.data(), avail.data());
    std::vector<uint8_t> inl;
    double best_h = -1, best_f = -1;
    for (int it = 0; it < iterations; ++it) {
        double s1[16], s2[16], ws[lpslam_tv::kWorkspace];
        for (int k = 0; k < 8; ++k) {
            const size_t idx = (size_t)table[(size_t)8 * it + k];
            s1[2 * k] = nm.n1[2 * idx]; s1[2 * k + 1] = nm.n1[2 * idx + 1]; s2[2 * k] = nm.n2[2 * idx]; s2[2 * k + 1] = nm.n2[2 * idx + 1];
        }
        M3 Hn, Fn;
        lpslam_tv::homography_from_matches<8>(s1, s2, 8, ws, 1, Hn.m);
        lpslam_tv::fundamental_from_matches<8>(s1, s2, 8, ws, 1, Fn.m);
        const M3 H21 = mul(mul(nm.T2inv, Hn), nm.T1);
        const M3 F21 = mul(mul(nm.T2t, Fn), nm.T1);
        if (std::fabs(det(H21)) > 1e-300) {
            const double sh = check_homography(H21, inverse(H21), p1, p2, n, sigma, inl);
            if (sh > best_h) { best_h = sh; out.it_h = it; std::memcpy(out.H, H21.m, sizeof(out.H)); out.inl_h = inl; }
        }
        const double sf = check_fundamental(F21, p1, p2, n, sigma, inl);
        if (sf > best_f) { best_f = sf; out.it_f = it; std::memcpy(out.F, F21.m, sizeof(out.F)); out.inl_f = inl; }
    }
    out.score_h = out.it_h >= 0 ? best_h : 0.0; out.score_f = out.it_f >= 0 ? best_f : 0.0;
}

// step 1 through the caller's function; false: it failed (nothing of `out` is to be used)
bool ransac_step(TwoViewSteps& st, const double* p1, const double* p2, size_t n, double sigma, int iterations, uint32_t seed, TwoViewModels& out)
{
    const int32_t offsets[2] = {0, (int32_t)n};
    int32_t best[2] = {-1, -1};
    double score[2] = {0, 0}, model[18] = {0};
    out = TwoViewModels();
    out.inl_h.assign(n, 0); out.inl_f.assign(n, 0);
    ++st.calls;
    if (st.ransac(st.ctx, 1, offsets, p1, p2, sigma, iterations, seed, best, score, model, out.inl_h.data(), out.inl_f.data()) != 0) { ++st.failed; return false; }
    out.it_h = best[0]; out.it_f = best[1]; out.score_h = score[0]; out.score_f = score[1];
    std::memcpy(out.H, model, sizeof(out.H)); std::memcpy(out.F, model + 9, sizeof(out.F));
    return true;
}

// ---- step 2: [UPSTREAM] find_via_ransac(..., recompute = true): the best model of each kind is estimated again from all its inliers
// (normalised coordinates) and its inliers and score are taken from that estimate; then the model choice by the score ratio.
// false: neither model has a score.  best_H / best_F / the flags of `w` are updated in place.
bool refit_and_choose(const Normalised& nm, const double* p1, const double* p2, size_t n, double sigma, TwoViewModels& w, TwoViewResult& out, bool& use_h)
{
    double best_h = w.it_h >= 0 ? w.score_h : -1, best_f = w.it_f >= 0 ? w.score_f : -1;
    M3 best_H, best_F;
    std::memcpy(best_H.m, w.H, sizeof(w.H)); std::memcpy(best_F.m, w.F, sizeof(w.F));
    std::vector<uint8_t> inl;
    auto gather = [&](const std::vector<uint8_t>& mask, std::vector<double>& a, std::vector<double>& b) {
        a.clear(); b.clear();
        for (size_t i = 0; i < n; ++i) if (mask[i]) { a.push_back(nm.n1[2 * i]); a.push_back(nm.n1[2 * i + 1]); b.push_back(nm.n2[2 * i]); b.push_back(nm.n2[2 * i + 1]); }
    };
    std::vector<double> ga, gb;
    if (best_h >= 0) {
        gather(w.inl_h, ga, gb);
        if (ga.size() >= 16) {
            M3 Hn; homography_from_matches(ga.data(), gb.data(), (int)(ga.size() / 2), Hn.m);
            const M3 H21 = mul(mul(nm.T2inv, Hn), nm.T1);
            if (std::fabs(det(H21)) > 1e-300) { best_h = check_homography(H21, inverse(H21), p1, p2, n, sigma, inl); best_H = H21; w.inl_h = inl; }
        }
    }
    if (best_f >= 0) {
        gather(w.inl_f, ga, gb);
        if (ga.size() >= 16) {
            M3 Fn; fundamental_from_matches(ga.data(), gb.data(), (int)(ga.size() / 2), Fn.m);
            const M3 F21 = mul(mul(nm.T2t, Fn), nm.T1);
            best_f = check_fundamental(F21, p1, p2, n, sigma, inl); best_F = F21; w.inl_f = inl;
        }
    }
    out.score_h = std::max(best_h, 0.0); out.score_f = std::max(best_f, 0.0);
    std::memcpy(out.H, best_H.m, sizeof(out.H)); std::memcpy(out.F, best_F.m, sizeof(out.F));
    std::memcpy(w.H, best_H.m, sizeof(w.H)); std::memcpy(w.F, best_F.m, sizeof(w.F));
    if (out.score_h + out.score_f <= 0) return false;
    use_h = out.score_h / (out.score_h + out.score_f) > 0.40;
    return true;
}

}  // namespace

void two_view_ransac(const double* p1, const double* p2, int n, double sigma, int iterations, uint32_t seed, TwoViewModels& out)
{
    const size_t m = (size_t)std::max(n, 0);
    if (m < 8) { out = TwoViewModels(); out.inl_h.assign(m, 0); out.inl_f.assign(m, 0); return; }
    const std::vector<double> a(p1, p1 + 2 * m), b(p2, p2 + 2 * m);
    Normalised nm;
    normalise_pair(a, b, nm);
    ransac_loop(nm, p1, p2, m, sigma, iterations, seed, out);
}

void two_view_check_poses(int n_hyp, const double* R, const double* t, const double* K4, int n, const double* p1, const double* p2,
                          const uint8_t* inlier, double th2, double* X, double* cosp, uint8_t* code)
{
    for (int h = 0; h < n_hyp; ++h) {
        lpslam_tv::PoseSetup ps;
        lpslam_tv::pose_setup(R + 9 * h, t + 3 * h, K4, ps);
        for (int i = 0; i < n; ++i) {
            const size_t o = (size_t)h * (size_t)n + (size_t)i;
            double x[3] = {0, 0, 0}, c = 0;
            const int k = inlier[i] ? lpslam_tv::pose_point(ps, R + 9 * h, t + 3 * h, K4, p1 + 2 * i, p2 + 2 * i, th2, x, &c) : lpslam_tv::kPoseRejected;
            code[o] = (uint8_t)k;
            cosp[o] = k ? c : 0.0;
            for (int a = 0; a < 3; ++a) X[3 * o + a] = k ? x[a] : std::numeric_limits<double>::quiet_NaN();
        }
    }
}

bool two_view_initialize(const double* K, const float* kp_ref, const float* kp_cur, const int32_t* matches, int n_matches,
                         const TwoViewParams& prm, TwoViewResult& out, TwoViewSteps* steps)
{
    out = TwoViewResult();
    out.inlier.assign((size_t)std::max(n_matches, 0), 0);
    out.triangulated.assign((size_t)std::max(n_matches, 0), 0);
    out.points.assign(3 * (size_t)std::max(n_matches, 0), std::numeric_limits<double>::quiet_NaN());
    if (n_matches < 8) return false;
    const size_t n = (size_t)n_matches;
    std::vector<double> p1(2 * n), p2(2 * n);
    for (size_t i = 0; i < n; ++i) {
        p1[2 * i] = kp_ref[2 * matches[2 * i]]; p1[2 * i + 1] = kp_ref[2 * matches[2 * i] + 1];
        p2[2 * i] = kp_cur[2 * matches[2 * i + 1]]; p2[2 * i + 1] = kp_cur[2 * matches[2 * i + 1] + 1];
    }
    Normalised nm;
    normalise_pair(p1, p2, nm);

    // (a caller with steps also gets the seconds each step took)
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](double TwoViewSteps::*field) {
        if (!steps) return;
        const auto t = std::chrono::steady_clock::now();
        steps->*field += std::chrono::duration<double>(t - t_last).count();
        t_last = t;
    };
    // 1. the RANSAC loop, 2. refit and model choice
    TwoViewModels w;
    if (!(steps && steps->ransac && ransac_step(*steps, p1.data(), p2.data(), n, prm.sigma, prm.ransac_iters, prm.seed, w)))
        ransac_loop(nm, p1.data(), p2.data(), n, prm.sigma, prm.ransac_iters, prm.seed, w);
    lap(&TwoViewSteps::t_ransac);
    bool use_h = false;
    const bool chosen = refit_and_choose(nm, p1.data(), p2.data(), n, prm.sigma, w, out, use_h);
    lap(&TwoViewSteps::t_refit);
    if (!chosen) return false;
    out.model = use_h ? 0 : 1;
    const std::vector<uint8_t>& model_inl = use_h ? w.inl_h : w.inl_f;
    out.inlier = model_inl;
    out.n_inliers = (int)std::count(model_inl.begin(), model_inl.end(), (uint8_t)1);

    // 3. the decomposition
    M3 best_H, best_F;
    std::memcpy(best_H.m, w.H, sizeof(w.H)); std::memcpy(best_F.m, w.F, sizeof(w.F));
    std::vector<Hypothesis> hyps;
    if (use_h) { if (!hypotheses_from_homography(best_H, K, hyps)) return false; }
    else hypotheses_from_fundamental(best_F, K, hyps);

    lap(&TwoViewSteps::t_decompose);
    // 4. the pose check of every hypothesis, then the acceptance rules
    const double th2 = prm.reproj_err_thr * prm.sigma * prm.sigma;       // ORB-SLAM: 4 sigma^2
    const size_t np = hyps.size();
    std::vector<double> Rs(9 * np), ts(3 * np), X(3 * np * n), cosp(np * n);
    std::vector<uint8_t> code(np * n);
    for (size_t i = 0; i < np; ++i) { std::memcpy(&Rs[9 * i], hyps[i].R.m, 9 * sizeof(double)); std::memcpy(&ts[3 * i], hyps[i].t, 3 * sizeof(double)); }
    bool checked = false;
    if (steps && steps->check_poses && np > 0) {
        ++steps->calls;
        checked = steps->check_poses(steps->ctx, (int32_t)np, Rs.data(), ts.data(), K, (int32_t)n, p1.data(), p2.data(), model_inl.data(), th2, X.data(), cosp.data(), code.data()) == 0;
        if (!checked) ++steps->failed;
    }
    if (!checked) two_view_check_poses((int)np, Rs.data(), ts.data(), K, (int)n, p1.data(), p2.data(), model_inl.data(), th2, X.data(), cosp.data(), code.data());
    int best_good = 0, second_good = 0, best_i = -1;
    double best_parallax = 0;
    std::vector<double> pts, best_pts;
    std::vector<uint8_t> good, best_goodmask;
    for (size_t i = 0; i < np; ++i) {
        double parallax = 0;
        const int ng = pose_tally(&X[3 * i * n], &cosp[i * n], &code[i * n], n, pts, good, parallax);
        if (ng > best_good) { second_good = best_good; best_good = ng; best_i = (int)i; best_parallax = parallax; best_pts = pts; best_goodmask = good; }
        else if (ng > second_good) second_good = ng;
    }
    out.n_valid = best_good; out.parallax_deg = best_parallax;
    lap(&TwoViewSteps::t_pose);
    // one clear winner with enough plausible points and enough parallax ([UPSTREAM] initialize::base::find_most_plausible_pose)
    const int min_valid = std::max(prm.min_triangulated, (int)(0.9 * out.n_inliers));
    if (best_i < 0 || best_good < min_valid) return false;
    if ((double)second_good > 0.8 * (double)best_good) return false;
    if (best_parallax < prm.parallax_deg_thr) return false;
    std::memcpy(out.R, hyps[(size_t)best_i].R.m, sizeof(out.R));
    std::memcpy(out.t, hyps[(size_t)best_i].t, sizeof(out.t));
    out.points = best_pts; out.triangulated = best_goodmask;
    out.ok = true;
    return true;
}


bool horn_absolute_orientation(const double* x1, const double* x2, int n, bool fix_scale, double* R, double* t, double* s_out)
{
    return lpslam_epnp::horn(x1, x2, n, fix_scale, R, t, s_out);
}

int sim3_solve_ransac(const double* p1c, const double* p2c, const double* obs1, const double* obs2, const double* inv_sigma2_1, const double* inv_sigma2_2,
                      int n, const double* cam1, const double* cam2, bool fix_scale, int iterations, uint32_t seed, double* s12, uint8_t* inlier)
{
    if (n < 3) return 0;
    uint32_t rng = seed ? seed : 1u;
    std::vector<int> avail((size_t)n);
    std::vector<uint8_t> cur((size_t)n);
    int best = 0;
    for (int it = 0; it < iterations; ++it) {
        int32_t idx[3];
        lpslam_ransac::draw<3>(rng, n, avail.data(), idx);
        double a1[9], a2[9], R[9], t[3], sc;
        for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) { a1[3 * k + a] = p1c[3 * idx[k] + a]; a2[3 * k + a] = p2c[3 * idx[k] + a]; }
        if (!lpslam_epnp::horn<3>(a1, a2, 3, fix_scale, R, t, &sc)) continue;                 // (the instance the device kernel runs)
        // the rule per pair (2 -> 1: x1 = s R x2 + t;  1 -> 2: x2 = R^T (x1 - t) / s) is csrc/sim3_math.h, the text the device kernels run
        const int count = lpslam_sim3::sim3_score(R, t, sc, p1c, p2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, n, cam1, cam2, cur.data());
        if (count > best) {
            best = count;
            double q[4];
            rotToQuat(R, q);
            s12[0] = q[0]; s12[1] = q[1]; s12[2] = q[2]; s12[3] = q[3]; s12[4] = t[0]; s12[5] = t[1]; s12[6] = t[2]; s12[7] = sc;
            if (inlier) std::copy(cur.begin(), cur.end(), inlier);
        }
    }
    return best;
}


// ---- [UPSTREAM] solve::pnp_solver (relocalisation without a pose prior): the algorithm and its arithmetic are csrc/epnp_math.h ------------
bool epnp_solve(const double* pw, const double* uv, int n, const double* cam, double* R, double* t)
{
    if (n < 4) return false;
    std::vector<double> scratch((size_t)7 * n);              // the alphas (4 n), the camera-frame landmarks (3 n)
    double ws[lpslam_epnp::kWorkspace];
    return lpslam_epnp::epnp(pw, uv, n, cam, scratch.data(), scratch.data() + (size_t)4 * n, ws, 1, R, t);
}

int pnp_solve_ransac(const double* pw, const double* obs, const double* inv_sigma2, int n, const double* cam, int iterations, uint32_t seed, double* pose7, uint8_t* inlier)
{
    namespace ep = lpslam_epnp;
    for (int i = 0; i < n; ++i) inlier[i] = 0;
    if (n < 4) return 0;
    std::vector<int> avail((size_t)n);
    std::vector<int32_t> table((size_t)4 * (size_t)std::max(iterations, 0));
    lpslam_ransac::sample_table<4>(n, iterations, seed, table.data(), avail.data());
    std::vector<uint8_t> cur((size_t)n);
    int best = 0;
    double bestR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, bestT[3] = {0, 0, 0};
    for (int it = 0; it < iterations; ++it) {
        double R[9], t[3];
        if (!ep::pnp_solve_sample(pw, obs, table.data() + (size_t)4 * it, cam, R, t)) continue;
        const int count = ep::pnp_score(R, t, cam, pw, obs, inv_sigma2, n, cur.data());
        if (count > best) {
            best = count;
            for (int i = 0; i < n; ++i) inlier[i] = cur[(size_t)i];
            for (int k = 0; k < 9; ++k) bestR[k] = R[k];
            for (int k = 0; k < 3; ++k) bestT[k] = t[k];
        }
    }
    if (best < 4) { for (int i = 0; i < n; ++i) inlier[i] = 0; return 0; }
    std::vector<double> scratch((size_t)12 * n);
    best = ep::pnp_refit(pw, obs, inv_sigma2, n, cam, best, inlier, bestR, bestT, scratch.data(), cur.data());
    double q[4];
    rotToQuat(bestR, q);
    for (int k = 0; k < 4; ++k) pose7[k] = q[k];
    for (int k = 0; k < 3; ++k) pose7[4 + k] = bestT[k];
    return best;
}

}  // namespace LpSlam

// ---- C shim for the ctypes tests ------------------------------------------------------------------------------------------
extern "C" {
__attribute__((visibility("default"))) int lpslam_two_view_initialize(const double* K, const float* kp_ref, const float* kp_cur, const int32_t* matches,
                                                                        int n_matches, double sigma, int ransac_iters, uint32_t seed,
                                                                        double* R9, double* t3, double* H9, double* F9, double* scores2, double* parallax_deg,
                                                                        int32_t* model, uint8_t* inlier, uint8_t* triangulated, double* points3)
{
    LpSlam::TwoViewParams prm;
    prm.sigma = sigma; prm.ransac_iters = ransac_iters; prm.seed = seed;
    LpSlam::TwoViewResult res;
    const bool ok = LpSlam::two_view_initialize(K, kp_ref, kp_cur, matches, n_matches, prm, res);
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
    return ok ? 1 : 0;
}

__attribute__((visibility("default"))) void lpslam_sym_eigen(const double* A, int n, double* eigval, double* eigvec) { LpSlam::sym_eigen_jacobi(A, n, eigval, eigvec); }
}

extern "C" __attribute__((visibility("default"))) int lpslam_sim3_solve_ransac(const double* p1c, const double* p2c, const double* obs1, const double* obs2,
                                                                                const double* is1, const double* is2, int n, const double* cam1, const double* cam2,
                                                                                int fix_scale, int iterations, uint32_t seed, double* s12, uint8_t* inlier)
{
    return LpSlam::sim3_solve_ransac(p1c, p2c, obs1, obs2, is1, is2, n, cam1, cam2, fix_scale != 0, iterations, seed, s12, inlier);
}

extern "C" __attribute__((visibility("default"))) int lpslam_epnp_solve(const double* pw, const double* uv, int n, const double* cam, double* R9, double* t3)
{
    return LpSlam::epnp_solve(pw, uv, n, cam, R9, t3) ? 1 : 0;
}

extern "C" __attribute__((visibility("default"))) int lpslam_pnp_solve_ransac(const double* pw, const double* obs, const double* inv_sigma2, int n, const double* cam,
                                                                             int iterations, uint32_t seed, double* pose7, uint8_t* inlier)
{
    return LpSlam::pnp_solve_ransac(pw, obs, inv_sigma2, n, cam, iterations, seed, pose7, inlier);
}
