// two_view_asan.cpp -- stand-alone driver of the two-view initialiser's host code for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ilpslam_amd/host \
//       tools/two_view_asan.cpp lpslam_amd/host/two_view.cpp lpslam_amd/host/two_view_batch.cpp -o two_view_asan && ./two_view_asan
// It runs the sample table, the estimators at eight and the batch host path over the shapes of tests/test_two_view_batch_cpu.py
// (n = 8, 9, 37, 300; seeds 0 and 0x9E3779B9; 1 and 100 iterations; a batch with a set of seven, an empty set and a one-point set in
// the middle), the pose check (1, 4 and 8 hypotheses; n = 1, 63, 64, 65, 300) with output arrays of exactly the documented size, and
// two_view_initialize with and without the steps handed in -- and checks what the tests check: indices distinct and in range, the
// fixed-size estimators equal to the run-time ones, the batch equal to separate calls, both forms of the function equal.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "two_view.h"

extern "C" {
int lpslam_two_view_sample_table(int n, int iterations, uint32_t seed, int32_t* table);
void lpslam_two_view_models8_host(const double* x1, const double* x2, double* H9, double* F9);
void lpslam_two_view_models_host(const double* x1, const double* x2, int n, double* H9, double* F9);
int lpslam_two_view_ransac_batch_host(int32_t n_sets, const int32_t* offsets, const double* p1, const double* p2, double sigma, int32_t iterations, uint32_t seed,
                                      int32_t* best_iteration, double* score, double* model, uint8_t* inlier_h, uint8_t* inlier_f);
int lpslam_two_view_check_poses_host(int32_t n_hyp, const double* R, const double* t, const double* K4, int32_t n, const double* p1, const double* p2,
                                     const uint8_t* inlier, double th2, double* X, double* cosp, uint8_t* code);
int lpslam_two_view_initialize(const double* K, const float* kp_ref, const float* kp_cur, const int32_t* matches, int n_matches, double sigma, int ransac_iters, uint32_t seed,
                               double* R9, double* t3, double* H9, double* F9, double* scores2, double* parallax_deg, int32_t* model, uint8_t* inlier, uint8_t* triangulated, double* points3);
int lpslam_two_view_initialize_steps(const double* K, const float* kp_ref, const float* kp_cur, const int32_t* matches, int n_matches, double sigma, int ransac_iters,
                                     uint32_t seed, double* R9, double* t3, double* H9, double* F9, double* scores2, double* parallax_deg, int32_t* model, uint8_t* inlier,
                                     uint8_t* triangulated, double* points3, int32_t* calls2);
}

namespace {
const double kCam[4] = {525.0, 525.0, 320.0, 240.0};
struct Lcg { uint64_t s; double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; } };
struct Set { std::vector<double> p1, p2; };

// points 4 .. 9 m in front of the reference camera (flat: on a tilted plane), seen again after a turn about y and a step; every fourth match wrong
Set planted(int n, uint64_t seed, bool flat)
{
    Lcg g{seed};
    const double a = 0.04 + 0.04 * g.next(), c = std::cos(a), s = std::sin(a), t[3] = {-0.4, 0.05, 0.1};
    Set st;
    for (int i = 0; i < n; ++i) {
        double X[3] = {6 * g.next() - 3, 4 * g.next() - 2, 4 + 5 * g.next()};
        if (flat) X[2] = 6.0 + 0.6 * X[0] - 0.4 * X[1];
        const double Y[3] = {c * X[0] + s * X[2] + t[0], X[1] + t[1], -s * X[0] + c * X[2] + t[2]};
        double u2 = kCam[0] * Y[0] / Y[2] + kCam[2] + 0.6 * g.next() - 0.3, v2 = kCam[1] * Y[1] / Y[2] + kCam[3] + 0.6 * g.next() - 0.3;
        if (n >= 15 && i % 4 == 3) { u2 = 640 * g.next(); v2 = 480 * g.next(); }
        st.p1.push_back((double)(float)(kCam[0] * X[0] / X[2] + kCam[2] + 0.6 * g.next() - 0.3)); st.p1.push_back((double)(float)(kCam[1] * X[1] / X[2] + kCam[3] + 0.6 * g.next() - 0.3));
        st.p2.push_back((double)(float)u2); st.p2.push_back((double)(float)v2);
    }
    return st;
}

int failures = 0;
void check(bool ok, const char* what, int a, int b) { if (!ok) { ++failures; std::printf("FAILED: %s (%d, %d)\n", what, a, b); } }

struct Init { int ok; double R[9], t[3], H[9], F[9], sc[2], par; int32_t model; std::vector<uint8_t> inl, tri; std::vector<double> pts; };
Init initialize(const Set& s, int iters, bool steps, int32_t* calls)
{
    const int n = (int)s.p1.size() / 2;
    std::vector<float> a(s.p1.begin(), s.p1.end()), b(s.p2.begin(), s.p2.end());
    std::vector<int32_t> m;
    for (int i = 0; i < n; ++i) { m.push_back(i); m.push_back(i); }
    Init r{};
    r.inl.assign((size_t)n, 0); r.tri.assign((size_t)n, 0); r.pts.assign(3 * (size_t)n, 0.0);
    r.ok = steps ? lpslam_two_view_initialize_steps(kCam, a.data(), b.data(), m.data(), n, 1.0, iters, 12345, r.R, r.t, r.H, r.F, r.sc, &r.par, &r.model, r.inl.data(), r.tri.data(), r.pts.data(), calls)
                 : lpslam_two_view_initialize(kCam, a.data(), b.data(), m.data(), n, 1.0, iters, 12345, r.R, r.t, r.H, r.F, r.sc, &r.par, &r.model, r.inl.data(), r.tri.data(), r.pts.data());
    return r;
}
bool same(const Init& a, const Init& b)
{
    return a.ok == b.ok && !std::memcmp(a.R, b.R, sizeof a.R) && !std::memcmp(a.t, b.t, sizeof a.t) && !std::memcmp(a.H, b.H, sizeof a.H) && !std::memcmp(a.F, b.F, sizeof a.F) &&
           !std::memcmp(a.sc, b.sc, sizeof a.sc) && !std::memcmp(&a.par, &b.par, 8) && a.model == b.model && a.inl == b.inl && a.tri == b.tri &&
           !std::memcmp(a.pts.data(), b.pts.data(), a.pts.size() * 8);
}
}  // namespace

int main()
{
    const uint32_t seeds[2] = {0u, 0x9E3779B9u};
    const int sizes[4] = {8, 9, 37, 300}, iters[2] = {1, 100};
    long tables = 0, eights = 0, inits = 0, initialised = 0;
    for (int n : sizes) for (uint32_t seed : seeds) for (int it : iters) {
        std::vector<int32_t> table((size_t)it * 8, -1);
        check(lpslam_two_view_sample_table(n, it, seed, table.data()) == 1, "sample table", n, it);
        ++tables;
        const Set s = planted(n, 17 + (uint64_t)n, false);
        for (int k = 0; k < it; ++k) {
            const int32_t* r = table.data() + 8 * k;
            bool ok = true;
            for (int a = 0; a < 8; ++a) { ok = ok && r[a] >= 0 && r[a] < n; for (int b = 0; b < a; ++b) ok = ok && r[a] != r[b]; }
            check(ok, "sample indices", n, k);
            if (!ok) continue;
            double x1[16], x2[16], H8[9], F8[9], H[9], F[9];
            for (int a = 0; a < 8; ++a) for (int c = 0; c < 2; ++c) { x1[2 * a + c] = (s.p1[2 * (size_t)r[a] + c] - 320.0) / 100.0; x2[2 * a + c] = (s.p2[2 * (size_t)r[a] + c] - 320.0) / 100.0; }
            lpslam_two_view_models8_host(x1, x2, H8, F8);
            lpslam_two_view_models_host(x1, x2, 8, H, F);
            check(!std::memcmp(H8, H, sizeof H) && !std::memcmp(F8, F, sizeof F), "estimators at eight against the run-time ones", n, k);
            ++eights;
        }
    }
    check(lpslam_two_view_sample_table(7, 10, 1, nullptr) == 0, "sample table of seven matches", 7, 10);
    for (int it : iters) {
        Set one; for (int i = 0; i < 20; ++i) { one.p1.push_back(100); one.p1.push_back(120); one.p2.push_back(130); one.p2.push_back(90); }
        const Set parts[6] = {planted(37, 1, false), planted(7, 2, false), Set{}, one, planted(65, 4, true), planted(9, 5, false)};
        std::vector<int32_t> off{0};
        Set all;
        for (const Set& p : parts) { all.p1.insert(all.p1.end(), p.p1.begin(), p.p1.end()); all.p2.insert(all.p2.end(), p.p2.begin(), p.p2.end()); off.push_back((int32_t)all.p1.size() / 2); }
        std::vector<int32_t> best(12);
        std::vector<double> score(12), model(6 * 18);
        std::vector<uint8_t> fh(all.p1.size() / 2), ff(all.p1.size() / 2);
        check(lpslam_two_view_ransac_batch_host(6, off.data(), all.p1.data(), all.p2.data(), 1.0, it, 0x9E3779B9u, best.data(), score.data(), model.data(), fh.data(), ff.data()) == 0, "batch", it, 0);
        for (int i = 0; i < 6; ++i) {
            const Set& p = parts[i];
            const int n = (int)p.p1.size() / 2;
            LpSlam::TwoViewModels w;
            LpSlam::two_view_ransac(p.p1.data(), p.p2.data(), n, 1.0, it, 0x9E3779B9u, w);
            check(w.it_h == best[2 * (size_t)i] && w.it_f == best[2 * (size_t)i + 1] && !std::memcmp(&w.score_h, &score[2 * (size_t)i], 8) && !std::memcmp(&w.score_f, &score[2 * (size_t)i + 1], 8) &&
                  !std::memcmp(w.H, &model[18 * (size_t)i], 72) && !std::memcmp(w.F, &model[18 * (size_t)i + 9], 72) &&
                  (n == 0 || (!std::memcmp(w.inl_h.data(), fh.data() + off[(size_t)i], (size_t)n) && !std::memcmp(w.inl_f.data(), ff.data() + off[(size_t)i], (size_t)n))), "batch set against a call of its own", it, i);
        }
        check(best[2] == -1 && best[3] == -1 && best[4] == -1 && best[5] == -1 && best[6] == -1 && best[7] == -1, "sets too small or degenerate answer none", it, 0);
        check(best[0] >= 0 && best[9] >= 0, "sets with a motion have winners", it, 0);
        check(lpslam_two_view_ransac_batch_host(6, off.data(), all.p1.data(), all.p2.data(), 1.0, 0, 1, best.data(), score.data(), model.data(), fh.data(), ff.data()) == 1, "iterations 0 refused", it, 0);
        check(lpslam_two_view_ransac_batch_host(6, off.data(), all.p1.data(), all.p2.data(), 0.0, it, 1, best.data(), score.data(), model.data(), fh.data(), ff.data()) == 1, "sigma 0 refused", it, 0);
    }
    long poses = 0;
    for (int P : {1, 4, 8}) for (int n : {1, 63, 64, 65, 300}) {
        const Set s = planted(n, 7, false);
        std::vector<double> R((size_t)9 * P), t((size_t)3 * P), X((size_t)3 * P * n), cosp((size_t)P * n);
        std::vector<uint8_t> code((size_t)P * n), fl((size_t)n);
        for (int h = 0; h < P; ++h) {
            const double a = 0.06 + 0.03 * h, c = std::cos(a), sn = std::sin(a);
            const double Rh[9] = {c, 0, sn, 0, 1, 0, -sn, 0, c};
            std::memcpy(&R[9 * (size_t)h], Rh, sizeof Rh);
            t[3 * (size_t)h] = h == 1 ? 0.96 : -0.96; t[3 * (size_t)h + 1] = 0.12; t[3 * (size_t)h + 2] = 0.24;
        }
        for (int i = 0; i < n; ++i) fl[(size_t)i] = (uint8_t)(i % 3 != 1);
        check(lpslam_two_view_check_poses_host(P, R.data(), t.data(), kCam, n, s.p1.data(), s.p2.data(), fl.data(), 4.0, X.data(), cosp.data(), code.data()) == 0, "pose check", P, n);
        bool ok = true;
        for (size_t k = 0; k < code.size(); ++k) ok = ok && code[k] <= 2 && (code[k] != 0 || (std::isnan(X[3 * k]) && cosp[k] == 0.0)) && (fl[k % (size_t)n] || code[k] == 0);
        check(ok, "codes, NaN points and flags", P, n);
        ++poses;
    }
    check(lpslam_two_view_check_poses_host(9, nullptr, nullptr, kCam, 0, nullptr, nullptr, nullptr, 4.0, nullptr, nullptr, nullptr) == 1, "nine hypotheses refused", 9, 0);
    for (int n : {7, 8, 37, 300}) for (int flat = 0; flat < 2; ++flat) for (int it : iters) {
        const Set s = planted(n, 300 + (uint64_t)n, flat != 0);
        int32_t calls[2] = {0, 0};
        const Init a = initialize(s, it, false, nullptr), b = initialize(s, it, true, calls);
        check(same(a, b), "the function with the steps handed in", n, it);
        check(calls[1] == 0 && (n >= 8 ? calls[0] >= 1 : calls[0] == 0), "step calls", calls[0], calls[1]);
        ++inits; initialised += a.ok;
    }
    std::printf("two_view_asan: %ld sample tables, %ld eights compared, 2 batches of 6 sets, %ld pose checks, %ld initialisations (%ld gave a map) in both forms; %d failures\n",
                tables, eights, poses, inits, initialised, failures);
    return failures ? 1 : 0;
}
