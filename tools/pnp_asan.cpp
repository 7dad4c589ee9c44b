// pnp_asan.cpp -- stand-alone driver of the batched PnP RANSAC's host code for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ilpslam_amd/host \
//       tools/pnp_asan.cpp lpslam_amd/host/two_view.cpp lpslam_amd/host/pnp_batch.cpp -o pnp_asan && ./pnp_asan
// It runs the sample table, the fixed-size EPnP and the batch host path over the shapes of tests/test_pnp_cpu.py (n = 4, 5, 37, 300;
// seeds 0 and 0x9E3779B9; 1, 7 and 100 iterations; a batch with an empty set, a set of three and a coplanar set in the middle) and
// checks what the tests check: indices distinct and in range, the fixed-size solve equal to epnp_solve, the batch equal to separate solver calls.
// Then the any-n EPnP of csrc/epnp_math.h at n = 5, 37 and 300 and the shared refit, each with heap scratch of exactly the documented
// size (4 n + 3 n doubles; 12 n doubles and n flags), so that a write past it is seen: equal to epnp_solve, and a refit that returns
// the number of flags it leaves set.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "two_view.h"
#include "../lpslam_amd/csrc/epnp_math.h"

extern "C" {
int lpslam_pnp_sample_table(int n, int iterations, uint32_t seed, int32_t* table);
int lpslam_epnp4_host(const double* p4, const double* u4, const double* cam, double* R9, double* t3);
int lpslam_pnp_ransac_batch_host(int32_t n_sets, const int32_t* offsets, const double* pw, const double* obs, const double* inv_sigma2, const double* cam4,
                                 int32_t iterations, uint32_t seed, double* pose7, int32_t* n_inliers, uint8_t* inlier, int32_t* best_iteration);
}

namespace {
const double kCam[4] = {525.0, 525.0, 320.0, 240.0};
struct Lcg { uint64_t s; double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; } };
struct Set { std::vector<double> pw, obs, w; };

// landmarks 2 .. 10 m in front of a camera turned about y and moved; every third match an outlier; flat: all in the world plane z = 1.5
Set planted(int n, uint64_t seed, bool flat)
{
    Lcg g{seed};
    const double a = 0.2 + 0.6 * g.next(), c = std::cos(a), s = std::sin(a), t[3] = {g.next() - 0.5, g.next() - 0.5, flat ? 4.0 : g.next()};
    Set st;
    for (int i = 0; i < n; ++i) {
        double xc[3], X[3];
        if (flat) {
            X[0] = 4 * g.next() - 2; X[1] = 4 * g.next() - 2; X[2] = 1.5;
            xc[0] = c * X[0] + s * X[2] + t[0]; xc[1] = X[1] + t[1]; xc[2] = -s * X[0] + c * X[2] + t[2];
        } else {
            const double z = 2 + 8 * g.next();
            xc[0] = (20 + 600 * g.next() - kCam[2]) / kCam[0] * z; xc[1] = (20 + 440 * g.next() - kCam[3]) / kCam[1] * z; xc[2] = z;
            const double d[3] = {xc[0] - t[0], xc[1] - t[1], xc[2] - t[2]};
            X[0] = c * d[0] - s * d[2]; X[1] = d[1]; X[2] = s * d[0] + c * d[2];
        }
        double u = kCam[0] * xc[0] / xc[2] + kCam[2] + 0.6 * g.next() - 0.3, v = kCam[1] * xc[1] / xc[2] + kCam[3] + 0.6 * g.next() - 0.3;
        if (!flat && n >= 15 && i % 3 == 2) { u += 40 + 50 * g.next(); v -= 35; }
        st.pw.insert(st.pw.end(), X, X + 3); st.obs.push_back(u); st.obs.push_back(v);
        const double sc = std::pow(1.2, (double)(i % 4));
        st.w.push_back(1.0 / (sc * sc));
    }
    return st;
}

int failures = 0;
void check(bool ok, const char* what, int a, int b) { if (!ok) { ++failures; std::printf("FAILED: %s (%d, %d)\n", what, a, b); } }
}  // namespace

int main()
{
    const uint32_t seeds[2] = {0u, 0x9E3779B9u};
    const int sizes[4] = {4, 5, 37, 300}, iters[3] = {1, 7, 100};
    long solved = 0, tables = 0;
    for (int n : sizes) for (uint32_t seed : seeds) for (int it : iters) {
        std::vector<int32_t> table((size_t)it * 4, -1);
        check(lpslam_pnp_sample_table(n, it, seed, table.data()) == 1, "sample table", n, it);
        ++tables;
        const Set s = planted(n, 17 + (uint64_t)n, false);
        for (int k = 0; k < it; ++k) {
            const int32_t* r = table.data() + 4 * k;
            bool ok = true;
            for (int a = 0; a < 4; ++a) { ok = ok && r[a] >= 0 && r[a] < n; for (int b = 0; b < a; ++b) ok = ok && r[a] != r[b]; }
            check(ok, "sample indices", n, k);
            if (!ok) continue;
            double p4[12], u4[8], R1[9], t1[3], R2[9], t2[3];
            for (int a = 0; a < 4; ++a) { for (int c = 0; c < 3; ++c) p4[3 * a + c] = s.pw[3 * (size_t)r[a] + c]; u4[2 * a] = s.obs[2 * (size_t)r[a]]; u4[2 * a + 1] = s.obs[2 * (size_t)r[a] + 1]; }
            const bool o1 = LpSlam::epnp_solve(p4, u4, 4, kCam, R1, t1), o2 = lpslam_epnp4_host(p4, u4, kCam, R2, t2) != 0;
            check(o1 == o2 && (!o1 || (!std::memcmp(R1, R2, sizeof R1) && !std::memcmp(t1, t2, sizeof t1))), "epnp4 against epnp_solve", n, k);
            solved += o1;
        }
    }
    check(lpslam_pnp_sample_table(3, 10, 1, nullptr) == 0, "sample table of three matches", 3, 10);
    for (int it : iters) {
        const Set parts[6] = {planted(37, 1, false), planted(3, 2, false), planted(40, 3, true), planted(64, 4, false), Set{}, planted(5, 5, false)};
        std::vector<int32_t> off{0};
        Set all;
        for (const Set& p : parts) {
            all.pw.insert(all.pw.end(), p.pw.begin(), p.pw.end()); all.obs.insert(all.obs.end(), p.obs.begin(), p.obs.end()); all.w.insert(all.w.end(), p.w.begin(), p.w.end());
            off.push_back((int32_t)all.w.size());
        }
        std::vector<double> pose(6 * 7);
        std::vector<int32_t> cnt(6), best(6);
        std::vector<uint8_t> fl(all.w.size());
        check(lpslam_pnp_ransac_batch_host(6, off.data(), all.pw.data(), all.obs.data(), all.w.data(), kCam, it, 0x9E3779B9u, pose.data(), cnt.data(), fl.data(), best.data()) == 0, "batch", it, 0);
        for (int i = 0; i < 6; ++i) {
            const Set& p = parts[i];
            const int n = (int)p.w.size();
            double p7[7] = {1, 0, 0, 0, 0, 0, 0};
            std::vector<uint8_t> inl((size_t)n + 1);
            const int want = LpSlam::pnp_solve_ransac(p.pw.data(), p.obs.data(), p.w.data(), n, kCam, it, 0x9E3779B9u, p7, inl.data());
            check(want == cnt[(size_t)i] && !std::memcmp(p7, pose.data() + 7 * i, sizeof p7) && (n == 0 || !std::memcmp(inl.data(), fl.data() + off[(size_t)i], (size_t)n)), "batch set against the solver", it, i);
            check((best[(size_t)i] >= 0) == (want > 0), "winning iteration", it, i);
        }
        check(cnt[1] == 0 && cnt[2] == 0 && cnt[4] == 0, "degenerate sets find nothing", it, 0);
        check(lpslam_pnp_ransac_batch_host(6, off.data(), all.pw.data(), all.obs.data(), all.w.data(), kCam, 0, 1, pose.data(), cnt.data(), fl.data(), nullptr) == 1, "iterations 0 refused", it, 0);
    }
    namespace ep = lpslam_epnp;
    long refits = 0;
    for (int n : {5, 37, 300}) for (uint64_t data = 1; data <= 3; ++data) {
        const Set s = planted(n, 100 * (uint64_t)n + data, false);
        std::vector<double> al((size_t)4 * n), pc((size_t)3 * n), ws((size_t)ep::kWorkspace);
        double R1[9], t1[3], R2[9], t2[3];
        const bool o1 = LpSlam::epnp_solve(s.pw.data(), s.obs.data(), n, kCam, R1, t1);
        const bool o2 = ep::epnp(s.pw.data(), s.obs.data(), n, kCam, al.data(), pc.data(), ws.data(), 1, R2, t2);
        check(o1 && o2 && !std::memcmp(R1, R2, sizeof R1) && !std::memcmp(t1, t2, sizeof t1), "any-n epnp against epnp_solve", n, (int)data);
        if (!o2) continue;
        // the refit from the inliers of that pose (with every third match an outlier from n = 15 on, they are a proper subset)
        std::vector<uint8_t> inl((size_t)n), cur((size_t)n);
        std::vector<double> scratch((size_t)12 * n);
        const int best = ep::pnp_score(R2, t2, kCam, s.pw.data(), s.obs.data(), s.w.data(), n, inl.data());
        const int got = ep::pnp_refit(s.pw.data(), s.obs.data(), s.w.data(), n, kCam, best, inl.data(), R2, t2, scratch.data(), cur.data());
        int set = 0;
        for (uint8_t f : inl) set += f;
        check(got >= best && got == set, "refit count against its flags", n, (int)data);
        ++refits;
    }
    std::printf("pnp_asan: %ld sample tables, %ld four-match solves compared, 3 batches of 6 sets, %ld any-n solves and refits; %d failures\n", tables, solved, refits, failures);
    return failures ? 1 : 0;
}
