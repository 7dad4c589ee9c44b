// sim3_ransac_asan.cpp -- stand-alone driver of the batched Sim3 RANSAC's host code for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ilpslam_amd/host \
//       tools/sim3_ransac_asan.cpp lpslam_amd/host/two_view.cpp lpslam_amd/host/sim3_batch.cpp -o sim3_ransac_asan && ./sim3_ransac_asan
// It runs the sample table and the batch host path over the shapes of tests/test_sim3_batch_cpu.py (n = 3, 4, 37, 300; seeds 0 and
// 0x9E3779B9; 1 and 200 iterations; both scale settings; a batch with a set of two pairs, an empty set and a set whose pairs all
// coincide in the middle, also from a pair_start that does not begin at 0) and checks what the tests check: indices distinct and in
// range, the batch equal to separate solver calls, what a set without a result answers.  Every array has exactly the documented size,
// so that a read or write past it is seen.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "two_view.h"
#include "../include/lpslam_hip.h"

extern "C" {
int lpslam_sim3_sample_table(int n, int iterations, uint32_t seed, int32_t* table);
int lpslam_sim3_ransac_batch_host(int32_t n_sets, const lpslam_hip_sim3_pair* pairs, const int32_t* pair_start, const double* cam1, const double* cam2,
                                  int32_t fix_scale, int32_t iterations, uint32_t seed, double* s12, int32_t* n_inliers, uint8_t* inlier, int32_t* best_iteration);
}

namespace {
const double kCam[4] = {520.0, 515.0, 318.5, 243.25};
struct Lcg { uint64_t s; double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; } };
typedef std::vector<lpslam_hip_sim3_pair> Set;

// landmarks 5 .. 20 m in front of camera 2, camera 1 turned about y, moved and scaled; from n = 15 on every third match is wrong;
// same: every pair is the first one
Set planted(int n, uint64_t seed, bool same = false)
{
    Lcg g{seed};
    const double a = 0.05 + 0.2 * g.next(), c = std::cos(a), s = std::sin(a), t[3] = {g.next() - 0.5, g.next() - 0.5, g.next() - 0.5}, sc = 1.0 + 0.1 * g.next();
    Set st;
    for (int i = 0; i < n; ++i) {
        lpslam_hip_sim3_pair p{};
        if (same && i > 0) { st.push_back(st[0]); continue; }
        p.p2c[0] = 10 * g.next() - 5; p.p2c[1] = 6 * g.next() - 3; p.p2c[2] = 5 + 15 * g.next();
        p.p1c[0] = sc * (c * p.p2c[0] + s * p.p2c[2]) + t[0]; p.p1c[1] = sc * p.p2c[1] + t[1]; p.p1c[2] = sc * (-s * p.p2c[0] + c * p.p2c[2]) + t[2];
        // (coordinates in 64ths: three times such a number is exact, so the mean of three equal points is the point and Horn sees zeros)
        if (same) for (int a = 0; a < 3; ++a) { p.p1c[a] = std::floor(p.p1c[a] * 64) / 64; p.p2c[a] = std::floor(p.p2c[a] * 64) / 64; }
        p.obs1[0] = kCam[0] * p.p1c[0] / p.p1c[2] + kCam[2] + 0.6 * g.next() - 0.3; p.obs1[1] = kCam[1] * p.p1c[1] / p.p1c[2] + kCam[3] + 0.6 * g.next() - 0.3;
        p.obs2[0] = kCam[0] * p.p2c[0] / p.p2c[2] + kCam[2] + 0.6 * g.next() - 0.3; p.obs2[1] = kCam[1] * p.p2c[1] / p.p2c[2] + kCam[3] + 0.6 * g.next() - 0.3;
        if (n >= 15 && i % 3 == 2) { p.obs1[0] += 40 + 50 * g.next(); p.obs1[1] -= 35; }
        const double l1 = std::pow(1.2, (double)(i % 4)), l2 = std::pow(1.2, (double)(i % 3));
        p.inv_sigma2_1 = 1.0 / (l1 * l1); p.inv_sigma2_2 = 1.0 / (l2 * l2);
        st.push_back(p);
    }
    return st;
}

int failures = 0;
void check(bool ok, const char* what, int a, int b) { if (!ok) { ++failures; std::printf("FAILED: %s (%d, %d)\n", what, a, b); } }

// sim3_solve_ransac on one set from arrays of exactly n entries; what the batch form answers when it finds nothing
int single(const Set& p, int fix_scale, int it, uint32_t seed, double* s12, std::vector<uint8_t>& inl)
{
    const size_t n = p.size();
    std::vector<double> p1(3 * n), p2(3 * n), o1(2 * n), o2(2 * n), w1(n), w2(n);
    for (size_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) { p1[3 * i + a] = p[i].p1c[a]; p2[3 * i + a] = p[i].p2c[a]; }
        for (int a = 0; a < 2; ++a) { o1[2 * i + a] = p[i].obs1[a]; o2[2 * i + a] = p[i].obs2[a]; }
        w1[i] = p[i].inv_sigma2_1; w2[i] = p[i].inv_sigma2_2;
    }
    inl.assign(n, 0);
    const double none[8] = {1, 0, 0, 0, 0, 0, 0, 1};
    std::memcpy(s12, none, sizeof none);
    return LpSlam::sim3_solve_ransac(p1.data(), p2.data(), o1.data(), o2.data(), w1.data(), w2.data(), (int)n, kCam, kCam, fix_scale != 0, it, seed, s12, inl.data());
}
}  // namespace

int main()
{
    const uint32_t seeds[2] = {0u, 0x9E3779B9u};
    const int sizes[4] = {3, 4, 37, 300}, iters[2] = {1, 200};
    long tables = 0, sets = 0;
    for (int n : sizes) for (uint32_t seed : seeds) for (int it : iters) {
        std::vector<int32_t> table((size_t)it * 3, -1);
        check(lpslam_sim3_sample_table(n, it, seed, table.data()) == 1, "sample table", n, it);
        ++tables;
        for (int k = 0; k < it; ++k) {
            const int32_t* r = table.data() + 3 * k;
            bool ok = true;
            for (int a = 0; a < 3; ++a) { ok = ok && r[a] >= 0 && r[a] < n; for (int b = 0; b < a; ++b) ok = ok && r[a] != r[b]; }
            check(ok, "sample indices", n, k);
        }
    }
    check(lpslam_sim3_sample_table(2, 10, 1, nullptr) == 0, "sample table of two pairs", 2, 10);
    for (int fix_scale : {0, 1}) for (uint32_t seed : seeds) for (int it : iters) for (int first : {0, 5}) {
        const Set parts[7] = {planted(3, 1), planted(2, 2), planted(4, 3), Set{}, planted(37, 5), planted(8, 6, true), planted(300, 7)};
        std::vector<int32_t> start{first};
        Set all((size_t)first);
        for (const Set& p : parts) { all.insert(all.end(), p.begin(), p.end()); start.push_back((int32_t)all.size()); }
        std::vector<double> s12(7 * 8);
        std::vector<int32_t> cnt(7), best(7);
        std::vector<uint8_t> fl(all.size(), 9);
        check(lpslam_sim3_ransac_batch_host(7, all.data(), start.data(), kCam, kCam, fix_scale, it, seed, s12.data(), cnt.data(), fl.data(), best.data()) == 0, "batch", it, first);
        for (int i = 0; i < 7; ++i) {
            const int n = (int)parts[i].size();
            double want12[8];
            std::vector<uint8_t> inl;
            const int want = single(parts[i], fix_scale, it, seed, want12, inl);
            check(want == cnt[(size_t)i] && !std::memcmp(want12, s12.data() + 8 * i, sizeof want12) && (n == 0 || !std::memcmp(inl.data(), fl.data() + start[(size_t)i], (size_t)n)),
                  "batch set against the solver", it, i);
            check((best[(size_t)i] >= 0) == (want > 0) && best[(size_t)i] < it, "winning iteration", it, i);
            ++sets;
        }
        check(cnt[1] == 0 && cnt[3] == 0 && (fix_scale || cnt[5] == 0), "sets without a result", it, fix_scale);
        for (int k = 0; k < first; ++k) check(fl[(size_t)k] == 9, "flags in front of pair_start[0] untouched", it, k);
        check(lpslam_sim3_ransac_batch_host(7, all.data(), start.data(), kCam, kCam, fix_scale, 0, 1, s12.data(), cnt.data(), fl.data(), nullptr) == 1, "iterations 0 refused", it, 0);
    }
    std::printf("sim3_ransac_asan: %ld sample tables, %ld sets of 16 batches compared with the solver; %d failures\n", tables, sets, failures);
    return failures ? 1 : 0;
}
