// pose_cov_asan.cpp -- stand-alone driver of the pose covariance call's host code for a sanitizer build:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/pose_cov_asan.cpp lpslam_amd/host/pose_cov_batch.cpp -o pose_cov_asan && ./pose_cov_asan
// It runs lpslam_pose_covariance_batch_host and lpslam_pose_sigmas_host over the shapes of tests/test_pose_cov_cpu.py (n = 0, 2, 3, 4,
// 63, 64, 65, 255, 256, 257, 513, 2000; mono, stereo and mixed; one point seen five times, seven collinear points, two stereo points; a
// set that is all inactive; points behind the camera; a batch of nine from a set_start that does not begin at 0; every refusal) and
// checks what can be checked without a reference: the status and count rules, H Sigma = I, a batch equal to separate calls.  Every
// array has exactly the documented size, so that a read or write past it is seen.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
int lpslam_pose_covariance_batch_host(int32_t n_sets, const int32_t* set_start, const double* pose7, const double* obs, const uint8_t* active, const double* cam,
                                      double* info21, double* cov21, double* chi2, double* min_pivot, int32_t* n_used, int32_t* status);
int lpslam_pose_sigmas_host(const double* pose7, const double* cov21, double* out4);
}

namespace {
const double kCam[5] = {500.0, 500.0, 320.0, 240.0, 60.0};
struct Lcg { uint64_t s; double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; } };
struct Set { double pose[7]; std::vector<double> obs; std::vector<uint8_t> active; };
enum Kind { MONO, STEREO, MIXED, SAME_POINT, COLLINEAR, TWO_STEREO, INACTIVE, BEHIND };

void rot(const double* q, double* R)
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

// n points 2 .. 20 m in front of a random pose, inside the image, weights 1.2^-2o, residuals of up to 2 pixels
Set make(int n, Kind kind, uint64_t seed)
{
    Lcg g{seed * 977 + (uint64_t)n};
    Set s;
    double q[4], nq = 0, R[9];
    for (int k = 0; k < 4; ++k) { q[k] = g.next() - 0.5; nq += q[k] * q[k]; }
    for (int k = 0; k < 4; ++k) { q[k] /= std::sqrt(nq); s.pose[k] = q[k]; }
    for (int k = 0; k < 3; ++k) s.pose[4 + k] = 4 * g.next() - 2;
    rot(q, R);
    if (kind == SAME_POINT) n = 5;
    if (kind == COLLINEAR) n = 7;
    if (kind == TWO_STEREO) n = 2;
    double first[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
        double pc[3];
        const double z = 2 + 18 * g.next(), u = 60 + 560 * g.next(), v = 20 + 440 * g.next();
        pc[0] = (u - kCam[2]) / kCam[0] * z; pc[1] = (v - kCam[3]) / kCam[1] * z; pc[2] = z;
        if (kind == COLLINEAR) { const double t = -1.5 + 0.5 * i; pc[0] = 0.3 + 0.8 * t; pc[1] = -0.2 + 0.6 * t; pc[2] = 6.0; }
        if (kind == SAME_POINT) { if (i == 0) memcpy(first, pc, sizeof pc); else memcpy(pc, first, sizeof pc); }
        const bool stereo = kind == STEREO || kind == TWO_STEREO || ((kind == MIXED || kind == BEHIND || kind == INACTIVE) && g.next() < 0.5);
        const double pu = kCam[0] * pc[0] / pc[2] + kCam[2], pv = kCam[1] * pc[1] / pc[2] + kCam[3];
        const double lvl = std::pow(1.2, (double)(int)(8 * g.next()));
        double o[7] = {pu + 4 * g.next() - 2, pv + 4 * g.next() - 2, stereo ? pu - kCam[4] / pc[2] + 4 * g.next() - 2 : -1.0, 1.0 / (lvl * lvl), 0, 0, 0};
        if (kind == BEHIND && (i == 1 || i == n / 2 || i == n - 1)) pc[2] = i == 1 ? -3.0 : i == n - 1 ? -0.5 : -1e-3;
        const double d[3] = {pc[0] - s.pose[4], pc[1] - s.pose[5], pc[2] - s.pose[6]};
        for (int a = 0; a < 3; ++a) o[4 + a] = R[a] * d[0] + R[3 + a] * d[1] + R[6 + a] * d[2];
        s.obs.insert(s.obs.end(), o, o + 7);
        s.active.push_back(kind == INACTIVE ? 0 : 1);
    }
    return s;
}

int failures = 0;
void check(bool ok, const char* what, int a, int b) { if (!ok) { ++failures; std::printf("FAILED: %s (%d, %d)\n", what, a, b); } }

struct Out { std::vector<double> info, cov, chi2, piv; std::vector<int32_t> used, status; explicit Out(size_t n) : info(21 * n), cov(21 * n), chi2(n), piv(n), used(n), status(n) {} };

double sym(const double* m, int a, int c) { const int lo = a < c ? a : c, hi = a < c ? c : a; return m[lo * 6 - lo * (lo - 1) / 2 + hi - lo]; }

// one set through the batch call from arrays of exactly its size; the rules that hold for every set
void single(const Set& s, Out& o, int want_used, int want_status, int tag)
{
    const int32_t start[2] = {0, (int32_t)s.active.size()};
    const int rc = lpslam_pose_covariance_batch_host(1, start, s.pose, s.obs.empty() ? nullptr : s.obs.data(), s.active.empty() ? nullptr : s.active.data(), kCam,
                                                     o.info.data(), o.cov.data(), o.chi2.data(), o.piv.data(), o.used.data(), o.status.data());
    check(rc == 0, "the call is accepted", rc, tag);
    check(o.used[0] == want_used, "n_used", o.used[0], want_used);
    check(o.status[0] == want_status, "status", o.status[0], want_status);
    if (o.status[0] != 0) { for (int k = 0; k < 21; ++k) check(o.cov[k] == 0.0, "a refused set's covariance is zeros", k, tag); return; }
    check(o.piv[0] > 1e-8 && o.piv[0] <= 1.0 + 1e-12, "the smallest pivot of an accepted set lies in (1e-8, 1]", tag, 0);
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 6; ++c) {
            double v = 0;
            for (int k = 0; k < 6; ++k) v += sym(o.info.data(), a, k) * sym(o.cov.data(), k, c);
            check(std::fabs(v - (a == c ? 1.0 : 0.0)) < 1e-6, "H Sigma = I", a, c);
        }
    double sg[4];
    check(lpslam_pose_sigmas_host(s.pose, o.cov.data(), sg) == 0, "pose_sigmas", tag, 0);
    for (int k = 0; k < 4; ++k) check(sg[k] > 0 && std::isfinite(sg[k]), "a sigma is positive and finite", k, tag);
}
}  // namespace

int main()
{
    const int sizes[] = {0, 2, 3, 4, 63, 64, 65, 255, 256, 257, 513, 2000};
    for (int n : sizes)
        for (Kind kind : {MONO, STEREO, MIXED}) {
            Out o(1);
            single(make(n, kind, 7), o, n, n >= 3 ? 0 : 1, n);
        }
    { Out o(1); single(make(0, SAME_POINT, 7), o, 5, 2, -1); check(std::fabs(o.piv[0]) <= 1e-9, "one point seen five times: pivot", 0, 0); }
    { Out o(1); single(make(0, COLLINEAR, 7), o, 7, 2, -2); check(std::fabs(o.piv[0]) <= 1e-9, "collinear points: pivot", 0, 0); }
    { Out o(1); single(make(0, TWO_STEREO, 7), o, 2, 1, -3); check(std::fabs(o.piv[0]) <= 1e-9, "two stereo points: pivot", 0, 0); }
    { Out o(1); single(make(30, INACTIVE, 7), o, 0, 1, -4); }
    { Out o(1); single(make(40, BEHIND, 7), o, 37, 0, -5); }

    // nine sets in one call, behind 11 records that belong to nobody, against separate calls
    const Set sets[9] = {make(64, MIXED, 3), make(0, SAME_POINT, 3), make(0, COLLINEAR, 3), make(0, TWO_STEREO, 3), make(30, INACTIVE, 3), make(40, BEHIND, 3),
                         make(257, MONO, 3), make(0, MIXED, 3), make(513, MIXED, 3)};
    for (int first : {0, 11}) {
        std::vector<int32_t> start{first};
        std::vector<double> obs((size_t)7 * first, NAN), pose;
        std::vector<uint8_t> active((size_t)first, 1);
        for (const Set& s : sets) {
            obs.insert(obs.end(), s.obs.begin(), s.obs.end()); active.insert(active.end(), s.active.begin(), s.active.end());
            pose.insert(pose.end(), s.pose, s.pose + 7); start.push_back((int32_t)active.size());
        }
        Out all(9);
        const int rc = lpslam_pose_covariance_batch_host(9, start.data(), pose.data(), obs.data(), active.data(), kCam, all.info.data(), all.cov.data(), all.chi2.data(),
                                                         all.piv.data(), all.used.data(), all.status.data());
        check(rc == 0, "the batch is accepted", rc, first);
        for (int i = 0; i < 9; ++i) {
            Out o(1);
            const int32_t st[2] = {0, (int32_t)sets[i].active.size()};
            lpslam_pose_covariance_batch_host(1, st, sets[i].pose, sets[i].obs.empty() ? nullptr : sets[i].obs.data(), sets[i].active.empty() ? nullptr : sets[i].active.data(), kCam,
                                              o.info.data(), o.cov.data(), o.chi2.data(), o.piv.data(), o.used.data(), o.status.data());
            const bool same = !memcmp(o.info.data(), &all.info[21 * i], 168) && !memcmp(o.cov.data(), &all.cov[21 * i], 168) && !memcmp(&o.chi2[0], &all.chi2[i], 8) &&
                              !memcmp(&o.piv[0], &all.piv[i], 8) && o.used[0] == all.used[i] && o.status[0] == all.status[i];
            check(same, "a set of the batch equals its own call", i, first);
        }
    }

    // the refusals: nothing is read or written
    {
        const Set s = make(20, MIXED, 5);
        Out o(1);
        const int32_t start[2] = {0, 20}, down[2] = {5, 3}, neg[2] = {-1, 3}, over[2] = {0, (1 << 18) + 1}, dip[3] = {0, 12, 8};
        std::vector<int32_t> many(4098, 0);
        const void* args[10] = {s.pose, s.obs.data(), s.active.data(), kCam, o.info.data(), o.cov.data(), o.chi2.data(), o.piv.data(), o.used.data(), o.status.data()};
        auto call = [&](int32_t n_sets, const int32_t* st, int null_at) {
            const void* a[10];
            for (int k = 0; k < 10; ++k) a[k] = k == null_at ? nullptr : args[k];
            return lpslam_pose_covariance_batch_host(n_sets, st, (const double*)a[0], (const double*)a[1], (const uint8_t*)a[2], (const double*)a[3], (double*)a[4], (double*)a[5],
                                                     (double*)a[6], (double*)a[7], (int32_t*)a[8], (int32_t*)a[9]);
        };
        check(call(1, start, -1) == 0, "a good call", 0, 0);
        check(call(1, nullptr, -1) == 1, "null set_start", 0, 0);
        for (int k = 0; k < 10; ++k) check(call(1, start, k) == 1, "a null argument", k, 0);
        check(call(0, start, -1) == 1 && call(-1, start, -1) == 1, "n_sets < 1", 0, 0);
        check(call(1, down, -1) == 1 && call(1, neg, -1) == 1 && call(2, dip, -1) == 1, "set_start not ascending", 0, 0);
        check(call(4097, many.data(), -1) == 3, "more than 4096 sets", 0, 0);
        check(call(1, over, -1) == 3, "more than 1 << 18 observations", 0, 0);
        double sg[4];
        check(lpslam_pose_sigmas_host(nullptr, o.cov.data(), sg) == 1 && lpslam_pose_sigmas_host(s.pose, nullptr, sg) == 1 && lpslam_pose_sigmas_host(s.pose, o.cov.data(), nullptr) == 1,
              "pose_sigmas refuses null", 0, 0);
    }
    std::printf(failures ? "pose_cov_asan: %d check(s) FAILED\n" : "pose_cov_asan: all checks passed\n", failures);
    return failures ? 1 : 0;
}
