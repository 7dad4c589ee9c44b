// sim3_batch.cpp -- the CPU side of the batched loop verification: C shims for the tests and the timing tool.
//   lpslam_sim3_sample_table        the 3-pair samples sim3_solve_ransac draws for a set of n pairs (csrc/ransac_sample.h)
//   lpslam_sim3_ransac_batch_host   lpslam_hip_sim3_ransac_batch without the context: sim3_solve_ransac on each set -- the CPU definition
#include "two_view.h"
#include "../csrc/epnp_math.h"
#include "../csrc/ransac_sample.h"
#include "../csrc/sim3_math.h"
#include "../../include/lpslam_hip.h"
#include <cmath>
#include <vector>

#define LP_EXPORT extern "C" __attribute__((visibility("default")))

// 1: table holds iterations x 3 indices; 0: n < 3 or iterations < 1, table untouched
LP_EXPORT int lpslam_sim3_sample_table(int n, int iterations, uint32_t seed, int32_t* table)
{
    if (n < 3 || iterations < 1 || !table) return 0;
    std::vector<int> avail((size_t)n);
    lpslam_ransac::sample_table<3>(n, iterations, seed, table, avail.data());
    return 1;
}

// 0: done; 1: refused (the argument rules of lpslam_hip_sim3_ransac_batch, but for its cap on the iterations), nothing written.
// What sim3_solve_ransac leaves open when it finds nothing (n < 3, every sample refused, no sample that explains a pair) is fixed
// here: count 0, best_iteration -1, flags cleared, s12 = 1 0 0 0 0 0 0 1.
LP_EXPORT int lpslam_sim3_ransac_batch_host(int32_t n_sets, const lpslam_hip_sim3_pair* pairs, const int32_t* pair_start, const double* cam1, const double* cam2,
                                            int32_t fix_scale, int32_t iterations, uint32_t seed, double* s12, int32_t* n_inliers, uint8_t* inlier, int32_t* best_iteration)
{
    int first = 0, total = 0;
    if (lpslam_ransac::check_offsets(n_sets, pair_start, &first, &total) || iterations < 1 || !cam1 || !cam2 || (n_sets > 0 && (!s12 || !n_inliers))) return 1;
    if (total > 0 && (!pairs || !inlier)) return 1;
    for (int k = 0; k < 4; ++k) if (!std::isfinite(cam1[k]) || !std::isfinite(cam2[k])) return 1;
    std::vector<double> p1, p2, o1, o2, w1, w2;
    std::vector<int32_t> table;
    std::vector<uint8_t> cur;
    for (int s = 0; s < n_sets; ++s) {
        const size_t o = (size_t)pair_start[s];
        const int n = pair_start[s + 1] - pair_start[s];
        p1.resize((size_t)3 * n); p2.resize((size_t)3 * n); o1.resize((size_t)2 * n); o2.resize((size_t)2 * n); w1.resize((size_t)n); w2.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            const lpslam_hip_sim3_pair& pr = pairs[o + (size_t)i];
            for (int a = 0; a < 3; ++a) { p1[3 * (size_t)i + a] = pr.p1c[a]; p2[3 * (size_t)i + a] = pr.p2c[a]; }
            for (int a = 0; a < 2; ++a) { o1[2 * (size_t)i + a] = pr.obs1[a]; o2[2 * (size_t)i + a] = pr.obs2[a]; }
            w1[(size_t)i] = pr.inv_sigma2_1; w2[(size_t)i] = pr.inv_sigma2_2;
            inlier[o + (size_t)i] = 0;
        }
        double* out = s12 + 8 * (size_t)s;
        out[0] = 1; for (int k = 1; k < 7; ++k) out[k] = 0; out[7] = 1;
        n_inliers[s] = LpSlam::sim3_solve_ransac(p1.data(), p2.data(), o1.data(), o2.data(), w1.data(), w2.data(), n, cam1, cam2, fix_scale != 0, iterations, seed, out, inlier + o);
        if (!best_iteration) continue;
        // which sample won: the loop of sim3_solve_ransac over the table, first maximum
        best_iteration[s] = -1;
        if (n < 3 || n_inliers[s] == 0) continue;
        table.resize((size_t)iterations * 3);
        lpslam_sim3_sample_table(n, iterations, seed, table.data());
        int best = 0;
        cur.resize((size_t)n);
        for (int it = 0; it < iterations; ++it) {
            const int32_t* idx = table.data() + (size_t)3 * it;
            double a1[9], a2[9], R[9], t[3], sc;
            for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) { a1[3 * k + a] = p1[3 * (size_t)idx[k] + a]; a2[3 * k + a] = p2[3 * (size_t)idx[k] + a]; }
            if (!lpslam_epnp::horn<3>(a1, a2, 3, fix_scale != 0, R, t, &sc)) continue;
            const int count = lpslam_sim3::sim3_score(R, t, sc, p1.data(), p2.data(), o1.data(), o2.data(), w1.data(), w2.data(), n, cam1, cam2, cur.data());
            if (count > best) { best = count; best_iteration[s] = it; }
        }
    }
    return 0;
}
