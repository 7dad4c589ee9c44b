// pnp_batch.cpp -- the CPU side of the batched PnP RANSAC: C shims for the tests and the timing tool.
//   lpslam_pnp_sample_table        the 4-match samples pnp_solve_ransac draws for a set of n matches (csrc/ransac_sample.h)
//   lpslam_epnp4_host              the header's epnp<4> on the host (LpSlam::epnp_solve at n = 4 runs the same template at a run-time n)
//   lpslam_pnp_ransac_batch_host   lpslam_hip_pnp_ransac_batch without the context: pnp_solve_ransac on each set -- the CPU definition
#include "two_view.h"
#include "../csrc/epnp_math.h"
#include "../csrc/ransac_sample.h"
#include <vector>

#define LP_EXPORT extern "C" __attribute__((visibility("default")))

// 1: table holds iterations x 4 indices; 0: n < 4 or iterations < 1, table untouched
LP_EXPORT int lpslam_pnp_sample_table(int n, int iterations, uint32_t seed, int32_t* table)
{
    if (n < 4 || iterations < 1 || !table) return 0;
    std::vector<int> avail((size_t)n);
    lpslam_ransac::sample_table<4>(n, iterations, seed, table, avail.data());
    return 1;
}

LP_EXPORT int lpslam_epnp4_host(const double* p4, const double* u4, const double* cam, double* R9, double* t3)
{
    double ws[lpslam_epnp::kWorkspace];
    return lpslam_epnp::epnp<4>(p4, u4, 4, cam, nullptr, nullptr, ws, 1, R9, t3) ? 1 : 0;
}

// 0: done; 1: refused (the argument rules of lpslam_hip_pnp_ransac_batch, but for its cap on the iterations), nothing written
LP_EXPORT int lpslam_pnp_ransac_batch_host(int32_t n_sets, const int32_t* offsets, const double* pw, const double* obs, const double* inv_sigma2, const double* cam4,
                                           int32_t iterations, uint32_t seed, double* pose7, int32_t* n_inliers, uint8_t* inlier, int32_t* best_iteration)
{
    int first = 0, total = 0;
    if (lpslam_ransac::check_offsets(n_sets, offsets, &first, &total) || iterations < 1 || !cam4 || (n_sets > 0 && (!pose7 || !n_inliers))) return 1;
    if (total > 0 && (!pw || !obs || !inv_sigma2 || !inlier)) return 1;
    std::vector<int32_t> table;
    std::vector<uint8_t> cur;
    for (int s = 0; s < n_sets; ++s) {
        const size_t o = (size_t)offsets[s];
        const int n = offsets[s + 1] - offsets[s];
        const double* spw = pw + 3 * o; const double* sob = obs + 2 * o; const double* sw = inv_sigma2 + o;
        double* p7 = pose7 + 7 * (size_t)s;
        p7[0] = 1; for (int k = 1; k < 7; ++k) p7[k] = 0;                       // (pnp_solve_ransac leaves the pose alone when it finds none)
        n_inliers[s] = LpSlam::pnp_solve_ransac(spw, sob, sw, n, cam4, iterations, seed, p7, inlier + o);
        if (!best_iteration) continue;
        // which sample won: the loop of pnp_solve_ransac over the table, first maximum
        best_iteration[s] = -1;
        if (n < 4 || n_inliers[s] == 0) continue;
        table.resize((size_t)iterations * 4);
        lpslam_pnp_sample_table(n, iterations, seed, table.data());
        int best = 0;
        cur.resize((size_t)n);
        for (int it = 0; it < iterations; ++it) {
            double R[9], t[3];
            if (!lpslam_epnp::pnp_solve_sample(spw, sob, table.data() + (size_t)4 * it, cam4, R, t)) continue;
            const int count = lpslam_epnp::pnp_score(R, t, cam4, spw, sob, sw, n, cur.data());
            if (count > best) { best = count; best_iteration[s] = it; }
        }
    }
    return 0;
}
