// pose_cov_batch.cpp -- the CPU side of the pose covariance call: C shims for the tests, the timing tool and the tracker.
//   lpslam_pose_covariance_batch_host   lpslam_hip_pose_covariance_batch without the context: the text of csrc/pose_cov_math.h on each set,
//                                       the sums in the stated order -- the CPU definition, the same bits
//   lpslam_pose_sigmas_host             pose_sigmas of that header: covariance -> x_sigma y_sigma z_sigma (lpslam axes), orientation sigma
#include "../csrc/pose_cov_math.h"
#include "../../include/lpslam_hip.h"
#include <vector>

#define LP_EXPORT extern "C" __attribute__((visibility("default")))

namespace pcv = lpslam_pose_cov;

// LPSLAM_HIP_OK, or the code lpslam_hip_pose_covariance_batch refuses the same arguments with (nothing written)
LP_EXPORT int lpslam_pose_covariance_batch_host(int32_t n_sets, const int32_t* set_start, const double* pose7, const double* obs, const uint8_t* active, const double* cam,
                                                double* info21, double* cov21, double* chi2, double* min_pivot, int32_t* n_used, int32_t* status)
{
    int first = 0, total = 0;
    const char* why = "";
    if (const int rc = pcv::check_args(n_sets, set_start, pose7, obs, active, cam, info21, cov21, chi2, min_pivot, n_used, status, &first, &total, &why)) return rc;
    std::vector<double> partial((size_t)pcv::kLanes * pcv::kSums);
    for (int s = 0; s < n_sets; ++s) {
        const size_t o = (size_t)set_start[s];
        const int n = set_start[s + 1] - set_start[s];
        double sums[pcv::kSums];
        const int used = pcv::set_sums(pose7 + 7 * (size_t)s, cam, n > 0 ? obs + pcv::kObsDoubles * o : nullptr, n > 0 ? active + o : nullptr, n, partial.data(), sums);
        for (int k = 0; k < 21; ++k) info21[21 * (size_t)s + k] = sums[k];
        chi2[s] = sums[21];
        n_used[s] = used;
        status[s] = pcv::invert(sums, used, cov21 + 21 * (size_t)s, min_pivot + s);
    }
    return LPSLAM_HIP_OK;
}

// 0: out4 written; 1: a null argument
LP_EXPORT int lpslam_pose_sigmas_host(const double* pose7, const double* cov21, double* out4)
{
    if (!pose7 || !cov21 || !out4) return 1;
    pcv::pose_sigmas(pose7, cov21, out4);
    return 0;
}
