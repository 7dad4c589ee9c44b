// pose_cov.hip -- the covariance of poses the motion-only optimiser returned, for the device.  The arithmetic is
// pose_cov_math.h, the text the host runs (lpslam_amd/host/pose_cov_batch.cpp): the same bits.  It stands beside pose_opt.hip, whose
// kernels keep H in LDS inside their chain of trials and hand nothing of it out; this is one pass at the final pose.
// lpslam_hip_pose_covariance_batch, S sets of observations, a pose each:
//   host                 the argument rules, then ONE upload of set_start (rebased to 0), the poses, the observations and their flags
//   k_pose_covariance    one workgroup of 256 lanes per set: lane l adds the active observations l, l + 256, ... of its set in ascending
//                        order onto 0.0 in registers (22 sums and its count), the 256 partial sums of every value are folded in LDS by the
//                        fixed tree (strides 128 .. 1), lane 0 inverts and writes the set's results to page-locked memory; the last
//                        workgroup to arrive at the call's own arrival counter releases the done flag
//   host                 one wait
// The round trip -- page-locked block, device block, done flag, what becomes of them when a stream is late or dead -- is LpStagedCall
// (internal.h).
#include "internal.h"
#include "pose_cov_math.h"
#include <cstring>

using namespace lpslam;
namespace pcv = lpslam_pose_cov;

namespace {

struct PcHead { double cam[5]; int32_t n_sets; uint32_t o_start, o_pose, o_obs, o_active; };      // by value with the launch
struct PcOut { double* info21; double* cov21; double* chi2; double* min_pivot; int32_t* n_used; int32_t* status; };      // page-locked

__global__ __launch_bounds__(256) void k_pose_covariance(const uint8_t* __restrict__ base, PcHead head, PcOut out, unsigned* counter, int* flag, int seq)
{
    __shared__ double sh[pcv::kSums * pcv::kLanes];
    __shared__ int sh_used[pcv::kLanes];
    const int s = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (s < head.n_sets) {      // (the grid is n_sets workgroups; a workgroup decides as one)
        const int32_t* start = (const int32_t*)(base + head.o_start);
        const int begin = start[s], end = start[s + 1];
        const double* pose = (const double*)(base + head.o_pose) + 7 * (size_t)s;
        const double* obs = (const double*)(base + head.o_obs);
        const uint8_t* active = base + head.o_active;
        double R[9], t[3], acc[pcv::kSums];
        {
            double p7[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) p7[k] = pose[k];
            pcv::quat_to_rot(p7, R);
            t[0] = p7[4]; t[1] = p7[5]; t[2] = p7[6];
        }
#pragma unroll
        for (int q = 0; q < pcv::kSums; ++q) acc[q] = 0.0;
        int used = 0;
        for (int k = begin + lane; k < end; k += pcv::kLanes) {
            if (active[k] != 1) continue;
            double o[pcv::kObsDoubles];
#pragma unroll
            for (int j = 0; j < pcv::kObsDoubles; ++j) o[j] = obs[(size_t)pcv::kObsDoubles * k + j];
            if (pcv::obs_add(R, t, head.cam, o, acc)) ++used;
        }
#pragma unroll
        for (int q = 0; q < pcv::kSums; ++q) sh[q * pcv::kLanes + lane] = acc[q];
        sh_used[lane] = used;
        for (int stride = pcv::kLanes / 2; stride >= 1; stride >>= 1) {
            __syncthreads();
            if (lane < stride) {
#pragma unroll
                for (int q = 0; q < pcv::kSums; ++q) sh[q * pcv::kLanes + lane] += sh[q * pcv::kLanes + lane + stride];
                sh_used[lane] += sh_used[lane + stride];
            }
        }
        if (lane == 0) {
            double sums[pcv::kSums], cov[21], piv;
#pragma unroll
            for (int q = 0; q < pcv::kSums; ++q) sums[q] = sh[q * pcv::kLanes];
            const int n_used = sh_used[0];
            const int st = pcv::invert(sums, n_used, cov, &piv);
#pragma unroll
            for (int q = 0; q < 21; ++q) { out.info21[21 * (size_t)s + q] = sums[q]; out.cov21[21 * (size_t)s + q] = cov[q]; }
            out.chi2[s] = sums[21]; out.min_pivot[s] = piv; out.n_used[s] = n_used; out.status[s] = st;
        }
    }
    lp_signal_done(counter, flag, seq);
}

}  // namespace

extern "C" {

int lpslam_hip_pose_covariance_batch(lpslam_hip_ctx* c, int32_t n_sets, const int32_t* set_start, const double* pose7, const double* obs, const uint8_t* active,
                                     const double* cam, double* info21, double* cov21, double* chi2, double* min_pivot, int32_t* n_used, int32_t* status)
{
    if (!c) { set_error("null context"); return LPSLAM_HIP_ERR_INVALID; }
    int first = 0, total = 0;
    const char* why = "";
    if (const int rc = pcv::check_args(n_sets, set_start, pose7, obs, active, cam, info21, cov21, chi2, min_pivot, n_used, status, &first, &total, &why)) {
        set_error("pose_covariance_batch: %s", why);
        return rc;
    }
    LP_HIP(hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    // page-locked block: flag | input (set_start rebased to 0, poses, observations, flags) | results; device block: the input
    const size_t o_in = 64, tot1 = (size_t)(total > 0 ? total : 1);
    LpLayout dev;
    const size_t o_start = dev.take((size_t)(n_sets + 1) * 4), o_pose = dev.take((size_t)n_sets * 56), o_obs = dev.take(tot1 * 56), o_active = dev.take(tot1);
    const size_t in_bytes = dev.at;
    LpLayout host{o_in + in_bytes};
    const size_t h_info = host.take((size_t)n_sets * 168), h_cov = host.take((size_t)n_sets * 168), h_chi = host.take((size_t)n_sets * 8), h_piv = host.take((size_t)n_sets * 8);
    const size_t h_used = host.take((size_t)n_sets * 4), h_status = host.take((size_t)n_sets * 4);
    LpStagedCall call{c, s, "pose_covariance_batch"};
    if (int rc = call.open(host.at, in_bytes, LP_DONE_POSE_COV)) return rc;
    uint8_t *hb = call.host, *base = call.dev(), *in = hb + o_in;
    int32_t* start0 = (int32_t*)(in + o_start);
    for (int i = 0; i <= n_sets; ++i) start0[i] = set_start[i] - first;
    memcpy(in + o_pose, pose7, (size_t)n_sets * 56);
    if (total > 0) {
        memcpy(in + o_obs, obs + 7 * (size_t)first, (size_t)total * 56);
        memcpy(in + o_active, active + (size_t)first, (size_t)total);
    }
    PcHead head{};
    memcpy(head.cam, cam, 40);
    head.n_sets = n_sets; head.o_start = (uint32_t)o_start; head.o_pose = (uint32_t)o_pose; head.o_obs = (uint32_t)o_obs; head.o_active = (uint32_t)o_active;
    const PcOut out{(double*)(hb + h_info), (double*)(hb + h_cov), (double*)(hb + h_chi), (double*)(hb + h_piv), (int32_t*)(hb + h_used), (int32_t*)(hb + h_status)};
    if (int rc = call.upload(o_in, in_bytes)) return rc;
    hipLaunchKernelGGL(k_pose_covariance, dim3((unsigned)n_sets), dim3(pcv::kLanes), 0, s, (const uint8_t*)base, head, out, call.done.counter, call.done.flag, call.done.seq);
    if (int rc = call.finish()) return rc;
    memcpy(info21, hb + h_info, (size_t)n_sets * 168); memcpy(cov21, hb + h_cov, (size_t)n_sets * 168);
    memcpy(chi2, hb + h_chi, (size_t)n_sets * 8); memcpy(min_pivot, hb + h_piv, (size_t)n_sets * 8);
    memcpy(n_used, hb + h_used, (size_t)n_sets * 4); memcpy(status, hb + h_status, (size_t)n_sets * 4);
    return LPSLAM_HIP_OK;
}

}  // extern "C"
