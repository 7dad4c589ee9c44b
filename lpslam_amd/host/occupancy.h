// occupancy.h -- the host half of the occupancy grid: a keyframe's laser pose in the map plane ("Occupancy grid").
#pragma once
#include <cmath>
#include "../../include/lpslam_hip.h"
#include "../../include/lpslam_types.h"

namespace LpSlam {

// The laser's pose in the camera's lpslam frame from what RequestNavTransformation answers for Laser -> Camera; an invalid answer (or
// a zero quaternion) is the identity.
inline void laserToCamera(const LpSlamGlobalState& s, double R[9], double t[3])
{
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    t[0] = t[1] = t[2] = 0.0;
    if (!s.valid) return;
    const double n = std::sqrt(s.orientation.w * s.orientation.w + s.orientation.x * s.orientation.x + s.orientation.y * s.orientation.y + s.orientation.z * s.orientation.z);
    if (!(n > 0) || !std::isfinite(n)) return;
    const double w = s.orientation.w / n, x = s.orientation.x / n, y = s.orientation.y / n, z = s.orientation.z / n;
    const double r[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 9; ++i) R[i] = r[i];
    t[0] = s.position.x; t[1] = s.position.y; t[2] = s.position.z;
}

// T_world_laser = T_world_cam (lpslam axes, from the keyframe's T_cw in optical axes: row-major R_cw, t_cw) * T_cam_laser, projected
// on the map plane: origin = (y, z) of the laser position, fwd / left = (y, z) of R_world_laser (0, 0, 1) / (0, -1, 0).  The laser's
// tilt is dropped by the projection.
inline void scanPose(const double R_cw[9], const double t_cw[3], const double R_cl[9], const double t_cl[3], double origin[2], double fwd[2], double left[2])
{
    // optical (x right, y down, z forward) -> lpslam (x up, y right, z forward): v_lp = A v_opt, A = [[0,-1,0],[1,0,0],[0,0,1]]
    double C[3], Rwc[9];
    for (int r = 0; r < 3; ++r) {
        C[r] = -(R_cw[r] * t_cw[0] + R_cw[3 + r] * t_cw[1] + R_cw[6 + r] * t_cw[2]);      // camera centre, optical world
        for (int c = 0; c < 3; ++c) Rwc[r * 3 + c] = R_cw[c * 3 + r];
    }
    static const double A[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    double T[9], Rl[9];                                                                       // Rl = A Rwc A^T
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) T[r * 3 + c] = A[r * 3] * Rwc[c] + A[r * 3 + 1] * Rwc[3 + c] + A[r * 3 + 2] * Rwc[6 + c];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rl[r * 3 + c] = T[r * 3] * A[c * 3] + T[r * 3 + 1] * A[c * 3 + 1] + T[r * 3 + 2] * A[c * 3 + 2];
    const double tl[3] = {-C[1], C[0], C[2]};
    double Rwl[9], twl[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Rwl[r * 3 + c] = Rl[r * 3] * R_cl[c] + Rl[r * 3 + 1] * R_cl[3 + c] + Rl[r * 3 + 2] * R_cl[6 + c];
        twl[r] = Rl[r * 3] * t_cl[0] + Rl[r * 3 + 1] * t_cl[1] + Rl[r * 3 + 2] * t_cl[2] + tl[r];
    }
    origin[0] = twl[1]; origin[1] = twl[2];
    fwd[0] = Rwl[5]; fwd[1] = Rwl[8];
    left[0] = -Rwl[4]; left[1] = -Rwl[7];
}

}  // namespace LpSlam
