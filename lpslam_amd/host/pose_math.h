// pose_math.h -- the host's pose algebra: world -> camera poses as (unit quaternion w x y z, translation), x_c = R x_w + t.
//
// The host library is built with -ffp-contract=off, so every expression below rounds as it is written: the order of the sums is
// part of the interface (a run of the tracker reproduces bit for bit).  The device-side twins (quat_to_rot,
// po_quat_to_rot, s3_q_to_R) differ on purpose in contraction and normalisation and are not these.
#pragma once
#include <cmath>
#include "../csrc/sim3_math.h"

namespace LpSlam {

struct Pose { double q[4] = {1, 0, 0, 0}; double t[3] = {0, 0, 0}; };   // world -> camera
struct Mat3 { double m[9]; };                                            // row major

inline Mat3 quatToRot(const double* q)
{
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    return {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
             2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
             2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
}

inline void quatMul(const double* a, const double* b, double* o)
{
    const double r[4] = {a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]};
    const double n = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
    for (int i = 0; i < 4; ++i) o[i] = r[i] / n;
}

// Eigen::Quaterniond(R) for a rotation matrix (row major): the one definition is csrc/sim3_math.h (the device calls it too)
inline void rotToQuat(const double* m, double* q) { lpslam_sim3::rot_to_quat(m, q); }
inline void rotToQuat(const Mat3& R, double* q) { rotToQuat(R.m, q); }

// out = R X + t (out must not be X)
inline void transform(const Mat3& R, const double* t, const double* X, double* out)
{
    for (int r = 0; r < 3; ++r) out[r] = R.m[r * 3] * X[0] + R.m[r * 3 + 1] * X[1] + R.m[r * 3 + 2] * X[2] + t[r];
}

inline Pose compose(const Pose& a, const Pose& b)          // a after b
{
    Pose o;
    quatMul(a.q, b.q, o.q);
    transform(quatToRot(a.q), a.t, b.t, o.t);
    return o;
}

inline void centre(const Pose& p, double* C)               // the camera centre in the world, -R^T t
{
    const Mat3 R = quatToRot(p.q);
    for (int a = 0; a < 3; ++a) C[a] = -(R.m[a] * p.t[0] + R.m[3 + a] * p.t[1] + R.m[6 + a] * p.t[2]);
}

inline Pose inverse(const Pose& a)
{
    Pose o;
    o.q[0] = a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = -a.q[3];
    centre(a, o.t);
    return o;
}

// a * b^-1 through the rotation matrices: R = R_a R_b^T, t = t_a - R t_b
inline Pose relative(const Pose& a, const Pose& b)
{
    const Mat3 Ra = quatToRot(a.q), Rb = quatToRot(b.q);
    Mat3 R;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R.m[r * 3 + c] = Ra.m[r * 3] * Rb.m[c * 3] + Ra.m[r * 3 + 1] * Rb.m[c * 3 + 1] + Ra.m[r * 3 + 2] * Rb.m[c * 3 + 2];
    Pose o;
    rotToQuat(R, o.q);
    for (int r = 0; r < 3; ++r) o.t[r] = a.t[r] - (R.m[r * 3] * b.t[0] + R.m[r * 3 + 1] * b.t[1] + R.m[r * 3 + 2] * b.t[2]);
    return o;
}

}  // namespace LpSlam
