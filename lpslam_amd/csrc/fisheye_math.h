// fisheye_math.h -- the equidistant ("fisheye", Kannala-Brandt) camera model of the monocular tracker, once,
// for the device kernels (frontend.hip), the host tracker (lpslam_amd/host/hip_tracker.cpp) and the CPU tests: FP64 throughout.
//   undistort   [UPSTREAM] cv::fisheye::undistortPoints with R = I, P = K and the default criteria (10 iterations, eps 1e-8), written
//               down from memory of OpenCV 4.5+ and not checked against OpenCV itself: Newton on theta (1 + k1 theta^2 + ...) = theta_d
//   validity    this project's own rule: converged, theta >= 0, theta_d0 <= pi/2, theta <= max_angle (OpenCV returns a mirrored
//               position for a pixel beyond 90 degrees; such a point has no undistorted position here)
//   forward     host only: the sensor pixel of a camera-frame point, for the tracker's visibility test
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LP_FISHEYE_FN __host__ __device__ __forceinline__
#else
#define LP_FISHEYE_FN inline
#endif

namespace lpslam_fisheye {

struct Model { double fx, fy, cx, cy, k[4], max_angle; };      // max_angle in radians

constexpr double kHalfPi = 1.57079632679489661923;
constexpr double kEps = 1e-8;
constexpr int kMaxIterations = 10;

// theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)
LP_FISHEYE_FN double distort_angle(const Model& m, double theta)
{
    const double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    return theta * (1.0 + m.k[0] * t2 + m.k[1] * t4 + m.k[2] * t6 + m.k[3] * t8);
}

// The undistorted (pinhole, same K) position of sensor pixel (px, py), rounded to float32 once at the end.  false: the point is
// invalid and *ux, *uy are not written.  *theta_out (may be null) receives the angle the iteration ended at.
LP_FISHEYE_FN bool undistort(const Model& m, double px, double py, float* ux, float* uy, double* theta_out = nullptr)
{
    const double x = (px - m.cx) / m.fx, y = (py - m.cy) / m.fy;
    const double theta_d0 = hypot(x, y);
    const double theta_d = theta_d0 < kHalfPi ? theta_d0 : kHalfPi;
    bool converged = false;
    double theta = theta_d, scale = 1.0;
    if (theta_d <= kEps) converged = true;
    else {
        for (int it = 0; it < kMaxIterations; ++it) {
            const double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const double k0t2 = m.k[0] * t2, k1t4 = m.k[1] * t4, k2t6 = m.k[2] * t6, k3t8 = m.k[3] * t8;
            const double fix = (theta * (1.0 + k0t2 + k1t4 + k2t6 + k3t8) - theta_d) / (1.0 + 3.0 * k0t2 + 5.0 * k1t4 + 7.0 * k2t6 + 9.0 * k3t8);
            theta -= fix;
            if (fabs(fix) < kEps) { converged = true; break; }
        }
        scale = tan(theta) / theta_d;
    }
    if (theta_out) *theta_out = theta;
    if (!(converged && theta >= 0.0 && theta_d0 <= kHalfPi && theta <= m.max_angle)) return false;      // (a NaN fails every comparison)
    *ux = (float)(m.fx * x * scale + m.cx);
    *uy = (float)(m.fy * y * scale + m.cy);
    return true;
}

// Host only from here on (plain inline functions).
// The sensor pixel of camera-frame point (X, Y, Z), Z > 0, and its angle from the axis.  On the axis: the principal point.
inline void forward(const Model& m, double X, double Y, double Z, double* sx, double* sy, double* theta_out)
{
    const double r = hypot(X, Y), theta = atan2(r, Z);
    *theta_out = theta;
    if (r > 0.0) {
        const double theta_d = distort_angle(m, theta);
        *sx = m.fx * theta_d * X / r + m.cx; *sy = m.fy * theta_d * Y / r + m.cy;
    } else { *sx = m.cx; *sy = m.cy; }
}
// Visible: in front of the camera, inside the angle limit, and the SENSOR pixel inside the width x height image.
inline bool visible(const Model& m, double X, double Y, double Z, int width, int height)
{
    if (!(Z > 0.0)) return false;
    double sx, sy, theta;
    forward(m, X, Y, Z, &sx, &sy, &theta);
    return theta <= m.max_angle && sx >= 0.0 && sx < (double)width && sy >= 0.0 && sy < (double)height;
}
// a model the library accepts: finite values, positive focal lengths, max_angle in (0, 89 degrees] (89 pi / 180 rounds to
// 1.5533430342749532 or ...535 depending on the order of the caller's conversion: both are 89 degrees)
inline bool model_ok(const Model& m)
{
    const double v[9] = {m.fx, m.fy, m.cx, m.cy, m.k[0], m.k[1], m.k[2], m.k[3], m.max_angle};
    for (double d : v) if (!isfinite(d)) return false;
    return m.fx > 0.0 && m.fy > 0.0 && m.max_angle > 0.0 && m.max_angle <= 1.5533430342749535;
}

}  // namespace lpslam_fisheye
