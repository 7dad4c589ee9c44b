// radtan_math.h -- the radial-tangential ("perspective", Brown-Conrady k1 k2 p1 p2 k3) camera model of the monocular tracker
// (DESIGN.md section 32), once, for the device kernels (frontend.hip), the host tracker (lpslam_amd/host/hip_tracker.cpp) and the CPU
// tests: FP64 throughout.
//   undistort   [UPSTREAM] camera::perspective::undistort_keypoints = cv::undistortPoints(pts, K, D, R = I, P = K) with the default
//               criteria: FIVE fixed-point steps and no epsilon test.  Restated from memory of OpenCV 4.x and not checked against
//               OpenCV itself.
//   validity    this project's own rule (upstream returns something for every pixel): the denominator positive in each of the five
//               steps, everything finite, and the forward model applied to the result within half a pixel of the input -- the
//               localisation quantum of a level-0 FAST corner.  The residual is taken at the FP64 normalised result, before the one
//               rounding to float32, so that validity does not depend on that rounding.
//   forward     host and device: the validity rule needs it; the tracker's visibility test uses it on the host
//   bounds      host only: [UPSTREAM] img_bounds undistorts the four corners; here every border pixel, so that a pincushion lens,
//               whose extremes lie at the mid-edges, is covered too
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LP_RADTAN_FN __host__ __device__ __forceinline__
#else
#define LP_RADTAN_FN inline
#endif

namespace lpslam_radtan {

struct Model { double fx, fy, cx, cy, k1, k2, p1, p2, k3; };
struct Bounds { double min_x, max_x, min_y, max_y; };          // undistorted pixel positions of the valid border pixels

constexpr int kIterations = 5;
constexpr double kMaxResidual2 = 0.25;                         // (0.5 pixel)^2

// normalised (x, y) -> normalised distorted (xd, yd)
LP_RADTAN_FN void distort(const Model& m, double x, double y, double* xd, double* yd)
{
    const double r2 = x * x + y * y;
    const double rad = 1.0 + ((m.k3 * r2 + m.k2) * r2 + m.k1) * r2;
    *xd = x * rad + 2.0 * m.p1 * x * y + m.p2 * (r2 + 2.0 * x * x);
    *yd = y * rad + m.p1 * (r2 + 2.0 * y * y) + 2.0 * m.p2 * x * y;
}

// The undistorted (pinhole, same K) position of sensor pixel (px, py), rounded to float32 once at the end.  false: the point is
// invalid and *ux, *uy are not written.  *res2_out (may be null) receives the squared distance in pixels between the input and the
// forward model of the result, *min_den_out (may be null) the smallest denominator of the five steps.
LP_RADTAN_FN bool undistort(const Model& m, double px, double py, float* ux, float* uy, double* res2_out = nullptr, double* min_den_out = nullptr)
{
    const double x0 = (px - m.cx) / m.fx, y0 = (py - m.cy) / m.fy;
    double x = x0, y = y0, min_den = INFINITY;
    bool positive = true;
    for (int it = 0; it < kIterations; ++it) {
        const double r2 = x * x + y * y;
        const double den = 1.0 + ((m.k3 * r2 + m.k2) * r2 + m.k1) * r2;
        const double dx = 2.0 * m.p1 * x * y + m.p2 * (r2 + 2.0 * x * x);
        const double dy = m.p1 * (r2 + 2.0 * y * y) + 2.0 * m.p2 * x * y;
        positive = positive && den > 0.0;                      // (a NaN fails the comparison)
        min_den = den < min_den ? den : min_den;
        x = (x0 - dx) / den; y = (y0 - dy) / den;
    }
    double xd, yd;
    distort(m, x, y, &xd, &yd);
    const double ex = m.fx * xd + m.cx - px, ey = m.fy * yd + m.cy - py, res2 = ex * ex + ey * ey;
    if (res2_out) *res2_out = res2;
    if (min_den_out) *min_den_out = min_den;
    const double rx = m.fx * x + m.cx, ry = m.fy * y + m.cy;
    if (!(positive && res2 <= kMaxResidual2 && isfinite(rx) && isfinite(ry))) return false;      // (a NaN residual fails the comparison)
    *ux = (float)rx; *uy = (float)ry;
    return true;
}

// The sensor pixel of camera-frame point (X, Y, Z), Z > 0.
LP_RADTAN_FN void forward(const Model& m, double X, double Y, double Z, double* sx, double* sy)
{
    double xd, yd;
    distort(m, X / Z, Y / Z, &xd, &yd);
    *sx = m.fx * xd + m.cx; *sy = m.fy * yd + m.cy;
}

// Host only from here on (plain inline functions).
// The bounds of the undistorted image: min and max of x and of y over the valid border pixels of the width x height image.  false: no
// border pixel is valid.  *n_invalid / *n_border (may be null): how many border pixels were invalid, of how many.
inline bool bounds(const Model& m, int width, int height, Bounds* out, long* n_invalid = nullptr, long* n_border = nullptr)
{
    Bounds b{INFINITY, -INFINITY, INFINITY, -INFINITY};
    long bad = 0, all = 0;
    auto take = [&](int px, int py) {
        float ux, uy;
        ++all;
        if (!undistort(m, (double)px, (double)py, &ux, &uy)) { ++bad; return; }
        b.min_x = fmin(b.min_x, (double)ux); b.max_x = fmax(b.max_x, (double)ux);
        b.min_y = fmin(b.min_y, (double)uy); b.max_y = fmax(b.max_y, (double)uy);
    };
    for (int px = 0; px < width; ++px) { take(px, 0); if (height > 1) take(px, height - 1); }
    for (int py = 1; py < height - 1; ++py) { take(0, py); if (width > 1) take(width - 1, py); }
    if (n_invalid) *n_invalid = bad;
    if (n_border) *n_border = all;
    if (all == bad) return false;
    *out = b;
    return true;
}
// Visible: in front of the camera, the pinhole (u, v) inside the bounds -- which is what rejects a far off-axis point that the polynomial
// folds back into the image -- and the SENSOR pixel inside the width x height image.
inline bool visible(const Model& m, const Bounds& b, double X, double Y, double Z, int width, int height)
{
    if (!(Z > 0.0)) return false;
    const double u = m.fx * X / Z + m.cx, v = m.fy * Y / Z + m.cy;
    if (!(u >= b.min_x && u <= b.max_x && v >= b.min_y && v <= b.max_y)) return false;
    double sx, sy;
    forward(m, X, Y, Z, &sx, &sy);
    return sx >= 0.0 && sx < (double)width && sy >= 0.0 && sy < (double)height;
}
// a model the library accepts: finite values, positive focal lengths
inline bool model_ok(const Model& m)
{
    const double v[9] = {m.fx, m.fy, m.cx, m.cy, m.k1, m.k2, m.p1, m.p2, m.k3};
    for (double d : v) if (!isfinite(d)) return false;
    return m.fx > 0.0 && m.fy > 0.0;
}
// all five coefficients exactly 0: no model (an ideal pinhole camera)
inline bool is_identity(const Model& m) { return m.k1 == 0.0 && m.k2 == 0.0 && m.p1 == 0.0 && m.p2 == 0.0 && m.k3 == 0.0; }

}  // namespace lpslam_radtan
