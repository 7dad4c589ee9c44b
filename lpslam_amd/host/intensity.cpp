// intensity.cpp -- see intensity.h.
#include "intensity.h"
#include "ingest.h"

#include <cmath>

namespace LpSlam {

bool intensity_params_valid(const IntensityAdjust& p)
{
    return std::isfinite(p.low_out) && std::isfinite(p.high_out) && p.low_out < p.high_out &&
           p.low_fraction >= 0.0 && p.low_fraction < p.high_fraction && p.high_fraction <= 1.0;
}

bool adjust_intensity_host(uint8_t* pixels, int width, int height, size_t stride, const IntensityAdjust& p, int* lo_hi)
{
    if (!pixels || width < 1 || height < 1 || stride < (size_t)width || !intensity_params_valid(p)) return false;
    const size_t N = (size_t)width * (size_t)height;
    if (N >= ((size_t)1 << 24)) return false;
    uint32_t hist[256] = {0};
    for (int y = 0; y < height; ++y) {
        const uint8_t* row = pixels + (size_t)y * stride;
        for (int x = 0; x < width; ++x) ++hist[row[x]];
    }
    const uint32_t low_count = (uint32_t)(p.low_fraction * (double)N), high_count = (uint32_t)((1.0 - p.high_fraction) * (double)N);
    // the walks test before they add: a bin is reached with the sum of the bins walked so far
    int lo = 0, hi = 1;
    uint32_t sum = 0;
    for (int i = 0; i < 256; ++i) { if (sum >= low_count) { lo = i; break; } sum += hist[i]; }
    sum = 0;
    for (int i = 255; i >= 0; --i) { if (sum >= high_count) { hi = i; break; } sum += hist[i]; }
    if (lo_hi) { lo_hi[0] = lo; lo_hi[1] = hi; }
    if (lo == hi) return true;          // alpha would be infinite (the reference's result is unspecified): the image stays as it is
    const double lo_n = (double)lo / 255.0, hi_n = (double)hi / 255.0;
    const double alpha = (p.high_out - p.low_out) / (hi_n - lo_n);
    const double beta = (p.high_out - hi_n * alpha) * 255.0;
    const float a = (float)alpha, b = (float)beta;
    uint8_t table[256];
    for (int x = 0; x < 256; ++x) {
        // single precision, product and sum unfused (the library is compiled with -ffp-contract=off; volatile keeps the rounded
        // product a value of its own whatever the flags), round half to even (the default rounding mode), saturate
        volatile float prod = (float)x * a;
        const float v = std::nearbyintf(prod + b);
        table[x] = (uint8_t)(v > 0.0f ? (v >= 255.0f ? 255.0f : v) : 0.0f);
    }
    for (int y = 0; y < height; ++y) {
        uint8_t* row = pixels + (size_t)y * stride;
        for (int x = 0; x < width; ++x) row[x] = table[row[x]];
    }
    return true;
}

void realiseAdjust(CameraQueueEntry& cam)
{
    if (!cam.adjust) return;
    realiseGray(cam);                   // the adjustment works on the grey image
    const IntensityAdjust p = *cam.adjust;
    cam.adjust.reset();
    if (!cam.image.empty() && !adjust_intensity_host(cam.image, p))
        logMessage(LpSlamLogLevel_Error, "AdjustIntensity: frame of " + std::to_string(cam.image.width) + " x " + std::to_string(cam.image.height) + " pixels not adjusted");
    if (cam.image_second && !cam.image_second->empty() && !adjust_intensity_host(*cam.image_second, p))
        logMessage(LpSlamLogLevel_Error, "AdjustIntensity: second image not adjusted");
}

bool AdjustIntensityProcessor::setConfig(std::string const& jsonConfig)
{
    ConfigOptions o;
    const IntensityAdjust d;
    o.optional("lowOut", d.low_out); o.optional("highOut", d.high_out);
    o.optional("lowFraction", d.low_fraction); o.optional("highFraction", d.high_fraction);
    try { o.parse(jsonConfig); }
    catch (std::exception& ex) { logMessage(LpSlamLogLevel_Error, std::string("Cannot parse config due to error: ") + ex.what()); return false; }
    IntensityAdjust p;
    p.low_out = o.getDouble("lowOut"); p.high_out = o.getDouble("highOut");
    p.low_fraction = o.getDouble("lowFraction"); p.high_fraction = o.getDouble("highFraction");
    if (!intensity_params_valid(p)) {
        logMessage(LpSlamLogLevel_Error, "AdjustIntensity needs lowOut < highOut and 0 <= lowFraction < highFraction <= 1");
        return false;
    }
    m_params = p;
    return true;
}

}  // namespace LpSlam
