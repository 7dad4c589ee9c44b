// intensity.h -- the AdjustIntensity processor (mirror of the reference's src/Processor/AdjustIntensityProcessor.h:10-41) and the host
// implementation of its arithmetic, ImageProcessing::imadjust(image, out, nullopt, nullopt, -0.3, 1.4) of
// src/Utils/ImageProcessing.h:258-370 on each eye.  DESIGN.md section 17 states the arithmetic; the device kernels
// (lpslam_amd/csrc/intensity.hip) compute the same bytes.
//
// The processor does not touch the pixels: it leaves a request on the CameraQueueEntry (core.h, IntensityAdjust).  A HIP tracker
// applies it on the device, behind the frame's upload; everything else that reads the pixels after the processors -- the recorder, a
// later processor, a tracker that is not one of ours -- calls realiseAdjust() first, which applies it here, once, and clears it.
#pragma once
#include "core.h"

namespace LpSlam {

// true: the parameters are ones adjust_intensity_host accepts (low_out < high_out, both finite; 0 <= low_fraction < high_fraction <= 1)
bool intensity_params_valid(const IntensityAdjust& p);

// In place on `rows` of `width` pixels, `stride` bytes apart.  lo_hi (may be null) receives the two limits.  false: invalid
// parameters or width * height >= 2^24 (the reference sums the histogram walk through a float, exact below that), nothing is written.
bool adjust_intensity_host(uint8_t* pixels, int width, int height, size_t stride, const IntensityAdjust& p, int* lo_hi = nullptr);
inline bool adjust_intensity_host(GrayImage& img, const IntensityAdjust& p, int* lo_hi = nullptr)
{
    return adjust_intensity_host(img.pixels.data(), img.width, img.height, (size_t)img.width, p, lo_hi);
}

// applies a pending request to both eyes and clears it (no request: nothing happens)
void realiseAdjust(CameraQueueEntry& cam);

class AdjustIntensityProcessor : public ProcessorBase {
public:
    // empty, or an object with the optional numbers lowOut, highOut, lowFraction, highFraction (keys that start with '_' are ignored)
    bool setConfig(std::string const& jsonConfig) override;
    // a request that is still pending (an earlier AdjustIntensity entry) is applied on the host first: this one adjusts the adjusted frame
    void processImage(CameraQueueEntry& cam) override { realiseAdjust(cam); cam.adjust = m_params; }
    bool readsPixels() const override { return false; }
    std::string type() override { return "AdjustIntensity"; }
    const IntensityAdjust& params() const { return m_params; }

private:
    IntensityAdjust m_params;
};

}  // namespace LpSlam
