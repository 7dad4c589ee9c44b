// ingest.h -- colour and YUV frames at ingest: the host implementation of the grey conversion and the pending colour source of a
// CameraQueueEntry (core.h, ColorSource).  DESIGN.md section 29 states the arithmetic; the device kernel
// (lpslam_amd/csrc/ingest.hip) is compiled from the same functions (lpslam_amd/csrc/ingest_math.h) and computes the same bytes.
//
// The manager only copies a colour frame at enqueue and marks the entry pending.  A HIP tracker converts it on the device, behind the
// frame's upload; everybody else who reads the pixels -- the recorder, the image callback, a processor that reads pixels, a tracker that
// is not one of ours -- calls realiseGray() first, which converts here, once, and clears the pending source.  It comes before
// realiseAdjust(): the adjustment works on the grey image.
#pragma once
#include "core.h"

namespace LpSlam {

// Grey image of `width` x `height` pixels, rows `out_stride` bytes apart, from a frame of `format` (LPSLAM_HIP_PIXEL_*) whose rows are
// `stride` bytes apart; chroma / chroma_stride: NV12's interleaved U V rows (nullptr: behind the Y plane, at data + stride * height,
// with its stride).  false: unknown format, an odd size where the format needs an even one, a stride smaller than a row; nothing is
// written.
bool gray_from_pixels_host(uint8_t* out, size_t out_stride, int width, int height, const uint8_t* data, size_t stride,
                           const uint8_t* chroma, size_t chroma_stride, int format);

// converts the pending colour sources of both eyes into `image` / `image_second` and clears them (none pending: nothing happens)
void realiseGray(CameraQueueEntry& cam);

}  // namespace LpSlam
