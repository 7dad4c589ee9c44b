// jpeg_device.cpp -- see jpeg_device.h
#include "jpeg_device.h"
#include "jpeg.h"
#include "../../include/lpslam_hip.h"

#include <algorithm>

namespace LpSlam {

JpegDecoder::~JpegDecoder() { if (m_dec) lpslam_hip_jpeg_dec_destroy(m_dec); }

void JpegDecoder::setUseDevice(bool on)
{
    std::lock_guard<std::mutex> l(m_mutex);
    m_useDevice = on;
    if (!on && m_dec) { lpslam_hip_jpeg_dec_destroy(m_dec); m_dec = nullptr; }
}

void JpegDecoder::setUseDeviceForColor(bool on)
{
    std::lock_guard<std::mutex> l(m_mutex);
    m_useDeviceForColor = on;
    // a device object made for colour would still take such a stream: the next one is made for grey
    if (!on && m_dec && m_decColor) { lpslam_hip_jpeg_dec_destroy(m_dec); m_dec = nullptr; }
    if (!on) m_decColor = false;
}

void JpegDecoder::setUseDeviceForRestart(bool on)
{
    std::lock_guard<std::mutex> l(m_mutex);
    m_useDeviceForRestart = on;
    if (m_dec) lpslam_hip_jpeg_dec_take_restart(m_dec, on ? 1 : 0);
}

JpegDecodeCounters JpegDecoder::counters() const
{
    JpegDecodeCounters c;
    c.device_images = m_deviceImages.load(); c.host_images = m_hostImages.load(); c.refused_images = m_refusedImages.load();
    return c;
}

bool JpegDecoder::decode(int n, const uint8_t* const* data, const size_t* sizes, GrayImage* const* outs, bool* ok, std::string* why)
{
    std::lock_guard<std::mutex> l(m_mutex);
    n = std::min(n, 2);
    for (int i = 0; i < n; ++i) ok[i] = false;
    if (m_useDevice) {
        // the frame sizes, from the headers: the decoder is sized by the first record and regrown when a larger frame comes
        int w = 0, h = 0, X[2] = {0, 0}, Y[2] = {0, 0};
        bool color = false;
        for (int i = 0; i < n; ++i) {
            if (!looks_like_jpeg(data[i], sizes[i])) continue;
            jpeg::Header hd; jpeg::Scan sc; size_t pos = 2;
            if (jpeg::walk_to_scan(data[i], sizes[i], pos, hd, sc, nullptr) != jpeg::Walk::scan) continue;
            const bool ycc = m_useDeviceForColor && jpeg::interleaved_ycc_scan(hd, sc, m_useDeviceForRestart);
            if (!jpeg::grey_scan(hd, m_useDeviceForRestart) && !ycc) continue;    // the device would answer "not taken"
            color = color || ycc;
            X[i] = hd.X; Y[i] = hd.Y;
            w = std::max(w, hd.X); h = std::max(h, hd.Y);
        }
        if (w > 0 && (!m_dec || w > m_decW || h > m_decH || (color && !m_decColor))) {
            if (m_dec) lpslam_hip_jpeg_dec_destroy(m_dec);
            m_dec = nullptr;
            m_decW = std::max(w, m_decW); m_decH = std::max(h, m_decH); m_decColor = m_decColor || color;
            if (lpslam_hip_jpeg_dec_create2(m_decW, m_decH, 2, m_decColor ? LPSLAM_HIP_JPEG_DEC_COLOR : 0u, &m_dec) != LPSLAM_HIP_OK) {
                logMessage(LpSlamLogLevel_Info, std::string("The device JPEG decoder cannot be created, decoding on the host: ") + lpslam_hip_last_error());
                m_dec = nullptr; m_useDevice = false;
            } else if (m_useDeviceForRestart) {
                lpslam_hip_jpeg_dec_take_restart(m_dec, 1);
            }
        }
        if (m_dec && w > 0) {
            const uint8_t* streams[2]; int64_t stream_sizes[2]; uint8_t* o[2]; int32_t strides[2], ws[2], hs[2], status[2]; int64_t caps[2];
            for (int i = 0; i < n; ++i) {                                              // rows land tightly packed
                streams[i] = data[i]; stream_sizes[i] = (int64_t)sizes[i];
                outs[i]->pixels.resize(std::max<size_t>(1, (size_t)X[i] * Y[i]));
                o[i] = outs[i]->pixels.data(); caps[i] = (int64_t)outs[i]->pixels.size();
                strides[i] = std::max(1, X[i]);
            }
            if (lpslam_hip_jpeg_decode(m_dec, n, streams, stream_sizes, o, strides, caps, ws, hs, status) == LPSLAM_HIP_OK) {
                for (int i = 0; i < n; ++i)
                    if (status[i] == LPSLAM_HIP_JPEG_DECODED) {
                        outs[i]->width = ws[i]; outs[i]->height = hs[i];
                        outs[i]->pixels.resize((size_t)ws[i] * hs[i]);
                        ok[i] = true; ++m_deviceImages;
                    }
            } else {
                logMessage(LpSlamLogLevel_Error, std::string("Device JPEG decoding failed, decoding on the host: ") + lpslam_hip_last_error());
            }
        }
    }
    bool all = true;
    for (int i = 0; i < n; ++i) {
        if (ok[i]) continue;
        ok[i] = decode_jpeg_gray(data[i], sizes[i], *outs[i], why ? &why[i] : nullptr);
        if (ok[i]) ++m_hostImages; else { ++m_refusedImages; all = false; }
    }
    return all;
}

}  // namespace LpSlam
