// The JPEG decoder the replay reader and the manager's ingest use: the device decoder (lpslam_hip_jpeg_decode, csrc/jpeg_dec.hip) for the
// streams it takes, the host decoder (jpeg.h) for every other one -- a stream the device leaves to the host ("not taken"), one it
// calls irregular (the host decoder gives the verdict), and everything when there is no device or the device path is switched off
// ("manager": {"jpeg_decode_device": false}).  Three-component streams of the class the device takes (jpeg::interleaved_ycc_scan:
// 4:4:4, 4:2:2, 4:2:0 in one interleaved scan) are offered to it too unless "manager": {"jpeg_decode_color_device": false} is set; the
// device object is made for colour (three times the memory) at the first such stream, not before.  Either way the samples are those
// of decode_jpeg_gray.  Streams of either class with a restart interval go to the host unless "manager":
// {"jpeg_decode_restart_device": true} is set (setUseDeviceForRestart; off by default).
#pragma once
#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>

#include "core.h"

struct lpslam_hip_jpeg_dec;

namespace LpSlam {

struct JpegDecodeCounters { uint64_t device_images = 0, host_images = 0, refused_images = 0; };

class JpegDecoder {
public:
    JpegDecoder() = default;
    ~JpegDecoder();
    JpegDecoder(const JpegDecoder&) = delete;
    JpegDecoder& operator=(const JpegDecoder&) = delete;
    void setUseDevice(bool on);
    void setUseDeviceForColor(bool on);        // false: three-component streams go to the host decoder
    void setUseDeviceForRestart(bool on);      // true: streams with a restart interval are offered to the device too
    // n = 1 or 2 streams (the two eyes of a record) in one device call; ok[i] says whether outs[i] holds an image, why[i] (optional) what
    // the host decoder said when it does not.  Returns true when every stream was decoded.
    bool decode(int n, const uint8_t* const* data, const size_t* sizes, GrayImage* const* outs, bool* ok, std::string* why = nullptr);
    JpegDecodeCounters counters() const;
private:
    std::mutex m_mutex;
    lpslam_hip_jpeg_dec* m_dec = nullptr;      // created at the first stream, regrown when a larger frame comes
    int m_decW = 0, m_decH = 0;
    bool m_decColor = false;                   // m_dec was made with LPSLAM_HIP_JPEG_DEC_COLOR
    bool m_useDevice = true, m_useDeviceForColor = true, m_useDeviceForRestart = false;
    std::atomic<uint64_t> m_deviceImages{0}, m_hostImages{0}, m_refusedImages{0};
};

}  // namespace LpSlam
