// record.h -- the recorder: a live session written to lpslam's recording stream, the file replay.h reads (mirror of the reference's
// /root/reference/src/Manager/RecordEngine.{h,cpp}, wired as in src/Manager/SlamManager.cpp:104,187,216,565-572,608,642-666).
//
// Records are `u64 type | u64 size | payload`, the payload a proto3 message of the reference's src/Serialize/SlamSerialize.proto in the
// canonical encoding the C++ protobuf writer produces (fields in number order, scalars equal to their default omitted, sub-messages the
// reference sets always present), written by a few lines of wire encoding here (no protoc in the image).  INTEGRATION.md ("Recording
// file") lists every field.  Camera records (type 1) hold the frame's images as JPEG at quality 95 -- cv::imencode(".jpg") in the
// reference (RecordEngine.cpp:93) -- encoded by the device encoder (lpslam_hip_jpeg_*) when a HIP device is present, by the host
// encoder (jpeg.h) otherwise: the two write the same bytes.  Result records (type 4) hold every pose a tracker returned.  Encoding and
// writing happen on the recorder's own thread; stop() writes everything queued before it (RecordEngine.cpp:330-350).
#pragma once
#include "core.h"

#include <atomic>
#include <fstream>
#include <string>
#include <thread>

struct lpslam_hip_jpeg;

namespace LpSlam {

struct RecorderCounters {
    uint64_t device_images = 0, host_images = 0;      // images encoded by the device / the host encoder
    uint64_t records = 0, bytes = 0;                  // records and bytes written to the recording stream
};

class Recorder {
public:
    Recorder() = default;
    ~Recorder() { stop(); }

    void setStoreImages(bool b) { m_storeImages = b; }            // RecordEngine::setStoreImages: false drops the camera records
    void setWriteRawFile(bool b) { m_writeRawFile = b; }          // record_raw: NNNNNN_left.jpg / NNNNNN_right.jpg beside the stream

    // record: open slam_%Y-%m-%d_%H-%M-%S.pb (local time) in the working directory; imageFiles: the thread also serves
    // SlamManager::setWriteImageFiles.  Neither: nothing is created.
    void start(bool record, bool imageFiles);
    void stop();                                      // drains the queue, then flushes and closes the file
    bool active() const { return m_thread.joinable(); }
    bool recording() const { return m_recording; }
    const std::string& fileName() const { return m_fileName; }

    // worker thread: the frame is copied; imageFileNumber >= 0 also writes <n>_left.jpg / <n>_right.jpg
    void storeCameraImage(const CameraQueueEntry& cam, const std::optional<GlobalStateInTime>& odom, const std::optional<GlobalStateInTime>& map,
                          int64_t imageFileNumber);
    void storeResult(const GlobalStateInTime& result);

    RecorderCounters counters() const;

private:
    struct Entry {
        enum class Type { Exit, Camera, Result } type = Type::Exit;
        bool record = false;                          // a camera record (setStoreImages), else image files only
        int64_t imageFileNumber = -1;
        CameraQueueEntry camera;
        std::optional<GlobalState> odom, map;
        GlobalStateInTime result;
    };
    void run();
    void encode(const CameraQueueEntry& cam, std::vector<uint8_t>& left, std::vector<uint8_t>& right);
    void writeRecord(uint64_t type, const std::string& payload);

    BlockingQueue<Entry> m_q;
    std::thread m_thread;
    std::ofstream m_out;                              // recorder thread only between start() and stop()
    bool m_recording = false;                         // the file is open: fixed at start(), read by the worker thread
    std::string m_fileName;
    std::atomic<bool> m_storeImages{true}, m_writeRawFile{false};
    uint32_t m_imgCount = 0;                          // camera records written (NNNNNN of the raw files), as RecordEngine::m_imgCount
    bool m_useDevice = false;
    lpslam_hip_jpeg* m_enc = nullptr;                 // recorder thread only
    int m_encW = 0, m_encH = 0;
    std::atomic<uint64_t> m_deviceImages{0}, m_hostImages{0}, m_records{0}, m_bytes{0};
};

// the proto3 payloads of the two record types this library writes
std::string serializeCameraImage(int64_t timestamp_ns, const std::vector<uint8_t>& image, uint32_t camera, const std::vector<uint8_t>* image_second,
                                 uint32_t camera_second, const std::optional<GlobalState>& odom, const std::optional<GlobalState>& map);
std::string serializeResult(const GlobalStateInTime& result);

}  // namespace LpSlam
