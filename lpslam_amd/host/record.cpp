// record.cpp -- see record.h.
#include "record.h"
#include "jpeg.h"
#include "../../include/lpslam_hip.h"

#include <cstdio>
#include <cstring>
#include <ctime>
#include <iomanip>
#include <sstream>

namespace LpSlam {

namespace {
// ---- proto3 wire encoding (canonical: fields in number order, default scalars omitted) ------------------------------------------
void putVarint(std::string& o, uint64_t v)
{
    while (v >= 0x80) { o.push_back((char)(uint8_t)(v | 0x80)); v >>= 7; }
    o.push_back((char)(uint8_t)v);
}
void putTag(std::string& o, int field, int wire) { putVarint(o, ((uint64_t)field << 3) | (uint64_t)wire); }
void putDouble(std::string& o, int field, double v)
{
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    if (bits == 0) return;                            // +0.0 is the default (-0.0 is not: the writer compares bit patterns)
    putTag(o, field, 1);
    for (int i = 0; i < 8; ++i) o.push_back((char)(uint8_t)(bits >> (8 * i)));
}
void putInt64(std::string& o, int field, int64_t v) { if (v) { putTag(o, field, 0); putVarint(o, (uint64_t)v); } }
void putInt32(std::string& o, int field, int32_t v) { if (v) { putTag(o, field, 0); putVarint(o, (uint64_t)(int64_t)v); } }     // negative: 10 bytes, as protobuf
void putBool(std::string& o, int field, bool v) { if (v) { putTag(o, field, 0); putVarint(o, 1); } }
void putBytes(std::string& o, int field, const void* p, size_t n)
{
    if (!n) return;
    putTag(o, field, 2); putVarint(o, n); o.append(static_cast<const char*>(p), n);
}
void putMessage(std::string& o, int field, const std::string& m) { putTag(o, field, 2); putVarint(o, m.size()); o += m; }     // set sub-messages are always written

std::string position(const Position3& p)              // message Position
{
    std::string o;
    putDouble(o, 1, p.value.x); putDouble(o, 2, p.value.y); putDouble(o, 3, p.value.z);
    putDouble(o, 4, p.sigma.x); putDouble(o, 5, p.sigma.y); putDouble(o, 6, p.sigma.z);
    return o;
}
std::string orientation(const Orientation& q)         // message Orientation
{
    std::string o;
    putDouble(o, 1, q.value.w); putDouble(o, 2, q.value.x); putDouble(o, 3, q.value.y); putDouble(o, 4, q.value.z); putDouble(o, 5, q.sigma);
    return o;
}
// message GlobalState as RecordEngine.cpp:41-75 fills it: position, orientation and an empty velocity (this library has none);
// velocityValid stays false
std::string globalState(const GlobalState& s, bool velocity)
{
    std::string o;
    putMessage(o, 1, position(s.position));
    putMessage(o, 2, orientation(s.orientation));
    if (velocity) putMessage(o, 3, std::string());
    return o;
}
std::string identityBase()                            // message TrackerCoordinateSystem of the identity base (SlamManager.cpp:1065-1073)
{
    std::string o;
    putMessage(o, 1, position(Position3{}));
    putMessage(o, 2, orientation(Orientation{}));
    return o;
}

bool writeFile(const std::string& name, const std::vector<uint8_t>& data)
{
    FILE* f = std::fopen(name.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(data.data(), 1, data.size(), f) == data.size();
    return std::fclose(f) == 0 && ok;
}
}  // namespace

std::string serializeCameraImage(int64_t timestamp_ns, const std::vector<uint8_t>& image, uint32_t camera, const std::vector<uint8_t>* image_second,
                                 uint32_t camera_second, const std::optional<GlobalState>& odom, const std::optional<GlobalState>& map)
{
    std::string o;
    putInt64(o, 1, timestamp_ns);
    putBytes(o, 3, image.data(), image.size());                                   // dataNumber (2) is never set by the reference
    putMessage(o, 4, globalState(odom.value_or(GlobalState{}), true));
    putMessage(o, 5, globalState(map.value_or(GlobalState{}), true));
    putInt32(o, 6, (int32_t)camera);
    if (image_second) {
        putBytes(o, 7, image_second->data(), image_second->size());
        putInt32(o, 8, (int32_t)camera_second);
    }
    putMessage(o, 9, identityBase());
    if (image_second) putMessage(o, 10, identityBase());
    putBool(o, 11, odom.has_value());
    putBool(o, 12, map.has_value());
    return o;
}

std::string serializeResult(const GlobalStateInTime& r)      // message GlobalStateInTime (RecordEngine.cpp:242-254: no velocity)
{
    std::string o;
    putInt64(o, 1, timeStampToInt64(r.first.system_time));
    putMessage(o, 2, globalState(r.second, false));
    return o;
}

void Recorder::start(bool record, bool imageFiles)
{
    if (active() || (!record && !imageFiles)) return;
    if (record) {
        const std::time_t now = std::time(nullptr);
        const std::tm tm = *std::localtime(&now);
        std::ostringstream name;
        name << "slam_" << std::put_time(&tm, "%Y-%m-%d_%H-%M-%S") << ".pb";
        m_fileName = name.str();
        m_out.open(m_fileName, std::ios::binary | std::ios::trunc);
        if (!m_out) logMessage(LpSlamLogLevel_Error, "Cannot open recording file " + m_fileName);
        else logMessage(LpSlamLogLevel_Info, "Recording to " + m_fileName);
        m_recording = m_out.is_open();
    }
    int devices = 0;
    m_useDevice = lpslam_hip_device_count(&devices) == LPSLAM_HIP_OK && devices > 0;
    m_thread = std::thread([this] { run(); });
}

void Recorder::stop()
{
    if (!active()) return;
    m_q.push(Entry{});                                // every entry queued before the exit marker is written
    m_thread.join();
    m_q.clear();
    m_recording = false;
    if (m_out.is_open()) { m_out.flush(); m_out.close(); }
    if (m_enc) { lpslam_hip_jpeg_destroy(m_enc); m_enc = nullptr; m_encW = m_encH = 0; }
}

void Recorder::storeCameraImage(const CameraQueueEntry& cam, const std::optional<GlobalStateInTime>& odom, const std::optional<GlobalStateInTime>& map,
                                int64_t imageFileNumber)
{
    const bool record = m_recording && m_storeImages.load();                   // RecordEngine.cpp:277
    if (!active() || (!record && imageFileNumber < 0) || cam.image.empty()) return;
    Entry e;
    e.type = Entry::Type::Camera; e.record = record; e.imageFileNumber = imageFileNumber;
    e.camera.valid = true; e.camera.timestamp = cam.timestamp;
    e.camera.cameraNumber = cam.cameraNumber; e.camera.cameraNumberSecond = cam.cameraNumberSecond;
    e.camera.image = cam.image;                                                    // a copy: the worker recycles its frame buffers
    e.camera.image_second = cam.image_second;
    if (odom) e.odom = odom->second;
    if (map) e.map = map->second;
    m_q.push(std::move(e));
}

void Recorder::storeResult(const GlobalStateInTime& result)
{
    if (!m_recording) return;
    Entry e;
    e.type = Entry::Type::Result; e.result = result;
    m_q.push(std::move(e));
}

RecorderCounters Recorder::counters() const
{
    RecorderCounters c;
    c.device_images = m_deviceImages.load(); c.host_images = m_hostImages.load(); c.records = m_records.load(); c.bytes = m_bytes.load();
    return c;
}

// both eyes in one device call; the host encoder where no device is present (or the device encoder cannot be made: logged)
void Recorder::encode(const CameraQueueEntry& cam, std::vector<uint8_t>& left, std::vector<uint8_t>& right)
{
    const int quality = 95;                                                        // cv::imencode's default (RecordEngine.cpp:93)
    const GrayImage* imgs[2] = {&cam.image, cam.image_second ? &*cam.image_second : nullptr};
    std::vector<uint8_t>* outs[2] = {&left, &right};
    const int n = imgs[1] ? 2 : 1;
    if (m_useDevice) {
        int w = 0, h = 0;
        for (int i = 0; i < n; ++i) { w = std::max(w, imgs[i]->width); h = std::max(h, imgs[i]->height); }
        if (!m_enc || w > m_encW || h > m_encH) {
            if (m_enc) lpslam_hip_jpeg_destroy(m_enc);
            m_enc = nullptr;
            m_encW = std::max(w, m_encW); m_encH = std::max(h, m_encH);
            if (lpslam_hip_jpeg_create(m_encW, m_encH, 2, &m_enc) != LPSLAM_HIP_OK) {
                logMessage(LpSlamLogLevel_Error, std::string("Recorder: the device JPEG encoder cannot be created, encoding on the host: ") + lpslam_hip_last_error());
                m_enc = nullptr; m_useDevice = false;
            }
        }
        if (m_enc) {
            const uint8_t* px[2]; int32_t ws[2], hs[2]; uint8_t* o[2]; int64_t caps[2], sizes[2] = {0, 0};
            for (int i = 0; i < n; ++i) {
                px[i] = imgs[i]->pixels.data();
                ws[i] = imgs[i]->width; hs[i] = imgs[i]->height;
                outs[i]->resize((size_t)imgs[i]->width * imgs[i]->height + 4096);  // a first guess: a stream of 8 bits per sample or less
                o[i] = outs[i]->data(); caps[i] = (int64_t)outs[i]->size();
            }
            int rc = lpslam_hip_jpeg_encode(m_enc, n, px, ws, hs, ws, quality, o, caps, sizes);
            if (rc == LPSLAM_HIP_ERR_INVALID && sizes[0] > 0) {                    // noise-like images: the stream is larger than the guess
                for (int i = 0; i < n; ++i) { outs[i]->resize((size_t)std::max<int64_t>(sizes[i], 1)); o[i] = outs[i]->data(); caps[i] = (int64_t)outs[i]->size(); }
                rc = lpslam_hip_jpeg_encode(m_enc, n, px, ws, hs, ws, quality, o, caps, sizes);
            }
            if (rc == LPSLAM_HIP_OK) {
                for (int i = 0; i < n; ++i) outs[i]->resize((size_t)sizes[i]);
                m_deviceImages += (uint64_t)n;
                return;
            }
            logMessage(LpSlamLogLevel_Error, std::string("Recorder: device JPEG encoding failed, encoding on the host: ") + lpslam_hip_last_error());
        }
    }
    for (int i = 0; i < n; ++i) encode_jpeg_gray(*imgs[i], quality, *outs[i]);
    m_hostImages += (uint64_t)n;
}

void Recorder::writeRecord(uint64_t type, const std::string& payload)
{
    const uint64_t head[2] = {type, (uint64_t)payload.size()};                   // ProtoStream.h: u64 type, u64 size (host byte order)
    m_out.write(reinterpret_cast<const char*>(head), sizeof(head));
    m_out.write(payload.data(), (std::streamsize)payload.size());
    ++m_records;
    m_bytes += sizeof(head) + payload.size();
}

void Recorder::run()
{
    std::vector<uint8_t> left, right;
    for (;;) {
        Entry e;
        m_q.pop(e);
        if (e.type == Entry::Type::Exit) return;
        if (e.type == Entry::Type::Result) { writeRecord(4, serializeResult(e.result)); continue; }      // Serialization::Result
        const CameraQueueEntry& c = e.camera;
        encode(c, left, right);
        const bool stereo = c.image_second.has_value();
        if (e.record) {
            writeRecord(1, serializeCameraImage(timeStampToInt64(c.timestamp), left, c.cameraNumber, stereo ? &right : nullptr, c.cameraNumberSecond,
                                                e.odom, e.map));                                         // Serialization::CameraImage
            if (m_writeRawFile.load()) {                                                                 // RecordEngine.cpp:138-156
                char num[32];
                std::snprintf(num, sizeof(num), "%06u", (unsigned)m_imgCount);
                writeFile(std::string(num) + "_left.jpg", left);
                if (stereo) writeFile(std::string(num) + "_right.jpg", right);
            }
            ++m_imgCount;
        }
        if (e.imageFileNumber >= 0) {                                                                    // SlamManager.cpp:70-85
            writeFile(std::to_string(e.imageFileNumber) + "_left.jpg", left);
            if (stereo) writeFile(std::to_string(e.imageFileNumber) + "_right.jpg", right);
        }
    }
}

}  // namespace LpSlam
