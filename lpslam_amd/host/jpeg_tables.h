// jpeg_tables.h -- what the host encoder (jpeg.cpp, encode_jpeg_gray) and the device encoder (csrc/jpeg.hip) share: the tables
// cv::imencode(".jpg", grey) asks libjpeg for -- one component, baseline, the standard (ITU-T T.81 Annex K) luminance quantisation
// and Huffman tables, quality scaling as jpeg_quality_scaling + force_baseline -- and the marker segments in front of the entropy-coded
// data (SOI, JFIF APP0, DQT, SOF0, DHT x 2, SOS).  Header-only: the HIP library and the host library both compile it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace LpSlam {
namespace jpeg {

inline constexpr uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
inline constexpr uint8_t kStdLumQuant[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
inline constexpr uint8_t kDcLumBits[17] = {0, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
inline constexpr uint8_t kDcLumVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
inline constexpr uint8_t kAcLumBits[17] = {0, 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
inline constexpr uint8_t kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// code and length of every symbol of a Huffman table (T.81 Annex C); symbols the table lacks have length 0
struct EncTable { uint16_t code[256]; uint8_t len[256]; };
inline void make_enc_table(const uint8_t* bits, const uint8_t* vals, EncTable& t)
{
    std::memset(&t, 0, sizeof(t));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l]; ++i, ++k, ++code) { t.code[vals[k]] = (uint16_t)code; t.len[vals[k]] = (uint8_t)l; }
        code <<= 1;
    }
}

// the quantisation table of `quality` (1 .. 100) in natural order: jpeg_quality_scaling, then force_baseline's clamp to 1 .. 255
inline void quant_table(int quality, uint8_t q[64])
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) { long t = ((long)kStdLumQuant[i] * scale + 50) / 100; q[i] = (uint8_t)std::min(255L, std::max(1L, t)); }
}

// SOI .. SOS of a one-component baseline stream of w x h samples (the entropy-coded segment and EOI follow)
inline void write_headers(std::vector<uint8_t>& out, int w, int h, const uint8_t q[64], int restart_interval = 0)
{
    auto put16 = [&](int v) { out.push_back((uint8_t)(v >> 8)); out.push_back((uint8_t)v); };
    auto marker = [&](int m) { out.push_back(0xFF); out.push_back((uint8_t)m); };
    marker(0xD8);
    marker(0xE0); put16(16); for (char c : {'J', 'F', 'I', 'F', '\0'}) out.push_back((uint8_t)c);
    out.push_back(1); out.push_back(1); out.push_back(0); put16(1); put16(1); out.push_back(0); out.push_back(0);      // JFIF 1.01, no density unit, 1:1
    marker(0xDB); put16(67); out.push_back(0); for (int k = 0; k < 64; ++k) out.push_back(q[kZigzag[k]]);
    marker(0xC0); put16(11); out.push_back(8); put16(h); put16(w); out.push_back(1); out.push_back(1); out.push_back(0x11); out.push_back(0);
    marker(0xC4); put16(2 + 1 + 16 + 12); out.push_back(0x00); for (int l = 1; l <= 16; ++l) out.push_back(kDcLumBits[l]); for (uint8_t v : kDcLumVals) out.push_back(v);
    marker(0xC4); put16(2 + 1 + 16 + 162); out.push_back(0x10); for (int l = 1; l <= 16; ++l) out.push_back(kAcLumBits[l]); for (uint8_t v : kAcLumVals) out.push_back(v);
    if (restart_interval > 0) { marker(0xDD); put16(4); put16(restart_interval); }                                     // DRI: where libjpeg writes it
    marker(0xDA); put16(8); out.push_back(1); out.push_back(1); out.push_back(0x00); out.push_back(0); out.push_back(63); out.push_back(0);
}

}  // namespace jpeg
}  // namespace LpSlam
