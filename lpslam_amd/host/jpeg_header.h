// The marker walk of a baseline JPEG file, from the start of the file (or from behind a scan) to the next SOS: DQT, DHT, SOF0 / SOF1,
// DRI and the scan header (ITU-T T.81 Annex B; Huffman decoding tables of Annex C / F.2.2.3 built from the file's own DHT segments).
// Header-only, because the host decoder (host/jpeg.cpp, liblpslam.so) and the device decoder (csrc/jpeg_dec.hip, liblpslam_hip.so)
// both use it: the two cannot disagree about a header.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "jpeg_tables.h"

namespace LpSlam {
namespace jpeg {

struct HuffTable {
    bool present = false;
    uint8_t bits[17] = {0};          // codes of each length 1..16
    uint8_t vals[256] = {0};
    // decoding (T.81 F.2.2.3): smallest / largest code of every length and the index of its first value
    int32_t mincode[17], maxcode[18], valptr[17];
    // 9-bit look-ahead: (length << 8) | symbol, 0 = longer than 9 bits
    uint16_t look[512];
    bool build()
    {
        int code = 0, k = 0;
        std::memset(look, 0, sizeof(look));
        mincode[0] = 0; maxcode[0] = -1; valptr[0] = 0;
        for (int l = 1; l <= 16; ++l) {
            valptr[l] = k; mincode[l] = code;
            for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
                if (k >= 256) return false;
                if (l <= 9) {
                    const int first = code << (9 - l), n = 1 << (9 - l);
                    if (first + n > 512) return false;
                    for (int j = 0; j < n; ++j) look[first + j] = (uint16_t)((l << 8) | vals[k]);
                }
            }
            maxcode[l] = bits[l] ? code - 1 : -1;
            if (code > (1 << l)) return false;                      // over-subscribed
            code <<= 1;
        }
        maxcode[17] = 0x7FFFFFFF;
        return true;
    }
};

struct Component { int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0; int pred = 0; };

// everything the marker segments in front of a scan have said so far
struct Header {
    uint16_t quant[4][64];                       // natural order
    bool have_q[4] = {false, false, false, false};
    bool q16[4] = {false, false, false, false};  // the table came with 16-bit entries (Pq = 1)
    HuffTable dc[4], ac[4];
    Component comp[4];
    int ncomp = 0, X = 0, Y = 0, hmax = 1, vmax = 1, restart_interval = 0;
    int plane_w = 0, plane_h = 0;                // component 0, padded to whole blocks / MCUs
    bool have_frame = false, decoded_luma = false;
};

struct Scan {
    int ns = 0;
    int idx[4] = {0, 0, 0, 0};                   // the components of the scan, in its order
    size_t data = 0;                             // offset of the entropy-coded data
};

enum class Walk { scan, end, error };

inline bool has_soi(const uint8_t* data, size_t size) { return size >= 4 && data[0] == 0xFF && data[1] == 0xD8 && data[2] == 0xFF; }

inline Walk walk_fail(std::string* why, const char* msg) { if (why) *why = msg; return Walk::error; }

// Walks the marker segments from `pos` (2 behind SOI at first) up to and including the next scan header.  Walk::scan: `scan` describes
// it and `pos` is where its entropy-coded data begins; Walk::end: EOI or the end of the file; Walk::error: `why` says what is wrong.
inline Walk walk_to_scan(const uint8_t* d, size_t size, size_t& pos, Header& hd, Scan& scan, std::string* why)
{
    auto u16 = [&](size_t o) { return (int)((d[o] << 8) | d[o + 1]); };
    for (;;) {
        // next marker (skip anything that is not FF, then fill FFs)
        while (pos < size && d[pos] != 0xFF) ++pos;
        while (pos < size && d[pos] == 0xFF) ++pos;
        if (pos >= size) return Walk::end;
        const int m = d[pos++];
        if (m == 0xD9) return Walk::end;                                                // EOI
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0x00) continue;               // stand-alone
        if (pos + 2 > size) return walk_fail(why, "truncated marker segment");
        const int len = u16(pos);
        if (len < 2 || pos + (size_t)len > size) return walk_fail(why, "bad marker segment length");
        const uint8_t* s = d + pos + 2; const int n = len - 2;
        if (m == 0xDB) {                                                               // DQT
            int o = 0;
            while (o < n) {
                const int pq = s[o] >> 4, tq = s[o] & 15; ++o;
                if (tq > 3 || pq > 1 || o + 64 * (pq + 1) > n) return walk_fail(why, "bad quantisation table");
                for (int k = 0; k < 64; ++k) { hd.quant[tq][kZigzag[k]] = pq ? (uint16_t)((s[o] << 8) | s[o + 1]) : s[o]; o += pq + 1; }
                hd.have_q[tq] = true; hd.q16[tq] = pq != 0;
            }
        } else if (m == 0xC4) {                                                        // DHT
            int o = 0;
            while (o < n) {
                if (o + 17 > n) return walk_fail(why, "bad Huffman table");
                const int tc = s[o] >> 4, th = s[o] & 15; ++o;
                if (tc > 1 || th > 3) return walk_fail(why, "bad Huffman table id");
                HuffTable& t = tc ? hd.ac[th] : hd.dc[th];
                int total = 0;
                for (int l = 1; l <= 16; ++l) { t.bits[l] = s[o + l - 1]; total += t.bits[l]; }
                o += 16;
                if (total > 256 || o + total > n) return walk_fail(why, "bad Huffman table size");
                std::memcpy(t.vals, s + o, (size_t)total); o += total;
                if (!t.build()) return walk_fail(why, "inconsistent Huffman table");
                t.present = true;
            }
        } else if (m == 0xC0 || m == 0xC1) {                                           // SOF0 / SOF1: Huffman, sequential
            if (hd.have_frame) return walk_fail(why, "second frame header");
            if (n < 6) return walk_fail(why, "bad frame header");
            if (s[0] != 8) return walk_fail(why, "only 8-bit samples are supported");
            const int Y = u16(pos + 3), X = u16(pos + 5), ncomp = s[5];
            if (X <= 0 || Y <= 0 || (ncomp != 1 && ncomp != 3) || n < 6 + 3 * ncomp) return walk_fail(why, "unsupported frame (size / component count)");
            if ((size_t)X * (size_t)Y > (size_t)1 << 28) return walk_fail(why, "frame too large");
            hd.X = X; hd.Y = Y; hd.ncomp = ncomp;
            for (int i = 0; i < ncomp; ++i) {
                Component& c = hd.comp[i];
                c.id = s[6 + 3 * i]; c.h = s[7 + 3 * i] >> 4; c.v = s[7 + 3 * i] & 15; c.tq = s[8 + 3 * i];
                if (c.h < 1 || c.h > 4 || c.v < 1 || c.v > 4 || c.tq > 3) return walk_fail(why, "bad component description");
                hd.hmax = std::max(hd.hmax, c.h); hd.vmax = std::max(hd.vmax, c.v);
            }
            if (ncomp == 1) { hd.comp[0].h = hd.comp[0].v = 1; hd.hmax = hd.vmax = 1; }    // a single component is never interleaved
            // the grey output is component 0's plane as it is coded: a file whose first component is SUBSAMPLED against another one
            // (luma 1x1 beside chroma 2x2, which no camera or encoder of this code base writes) would need libjpeg's upsampling
            if (hd.comp[0].h != hd.hmax || hd.comp[0].v != hd.vmax) return walk_fail(why, "first component is subsampled (not supported)");
            const int mcux = (X + 8 * hd.hmax - 1) / (8 * hd.hmax), mcuy = (Y + 8 * hd.vmax - 1) / (8 * hd.vmax);
            hd.plane_w = mcux * hd.comp[0].h * 8; hd.plane_h = mcuy * hd.comp[0].v * 8;
            if (hd.plane_w < X || hd.plane_h < Y) return walk_fail(why, "frame geometry is inconsistent");
            hd.have_frame = true;
        } else if (m == 0xC2 || (m >= 0xC5 && m <= 0xCF && m != 0xC8 && m != 0xCC) || m == 0xC3) {
            return walk_fail(why, m == 0xC2 ? "progressive JPEG is not supported (baseline only)" : "unsupported JPEG process (arithmetic / lossless / hierarchical)");
        } else if (m == 0xDD) {                                                        // DRI
            if (n < 2) return walk_fail(why, "bad restart interval");
            hd.restart_interval = u16(pos + 2);
        } else if (m == 0xDA) {                                                        // SOS
            if (!hd.have_frame) return walk_fail(why, "scan before the frame header");
            if (n < 1) return walk_fail(why, "bad scan header");
            const int ns = s[0];
            if (ns < 1 || ns > hd.ncomp || n < 1 + 2 * ns + 3) return walk_fail(why, "bad scan header");
            for (int i = 0; i < ns; ++i) {
                int ci = -1;
                for (int c = 0; c < hd.ncomp; ++c) if (hd.comp[c].id == s[1 + 2 * i]) ci = c;
                if (ci < 0) return walk_fail(why, "scan names an unknown component");
                for (int k = 0; k < i; ++k) if (scan.idx[k] == ci) return walk_fail(why, "scan names a component twice");
                if (ci == 0 && hd.decoded_luma) return walk_fail(why, "second scan of the first component in a sequential file");
                Component& c = hd.comp[ci];
                c.td = s[2 + 2 * i] >> 4; c.ta = s[2 + 2 * i] & 15;
                if (c.td > 3 || c.ta > 3 || !hd.dc[c.td].present || !hd.ac[c.ta].present || !hd.have_q[c.tq]) return walk_fail(why, "scan uses a missing table");
                scan.idx[i] = ci;
            }
            scan.ns = ns;
            pos += (size_t)len;
            scan.data = pos;
            return Walk::scan;
        }
        pos += (size_t)len;
    }
}

// The three-component class the device decoder takes when it was made for colour (csrc/jpeg_dec.hip; DESIGN.md, the section on colour
// streams): one interleaved scan of all three components in frame order, component 0 sampled 1 x 1, 2 x 1 or 2 x 2 (h x v), the other
// two 1 x 1, an 8-bit quantisation table for component 0 (the chroma tables are never used), and no restart interval unless the caller
// allows one (a decoder switched to take them: lpslam_hip_jpeg_dec_take_restart).  Asked by the device decoder and by the host layer
// that offers streams to it, so the two cannot disagree.
inline bool interleaved_ycc_scan(const Header& hd, const Scan& scan, bool restart_allowed = false)
{
    if (hd.ncomp != 3 || scan.ns != 3 || scan.idx[0] != 0 || scan.idx[1] != 1 || scan.idx[2] != 2) return false;
    const Component& y = hd.comp[0];
    if (!((y.h == 1 && y.v == 1) || (y.h == 2 && y.v == 1) || (y.h == 2 && y.v == 2))) return false;
    if (hd.comp[1].h != 1 || hd.comp[1].v != 1 || hd.comp[2].h != 1 || hd.comp[2].v != 1) return false;
    return (restart_allowed || hd.restart_interval == 0) && !hd.q16[y.tq];
}

// The one-component class of the device decoder: an 8-bit quantisation table, and the same rule for a restart interval.
inline bool grey_scan(const Header& hd, bool restart_allowed = false)
{
    return hd.ncomp == 1 && (restart_allowed || hd.restart_interval == 0) && !hd.q16[hd.comp[0].tq];
}

// Restart markers the entropy-coded data of a scan over `mcus` MCUs must hold: one behind every full interval but the last.  A DRI of
// 0, or of the MCU count or more, means none.
inline int restart_markers(const Header& hd, long long mcus)
{
    const long long ri = hd.restart_interval;
    return ri > 0 && ri < mcus ? (int)((mcus + ri - 1) / ri - 1) : 0;
}

}  // namespace jpeg
}  // namespace LpSlam
