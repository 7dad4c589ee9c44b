// Baseline (Huffman, sequential DCT, 8-bit) JPEG -> grey: see jpeg.h.  Written from the standard (ITU-T T.81: marker syntax,
// Huffman procedures of Annex F, table construction of Annex C) and the published description of libjpeg's "islow" inverse DCT
// (Loeffler-Ligtenberg-Moschytz, 13-bit constants, two passes with 2 extra bits after the first) so that the samples are libjpeg's.
#include "jpeg.h"
#include "jpeg_header.h"
#include "jpeg_tables.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace LpSlam {
namespace {

using jpeg::kZigzag;

using jpeg::HuffTable;
using jpeg::Component;

struct BitReader {
    const uint8_t* p; const uint8_t* end;
    uint64_t acc = 0; int n = 0;         // n valid bits at the top of acc's low 64 - ... kept right-aligned
    int marker = 0;                      // a marker met inside the entropy-coded data (0 = none): zeros are fed from then on
    void fill()
    {
        while (n <= 48) {
            int b = 0;
            if (!marker && p < end) {
                b = *p++;
                if (b == 0xFF) {
                    int b2 = p < end ? *p : 0xD9;
                    while (b2 == 0xFF && p < end) { ++p; b2 = p < end ? *p : 0xD9; }       // fill bytes
                    if (b2 == 0) ++p;                                 // stuffed zero: a data byte FF
                    else { marker = b2; ++p; b = 0; }
                }
            }
            acc = (acc << 8) | (uint64_t)b; n += 8;
        }
    }
    int peek(int k) { if (n < k) fill(); return (int)((acc >> (n - k)) & ((1u << k) - 1)); }
    void skip(int k) { n -= k; }
    int get(int k) { if (k == 0) return 0; const int v = peek(k); skip(k); return v; }
    void restart() { acc = 0; n = 0; marker = 0; }
};

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

bool decode_symbol(BitReader& br, const HuffTable& t, int& sym)
{
    const int look = br.peek(9);
    const uint16_t e = t.look[look];
    if (e) { br.skip(e >> 8); sym = e & 255; return true; }
    int code = look, l = 9;
    while (l < 16) {
        ++l;
        code = br.peek(l);
        if (t.maxcode[l] >= 0 && code <= t.maxcode[l] && code >= t.mincode[l]) { br.skip(l); sym = t.vals[t.valptr[l] + code - t.mincode[l]]; return true; }
    }
    return false;
}

// libjpeg's jpeg_idct_islow: coefficients (natural order) x quantisation table -> 8x8 samples
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int32_t F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373, F_1_175875602 = 9633,
                  F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;
inline int32_t descale(int64_t x, int n) { return (int32_t)((x + ((int64_t)1 << (n - 1))) >> n); }
inline uint8_t range_limit(int32_t x)
{
    const int32_t xs = ((x & 1023) ^ 512) - 512;                      // the table is indexed modulo 1024
    const int32_t v = xs + 128;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

void idct_islow(const int16_t* coef, const uint16_t* quant, uint8_t* out, int pitch)
{
    int32_t ws[64];
    for (int c = 0; c < 8; ++c) {
        const int16_t* in = coef + c; const uint16_t* q = quant + c; int32_t* w = ws + c;
        if (in[8] == 0 && in[16] == 0 && in[24] == 0 && in[32] == 0 && in[40] == 0 && in[48] == 0 && in[56] == 0) {
            const int32_t dc = (int32_t)((uint32_t)((int32_t)in[0] * (int32_t)q[0]) << PASS1_BITS);
            for (int r = 0; r < 8; ++r) w[8 * r] = dc;
            continue;
        }
        int64_t z2 = (int32_t)in[16] * (int32_t)q[16], z3 = (int32_t)in[48] * (int32_t)q[48];
        int64_t z1 = (z2 + z3) * F_0_541196100;
        int64_t tmp2 = z1 + z3 * (-F_1_847759065), tmp3 = z1 + z2 * F_0_765366865;
        z2 = (int32_t)in[0] * (int32_t)q[0]; z3 = (int32_t)in[32] * (int32_t)q[32];
        int64_t tmp0 = (z2 + z3) * (1 << CONST_BITS), tmp1 = (z2 - z3) * (1 << CONST_BITS);
        const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = (int32_t)in[56] * (int32_t)q[56]; tmp1 = (int32_t)in[40] * (int32_t)q[40]; tmp2 = (int32_t)in[24] * (int32_t)q[24]; tmp3 = (int32_t)in[8] * (int32_t)q[8];
        z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
        int64_t z4 = tmp1 + tmp3;
        const int64_t z5 = (z3 + z4) * F_1_175875602;
        tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
        z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
        z3 += z5; z4 += z5;
        tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
        w[0] = descale(tmp10 + tmp3, CONST_BITS - PASS1_BITS);  w[56] = descale(tmp10 - tmp3, CONST_BITS - PASS1_BITS);
        w[8] = descale(tmp11 + tmp2, CONST_BITS - PASS1_BITS);  w[48] = descale(tmp11 - tmp2, CONST_BITS - PASS1_BITS);
        w[16] = descale(tmp12 + tmp1, CONST_BITS - PASS1_BITS); w[40] = descale(tmp12 - tmp1, CONST_BITS - PASS1_BITS);
        w[24] = descale(tmp13 + tmp0, CONST_BITS - PASS1_BITS); w[32] = descale(tmp13 - tmp0, CONST_BITS - PASS1_BITS);
    }
    for (int r = 0; r < 8; ++r) {
        const int32_t* w = ws + 8 * r; uint8_t* o = out + (size_t)r * pitch;
        if (w[1] == 0 && w[2] == 0 && w[3] == 0 && w[4] == 0 && w[5] == 0 && w[6] == 0 && w[7] == 0) {
            const uint8_t dc = range_limit(descale(w[0], PASS1_BITS + 3));
            for (int c = 0; c < 8; ++c) o[c] = dc;
            continue;
        }
        int64_t z2 = w[2], z3 = w[6];
        int64_t z1 = (z2 + z3) * F_0_541196100;
        int64_t tmp2 = z1 + z3 * (-F_1_847759065), tmp3 = z1 + z2 * F_0_765366865;
        int64_t tmp0 = ((int64_t)w[0] + w[4]) * (1 << CONST_BITS), tmp1 = ((int64_t)w[0] - w[4]) * (1 << CONST_BITS);
        const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = w[7]; tmp1 = w[5]; tmp2 = w[3]; tmp3 = w[1];
        z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
        int64_t z4 = tmp1 + tmp3;
        const int64_t z5 = (z3 + z4) * F_1_175875602;
        tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
        z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
        z3 += z5; z4 += z5;
        tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
        constexpr int S = CONST_BITS + PASS1_BITS + 3;
        o[0] = range_limit(descale(tmp10 + tmp3, S)); o[7] = range_limit(descale(tmp10 - tmp3, S));
        o[1] = range_limit(descale(tmp11 + tmp2, S)); o[6] = range_limit(descale(tmp11 - tmp2, S));
        o[2] = range_limit(descale(tmp12 + tmp1, S)); o[5] = range_limit(descale(tmp12 - tmp1, S));
        o[3] = range_limit(descale(tmp13 + tmp0, S)); o[4] = range_limit(descale(tmp13 - tmp0, S));
    }
}

bool fail(std::string* why, const char* msg) { if (why) *why = msg; return false; }

}  // namespace

bool decode_jpeg_gray(const uint8_t* d, size_t size, GrayImage& out, std::string* why)
{
    if (!looks_like_jpeg(d, size)) return fail(why, "not a JPEG stream (no SOI)");
    jpeg::Header hd;
    jpeg::Scan scan;
    uint16_t (&quant)[4][64] = hd.quant;
    HuffTable (&dc)[4] = hd.dc; HuffTable (&ac)[4] = hd.ac;
    Component (&comp)[4] = hd.comp;
    std::vector<uint8_t> plane;            // component 0, padded to whole blocks / MCUs
    size_t pos = 2;
    for (;;) {
        const jpeg::Walk w = jpeg::walk_to_scan(d, size, pos, hd, scan, why);         // the marker segments up to the next scan (jpeg_header.h)
        if (w == jpeg::Walk::error) return false;
        if (w == jpeg::Walk::end) break;
        {
            const int ncomp = hd.ncomp, X = hd.X, Y = hd.Y, hmax = hd.hmax, vmax = hd.vmax, restart_interval = hd.restart_interval;
            const int plane_w = hd.plane_w, plane_h = hd.plane_h, ns = scan.ns;
            const int* idx = scan.idx;
            if (plane.empty()) plane.assign((size_t)plane_w * plane_h, 0);
            BitReader br{d + scan.data, d + size};
            for (int c = 0; c < ncomp; ++c) comp[c].pred = 0;
            int16_t block[64];
            auto decode_block = [&](Component& c, bool keep, int bx, int by) -> bool {
                std::memset(block, 0, sizeof(block));
                int sym;
                if (!decode_symbol(br, dc[c.td], sym) || sym > 11) return false;
                c.pred += sym ? extend(br.get(sym), sym) : 0;
                block[0] = (int16_t)c.pred;
                for (int k = 1; k < 64;) {
                    if (!decode_symbol(br, ac[c.ta], sym)) return false;
                    const int r = sym >> 4, sz = sym & 15;
                    if (sz == 0) { if (r == 15) { k += 16; continue; } break; }
                    k += r;
                    if (k > 63) return false;
                    block[kZigzag[k]] = (int16_t)extend(br.get(sz), sz);
                    ++k;
                }
                if (keep) idct_islow(block, quant[c.tq], plane.data() + (size_t)by * 8 * plane_w + (size_t)bx * 8, plane_w);
                return true;
            };
            auto restart = [&]() -> bool {
                // the bit reader stops at the marker: it must be an RSTn; then byte alignment and fresh predictions
                br.fill();
                if (br.marker < 0xD0 || br.marker > 0xD7) return false;
                br.restart();
                for (int c = 0; c < ncomp; ++c) comp[c].pred = 0;
                return true;
            };
            if (ns == 1) {                                                             // non-interleaved: the component's own block raster
                Component& c = comp[idx[0]];
                const int cw = (X * c.h + hmax - 1) / hmax, chh = (Y * c.v + vmax - 1) / vmax;
                const int bw = (cw + 7) / 8, bh = (chh + 7) / 8;
                int count = 0;
                for (int by = 0; by < bh; ++by)
                    for (int bx = 0; bx < bw; ++bx) {
                        if (restart_interval && count && count % restart_interval == 0 && !restart()) return fail(why, "missing restart marker");
                        const bool keep = idx[0] == 0 && (bx + 1) * 8 <= plane_w && (by + 1) * 8 <= plane_h;
                        if (!decode_block(c, keep, bx, by)) return fail(why, "corrupt entropy-coded data");
                        ++count;
                    }
            } else {
                const int mcux = (X + 8 * hmax - 1) / (8 * hmax), mcuy = (Y + 8 * vmax - 1) / (8 * vmax);
                int count = 0;
                for (int my = 0; my < mcuy; ++my)
                    for (int mx = 0; mx < mcux; ++mx) {
                        if (restart_interval && count && count % restart_interval == 0 && !restart()) return fail(why, "missing restart marker");
                        for (int i = 0; i < ns; ++i) {
                            Component& c = comp[idx[i]];
                            for (int v = 0; v < c.v; ++v)
                                for (int h = 0; h < c.h; ++h)
                                    if (!decode_block(c, idx[i] == 0, mx * c.h + h, my * c.v + v)) return fail(why, "corrupt entropy-coded data");
                        }
                        ++count;
                    }
            }
            for (int i = 0; i < ns; ++i) if (idx[i] == 0) hd.decoded_luma = true;
            // continue behind the entropy-coded data: at the marker the reader stopped at, or scan for the next one
            const size_t q = (size_t)(br.p - d);
            pos = q >= 2 ? q - 2 : q;
        }
    }
    if (!hd.have_frame || !hd.decoded_luma) return fail(why, "no image data");
    const int X = hd.X, Y = hd.Y, plane_w = hd.plane_w, plane_h = hd.plane_h;
    if (plane_w < X || plane_h < Y || plane.size() < (size_t)plane_w * (size_t)Y) return fail(why, "frame geometry is inconsistent");
    out.width = X; out.height = Y;
    out.pixels.resize((size_t)X * Y);
    for (int y = 0; y < Y; ++y) std::memcpy(&out.pixels[(size_t)y * X], &plane[(size_t)y * plane_w], (size_t)X);
    return true;
}

}  // namespace LpSlam

namespace LpSlam {
namespace {

// ---- encoder: what cv::imencode(".jpg", grey) asks libjpeg for -- tables and headers in jpeg_tables.h, quality 95 by default
using jpeg::EncTable;

// libjpeg's jpeg_fdct_islow on an 8 x 8 block of level-shifted samples (the result is 8 x the DCT)
void fdct_islow(int32_t* data)
{
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i < 8; ++i) {
            int32_t* d = pass == 0 ? data + 8 * i : data + i;
            const int st = pass == 0 ? 1 : 8;
            const int64_t tmp0 = d[0] + d[7 * st], tmp7 = d[0] - d[7 * st], tmp1 = d[st] + d[6 * st], tmp6 = d[st] - d[6 * st];
            const int64_t tmp2 = d[2 * st] + d[5 * st], tmp5 = d[2 * st] - d[5 * st], tmp3 = d[3 * st] + d[4 * st], tmp4 = d[3 * st] - d[4 * st];
            const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
            const int sh = pass == 0 ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
            if (pass == 0) { d[0] = (int32_t)((tmp10 + tmp11) * (1 << PASS1_BITS)); d[4 * st] = (int32_t)((tmp10 - tmp11) * (1 << PASS1_BITS)); }
            else { d[0] = descale(tmp10 + tmp11, PASS1_BITS); d[4 * st] = descale(tmp10 - tmp11, PASS1_BITS); }
            int64_t z1 = (tmp12 + tmp13) * F_0_541196100;
            d[2 * st] = descale(z1 + tmp13 * F_0_765366865, sh);
            d[6 * st] = descale(z1 + tmp12 * (-F_1_847759065), sh);
            z1 = tmp4 + tmp7;
            int64_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
            const int64_t z5 = (z3 + z4) * F_1_175875602;
            const int64_t t4 = tmp4 * F_0_298631336, t5 = tmp5 * F_2_053119869, t6 = tmp6 * F_3_072711026, t7 = tmp7 * F_1_501321110;
            z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
            z3 += z5; z4 += z5;
            d[7 * st] = descale(t4 + z1 + z3, sh); d[5 * st] = descale(t5 + z2 + z4, sh);
            d[3 * st] = descale(t6 + z2 + z3, sh); d[st] = descale(t7 + z1 + z4, sh);
        }
    }
}

struct BitWriter {
    std::vector<uint8_t>& out; uint32_t acc = 0; int n = 0;
    void put(uint32_t code, int len)
    {
        acc = (acc << len) | (code & ((1u << len) - 1)); n += len;
        while (n >= 8) { const uint8_t b = (uint8_t)(acc >> (n - 8)); out.push_back(b); if (b == 0xFF) out.push_back(0); n -= 8; }
    }
    void flush() { if (n) put(0x7F, 8 - n); }             // pad with ones
    void restart(int number) { flush(); out.push_back(0xFF); out.push_back((uint8_t)(0xD0 + (number & 7))); }
};

}  // namespace

bool encode_jpeg_gray(const GrayImage& img, int quality, std::vector<uint8_t>& out) { return encode_jpeg_gray_restart(img, quality, 0, out); }

bool encode_jpeg_gray_restart(const GrayImage& img, int quality, int restart_interval, std::vector<uint8_t>& out)
{
    if (restart_interval < 0 || restart_interval > 65535) return false;
    if (img.width <= 0 || img.height <= 0 || img.width > 65535 || img.height > 65535 || img.pixels.size() < (size_t)img.width * img.height) return false;
    quality = std::min(100, std::max(1, quality));
    uint8_t q[64];
    jpeg::quant_table(quality, q);
    EncTable dct, act;
    jpeg::make_enc_table(jpeg::kDcLumBits, jpeg::kDcLumVals, dct); jpeg::make_enc_table(jpeg::kAcLumBits, jpeg::kAcLumVals, act);
    out.clear();
    jpeg::write_headers(out, img.width, img.height, q, restart_interval);
    BitWriter bw{out};
    const int bw_n = (img.width + 7) / 8, bh_n = (img.height + 7) / 8;
    int pred = 0, count = 0;
    for (int by = 0; by < bh_n; ++by)
        for (int bx = 0; bx < bw_n; ++bx, ++count) {
            if (restart_interval && count && count % restart_interval == 0) { bw.restart(count / restart_interval - 1); pred = 0; }
            int32_t blk[64];
            for (int r = 0; r < 8; ++r) {
                const int y = std::min(8 * by + r, img.height - 1);                // edge blocks: the last row / column repeated (libjpeg's edge expansion)
                for (int c = 0; c < 8; ++c) blk[8 * r + c] = (int32_t)img.pixels[(size_t)y * img.width + std::min(8 * bx + c, img.width - 1)] - 128;
            }
            fdct_islow(blk);
            int16_t zz[64];
            for (int k = 0; k < 64; ++k) {
                const int i = kZigzag[k];
                const int32_t qv = (int32_t)q[i] << 3;                            // the transform's output is scaled by 8
                int32_t t = blk[i];
                if (t < 0) { t = -t; t += qv >> 1; t = t >= qv ? t / qv : 0; t = -t; }
                else { t += qv >> 1; t = t >= qv ? t / qv : 0; }
                zz[k] = (int16_t)t;
            }
            auto category = [](int v) { int a = v < 0 ? -v : v, s = 0; while (a) { ++s; a >>= 1; } return s; };
            const int diff = zz[0] - pred; pred = zz[0];
            int s2 = category(diff);
            bw.put(dct.code[s2], dct.len[s2]);
            if (s2) bw.put((uint32_t)(diff < 0 ? diff - 1 : diff), s2);
            int run = 0;
            for (int k = 1; k < 64; ++k) {
                const int v = zz[k];
                if (v == 0) { ++run; continue; }
                while (run > 15) { bw.put(act.code[0xF0], act.len[0xF0]); run -= 16; }
                s2 = category(v);
                bw.put(act.code[(run << 4) | s2], act.len[(run << 4) | s2]);
                bw.put((uint32_t)(v < 0 ? v - 1 : v), s2);
                run = 0;
            }
            if (run) bw.put(act.code[0], act.len[0]);
        }
    bw.flush();
    out.push_back(0xFF); out.push_back(0xD9);
    return true;
}

}  // namespace LpSlam

// tests: encode a grey image; returns the number of bytes written, 0 when the buffer is too small or the image is not encodable
extern "C" __attribute__((visibility("default"))) size_t lpslam_jpeg_encode_gray(const uint8_t* pixels, int w, int h, int quality, uint8_t* out, size_t cap)
{
    LpSlam::GrayImage img; img.width = w; img.height = h; img.pixels.assign(pixels, pixels + (size_t)w * h);
    std::vector<uint8_t> buf;
    if (!LpSlam::encode_jpeg_gray(img, quality, buf) || buf.size() > cap) return 0;
    std::memcpy(out, buf.data(), buf.size());
    return buf.size();
}

// the same with a restart interval in blocks (0: the bytes of lpslam_jpeg_encode_gray)
extern "C" __attribute__((visibility("default"))) size_t lpslam_jpeg_encode_gray_restart(const uint8_t* pixels, int w, int h, int quality, int restart_interval,
                                                                                         uint8_t* out, size_t cap)
{
    LpSlam::GrayImage img; img.width = w; img.height = h; img.pixels.assign(pixels, pixels + (size_t)w * h);
    std::vector<uint8_t> buf;
    if (!LpSlam::encode_jpeg_gray_restart(img, quality, restart_interval, buf) || buf.size() > cap) return 0;
    std::memcpy(out, buf.data(), buf.size());
    return buf.size();
}

// tests: is the first scan of the stream of the class the device decoder takes (csrc/jpeg_dec.hip asks the same functions)?  color: a
// decoder made for three-component streams; restart: one switched to take restart intervals.  1 yes, 0 no, -1 no scan header found.
extern "C" __attribute__((visibility("default"))) int lpslam_jpeg_device_class(const uint8_t* data, size_t size, int color, int restart)
{
    using namespace LpSlam;
    if (!jpeg::has_soi(data, size)) return -1;
    jpeg::Header hd; jpeg::Scan sc; size_t pos = 2;
    if (jpeg::walk_to_scan(data, size, pos, hd, sc, nullptr) != jpeg::Walk::scan) return -1;
    return (jpeg::grey_scan(hd, restart != 0) || (color && jpeg::interleaved_ycc_scan(hd, sc, restart != 0))) ? 1 : 0;
}

// tests: decode into a caller buffer; returns 0 on success, 1 when the buffer is too small (w / h are set), 2 on a decoding error
extern "C" __attribute__((visibility("default"))) int lpslam_jpeg_decode_gray(const uint8_t* data, size_t size, uint8_t* out, size_t cap, int* w, int* h)
{
    LpSlam::GrayImage img;
    if (!LpSlam::decode_jpeg_gray(data, size, img, nullptr)) return 2;
    if (w) *w = img.width;
    if (h) *h = img.height;
    if (img.pixels.size() > cap) return 1;
    std::memcpy(out, img.pixels.data(), img.pixels.size());
    return 0;
}
