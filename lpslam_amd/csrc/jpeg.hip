// jpeg.hip -- baseline JPEG encoder (one grey component) on gfx950: the recorder's cv::imencode(".jpg") (the reference's
// src/Manager/RecordEngine.cpp:93).  The output is byte for byte what the host encoder LpSlam::encode_jpeg_gray writes
// (lpslam_amd/host/jpeg.cpp; tables and marker segments shared through host/jpeg_tables.h), which is libjpeg's stream.
//
// A batch of images is one chain of six launches on the encoder's stream and one wait:
//   k_jpeg_dct      one workgroup per chunk of 32 blocks of one image (4 waves x 8 blocks): lane = (block, row) for the row pass of
//                   libjpeg's islow FDCT, lane = (block, column) for the column pass through LDS, then lane = zigzag index per block:
//                   quantised coefficients out, and the block's AC bit length (ballot of the non-zero coefficients, runs from the
//                   previous set bit, ZRLs only in front of a non-zero coefficient, one EOB when coefficient 63 is zero)
//   k_jpeg_offsets  one workgroup per image: DC differences (raster predecessor in the same image), exclusive scan of the block bit
//                   lengths -> bit offset of every block; zeroes the seam words two chunks share
//   k_jpeg_pack     one workgroup per chunk: every lane ORs its symbols into the chunk's bit range in LDS; the words the chunk owns
//                   completely are written with plain stores, the (at most two) seam words with a global OR into the zeroed words;
//                   the image's last chunk pads the last byte with 1-bits
//   k_jpeg_count    one workgroup per image: 0xFF bytes per 256-byte piece of the entropy-coded data, exclusive scan -> where every
//                   piece lands after byte stuffing
//   k_jpeg_stuff    a wave per piece, lane per word: each byte, and a 0x00 behind every 0xFF, to its place
//   k_jpeg_out      the stuffed bytes and the sizes to page-locked host memory with 16-byte stores
// Every write is a plain store or an OR of disjoint bits, so the output does not depend on scheduling.
#include "internal.h"
#include "../host/jpeg_tables.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

using namespace lpslam;

namespace {

constexpr int kBlocksPerWave = 8, kWaves = 4, kChunkBlocks = kBlocksPerWave * kWaves, kThreads = 64 * kWaves;
constexpr int kMaxBlockBits = 20 + 63 * 26;                   // DC: 9-bit code + 11 bits; 63 x (16-bit code + 10 bits); ZRL / EOB only with fewer
constexpr int kChunkWords = (kChunkBlocks * kMaxBlockBits + 7 + 31) / 32 + 2;
constexpr int kPieceBytes = 256;                              // stuffing granule: one wave, one word per lane
constexpr int kScanThreads = 1024;
constexpr int kCopyGrid = 512, kStuffGrid = 512;

struct JpegImg {            // one image of a batch (device table)
    long long px;           // its samples in the staging buffer (tightly packed rows)
    int w, h, bw, nblk;
    int blk0;               // first block in the batch's block arrays
    int chunk0, nchunks;    // its workgroups in k_jpeg_dct / k_jpeg_pack
    int pad;
};
struct JpegStat { unsigned int bits, bytes, out, pad; };     // entropy-coded bits, bytes after padding, bytes after stuffing

struct JpegArgs {
    const uint8_t* px;
    const JpegImg* imgs;
    int n;
    int16_t* coef;          // quantised coefficients, zigzag order, 64 per block
    int* dc;                // quantised DC of every block
    unsigned int* acbits;   // AC bit length of every block
    unsigned int* off;      // bit offset of every block inside its image's entropy-coded segment
    unsigned int* ent;      // entropy-coded words (big-endian bit order), ent_words per image
    long long ent_words;
    unsigned int* poff;     // stuffed offset of every 256-byte piece, ent_words / 64 per image
    uint8_t* out;           // stuffed bytes, out_cap per image
    long long out_cap;
    JpegStat* stat;
    uint8_t* host_out;      // page-locked: out_cap per image
    JpegStat* host_stat;
    const unsigned int* huff;    // 256 AC entries, then 16 DC entries: (length << 16) | code
    int qz[64];             // quantiser (q << 3) in zigzag order
    int nat[64];            // natural index of every zigzag position
};

constexpr long long F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
                    F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
                    F_2_562915447 = 20995, F_3_072711026 = 25172;

#include "jpeg_scan.inl"

__device__ __forceinline__ int descale(long long x, int n) { return (int)((x + (1LL << (n - 1))) >> n); }

// one pass of libjpeg's jpeg_fdct_islow on 8 values (host: fdct_islow in host/jpeg.cpp, the same integers); pass 0 = rows
template <int PASS>
__device__ __forceinline__ void fdct8(int d[8])
{
    constexpr int sh = PASS == 0 ? 13 - 2 : 13 + 2;
    const long long tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const long long tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (PASS == 0) { d[0] = (int)((tmp10 + tmp11) * 4); d[4] = (int)((tmp10 - tmp11) * 4); }
    else { d[0] = descale(tmp10 + tmp11, 2); d[4] = descale(tmp10 - tmp11, 2); }
    long long z1 = (tmp12 + tmp13) * F_0_541196100;
    d[2] = descale(z1 + tmp13 * F_0_765366865, sh);
    d[6] = descale(z1 + tmp12 * (-F_1_847759065), sh);
    z1 = tmp4 + tmp7;
    long long z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const long long z5 = (z3 + z4) * F_1_175875602;
    const long long t4 = tmp4 * F_0_298631336, t5 = tmp5 * F_2_053119869, t6 = tmp6 * F_3_072711026, t7 = tmp7 * F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    d[7] = descale(t4 + z1 + z3, sh); d[5] = descale(t5 + z2 + z4, sh);
    d[3] = descale(t6 + z2 + z3, sh); d[1] = descale(t7 + z1 + z4, sh);
}

__device__ __forceinline__ int category(int v) { const int a = v < 0 ? -v : v; return a ? 32 - __clz(a) : 0; }
__device__ __forceinline__ int hlen(unsigned int e) { return (int)(e >> 16); }

// the AC symbols of lane `lane` (zigzag index) of a block whose coefficient there is v; nz = ballot of the non-zero AC coefficients.
// Returns the lane's bit count; run / eob describe the symbols for the packer.
__device__ __forceinline__ int ac_symbols(int lane, int v, unsigned long long nz, const unsigned int* huff, int& run, bool& eob)
{
    int bits = 0;
    run = 0;
    if (lane > 0 && v != 0) {
        const unsigned long long below = nz & ((1ULL << lane) - 1);
        const int prev = below ? 63 - __clzll(below) : 0;
        run = lane - prev - 1;
        const int s = category(v);
        bits = (run >> 4) * hlen(huff[0xF0]) + hlen(huff[((run & 15) << 4) | s]) + s;
    }
    const int last = nz ? 63 - __clzll(nz) : 0;
    eob = lane == last && last < 63;
    if (eob) bits += hlen(huff[0]);
    return bits;
}

__device__ __forceinline__ int image_of_chunk(const JpegImg* imgs, int n, int chunk)
{
    int i = 0;
    while (i + 1 < n && imgs[i + 1].chunk0 <= chunk) ++i;
    return i;
}

__global__ __launch_bounds__(kThreads) void k_jpeg_dct(JpegArgs a)
{
    __shared__ int tile[kWaves][kBlocksPerWave][64];
    __shared__ unsigned int huff[256];
    for (int k = threadIdx.x; k < 256; k += kThreads) huff[k] = a.huff[k];
    const int chunk = blockIdx.x;
    const JpegImg im = a.imgs[image_of_chunk(a.imgs, a.n, chunk)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = (chunk - im.chunk0) * kChunkBlocks + wave * kBlocksPerWave;
    const int j = lane >> 3, r = lane & 7;
    const int lb = first + j;
    int* t = tile[wave][j];
    if (lb < im.nblk) {                               // rows: lane = (block j, row r), libjpeg's edge replication
        const int by = lb / im.bw, bx = lb - by * im.bw;
        const uint8_t* row = a.px + im.px + (long long)min(8 * by + r, im.h - 1) * im.w;
        int d[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) d[c] = (int)row[min(8 * bx + c, im.w - 1)] - 128;
        fdct8<0>(d);
#pragma unroll
        for (int c = 0; c < 8; ++c) t[8 * r + c] = d[c];
    }
    __syncthreads();
    if (lb < im.nblk) {                               // columns: lane = (block j, column r)
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = t[8 * k + r];
        fdct8<1>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) t[8 * k + r] = d[k];
    }
    __syncthreads();
    const int qv = a.qz[lane], nat = a.nat[lane];
    for (int jj = 0; jj < kBlocksPerWave; ++jj) {     // lane = zigzag index
        const int lbj = first + jj;
        if (lbj >= im.nblk) break;
        int v = tile[wave][jj][nat];
        if (v < 0) v = -((-v + (qv >> 1)) / qv);      // libjpeg's quantiser: (|t| + q/2) / q with the sign of t
        else v = (v + (qv >> 1)) / qv;
        const long long b = im.blk0 + lbj;
        a.coef[b * 64 + lane] = (int16_t)v;
        const unsigned long long nz = __ballot(lane > 0 && v != 0);
        int run; bool eob;
        const int bits = wave_sum(ac_symbols(lane, v, nz, huff, run, eob));
        if (lane == 0) { a.dc[b] = v; a.acbits[b] = (unsigned int)bits; }
    }
}

__device__ __forceinline__ unsigned int block_bits(const JpegArgs& a, const JpegImg& im, int lb, const unsigned int* huff)
{
    const long long b = im.blk0 + lb;
    const int s = category(a.dc[b] - (lb > 0 ? a.dc[b - 1] : 0));
    return a.acbits[b] + (unsigned int)(hlen(huff[256 + s]) + s);
}

__global__ __launch_bounds__(kScanThreads) void k_jpeg_offsets(JpegArgs a)
{
    __shared__ unsigned int huff[256 + 16];
    __shared__ unsigned int wsum[kScanThreads / 64 + 1];
    for (int k = threadIdx.x; k < 256 + 16; k += kScanThreads) huff[k] = a.huff[k];
    __syncthreads();
    const int i = blockIdx.x;
    const JpegImg im = a.imgs[i];
    const int per = (im.nblk + kScanThreads - 1) / kScanThreads;
    const int b0 = min(im.nblk, (int)threadIdx.x * per), b1 = min(im.nblk, b0 + per);
    unsigned int sum = 0;
    for (int lb = b0; lb < b1; ++lb) sum += block_bits(a, im, lb, huff);
    unsigned int total;
    unsigned int o = block_exclusive(sum, wsum, &total);
    unsigned int* ent = a.ent + (long long)i * a.ent_words;
    for (int lb = b0; lb < b1; ++lb) {
        a.off[im.blk0 + lb] = o;
        if (lb > 0 && lb % kChunkBlocks == 0) { ent[o >> 5] = 0u; ent[(o - 1) >> 5] = 0u; }    // the seam words of two chunks: OR-ed by both
        o += block_bits(a, im, lb, huff);
    }
    if (threadIdx.x == 0) {
        JpegStat s; s.bits = total; s.bytes = (total + 7) / 8; s.out = 0; s.pad = 0;
        a.stat[i] = s;
    }
}

__device__ __forceinline__ void put_bits(unsigned int* buf, unsigned int p, unsigned int v, int len)
{
    if (len == 0) return;
    const unsigned long long x = (unsigned long long)(v & ((1u << len) - 1)) << (64 - len - (int)(p & 31));
    atomicOr(&buf[p >> 5], (unsigned int)(x >> 32));
    if ((unsigned int)x) atomicOr(&buf[(p >> 5) + 1], (unsigned int)x);
}

__global__ __launch_bounds__(kThreads) void k_jpeg_pack(JpegArgs a)
{
    __shared__ unsigned int buf[kChunkWords];
    __shared__ unsigned int huff[256 + 16];
    const int chunk = blockIdx.x;
    const int i = image_of_chunk(a.imgs, a.n, chunk);
    const JpegImg im = a.imgs[i];
    const int c = chunk - im.chunk0;
    const int lb0 = c * kChunkBlocks, lb1 = min(im.nblk, lb0 + kChunkBlocks);
    const unsigned int* off = a.off + im.blk0;
    const bool last_chunk = c == im.nchunks - 1;
    const unsigned int w0 = off[lb0] >> 5;
    const unsigned int end = last_chunk ? a.stat[i].bytes * 8 : off[lb1];           // the last chunk ends behind the padding
    const int nwords = (int)(((end - 1) >> 5) - w0 + 1);
    for (int k = threadIdx.x; k < kChunkWords; k += kThreads) buf[k] = 0u;
    for (int k = threadIdx.x; k < 256 + 16; k += kThreads) huff[k] = a.huff[k];
    __syncthreads();
    const unsigned int base = w0 * 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int jj = 0; jj < kBlocksPerWave; ++jj) {
        const int lb = lb0 + wave * kBlocksPerWave + jj;
        if (lb >= lb1) break;
        const long long b = im.blk0 + lb;
        const int v = a.coef[b * 64 + lane];
        const unsigned long long nz = __ballot(lane > 0 && v != 0);
        int run; bool eob;
        int bits = ac_symbols(lane, v, nz, huff, run, eob);
        int diff = 0, sdc = 0;
        if (lane == 0) { diff = v - (lb > 0 ? a.dc[b - 1] : 0); sdc = category(diff); bits += hlen(huff[256 + sdc]) + sdc; }
        unsigned int p = off[lb] - base + (unsigned int)wave_exclusive(bits, lane);
        if (lane == 0) {
            const unsigned int e = huff[256 + sdc];
            put_bits(buf, p, e & 0xFFFF, hlen(e)); p += hlen(e);
            put_bits(buf, p, (unsigned int)(diff < 0 ? diff - 1 : diff), sdc); p += sdc;
        } else if (v != 0) {
            const unsigned int zrl = huff[0xF0];
            for (int z = 0; z < (run >> 4); ++z) { put_bits(buf, p, zrl & 0xFFFF, hlen(zrl)); p += hlen(zrl); }
            const int s = category(v);
            const unsigned int e = huff[((run & 15) << 4) | s];
            put_bits(buf, p, e & 0xFFFF, hlen(e)); p += hlen(e);
            put_bits(buf, p, (unsigned int)(v < 0 ? v - 1 : v), s); p += s;
        }
        if (eob) put_bits(buf, p, huff[0] & 0xFFFF, hlen(huff[0]));
    }
    if (last_chunk && threadIdx.x == 0) {             // pad the last byte with 1-bits
        const unsigned int bits = a.stat[i].bits, pad = a.stat[i].bytes * 8 - bits;
        put_bits(buf, bits - base, 0x7Fu, (int)pad);
    }
    __syncthreads();
    unsigned int* ent = a.ent + (long long)i * a.ent_words + w0;
    for (int k = threadIdx.x; k < nwords; k += kThreads) {
        const bool seam = (k == 0 && c > 0) || (k == nwords - 1 && !last_chunk);
        if (seam) atomicOr(&ent[k], buf[k]);
        else ent[k] = buf[k];
    }
}

__device__ __forceinline__ int ff_count(unsigned int x, int nb)      // 0xFF among the first nb (big-endian) bytes of x
{
    int n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) n += (j < nb && ((x >> (24 - 8 * j)) & 0xFF) == 0xFF) ? 1 : 0;
    return n;
}

__global__ __launch_bounds__(kScanThreads) void k_jpeg_count(JpegArgs a)
{
    __shared__ unsigned int wsum[kScanThreads / 64 + 1];
    const int i = blockIdx.x;
    const unsigned int nbytes = a.stat[i].bytes;
    const int npieces = (int)((nbytes + kPieceBytes - 1) / kPieceBytes);
    const uint4* src = reinterpret_cast<const uint4*>(a.ent + (long long)i * a.ent_words);
    unsigned int* poff = a.poff + (long long)i * (a.ent_words / 64);
    unsigned int carry = 0;
    for (int base = 0; base < npieces; base += kScanThreads) {
        const int piece = base + (int)threadIdx.x;
        unsigned int cnt = 0;
        if (piece < npieces) {
            const long long b0 = (long long)piece * kPieceBytes;
#pragma unroll 4
            for (int q = 0; q < kPieceBytes / 16; ++q) {
                const uint4 v = src[(long long)piece * (kPieceBytes / 16) + q];
                const long long bq = b0 + 16 * q;
                const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long long left = (long long)nbytes - (bq + 4 * k);
                    cnt += ff_count(w[k], left >= 4 ? 4 : (left > 0 ? (int)left : 0));
                }
            }
        }
        unsigned int total;
        const unsigned int pre = block_exclusive(cnt, wsum, &total);
        if (piece < npieces) poff[piece] = carry + pre;
        carry += total;
    }
    if (threadIdx.x == 0) a.stat[i].out = nbytes + carry;
}

__global__ __launch_bounds__(kThreads) void k_jpeg_stuff(JpegArgs a)
{
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * kWaves + (threadIdx.x >> 6), nw = gridDim.x * kWaves;
    for (int i = 0; i < a.n; ++i) {
        const unsigned int nbytes = a.stat[i].bytes;
        const int npieces = (int)((nbytes + kPieceBytes - 1) / kPieceBytes);
        const unsigned int* ent = a.ent + (long long)i * a.ent_words;
        const unsigned int* poff = a.poff + (long long)i * (a.ent_words / 64);
        uint8_t* out = a.out + (long long)i * a.out_cap;
        for (int piece = gw; piece < npieces; piece += nw) {
            const unsigned int byte0 = (unsigned int)piece * kPieceBytes + 4u * lane;
            const int nb = byte0 >= nbytes ? 0 : (int)min(4u, nbytes - byte0);
            const unsigned int x = nb ? ent[byte0 >> 2] : 0u;
            const int cnt = ff_count(x, nb);
            unsigned int pos = poff[piece] + byte0 + (unsigned int)wave_exclusive(cnt, lane);
            for (int j = 0; j < nb; ++j) {
                const uint8_t v = (uint8_t)(x >> (24 - 8 * j));
                out[pos++] = v;
                if (v == 0xFF) out[pos++] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_jpeg_out(JpegArgs a)
{
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x, nt = (long long)gridDim.x * kThreads;
    for (int i = 0; i < a.n; ++i) {
        const long long n16 = ((long long)a.stat[i].out + 15) / 16;
        const uint4* src = reinterpret_cast<const uint4*>(a.out + (long long)i * a.out_cap);
        uint4* dst = reinterpret_cast<uint4*>(a.host_out + (long long)i * a.out_cap);
        for (long long k = tid; k < n16; k += nt) dst[k] = src[k];
    }
    if (tid < a.n) a.host_stat[tid] = a.stat[tid];
}

}  // namespace

struct lpslam_hip_jpeg {
    int device = 0;
    int max_w = 0, max_h = 0, max_images = 0;
    long long max_blocks = 0;          // per image
    long long ent_words = 0, out_cap = 0;
    hipStream_t stream = nullptr;
    uint8_t* d_px = nullptr;
    JpegImg* d_imgs = nullptr;
    int16_t* d_coef = nullptr;
    int* d_dc = nullptr;
    unsigned int *d_acbits = nullptr, *d_off = nullptr, *d_ent = nullptr, *d_poff = nullptr, *d_huff = nullptr;
    uint8_t* d_out = nullptr;
    JpegStat* d_stat = nullptr;
    uint8_t* h_px = nullptr;           // page-locked staging of the samples
    JpegImg* h_imgs = nullptr;
    uint8_t* h_out = nullptr;          // page-locked: written by k_jpeg_out
    JpegStat* h_stat = nullptr;
    uint8_t* dh_out = nullptr;         // their device addresses
    JpegStat* dh_stat = nullptr;
    std::mutex mutex;
};

namespace {
void jpeg_free(lpslam_hip_jpeg* e)
{
    if (!e) return;
    if (e->stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->stream); }
    for (void* p : {(void*)e->d_px, (void*)e->d_imgs, (void*)e->d_coef, (void*)e->d_dc, (void*)e->d_acbits, (void*)e->d_off, (void*)e->d_ent,
                    (void*)e->d_poff, (void*)e->d_huff, (void*)e->d_out, (void*)e->d_stat})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)e->h_px, (void*)e->h_imgs, (void*)e->h_out, (void*)e->h_stat})
        if (p) (void)hipHostFree(p);
    delete e;
}
}  // namespace

extern "C" {

int lpslam_hip_jpeg_create(int32_t max_width, int32_t max_height, int32_t max_images, lpslam_hip_jpeg** out)
{
    if (!out) { set_error("jpeg_create: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    *out = nullptr;
    if (max_width < 1 || max_height < 1 || max_width > 65535 || max_height > 65535 || max_images < 1 || max_images > 256) {
        set_error("jpeg_create: sizes out of range (1 .. 65535 samples, 1 .. 256 images)");
        return LPSLAM_HIP_ERR_INVALID;
    }
    const long long blocks = (long long)((max_width + 7) / 8) * ((max_height + 7) / 8);
    if (blocks * kMaxBlockBits >= (1LL << 31)) { set_error("jpeg_create: image too large for 32-bit bit offsets"); return LPSLAM_HIP_ERR_INVALID; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("jpeg_create: no HIP device (there is no CPU fallback)"); return LPSLAM_HIP_ERR_DEVICE; }
    lpslam_hip_jpeg* e = new (std::nothrow) lpslam_hip_jpeg();
    if (!e) { set_error("jpeg_create: out of host memory"); return LPSLAM_HIP_ERR_INVALID; }
    e->max_w = max_width; e->max_h = max_height; e->max_images = max_images; e->max_blocks = blocks;
    // worst case before stuffing: kMaxBlockBits per block, whole 256-byte pieces; after stuffing at most twice that
    e->ent_words = ((blocks * kMaxBlockBits + 7) / 32 + 2 + 63) / 64 * 64;
    e->out_cap = 2 * e->ent_words * 4;
    const long long px = (long long)max_width * max_height * max_images, nb = blocks * max_images;
    auto fail = [&](hipError_t err, const char* what) { const int rc = hip_fail(err, what); jpeg_free(e); return rc; };
    hipError_t err;
    if ((err = hipGetDevice(&e->device)) != hipSuccess) return fail(err, "hipGetDevice");
    if ((err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return fail(err, "hipStreamCreateWithFlags");
    if ((err = hipMalloc((void**)&e->d_px, (size_t)px)) != hipSuccess) return fail(err, "hipMalloc(jpeg samples)");
    if ((err = hipMalloc((void**)&e->d_imgs, sizeof(JpegImg) * max_images)) != hipSuccess) return fail(err, "hipMalloc(jpeg images)");
    if ((err = hipMalloc((void**)&e->d_coef, (size_t)nb * 64 * sizeof(int16_t))) != hipSuccess) return fail(err, "hipMalloc(jpeg coefficients)");
    if ((err = hipMalloc((void**)&e->d_dc, (size_t)nb * sizeof(int))) != hipSuccess) return fail(err, "hipMalloc(jpeg dc)");
    if ((err = hipMalloc((void**)&e->d_acbits, (size_t)nb * sizeof(unsigned int))) != hipSuccess) return fail(err, "hipMalloc(jpeg lengths)");
    if ((err = hipMalloc((void**)&e->d_off, (size_t)nb * sizeof(unsigned int))) != hipSuccess) return fail(err, "hipMalloc(jpeg offsets)");
    if ((err = hipMalloc((void**)&e->d_ent, (size_t)(e->ent_words * max_images) * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg entropy)");
    if ((err = hipMalloc((void**)&e->d_poff, (size_t)(e->ent_words / 64 * max_images) * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg pieces)");
    if ((err = hipMalloc((void**)&e->d_huff, (256 + 16) * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg tables)");
    if ((err = hipMalloc((void**)&e->d_out, (size_t)(e->out_cap * max_images))) != hipSuccess) return fail(err, "hipMalloc(jpeg out)");
    if ((err = hipMalloc((void**)&e->d_stat, sizeof(JpegStat) * max_images)) != hipSuccess) return fail(err, "hipMalloc(jpeg stat)");
    if ((err = hipHostMalloc((void**)&e->h_px, (size_t)px)) != hipSuccess) return fail(err, "hipHostMalloc(jpeg samples)");
    if ((err = hipHostMalloc((void**)&e->h_imgs, sizeof(JpegImg) * max_images)) != hipSuccess) return fail(err, "hipHostMalloc(jpeg images)");
    if ((err = hipHostMalloc((void**)&e->h_out, (size_t)(e->out_cap * max_images), hipHostMallocMapped)) != hipSuccess) return fail(err, "hipHostMalloc(jpeg out)");
    if ((err = hipHostMalloc((void**)&e->h_stat, sizeof(JpegStat) * max_images, hipHostMallocMapped)) != hipSuccess) return fail(err, "hipHostMalloc(jpeg stat)");
    if ((err = hipHostGetDevicePointer((void**)&e->dh_out, e->h_out, 0)) != hipSuccess) return fail(err, "hipHostGetDevicePointer(jpeg out)");
    if ((err = hipHostGetDevicePointer((void**)&e->dh_stat, e->h_stat, 0)) != hipSuccess) return fail(err, "hipHostGetDevicePointer(jpeg stat)");
    LpSlam::jpeg::EncTable ac, dc;
    LpSlam::jpeg::make_enc_table(LpSlam::jpeg::kAcLumBits, LpSlam::jpeg::kAcLumVals, ac);
    LpSlam::jpeg::make_enc_table(LpSlam::jpeg::kDcLumBits, LpSlam::jpeg::kDcLumVals, dc);
    unsigned int huff[256 + 16] = {0};
    for (int s = 0; s < 256; ++s) huff[s] = ((unsigned int)ac.len[s] << 16) | ac.code[s];
    for (int s = 0; s < 12; ++s) huff[256 + s] = ((unsigned int)dc.len[s] << 16) | dc.code[s];
    if ((err = hipMemcpy(e->d_huff, huff, sizeof(huff), hipMemcpyHostToDevice)) != hipSuccess) return fail(err, "hipMemcpy(jpeg tables)");
    *out = e;
    return LPSLAM_HIP_OK;
}

void lpslam_hip_jpeg_destroy(lpslam_hip_jpeg* enc) { jpeg_free(enc); }

int lpslam_hip_jpeg_encode(lpslam_hip_jpeg* e, int32_t n, const uint8_t* const* pixels, const int32_t* widths, const int32_t* heights,
                           const int32_t* strides, int32_t quality, uint8_t* const* outs, const int64_t* caps, int64_t* sizes)
{
    if (!e || !pixels || !widths || !heights || !strides || !outs || !caps || !sizes) { set_error("jpeg_encode: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (n < 1 || n > e->max_images) { set_error("jpeg_encode: %d images, the encoder takes 1 .. %d", n, e->max_images); return LPSLAM_HIP_ERR_INVALID; }
    if (quality < 1 || quality > 100) { set_error("jpeg_encode: quality %d outside 1 .. 100", quality); return LPSLAM_HIP_ERR_INVALID; }
    for (int i = 0; i < n; ++i) {
        if (!pixels[i] || widths[i] < 1 || heights[i] < 1 || widths[i] > e->max_w || heights[i] > e->max_h || strides[i] < widths[i]) {
            set_error("jpeg_encode: image %d (%d x %d, stride %d) does not fit the encoder (%d x %d)", i, widths[i], heights[i], strides[i], e->max_w, e->max_h);
            return LPSLAM_HIP_ERR_INVALID;
        }
    }
    std::lock_guard<std::mutex> lock(e->mutex);
    LP_HIP(hipSetDevice(e->device));
    JpegArgs a{};
    long long px = 0;
    int blk = 0, chunks = 0;
    for (int i = 0; i < n; ++i) {
        JpegImg& im = e->h_imgs[i];
        im.px = px; im.w = widths[i]; im.h = heights[i]; im.bw = (im.w + 7) / 8;
        im.nblk = im.bw * ((im.h + 7) / 8);
        im.blk0 = blk; im.chunk0 = chunks; im.nchunks = (im.nblk + kChunkBlocks - 1) / kChunkBlocks; im.pad = 0;
        for (int y = 0; y < im.h; ++y) std::memcpy(e->h_px + px + (long long)y * im.w, pixels[i] + (long long)y * strides[i], (size_t)im.w);
        px += (long long)im.w * im.h; blk += im.nblk; chunks += im.nchunks;
    }
    uint8_t q[64];
    LpSlam::jpeg::quant_table(quality, q);
    for (int k = 0; k < 64; ++k) { a.nat[k] = LpSlam::jpeg::kZigzag[k]; a.qz[k] = (int)q[a.nat[k]] << 3; }
    a.px = e->d_px; a.imgs = e->d_imgs; a.n = n; a.coef = e->d_coef; a.dc = e->d_dc; a.acbits = e->d_acbits; a.off = e->d_off;
    a.ent = e->d_ent; a.ent_words = e->ent_words; a.poff = e->d_poff; a.out = e->d_out; a.out_cap = e->out_cap; a.stat = e->d_stat;
    a.host_out = e->dh_out; a.host_stat = e->dh_stat; a.huff = e->d_huff;
    hipStream_t s = e->stream;
    LP_HIP(hipMemcpyAsync(e->d_px, e->h_px, (size_t)px, hipMemcpyHostToDevice, s));
    LP_HIP(hipMemcpyAsync(e->d_imgs, e->h_imgs, sizeof(JpegImg) * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_jpeg_dct, dim3(chunks), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(k_jpeg_offsets, dim3(n), dim3(kScanThreads), 0, s, a);
    hipLaunchKernelGGL(k_jpeg_pack, dim3(chunks), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(k_jpeg_count, dim3(n), dim3(kScanThreads), 0, s, a);
    hipLaunchKernelGGL(k_jpeg_stuff, dim3(kStuffGrid), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(k_jpeg_out, dim3(kCopyGrid), dim3(kThreads), 0, s, a);
    LP_HIP(hipGetLastError());
    LP_HIP(hipStreamSynchronize(s));
    static const size_t kHeader = [] { std::vector<uint8_t> h; uint8_t q1[64] = {0}; LpSlam::jpeg::write_headers(h, 1, 1, q1); return h.size(); }();
    bool fits = true;
    for (int i = 0; i < n; ++i) {
        sizes[i] = (int64_t)(kHeader + e->h_stat[i].out + 2);
        if (sizes[i] > caps[i]) fits = false;
    }
    if (!fits) { set_error("jpeg_encode: an output buffer is smaller than its stream (sizes[] holds the lengths)"); return LPSLAM_HIP_ERR_INVALID; }
    std::vector<uint8_t> hdr;
    for (int i = 0; i < n; ++i) {
        hdr.clear();
        LpSlam::jpeg::write_headers(hdr, widths[i], heights[i], q);
        uint8_t* o = outs[i];
        std::memcpy(o, hdr.data(), hdr.size());
        std::memcpy(o + hdr.size(), e->h_out + (long long)i * e->out_cap, e->h_stat[i].out);
        o[hdr.size() + e->h_stat[i].out] = 0xFF; o[hdr.size() + e->h_stat[i].out + 1] = 0xD9;
    }
    return LPSLAM_HIP_OK;
}

}  // extern "C"
