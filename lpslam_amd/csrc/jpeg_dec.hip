// jpeg_dec.hip -- baseline JPEG decoder (one grey component, or -- a decoder made with LPSLAM_HIP_JPEG_DEC_COLOR -- component 0 of a
// three-component 4:4:4 / 4:2:2 / 4:2:0 stream; with a restart interval only on a decoder switched to take them,
// lpslam_hip_jpeg_dec_take_restart) on gfx950: the direction jpeg.hip lacks.  The samples are bit for bit
// those of the host decoder LpSlam::decode_jpeg_gray (lpslam_amd/host/jpeg.cpp), which are libjpeg's.  The header is
// parsed on the host by the routine the host decoder uses (host/jpeg_header.h); the entropy-coded data of one scan is decoded in
// parallel with the self-synchronising scheme of Weissenberger and Schmidt ("Accelerating JPEG decompression on GPUs"): a Huffman
// decoder started in a wrong state falls into step with the true one after a few symbols.  Restart markers do not change the grid:
// they leave the clean bit string like the stuffed zeros, their places go into a boundary table per image, and a decoder that
// reaches a boundary jumps to it with the true entry state of an interval.
//
// A batch of streams is one upload, one chain of launches on the decoder's stream and one wait at its end, plus one wait per batch of
// synchronisation rounds:
//   k_jdec_count    one workgroup per image: FF 00 pairs per 256-byte piece of the raw data, exclusive scan -> where every piece lands
//                   without its stuffed zeros; the first real marker (an FF that no 00 follows) ends the data.  An image with a restart
//                   interval: FF D0 .. FF D7 does not end the data, both bytes leave with the zeros (the FF may end one piece and the Dn
//                   begin the next), and a second scan counts the markers in front of every piece; any other FF xx ends the data, FF FF
//                   fill bytes included.  Another marker count than ceil(MCUs / Ri) - 1: no subsequences, irregular at once
//   k_jdec_unstuff  a wave per piece, lane per word: every byte but the stuffed zeros and the restart markers to its place -> the clean
//                   bit string; restart marker m (from 1, stream order) stores the clean offset behind it in the image's boundary table
//   k_jdec_sync     one launch per round, lane = subsequence of kSubBits bits: decodes its subsequence from the exit state of its
//                   predecessor (bit overhang, zigzag index, and in a batch with a three-component image the place of the block in its
//                   MCU; subsequence 0 from the true state, every other one from (0, DC next, place 0) at first) whenever that state changed, and records its own exit state and the blocks it completed.  States are read
//                   from the previous round's array and written to this round's (two arrays in turn), so no workgroup waits for
//                   another one and a round does not depend on scheduling.  A round that changes nothing ends the iteration: at most
//                   as many rounds as subsequences, since subsequence s is final after round s.  A subsequence that holds a boundary
//                   leaves with a state that does not depend on its entry state: it is final after round 0.
//   k_jdec_blocks   one workgroup per image: exclusive scan of the completed-block counts -> first block of every subsequence; the
//                   total has to be the block count of the frame header, all components counted
//   k_jdec_write    as k_jdec_sync, from the final entry states: coefficients of component 0 to int16[its blocks][64] (natural order,
//                   zeroed before), DC differences in place 0, the symbols of the other components decoded and dropped; flags what the host decoder refuses (undecodable code, index past 63, DC category > 11)
//                   and every jump to a boundary that is not made at (DC next, place 0, block m * Ri * blocks per MCU)
//   k_jdec_dc       one workgroup per image: running sum of component 0's DC differences in decode order (integers, predictor 0 at the
//                   first block and at every multiple of Ri MCUs; the predictors of the other components are never needed)
//   k_jdec_idct     one workgroup per chunk of 32 blocks: dequantisation and libjpeg's islow IDCT, lane = (block, column) for the first
//                   pass, lane = (block, row) for the second one through LDS, range limit, 8 samples per store; a block's place in
//                   the plane follows from its MCU and its place inside it (decode order is MCU by MCU, not the plane's raster)
//   k_jdec_out      the planes and the per-image results to page-locked host memory with 16-byte stores
// k_jdec_sync and k_jdec_write exist twice: <false> for a batch of one-component images (state without the MCU place, one table pair
// in LDS -- the code of the grey-only decoder), <true> for a batch that holds a three-component image (a grey image in it is an MCU of
// one block); and each of those twice again: without the boundary handling for a batch in which no image has restart markers -- the
// loop of a decoder that knows no restarts, which measured 15 to 35 % faster per round than the folded one -- and with it.
// k_jdec_count, k_jdec_unstuff and k_jdec_dc are split the same way (a branch more per byte cost 30 to 40 us a stereo pair).  Every write is a plain store to a place of its own, an integer sum or an OR / MIN / MAX of integers: the output does
// not depend on scheduling.  Every decode loop consumes at least one bit per turn or jumps forward to a boundary, and ends at its
// subsequence's last bit.  Plain C++ throughout: no inline assembly and no builtins beyond byte swap, shuffles and ballots.
#include "internal.h"
#include "../host/jpeg_header.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

using namespace lpslam;

namespace {

#ifndef LPSLAM_JDEC_SUB_BITS
#define LPSLAM_JDEC_SUB_BITS 1024
#endif
constexpr int kSubBits = LPSLAM_JDEC_SUB_BITS;                // subsequence length; a symbol (code + value bits) has at most 31 bits
#ifndef LPSLAM_JDEC_SYNC_THREADS
#define LPSLAM_JDEC_SYNC_THREADS 256
#endif
#ifndef LPSLAM_JDEC_ROUNDS_PER_CHECK
#define LPSLAM_JDEC_ROUNDS_PER_CHECK 8
#endif
constexpr int kSyncThreads = LPSLAM_JDEC_SYNC_THREADS;        // k_jdec_sync / k_jdec_write: lanes (subsequences) per workgroup
constexpr int kThreads = 256;                                 // k_jdec_unstuff / k_jdec_idct / copies
constexpr int kChunkBlocks = 32;                              // k_jdec_idct: 4 waves x 8 blocks
constexpr int kPieceBytes = 256;                              // unstuffing granule: one wave, one word per lane
constexpr int kScanThreads = 1024;
constexpr int kCopyGrid = 512, kStuffGrid = 512;
constexpr int kRoundsPerCheck = LPSLAM_JDEC_ROUNDS_PER_CHECK;                       // rounds launched before the host reads the "changed" word
constexpr int kRing = 64;                                     // "changed" words: round r writes r % kRing, reads r - 1, clears r + 1
constexpr unsigned int kStop = 0xFFFFu;                       // exit state: the data ended inside a symbol
constexpr unsigned int kNoEntry = 0xFFFFFFFFu;
static_assert(kSubBits >= 32 && kSubBits % 32 == 0, "a symbol must not span more than two subsequences");
static_assert(kSyncThreads >= 64 && kSyncThreads <= 1024 && kSyncThreads % 64 == 0, "whole waves");
static_assert(kRoundsPerCheck >= 1 && kRoundsPerCheck <= kRing / 2, "a batch of rounds must not lap the ring of changed words");

constexpr int kMaxPairs = 3;                                  // distinct (DC, AC) table pairs of one scan: one per component at most
struct DecPair {            // decoding tables of one component (T.81 F.2.2.3, as jpeg::HuffTable): [0] = DC, [1] = AC
    unsigned short look[2][512];
    int mincode[2][17], maxcode[2][18], valptr[2][17];
    unsigned char vals[2][256];
};
struct DecTab {             // of one image: pair[0] is component 0's; a grey image uses no other
    DecPair pair[kMaxPairs];
    unsigned short quant[64];   // component 0's, natural order
};
struct DecImg {             // one image of a batch (device table)
    long long raw0;         // its entropy-coded data in the raw / clean buffers (a multiple of kPieceBytes)
    long long plane0;       // its plane (pitch x 8 * block rows) in the plane buffers
    unsigned int raw_n;     // bytes from the start of the data to the end of the file
    int w, h;
    int bw;                 // blocks in a row of its plane (whole MCUs)
    int nblk;               // blocks of all components in its scan: what the subsequences have to complete
    int nluma;              // blocks of component 0: the coefficient array, k_jdec_dc and k_jdec_idct see no others
    int h0, v0, mcux;       // component 0's blocks in an MCU (h0 x v0, in this order inside the MCU) and MCUs in a row
    int mcu;                // blocks in an MCU: h0 * v0 of component 0, then one each of the others (grey: 1)
    unsigned int pairs;     // 4 bits per place in the MCU: the table pair of the block there
    int blk0;               // first block in the coefficient array
    int piece0;             // first entry of its piece offsets
    int sub0;               // first entry of its subsequence arrays
    int wg0, nwg;           // its workgroups in k_jdec_sync / k_jdec_write
    int chunk0, nchunks;    // its workgroups in k_jdec_idct
    int nrst;               // restart markers its data must hold: ceil(MCUs / Ri) - 1 (0: no restart interval, or one of the MCU count or more)
    int ribl;               // blocks of all components in a restart interval: Ri * mcu
    int lumaseg;            // blocks of component 0 in one: Ri * h0 * v0 (nluma when nrst is 0)
    int bound0;             // first entry of its boundary table; entry m (1 .. nrst): the clean byte offset behind restart marker m
};
struct DecStat {
    unsigned int marker;    // offset of the first real marker in the raw data (raw_n: none)
    unsigned int nbytes;    // clean bytes in front of it
    unsigned int nsub;      // subsequences
    int last_changed;       // the last round in which an exit state changed
    unsigned int blocks;    // blocks completed by all subsequences
    unsigned int err;       // the write pass met what the host decoder refuses
    unsigned int nrst;      // restart markers in front of the first real marker; another count than DecImg::nrst: nsub = 0, irregular
    unsigned int pad;
};

struct DecArgs {
    const uint8_t* raw;
    uint8_t* clean;
    const DecImg* imgs;
    DecStat* stat;
    const DecTab* tabs;
    int n;
    unsigned int* poff;     // bytes that leave the clean string (stuffed zeros, restart markers) in front of every piece
    unsigned int* moff;     // restart markers in front of every piece (images with a restart interval only)
    unsigned int* bound;    // the boundary tables
    unsigned int* entry;    // per subsequence: the entry state of its last decode
    unsigned int* exit;     // 2 x sub_total: exit states of the even / odd rounds
    long long sub_total;
    unsigned int* nblk;     // blocks completed
    unsigned int* bfirst;   // index of the first block
    unsigned int* changed;  // kRing words
    int16_t* coef;          // 64 per block, natural order
    uint8_t* plane;
    uint8_t* host_plane;    // page-locked
    DecStat* host_stat;
    unsigned char nat[64];  // natural index of every zigzag position
};

#include "jpeg_scan.inl"

constexpr long long F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
                    F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
                    F_2_562915447 = 20995, F_3_072711026 = 25172;

__device__ __forceinline__ int descale(long long x, int n) { return (int)((x + (1LL << (n - 1))) >> n); }
__device__ __forceinline__ unsigned int range_limit(int x)
{
    const int v = (((x & 1023) ^ 512) - 512) + 128;           // libjpeg's table is indexed modulo 1024
    return (unsigned int)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one pass of libjpeg's jpeg_idct_islow on 8 values (host: idct_islow in host/jpeg.cpp, the same integers); SHIFT = 11 for the first
// pass (columns), 18 for the second one (rows)
template <int SHIFT>
__device__ __forceinline__ void idct8(const int in[8], int out[8])
{
    long long z2 = in[2], z3 = in[6];
    long long z1 = (z2 + z3) * F_0_541196100;
    long long tmp2 = z1 + z3 * (-F_1_847759065), tmp3 = z1 + z2 * F_0_765366865;
    long long tmp0 = ((long long)in[0] + in[4]) * 8192, tmp1 = ((long long)in[0] - in[4]) * 8192;
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    long long z4 = tmp1 + tmp3;
    const long long z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = descale(tmp10 + tmp3, SHIFT); out[7] = descale(tmp10 - tmp3, SHIFT);
    out[1] = descale(tmp11 + tmp2, SHIFT); out[6] = descale(tmp11 - tmp2, SHIFT);
    out[2] = descale(tmp12 + tmp1, SHIFT); out[5] = descale(tmp12 - tmp1, SHIFT);
    out[3] = descale(tmp13 + tmp0, SHIFT); out[4] = descale(tmp13 - tmp0, SHIFT);
}

__device__ __forceinline__ int image_of(const DecImg* imgs, int n, int group, bool chunks)
{
    int i = 0;
    while (i + 1 < n && (chunks ? imgs[i + 1].chunk0 : imgs[i + 1].wg0) <= group) ++i;
    return i;
}

template <bool RST>
__global__ __launch_bounds__(kScanThreads) void k_jdec_count(DecArgs a)
{
    __shared__ unsigned int wsum[kScanThreads / 64 + 1];
    __shared__ unsigned int s_marker, s_removed, s_markers;
    const int i = blockIdx.x;
    const DecImg im = a.imgs[i];
    const unsigned int raw_n = im.raw_n;
    const uint8_t* raw = a.raw + im.raw0;
    const uint4* src = reinterpret_cast<const uint4*>(raw);
    unsigned int* poff = a.poff + im.piece0;
    unsigned int* moff = a.moff + im.piece0;
    const int npieces = (int)((raw_n + kPieceBytes - 1) / kPieceBytes);
    const bool rst = RST && im.nrst > 0;                      // FF D0 .. FF D7 is a restart marker: both bytes leave, the data goes on
    if (threadIdx.x == 0) { s_marker = raw_n; s_removed = 0; s_markers = 0; }
    __syncthreads();
    unsigned int carry = 0, mcarry = 0, mk = 0xFFFFFFFFu;
    for (int base = 0; base < npieces; base += kScanThreads) {
        const int piece = base + (int)threadIdx.x;
        unsigned int cnt = 0, mc = 0;                         // bytes of the piece that leave; markers whose second byte is in it
        if (piece < npieces) {
            const unsigned int b0 = (unsigned int)piece * kPieceBytes;
            unsigned int prev = b0 ? raw[b0 - 1] : 0u;
#pragma unroll 4
            for (int q = 0; q < kPieceBytes / 16; ++q) {
                const uint4 v = src[(long long)piece * (kPieceBytes / 16) + q];
                const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const unsigned int p = b0 + 16 * q + k;
                    if (p < raw_n) {
                        const unsigned int b = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                        if (prev == 0xFFu) {
                            if (b == 0u) ++cnt;
                            else if (rst && (b & 0xF8u) == 0xD0u) { ++mc; cnt += p > b0 ? 2u : 1u; }    // its FF may be the last byte of the piece in front
                            else mk = min(mk, p - 1);
                        }
                        if (b == 0xFFu && p + 1 == raw_n) mk = min(mk, p);          // an FF at the very end: the host reads a marker there
                        prev = b;
                    }
                }
            }
            // ... and this piece's last byte the FF of a marker whose second byte is the first of the next piece
            if (rst && prev == 0xFFu && b0 + kPieceBytes < raw_n && (raw[b0 + kPieceBytes] & 0xF8u) == 0xD0u) ++cnt;
        }
        unsigned int total;
        const unsigned int pre = block_exclusive(cnt, wsum, &total);
        if (piece < npieces) poff[piece] = carry + pre;
        carry += total;
        if (rst) {                                            // the same for everyone of the workgroup
            const unsigned int mpre = block_exclusive(mc, wsum, &total);
            if (piece < npieces) moff[piece] = mcarry + mpre;
            mcarry += total;
        }
    }
    if (mk != 0xFFFFFFFFu) atomicMin(&s_marker, mk);
    if (threadIdx.x == 0) { poff[npieces] = carry; if (rst) moff[npieces] = mcarry; }
    __syncthreads();
    // what left in front of the marker: the bytes of the pieces before its piece, and those inside it up to the marker; the restart
    // markers in front of it likewise
    const unsigned int marker = s_marker, mp = marker / kPieceBytes;
    if (threadIdx.x < kPieceBytes) {
        const unsigned int p = mp * kPieceBytes + threadIdx.x;
        if (p >= 1 && p < marker && raw[p - 1] == 0xFFu) {
            if (raw[p] == 0u) atomicAdd(&s_removed, 1u);
            else if (rst && (raw[p] & 0xF8u) == 0xD0u) { atomicAdd(&s_removed, 1u); atomicAdd(&s_markers, 1u); }
        }
        if (rst && p + 1 < marker && raw[p] == 0xFFu && (raw[p + 1] & 0xF8u) == 0xD0u) atomicAdd(&s_removed, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        DecStat s = a.stat[i];
        s.marker = marker;
        s.nbytes = marker - (poff[mp] + s_removed);
        s.nsub = (unsigned int)(((unsigned long long)s.nbytes * 8 + kSubBits - 1) / kSubBits);
        s.nrst = rst ? moff[mp] + s_markers : 0u;
        if (s.nrst != (unsigned int)im.nrst) s.nsub = 0u;     // irregular at once: nobody decodes against a table with holes
        a.stat[i] = s;
    }
}

template <bool RST>
__global__ __launch_bounds__(kThreads) void k_jdec_unstuff(DecArgs a)
{
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), nw = gridDim.x * (kThreads / 64);
    for (int i = 0; i < a.n; ++i) {
        const DecImg im = a.imgs[i];
        const unsigned int raw_n = im.raw_n;
        const int npieces = (int)((raw_n + kPieceBytes - 1) / kPieceBytes);
        const uint8_t* raw = a.raw + im.raw0;
        const unsigned int* words = reinterpret_cast<const unsigned int*>(raw);
        const unsigned int* poff = a.poff + im.piece0;
        const unsigned int* moff = a.moff + im.piece0;
        unsigned int* bound = a.bound + im.bound0;
        const bool rst = RST && im.nrst > 0;
        uint8_t* clean = a.clean + im.raw0;
        for (int piece = gw; piece < npieces; piece += nw) {
            const unsigned int byte0 = (unsigned int)piece * kPieceBytes + 4u * lane;
            const int nb = byte0 >= raw_n ? 0 : (int)min(4u, raw_n - byte0);
            const unsigned int x = nb ? words[byte0 >> 2] : 0u;
            unsigned int prev = (nb && byte0) ? raw[byte0 - 1] : 0u;
            const unsigned int next = (rst && nb == 4 && byte0 + 4u < raw_n) ? raw[byte0 + 4u] : 0u;
            int cnt = 0;                                      // bytes that leave, and in the upper half the markers among them
            unsigned int removed = 0, marks = 0;
            for (int j = 0; j < nb; ++j) {
                const unsigned int b = (x >> (8 * j)) & 0xFFu;
                if (prev == 0xFFu && b == 0u) { ++cnt; removed |= 1u << j; }
                else if (rst) {                               // as k_jdec_count: the second byte of a restart marker, or the FF of one
                    if (prev == 0xFFu && (b & 0xF8u) == 0xD0u) { cnt += 0x10001; removed |= 1u << j; marks |= 1u << j; }
                    else if (b == 0xFFu) {
                        const unsigned int b2 = j + 1 < nb ? (x >> (8 * (j + 1))) & 0xFFu : (j == 3 ? next : 0u);
                        if ((b2 & 0xF8u) == 0xD0u) { ++cnt; removed |= 1u << j; }
                    }
                }
                prev = b;
            }
            const unsigned int before = (unsigned int)wave_exclusive(cnt, lane);             // at most 256 and 128: no carry between the halves
            unsigned int pos = byte0 - poff[piece] - (before & 0xFFFFu);
            unsigned int m = rst ? moff[piece] + (before >> 16) : 0u;
            for (int j = 0; j < nb; ++j) {
                if (!((removed >> j) & 1u)) clean[pos++] = (uint8_t)(x >> (8 * j));
                else if ((marks >> j) & 1u) { ++m; if (m <= (unsigned int)im.nrst) bound[m] = pos; }      // a marker past the table is dropped
            }
        }
    }
}

template <int NP>
struct DecLds {             // NP = 1: a batch of grey images (3040 B); NP = kMaxPairs: a batch that holds a three-component one (8992 B)
    DecPair pair[NP];
    unsigned char nat[64];
};

template <int NP>
__device__ __forceinline__ void load_tables(DecLds<NP>& t, const DecTab& g, const unsigned char* nat)
{
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        DecPair& tp = t.pair[q]; const DecPair& gp = g.pair[q];
        for (int k = threadIdx.x; k < 1024; k += kSyncThreads) (&tp.look[0][0])[k] = (&gp.look[0][0])[k];
        for (int k = threadIdx.x; k < 34; k += kSyncThreads) { (&tp.mincode[0][0])[k] = (&gp.mincode[0][0])[k]; (&tp.valptr[0][0])[k] = (&gp.valptr[0][0])[k]; }
        for (int k = threadIdx.x; k < 36; k += kSyncThreads) (&tp.maxcode[0][0])[k] = (&gp.maxcode[0][0])[k];
        for (int k = threadIdx.x; k < 512; k += kSyncThreads) (&tp.vals[0][0])[k] = (&gp.vals[0][0])[k];
    }
    for (int k = threadIdx.x; k < 64; k += kSyncThreads) t.nat[k] = nat[k];
}

__device__ __forceinline__ int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// Decodes the symbols that START in the subsequence [start, start + kSubBits) of the clean bit string (total bits) from the entry state.
// COLOR = false (every image of the batch has one component): the state is (bit overhang << 8 | zigzag index, 0 = DC next).  COLOR =
// true: (bit overhang << 12 | j << 8 | zigzag index) with j the place of the block inside its MCU, 0 .. mcu - 1; places below hv hold
// component 0, the table pair of every place is in `pairs`.  Two states are equal only if all parts are; kStop (zigzag index 255) and
// kNoEntry are no state of either kind.  Returns the exit state; nb = blocks completed, of all components.  A block is complete at an
// EOB, at a coefficient in place 63, and where a run leaves the block (a ZRL as in the host decoder; any other run is flagged in err,
// as are an undecodable code and a DC category above 11 -- the host decoder refuses those, this one goes on so that the state it
// reaches is a function of the entry state alone).  WRITE: the coefficients (DC: the difference) of component 0's blocks to coef,
// inside [0, nluma): block first + nb of the scan is a block of component 0 iff (first + nb) % mcu < hv, and then its number
// (first + nb) / mcu * hv + (first + nb) % mcu; the symbols of the other components are decoded and dropped.
// Restart intervals (nrst > 0): bound[1 .. nrst] are the places of the restart markers in the clean string, in bytes.  Every one is a
// true entry state -- byte aligned, DC next, place 0, all predictors 0 -- so a symbol that would end behind the next boundary is not
// decoded (it is the 1-bit padding, which no Huffman code consists of): the decoder jumps to the boundary with the fresh state and
// goes on; what it leaves the subsequence with no longer depends on what it entered with.  The last boundary is the end of the data,
// which the loop compares against anyway: a stream without restarts takes the same turns as before.  WRITE: at every jump the state
// has to be (DC next, place 0) and the running block index m * ribl, or err is set -- a block too many, decoded out of padding that
// is not 1-bits, breaks the count and cannot give other samples.  RST = false (no image of the batch has restart markers): none of
// this is compiled in, and nrst is 0.
struct DecMcu { unsigned int mcu, hv, pairs, nrst, ribl; const unsigned int* bound; };
template <bool WRITE, bool COLOR, bool RST>
__device__ __forceinline__ unsigned int decode_sub(const DecLds<COLOR ? kMaxPairs : 1>& t, const unsigned int* words, unsigned int start, unsigned int total,
                                                   unsigned int entry, unsigned int& nb, int16_t* coef, unsigned int first, unsigned int nluma,
                                                   unsigned int& err, const DecMcu mc)
{
    nb = 0;
    if (entry == kStop) return kStop;
    const unsigned int end = start + kSubBits;
    unsigned int p = start + (entry >> (COLOR ? 12 : 8));
    int k = (int)(entry & 0xFFu);
    unsigned int j = 0, q = 0, lb = first;                    // COLOR: place in the MCU by the state / by the running index, next block of component 0
    const DecPair* tp = &t.pair[0];
    if constexpr (COLOR) {
        j = (entry >> 8) & 15u;
        tp = &t.pair[(mc.pairs >> (4u * j)) & 3u];
        if (WRITE) { const unsigned int u = first / mc.mcu; q = first - u * mc.mcu; lb = u * mc.hv + min(q, mc.hv); }
    }
    unsigned int m = 1u, lim = total;                         // the next boundary: restart marker m, or (m > nrst) the end of the data
    if (RST && mc.nrst) {                                     // the first one at or behind the entry position
        unsigned int lo = 1u, hi = mc.nrst + 1u;
        while (lo < hi) { const unsigned int mid = (lo + hi) >> 1; if (mc.bound[mid] * 8u >= p) hi = mid; else lo = mid + 1u; }
        m = lo;
        if (m <= mc.nrst) lim = mc.bound[m] * 8u;
    }
    unsigned int wi = 0xFFFFFFFFu, w0 = 0, w1 = 0;
    while (p < end) {                                         // at least one bit per turn, or forward to a boundary
        if (p >= lim) {
            if (!RST || m > mc.nrst) break;                   // the end of the data
            if (WRITE && (k != 0 || j != 0u || first + nb != m * mc.ribl)) err = 1u;
            p = lim; k = 0;                                   // restart marker m: byte aligned, DC next, place 0
            if constexpr (COLOR) { j = 0u; tp = &t.pair[0]; }
            ++m; lim = m <= mc.nrst ? mc.bound[m] * 8u : total;
            continue;
        }
        if ((p >> 5) != wi) { wi = p >> 5; w0 = __builtin_bswap32(words[wi]); w1 = __builtin_bswap32(words[wi + 1]); }
        const unsigned int bits = (unsigned int)(((((unsigned long long)w0) << 32) | w1) >> (32 - (p & 31)));
        const int tc = k ? 1 : 0;
        const unsigned int e = tp->look[tc][bits >> 23];
        int len = (int)(e >> 8), sym = (int)(e & 0xFFu);
        if (!e) {                                             // longer than 9 bits: F.2.2.3
            for (int l = 10; l <= 16; ++l) {
                const int code = (int)(bits >> (32 - l));
                if (tp->maxcode[tc][l] >= 0 && code <= tp->maxcode[tc][l] && code >= tp->mincode[tc][l]) { len = l; sym = tp->vals[tc][tp->valptr[tc][l] + code - tp->mincode[tc][l]]; break; }
            }
            if (!len) {
                if (p + 16 > lim) { if (!RST || m > mc.nrst) return kStop; p = lim; continue; }      // the data, or the interval, ends inside what may be a code
                err = 1u; len = 16; sym = 0;
            }
        }
        bool complete = false;
        if (k == 0) {
            const int s = sym & 15;
            if (p + len + s > lim) { if (!RST || m > mc.nrst) return kStop; p = lim; continue; }     // before the verdict: behind the last block the window holds leftovers
            if (sym > 11) err = 1u;
            if constexpr (COLOR) { if (WRITE && s && q < mc.hv && lb < nluma) coef[(long long)lb * 64] = (int16_t)extend((int)((bits << len) >> (32 - s)), s); }
            else { if (WRITE && s && first + nb < nluma) coef[(long long)(first + nb) * 64] = (int16_t)extend((int)((bits << len) >> (32 - s)), s); }
            p += len + s; k = 1;
        } else {
            const int r = sym >> 4, s = sym & 15;
            if (p + len + s > lim) { if (!RST || m > mc.nrst) return kStop; p = lim; continue; }
            if (s == 0) {
                if (r == 15) { k += 16; complete = k >= 64; }
                else complete = true;
            } else {
                k += r;
                if (k > 63) { err = 1u; complete = true; }
                else {
                    if constexpr (COLOR) { if (WRITE && q < mc.hv && lb < nluma) coef[(long long)lb * 64 + t.nat[k]] = (int16_t)extend((int)((bits << len) >> (32 - s)), s); }
                    else { if (WRITE && first + nb < nluma) coef[(long long)(first + nb) * 64 + t.nat[k]] = (int16_t)extend((int)((bits << len) >> (32 - s)), s); }
                    ++k; complete = k == 64;
                }
            }
            p += len + s;
        }
        if (complete) {
            ++nb; k = 0;
            if constexpr (COLOR) {
                j = j + 1u == mc.mcu ? 0u : j + 1u;
                tp = &t.pair[(mc.pairs >> (4u * j)) & 3u];
                if (WRITE) { if (q < mc.hv) ++lb; q = q + 1u == mc.mcu ? 0u : q + 1u; }
            }
        }
    }
    if (RST && WRITE && m <= mc.nrst && end >= total) err = 1u;       // the last subsequence: a boundary nobody jumped (a marker at the very end)
    return p >= end ? (((p - end) << (COLOR ? 12 : 8)) | (COLOR ? j << 8 : 0u) | (unsigned int)k) : kStop;
}

template <bool COLOR, bool RST>
__global__ __launch_bounds__(kSyncThreads) void k_jdec_sync(DecArgs a, int round)
{
    __shared__ DecLds<COLOR ? kMaxPairs : 1> t;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.changed[(round + 1) % kRing] = 0u;
    if (round > 0 && a.changed[(round - 1) % kRing] == 0u) return;           // the iteration has ended: nothing to do, for everyone
    const int i = image_of(a.imgs, a.n, blockIdx.x, false);
    const DecImg im = a.imgs[i];
    const unsigned int nsub = a.stat[i].nsub, total = a.stat[i].nbytes * 8u;
    const unsigned int s = (unsigned int)(blockIdx.x - im.wg0) * kSyncThreads + threadIdx.x;
    const long long g = im.sub0 + (long long)s;
    const unsigned int* prev = a.exit + (long long)((round + 1) & 1) * a.sub_total;
    unsigned int* cur = a.exit + (long long)(round & 1) * a.sub_total;
    const bool mine = s < nsub;
    unsigned int entry = 0u, old_exit = kNoEntry;
    bool need = false;
    if (mine) {
        if (round > 0) { if (s > 0) entry = prev[g - 1]; old_exit = prev[g]; }
        need = round == 0 || entry != a.entry[g];
        if (!need) cur[g] = old_exit;
    }
    if (!__syncthreads_or(need ? 1 : 0)) return;
    load_tables(t, a.tabs[i], a.nat);
    __syncthreads();
    bool changed = false;
    if (need) {
        unsigned int nb, err = 0;
        const unsigned int ex = decode_sub<false, COLOR, RST>(t, reinterpret_cast<const unsigned int*>(a.clean + im.raw0), s * kSubBits, total, entry, nb, nullptr, 0, 0, err,
                                                         DecMcu{(unsigned int)im.mcu, (unsigned int)(im.h0 * im.v0), im.pairs, (unsigned int)im.nrst, (unsigned int)im.ribl, a.bound + im.bound0});
        a.entry[g] = entry; a.nblk[g] = nb; cur[g] = ex;
        changed = ex != old_exit;
    }
    if (__ballot(changed) && (threadIdx.x & 63) == 0) { atomicOr(&a.changed[round % kRing], 1u); atomicMax(&a.stat[i].last_changed, round); }
}

__global__ __launch_bounds__(kScanThreads) void k_jdec_blocks(DecArgs a)
{
    __shared__ unsigned int wsum[kScanThreads / 64 + 1];
    const int i = blockIdx.x;
    const DecImg im = a.imgs[i];
    const int nsub = (int)a.stat[i].nsub;
    unsigned int carry = 0;
    for (int base = 0; base < nsub; base += kScanThreads) {
        const int s = base + (int)threadIdx.x;
        const unsigned int cnt = s < nsub ? a.nblk[im.sub0 + s] : 0u;
        unsigned int total;
        const unsigned int pre = block_exclusive(cnt, wsum, &total);
        if (s < nsub) a.bfirst[im.sub0 + s] = carry + pre;
        carry += total;
    }
    if (threadIdx.x == 0) a.stat[i].blocks = carry;
}

template <bool COLOR, bool RST>
__global__ __launch_bounds__(kSyncThreads) void k_jdec_write(DecArgs a)
{
    __shared__ DecLds<COLOR ? kMaxPairs : 1> t;
    const int i = image_of(a.imgs, a.n, blockIdx.x, false);
    const DecImg im = a.imgs[i];
    const DecStat st = a.stat[i];
    if (st.blocks != (unsigned int)im.nblk) return;           // irregular: the host decoder gives the verdict
    const unsigned int s = (unsigned int)(blockIdx.x - im.wg0) * kSyncThreads + threadIdx.x;
    if ((unsigned int)(blockIdx.x - im.wg0) * kSyncThreads >= st.nsub) return;
    load_tables(t, a.tabs[i], a.nat);
    __syncthreads();
    unsigned int err = 0;
    if (s < st.nsub) {
        const long long g = im.sub0 + (long long)s;
        unsigned int nb;
        decode_sub<true, COLOR, RST>(t, reinterpret_cast<const unsigned int*>(a.clean + im.raw0), s * kSubBits, st.nbytes * 8u, a.entry[g], nb,
                                a.coef + (long long)im.blk0 * 64, a.bfirst[g], (unsigned int)im.nluma, err,
                                DecMcu{(unsigned int)im.mcu, (unsigned int)(im.h0 * im.v0), im.pairs, (unsigned int)im.nrst, (unsigned int)im.ribl, a.bound + im.bound0});
    }
    if (__ballot(err != 0u) && (threadIdx.x & 63) == 0) atomicOr(&a.stat[i].err, 1u);
}

template <bool RST>
__global__ __launch_bounds__(kScanThreads) void k_jdec_dc(DecArgs a)
{
    __shared__ unsigned int wsum[kScanThreads / 64 + 1];
    __shared__ unsigned int pfx[RST ? kScanThreads : 1];
    const int i = blockIdx.x;
    const DecImg im = a.imgs[i];
    if (a.stat[i].blocks != (unsigned int)im.nblk) return;
    int16_t* coef = a.coef + (long long)im.blk0 * 64;
    const int per = (im.nluma + kScanThreads - 1) / kScanThreads;
    const int b0 = min(im.nluma, (int)threadIdx.x * per), b1 = min(im.nluma, b0 + per);
    int sum = 0;
    for (int b = b0; b < b1; ++b) sum += coef[(long long)b * 64];
    unsigned int total;
    int pred = (int)block_exclusive((unsigned int)sum, wsum, &total);
    // restart intervals: the sum starts again at every multiple of lumaseg blocks, so a thread's predictor is the plain prefix less the
    // plain prefix of the segment start in front of it -- which is in the range of the thread s0 / per (integers: exact whatever the wrap)
    const bool rst = RST && im.nrst > 0;                      // the same for everyone of the workgroup
    const int seg = im.lumaseg;
    if (rst) {
        pfx[threadIdx.x] = (unsigned int)pred;
        __syncthreads();
        const int s0 = b0 - b0 % seg;
        if (b0 < b1 && s0 > 0) {
            const int owner = s0 / per;
            unsigned int ps = pfx[owner];
            for (int b = owner * per; b < s0; ++b) ps += (unsigned int)(int)coef[(long long)b * 64];
            pred = (int)((unsigned int)pred - ps);
        }
        __syncthreads();                                      // everyone has read the differences it needs before anyone overwrites one
    }
    int r = rst ? b0 % seg : 1;
    for (int b = b0; b < b1; ++b) {
        if (r == 0) pred = 0;
        pred += coef[(long long)b * 64]; coef[(long long)b * 64] = (int16_t)pred;
        if (rst && ++r == seg) r = 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_jdec_idct(DecArgs a)
{
    // a wave's 8 blocks: element (block j, row r, column c) at 64 r + 8 j + ((r + c) & 7), so that the 64 lanes of either pass, (j, c)
    // at one r and (j, r) at one c, fall into 64 different banks
    __shared__ int tile[kThreads / 64][512];
    __shared__ int quant[64];
    const int chunk = blockIdx.x;
    const int i = image_of(a.imgs, a.n, chunk, true);
    const DecImg im = a.imgs[i];
    if (a.stat[i].blocks != (unsigned int)im.nblk) return;
    if (threadIdx.x < 64) quant[threadIdx.x] = a.tabs[i].quant[threadIdx.x];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = lane >> 3, c = lane & 7;
    const int lb = (chunk - im.chunk0) * kChunkBlocks + wave * 8 + j;
    int* t = tile[wave] + 8 * j;
    if (lb < im.nluma) {                              // columns: lane = (block j, column c)
        const int16_t* in = a.coef + ((long long)im.blk0 + lb) * 64;
        int d[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = (int)in[8 * r + c] * quant[8 * r + c];
        idct8<11>(d, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) t[64 * r + ((r + c) & 7)] = o[r];
    }
    __syncthreads();
    if (lb < im.nluma) {                              // rows: lane = (block j, row c)
        int d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = t[64 * c + ((c + k) & 7)];
        idct8<18>(d, o);
        const int hv = im.h0 * im.v0, m = lb / hv, q = lb - m * hv;               // decode order: MCU m, place q inside it (h0 x v0, rows first)
        const int my = m / im.mcux, qy = q / im.h0;
        const int by = my * im.v0 + qy, bx = (m - my * im.mcux) * im.h0 + (q - qy * im.h0);
        uint2 v;
        v.x = range_limit(o[0]) | (range_limit(o[1]) << 8) | (range_limit(o[2]) << 16) | (range_limit(o[3]) << 24);
        v.y = range_limit(o[4]) | (range_limit(o[5]) << 8) | (range_limit(o[6]) << 16) | (range_limit(o[7]) << 24);
        *reinterpret_cast<uint2*>(a.plane + im.plane0 + (long long)(8 * by + c) * (8 * im.bw) + 8 * bx) = v;
    }
}

__global__ __launch_bounds__(kThreads) void k_jdec_out(DecArgs a)
{
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x, nt = (long long)gridDim.x * kThreads;
    for (int i = 0; i < a.n; ++i) {
        const DecImg im = a.imgs[i];
        if (a.stat[i].blocks != (unsigned int)im.nblk) continue;
        const long long n16 = ((long long)8 * im.bw * im.h + 15) / 16;          // the rows of the image; a plane is a multiple of 64 bytes
        const uint4* src = reinterpret_cast<const uint4*>(a.plane + im.plane0);
        uint4* dst = reinterpret_cast<uint4*>(a.host_plane + im.plane0);
        for (long long k = tid; k < n16; k += nt) dst[k] = src[k];
    }
    if (tid < a.n) a.host_stat[tid] = a.stat[tid];
}

long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

}  // namespace

struct lpslam_hip_jpeg_dec {
    int device = 0;
    int max_w = 0, max_h = 0, max_images = 0;
    bool color = false;                // made with LPSLAM_HIP_JPEG_DEC_COLOR: takes three-component streams too
    long long max_blocks = 0;          // per image
    long long raw_cap = 0;             // entropy-coded bytes per image
    long long plane_cap = 0;           // per image
    long long head_bytes = 0;          // image table, results and decoding tables in front of the raw data in the upload
    long long raw_total = 0, sub_total = 0, piece_total = 0;
    hipStream_t stream = nullptr;
    uint8_t* h_up = nullptr;           // page-locked: everything one call uploads
    uint8_t* d_up = nullptr;
    uint8_t* d_clean = nullptr;
    bool take_restart = false;         // lpslam_hip_jpeg_dec_take_restart: streams with a restart interval are decoded too
    unsigned int *d_moff = nullptr, *d_bound = nullptr;
    unsigned int *d_poff = nullptr, *d_entry = nullptr, *d_exit = nullptr, *d_nblk = nullptr, *d_bfirst = nullptr, *d_changed = nullptr;
    int16_t* d_coef = nullptr;
    uint8_t* d_plane = nullptr;
    uint8_t* h_plane = nullptr;        // page-locked: written by k_jdec_out
    DecStat* h_stat = nullptr;
    unsigned int* h_changed = nullptr;
    uint8_t* dh_plane = nullptr;       // their device addresses
    DecStat* dh_stat = nullptr;
    std::vector<int32_t> last_rounds, last_subs, last_blocks;
    std::mutex mutex;
};

namespace {
void jdec_free(lpslam_hip_jpeg_dec* e)
{
    if (!e) return;
    if (e->stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->stream); }
    for (void* p : {(void*)e->d_up, (void*)e->d_clean, (void*)e->d_moff, (void*)e->d_bound, (void*)e->d_poff, (void*)e->d_entry, (void*)e->d_exit, (void*)e->d_nblk, (void*)e->d_bfirst,
                    (void*)e->d_changed, (void*)e->d_coef, (void*)e->d_plane})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)e->h_up, (void*)e->h_plane, (void*)e->h_stat, (void*)e->h_changed})
        if (p) (void)hipHostFree(p);
    delete e;
}

// what the host learns about one stream before anything is launched
struct Parsed {
    LpSlam::jpeg::Header hd;
    LpSlam::jpeg::Scan scan;
    int status = LPSLAM_HIP_JPEG_IRREGULAR;
    int dev = -1;                      // its place in the device batch
};
}  // namespace

extern "C" {

int lpslam_hip_jpeg_dec_create(int32_t max_width, int32_t max_height, int32_t max_images, lpslam_hip_jpeg_dec** out)
{
    return lpslam_hip_jpeg_dec_create2(max_width, max_height, max_images, 0u, out);
}

int lpslam_hip_jpeg_dec_create2(int32_t max_width, int32_t max_height, int32_t max_images, uint32_t flags, lpslam_hip_jpeg_dec** out)
{
    if (!out) { set_error("jpeg_dec_create: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    *out = nullptr;
    if (max_width < 1 || max_height < 1 || max_width > 65535 || max_height > 65535 || max_images < 1 || max_images > 256) {
        set_error("jpeg_dec_create: sizes out of range (1 .. 65535 samples, 1 .. 256 images)");
        return LPSLAM_HIP_ERR_INVALID;
    }
    if (flags & ~(uint32_t)LPSLAM_HIP_JPEG_DEC_COLOR) { set_error("jpeg_dec_create: unknown flag bits 0x%x", flags & ~(uint32_t)LPSLAM_HIP_JPEG_DEC_COLOR); return LPSLAM_HIP_ERR_INVALID; }
    const bool color = (flags & LPSLAM_HIP_JPEG_DEC_COLOR) != 0;
    // component 0's blocks: whole 8 x 8 blocks of a grey image; whole 16 x 16 MCUs (the largest of the class, 2 x 2) of a colour one
    const long long bw = color ? (max_width + 15) / 16 * 2 : (max_width + 7) / 8, bh = color ? (max_height + 15) / 16 * 2 : (max_height + 7) / 8, blocks = bw * bh;
    // entropy-coded data the decoder takes: 4 bytes per sample (a coefficient has at most 26 bits; twice that with every byte stuffed),
    // and three coefficients per sample of component 0 in a 4:4:4 stream
    const long long raw_cap = align_up(blocks * 64 * (color ? 12 : 4) + 4096, kPieceBytes);
    if (raw_cap * 8 >= (1LL << 31)) { set_error("jpeg_dec_create: image too large for 32-bit bit offsets"); return LPSLAM_HIP_ERR_INVALID; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("jpeg_dec_create: no HIP device (the host decoder is LpSlam::decode_jpeg_gray)"); return LPSLAM_HIP_ERR_DEVICE; }
    lpslam_hip_jpeg_dec* e = new (std::nothrow) lpslam_hip_jpeg_dec();
    if (!e) { set_error("jpeg_dec_create: out of host memory"); return LPSLAM_HIP_ERR_INVALID; }
    e->max_w = max_width; e->max_h = max_height; e->max_images = max_images; e->max_blocks = blocks; e->color = color;
    e->raw_cap = raw_cap; e->plane_cap = blocks * 64;
    e->head_bytes = align_up((long long)(sizeof(DecImg) + sizeof(DecStat) + sizeof(DecTab)) * max_images, kPieceBytes);
    e->raw_total = (raw_cap + kPieceBytes) * max_images + kPieceBytes;            // every image: its bytes and a piece of slack for the readers
    e->sub_total = e->raw_total * 8 / kSubBits + 2 * max_images;
    e->piece_total = e->raw_total / kPieceBytes + 2 * max_images;
    e->last_rounds.assign(max_images, 0); e->last_subs.assign(max_images, 0); e->last_blocks.assign(max_images, 0);
    auto fail = [&](hipError_t err, const char* what) { const int rc = hip_fail(err, what); jdec_free(e); return rc; };
    hipError_t err;
    if ((err = hipGetDevice(&e->device)) != hipSuccess) return fail(err, "hipGetDevice");
    if ((err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return fail(err, "hipStreamCreateWithFlags");
    if ((err = hipMalloc((void**)&e->d_up, (size_t)(e->head_bytes + e->raw_total))) != hipSuccess) return fail(err, "hipMalloc(jpeg streams)");
    if ((err = hipMalloc((void**)&e->d_clean, (size_t)e->raw_total)) != hipSuccess) return fail(err, "hipMalloc(jpeg clean data)");
    if ((err = hipMalloc((void**)&e->d_poff, (size_t)e->piece_total * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg pieces)");
    if ((err = hipMalloc((void**)&e->d_moff, (size_t)e->piece_total * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg restart markers)");
    if ((err = hipMalloc((void**)&e->d_bound, (size_t)((blocks + 1) * max_images) * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg boundaries)");
    if ((err = hipMalloc((void**)&e->d_entry, (size_t)e->sub_total * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg entry states)");
    if ((err = hipMalloc((void**)&e->d_exit, (size_t)e->sub_total * 8)) != hipSuccess) return fail(err, "hipMalloc(jpeg exit states)");
    if ((err = hipMalloc((void**)&e->d_nblk, (size_t)e->sub_total * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg block counts)");
    if ((err = hipMalloc((void**)&e->d_bfirst, (size_t)e->sub_total * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg first blocks)");
    if ((err = hipMalloc((void**)&e->d_changed, kRing * 4)) != hipSuccess) return fail(err, "hipMalloc(jpeg rounds)");
    if ((err = hipMalloc((void**)&e->d_coef, (size_t)(blocks * max_images) * 64 * sizeof(int16_t))) != hipSuccess) return fail(err, "hipMalloc(jpeg coefficients)");
    if ((err = hipMalloc((void**)&e->d_plane, (size_t)(e->plane_cap * max_images))) != hipSuccess) return fail(err, "hipMalloc(jpeg planes)");
    if ((err = hipHostMalloc((void**)&e->h_up, (size_t)(e->head_bytes + e->raw_total))) != hipSuccess) return fail(err, "hipHostMalloc(jpeg streams)");
    if ((err = hipHostMalloc((void**)&e->h_plane, (size_t)(e->plane_cap * max_images), hipHostMallocMapped)) != hipSuccess) return fail(err, "hipHostMalloc(jpeg planes)");
    if ((err = hipHostMalloc((void**)&e->h_stat, sizeof(DecStat) * max_images, hipHostMallocMapped)) != hipSuccess) return fail(err, "hipHostMalloc(jpeg results)");
    if ((err = hipHostMalloc((void**)&e->h_changed, 4)) != hipSuccess) return fail(err, "hipHostMalloc(jpeg rounds)");
    if ((err = hipHostGetDevicePointer((void**)&e->dh_plane, e->h_plane, 0)) != hipSuccess) return fail(err, "hipHostGetDevicePointer(jpeg planes)");
    if ((err = hipHostGetDevicePointer((void**)&e->dh_stat, e->h_stat, 0)) != hipSuccess) return fail(err, "hipHostGetDevicePointer(jpeg results)");
    if ((err = hipMemset(e->d_up, 0, (size_t)(e->head_bytes + e->raw_total))) != hipSuccess) return fail(err, "hipMemset(jpeg streams)");
    if ((err = hipMemset(e->d_clean, 0, (size_t)e->raw_total)) != hipSuccess) return fail(err, "hipMemset(jpeg clean data)");
    *out = e;
    return LPSLAM_HIP_OK;
}

void lpslam_hip_jpeg_dec_destroy(lpslam_hip_jpeg_dec* dec) { jdec_free(dec); }

int lpslam_hip_jpeg_decode(lpslam_hip_jpeg_dec* e, int32_t n, const uint8_t* const* streams, const int64_t* stream_sizes,
                           uint8_t* const* outs, const int32_t* out_strides, const int64_t* out_caps,
                           int32_t* widths, int32_t* heights, int32_t* status)
{
    using namespace LpSlam;
    if (!e || !streams || !stream_sizes || !outs || !out_strides || !out_caps || !widths || !heights || !status) { set_error("jpeg_decode: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (n < 1 || n > e->max_images) { set_error("jpeg_decode: %d streams, the decoder takes 1 .. %d", n, e->max_images); return LPSLAM_HIP_ERR_INVALID; }
    for (int i = 0; i < n; ++i)
        if (!streams[i] || stream_sizes[i] < 0 || !outs[i]) { set_error("jpeg_decode: stream %d is null or has a negative size", i); return LPSLAM_HIP_ERR_INVALID; }
    std::lock_guard<std::mutex> lock(e->mutex);
    std::fill(e->last_rounds.begin(), e->last_rounds.end(), 0); std::fill(e->last_subs.begin(), e->last_subs.end(), 0); std::fill(e->last_blocks.begin(), e->last_blocks.end(), 0);

    // headers: on the host, by the routine the host decoder uses
    std::vector<Parsed> ps((size_t)n);
    DecImg* imgs = reinterpret_cast<DecImg*>(e->h_up);
    DecStat* stats = reinterpret_cast<DecStat*>(e->h_up + sizeof(DecImg) * e->max_images);
    DecTab* tabs = reinterpret_cast<DecTab*>(e->h_up + (sizeof(DecImg) + sizeof(DecStat)) * e->max_images);
    uint8_t* h_raw = e->h_up + e->head_bytes;
    int nd = 0, blk = 0, piece = 0, sub = 0, wg = 0, chunks = 0, bnd = 0;
    bool any_color = false;                                   // the batch holds a three-component image: the kernels that know the MCU
    bool any_rst = false;                                     // ... an image with restart markers: the kernels that know the boundaries
    long long raw = 0, plane = 0;
    unsigned int max_sub = 0;
    bool fits = true;
    for (int i = 0; i < n; ++i) {
        Parsed& p = ps[(size_t)i];
        widths[i] = heights[i] = 0; status[i] = LPSLAM_HIP_JPEG_IRREGULAR;
        const uint8_t* d = streams[i]; const size_t size = (size_t)stream_sizes[i];
        if (!jpeg::has_soi(d, size)) continue;
        size_t pos = 2;
        const jpeg::Walk w = jpeg::walk_to_scan(d, size, pos, p.hd, p.scan, nullptr);
        if (p.hd.have_frame) { widths[i] = p.hd.X; heights[i] = p.hd.Y; }
        if (w != jpeg::Walk::scan) continue;
        const jpeg::Header& hd = p.hd;
        const long long raw_n = (long long)(size - p.scan.data);
        if (raw_n < 1) continue;
        const bool grey = jpeg::grey_scan(hd, e->take_restart);
        const bool ycc = e->color && jpeg::interleaved_ycc_scan(hd, p.scan, e->take_restart);
        if (!(grey || ycc) || hd.X > e->max_w || hd.Y > e->max_h || raw_n > e->raw_cap) {
            p.status = status[i] = LPSLAM_HIP_JPEG_NOT_TAKEN;
            continue;
        }
        if (out_strides[i] < hd.X || out_caps[i] < (int64_t)(hd.Y - 1) * out_strides[i] + hd.X) fits = false;
        p.dev = nd;
        DecImg& im = imgs[nd];
        im.raw0 = raw; im.plane0 = plane; im.raw_n = (unsigned int)raw_n;
        // the plane of component 0 is whole MCUs (hd.plane_w x hd.plane_h; whole blocks for one component, whose h and v the walk sets to 1)
        im.w = hd.X; im.h = hd.Y; im.bw = hd.plane_w / 8; im.nluma = im.bw * (hd.plane_h / 8);
        im.h0 = hd.comp[0].h; im.v0 = hd.comp[0].v; im.mcux = im.bw / im.h0;
        im.mcu = im.h0 * im.v0 + (ycc ? 2 : 0); im.nblk = im.nluma / (im.h0 * im.v0) * im.mcu;
        im.pairs = 0u;
        any_color = any_color || ycc;
        // restart intervals: a table entry per marker the data must hold (fewer than its MCUs, so than the blocks the table is sized by)
        im.nrst = jpeg::restart_markers(hd, im.nluma / (im.h0 * im.v0));
        im.ribl = im.nrst ? hd.restart_interval * im.mcu : 0; im.lumaseg = im.nrst ? hd.restart_interval * im.h0 * im.v0 : im.nluma;
        im.bound0 = bnd; bnd += im.nrst + 1;
        any_rst = any_rst || im.nrst > 0;
        im.blk0 = blk; im.piece0 = piece; im.sub0 = sub;
        const unsigned int nsub_cap = (unsigned int)((raw_n * 8 + kSubBits - 1) / kSubBits);
        im.wg0 = wg; im.nwg = (int)((nsub_cap + kSyncThreads - 1) / kSyncThreads);
        im.chunk0 = chunks; im.nchunks = (im.nluma + kChunkBlocks - 1) / kChunkBlocks;
        DecStat& st = stats[nd];
        st = DecStat{}; st.marker = im.raw_n; st.last_changed = -1;
        DecTab& t = tabs[nd];
        // the distinct (DC, AC) pairs of the scan's components, component 0's first; every place of the MCU names its pair
        int npairs = 0, pair_td[kMaxPairs], pair_ta[kMaxPairs];
        for (int ci = 0; ci < hd.ncomp; ++ci) {
            int q = 0;
            while (q < npairs && (pair_td[q] != hd.comp[ci].td || pair_ta[q] != hd.comp[ci].ta)) ++q;
            if (q == npairs) {
                pair_td[q] = hd.comp[ci].td; pair_ta[q] = hd.comp[ci].ta; ++npairs;
                const jpeg::HuffTable* ht[2] = {&hd.dc[pair_td[q]], &hd.ac[pair_ta[q]]};
                DecPair& tp = t.pair[q];
                for (int c = 0; c < 2; ++c) {
                    std::memcpy(tp.look[c], ht[c]->look, sizeof(tp.look[c]));
                    std::memcpy(tp.mincode[c], ht[c]->mincode, sizeof(tp.mincode[c])); std::memcpy(tp.maxcode[c], ht[c]->maxcode, sizeof(tp.maxcode[c]));
                    std::memcpy(tp.valptr[c], ht[c]->valptr, sizeof(tp.valptr[c])); std::memcpy(tp.vals[c], ht[c]->vals, sizeof(tp.vals[c]));
                }
            }
            if (ci > 0) im.pairs |= (unsigned int)q << (4 * (im.h0 * im.v0 + ci - 1));
        }
        for (int q = npairs; q < kMaxPairs; ++q) t.pair[q] = t.pair[0];              // staged in LDS with the others: defined bytes
        std::memcpy(t.quant, hd.quant[hd.comp[0].tq], sizeof(t.quant));
        std::memcpy(h_raw + raw, d + p.scan.data, (size_t)raw_n);
        raw += align_up(raw_n + 32, kPieceBytes); plane += (long long)im.nluma * 64;
        blk += im.nluma; piece += (int)((raw_n + kPieceBytes - 1) / kPieceBytes) + 1; sub += (int)nsub_cap + 1;
        wg += im.nwg; chunks += im.nchunks;
        max_sub = std::max(max_sub, nsub_cap);
        ++nd;
    }
    if (!fits) { set_error("jpeg_decode: an output buffer is smaller than its image (widths[] / heights[] hold the sizes)"); return LPSLAM_HIP_ERR_INVALID; }
    if (nd == 0) return LPSLAM_HIP_OK;

    LP_HIP(hipSetDevice(e->device));
    DecArgs a{};
    a.raw = e->d_up + e->head_bytes; a.clean = e->d_clean;
    a.imgs = reinterpret_cast<const DecImg*>(e->d_up);
    a.stat = reinterpret_cast<DecStat*>(e->d_up + sizeof(DecImg) * e->max_images);
    a.tabs = reinterpret_cast<const DecTab*>(e->d_up + (sizeof(DecImg) + sizeof(DecStat)) * e->max_images);
    a.n = nd; a.poff = e->d_poff; a.moff = e->d_moff; a.bound = e->d_bound; a.entry = e->d_entry; a.exit = e->d_exit; a.sub_total = e->sub_total; a.nblk = e->d_nblk; a.bfirst = e->d_bfirst;
    a.changed = e->d_changed; a.coef = e->d_coef; a.plane = e->d_plane; a.host_plane = e->dh_plane; a.host_stat = e->dh_stat;
    for (int k = 0; k < 64; ++k) a.nat[k] = (unsigned char)jpeg::kZigzag[k];
    hipStream_t s = e->stream;
    LP_HIP(hipMemcpyAsync(e->d_up, e->h_up, (size_t)(e->head_bytes + raw), hipMemcpyHostToDevice, s));
    LP_HIP(hipMemsetAsync(e->d_changed, 0, kRing * 4, s));
    LP_HIP(hipMemsetAsync(e->d_coef, 0, (size_t)blk * 64 * sizeof(int16_t), s));
    if (any_rst) { hipLaunchKernelGGL(k_jdec_count<true>, dim3(nd), dim3(kScanThreads), 0, s, a); hipLaunchKernelGGL(k_jdec_unstuff<true>, dim3(kStuffGrid), dim3(kThreads), 0, s, a); }
    else { hipLaunchKernelGGL(k_jdec_count<false>, dim3(nd), dim3(kScanThreads), 0, s, a); hipLaunchKernelGGL(k_jdec_unstuff<false>, dim3(kStuffGrid), dim3(kThreads), 0, s, a); }
    void (*const sync_kernel)(DecArgs, int) = any_color ? (any_rst ? k_jdec_sync<true, true> : k_jdec_sync<true, false>) : (any_rst ? k_jdec_sync<false, true> : k_jdec_sync<false, false>);
    void (*const write_kernel)(DecArgs) = any_color ? (any_rst ? k_jdec_write<true, true> : k_jdec_write<true, false>) : (any_rst ? k_jdec_write<false, true> : k_jdec_write<false, false>);
    // rounds until one changes nothing: subsequence s is final after round s, so max_sub + 1 rounds always do
    int round = 0;
    bool converged = false;
    for (int batch = kRoundsPerCheck; !converged && round <= (int)max_sub + 1; batch = std::min(2 * batch, kRing / 2)) {
        for (int b = 0; b < batch; ++b, ++round) {
            hipLaunchKernelGGL(sync_kernel, dim3(wg), dim3(kSyncThreads), 0, s, a, round);
        }
        LP_HIP(hipGetLastError());
        LP_HIP(hipMemcpyAsync(e->h_changed, e->d_changed + (round - 1) % kRing, 4, hipMemcpyDeviceToHost, s));
        LP_HIP(hipStreamSynchronize(s));
        converged = *e->h_changed == 0u;
    }
    hipLaunchKernelGGL(k_jdec_blocks, dim3(nd), dim3(kScanThreads), 0, s, a);
    hipLaunchKernelGGL(write_kernel, dim3(wg), dim3(kSyncThreads), 0, s, a);
    if (any_rst) hipLaunchKernelGGL(k_jdec_dc<true>, dim3(nd), dim3(kScanThreads), 0, s, a);
    else hipLaunchKernelGGL(k_jdec_dc<false>, dim3(nd), dim3(kScanThreads), 0, s, a);
    hipLaunchKernelGGL(k_jdec_idct, dim3(chunks), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(k_jdec_out, dim3(kCopyGrid), dim3(kThreads), 0, s, a);
    LP_HIP(hipGetLastError());
    LP_HIP(hipStreamSynchronize(s));

    for (int i = 0; i < n; ++i) {
        const Parsed& p = ps[(size_t)i];
        if (p.dev < 0) continue;
        const DecImg& im = imgs[p.dev];
        const DecStat& st = e->h_stat[p.dev];
        e->last_rounds[(size_t)i] = st.last_changed + 1; e->last_subs[(size_t)i] = (int32_t)st.nsub; e->last_blocks[(size_t)i] = (int32_t)st.blocks;
        if (!converged || st.blocks != (unsigned int)im.nblk || st.err) continue;
        // what follows the data has to be what the host decoder accepts as the end of the file: it walks on from the marker
        Parsed rest = p;
        rest.hd.decoded_luma = true;
        size_t pos = std::min((size_t)stream_sizes[i], p.scan.data + (size_t)st.marker);
        if (jpeg::walk_to_scan(streams[i], (size_t)stream_sizes[i], pos, rest.hd, rest.scan, nullptr) != jpeg::Walk::end) continue;
        const uint8_t* src = e->h_plane + im.plane0;
        for (int y = 0; y < im.h; ++y) std::memcpy(outs[i] + (long long)y * out_strides[i], src + (long long)y * 8 * im.bw, (size_t)im.w);
        status[i] = LPSLAM_HIP_JPEG_DECODED;
    }
    return LPSLAM_HIP_OK;
}

int lpslam_hip_jpeg_dec_take_restart(lpslam_hip_jpeg_dec* e, int32_t on)
{
    if (!e) { set_error("jpeg_dec_take_restart: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    std::lock_guard<std::mutex> lock(e->mutex);
    e->take_restart = on != 0;
    return LPSLAM_HIP_OK;
}

int lpslam_hip_jpeg_dec_last(lpslam_hip_jpeg_dec* e, int32_t n, int32_t* rounds, int32_t* subsequences, int32_t* blocks)
{
    if (!e || !rounds || !subsequences || !blocks || n < 1 || n > e->max_images) { set_error("jpeg_dec_last: null argument or n outside 1 .. max_images"); return LPSLAM_HIP_ERR_INVALID; }
    std::lock_guard<std::mutex> lock(e->mutex);
    for (int i = 0; i < n; ++i) { rounds[i] = e->last_rounds[(size_t)i]; subsequences[i] = e->last_subs[(size_t)i]; blocks[i] = e->last_blocks[(size_t)i]; }
    return LPSLAM_HIP_OK;
}

}  // extern "C"
