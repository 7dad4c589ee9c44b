// desc_wave.h -- what the descriptor kernels of match.hip, bow.hip and triangulate.hip share on the device: the 256-bit Hamming distance,
// the per-lane 2-NN update and the per-wavefront top-K of packed keys.  The tie rules the CPU oracle pins down live HERE and nowhere else:
//   keys are unique      a key is distance << 32 | what names the candidate, so no two lanes hold the same one;
//   smallest key wins    the K smallest keys of a wavefront are its K answers, whatever order the candidates were met in;
//   first strictly smaller distance   a lane that meets its candidates in index order keeps the first minimum (knn2_update).
// Arrays are taken by reference and indexed by unrolled constants, so after inlining they stay in registers.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lpslam {

constexpr unsigned long long kNoKey = ~0ull;       // an empty entry of a top-K list: above every real key

// a 32-byte descriptor into 8 registers
__device__ __forceinline__ void desc_load8(const uint8_t* p, uint32_t (&a)[8])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = reinterpret_cast<const uint32_t*>(p)[k];
}
__device__ __forceinline__ int hamming256(const uint32_t (&a)[8], const uint32_t* b)
{
    int d = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) d += __popc(a[k] ^ b[k]);
    return d;
}
// the same for descriptors held as two 16-byte halves (an LDS broadcast read gives the b side that way)
__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
// one candidate into a lane's 2-NN: the first strictly smaller distance becomes the best, second = the second smallest distance
__device__ __forceinline__ void knn2_update(int d, int idx, int& best, int& second, int& bidx)
{
    if (d < best) { second = best; best = d; bidx = idx; }
    else if (d < second) second = d;
}

// over the 64 lanes of a wavefront, every lane active
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }

// a lane's K smallest keys, ascending: the sorted insert
template <int K>
__device__ __forceinline__ void topk_insert(unsigned long long (&top)[K], unsigned long long key)
{
#pragma unroll
    for (int t = 0; t < K; ++t) if (key < top[t]) { const unsigned long long tmp = top[t]; top[t] = key; key = tmp; }
}
// The wavefront's K smallest keys out of its lanes' lists, ascending: K rounds of the minimum over the lists' heads; the one lane
// that owns a minimum (keys are unique) pops it.  emit(r, m) runs on every lane with round r's minimum (kNoKey: fewer than r + 1 keys).
template <int K, class Emit>
__device__ __forceinline__ void wave_topk_pop(unsigned long long (&top)[K], Emit emit)
{
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const unsigned long long m = wave_min_u64(top[0]);
        emit(r, m);
        if (top[0] == m && m != kNoKey) {
#pragma unroll
            for (int t = 0; t + 1 < K; ++t) top[t] = top[t + 1];
            top[K - 1] = kNoKey;
        }
    }
}
// Appends `value` of the lanes that `pass` to the wavefront's list in LDS, in lane order (ballot + prefix count); n_list is uniform
// over the wavefront, and every lane must call (the ballot wants them all).
__device__ __forceinline__ void wave_append(uint16_t* list, int& n_list, bool pass, int value)
{
    const unsigned long long b = __ballot(pass);
    if (pass) list[n_list + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u))] = (uint16_t)value;
    n_list += __popcll(b);
}

}  // namespace lpslam
#endif
