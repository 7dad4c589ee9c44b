// Wave and workgroup sums / exclusive scans shared by the JPEG encoder (jpeg.hip) and decoder (jpeg_dec.hip); included inside each
// file's unnamed namespace.
__device__ __forceinline__ int wave_sum(int x)
{
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}
__device__ __forceinline__ int wave_exclusive(int x, int lane)
{
    int s = x;
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(s, d); if (lane >= d) s += y; }
    return s - x;
}

// exclusive scan of one value per thread over the workgroup; returns the prefix, *total = the sum
__device__ unsigned int block_exclusive(unsigned int x, unsigned int* wsum, unsigned int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned int pre = (unsigned int)wave_exclusive((int)x, lane);
    if (lane == 63) wsum[wave] = pre + x;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int s = 0;
        for (int w = 0; w < nw; ++w) { const unsigned int v = wsum[w]; wsum[w] = s; s += v; }
        wsum[nw] = s;
    }
    __syncthreads();
    const unsigned int r = wsum[wave] + pre;
    *total = wsum[nw];
    __syncthreads();
    return r;
}
