// ransac_sample.h -- what the RANSAC solvers share on the host: the sample draw, the sample tables of a batch
// and the argument rules of a batch's offsets.  Plain inline code, no HIP.  The draw is sequential by definition (one xorshift32
// state runs through all iterations of a set), so it is made on the host and the kernels read the table.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace lpslam_ransac {

// One sample of K different matches out of n >= K: avail[0 .. n) (scratch) is rebuilt, then K steps of a partial Fisher-Yates over it,
// each with the next xorshift32 number of the state s (a solver starts from seed ? seed : 1).  idx receives the K match indices.
template <int K> inline void draw(uint32_t& s, int n, int* avail, int32_t* idx)
{
    for (int i = 0; i < n; ++i) avail[i] = i;
    int left = n;
    for (int k = 0; k < K; ++k) {
        s ^= s << 13; s ^= s >> 17; s ^= s << 5;
        const int r = (int)(s % (uint32_t)left);
        idx[k] = avail[r]; avail[r] = avail[left - 1]; --left;
    }
}

// The samples a solver draws for a set of n >= K matches, K draws per iteration whether or not the iteration's solve succeeds:
// table receives iterations x K match indices.
template <int K> inline void sample_table(int n, int iterations, uint32_t seed, int32_t* table, int* avail)
{
    uint32_t s = seed ? seed : 1u;
    for (int it = 0; it < iterations; ++it) draw<K>(s, n, avail, table + (size_t)K * (size_t)it);
}

// The tables of every set of a batch (off0: n_sets + 1 offsets), each set from the same seed: n_sets x iterations x K indices, zeros
// for a set of fewer than K matches (its kernels read no sample).
template <int K> inline void batch_tables(int n_sets, const int32_t* off0, int iterations, uint32_t seed, int32_t* table)
{
    int max_n = 1;
    for (int i = 0; i < n_sets; ++i) max_n = std::max(max_n, off0[i + 1] - off0[i]);
    std::vector<int> avail((size_t)max_n);
    for (int i = 0; i < n_sets; ++i, table += (size_t)K * (size_t)iterations) {
        const int n = off0[i + 1] - off0[i];
        if (n >= K) sample_table<K>(n, iterations, seed, table, avail.data());
        else memset(table, 0, (size_t)iterations * K * sizeof(int32_t));
    }
}

// The rules every batch call holds its sets to: n_sets >= 0, offsets there, offsets[0] >= 0, offsets ascending.  nullptr: they hold,
// *first = offsets[0] and *total = the matches of all sets; otherwise the reason (the calling thread's, until its next check).
inline const char* check_offsets(int32_t n_sets, const int32_t* offsets, int* first, int* total)
{
    static thread_local char why[64];
    if (n_sets < 0) { snprintf(why, sizeof why, "%d sets", n_sets); return why; }
    if (!offsets) return "null argument";
    if (offsets[0] < 0) { snprintf(why, sizeof why, "offsets[0] = %d is negative", offsets[0]); return why; }
    for (int s = 0; s < n_sets; ++s) if (offsets[s + 1] < offsets[s]) { snprintf(why, sizeof why, "offsets do not ascend at set %d", s); return why; }
    *first = offsets[0]; *total = offsets[n_sets] - offsets[0];
    return nullptr;
}

}  // namespace lpslam_ransac
