// One wavefront, one 32-column panel [D; B] with 64 riding rows: cycles of each part of the register Cholesky that k_chol_pair,
// k_chol_wg and k_chol_band run, taken with s_memtime around the product's own code (csrc/chol_panel.inl is included, not copied),
// and the factor checked against a plain host Cholesky of the same block.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I lpslam_amd/csrc -I include -o panel_bench tools/dev/panel_bench.hip
// An -I in front of lpslam_amd/csrc that holds another revision's chol_panel.inl measures that revision: the two sides of
// DESIGN.md 25 are this file built twice.
// Rows:
//   parts   load | strip A | between | strip B             panel_load, strip_factor, panel_between, strip_factor
//   chol_panel_dpp                                         the panel of k_chol_pair, no stamps inside
//   chol_panel_core<48>                                    the panel of k_chol_wg behind a loader of this file's, no stamps inside
//   chol_panel_split                                       the panel of k_chol_pair that loads its right half behind strip A (nothing to
//                                                          wait for here: want = 0), no stamps inside
// A stamp waits for the LDS queue first (s_waitcnt lgkmcnt(0)), so a part owns the reads and writes it issued; the rows without
// stamps inside are the ones to compare.  Ten launches of REPS panels each: minimum / median / maximum of the launch means.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ba_common.h"
#include "chol_panel.inl"

constexpr int PB_BLK = NB * (NB + 1);
constexpr int PB_SCR = 2 * 64 * 17;
enum { PB_PARTS, PB_DPP, PB_CORE48, PB_SPLIT, PB_MODES };

// all four register sets of a panel, as k_chol_wg's own loader hands them to chol_panel_core
__device__ __forceinline__ void pb_load_all(PanelRegs& p, const double* Dblk, const double* Bblk, int lane)
{
    const int r = lane & 15;
    const double* own = lane < 16 ? Dblk + (16 + lane) * (NB + 1) : (lane < 48 ? Bblk + (lane - 16) * (NB + 1) : nullptr);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        p.dA[c] = Dblk[r * (NB + 1) + c];
        p.x[c] = own ? own[c] : 0.0;
        p.y[c] = own ? own[16 + c] : 0.0;
        p.dB[c] = Dblk[(16 + r) * (NB + 1) + 16 + c];
    }
}

__device__ __forceinline__ long long pb_stamp()
{
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const long long t = (long long)__builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

template <int MODE>
__global__ __launch_bounds__(64) void k_panel(const double* A, double* out, int reps, long long* cyc, int* failed)
{
    __shared__ double Dblk[PB_BLK], Bblk[PB_BLK], scr[PB_SCR];
    const int lane = threadIdx.x;
    for (int e = lane; e < NB * NB; e += 64) {
        const int r = e / NB, c = e % NB;
        Dblk[r * (NB + 1) + c] = A[r * NB + c];
        Bblk[r * (NB + 1) + c] = A[(NB + r) * NB + c];
    }
    __syncthreads();
    const double d00 = Dblk[0];
    long long part[4] = {0, 0, 0, 0};
    double carry = 0.0;
    bool fail = false;
    PanelRegs p;
    const long long w0 = pb_stamp();
    for (int rep = 0; rep < reps; ++rep) {
        if (lane == 0) Dblk[0] = d00 + carry;            // every panel waits for the one before it (adds nothing: carry ~ 1e-300)
        if (MODE == PB_PARTS) {
            const long long t0 = pb_stamp();
            panel_load(p, Dblk, Bblk, lane);
            const long long t1 = pb_stamp();
            fail |= strip_factor(p.dA, p.x);
            const long long t2 = pb_stamp();
            panel_between<64>(p, lane, scr);
            const long long t3 = pb_stamp();
            fail |= strip_factor(p.dB, p.y);
            const long long t4 = pb_stamp();
            part[0] += t1 - t0; part[1] += t2 - t1; part[2] += t3 - t2; part[3] += t4 - t3;
        } else {
            if (MODE == PB_DPP) fail |= chol_panel_dpp(p, Dblk, Bblk, lane, scr);
            else if (MODE == PB_SPLIT) fail |= chol_panel_split<false>(p, Dblk, Bblk, lane, scr, nullptr, 0, NB);
            else { pb_load_all(p, Dblk, Bblk, lane); fail |= chol_panel_core<48>(p, lane, scr); }
        }
        carry = p.dB[0] * 1e-300;                        // L11[r][0]: a number every lane owns (the wavefront issues in order)
    }
    const long long w1 = pb_stamp();
    // rows 0..15: L00 | 0, rows 16..31: L10 | L11 (lanes 0-15), rows 32..63: L_B (lanes 16-47)
    if (lane < 16) {
        for (int c = 0; c < 16; ++c) {
            out[lane * NB + c] = c <= lane ? p.dA[c] : 0.0;           out[lane * NB + 16 + c] = 0.0;
            out[(16 + lane) * NB + c] = p.x[c];                       out[(16 + lane) * NB + 16 + c] = c <= lane ? p.dB[c] : 0.0;
        }
    } else if (lane < 48) {
        for (int c = 0; c < 16; ++c) { out[(16 + lane) * NB + c] = p.x[c]; out[(16 + lane) * NB + 16 + c] = p.y[c]; }
    }
    if (lane == 0) {
        cyc[0] = w1 - w0;
        for (int q = 0; q < 4; ++q) cyc[1 + q] = part[q];
    }
    if (__ballot(fail) != 0 && lane == 0) *failed = 1;
}

static void launch(int mode, const double* dA, double* dO, int reps, long long* dC, int* dF)
{
    switch (mode) {
    case PB_PARTS: hipLaunchKernelGGL(k_panel<PB_PARTS>, 1, 64, 0, 0, dA, dO, reps, dC, dF); break;
    case PB_DPP: hipLaunchKernelGGL(k_panel<PB_DPP>, 1, 64, 0, 0, dA, dO, reps, dC, dF); break;
    case PB_SPLIT: hipLaunchKernelGGL(k_panel<PB_SPLIT>, 1, 64, 0, 0, dA, dO, reps, dC, dF); break;
    default: hipLaunchKernelGGL(k_panel<PB_CORE48>, 1, 64, 0, 0, dA, dO, reps, dC, dF); break;
    }
}

#define PB_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main()
{
    const int n = NB, rows = 2 * NB, reps = 200, launches = 10;
    std::vector<double> A(rows * n), L(rows * n, 0.0), G(rows * n);
    srand(1);
    for (auto& g : G) g = rand() / (double)RAND_MAX - 0.5;
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0;
            for (int k = 0; k < n; ++k) s += G[i * n + k] * G[j * n + k];
            A[i * n + j] = i < n ? s + (i == j ? 8.0 : 0.0) : G[i * n + j];          // D = G G^T + 8 I (rows 0..31), B as drawn
        }
    for (int j = 0; j < n; ++j) {                        // L = chol(D); L_B = B L^-T
        double dd = A[j * n + j];
        for (int k = 0; k < j; ++k) dd -= L[j * n + k] * L[j * n + k];
        dd = sqrt(dd);
        for (int i = j; i < rows; ++i) {
            double s = A[i * n + j];
            for (int k = 0; k < j; ++k) s -= L[i * n + k] * L[j * n + k];
            L[i * n + j] = i == j ? dd : s / dd;
        }
    }
    double *dA, *dO; long long* dC; int* dF;
    PB_CHECK(hipMalloc(&dA, 8 * rows * n)); PB_CHECK(hipMalloc(&dO, 8 * rows * n)); PB_CHECK(hipMalloc(&dC, 8 * 5)); PB_CHECK(hipMalloc(&dF, 4));
    PB_CHECK(hipMemcpy(dA, A.data(), 8 * rows * n, hipMemcpyHostToDevice));
    const char* names[PB_MODES] = {"parts", "chol_panel_dpp", "chol_panel_core<48>", "chol_panel_split"};
    int bad = 0;
    printf("cycles per panel (s_memtime), %d launches of %d panels: min / median / max\n", launches, reps);
    for (int mode = 0; mode < PB_MODES; ++mode) {
        std::vector<double> whole, parts[4];
        PB_CHECK(hipMemset(dF, 0, 4));
        for (int it = 0; it < launches + 1; ++it) {     // the first launch warms the instruction cache
            launch(mode, dA, dO, reps, dC, dF);
            PB_CHECK(hipDeviceSynchronize());
            long long c[5];
            PB_CHECK(hipMemcpy(c, dC, sizeof c, hipMemcpyDeviceToHost));
            if (it == 0) continue;
            whole.push_back((double)c[0] / reps);
            for (int q = 0; q < 4; ++q) parts[q].push_back((double)c[1 + q] / reps);
        }
        std::vector<double> O(rows * n); int f = 0;
        PB_CHECK(hipMemcpy(O.data(), dO, 8 * rows * n, hipMemcpyDeviceToHost)); PB_CHECK(hipMemcpy(&f, dF, 4, hipMemcpyDeviceToHost));
        double err = 0;
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < n; ++j) if (i >= j || i >= n) err = fmax(err, fabs(O[i * n + j] - L[i * n + j]));
        const bool ok = err < 1e-12 && !f && std::isfinite(err);       // entries are O(1): a thousand times the rounding of a 32-term sum
        bad += !ok;
        auto mmm = [](std::vector<double> v, char* buf) { std::sort(v.begin(), v.end()); sprintf(buf, "%7.0f /%7.0f /%7.0f", v.front(), v[v.size() / 2], v.back()); };
        char b[64];
        mmm(whole, b);
        printf("%-20s whole %s   max |L - host| %.2e  pivot flag %d  %s\n", names[mode], b, err, f, ok ? "ok" : "FAILED");
        if (mode == PB_PARTS) {
            const char* pn[4] = {"load", "strip A", "between", "strip B"};
            for (int q = 0; q < 4; ++q) { mmm(parts[q], b); printf("    %-10s %s\n", pn[q], b); }
        }
    }
    return bad ? 1 : 0;
}
