// The panel arithmetic of the dense Cholesky chain (k_chol_pair in ba.hip, k_chol_wg in ba_solve.inl, k_chol_band in ba_band.inl):
// device code only, included by ba.hip and by tools/dev/panel_bench.hip, which times exactly this text.  Needs NB and f64x4
// (ba_common.h).
// ---- 16-column strip of a panel, rank-1 multipliers by DPP ---------------------------------------------------------------
// The diagonal block D (16 x 16) is held REPLICATED: lane l keeps row l & 15 in d[0..15], so every 16-lane DPP row owns a full
// copy, and x[0..15] is the lane's own row of whatever rides along below D (64 rows per wavefront).  The rank-1 update of column
// jj, a[c] -= l[c] * l[row], then is ONE instruction per column and register set: v_fmac_f64_dpp with row_newbcast:c fetches
// l[c] from lane c of the lane's own DPP row (the DP ALU only knows this DPP control, gfx90a+).  The readlane form it replaces
// costs three issue slots per column (two v_readlane_b32 + the fma) and keeps the multipliers in SGPRs, which spilled; on
// MI355X a strip with 64 riding rows takes 2.4k cycles against 3.4k (micro-benchmark) and 7.4k inside k_chol_pair.
// Hazard: a VALU write of the DPP source needs two wait states before the DPP read and the compiler does not look into inline
// assembly, so every block starts with s_nop 1.
#define LP_DPPF(c) "v_fmac_f64_dpp %" #c ", %16, -%17 row_newbcast:" #c " row_mask:0xf bank_mask:0xf\n\t"
#define LP_F15 LP_DPPF(15)
#define LP_F14 LP_DPPF(14) LP_F15
#define LP_F13 LP_DPPF(13) LP_F14
#define LP_F12 LP_DPPF(12) LP_F13
#define LP_F11 LP_DPPF(11) LP_F12
#define LP_F10 LP_DPPF(10) LP_F11
#define LP_F9 LP_DPPF(9) LP_F10
#define LP_F8 LP_DPPF(8) LP_F9
#define LP_F7 LP_DPPF(7) LP_F8
#define LP_F6 LP_DPPF(6) LP_F7
#define LP_F5 LP_DPPF(5) LP_F6
#define LP_F4 LP_DPPF(4) LP_F5
#define LP_F3 LP_DPPF(3) LP_F4
#define LP_F2 LP_DPPF(2) LP_F3
#define LP_F1 LP_DPPF(1) LP_F2
#define LP_ACC16(a) "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15])
// a[c] -= (src of lane c of this DPP row) * mul   for c = FROM .. 15
template <int FROM>
__device__ __forceinline__ void dpp_rank1(double (&a)[16], double src, double mul)
{
#define LP_CASE(k, S) if constexpr (FROM == k) asm("s_nop 1\n\t" S : LP_ACC16(a) : "v"(src), "v"(mul));
    LP_CASE(1, LP_F1) LP_CASE(2, LP_F2) LP_CASE(3, LP_F3) LP_CASE(4, LP_F4) LP_CASE(5, LP_F5) LP_CASE(6, LP_F6) LP_CASE(7, LP_F7) LP_CASE(8, LP_F8)
    LP_CASE(9, LP_F9) LP_CASE(10, LP_F10) LP_CASE(11, LP_F11) LP_CASE(12, LP_F12) LP_CASE(13, LP_F13) LP_CASE(14, LP_F14) LP_CASE(15, LP_F15)
#undef LP_CASE
}
template <int L>
__device__ __forceinline__ double dpp_bcast(double v)          // the value of lane L of this lane's DPP row
{
    double r;
    asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(L));
    return r;
}
// One pivot of a strip.  The strip is bound by its instruction COUNT (measured, tools/dev/strip_bench2.hip: 240 DPP updates at
// 5.5 cycles + the per-pivot instructions at 4 to 5 cycles each; placing the next pivot's root between the updates by hand changes
// nothing), so a pivot is written with as few instructions as the arithmetic allows:
//   * 1 / sqrt(d) = y0 (1 + e / 2 + 3 e^2 / 8), e = 1 - d y0^2, y0 = v_rsq_f64 (2^-24, measured): one cubic step, five operations,
//     1.4e-16 relative error over 4M samples (two Goldschmidt steps: eight operations, 2.1e-16);
//   * the positivity guard sits BEFORE the root (compare + one 64-bit select; a failed pivot continues on 1.0: harmless finite
//     numbers, the factorisation is flagged and its result discarded);
//   * the next pivot is read back from the updated column with one DPP broadcast (a recurrence a(jj+1,jj+1) - l(jj+1)^2 on values
//     broadcast beforehand shortens the dependent chain but costs four more instructions: 3.15 k against 2.84 k cycles per strip).
template <int JJ>
__device__ __forceinline__ void strip_step(double (&d)[16], double (&x)[16], double piv, bool& fail)
{
    const bool ok = piv > 0.0;
    fail |= !ok;
    const double pg = ok ? piv : 1.0;
    const double y0 = __builtin_amdgcn_rsq(pg);
    const double t = pg * y0;
    const double e = fma(-t, y0, 1.0);
    const double pp = fma(0.375, e, 0.5), ye = y0 * e;
    const double rs = fma(ye, pp, y0);
    const double l = d[JJ] * rs, lx = x[JJ] * rs;
    d[JJ] = l; x[JJ] = lx;
    if constexpr (JJ < 15) {
        dpp_rank1<JJ + 1>(d, l, l);
        const double next = dpp_bcast<JJ + 1>(d[JJ + 1]);
        dpp_rank1<JJ + 1>(x, l, lx);
        strip_step<JJ + 1>(d, x, next, fail);
    }
}
// d <- chol(D) (lower part; rows above the diagonal of a column hold values nobody reads), x <- x chol(D)^-T
__device__ __forceinline__ bool strip_factor(double (&d)[16], double (&x)[16])
{
    bool fail = false;
    strip_step<0>(d, x, dpp_bcast<0>(d[0]), fail);
    return fail;
}
// Register Cholesky of a 32-column panel [D; B] from two padded LDS blocks (B may be absent): two strips with the block product
// between them on the matrix cores (through this wavefront's scratch).  Lane l carries row l & 15 of the replicated diagonal
// block of each strip, and in x / y its own row of the stack  [D rows 16..31 (lanes 0-15); B rows 0..31 (lanes 16-47)]:
//   dA = L00, x = [L10; L_B,0], dB = L11, y = [L11; L_B,1]  (lanes 48-63 idle along with zeros)
// On entry dB holds row 16 + (l & 15) of D, columns 16 .. 31: what lanes 0-15 carry in y, in every DPP row.
#ifdef LPSLAM_PAIR_STAMPS
struct PanelRegs { double dA[16], x[16], dB[16], y[16]; unsigned long long clk[2]; };     // development: the wait of chol_panel_split
// (the clock is a scalar instruction and the strips are plain inline assembly: without the barriers it is read ahead of strip A)
#define LP_PANEL_STAMP(k) do { __builtin_amdgcn_sched_barrier(0); p.clk[k] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
struct PanelRegs { double dA[16], x[16], dB[16], y[16]; };
#define LP_PANEL_STAMP(k) do {} while (0)
#endif
// ---- the block product between the strips ----------------------------------------------------------------------------------
// y -= U, U = X (X[0..15, :])^T (K = 16, matrix cores, through this wavefront's scratch: Ls takes x one row per lane, Us the
// product), and dB, which the caller loaded with the rows of the second diagonal block that lanes 0-15 carry in y, -= U as well:
// every lane takes row l & 15 of U for it, so the updated block needs no second trip through LDS to reach every DPP row.
// ROWS: lanes that carry rows (64, or 48 where the scratch is short: 2 * ROWS * 17 doubles).
// An LDS instruction costs this single wavefront about as much as four of its FP64 instructions (measured), so the
// trip is laid out for few of them: column k of a row sits at position (k & 3) * 4 + (k >> 2).  The four K values an MFMA lane
// (lr, lk) takes from a row, k = lk + 4 j, then are neighbours, and with the operands exchanged -- the tile computed is U^T, the
// products and their order are the same, so are the bits -- a lane holds columns lk + 4 q of row lr of U: neighbours again.
// 36 LDS instructions where the plain layout takes 48 and a dB that went through y took 64.
__device__ __forceinline__ constexpr int prod_pos(int k) { return (k & 3) * 4 + (k >> 2); }
template <int ROWS>
__device__ __forceinline__ void panel_between(PanelRegs& p, int lane, double* scr)
{
    const int r = lane & 15, lk = lane >> 4;
    double* Ls = scr; double* Us = scr + ROWS * 17;
    if (ROWS == 64 || lane < ROWS) {
#pragma unroll
        for (int k = 0; k < 16; ++k) Ls[lane * 17 + prod_pos(k)] = p.x[k];
    }
    double a[3][4];                                      // X[16 t + lr][lk + 4 j]
#pragma unroll
    for (int t = 0; t < 3; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[t][j] = Ls[(16 * t + r) * 17 + lk * 4 + j];
    }
    // U[16t.., :]^T = X[0..15, :] (X[16t.., :])^T (rows 48.. are zero), one tile after the other.  The wavefront issues in order
    // and waits ~60 cycles in front of every MFMA for the one before it; LDS instructions placed there cost nothing (an MFMA holds
    // up FP64 vector instructions, not LDS ones).  So tile t leaves for Us among the MFMAs of tile t + 1, and the rows of tile 0
    // that dB takes come back among those of tiles 1 and 2; sched_barrier(0) pins the places.
#define LP_SB() __builtin_amdgcn_sched_barrier(0)
#define LP_MFMA(t, j) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][j], a[t][j], acc[t], 0, 0, 0); LP_SB()
#define LP_UOUT(t) _Pragma("unroll") for (int q = 0; q < 4; ++q) Us[(16 * t + r) * 17 + lk * 4 + q] = acc[t][q]; LP_SB()
#define LP_UD(c0) _Pragma("unroll") for (int c = c0; c < c0 + 4; ++c) ud[c] = Us[r * 17 + prod_pos(c)]; LP_SB()
    f64x4 acc[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    double ud[16];                                       // row l & 15 of U
    LP_SB();
    LP_MFMA(0, 0); LP_MFMA(0, 1); LP_MFMA(0, 2); LP_MFMA(0, 3);
    LP_MFMA(1, 0); LP_UOUT(0);
    LP_MFMA(1, 1); LP_UD(0);
    LP_MFMA(1, 2); LP_UD(4);
    LP_MFMA(1, 3); LP_UD(8);
    LP_MFMA(2, 0); LP_UD(12);
    LP_MFMA(2, 1); LP_UOUT(1);
    LP_MFMA(2, 2); LP_MFMA(2, 3);
    LP_UOUT(2);
#undef LP_UD
#undef LP_UOUT
#undef LP_MFMA
#undef LP_SB
    if (lane < 48) {
#pragma unroll
        for (int c = 0; c < 16; ++c) p.y[c] -= Us[lane * 17 + prod_pos(c)];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) p.dB[c] -= ud[c];
}
template <int ROWS>
__device__ __forceinline__ bool chol_panel_core(PanelRegs& p, int lane, double* scr)
{
    bool fail = strip_factor(p.dA, p.x);
    panel_between<ROWS>(p, lane, scr);
    fail |= strip_factor(p.dB, p.y);
    return fail;
}
__device__ __forceinline__ void panel_load(PanelRegs& p, const double* Dblk, const double* Bblk, int lane)
{
    const int r = lane & 15;
    const double* own = lane < 16 ? Dblk + (16 + lane) * (NB + 1) : (Bblk != nullptr && lane < 48 ? Bblk + (lane - 16) * (NB + 1) : nullptr);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        p.dA[c] = Dblk[r * (NB + 1) + c];
        p.x[c] = own ? own[c] : 0.0;
        p.y[c] = own ? own[16 + c] : 0.0;
        p.dB[c] = Dblk[(16 + r) * (NB + 1) + 16 + c];    // the rows lanes 0-15 carry in y, in every DPP row
    }
}
__device__ __forceinline__ bool chol_panel_dpp(PanelRegs& p, const double* Dblk, const double* Bblk, int lane, double* scr)
{
    panel_load(p, Dblk, Bblk, lane);
    return chol_panel_core<64>(p, lane, scr);
}
// ---- the LAST panel column of a system: only its first `need` = dim - 32 (nb - 1) columns are real ---------------------------
// Behind them sit the diagonal of the rhs row (1e200) and the identity padding, and nothing reads a factor column >= dim:
// k_chol_xsolve takes Minv[i][c] and y[c] for c < dim only, and the factor leaves this file through x_p alone.  Pivot c feeds the
// columns right of c and never one left of it, so stopping after `need` pivots leaves columns < need exactly as the full panel does;
// the columns from `need` on keep half-updated (finite) numbers.  strip_step_n is strip_step with a uniform branch behind every
// pivot; the common panels keep the straight-line strip.
template <int JJ>
__device__ __forceinline__ void strip_step_n(double (&d)[16], double (&x)[16], double piv, bool& fail, int need)
{
    const bool ok = piv > 0.0;
    fail |= !ok;
    const double pg = ok ? piv : 1.0;
    const double y0 = __builtin_amdgcn_rsq(pg);
    const double t = pg * y0;
    const double e = fma(-t, y0, 1.0);
    const double pp = fma(0.375, e, 0.5), ye = y0 * e;
    const double rs = fma(ye, pp, y0);
    const double l = d[JJ] * rs, lx = x[JJ] * rs;
    d[JJ] = l; x[JJ] = lx;
    if constexpr (JJ < 15) {
        if (JJ + 1 < need) {
            dpp_rank1<JJ + 1>(d, l, l);
            const double next = dpp_bcast<JJ + 1>(d[JJ + 1]);
            dpp_rank1<JJ + 1>(x, l, lx);
            strip_step_n<JJ + 1>(d, x, next, fail, need);
        }
    }
}
// the first `need` (0 .. 32) columns of the panel [D; B]
__device__ __forceinline__ bool chol_panel_trim(PanelRegs& p, const double* Dblk, const double* Bblk, int lane, double* scr, int need)
{
    panel_load(p, Dblk, Bblk, lane);
    bool fail = false;
    if (need > 0) strip_step_n<0>(p.dA, p.x, dpp_bcast<0>(p.dA[0]), fail, min(need, 16));
    if (need > 16) {
        panel_between<64>(p, lane, scr);
        strip_step_n<0>(p.dB, p.y, dpp_bcast<0>(p.dB[0]), fail, need - 16);
    } else {                                             // the second strip's columns stay as loaded
#pragma unroll
        for (int c = 0; c < 16; ++c) p.dB[c] = 0.0;
    }
    return fail;
}
// ---- a panel whose right half arrives while strip A runs (k_chol_pair) ------------------------------------------
// Strip A reads columns 0-15 of its two blocks only (dA, x); columns 16-31 (y, dB) are first needed by the block product, a load and
// a strip later.  So the panel starts on the left halves, and the wavefronts that produce the right halves announce them on a
// counter in LDS: release fence + relaxed add there, relaxed load + acquire fence here, all at workgroup scope (s_diag in k_chol_wg
// works the same way).  Every wavefront of a workgroup is resident and the announcers wait for nothing, so the wait is bounded by
// work that is already running.  The wait stands in EVERY path, also where the right half is not factored (need <= 16): whoever
// returns from here may overwrite the blocks the announcers read.
// The right half is loaded without a condition around the load (lanes that carry no row read the diagonal block and drop the
// value): a guarded load is awaited on its own, 1132 cycles for a split load against 668.  The left half keeps
// panel_load's guarded form: unconditional there as well, the kernel needs 271 registers and falls to one wavefront per SIMD.
__device__ __forceinline__ void panel_gate_open(int* gate, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_fetch_add(gate, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void panel_gate_wait(int* gate, int want)
{
    while (__hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < want) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// TRIM: the system's last panel column, `need` real columns (chol_panel_trim); otherwise the full panel (chol_panel_dpp), need unused.
// want == 0: nothing is announced (no previous pair), the gate is not read.
template <bool TRIM>
__device__ __forceinline__ bool chol_panel_split(PanelRegs& p, const double* Dblk, const double* Bblk, int lane, double* scr, int* gate, int want, int need)
{
    const int r = lane & 15;
    const bool has = lane < 16 || (Bblk != nullptr && lane < 48);
    const double* own = lane < 16 ? Dblk + (16 + lane) * (NB + 1) : (has ? Bblk + (lane - 16) * (NB + 1) : Dblk);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        p.dA[c] = Dblk[r * (NB + 1) + c];
        p.x[c] = has ? own[c] : 0.0;
    }
    bool fail = false;
    if constexpr (TRIM) { if (need > 0) strip_step_n<0>(p.dA, p.x, dpp_bcast<0>(p.dA[0]), fail, min(need, 16)); }
    else fail = strip_factor(p.dA, p.x);
    LP_PANEL_STAMP(0);
    if (want > 0) panel_gate_wait(gate, want);
    LP_PANEL_STAMP(1);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const double v = own[16 + c];
        p.y[c] = has ? v : 0.0;
        p.dB[c] = Dblk[(16 + r) * (NB + 1) + 16 + c];    // the rows lanes 0-15 carry in y, in every DPP row
    }
    if constexpr (TRIM) {
        if (need > 16) {
            panel_between<64>(p, lane, scr);
            strip_step_n<0>(p.dB, p.y, dpp_bcast<0>(p.dB[0]), fail, need - 16);
        } else {                                         // the second strip's columns stay as loaded
#pragma unroll
            for (int c = 0; c < 16; ++c) p.dB[c] = 0.0;
        }
    } else {
        panel_between<64>(p, lane, scr);
        fail |= strip_factor(p.dB, p.y);
    }
    return fail;
}
// acc += A[tr.., :] B[tc.., :]^T over one 32-wide k-block (16x16 tile, 8 x v_mfma_f64_16x16x4)
__device__ __forceinline__ f64x4 mfma_tile32(const double* A, const double* B, int tr, int tc, int lr, int lk, f64x4 acc)
{
#pragma unroll
    for (int s4 = 0; s4 < NB; s4 += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(tr + lr) * (NB + 1) + s4 + lk], B[(tc + lr) * (NB + 1) + s4 + lk], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ void tile_sub(double* D, int tr, int tc, int lr, int lk, f64x4 acc)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) D[(tr + lk + 4 * q) * (NB + 1) + tc + lr] -= acc[q];
}
