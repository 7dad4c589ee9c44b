// ba_host.inl -- host driver of the window bundle adjuster (included by ba.hip, in whose anonymous namespace the kernels live): the problem
// object, its launch chains, creation, optimize() single and batched, state exchange, the local-BA and pose-optimise flows.

struct lpslam_hip_ba {
    lpslam_hip_ctx* ctx = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr;                       // orders this problem's stream before a batch that runs on another one
    int n_poses = 0, n_points = 0, n_obs = 0, n_free = 0, dim = 0, dim_pad = 0, n_blocks = 0;
    // one block of the context's cache holds everything (carved at creation); the members below point into it
    void* block = nullptr; size_t block_cap = 0;
    BaView h_view{};                               // host copy of the device-resident view
    BaView* d_view = nullptr;
    double *d_poses[2] = {nullptr, nullptr}, *d_points[2] = {nullptr, nullptr};
    uint8_t* d_o_active = nullptr; uint8_t* d_act_in = nullptr; int* d_o_orig = nullptr;
    double* d_red = nullptr; int64_t red_n = 0;
    double* d_scal = nullptr;
    double* d_chi_obs = nullptr; uint8_t* d_depth = nullptr;
    BaCtl* d_ctl = nullptr; lpslam_hip_ba_iter_log* d_log = nullptr;
    std::vector<double> h_ur;                      // mono/stereo classification for the outlier thresholds
    BaCtl h_ctl{};                                 // last control block read back
    struct Pinned { BaCtl ctl; lpslam_hip_ba_iter_log log[MAX_LOG]; };
    Pinned* pin = nullptr;                         // page-locked: control block and iteration log come back in one round trip
    void* stage = nullptr; size_t stage_cap = 0;   // page-locked staging of the creation inputs, handed back at the first synchronisation
    // page-locked, device-mapped exchange block [poses in | points in | poses out | points out]: the small per-keyframe transfers
    // (set_state, get, control block) are done by KERNELS that read / write host memory over PCIe, not by the DMA engines -- a
    // hipMemcpyAsync of a few KB queues behind whatever the engine is busy with (the 0.9 MB image uploads of the front end:
    // +0.08 ms per keyframe, measured) and costs a packet round trip of its own even on an idle engine
    uint8_t* xfer = nullptr; size_t xfer_cap = 0;
    hipEvent_t xfer_in_read = nullptr; bool xfer_in_pending = false;      // the kernel that reads the "in" half has been enqueued
    int robust = 1, points_fixed = 0;
    int pending_iters = -1;                            // >= 0 between optimize_begin and optimize_end
    int band_hbw_structure = -1;                       // block half-bandwidth of the window when the band path can take it (creation), else -1
    int band_gmax = 0;                                 // landmarks per group at most (LDS of k_schur_group)
    int faults_band = 0, faults_update = 0;            // timed-out hand-overs seen so far (report_faults)
    bool quiesced = false;                             // everything enqueued for this problem is known to be complete (a shared batch waited for it): destroy need not wait for its stream again
    bool built = false;                                // the structure build has been enqueued (lpslam_hip_ba_build_batch); prepare alone leaves the block untouched
    int schur_fit = 0;                                 // further Schur parts that fit in one generation of k_ba_schur's workgroups (prepare), what the build chooses the part size by
    void* build_desc = nullptr;                        // BuildDesc of this problem (host copy), ba_build.inl
    size_t o_descs = 0;                                // offset of the descriptor array (device: in the block; host: in the staging block)
    hipEvent_t ev_built = nullptr;                     // a build enqueued on another problem's stream: this problem's stream waits for it
};

namespace {

// what a launch chain needs to know: the view array, how many problems it holds and the launch extents (maxima over them)
struct BaLaunch {
    const BaView* d_views = nullptr; int count = 0; hipStream_t s = nullptr; lpslam_hip_ctx* ctx = nullptr;
    int obs_blocks = 0, pose_blocks = 0, point_blocks = 0, part_n = 0, n_free = 0, n_blocks = 0, dim = 0, nb = 0, land_blocks = 0, n_poses = 0, schur_items = 0;
    int robust = 1, points_fixed = 0;
    bool any_small = false, any_large = false;          // systems for k_chol_wg / for the panel-pair chain
    bool any_band = false, any_dense = false;           // banded windows (ba_band.inl) / pair lists + dense factorisation
    int band_groups = 0, band_blocks = 0, band_gmax = 0; // extents of k_schur_group / k_schur_band_reduce, landmarks per group
    bool spread = false;                                // the context reserves CUs of every XCD for the solves: no XCD pinning
    bool any_one_pass = false, any_two_launch = false;  // problems that take k_ba_update behind the fused solve / that keep k_ba_backsub + k_ba_trial (upd_takes)
    // profiled run (lpslam_hip_ba_optimize_profiled): an event after every launch, tagged with the kernel it closes
    std::vector<std::pair<hipEvent_t, int>>* marks = nullptr;
    void mark(int kernel) const
    {
        if (!marks) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, s);
        marks->emplace_back(e, kernel);
    }
    void add(const lpslam_hip_ba* b)
    {
        const BaView& v = b->h_view;
        obs_blocks = std::max(obs_blocks, v.obs_blocks); pose_blocks = std::max(pose_blocks, v.pose_blocks);
        point_blocks = std::max(point_blocks, v.point_blocks); part_n = std::max(part_n, v.part_n); land_blocks = std::max(land_blocks, v.land_blocks);
        n_free = std::max(n_free, v.n_free); n_poses = std::max(n_poses, v.n_poses);
        if (upd_takes(v.n_points, v.n_free, v.n_poses)) any_one_pass = true; else any_two_launch = true;
        if (v.band_hbw >= 0) {
            any_band = true;
            band_groups = std::max(band_groups, v.band_groups); band_blocks = std::max(band_blocks, v.n_free * (v.band_hbw + 2));
            band_gmax = std::max(band_gmax, b->band_gmax);
        } else {
            if (v.n_free) any_dense = true;
            n_blocks = std::max(n_blocks, v.n_blocks); dim = std::max(dim, v.dim); schur_items = std::max(schur_items, v.n_poses * SPLIT + (v.extra_pack >> 12) + v.n_blocks);
            nb = std::max(nb, v.dim_pad / NB);
            if (v.dim > 0) { if (cw_fits(v.dim)) any_small = true; else any_large = true; }
        }
        ++count;
    }
};
BaLaunch single_launch(lpslam_hip_ba* b)
{
    BaLaunch L;
    L.d_views = b->d_view; L.s = b->stream; L.ctx = b->ctx; L.robust = b->robust; L.points_fixed = b->points_fixed;
    L.add(b);
    // a small reserve (<= 8 CUs of every XCD) cannot hold the pinned chain's workgroups on ONE XCD: spread them over all XCDs then (4 CUs:
    // 4256 against 4145 frames/s pinned); from 12 on the pinned chain is the better one again (12: 4392 against 4336, 16: 4428 against 4357)
    L.spread = b->ctx && b->ctx->reserve_cus > 0 && b->ctx->reserve_cus <= 8;
    return L;
}

// linearisation of the accepted state (skipped on the device when the previous trial was rejected)
int enqueue_linearize(const BaLaunch& L, int fused, bool explicit_lin = true)
{
    // fused solve: only the first unit of an optimize() call linearises here; every later state is linearised COMPLETELY beside its
    // trial (k_ba_trial: observation side with the landmark sums, pose side, combine), so later units start at the Schur complement
    if (!explicit_lin) return LPSLAM_HIP_OK;
    hipLaunchKernelGGL(k_ba_lin, dim3(L.obs_blocks + L.pose_blocks, L.count), dim3(256), 0, L.s, L.d_views, L.robust, L.points_fixed); L.mark(LPSLAM_HIP_BA_K_LIN);
    hipLaunchKernelGGL(k_ba_point_sum, dim3(L.point_blocks + 1, L.count), dim3(256), 0, L.s, L.d_views, fused);      // + the workgroup that combines the pose partials
    L.mark(LPSLAM_HIP_BA_K_POINT_SUM);
    LP_HIP(hipGetLastError());
    return LPSLAM_HIP_OK;
}

// Schur complement for the device's current lambda into the reduced buffer
int enqueue_reduce(const BaLaunch& L, int fused)
{
    if (L.any_dense) hipLaunchKernelGGL(k_ba_schur, dim3(L.schur_items, L.count), dim3(64), 0, L.s, L.d_views, fused, L.robust);
    if (L.any_band) {
        if (bd_set_attributes() != hipSuccess) return LPSLAM_HIP_ERR_DEVICE;
        // The band reduction is a launch of its own.  As trailing workgroups of the group launch it was measured and removed: the
        // groups' shares (3.1 MB per trial) then cross from workgroup to workgroup inside one launch, which on this part means
        // write-through stores and L2-bypassing loads -- 38.2 us for the one launch against 14.7 + 9.3 us for the two (MI355X, config 3).
        // a batch fills the chip with group workgroups: the variant that fits two of them on a compute unit (128 registers; the pose side
        // spills a few values there -- it is off the path) took a batch of 16 contiguous windows from 2.87 to 2.65 ms per 10 iterations; a single window keeps the
        // variant without spills (its pose-side workgroups are its longest).  Same arithmetic, same bytes.
        const dim3 sg_grid(L.n_poses + std::max(L.band_groups, 1), L.count);
        const size_t sg_lds = std::max(bd_lds_bytes(L.band_gmax), (size_t)4096);
        if (L.count >= 4) hipLaunchKernelGGL(k_schur_group<4>, sg_grid, dim3(BD_THREADS), sg_lds, L.s, L.d_views, fused, L.robust);
        else hipLaunchKernelGGL(k_schur_group<1>, sg_grid, dim3(BD_THREADS), sg_lds, L.s, L.d_views, fused, L.robust);
        L.mark(LPSLAM_HIP_BA_K_SCHUR);
        hipLaunchKernelGGL(k_schur_band_reduce, dim3(L.band_blocks, L.count), dim3(256), 0, L.s, L.d_views, fused);
        L.mark(LPSLAM_HIP_BA_K_BAND_REDUCE);
    } else if (L.any_dense) L.mark(LPSLAM_HIP_BA_K_SCHUR);
    LP_HIP(hipGetLastError());
    return LPSLAM_HIP_OK;
}

// factor + solve, update into the trial state, trial chi2 and scale terms (+ the lambda control when fused)
int enqueue_solve(const BaLaunch& L, int fused)
{
    hipStream_t s = L.s;
    if (L.any_band) {
        if (bd_set_attributes() != hipSuccess) return LPSLAM_HIP_ERR_DEVICE;
        hipLaunchKernelGGL(k_chol_band, dim3(2, L.count), dim3(BC_THREADS), BC_LDS_BYTES, s, L.d_views);      // workgroup 0: the bottom-up helper of a twisted factorisation
        if (!L.any_dense) L.mark(LPSLAM_HIP_BA_K_CHOL);
    }
    if (L.dim > 0) {
        if (!fused) {
            hipLaunchKernelGGL(k_lm_begin, dim3(1, L.count), dim3(64), 0, s, L.d_views);
            hipLaunchKernelGGL(k_chol_prep, dim3((L.nb * NB + 255) / 256, L.count), dim3(256), 0, s, L.d_views);
        }
        const bool wg = L.count >= cw_min_batch();
        if (wg && L.any_small && L.ctx) L.ctx->ba_wg_launches.fetch_add(1);
        if (L.marks && !(wg && L.any_small)) {              // profiled run through the panel-pair chain: factorisation and solve timed apart
            enqueue_cholesky(s, L.d_views, L.count, L.nb, 0, L.spread);
            L.mark(LPSLAM_HIP_BA_K_CHOL);
            enqueue_xsolve(s, L.d_views, L.count, L.dim, 0, L.spread);
            L.mark(LPSLAM_HIP_BA_K_XSOLVE);
        } else {
            lp_enqueue_factor_solve(s, L.d_views, L.count, L.nb, L.dim, wg, L.any_small, L.any_large, L.spread);
            L.mark(LPSLAM_HIP_BA_K_CHOL);
        }
    } else if (!fused) {
        hipLaunchKernelGGL(k_lm_begin, dim3(1, L.count), dim3(64), 0, s, L.d_views);
    }
    static const bool two_launch_env = [] { const char* e = getenv("LPSLAM_HIP_BA_TWO_LAUNCH_UPDATE"); return e && atoi(e) != 0; }();      // measurements: the round-4 form
    const bool one_pass = fused && !two_launch_env;
    if (one_pass && L.any_one_pass) {
        // back substitution, trial state, its chi2 and complete linearisation, the lambda control: one launch (ba_update.inl)
        hipLaunchKernelGGL(k_ba_update, dim3(L.land_blocks, L.count), dim3(256), 0, s, L.d_views, L.robust, L.points_fixed);
        L.mark(LPSLAM_HIP_BA_K_TRIAL);
        LP_HIP(hipGetLastError());
        if (!L.any_two_launch) return LPSLAM_HIP_OK;
    }
    // (the problems k_ba_update does not take -- no landmarks, no free keyframe, more keyframes than its LDS holds -- and the partitioned solve)
    hipLaunchKernelGGL(k_ba_backsub, dim3(L.part_n + 1, L.count), dim3(256), 0, s, L.d_views, one_pass ? 1 : 0);
    L.mark(LPSLAM_HIP_BA_K_BACKSUB);
    {
        // fused solve: the trial launch also linearises the trial state on speculation (observation side + pose side)
        const int spec = fused ? 1 : 0;
        hipLaunchKernelGGL(k_ba_trial, dim3(L.pose_blocks + (spec ? L.land_blocks + L.pose_blocks : 0), L.count), dim3(256), 0, s, L.d_views, L.robust, fused, L.points_fixed, spec, one_pass ? 1 : 0);
        L.mark(LPSLAM_HIP_BA_K_TRIAL);
    }
    LP_HIP(hipGetLastError());
    return LPSLAM_HIP_OK;
}

// ---- control block on the device: armed, reset and collected by kernels (one launch for any number of problems) -------------
// arms the control block for an optimize() call of `iters` outer iterations (g2o: lambda_0 is recomputed per call)
__global__ __launch_bounds__(64) void k_ba_arm(const BaView* __restrict__ views, int iters)
{
    BA_VIEW(v);
    if (threadIdx.x != 0) return;
    BaCtl c = *v.ctl;
    c.max_outer = iters; c.outer_done = 0; c.need_lin = 1; c.first = 1; c.qmax = 0; c.stopped = 0; c.ni = 2; c.rho = 0; c.last_accepted = 0;
    c.ticket = 0; c.spec = 0; c.cur_launch = c.cur;
    *v.ctl = c;
    ba_sync_words(v)[3] = 0;              // the call starts with an explicit linearisation (pose side included)
    ba_sync_words(v)[2] = 0; ba_sync_words(v)[4] = 0;      // [4]: pose-side wavefronts of the Schur launch that have stored; [2] is unused and cleared with its neighbours (one store)
}
// state given at creation back into buffer 0, every observation active, LM state cleared
__global__ __launch_bounds__(256) void k_ba_reset(const BaView* __restrict__ views)
{
    BA_VIEW(v);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 7 * v.n_poses) v.poses_buf[0][i] = v.poses0[i];
    if (i < 3 * v.n_points) v.points_buf[0][i] = v.points0[i];
    if (i < v.n_obs) v.o_active[i] = 1;
    if (i == 0) {
        BaCtl c{};
        c.ni = 2; c.need_lin = 1; c.first = 1;
        *v.ctl = c;
    }
}
// control block + iteration log of every problem of a batch into one contiguous buffer (one copy to the host)
constexpr int COLLECT_STRIDE = (int)((sizeof(BaCtl) + MAX_LOG * sizeof(lpslam_hip_ba_iter_log) + 15) / 16 * 16);
__global__ __launch_bounds__(64) void k_ba_collect(const BaView* __restrict__ views, uint8_t* out, int n_log)
{
    BA_VIEW(v);
    uint8_t* dst = out + (size_t)blockIdx.y * COLLECT_STRIDE;
    const int* src_c = reinterpret_cast<const int*>((const BaCtl*)v.ctl);
    int* dst_c = reinterpret_cast<int*>(dst);
    const int* sw = ba_sync_words(v);
    for (int i = threadIdx.x; i < (int)(sizeof(BaCtl) / 4); i += 64)
        dst_c[i] = i == (int)(offsetof(BaCtl, faults_band) / 4) ? sw[0] : (i == (int)(offsetof(BaCtl, faults_update) / 4) ? sw[1] : src_c[i]);
    const int* src_l = reinterpret_cast<const int*>((const lpslam_hip_ba_iter_log*)v.log);
    int* dst_l = reinterpret_cast<int*>(dst + sizeof(BaCtl));
    const int words = min(n_log, MAX_LOG) * (int)(sizeof(lpslam_hip_ba_iter_log) / 4);
    for (int i = threadIdx.x; i < words; i += 64) dst_l[i] = src_l[i];
}

// host (page-locked, device-mapped) -> device by load / store: 16 bytes per lane and round, grid-stride
__global__ __launch_bounds__(256) void k_copy_from_host(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
// current state -> page-locked host memory (kernel stores over PCIe: no DMA packet, no engine queue)
__global__ __launch_bounds__(256) void k_ba_state_to_host(const BaView* __restrict__ views, double* poses, double* points)
{
    BA_VIEW(v);
    const int cur = v.ctl->cur;
    // two doubles per thread: 16-byte stores (a PCIe write per 8 bytes made this kernel 14.7 us for 123 KB)
    const int i = 2 * (blockIdx.x * 256 + threadIdx.x);
    const double* sp = sel2(v.poses_buf[0], v.poses_buf[1], cur); const double* sx = sel2(v.points_buf[0], v.points_buf[1], cur);
    const int np = 7 * v.n_poses, nx = 3 * v.n_points;
    if (poses && i + 1 < np) *reinterpret_cast<f64x2*>(poses + i) = f64x2{sp[i], sp[i + 1]}; else if (poses && i < np) poses[i] = sp[i];
    if (points && i + 1 < nx) *reinterpret_cast<f64x2*>(points + i) = f64x2{sx[i], sx[i + 1]}; else if (points && i < nx) points[i] = sx[i];
}
// k_ba_reset with new creation-time values read from page-locked host memory (lpslam_hip_ba_set_state)
__global__ __launch_bounds__(256) void k_ba_reset_from_host(const BaView* __restrict__ views, const double* poses, const double* points)
{
    BA_VIEW(v);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 7 * v.n_poses) { const double x = poses ? poses[i] : v.poses0[i]; if (poses) const_cast<double*>((const double*)v.poses0)[i] = x; v.poses_buf[0][i] = x; }
    if (i < 3 * v.n_points) { const double x = points ? points[i] : v.points0[i]; if (points) const_cast<double*>((const double*)v.points0)[i] = x; v.points_buf[0][i] = x; }
    if (i < v.n_obs) v.o_active[i] = 1;
    if (i == 0) {
        BaCtl c{};
        c.ni = 2; c.need_lin = 1; c.first = 1;
        *v.ctl = c;
    }
}

// layout of the exchange block in doubles: poses in at 0, points in, then the "out" half; it and its points start on 16 bytes (f64x2 stores)
struct Xfer {
    size_t in_points, out_poses, out_points, doubles;
    explicit Xfer(const lpslam_hip_ba* b)
    {
        const size_t np = 7 * (size_t)b->n_poses, nx = 3 * (size_t)std::max(b->n_points, 1), even = ~(size_t)1;
        in_points = np; out_poses = (np + nx + 1) & even; out_points = out_poses + ((np + 1) & even); doubles = out_points + ((nx + 1) & even);
    }
};
uint8_t* ensure_xfer(lpslam_hip_ba* b)
{
    if (b->xfer) return b->xfer;
    b->xfer = (uint8_t*)lp_pin_big_alloc(b->ctx, Xfer(b).doubles * sizeof(double), &b->xfer_cap);
    if (b->xfer && hipEventCreateWithFlags(&b->xfer_in_read, hipEventDisableTiming) != hipSuccess) { lp_pin_big_free(b->ctx, b->xfer, b->xfer_cap); b->xfer = nullptr; }
    return b->xfer;
}

void release_stage(lpslam_hip_ba* b)
{
    if (b->stage) { lp_pin_big_free(b->ctx, b->stage, b->stage_cap); b->stage = nullptr; b->stage_cap = 0; }
}
// control block (and, with log_entries > 0, that many entries of the iteration log) to the host: one synchronisation
int read_ctl(lpslam_hip_ba* b, int log_entries = 0)
{
    if (b->pin) {
        // one small kernel stores the control block and the log entries straight into the page-locked block
        static_assert(offsetof(lpslam_hip_ba::Pinned, log) == sizeof(BaCtl), "k_ba_collect writes the log right behind the control block");
        hipLaunchKernelGGL(k_ba_collect, dim3(1, 1), dim3(64), 0, b->stream, b->d_view, (uint8_t*)b->pin, std::max(log_entries, 0));
        LP_HIP(hipGetLastError());
        LP_HIP(hipStreamSynchronize(b->stream));
        b->h_ctl = b->pin->ctl;
        release_stage(b);
        return LPSLAM_HIP_OK;
    }
    int sw[2] = {0, 0};
    LP_HIP(hipMemcpyAsync(&b->h_ctl, b->d_ctl, sizeof(BaCtl), hipMemcpyDeviceToHost, b->stream));
    LP_HIP(hipMemcpyAsync(sw, b->d_scal + 8, sizeof(sw), hipMemcpyDeviceToHost, b->stream));
    LP_HIP(hipStreamSynchronize(b->stream));
    b->h_ctl.faults_band = sw[0]; b->h_ctl.faults_update = sw[1];
    release_stage(b);
    return LPSLAM_HIP_OK;
}

// A hand-over between workgroups that timed out -- the two chains of the twisted band factorisation, the keyframe blocks of
// k_ba_update -- leaves a result that must not be used: the call that sees new time-outs in the collected control block fails with
// the reason.  The late chain may have left the band factorisation's flags set: they are cleared and the problem solves dense from
// here on (a stale flag would let the next launch merge blocks that are not there yet).
int report_faults(lpslam_hip_ba* b)
{
    const int nb = b->h_ctl.faults_band - b->faults_band, nu = b->h_ctl.faults_update - b->faults_update;
    if (nb <= 0 && nu <= 0) return LPSLAM_HIP_OK;
    b->faults_band = b->h_ctl.faults_band; b->faults_update = b->h_ctl.faults_update;
    if (b->ctx) { b->ctx->ba_timeouts_band.fetch_add(std::max(nb, 0)); b->ctx->ba_timeouts_update.fetch_add(std::max(nu, 0)); }
    if (nb > 0) {
        (void)hipMemsetAsync((void*)b->h_view.blk_ticket, 0, 2 * sizeof(int), b->stream);
        if (b->h_view.band_hbw >= 0) (void)lpslam_hip_ba_set_solver(b, LPSLAM_HIP_BA_SOLVER_DENSE);
    }
    set_error("bundle adjustment: %d band-factorisation and %d update hand-over(s) between workgroups timed out; this call's result is not valid", std::max(nb, 0), std::max(nu, 0));
    return LPSLAM_HIP_ERR_DEVICE;
}

// every entry point that touches a problem's device state starts here
int need_built(const lpslam_hip_ba* b)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    if (!b->built) { set_error("the problem has been prepared but not built (lpslam_hip_ba_build_batch)"); return LPSLAM_HIP_ERR_INVALID; }
    return LPSLAM_HIP_OK;
}
// a batch for the structure build (prepared, not built) or for a solve / reset (built, nothing pending)
int need_batch(lpslam_hip_ba* const* ps, int n, bool built_wanted)
{
    if (!ps || n < 1) { set_error("empty batch"); return LPSLAM_HIP_ERR_INVALID; }
    for (int i = 0; i < n; ++i) {
        const lpslam_hip_ba* b = ps[i];
        if (!built_wanted) {
            if (!b || !b->build_desc) { set_error("build_batch: entry %d is not a prepared problem", i); return LPSLAM_HIP_ERR_INVALID; }
            if (b->built) { set_error("build_batch: entry %d has been built already", i); return LPSLAM_HIP_ERR_INVALID; }
        } else if (!b) { set_error("null problem in batch (entry %d)", i); return LPSLAM_HIP_ERR_INVALID; }
        if (b->ctx->cfg.device != ps[0]->ctx->cfg.device) { set_error("batch spans devices (entry %d)", i); return LPSLAM_HIP_ERR_INVALID; }
        if (built_wanted) {
            if (b->pending_iters >= 0) { set_error("batch entry %d has an optimize_begin pending", i); return LPSLAM_HIP_ERR_INVALID; }
            if (!b->built) { set_error("batch entry %d has been prepared but not built (lpslam_hip_ba_build_batch)", i); return LPSLAM_HIP_ERR_INVALID; }
        }
        for (int k = 0; k < i; ++k) if (ps[k] == b) { set_error("problem listed twice in a batch (entries %d, %d)", k, i); return LPSLAM_HIP_ERR_INVALID; }
    }
    return LPSLAM_HIP_OK;
}
// the control block as k_ba_reset, k_ba_reset_from_host and the structure build leave it, and the extent of those launches
BaCtl fresh_ctl() { BaCtl c{}; c.ni = 2; c.need_lin = 1; c.first = 1; return c; }
long state_extent(const lpslam_hip_ba* b) { return std::max<long>(std::max<long>(7L * b->n_poses, 3L * b->n_points), b->n_obs); }
// g2o's 95 % chi-square bounds: two degrees of freedom for a monocular observation (ur < 0), three for a stereo one
double chi2_limit(double ur) { return ur < 0 ? 5.99146 : 7.81473; }
// what stays active behind a robust pass: inside its bound and, where the caller has the depth signs (local BA), in front of its keyframe
int classify_active(const lpslam_hip_ba* b, const double* chi, const uint8_t* pos, uint8_t* active)
{
    int bad = 0;
    for (int k = 0; k < b->n_obs; ++k) { active[k] = !(chi2_limit(b->h_ur[(size_t)k]) < chi[k] || (pos && !pos[k])); bad += !active[k]; }
    return bad;
}
// the local BA's verdict: switched off behind the first pass, or outside the bound / behind the keyframe after the second
void classify_outliers(const lpslam_hip_ba* b, const double* chi, const uint8_t* pos, const uint8_t* active, uint8_t* outlier)
{
    for (int k = 0; k < b->n_obs; ++k) outlier[k] = (!active[k]) || (chi2_limit(b->h_ur[(size_t)k]) < chi[k]) || !pos[k];
}

int begin_optimize(lpslam_hip_ba* b, int robust, int iters)
{
    b->robust = robust;
    hipLaunchKernelGGL(k_ba_arm, dim3(1, 1), dim3(64), 0, b->stream, b->d_view, iters);
    LP_HIP(hipGetLastError());
    return LPSLAM_HIP_OK;
}

// Behind the first batch of a call: read the control blocks (`collect`), and while a problem that has not stopped owes outer iterations --
// every rejected trial costs one more unit -- `enqueue` as many units as the one furthest behind needs and read again.
template <class Enqueue, class Collect>
int finish_trials(lpslam_hip_ba* const* ps, int n, int iters, Enqueue enqueue, Collect collect)
{
    int rc = collect();
    for (int guard = 0; !rc && iters > 0 && guard < 16 * MAX_LOG; ++guard) {
        int remaining = 0;
        for (int i = 0; i < n; ++i) if (!ps[i]->h_ctl.stopped) remaining = std::max(remaining, iters - ps[i]->h_ctl.outer_done);
        if (remaining <= 0) break;
        if (!(rc = enqueue(remaining))) rc = collect();
    }
    return rc;
}
// the end of a single problem's call: time-outs reported, the log (it came with the control block, or one blocking copy fetches it), the count
int finish_call(lpslam_hip_ba* b, lpslam_hip_ba_iter_log* log, bool log_came_with_ctl, int32_t* done_out)
{
    const int rc = report_faults(b); if (rc) return rc;
    const int done = b->h_ctl.outer_done;
    if (log && done) {
        if (log_came_with_ctl) memcpy(log, b->pin->log, (size_t)std::min(done, MAX_LOG) * sizeof(lpslam_hip_ba_iter_log));
        else LP_HIP(hipMemcpy(log, b->d_log, std::min(done, MAX_LOG) * sizeof(lpslam_hip_ba_iter_log), hipMemcpyDeviceToHost));
    }
    if (done_out) *done_out = done;
    return LPSLAM_HIP_OK;
}

// Host-side plan of the band path (ba_band.inl), made at creation from the caller's observation list.
struct BandPlan {
    int hbw = -1;                               // block half-bandwidth; -1: the window does not qualify
    std::vector<int> order, qinfo, bstart;      // landmarks with free observations by (first slot, id); (f0 << 8 | index in group); entry offsets
    std::vector<int> groups, glo, ghi;          // BD_REC ints per group; per free slot: first / last group that can touch it
    void build(const lpslam_hip_ba_obs* obs, int n_obs, int n_points, const int* slot, int n_free, int dim, const int* deg, int gmax)
    {
        if (n_free < 1 || n_obs < 1 || !bc_fits(dim)) return;
        std::vector<int> fmin((size_t)n_points, INT32_MAX), fmax((size_t)n_points, -1);
        for (int k = 0; k < n_obs; ++k) {
            const int sl = slot[obs[k].pose], j = obs[k].point;
            if (sl < 0) continue;
            fmin[j] = std::min(fmin[j], sl); fmax[j] = std::max(fmax[j], sl);
        }
        int h = 0;
        std::vector<int> first_count((size_t)n_free + 1, 0);
        for (int j = 0; j < n_points; ++j) if (fmax[j] >= 0) { h = std::max(h, fmax[j] - fmin[j]); first_count[(size_t)fmin[j] + 1]++; }
        if (h > BD_MAXHBW) return;
        for (int i = 0; i < n_free; ++i) first_count[(size_t)i + 1] += first_count[(size_t)i];
        order.resize((size_t)first_count[(size_t)n_free]);
        {
            std::vector<int> at(first_count.begin(), first_count.end() - 1);
            for (int j = 0; j < n_points; ++j) if (fmax[j] >= 0) order[(size_t)at[(size_t)fmin[j]]++] = j;      // counting sort: ties stay in landmark order
        }
        const int n_ord = (int)order.size();
        qinfo.resize((size_t)n_ord); bstart.resize((size_t)n_ord + 1);
        int e = 0;
        for (int q = 0; q < n_ord;) {
            const int f0 = fmin[order[(size_t)q]];
            int last = f0, cnt = 0, e0 = e;
            while (q + cnt < n_ord && cnt < gmax) {
                const int j = order[(size_t)(q + cnt)];
                const int l2 = std::max(last, fmax[j]);
                if (l2 - f0 + 1 > BD_MAXKF) break;
                last = l2;
                qinfo[(size_t)(q + cnt)] = (f0 << 8) | cnt; bstart[(size_t)(q + cnt)] = e;
                e += deg[j]; ++cnt;
            }
            const int rec[BD_REC] = {e0, e, f0, cnt, 6 * (last - f0 + 1), 0, 0, 0};
            groups.insert(groups.end(), rec, rec + BD_REC);
            q += cnt;
        }
        bstart[(size_t)n_ord] = e;
        // a group touches slots f0 .. f0 + rows / 6 - 1; groups are sorted by f0, so the candidates of a block (i, k), k <= i, are those
        // with f0 > i - BD_MAXKF (first: glo[i]) and f0 <= k (last: ghi[k]); the kernel tests the cover itself
        const int n_grp = (int)groups.size() / BD_REC;
        glo.assign((size_t)n_free, n_grp); ghi.assign((size_t)n_free, -1);
        for (int i = 0, g = 0; i < n_free; ++i) { while (g < n_grp && groups[(size_t)BD_REC * g + 2] <= i - BD_MAXKF) ++g; glo[(size_t)i] = g; }
        for (int i = 0, g = -1; i < n_free; ++i) { while (g + 1 < n_grp && groups[(size_t)BD_REC * (g + 1) + 2] <= i) ++g; ghi[(size_t)i] = g; }
        hbw = h;
    }
};

// wavefronts of k_ba_schur (one per workgroup) the device holds at once: what the runtime says fits on a compute unit x compute units,
// asked once per device.  No kernel and no stream operation: lpslam_hip_ba_prepare stays callable from several threads.
int schur_resident_waves(int device)
{
    static std::mutex mu;
    static std::map<int, int> known;
    std::lock_guard<std::mutex> lock(mu);
    auto it = known.find(device);
    if (it != known.end()) return it->second;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_ba_schur, 64, 0) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; cus = 0; }
    return known[device] = per_cu * cus;               // (0: nothing is known, every window keeps SCH_PART)
}

struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; }
};

}  // namespace

extern "C" {

// Creation in two halves.  lpslam_hip_ba_prepare is the HOST half: validation, the window's shape (band plan, landmark blocks), one block of
// the context's cache carved, the inputs copied into a page-locked staging block -- no kernel, no stream operation, safe to call from
// several threads at once (a server's sessions prepare their windows side by side).  lpslam_hip_ba_build_batch is the DEVICE half for
// any number of prepared problems: ~16 launches in all (blockIdx.y = problem) on the first problem's stream.  lpslam_hip_ba_create =
// prepare + build_batch of one.
int lpslam_hip_ba_prepare(lpslam_hip_ctx* ctx, const double* poses, const uint8_t* fixed, int32_t n_poses, const double* points,
                          int32_t n_points, const lpslam_hip_ba_obs* obs, int32_t n_obs, const lpslam_hip_ba_camera* cam,
                          lpslam_hip_ba** out)
{
    if (!ctx || !poses || !points || !obs || !cam || !out || n_poses < 1 || n_points < 0 || n_obs < 0) {
        set_error("invalid bundle-adjustment arguments"); return LPSLAM_HIP_ERR_INVALID;
    }
    *out = nullptr;
    // range check + landmark degrees (bound of the pair lists: every ordered pair of observations of a landmark)
    std::vector<int> deg((size_t)std::max(n_points, 1), 0);
    for (int k = 0; k < n_obs; ++k) {
        if (obs[k].pose < 0 || obs[k].pose >= n_poses || obs[k].point < 0 || obs[k].point >= n_points) {
            set_error("observation %d references pose %d / point %d out of range", k, obs[k].pose, obs[k].point);
            return LPSLAM_HIP_ERR_INVALID;
        }
        deg[obs[k].point]++;
    }
    size_t terms_cap = 0;
    for (int j = 0; j < n_points; ++j) { terms_cap += (size_t)deg[j] * deg[j]; if (deg[j] > 0xFFFF) { set_error("landmark %d has more than 65535 observations", j); return LPSLAM_HIP_ERR_INVALID; } }
    LP_HIP(hipSetDevice(ctx->cfg.device));
    lpslam_hip_ba* b = new lpslam_hip_ba();
    b->ctx = ctx;
    static_assert(sizeof(lpslam_hip_ba::Pinned) <= 8192, "pinned block size");
    b->pin = static_cast<lpslam_hip_ba::Pinned*>(lp_pin_alloc(ctx));      // nullptr: the pageable path stays
    // own stream (from the context's cache): a bundle adjustment runs beside the front end of later frames
    b->stream = lp_stream_acquire(ctx);
    if (!b->stream) { lpslam_hip_ba_destroy(b); set_error("hipStreamCreate failed"); return LPSLAM_HIP_ERR_DEVICE; }
    b->n_poses = n_poses; b->n_points = n_points; b->n_obs = n_obs;
    std::vector<int> slot(n_poses), free_pose;
    for (int i = 0; i < n_poses; ++i) { if (fixed && fixed[i]) slot[i] = -1; else { slot[i] = (int)free_pose.size(); free_pose.push_back(i); } }
    b->n_free = (int)free_pose.size();
    b->dim = 6 * b->n_free;
    b->dim_pad = ((b->dim + 1 + NB - 1) / NB) * NB;           // room for the rhs row
    b->n_blocks = b->n_free * (b->n_free + 1) / 2;
    b->h_ur.resize((size_t)n_obs);
    std::vector<int> kf_obs((size_t)n_poses, 0);
    for (int k = 0; k < n_obs; ++k) { b->h_ur[k] = obs[k].ur; ++kf_obs[(size_t)obs[k].pose]; }   // caller order (host-side outlier thresholds)

    // ---- shape of the window (ba_band.inl): first / last FREE keyframe slot of every landmark.  When no landmark spans more than
    //      BD_MAXHBW slots the reduced system is block-banded and the problem takes the band path: landmarks ordered by their first
    //      slot, cut into groups of <= band_gmax whose observations fall into <= BD_MAXKF neighbouring keyframes.
    BandPlan plan;
    {
        static const int solver_env = [] { const char* e = getenv("LPSLAM_HIP_BA_SOLVER"); return !e ? 0 : (!strcmp(e, "dense") ? 1 : 0); }();
        static const int group_env = [] { const char* e = getenv("LPSLAM_HIP_BA_GROUP"); const int g = e ? atoi(e) : 0; return g >= 4 && g <= BD_GMAX ? g : 32; }();
        if (solver_env != 1) plan.build(obs, n_obs, n_points, slot.data(), b->n_free, b->dim, deg.data(), group_env);
        if (plan.hbw >= 0 && bd_set_attributes() != hipSuccess) { lpslam_hip_ba_destroy(b); return LPSLAM_HIP_ERR_DEVICE; }      // (the reason is in lpslam_hip_last_error)
        b->band_hbw_structure = plan.hbw;
        b->band_gmax = plan.hbw >= 0 ? group_env : 0;
        static const bool trace = getenv("LPSLAM_HIP_BA_TRACE") != nullptr;
        if (trace) fprintf(stderr, "[lpslam_hip_ba_create] %d poses (%d free) %d points %d obs: block half-bandwidth %d, %zu groups -> %s\n", n_poses, b->n_free, n_points,
                           n_obs, plan.hbw, plan.groups.size() / BD_REC, plan.hbw >= 0 ? "band" : "dense");
    }

    // ---- landmark blocks of the landmark-major passes (k_ba_update, land_lin_body): consecutive landmarks, at most LAND_B of them and --
    //      unless a single landmark has more -- at most 256 CSR entries, so that a block's entries are one per thread
    std::vector<int> land_start;
    {
        int cnt = 0, ent = 0, first_entry = 0;
        land_start.push_back(0); land_start.push_back(0);
        for (int j = 0; j < n_points; ++j) {
            if (cnt == LAND_B || (cnt > 0 && ent + deg[j] > 256)) { first_entry += ent; land_start.push_back(j); land_start.push_back(first_entry); cnt = 0; ent = 0; }
            ++cnt; ent += deg[j];
        }
        if (n_points > 0) { land_start.push_back(n_points); land_start.push_back(first_entry + ent); }
    }
    const int land_blocks = (int)land_start.size() / 2 - 1;

    // ---- k_ba_schur's further parts (ba_build.inl).  The part size is chosen on the device, where the pair counts are; the host gives
    //      it the room: extra_fit = the wavefronts of k_ba_schur the device holds at once - the leading pose-side workgroups
    //      - part 0 of every block, so that a launch stays ONE generation of workgroups (a negative figure: no room, the window keeps
    //      SCH_PART).  The table -- and the launch -- must hold that many items and what SCH_PART gives: a list of n > part terms has at
    //      most n / part further parts and at most the part limit - 1.  What the host can foresee for the stretch in front of the pairs
    //      are the diagonal blocks' parts (one term per observation of the keyframe) at the smallest part size + some slack.
    int extra_cap = 0, extra_first = 0, extra_fit = 0;
    {
        const size_t cap_wide = std::min<size_t>((SCH_MAXP_WIDE - 1) * (size_t)b->n_blocks, terms_cap / SCH_PART);
        const size_t cap_fine = std::min<size_t>((SCH_MAXP - 1) * (size_t)b->n_blocks, terms_cap / SCH_PART_MIN);
        const long room = (long)schur_resident_waves(ctx->cfg.device) - (long)n_poses * SPLIT - (long)b->n_blocks;
        extra_fit = (int)std::min<size_t>(std::min<size_t>((size_t)std::max(room, 0L), cap_fine), (size_t)1 << 18);
#ifdef LPSLAM_SCHUR_FORCE_PART
        extra_cap = (int)std::min<size_t>(std::max(cap_wide, cap_fine), (size_t)1 << 18);
#else
        extra_cap = (int)std::min<size_t>(std::max(cap_wide, (size_t)extra_fit), (size_t)1 << 18);
#endif
        for (int i = 0; i < b->n_free; ++i) extra_first += schur_parts(kf_obs[(size_t)free_pose[(size_t)i]], SCH_PART_MIN) - 1;
        extra_first = std::min(std::min(extra_first + 32, extra_cap), 4095);
    }
    b->schur_fit = extra_fit;
    // ---- one block: [view | inputs as staged | zero-initialised part | the rest]
    const size_t np = (size_t)n_poses, npt = (size_t)std::max(n_points, 1), no = (size_t)std::max(n_obs, 1), n = (size_t)b->dim_pad;
    const size_t nblk = (size_t)std::max(b->n_blocks, 1), nfree = (size_t)std::max(b->n_free, 1);
    b->red_n = (int64_t)(n * n + 3 * n + 8);
    const int part_n = std::max((n_points + 63) / 64, 1);
    Carve cv;
    const size_t o_view = cv.take(sizeof(BaView));
    const size_t o_poses0 = cv.take(7 * np * 8), o_points0 = cv.take(3 * npt * 8), o_slot = cv.take(np * 4), o_free = cv.take(nfree * 4);
    const size_t o_obs_in = cv.take(no * sizeof(lpslam_hip_ba_obs));
    const size_t n_ord = plan.order.size(), n_grp = plan.groups.size() / BD_REC;
    const size_t o_land_start = cv.take(land_start.size() * 4);
    const size_t o_blk_perm = cv.take(nblk * 4);
    const size_t o_band_tab = cv.take((BD_REC * n_grp + 2 * nfree) * 4), o_band_order = cv.take(n_ord * 4), o_band_qinfo = cv.take(n_ord * 4), o_band_bstart = cv.take((n_ord + 1) * 4);
    const size_t staged_bytes = cv.off;                 // what the copy kernel moves: [0, staged_bytes)
    const size_t o_descs = cv.take(BUILD_MAX_BATCH * sizeof(BuildDesc));      // descriptors of a batched build led by this problem (device: here; host: same offset of the staging block)
    const size_t stage_alloc = cv.off;
    const size_t z_begin = cv.off;
    const size_t o_A = cv.take(np * npt * 4), o_ptcount = cv.take(npt * 4);
    const SetOff so = set_offsets(n_poses, n_points, n_obs, b->n_free, b->dim_pad);
    const size_t o_setz0 = cv.take(so.z_total * 8), o_setz1 = cv.take(so.z_total * 8);
    const size_t o_red = cv.take((size_t)b->red_n * 8), o_minv = cv.take(std::max(n * n, 64 * n) * 8) /* L^-T rows, or the band path's M blocks: 1024 doubles per 16 columns */, o_xp = cv.take(n * 8);
    const size_t o_scal = cv.take(16 * 8) /* 8 scalars + the fault words (ba_update.inl) */, o_ctl = cv.take(sizeof(BaCtl)), o_ticket = cv.take((nblk + 2 + (size_t)extra_cap) * 4) /* tickets | count | items (+ one word: a workgroup reads an item slot before it looks at the count) */, o_log = cv.take(MAX_LOG * sizeof(lpslam_hip_ba_iter_log));
    const size_t z_end = cv.off;
    const size_t o_R = cv.take(np * npt * 4), o_pscount = cv.take(np * 4), o_slotof = cv.take(no * 4);
    const size_t o_ps_start = cv.take((np + 1) * 4), o_pt_start = cv.take((npt + 1) * 4), o_pt_obs = cv.take(no * 4), o_orig = cv.take(no * 4);
    const size_t o_opose = cv.take(no * 4), o_opoint = cv.take(no * 4), o_u = cv.take(no * 8), o_v = cv.take(no * 8), o_ur = cv.take(no * 8), o_w = cv.take(no * 8);
    const size_t o_active = cv.take(no), o_actin = cv.take(no);
    const size_t o_poses_a = cv.take(7 * np * 8), o_poses_b = cv.take(7 * np * 8), o_points_a = cv.take(3 * npt * 8), o_points_b = cv.take(3 * npt * 8);
    const size_t o_setd0 = cv.take(so.d_total * 8), o_setd1 = cv.take(so.d_total * 8), o_ptrial = cv.take(np * SPLIT * 8);
    const size_t cst = csr_stride(n_obs), o_csr = cv.take(6 * cst * 8);          // u, v, ur, w (doubles) + pose, point (ints) + pose slot (int)
    const size_t o_ldiag = cv.take(n * NB * 8), o_lsub = cv.take(n * NB * 8), o_chipose = cv.take(np * 8), o_part = cv.take((size_t)std::max(part_n, 2 * std::max(land_blocks, 1)) * 8) /* k_ba_backsub: part_n; k_ba_update: scale term and chi2 per landmark block */;
    const size_t o_chiobs = cv.take(no * 8), o_depth = cv.take(no);
    const size_t o_blk_count = cv.take(nblk * 4), o_blk_start = cv.take((nblk + 1) * 4), o_blk_part = cv.take(nblk * SCH_MAXP * SCH_PV * 8);
    const size_t o_terms = cv.take(std::max<size_t>(terms_cap, 1) * sizeof(int4));
    const size_t o_band_ent = cv.take(plan.hbw >= 0 ? no * sizeof(int4) : 0), o_band_part = cv.take((n_grp + 1) * BD_PART * 8) /* + the exchange block of the twisted band factorisation */;
    {
        const int rc = lp_pool_alloc(ctx, cv.off, &b->block, &b->block_cap);
        if (rc) { lpslam_hip_ba_destroy(b); return rc; }
    }
    uint8_t* base = (uint8_t*)b->block;
    auto fail = [&](int code) { lpslam_hip_ba_destroy(b); return code; };
#define BA_HIP(x) do { if ((x) != hipSuccess) { set_error("HIP call failed: %s", #x); return fail(LPSLAM_HIP_ERR_DEVICE); } } while (0)
    // ---- the view
    BaView& v = b->h_view;
    v = BaView{};
    v.n_poses = n_poses; v.n_points = n_points; v.n_obs = n_obs; v.n_free = b->n_free; v.dim = b->dim; v.dim_pad = b->dim_pad;
    v.obs_blocks = (n_obs + 255) / 256; v.pose_blocks = (n_poses * SPLIT + 3) / 4; v.point_blocks = (n_points + 255) / 256; v.part_n = part_n;
    v.n_blocks = b->n_blocks; v.land_blocks = land_blocks;
    v.extra_pack = (extra_cap << 12) | extra_first;
    vset(v.land_start, (const int*)(base + o_land_start));
    b->d_poses[0] = (double*)(base + o_poses_a); b->d_poses[1] = (double*)(base + o_poses_b);
    b->d_points[0] = (double*)(base + o_points_a); b->d_points[1] = (double*)(base + o_points_b);
    for (int s2 = 0; s2 < 2; ++s2) { vset(v.poses_buf[s2], b->d_poses[s2]); vset(v.points_buf[s2], b->d_points[s2]); }
    vset(v.poses0, (const double*)(base + o_poses0)); vset(v.points0, (const double*)(base + o_points0));
    vset(v.pose_slot, (const int*)(base + o_slot)); vset(v.free_pose, (const int*)(base + o_free));
    vset(v.o_pose, (const int*)(base + o_opose)); vset(v.o_point, (const int*)(base + o_opoint));
    vset(v.o_u, (const double*)(base + o_u)); vset(v.o_v, (const double*)(base + o_v)); vset(v.o_ur, (const double*)(base + o_ur)); vset(v.o_w, (const double*)(base + o_w));
    b->d_o_active = base + o_active; b->d_act_in = base + o_actin; b->d_o_orig = (int*)(base + o_orig);
    vset(v.o_active, b->d_o_active);
    vset(v.pt_start, (const int*)(base + o_pt_start)); vset(v.pt_obs, (const int*)(base + o_pt_obs)); vset(v.ps_start, (const int*)(base + o_ps_start));
    vset(v.o_orig, (const int*)b->d_o_orig);
    vset(v.set_z[0], (double*)(base + o_setz0)); vset(v.set_z[1], (double*)(base + o_setz1));
    vset(v.set_d[0], (double*)(base + o_setd0)); vset(v.set_d[1], (double*)(base + o_setd1));
    vset(v.csr, (const double*)(base + o_csr));
    {   // the selected set's pointers (kernels set them with ba_lin_set before use): set 0
        double* z = (double*)(base + o_setz0); double* d = (double*)(base + o_setd0);
        vset(v.partial, z); vset(v.bp_loc, z + so.loc); vset(v.hppdiag_loc, z + so.loc + n); vset(v.chi_loc, z + so.loc + 2 * n);
        vset(v.Hll, d); vset(v.bl, d + so.bl); vset(v.Hpp, d + so.Hpp); vset(v.W, d + so.W); vset(v.hl_obs, d + so.hl);
    }
    vset(v.partial_trial, (double*)(base + o_ptrial));
    b->d_red = (double*)(base + o_red);
    vset(v.S, b->d_red); vset(v.rhs, b->d_red + n * n); vset(v.bp, b->d_red + n * n + n); vset(v.hppdiag, b->d_red + n * n + 2 * n); vset(v.chi_cur, b->d_red + n * n + 3 * n);
    vset(v.Minv, (double*)(base + o_minv)); vset(v.Ldiag, (double*)(base + o_ldiag)); vset(v.Lsub, (double*)(base + o_lsub));
    b->d_scal = (double*)(base + o_scal);
    vset(v.xp, (double*)(base + o_xp)); vset(v.chi_pose, (double*)(base + o_chipose)); vset(v.part, (double*)(base + o_part)); vset(v.scal, b->d_scal);
    vset(v.blk_start, (const int*)(base + o_blk_start)); vset(v.blk_terms, (const int4*)(base + o_terms));
    vset(v.blk_part, (double*)(base + o_blk_part)); vset(v.blk_ticket, (int*)(base + o_ticket));
    vset(v.blk_perm, (const int*)(base + o_blk_perm));
    b->d_ctl = (BaCtl*)(base + o_ctl); b->d_log = (lpslam_hip_ba_iter_log*)(base + o_log);
    vset(v.ctl, b->d_ctl); vset(v.log, b->d_log);
    v.cam = BaCam{cam->fx, cam->fy, cam->cx, cam->cy, cam->focal_x_baseline, cam->huber_mono, cam->huber_stereo};
    v.band_hbw = plan.hbw; v.band_groups = (int)n_grp; v.band_groups_cap = (int)n_grp;
    vset(v.band_tab, (const int*)(base + o_band_tab)); vset(v.band_ent, (const int*)(base + o_band_ent)); vset(v.band_part, (double*)(base + o_band_part));
    b->d_view = (BaView*)(base + o_view);
    b->d_chi_obs = (double*)(base + o_chiobs); b->d_depth = base + o_depth;
    // ---- inputs through one page-locked staging block, one copy
    b->stage = lp_pin_big_alloc(ctx, stage_alloc, &b->stage_cap);
    if (!b->stage) { set_error("page-locked staging of %zu bytes failed", stage_alloc); return fail(LPSLAM_HIP_ERR_DEVICE); }
    b->o_descs = o_descs;
    uint8_t* hs = (uint8_t*)b->stage;
    memcpy(hs + o_view, &v, sizeof(BaView));
    memcpy(hs + o_poses0, poses, 7 * np * 8);
    if (n_points) memcpy(hs + o_points0, points, 3 * (size_t)n_points * 8);
    memcpy(hs + o_slot, slot.data(), np * 4);
    if (b->n_free) memcpy(hs + o_free, free_pose.data(), (size_t)b->n_free * 4);
    if (n_obs) memcpy(hs + o_obs_in, obs, (size_t)n_obs * sizeof(lpslam_hip_ba_obs));
    memcpy(hs + o_land_start, land_start.data(), land_start.size() * 4);
    {
        // k_ba_schur's work item w (part 0 of a pose-block pair) runs on XCD (lead + extra_first + w) mod 8 -- workgroups go round the XCDs -- and every
        // XCD has an L2 of its own: with the pairs in row-major order each L2 fetched all of W (50.7 MB per launch for 5.76 MB of W,
        // profiles/r05c_pmc.json).  The free keyframes are cut into four groups and the ten group pairs dealt to the eight XCDs (six
        // off-diagonal tiles one each, the four diagonal tiles two to an XCD): an XCD's pairs then touch the W blocks of two groups, half
        // of the window.  Any assignment is valid (every pair is taken once); batched launches place problems, not pairs, on XCDs.
        std::vector<int> perm((size_t)nblk, 0);
        const int N = b->n_free, nb_ = b->n_blocks;
        if (nb_ > 0) {
            std::vector<std::vector<int>> of_xcd(8);
            auto grp = [N](int i) { return std::min(3, i * 4 / std::max(N, 1)); };
            static const int tile_xcd[4][4] = {{6, 0, 1, 2}, {0, 6, 3, 4}, {1, 3, 7, 5}, {2, 4, 5, 7}};
            int blk = 0;
            // (every XCD's diagonal blocks first: theirs are the longest lists -- a term per observation -- and their epilogue waits for the pose side)
            for (int pass = 0; pass < 2; ++pass) {
                blk = 0;
                for (int i = 0; i < N; ++i) for (int k = i; k < N; ++k, ++blk) if ((i == k) == (pass == 0)) of_xcd[N >= 16 ? (size_t)tile_xcd[grp(i)][grp(k)] : (size_t)(blk & 7)].push_back(blk);
            }
            const int lead = n_poses * SPLIT;
            std::vector<size_t> at(8, 0);
            for (int w = 0; w < nb_; ++w) {
                size_t x = (size_t)((lead + extra_first + w) & 7);
                if (at[x] >= of_xcd[x].size()) { size_t best = 0, left = 0; for (size_t y = 0; y < 8; ++y) if (of_xcd[y].size() - at[y] > left) { left = of_xcd[y].size() - at[y]; best = y; } x = best; }      // its own tile is used up: from the fullest
                perm[(size_t)w] = of_xcd[x][at[x]++];
            }
        }
        memcpy(hs + o_blk_perm, perm.data(), nblk * 4);
    }
    if (plan.hbw >= 0) {
        memcpy(hs + o_band_tab, plan.groups.data(), plan.groups.size() * 4);
        memcpy(hs + o_band_tab + BD_REC * n_grp * 4, plan.glo.data(), plan.glo.size() * 4);
        memcpy(hs + o_band_tab + (BD_REC * n_grp + nfree) * 4, plan.ghi.data(), plan.ghi.size() * 4);
        memcpy(hs + o_band_order, plan.order.data(), n_ord * 4); memcpy(hs + o_band_qinfo, plan.qinfo.data(), n_ord * 4);
        memcpy(hs + o_band_bstart, plan.bstart.data(), (n_ord + 1) * 4);
    }
    // ---- what the device half will need (ba_build.inl)
    {
        BuildDesc* d = new BuildDesc();
        b->build_desc = d;
        d->n_poses = n_poses; d->n_points = n_points; d->n_obs = n_obs; d->n_free = b->n_free; d->n_blocks = b->n_blocks; d->dim = b->dim; d->dim_pad = b->dim_pad;
        d->n_ord = plan.hbw >= 0 ? (int)n_ord : 0;
        d->extra_cap = extra_cap; d->extra_fit = extra_fit;
        d->obs = (const lpslam_hip_ba_obs*)(base + o_obs_in);
        d->A = (int*)(base + o_A); d->R = (int*)(base + o_R); d->pt_count = (int*)(base + o_ptcount); d->ps_count = (int*)(base + o_pscount);
        d->ps_start = (int*)(base + o_ps_start); d->pt_start = (int*)(base + o_pt_start); d->slot_of = (int*)(base + o_slotof); d->pt_obs = (int*)(base + o_pt_obs);
        d->o_orig = b->d_o_orig; d->o_pose = (int*)(base + o_opose); d->o_point = (int*)(base + o_opoint);
        d->o_u = (double*)(base + o_u); d->o_v = (double*)(base + o_v); d->o_ur = (double*)(base + o_ur); d->o_w = (double*)(base + o_w);
        d->o_active = b->d_o_active; d->act_in = b->d_act_in;
        d->pose_slot = (const int*)(base + o_slot); d->free_pose = (const int*)(base + o_free);
        d->c_pose = (int*)(base + o_csr + 4 * cst * 8); d->c_point = d->c_pose + cst; d->c_slot = (int*)(base + o_csr + 5 * cst * 8);
        d->c_u = (double*)(base + o_csr); d->c_v = d->c_u + cst; d->c_ur = d->c_u + 2 * cst; d->c_w = d->c_u + 3 * cst;
        d->blk_count = (int*)(base + o_blk_count); d->blk_start = (int*)(base + o_blk_start); d->blk_ticket = (int*)(base + o_ticket); d->blk_terms = (int4*)(base + o_terms);
        d->band_order = (const int*)(base + o_band_order); d->band_qinfo = (const int*)(base + o_band_qinfo); d->band_bstart = (const int*)(base + o_band_bstart);
        d->band_ent = (int4*)(base + o_band_ent);
        d->S = b->d_red;
        d->copy_dst = (uint4*)base; d->copy_src = (const uint4*)hs; d->copy_n16 = (staged_bytes + 15) / 16;
        d->zero_dst = (uint4*)(base + z_begin); d->zero_n16 = (z_end - z_begin + 15) / 16;      // (carved in multiples of 256 bytes)
        d->view = b->d_view;
    }
#undef BA_HIP
    b->h_ctl = fresh_ctl();
    *out = b;
    return LPSLAM_HIP_OK;
}

// The device half of creation for n prepared problems: the structure phase (= g2o buildStructure of every window) as ONE launch chain,
// blockIdx.y = problem, on the first problem's stream; the other problems' streams wait for it on the device.  Asynchronous.
int lpslam_hip_ba_build_batch(lpslam_hip_ba* const* ps, int32_t n)
{
    const int rc = need_batch(ps, n, false); if (rc) return rc;
    LP_HIP(hipSetDevice(ps[0]->ctx->cfg.device));
    for (int c0 = 0; c0 < n; c0 += BUILD_MAX_BATCH) {
        const int m = std::min(n - c0, (int)BUILD_MAX_BATCH);
        lpslam_hip_ba* lead = ps[c0];
        hipStream_t s = lead->stream;
        BuildDesc* h_descs = (BuildDesc*)((uint8_t*)lead->stage + lead->o_descs);
        const BuildDesc* d_descs = (const BuildDesc*)((uint8_t*)lead->block + lead->o_descs);
        int mx_obs = 0, mx_poses = 0, mx_points = 0, mx_blocks = 0, mx_ord = 0, mx_pad = 0;
        size_t mx_copy = 0, mx_zero = 0;
        bool any_band = false;
        for (int i = 0; i < m; ++i) {
            const BuildDesc& d = *(const BuildDesc*)ps[c0 + i]->build_desc;
            h_descs[i] = d;
            mx_obs = std::max(mx_obs, d.n_obs); mx_poses = std::max(mx_poses, d.n_poses); mx_points = std::max(mx_points, d.n_points);
            mx_blocks = std::max(mx_blocks, d.n_blocks); mx_ord = std::max(mx_ord, d.n_ord); mx_pad = std::max(mx_pad, d.dim_pad - d.dim - 1);
            mx_copy = std::max(mx_copy, d.copy_n16); mx_zero = std::max(mx_zero, d.zero_n16);
            any_band = any_band || d.n_ord > 0;
        }
        const dim3 B256(256), BS(BS_THREADS);
        auto blocks = [](long x) { return (unsigned)std::max<long>((x + 255) / 256, 1); };
        hipLaunchKernelGGL(k_bs_descs_in, dim3(1), B256, 0, s, (uint4*)d_descs, (const uint4*)h_descs, (int)(((size_t)m * sizeof(BuildDesc) + 15) / 16));
        hipLaunchKernelGGL(k_bs_copy_in, dim3(std::min<unsigned>(64, blocks((long)mx_copy)), m), B256, 0, s, d_descs);
        hipLaunchKernelGGL(k_bs_zero, dim3(std::min<unsigned>(256, blocks((long)mx_zero)), m), B256, 0, s, d_descs);
        hipLaunchKernelGGL(k_bs_count, dim3(blocks(std::max(mx_obs, mx_pad)), m), B256, 0, s, d_descs);
        hipLaunchKernelGGL(k_bs_rowscan, dim3(mx_poses, m), BS, 0, s, d_descs);
        hipLaunchKernelGGL(k_bs_starts, dim3(2, m), BS, 0, s, d_descs);
        if (mx_obs) {
            hipLaunchKernelGGL(k_bs_scatter, dim3(blocks(mx_obs), m), B256, 0, s, d_descs);
            hipLaunchKernelGGL(k_bs_gather, dim3(blocks(mx_obs), m), B256, 0, s, d_descs);
            hipLaunchKernelGGL(k_bs_ptfill, dim3(blocks(4L * mx_points), m), B256, 0, s, d_descs);      // four lanes per landmark
            hipLaunchKernelGGL(k_bs_csrcopy, dim3(blocks(mx_obs), m), B256, 0, s, d_descs);
        }
        hipLaunchKernelGGL(k_bs_paircount, dim3((unsigned)std::max((mx_blocks + 3) / 4, 1), m), B256, 0, s, d_descs);
        hipLaunchKernelGGL(k_bs_blkscan, dim3(1, m), BS, 0, s, d_descs);
        if (mx_blocks) hipLaunchKernelGGL(k_bs_pairfill, dim3((unsigned)((mx_blocks + 3) / 4), m), B256, 0, s, d_descs);
        if (any_band && mx_ord) hipLaunchKernelGGL(k_bs_band_entries, dim3(blocks(mx_ord), m), B256, 0, s, d_descs);
        hipLaunchKernelGGL(k_bs_reset, dim3(blocks(std::max<long>(std::max<long>(7L * mx_poses, 3L * mx_points), mx_obs)), m), B256, 0, s, d_descs);
        LP_HIP(hipGetLastError());
        for (int i = 0; i < m; ++i) ps[c0 + i]->built = true;
        if (m > 1) {
            // the other problems' own streams (their solves, reads and set_state calls) are ordered behind the build on the device
            if (!lead->ev_built) LP_HIP(hipEventCreateWithFlags(&lead->ev_built, hipEventDisableTiming));
            LP_HIP(hipEventRecord(lead->ev_built, s));
            for (int i = 1; i < m; ++i) if (ps[c0 + i]->stream != s) LP_HIP(hipStreamWaitEvent(ps[c0 + i]->stream, lead->ev_built, 0));
        }
    }
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_create(lpslam_hip_ctx* ctx, const double* poses, const uint8_t* fixed, int32_t n_poses, const double* points,
                         int32_t n_points, const lpslam_hip_ba_obs* obs, int32_t n_obs, const lpslam_hip_ba_camera* cam,
                         lpslam_hip_ba** out)
{
    int rc = lpslam_hip_ba_prepare(ctx, poses, fixed, n_poses, points, n_points, obs, n_obs, cam, out);
    if (rc) return rc;
    if ((rc = lpslam_hip_ba_build_batch(out, 1))) { lpslam_hip_ba_destroy(*out); *out = nullptr; }
    return rc;
}

void lpslam_hip_ba_destroy(lpslam_hip_ba* b)
{
    if (!b) return;
    if (b->stream && !b->quiesced) (void)hipStreamSynchronize(b->stream);
    if (b->block) lp_pool_free(b->ctx, b->block, b->block_cap);
    release_stage(b);
    if (b->pin) lp_pin_free(b->ctx, b->pin);
    if (b->xfer) lp_pin_big_free(b->ctx, b->xfer, b->xfer_cap);
    if (b->xfer_in_read) (void)hipEventDestroy(b->xfer_in_read);
    if (b->ev) (void)hipEventDestroy(b->ev);
    if (b->ev_built) (void)hipEventDestroy(b->ev_built);
    if (b->stream) lp_stream_release(b->ctx, b->stream);
    delete (BuildDesc*)b->build_desc;
    delete b;
}

// caller-order activity flags -> storage order
__global__ __launch_bounds__(256) void k_ba_gather_active(const uint8_t* in, const int* o_orig, uint8_t* out, int n)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = in[o_orig[k]];
}

// the two passes between the solves of a local BA, enqueued without a wait (a batch waits once for all): activity flags in caller order (nullptr: all active)
static int enqueue_active(lpslam_hip_ba* b, const uint8_t* active)
{
    if (!b->n_obs) return LPSLAM_HIP_OK;
    if (active) {
        LP_HIP(hipMemcpyAsync(b->d_act_in, active, b->n_obs, hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(k_ba_gather_active, dim3((b->n_obs + 255) / 256), dim3(256), 0, b->stream, b->d_act_in, b->d_o_orig, b->d_o_active, b->n_obs);
        LP_HIP(hipGetLastError());
    } else LP_HIP(hipMemsetAsync(b->d_o_active, 1, b->n_obs, b->stream));
    return LPSLAM_HIP_OK;
}
// chi2 and depth sign of every observation at the current state, in caller order (either may be nullptr)
static int enqueue_chi2(lpslam_hip_ba* b, double* chi2, uint8_t* depth_positive)
{
    if (!b->n_obs) return LPSLAM_HIP_OK;
    hipLaunchKernelGGL(k_ba_obs_chi2, dim3((b->n_obs + 255) / 256, 1), dim3(256), 0, b->stream, b->d_view, b->d_chi_obs, b->d_depth);
    LP_HIP(hipGetLastError());
    if (chi2) LP_HIP(hipMemcpyAsync(chi2, b->d_chi_obs, (size_t)b->n_obs * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (depth_positive) LP_HIP(hipMemcpyAsync(depth_positive, b->d_depth, (size_t)b->n_obs, hipMemcpyDeviceToHost, b->stream));
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_set_active(lpslam_hip_ba* b, const uint8_t* active)
{
    int rc = need_built(b); if (rc) return rc;
    if (!b->n_obs) return LPSLAM_HIP_OK;              // nothing enqueued: no wait either
    if ((rc = enqueue_active(b, active))) return rc;
    LP_HIP(hipStreamSynchronize(b->stream));
    release_stage(b);
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_chi2(lpslam_hip_ba* b, double* chi2, uint8_t* depth_positive)
{
    int rc = need_built(b); if (rc) return rc;
    if (!b->n_obs) return LPSLAM_HIP_OK;
    if ((rc = enqueue_chi2(b, chi2, depth_positive))) return rc;
    LP_HIP(hipStreamSynchronize(b->stream));
    release_stage(b);
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_set_points_fixed(lpslam_hip_ba* b, int32_t points_fixed)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    b->points_fixed = points_fixed ? 1 : 0;
    return LPSLAM_HIP_OK;
}

// One unit = one LM trial.  Without rejected steps `iters` units finish the call with a single look at the control block;
// every rejected trial costs one more unit, enqueued after that look.
static const hipGraphExec_t kGraphFailed = (hipGraphExec_t)(uintptr_t)1;      // cache sentinel: capture / instantiate failed for this signature
// Graph replay is OFF in a process that runs under a rocprofiler-sdk tool (rocprofv3, rocprof-compute).  A replay rings the doorbell once
// for its ~125 AQL packets; with a tool attached the HSA runtime routes every queue through its InterceptQueue, which hands the tool's
// packet interceptor (pointer into the ring, packet count) WITHOUT splitting a batch that wraps the end of the 1 MB ring, and the tool
// reads the packets as a linear array: the first replay that straddles the ring's end (after ~16 k packets on the queue) faults in the
// tool's packet loop (gpurun_out/tm2.log of round 5, resolved in DESIGN.md 13.1).  One packet per doorbell -- a direct launch -- never
// wraps.  LPSLAM_HIP_BA_GRAPH=1 forces replay (to profile it on short runs), =0 switches it off anywhere.
static bool ba_graphs_enabled()
{
    static const bool on = [] {
        if (const char* e = getenv("LPSLAM_HIP_BA_GRAPH")) return atoi(e) != 0;
        const char* tool = getenv("ROCP_TOOL_LIBRARIES"); const char* pre = getenv("LD_PRELOAD");
        return !((tool && *tool) || (pre && strstr(pre, "rocprofiler-sdk")));
    }();
    return on;
}
// capture + instantiate happen once per (stream, signature): serialised over the whole process, so that two mapping threads (two managers)
// never build graphs at the same time -- the replay itself, the hot path, takes no lock
static std::mutex g_ba_capture_mutex;
static int enqueue_batch(const BaLaunch& L, int units, bool first_batch)
{
    for (int u = 0; u < units; ++u) {
        int rc;
        if ((rc = enqueue_linearize(L, 1, first_batch && u == 0))) return rc;
        if ((rc = enqueue_reduce(L, 1))) return rc;
        if ((rc = enqueue_solve(L, 1))) return rc;
    }
    return LPSLAM_HIP_OK;
}

// The first batch of a call -- the arming of the control block and `iters` units, the first with its explicit linearisation --
// has a fixed launch sequence for a given (launch extents, robust, iters, points_fixed).  The second time a stream of this context
// sees a signature the sequence is captured into a hipGraph whose kernels read their view from the STREAM's slot, and from then
// on every problem with that signature on that stream -- the same window solved again, or the next keyframe's new window --
// copies its view into the slot and replays the graph with one hipGraphLaunch.  Extents are rounded up (surplus workgroups
// exit on the view's own extents, as in a batch), so windows of slightly different size share a graph.
// Returns the executable to replay with the stream's slot in *slot_out, or nullptr: the caller launches directly.
static hipGraphExec_t first_batch_graph(lpslam_hip_ba* b, int iters, void** slot_out)
{
    BaLaunch L = single_launch(b);
    auto up = [](int x, int m) { return (x + m - 1) / m * m; };
    L.obs_blocks = up(L.obs_blocks, 8); L.pose_blocks = up(L.pose_blocks, 4); L.point_blocks = up(L.point_blocks, 4); L.part_n = up(L.part_n, 8); L.land_blocks = up(L.land_blocks, 8);
    L.band_groups = up(L.band_groups, 8); L.band_blocks = up(L.band_blocks, 8); L.schur_items = up(L.schur_items, 128);
    const std::array<int, 24> sig = {L.schur_items, iters, b->robust ? 1 : 0, b->points_fixed ? 1 : 0, L.obs_blocks, L.pose_blocks, L.point_blocks, L.part_n, L.n_free,
                                     L.n_blocks, L.dim, L.nb, L.any_small ? 1 : 0, L.any_large ? 1 : 0, L.land_blocks, L.spread ? 1 : 0,
                                     L.any_band ? 1 : 0, L.any_dense ? 1 : 0, L.band_groups, L.band_blocks, L.band_gmax, L.any_one_pass ? 1 : 0, L.any_two_launch ? 1 : 0, L.n_poses};
    lpslam_hip_ctx* c = b->ctx;
    hipGraphExec_t exec = nullptr;
    void* slot = nullptr;
    bool capture = false;
    if (ba_graphs_enabled() && b->stream != c->role_solve) {      // (several sessions' windows run on the solves' role stream: no capture on a stream other threads launch on)
        std::lock_guard<std::mutex> lock(c->pool_mutex);
        auto key = std::make_pair(b->stream, sig);
        auto it = c->ba_graphs.find(key);
        if (it == c->ba_graphs.end()) { if (c->ba_graphs.size() < 256) c->ba_graphs.emplace(key, nullptr); }   // seen once: run directly (also sets function attributes); the cache is bounded, never evicted (an entry may be in flight on its stream)
        else { exec = it->second; capture = exec == nullptr; if (exec == kGraphFailed) exec = nullptr; }      // a signature whose capture failed once runs direct from then on
        auto sl = c->ba_view_slot.find(b->stream);
        if (sl != c->ba_view_slot.end()) slot = sl->second;
    }
    if ((exec || capture) && !slot) {
        if (hipMalloc(&slot, sizeof(BaView)) == hipSuccess) { std::lock_guard<std::mutex> lock(c->pool_mutex); c->ba_view_slot[b->stream] = slot; }
        else { slot = nullptr; (void)hipGetLastError(); }
    }
    if (capture && slot) {
        std::lock_guard<std::mutex> capture_lock(g_ba_capture_mutex);
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            L.d_views = (const BaView*)slot;
            hipLaunchKernelGGL(k_ba_arm, dim3(1, 1), dim3(64), 0, b->stream, (const BaView*)slot, iters);
            int r2 = enqueue_batch(L, iters, true);
            const hipError_t e2 = hipStreamEndCapture(b->stream, &graph);
            if (r2 == LPSLAM_HIP_OK && e2 == hipSuccess && graph) {
                if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                    std::lock_guard<std::mutex> lock(c->pool_mutex);
                    c->ba_graphs[std::make_pair(b->stream, sig)] = exec;
                    c->ba_graphs_built.fetch_add(1);
                } else exec = nullptr;
            }
            if (graph) (void)hipGraphDestroy(graph);
        }
        if (!exec) { std::lock_guard<std::mutex> lock(c->pool_mutex); c->ba_graphs[std::make_pair(b->stream, sig)] = kGraphFailed; }
        (void)hipGetLastError();
    }
    *slot_out = slot;
    return slot ? exec : nullptr;
}

// optimize() in two halves: begin enqueues the whole first batch on the problem's stream and returns (the mapping side of the
// reference runs beside tracking: the caller can enqueue front-end work of the next frames meanwhile), end waits, handles
// rejected trials and fetches the log.
int lpslam_hip_ba_optimize_begin(lpslam_hip_ba* b, int32_t robust, int32_t iters)
{
    int rc = need_built(b); if (rc) return rc;
    if (iters < 0 || iters > MAX_LOG) { set_error("iterations must be in [0,%d]", MAX_LOG); return LPSLAM_HIP_ERR_INVALID; }
    if (b->pending_iters >= 0) { set_error("optimize_begin: the previous optimize_begin has not been ended"); return LPSLAM_HIP_ERR_INVALID; }
    LP_HIP(hipSetDevice(b->ctx->cfg.device));
    b->robust = robust;
    void* slot = nullptr;
    if (hipGraphExec_t exec = iters > 0 ? first_batch_graph(b, iters, &slot) : nullptr) {
        LP_HIP(hipMemcpyAsync(slot, b->d_view, sizeof(BaView), hipMemcpyDeviceToDevice, b->stream));
        LP_HIP(hipGraphLaunch(exec, b->stream));
        b->ctx->ba_graph_replays.fetch_add(1);
    } else {
        if ((rc = begin_optimize(b, robust, iters))) return rc;
        if (iters > 0 && (rc = enqueue_batch(single_launch(b), iters, true))) return rc;
    }
    b->pending_iters = iters;
    return LPSLAM_HIP_OK;
}

int64_t lpslam_hip_ba_graph_replays(lpslam_hip_ctx* c) { return c ? (int64_t)c->ba_graph_replays.load() : 0; }
int lpslam_hip_ba_counters(lpslam_hip_ctx* c, int64_t* out, int32_t n)
{
    if (!c || !out || n < 0) { set_error("null argument"); return LPSLAM_HIP_ERR_INVALID; }
    int64_t v[LPSLAM_HIP_BA_COUNTERS] = {0};
    {
        std::lock_guard<std::mutex> lock(c->pool_mutex);
        v[LPSLAM_HIP_BA_COUNTER_SIGNATURES] = (int64_t)c->ba_graphs.size();
    }
    v[LPSLAM_HIP_BA_COUNTER_GRAPHS] = (int64_t)c->ba_graphs_built.load();
    v[LPSLAM_HIP_BA_COUNTER_REPLAYS] = (int64_t)c->ba_graph_replays.load();
    v[LPSLAM_HIP_BA_COUNTER_TIMEOUTS_BAND] = (int64_t)c->ba_timeouts_band.load();
    v[LPSLAM_HIP_BA_COUNTER_TIMEOUTS_UPDATE] = (int64_t)c->ba_timeouts_update.load();
    for (int i = 0; i < n && i < LPSLAM_HIP_BA_COUNTERS; ++i) out[i] = v[i];
    return LPSLAM_HIP_OK;
}
int64_t lpslam_hip_ba_wg_factorisations(lpslam_hip_ctx* c) { return c ? (int64_t)c->ba_wg_launches.load() : 0; }

int lpslam_hip_ba_optimize_end(lpslam_hip_ba* b, lpslam_hip_ba_iter_log* log, int32_t* done_out)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    if (b->pending_iters < 0) { set_error("optimize_end without optimize_begin"); return LPSLAM_HIP_ERR_INVALID; }
    LP_HIP(hipSetDevice(b->ctx->cfg.device));
    const int iters = b->pending_iters;
    b->pending_iters = -1;
    const int want_log = (log && b->pin) ? iters : 0;
    const int rc = finish_trials(&b, 1, iters, [&](int units) { return enqueue_batch(single_launch(b), units, false); }, [&] { return read_ctl(b, want_log); });
    return rc ? rc : finish_call(b, log, want_log > 0, done_out);
}

int lpslam_hip_ba_optimize(lpslam_hip_ba* b, int32_t robust, int32_t iters, lpslam_hip_ba_iter_log* log, int32_t* done_out)
{
    const int rc = lpslam_hip_ba_optimize_begin(b, robust, iters);
    return rc ? rc : lpslam_hip_ba_optimize_end(b, log, done_out);
}

// optimize() with a HIP event after every launch: where the time of the chain goes, kernel by kernel, measured in place on the
// problem's stream (bench.py's roofline of the dominant kernel).  No graph replay; the events serialise nothing the chain does
// not serialise itself (every launch depends on its predecessor).
int lpslam_hip_ba_optimize_profiled(lpslam_hip_ba* b, int32_t robust, int32_t iters, lpslam_hip_ba_kernel_times* out)
{
    int rc = b ? need_built(b) : LPSLAM_HIP_OK; if (rc) return rc;
    if (!b || !out) { set_error("null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (iters < 0 || iters > MAX_LOG) { set_error("iterations must be in [0,%d]", MAX_LOG); return LPSLAM_HIP_ERR_INVALID; }
    if (b->pending_iters >= 0) { set_error("optimize_begin pending"); return LPSLAM_HIP_ERR_INVALID; }
    LP_HIP(hipSetDevice(b->ctx->cfg.device));
    memset(out, 0, sizeof(*out));
    std::vector<std::pair<hipEvent_t, int>> marks;
    BaLaunch L = single_launch(b);
    L.robust = robust; b->robust = robust;
    L.marks = &marks;
    rc = begin_optimize(b, robust, iters);
    L.mark(-1);                                            // start of the chain
    if (!rc && iters > 0) rc = enqueue_batch(L, iters, true);
    if (!rc) rc = finish_trials(&b, 1, iters, [&](int units) { L.mark(-1); return enqueue_batch(L, units, false); }, [&] { return read_ctl(b); });
    for (size_t i = 1; i < marks.size() && !rc; ++i) {
        const int k = marks[i].second;
        if (k < 0 || k >= LPSLAM_HIP_BA_KERNELS) continue;
        float ms = 0;
        if (hipEventElapsedTime(&ms, marks[i - 1].first, marks[i].first) == hipSuccess) { out->ms[k] += ms; out->launches[k] += 1; }
    }
    for (auto& m : marks) (void)hipEventDestroy(m.first);
    out->iterations = b->h_ctl.outer_done;
    // launches of the factorisation per mark: the panel-pair chain is several launches behind one mark
    out->launches_per_mark[LPSLAM_HIP_BA_K_CHOL] = b->h_view.band_hbw >= 0 ? 1 : (b->dim_pad / NB + 1) / 2;
    for (int k = 0; k < LPSLAM_HIP_BA_KERNELS; ++k) if (k != LPSLAM_HIP_BA_K_CHOL) out->launches_per_mark[k] = 1;
    out->dim = b->dim;
    return rc;
}

// ---- batched solve: B independent problems, ONE launch chain (blockIdx.y = problem) ------------------------------------------
// What a host that serves several SLAM sessions (or several windows of one map) on one GPU calls: every kernel of the chain is
// launched once for the whole batch with the launch extents of its largest problem, each problem follows its own control block
// (a problem that has finished, or terminated, idles through the remaining launches), and the control blocks and logs of all
// problems come back in one copy.  The single-problem chain is latency bound; a batch fills the chip.
static int batch_sync_streams(lpslam_hip_ba* const* ps, int n, hipStream_t s)
{
    for (int i = 0; i < n; ++i) {
        if (ps[i]->stream == s) continue;
        if (!ps[i]->ev) LP_HIP(hipEventCreateWithFlags(&ps[i]->ev, hipEventDisableTiming));
        LP_HIP(hipEventRecord(ps[i]->ev, ps[i]->stream));
        LP_HIP(hipStreamWaitEvent(s, ps[i]->ev, 0));
    }
    return LPSLAM_HIP_OK;
}
// device array of the problems' views (a block of the first problem's context) + its launch extents
struct BatchViews {
    lpslam_hip_ctx* ctx = nullptr; void* blk = nullptr; size_t cap = 0; void* hst = nullptr; size_t hcap = 0;
    BaLaunch L;
    ~BatchViews() { if (blk) lp_pool_free(ctx, blk, cap); if (hst) lp_pin_big_free(ctx, hst, hcap); }
};
static int batch_views(lpslam_hip_ba* const* ps, int n, size_t extra_bytes, BatchViews* bv)
{
    bv->ctx = ps[0]->ctx;
    const size_t view_bytes = (size_t)n * sizeof(BaView), total = ((view_bytes + 255) & ~(size_t)255) + extra_bytes;
    int rc = lp_pool_alloc(bv->ctx, total, &bv->blk, &bv->cap); if (rc) return rc;
    bv->hst = lp_pin_big_alloc(bv->ctx, total, &bv->hcap);
    if (!bv->hst) { set_error("page-locked staging of %zu bytes failed", total); return LPSLAM_HIP_ERR_DEVICE; }
    BaLaunch& L = bv->L;
    L.d_views = (const BaView*)bv->blk; L.s = ps[0]->stream; L.ctx = bv->ctx;
    for (int i = 0; i < n; ++i) { memcpy((uint8_t*)bv->hst + (size_t)i * sizeof(BaView), &ps[i]->h_view, sizeof(BaView)); L.add(ps[i]); }
    LP_HIP(hipMemcpyAsync(bv->blk, bv->hst, view_bytes, hipMemcpyHostToDevice, L.s));
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_reset_batch(lpslam_hip_ba* const* ps, int32_t n)
{
    int rc = need_batch(ps, n, true); if (rc) return rc;
    LP_HIP(hipSetDevice(ps[0]->ctx->cfg.device));
    BatchViews bv;
    if ((rc = batch_sync_streams(ps, n, ps[0]->stream))) return rc;
    if ((rc = batch_views(ps, n, 0, &bv))) return rc;
    long n_max = 1;
    for (int i = 0; i < n; ++i) { n_max = std::max(n_max, state_extent(ps[i])); ps[i]->h_ctl = fresh_ctl(); }
    hipLaunchKernelGGL(k_ba_reset, dim3((unsigned)((n_max + 255) / 256), n), dim3(256), 0, bv.L.s, bv.L.d_views);
    LP_HIP(hipGetLastError());
    LP_HIP(hipStreamSynchronize(bv.L.s));          // the view array is released on return
    for (int i = 0; i < n; ++i) release_stage(ps[i]);
    return LPSLAM_HIP_OK;
}

// Test entry into the factor-and-solve: the caller's systems A x = b through the launches a solve of these problems takes
// (tests/test_ba_solve_gpu.py, tests/test_ba_band_solve_gpu.py; no product path calls it).  Every problem's reduced buffer is written as
// the product leaves it in front of its solve -- A (it stands for S + lambda I, nothing is added) in the dim_pad layout, b in rhs and in
// row `dim`, 1e200 on that row's diagonal, identity padding, pivot flag cleared -- the control blocks are armed so that no kernel idles.
// Dense problems: lp_enqueue_factor_solve gets what enqueue_solve computes for the batch (wg, any_small / any_large, nb, dim, spread).
// Band problems (band_hbw >= 0): what the fused reduction leaves in front of k_chol_band, the two hand-over words of the twisted form
// cleared, then k_chol_band as enqueue_solve launches it.  A must be zero below the diagonal further than 6 band_hbw + 5 from it (the
// product zeroes that region in set_solver and the kernel reads 79 columns left of the diagonal whatever band_hbw says); the strict
// upper triangle is copied as given and never read.  The hand-over words must be back at zero behind the solve: LPSLAM_HIP_ERR_DEVICE
// otherwise.  A batch may mix both kinds: both launch families run, each kernel skips the other's views.
// It overwrites the reduced system and the control block: lpslam_hip_ba_reset (or reset_batch) the problems before they optimise again.
int lpslam_hip_ba_debug_solve(lpslam_hip_ba* const* ps, int32_t n, const double* const* A, const double* const* rhs, double* const* x, int32_t* pivot_flag)
{
    int rc = need_batch(ps, n, true); if (rc) return rc;
    if (!A || !rhs || !x) { set_error("debug_solve: null matrix / right-hand side / solution array"); return LPSLAM_HIP_ERR_INVALID; }
    for (int i = 0; i < n; ++i) {
        if (!A[i] || !rhs[i] || !x[i]) { set_error("debug_solve: null matrix / right-hand side / solution (entry %d)", i); return LPSLAM_HIP_ERR_INVALID; }
        if (ps[i]->dim < 1) { set_error("debug_solve: entry %d has no free keyframe", i); return LPSLAM_HIP_ERR_INVALID; }
        if (ps[i]->h_view.band_hbw >= 0) {
            const long dim = ps[i]->dim, w = 6L * ps[i]->h_view.band_hbw + 5;
            for (long r = w + 1; r < dim; ++r)
                for (long c = 0; c < r - w; ++c)
                    if (!(A[i][r * dim + c] == 0.0)) { set_error("debug_solve: entry %d is a band problem of scalar half-bandwidth %ld, A(%ld, %ld) is not zero", i, w, r, c); return LPSLAM_HIP_ERR_INVALID; }
        }
    }
    LP_HIP(hipSetDevice(ps[0]->ctx->cfg.device));
    BatchViews bv;
    BaLaunch L;
    if (n == 1) L = single_launch(ps[0]);
    else {
        if ((rc = batch_sync_streams(ps, n, ps[0]->stream))) return rc;
        if ((rc = batch_views(ps, n, 0, &bv))) return rc;
        L = bv.L;
    }
    std::vector<std::vector<double>> stage((size_t)n);
    std::vector<double> flags((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) {
        const lpslam_hip_ba* b = ps[i];
        const size_t np = (size_t)b->dim_pad, dim = (size_t)b->dim;
        std::vector<double>& h = stage[i];
        h.assign(np * np + np, 0.0);                                    // S | rhs
        for (size_t r = 0; r < dim; ++r) {
            memcpy(&h[r * np], A[i] + r * dim, dim * sizeof(double));
            h[dim * np + r] = rhs[i][r];
            h[np * np + r] = rhs[i][r];
        }
        h[dim * np + dim] = 1e200;
        for (size_t r = dim + 1; r < np; ++r) h[r * np + r] = 1.0;
        LP_HIP(hipMemcpyAsync(b->d_red, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, L.s));
        LP_HIP(hipMemsetAsync(b->d_scal + 5, 0, sizeof(double), L.s));
        if (b->h_view.band_hbw >= 0) LP_HIP(hipMemsetAsync((void*)b->h_view.blk_ticket, 0, 2 * sizeof(int), L.s));
    }
    hipLaunchKernelGGL(k_ba_arm, dim3(1, n), dim3(64), 0, L.s, L.d_views, 1);
    if (L.any_band) {
        if (bd_set_attributes() != hipSuccess) return LPSLAM_HIP_ERR_DEVICE;
        hipLaunchKernelGGL(k_chol_band, dim3(2, L.count), dim3(BC_THREADS), BC_LDS_BYTES, L.s, L.d_views);
    }
    if (L.dim > 0) {
        const bool wg = L.count >= cw_min_batch();
        if (wg && L.any_small && L.ctx) L.ctx->ba_wg_launches.fetch_add(1);
        lp_enqueue_factor_solve(L.s, L.d_views, L.count, L.nb, L.dim, wg, L.any_small, L.any_large, L.spread);
    }
    LP_HIP(hipGetLastError());
    std::vector<int> handover(2 * (size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        LP_HIP(hipMemcpyAsync(x[i], (const double*)ps[i]->h_view.xp, (size_t)ps[i]->dim * sizeof(double), hipMemcpyDeviceToHost, L.s));
        LP_HIP(hipMemcpyAsync(&flags[i], ps[i]->d_scal + 5, sizeof(double), hipMemcpyDeviceToHost, L.s));
        if (ps[i]->h_view.band_hbw >= 0) LP_HIP(hipMemcpyAsync(&handover[2 * (size_t)i], (const void*)ps[i]->h_view.blk_ticket, 2 * sizeof(int), hipMemcpyDeviceToHost, L.s));
    }
    LP_HIP(hipStreamSynchronize(L.s));          // the staging blocks and the view array are released on return
    for (int i = 0; i < n; ++i) { release_stage(ps[i]); if (pivot_flag) pivot_flag[i] = flags[i] != 0.0 ? 1 : 0; }
    for (int i = 0; i < n; ++i)
        if (handover[2 * (size_t)i] || handover[2 * (size_t)i + 1]) { set_error("debug_solve: entry %d: k_chol_band left its hand-over words at %d, %d", i, handover[2 * (size_t)i], handover[2 * (size_t)i + 1]); return LPSLAM_HIP_ERR_DEVICE; }
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_optimize_batch(lpslam_hip_ba* const* ps, int32_t n, int32_t robust, int32_t iters, lpslam_hip_ba_iter_log* logs,
                                 int32_t log_stride, int32_t* done)
{
    int rc = need_batch(ps, n, true); if (rc) return rc;
    if (iters < 0 || iters > MAX_LOG) { set_error("iterations must be in [0,%d]", MAX_LOG); return LPSLAM_HIP_ERR_INVALID; }
    if (logs && log_stride < iters) { set_error("log_stride %d is smaller than the iteration count %d", log_stride, iters); return LPSLAM_HIP_ERR_INVALID; }
    for (int i = 1; i < n; ++i)
        if (ps[i]->points_fixed != ps[0]->points_fixed) { set_error("batch mixes motion-only and full problems (entry %d)", i); return LPSLAM_HIP_ERR_INVALID; }
    LP_HIP(hipSetDevice(ps[0]->ctx->cfg.device));
    BatchViews bv;
    const size_t collect_bytes = (size_t)n * COLLECT_STRIDE;
    if ((rc = batch_sync_streams(ps, n, ps[0]->stream))) return rc;
    if ((rc = batch_views(ps, n, collect_bytes, &bv))) return rc;
    BaLaunch& L = bv.L;
    L.robust = robust; L.points_fixed = ps[0]->points_fixed;
    for (int i = 0; i < n; ++i) ps[i]->robust = robust;
    const size_t coll_off = ((size_t)n * sizeof(BaView) + 255) & ~(size_t)255;
    uint8_t* d_coll = (uint8_t*)bv.blk + coll_off;
    uint8_t* h_coll = (uint8_t*)bv.hst + coll_off;
    hipLaunchKernelGGL(k_ba_arm, dim3(1, n), dim3(64), 0, L.s, L.d_views, iters);
    auto collect = [&]() -> int {
        hipLaunchKernelGGL(k_ba_collect, dim3(1, n), dim3(64), 0, L.s, L.d_views, d_coll, iters);
        LP_HIP(hipGetLastError());
        LP_HIP(hipMemcpyAsync(h_coll, d_coll, collect_bytes, hipMemcpyDeviceToHost, L.s));
        LP_HIP(hipStreamSynchronize(L.s));
        for (int i = 0; i < n; ++i) memcpy(&ps[i]->h_ctl, h_coll + (size_t)i * COLLECT_STRIDE, sizeof(BaCtl));
        return LPSLAM_HIP_OK;
    };
    if (iters > 0 && (rc = enqueue_batch(L, iters, true))) return rc;
    if ((rc = finish_trials(ps, n, iters, [&](int units) { return enqueue_batch(L, units, false); }, collect))) return rc;
    for (int i = 0; i < n; ++i) if ((rc = report_faults(ps[i]))) { for (int k = 0; k < n; ++k) release_stage(ps[k]); return rc; }
    for (int i = 0; i < n; ++i) {
        release_stage(ps[i]);
        const int d = ps[i]->h_ctl.outer_done;
        if (done) done[i] = d;
        if (logs && d) memcpy(logs + (size_t)i * log_stride, h_coll + (size_t)i * COLLECT_STRIDE + sizeof(BaCtl), (size_t)std::min(d, MAX_LOG) * sizeof(lpslam_hip_ba_iter_log));
    }
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_timeouts(lpslam_hip_ba* b, int32_t* band, int32_t* update)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    if (band) *band = b->faults_band;
    if (update) *update = b->faults_update;
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_get_solver(lpslam_hip_ba* b, int32_t* solver, int32_t* block_half_bandwidth)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    if (solver) *solver = b->h_view.band_hbw >= 0 ? LPSLAM_HIP_BA_SOLVER_BAND : LPSLAM_HIP_BA_SOLVER_DENSE;
    if (block_half_bandwidth) *block_half_bandwidth = b->band_hbw_structure;
    return LPSLAM_HIP_OK;
}

// the part size k_ba_schur cuts this window's pair lists by (chosen by the build, read back from the table's head word: waits for
// the problem's stream) and the room the choice was made for
int lpslam_hip_ba_get_schur_part(lpslam_hip_ba* b, int32_t* part, int32_t* capacity)
{
    { const int nb = need_built(b); if (nb) return nb; }
    if (capacity) *capacity = b->schur_fit;
    if (part) {
        int head = 0;
        LP_HIP(hipSetDevice(b->ctx->cfg.device));
        LP_HIP(hipStreamSynchronize(b->stream));
        LP_HIP(hipMemcpy(&head, b->h_view.blk_ticket + b->n_blocks, sizeof(int), hipMemcpyDeviceToHost));
        *part = schur_head_part(head);
    }
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_set_solver(lpslam_hip_ba* b, int32_t solver)
{
    { const int nb = need_built(b); if (nb) return nb; }
    if (b->pending_iters >= 0) { set_error("set_solver between optimize_begin and optimize_end"); return LPSLAM_HIP_ERR_INVALID; }
    int want = solver == LPSLAM_HIP_BA_SOLVER_DENSE ? -1 : b->band_hbw_structure;
    if (solver == LPSLAM_HIP_BA_SOLVER_BAND && b->band_hbw_structure < 0) { set_error("the window is not block-banded (a landmark spans more than %d free keyframes, or the system exceeds %d unknowns)", BD_MAXHBW + 1, 16 * BC_MAXS); return LPSLAM_HIP_ERR_INVALID; }
    if (want == b->h_view.band_hbw) return LPSLAM_HIP_OK;
    LP_HIP(hipSetDevice(b->ctx->cfg.device));
    LP_HIP(hipStreamSynchronize(b->stream));
    release_stage(b);
    b->h_view.band_hbw = want;
    LP_HIP(hipMemcpy(&b->d_view->band_hbw, &b->h_view.band_hbw, sizeof(int), hipMemcpyHostToDevice));
    // the other solver's leftovers in S (factor entries outside the band / inside it) must not be taken for matrix entries
    const size_t n = (size_t)b->dim_pad;
    LP_HIP(hipMemsetAsync(b->d_red, 0, n * n * sizeof(double), b->stream));
    if (b->dim_pad > b->dim + 1) hipLaunchKernelGGL(k_bs_identity, dim3((b->dim_pad - b->dim - 1 + 255) / 256), dim3(256), 0, b->stream, b->d_red, b->dim, b->dim_pad);
    LP_HIP(hipStreamSynchronize(b->stream));
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_reset(lpslam_hip_ba* b)
{
    const int rc = need_built(b); if (rc) return rc;
    b->h_ctl = fresh_ctl();
    // one launch instead of two device copies and a fill (three runtime operations of ~4 us each on the solve's stream)
    hipLaunchKernelGGL(k_ba_reset, dim3((unsigned)((state_extent(b) + 255) / 256), 1), dim3(256), 0, b->stream, b->d_view);
    LP_HIP(hipGetLastError());
    return LPSLAM_HIP_OK;
}

// New creation-time values for an existing structure (the observation graph stays): what lets a mapping thread build the
// structure of the next window (lpslam_hip_ba_create is asynchronous) while the previous window is still being solved, and hand
// over the poses / landmarks that solve produced when it is done.
int lpslam_hip_ba_set_state(lpslam_hip_ba* b, const double* poses, const double* points)
{
    const int rc = need_built(b); if (rc) return rc;
    if (b->pending_iters >= 0) { set_error("lpslam_hip_ba_set_state while a solve is in flight"); return LPSLAM_HIP_ERR_INVALID; }
    if (!poses && !(points && b->n_points)) return lpslam_hip_ba_reset(b);
    if (uint8_t* x = ensure_xfer(b)) {
        if (b->xfer_in_pending) { LP_HIP(hipEventSynchronize(b->xfer_in_read)); b->xfer_in_pending = false; }      // the previous set_state's kernel has read its values
        double* in_poses = (double*)x; double* in_points = in_poses + Xfer(b).in_points;
        if (poses) memcpy(in_poses, poses, 7 * (size_t)b->n_poses * sizeof(double));
        if (points && b->n_points) memcpy(in_points, points, 3 * (size_t)b->n_points * sizeof(double));
        b->h_ctl = fresh_ctl();
        hipLaunchKernelGGL(k_ba_reset_from_host, dim3((unsigned)((state_extent(b) + 255) / 256), 1), dim3(256), 0, b->stream, b->d_view,
                           poses ? in_poses : nullptr, (points && b->n_points) ? in_points : nullptr);
        LP_HIP(hipGetLastError());
        LP_HIP(hipEventRecord(b->xfer_in_read, b->stream));
        b->xfer_in_pending = true;
        return LPSLAM_HIP_OK;
    }
    if (poses) LP_HIP(hipMemcpyAsync((void*)b->h_view.poses0, poses, 7 * (size_t)b->n_poses * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (points && b->n_points) LP_HIP(hipMemcpyAsync((void*)b->h_view.points0, points, 3 * (size_t)b->n_points * sizeof(double), hipMemcpyHostToDevice, b->stream));
    return lpslam_hip_ba_reset(b);
}

// A read-back through the exchange block in two phases (a batch enqueues every problem's kernel before it waits for the first): the kernel
// that stores the wanted parts of the current state into the "out" half ...
static int state_out_enqueue(lpslam_hip_ba* b, const double* poses, const double* points)
{
    const Xfer f(b);
    const bool want_points = points && b->n_points;
    const long n_max = std::max<long>(poses ? 7L * b->n_poses : 0, want_points ? 3L * b->n_points : 0);
    if (n_max <= 0) return LPSLAM_HIP_OK;
    hipLaunchKernelGGL(k_ba_state_to_host, dim3((unsigned)((n_max + 511) / 512), 1), dim3(256), 0, b->stream, b->d_view,
                       poses ? (double*)b->xfer + f.out_poses : nullptr, want_points ? (double*)b->xfer + f.out_points : nullptr);
    LP_HIP(hipGetLastError());
    return LPSLAM_HIP_OK;
}
// ... and the wait for the problem's stream with the copies out of the block
static int state_out_finish(lpslam_hip_ba* b, double* poses, double* points)
{
    const Xfer f(b);
    LP_HIP(hipStreamSynchronize(b->stream));
    release_stage(b);
    if (poses) memcpy(poses, (const double*)b->xfer + f.out_poses, 7 * (size_t)b->n_poses * sizeof(double));
    if (points && b->n_points) memcpy(points, (const double*)b->xfer + f.out_points, 3 * (size_t)b->n_points * sizeof(double));
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_get(lpslam_hip_ba* b, double* poses, double* points)
{
    const int rc = need_built(b); if (rc) return rc;
    if (ensure_xfer(b)) { const int r2 = state_out_enqueue(b, poses, points); return r2 ? r2 : state_out_finish(b, poses, points); }
    const int cur = b->h_ctl.cur;
    if (poses) LP_HIP(hipMemcpyAsync(poses, b->d_poses[cur], 7 * (size_t)b->n_poses * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (points && b->n_points) LP_HIP(hipMemcpyAsync(points, b->d_points[cur], 3 * (size_t)b->n_points * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    LP_HIP(hipStreamSynchronize(b->stream));
    release_stage(b);
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_set_state_batch(lpslam_hip_ba* const* ps, int32_t n, const double* const* poses, const double* const* points)
{
    if (n < 0 || (n > 0 && !ps)) { set_error("bad batch"); return LPSLAM_HIP_ERR_INVALID; }
    for (int i = 0; i < n; ++i) {
        const int rc = lpslam_hip_ba_set_state(ps[i], poses ? poses[i] : nullptr, points ? points[i] : nullptr);      // (asynchronous: a copy into the exchange block + one launch)
        if (rc) return rc;
    }
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_get_batch(lpslam_hip_ba* const* ps, int32_t n, double* const* poses, double* const* points)
{
    if (n < 0 || (n > 0 && !ps)) { set_error("bad batch"); return LPSLAM_HIP_ERR_INVALID; }
    std::vector<uint8_t> through_block((size_t)n, 0);
    // every problem's state kernel first ...
    for (int i = 0; i < n; ++i) {
        lpslam_hip_ba* b = ps[i];
        if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
        if (!ensure_xfer(b)) continue;                  // no exchange block: the single call below
        const int rc = state_out_enqueue(b, poses ? poses[i] : nullptr, points ? points[i] : nullptr); if (rc) return rc;
        through_block[(size_t)i] = 1;
    }
    // ... then the waits and the copies out
    for (int i = 0; i < n; ++i) {
        lpslam_hip_ba* b = ps[i];
        double* po = poses ? poses[i] : nullptr; double* pt = points ? points[i] : nullptr;
        const int rc = through_block[(size_t)i] ? state_out_finish(b, po, pt) : lpslam_hip_ba_get(b, po, pt);
        if (rc) return rc;
    }
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_pose_optimize(lpslam_hip_ba* b, uint8_t* outlier, int32_t* n_inliers)
{
    int rc = need_built(b); if (rc) return rc;
    const int n = b->n_obs;
    std::vector<uint8_t> active((size_t)std::max(n, 1), 1);
    std::vector<double> chi((size_t)std::max(n, 1));
    const int keep_fixed = b->points_fixed;
    b->points_fixed = 1;
    int done, bad = 0, robust = 1;
    if ((rc = lpslam_hip_ba_set_active(b, nullptr))) return rc;
    for (int trial = 0; trial < 4; ++trial) {
        if ((rc = lpslam_hip_ba_optimize(b, robust, 10, nullptr, &done))) return rc;
        if ((rc = lpslam_hip_ba_chi2(b, chi.data(), nullptr))) return rc;
        bad = classify_active(b, chi.data(), nullptr, active.data());
        if ((rc = lpslam_hip_ba_set_active(b, active.data()))) return rc;
        if (trial == 4 - 2) robust = 0;
        if (n - bad < 5) break;
    }
    b->points_fixed = keep_fixed;
    if (outlier) for (int k = 0; k < n; ++k) outlier[k] = !active[(size_t)k];      // every pass classifies anew: an outlier is what the last one switched off
    if (n_inliers) *n_inliers = n - bad;
    return LPSLAM_HIP_OK;
}

// One window here, n windows in lp_ba_local_batch: the same steps with the same helpers between the solves.  The solves differ on purpose:
// a single window goes through optimize_begin / _end and so through graph replay, the batch is one launch chain and waits once per step.
int lpslam_hip_ba_local(lpslam_hip_ba* b, int32_t first_iters, int32_t second_iters, uint8_t* outlier)
{
    int rc = need_built(b); if (rc) return rc;
    const int n = b->n_obs;
    std::vector<uint8_t> active((size_t)std::max(n, 1), 1), pos((size_t)std::max(n, 1));
    std::vector<double> chi((size_t)std::max(n, 1));
    int done;
    if ((rc = lpslam_hip_ba_set_active(b, nullptr))) return rc;
    if ((rc = lpslam_hip_ba_optimize(b, 1, first_iters, nullptr, &done))) return rc;
    if ((rc = lpslam_hip_ba_chi2(b, chi.data(), pos.data()))) return rc;
    classify_active(b, chi.data(), pos.data(), active.data());
    if ((rc = lpslam_hip_ba_set_active(b, active.data()))) return rc;
    if ((rc = lpslam_hip_ba_optimize(b, 0, second_iters, nullptr, &done))) return rc;
    if ((rc = lpslam_hip_ba_chi2(b, chi.data(), pos.data()))) return rc;
    if (outlier) classify_outliers(b, chi.data(), pos.data(), active.data(), outlier);
    return LPSLAM_HIP_OK;
}

}  // extern "C"

// lpslam_hip_ba_local for n prepared (not yet built) windows at once: ONE structure build, the two optimisations as batched launch
// chains (blockIdx.y = window), the per-observation chi2 passes and activity masks of all windows between them with one wait each.
// What the mapping threads of several sessions submit together (share.hip); the arithmetic per window is that of the single call.
int lp_ba_local_batch(lpslam_hip_ba* const* ps, int n, int first_iters, int second_iters, uint8_t* const* outliers, double* const* poses_out, double* const* points_out)
{
    int rc = lpslam_hip_ba_build_batch(ps, n); if (rc) return rc;
    hipStream_t s = ps[0]->stream;
    for (int i = 1; i < n; ++i) if (ps[i]->stream != s) { set_error("a shared batch of windows needs them on one stream"); return LPSLAM_HIP_ERR_INVALID; }
    std::vector<std::vector<double>> chi((size_t)n);
    std::vector<std::vector<uint8_t>> pos((size_t)n), active((size_t)n);
    for (int i = 0; i < n; ++i) { const size_t no = (size_t)std::max(ps[i]->n_obs, 1); chi[(size_t)i].resize(no); pos[(size_t)i].resize(no); active[(size_t)i].resize(no, 1); }
    auto chi2_all = [&]() -> int {
        for (int i = 0; i < n; ++i) { const int r2 = enqueue_chi2(ps[i], chi[(size_t)i].data(), pos[(size_t)i].data()); if (r2) return r2; }
        LP_HIP(hipStreamSynchronize(s));
        return LPSLAM_HIP_OK;
    };
    if ((rc = lpslam_hip_ba_optimize_batch(ps, n, 1, first_iters, nullptr, 0, nullptr))) return rc;
    if ((rc = chi2_all())) return rc;
    for (int i = 0; i < n; ++i) {
        classify_active(ps[i], chi[(size_t)i].data(), pos[(size_t)i].data(), active[(size_t)i].data());
        if ((rc = enqueue_active(ps[i], active[(size_t)i].data()))) return rc;
    }
    if ((rc = lpslam_hip_ba_optimize_batch(ps, n, 0, second_iters, nullptr, 0, nullptr))) return rc;
    if ((rc = chi2_all())) return rc;
    for (int i = 0; i < n; ++i)
        if (outliers && outliers[i]) classify_outliers(ps[i], chi[(size_t)i].data(), pos[(size_t)i].data(), active[(size_t)i].data(), outliers[i]);
    if ((rc = lpslam_hip_ba_get_batch(ps, n, poses_out, points_out))) return rc;
    for (int i = 0; i < n; ++i) { release_stage(ps[i]); ps[i]->quiesced = true; }
    return LPSLAM_HIP_OK;
}

extern "C" {

// A keyframe's local bundle adjustment as ONE call: the window is created from the caller's arrays, solved (lpslam_hip_ba_local:
// first_iters with the robust kernel, outlier classification, second_iters without), its state read back into `poses` / `points` and
// destroyed -- what a mapping thread does per keyframe.  With several sessions submitting windows at the same time (shared launches on)
// the windows are built and solved together by one of the calling threads.
int lpslam_hip_ba_local_window(lpslam_hip_ctx* ctx, double* poses, const uint8_t* fixed, int32_t n_poses, double* points, int32_t n_points,
                               const lpslam_hip_ba_obs* obs, int32_t n_obs, const lpslam_hip_ba_camera* cam, int32_t first_iters, int32_t second_iters, uint8_t* outlier)
{
    lpslam_hip_ba* b = nullptr;
    int rc = lpslam_hip_ba_prepare(ctx, poses, fixed, n_poses, points, n_points, obs, n_obs, cam, &b);
    if (rc) return rc;
    const int shared = (ctx->role_solve && b->stream == ctx->role_solve) ? lp_share_ba_local(ctx, b, first_iters, second_iters, outlier, poses, points) : LP_SHARE_DIRECT;
    if (shared < 0) rc = -shared;
    else if (shared == LP_SHARE_DIRECT) {
        rc = lpslam_hip_ba_build_batch(&b, 1);
        if (!rc) rc = lpslam_hip_ba_local(b, first_iters, second_iters, outlier);
        if (!rc) rc = lpslam_hip_ba_get(b, poses, points);
    }
    lpslam_hip_ba_destroy(b);
    return rc;
}

}  // extern "C"
