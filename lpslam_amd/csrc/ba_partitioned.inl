// ba_partitioned.inl -- the landmark-partitioned (multi-GPU) solve (included by ba.hip behind ba_host.inl): the step_* API, whose
// all-reduces the caller runs, and optimize_partitioned*, which enqueues them itself through RCCL or a callback.

// ---- partitioned (multi-GPU) solve: one LM trial in three phases with the caller's all-reduces in between ------------------
//   lpslam_hip_ba_step_begin : (linearise if needed) + partial Schur complement -> reduced buffer [S | rhs | b_p | diag H_pp |
//                              chi2]: SUM all-reduce; scalar buffer entry [4] = max diag H_ll: MAX all-reduce (first trial)
//   lpslam_hip_ba_step_solve : lambda control start, factor, solve, update into the trial state; scalar buffer [1] = trial
//                              chi2 and [2] = landmark scale term: SUM all-reduce ([3], the pose term, is identical on all ranks)
//   lpslam_hip_ba_step_end   : accept / reject; reports the control state
// Every phase ends with a stream synchronise so the caller's collective may touch the buffers right away.
extern "C" {

// the partitioned (all-reduced) solve works on the dense reduced buffer
static int ensure_dense(lpslam_hip_ba* b) { return b->h_view.band_hbw >= 0 ? lpslam_hip_ba_set_solver(b, LPSLAM_HIP_BA_SOLVER_DENSE) : LPSLAM_HIP_OK; }

int lpslam_hip_ba_step_begin(lpslam_hip_ba* b, int32_t robust, int32_t first)
{
    { const int nb = need_built(b); if (nb) return nb; }
    LP_HIP(hipSetDevice(b->ctx->cfg.device));
    int rc;
    if ((rc = ensure_dense(b))) return rc;
    if (first) { if ((rc = begin_optimize(b, robust, MAX_LOG))) return rc; }
    b->robust = robust;
    // lambda is needed by the Schur complement but lambda_0 depends on all-reduced diagonals: on the very first trial the
    // caller runs begin twice (first = 1: linearisation only; first = 0 after the reduction of the diagonals)
    if ((rc = enqueue_linearize(single_launch(b), 0))) return rc;
    if (!first) { if ((rc = enqueue_reduce(single_launch(b), 0))) return rc; }
    LP_HIP(hipStreamSynchronize(b->stream));
    release_stage(b);
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_step_lambda0(lpslam_hip_ba* b)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    hipLaunchKernelGGL(k_lm_begin, dim3(1, 1), dim3(64), 0, b->stream, b->d_view);
    LP_HIP(hipGetLastError());
    LP_HIP(hipStreamSynchronize(b->stream));
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_step_solve(lpslam_hip_ba* b)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    int rc = enqueue_solve(single_launch(b), 0); if (rc) return rc;
    LP_HIP(hipStreamSynchronize(b->stream));
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_step_end(lpslam_hip_ba* b, int32_t* accepted, int32_t* iteration_finished)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    const int before = b->h_ctl.outer_done;
    hipLaunchKernelGGL(k_lm_decide, dim3(1, 1), dim3(64), 0, b->stream, b->d_view);
    LP_HIP(hipGetLastError());
    int rc = read_ctl(b); if (rc) return rc;
    if (accepted) *accepted = b->h_ctl.last_accepted;
    if (iteration_finished) *iteration_finished = (b->h_ctl.outer_done != before || b->h_ctl.stopped) ? 1 : 0;
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_status(lpslam_hip_ba* b, int32_t* outer_done, int32_t* stopped, double* lambda, double* chi2)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    if (outer_done) *outer_done = b->h_ctl.outer_done;
    if (stopped) *stopped = b->h_ctl.stopped;
    if (lambda) *lambda = b->h_ctl.lambda;
    if (chi2) *chi2 = b->h_ctl.current_chi;
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_reduced_buffer(lpslam_hip_ba* b, void** dev_ptr, int64_t* n_doubles)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    if (dev_ptr) *dev_ptr = b->d_red;
    if (n_doubles) *n_doubles = b->red_n;
    return LPSLAM_HIP_OK;
}

int lpslam_hip_ba_scalar_buffer(lpslam_hip_ba* b, void** dev_ptr, int64_t* n_doubles)
{
    if (!b) { set_error("null problem"); return LPSLAM_HIP_ERR_INVALID; }
    if (dev_ptr) *dev_ptr = b->d_scal;
    if (n_doubles) *n_doubles = 8;
    return LPSLAM_HIP_OK;
}

}  // extern "C"

// ---- landmark-partitioned global BA driven from C++: RCCL all-reduces enqueued on the problem's own stream ---------------------
// north star: "host code stays C++ ... RCCL all-reduce over xGMI only for the shared-pose normal equations" (SURVEY.md 8(e)).
// Every rank holds all poses and the observations of its landmarks.  One LM trial on the stream, no host synchronisation in it:
//   linearise -> [first trial of a call: SUM (b_p, diag H_pp, chi2) + MAX (max diag H_ll) -> lambda_0] -> partial Schur complement
//   -> pack the lower triangle of S + rhs + b_p + diag H_pp + chi2 -> ONE sum all-reduce (5.9 MB at 200 keyframes instead of the
//   11.8 MB of the dense square) -> unpack -> factor / solve (redundantly on every rank) -> landmark back substitution, trial chi2 ->
//   SUM (trial chi2, landmark scale term) -> accept / reject on the device, identical on every rank.
// RCCL is bound at run time (dlopen): the library has no link-time dependency on it and single-GPU users never load it.
namespace {

typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
constexpr int kNcclFloat64 = 8, kNcclSum = 0, kNcclMax = 2;      // rccl.h: ncclFloat64, ncclSum, ncclMax
nccl_allreduce_fn load_nccl_allreduce(std::string* why)
{
    static std::atomic<nccl_allreduce_fn> cached{nullptr};
    nccl_allreduce_fn f = cached.load();
    if (f) return f;
    // the copy already in the process first (a host that links RCCL, or torch's bundled one), then the system library
    void* h = nullptr;
    const char* last = nullptr;
    const struct { const char* name; int flags; } tries[] = {{"librccl.so.1", RTLD_NOW | RTLD_NOLOAD}, {"librccl.so", RTLD_NOW | RTLD_NOLOAD},
        {"librccl.so.1", RTLD_NOW | RTLD_GLOBAL}, {"librccl.so", RTLD_NOW | RTLD_GLOBAL}, {"/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL}};
    for (const auto& t : tries) {
        (void)dlerror();
        h = dlopen(t.name, t.flags);
        if (h) break;
        if (!(t.flags & RTLD_NOLOAD)) { const char* e = dlerror(); if (e) { if (why) *why = e; last = e; } }      // read once: dlerror() clears itself
    }
    if (!h) { if (why && !last) *why = "not found"; return nullptr; }
    (void)dlerror();
    f = (nccl_allreduce_fn)dlsym(h, "ncclAllReduce");
    if (!f) { const char* e = dlerror(); if (why) *why = e ? e : "ncclAllReduce: symbol not found"; return nullptr; }
    cached.store(f);
    return f;
}
struct NcclUser { nccl_allreduce_fn fn; void* comm; };
int nccl_adapter(void* user, void* buf, size_t count, int32_t op, void* stream)
{
    const NcclUser* u = (const NcclUser*)user;
    return u->fn(buf, buf, count, kNcclFloat64, op == LPSLAM_HIP_REDUCE_MAX ? kNcclMax : kNcclSum, u->comm, (hipStream_t)stream);
}

// lower triangle of the dim x dim reduced system (row r, columns 0..r) <-> packed [r (r + 1) / 2 + c]; the tail of the reduced
// buffer (rhs | b_p | diag H_pp | chi2, 3 n + 8 doubles) rides behind it
__global__ __launch_bounds__(256) void k_ba_pack(const BaView* __restrict__ views, double* packed, int unpack)
{
    BaView v = views[0];                                 // one problem; blockIdx.y is the matrix row here
    const int n = v.dim_pad, dim = v.dim;
    const size_t tri = (size_t)dim * (dim + 1) / 2;
    const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (r < dim) {
        if (c <= r) {
            const size_t p = (size_t)r * (r + 1) / 2 + c;
            if (unpack) v.S[(size_t)r * n + c] = packed[p]; else packed[p] = v.S[(size_t)r * n + c];
        }
    } else if (r == dim) {
        for (int i = c; i < 3 * n + 8; i += gridDim.x * 256) { if (unpack) v.rhs[i] = packed[tri + i]; else packed[tri + i] = v.rhs[i]; }
    }
}

}  // namespace

extern "C" int lpslam_hip_ba_optimize_partitioned(lpslam_hip_ba* b, void* nccl_comm, int32_t robust, int32_t iters, lpslam_hip_ba_iter_log* log, int32_t* done_out)
{
    if (!b || !nccl_comm) { set_error("null problem / communicator"); return LPSLAM_HIP_ERR_INVALID; }
    std::string why;
    NcclUser u{load_nccl_allreduce(&why), nccl_comm};
    if (!u.fn) { set_error("RCCL (librccl.so) could not be loaded: %s", why.c_str()); return LPSLAM_HIP_ERR_DEVICE; }
    return lpslam_hip_ba_optimize_partitioned_with(b, nccl_adapter, &u, robust, iters, log, done_out);
}

extern "C" int lpslam_hip_ba_optimize_partitioned_with(lpslam_hip_ba* b, lpslam_hip_allreduce_fn allreduce_cb, void* user, int32_t robust, int32_t iters,
                                                       lpslam_hip_ba_iter_log* log, int32_t* done_out)
{
    if (b) { const int nb = need_built(b); if (nb) return nb; }
    if (!b || !allreduce_cb) { set_error("null problem / all-reduce callback"); return LPSLAM_HIP_ERR_INVALID; }
    if (iters < 0 || iters > MAX_LOG) { set_error("iterations must be in [0,%d]", MAX_LOG); return LPSLAM_HIP_ERR_INVALID; }
    if (b->pending_iters >= 0) { set_error("optimize_begin pending"); return LPSLAM_HIP_ERR_INVALID; }
    auto allreduce = [&](double* buf, size_t count, int op) -> int { return allreduce_cb(user, buf, count, op, (void*)b->stream); };      // in place, on the problem's stream
    LP_HIP(hipSetDevice(b->ctx->cfg.device));
    { const int rd = ensure_dense(b); if (rd) return rd; }      // every rank all-reduces the dense reduced buffer, whatever the window's shape
    hipStream_t s = b->stream;
    const size_t n = (size_t)b->dim_pad, tri = (size_t)b->dim * (b->dim + 1) / 2, packed_n = tri + 3 * n + 8;
    void* pk = nullptr; size_t pk_cap = 0;
    int rc = lp_pool_alloc(b->ctx, packed_n * sizeof(double), &pk, &pk_cap); if (rc) return rc;
    double* d_packed = (double*)pk;
    auto release = [&]() { lp_pool_free(b->ctx, pk, pk_cap); };
#define PT_TRY(x) do { rc = (x); if (rc) { (void)hipStreamSynchronize(s); release(); return rc; } } while (0)
    BaLaunch L = single_launch(b);
    L.robust = robust; b->robust = robust;
    double* tail = b->d_red + n * n;                         // rhs | b_p | diag H_pp | chi2
    PT_TRY(begin_optimize(b, robust, iters));
    auto enqueue_units = [&](int units, bool first_batch) -> int {
        for (int u = 0; u < units; ++u) {
            int r2;
            if ((r2 = enqueue_linearize(L, 0))) return r2;
            if (first_batch && u == 0) {
                // lambda_0 = 1e-5 max diag H over ALL ranks' landmarks and the summed pose blocks: needed before the first Schur complement
                if (allreduce(tail, 3 * n + 8, LPSLAM_HIP_REDUCE_SUM)) { set_error("all-reduce (diagonals) failed"); return LPSLAM_HIP_ERR_DEVICE; }
                if (allreduce(b->d_scal + 4, 1, LPSLAM_HIP_REDUCE_MAX)) { set_error("all-reduce (max diag) failed"); return LPSLAM_HIP_ERR_DEVICE; }
                hipLaunchKernelGGL(k_lm_begin, dim3(1, 1), dim3(64), 0, s, L.d_views);
            }
            if ((r2 = enqueue_reduce(L, 0))) return r2;
            if (b->dim > 0) {
                hipLaunchKernelGGL(k_ba_pack, dim3((b->dim + 255) / 256, b->dim + 1, 1), dim3(256), 0, s, L.d_views, d_packed, 0);
                if (allreduce(d_packed, packed_n, LPSLAM_HIP_REDUCE_SUM)) { set_error("all-reduce (reduced system) failed"); return LPSLAM_HIP_ERR_DEVICE; }
                hipLaunchKernelGGL(k_ba_pack, dim3((b->dim + 255) / 256, b->dim + 1, 1), dim3(256), 0, s, L.d_views, d_packed, 1);
            } else if (allreduce(tail, 3 * n + 8, LPSLAM_HIP_REDUCE_SUM)) { set_error("all-reduce failed"); return LPSLAM_HIP_ERR_DEVICE; }
            if ((r2 = enqueue_solve(L, 0))) return r2;
            if (allreduce(b->d_scal + 1, 2, LPSLAM_HIP_REDUCE_SUM)) { set_error("all-reduce (trial chi2) failed"); return LPSLAM_HIP_ERR_DEVICE; }
            hipLaunchKernelGGL(k_lm_decide, dim3(1, 1), dim3(64), 0, s, L.d_views);
            LP_HIP(hipGetLastError());
        }
        return LPSLAM_HIP_OK;
    };
    const int want_log = (log && b->pin) ? iters : 0;
    if (iters > 0) PT_TRY(enqueue_units(iters, true));
    // every rank sees the same control block (identical inputs after every all-reduce), so every rank runs the same number of units
    PT_TRY(finish_trials(&b, 1, iters, [&](int units) { return enqueue_units(units, false); }, [&] { return read_ctl(b, want_log); }));
#undef PT_TRY
    release();
    return finish_call(b, log, want_log > 0, done_out);
}
