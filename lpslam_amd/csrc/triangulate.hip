// triangulate.hip -- new landmarks between keyframes on the device (the definition is triangulate_math.h).
//   k_epi_topk    one wavefront per (query keypoint of the new keyframe, neighbour keyframe): the neighbour's keypoints pass the
//                 candidate gate (group, epipole, epipolar line -- FP64), the survivors' descriptors are compared, the eight nearest
//                 by (distance, index) and the number that passed are kept
//   k_tri_pairs   one thread per listed candidate: tri_pair in FP64, results straight into page-locked host memory, then the
//                 completion flag (internal.h, lp_signal_done)
// One upload, the two launches and one wait per keyframe: an LpStagedCall (internal.h, DESIGN.md section 40 -- the two blocks, the
// done flag and what becomes of them when a stream is late or dead).  The order-dependent part (a neighbour's keypoint taken by an
// earlier query is invisible to later ones) is the caller's replay over these lists (lpslam_tri::replay_host).
#include "internal.h"
#include "desc_wave.h"
#include "triangulate_math.h"
#include <algorithm>
#include <cmath>

using namespace lpslam;
namespace tri = lpslam_tri;

namespace {

// what a neighbour's keypoint needs for the gate, one 16-byte load: position, octave | stereo flag << 8, group
struct GateRec { float x, y; int32_t oct_flags, group; };
static_assert(sizeof(GateRec) == 16, "gate record");
// the staged input block: head, sets, group1, then per set the gate records, descriptors, right-image columns and depths
struct TriSetDev { tri::Epipolar e; tri::View v; unsigned o_gate, o_desc, o_xr, o_depth; int32_t n, pad[3]; };
struct TriHead { tri::Camera cam; tri::View v1; float scale[LPSLAM_HIP_MAX_LEVELS]; unsigned o_sets, o_group1; int32_t nq, n_sets; };

constexpr unsigned long long NONE = tri::kNoKey;
static_assert(NONE == kNoKey, "the empty list entry of the host definition and of the wavefront top-K");

// (depth1: the slot's depth column, nullptr for a camera without a baseline)
__global__ __launch_bounds__(256) void k_epi_topk(const uint8_t* __restrict__ blk, const lpslam_hip_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1,
                                                  const float* __restrict__ depth1, unsigned long long* __restrict__ out_keys, int* __restrict__ out_count)
{
    const TriHead* head = reinterpret_cast<const TriHead*>(blk);
    const int nq = head->nq;
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;                                                // (no workgroup barrier below: a wavefront may leave)
    const TriSetDev* set = reinterpret_cast<const TriSetDev*>(blk + head->o_sets) + blockIdx.y;
    const size_t oq = (size_t)blockIdx.y * (size_t)nq + (size_t)q;
    const int g = reinterpret_cast<const int32_t*>(blk + head->o_group1)[q];
    const int n = g < 0 ? 0 : set->n;
    const tri::Epipolar e = set->e;
    const float qx = kp1[q].x, qy = kp1[q].y;
    const bool q_stereo = depth1 ? tri::is_stereo(head->cam, depth1[q]) : false;
    double l[3];
    tri::epipolar_line(e.F, (double)qx, (double)qy, l);
    uint32_t a[8];
    desc_load8(desc1 + 32 * (size_t)q, a);
    const GateRec* gate = reinterpret_cast<const GateRec*>(blk + set->o_gate);
    const uint8_t* desc2 = blk + set->o_desc;
    const float* scale = head->scale;
    unsigned long long top[tri::kListed];
#pragma unroll
    for (int r = 0; r < tri::kListed; ++r) top[r] = NONE;
    int cnt = 0;
    // Two passes, in the shape of the window matcher's scan (match.hip, proj_topk_body; list and top-K steps: desc_wave.h): pass 1 keeps
    // eight gate records of a lane in flight and appends the survivors of the gate to the wavefront's list in LDS; pass 2 gives every
    // listed keypoint a lane, which loads its descriptor.  Keys are unique and the eight smallest are wanted: their order is free.
    constexpr int PT_U = 8, PT_CAP = 2048;
    __shared__ uint16_t s_list[4][PT_CAP];
    uint16_t* list = s_list[threadIdx.x >> 6];
    int n_list = 0;                                                     // uniform over the wavefront
    auto second_pass = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < n_list; k += 64) {
            const int j = list[k];
            const uint4* d = reinterpret_cast<const uint4*>(desc2 + 32 * (size_t)j);
            const uint4 d0 = d[0], d1 = d[1];
            const uint32_t b[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
            const int h = tri::hamming(a, b);
            if (h > tri::kHammingMax) continue;
            ++cnt;
            unsigned long long key = ((unsigned long long)h << 32) | (unsigned long long)j;
            topk_insert(top, key);
        }
        __builtin_amdgcn_wave_barrier();
        n_list = 0;
    };
    for (int j0 = lane; j0 - lane < n; j0 += 64 * PT_U) {               // (uniform trip count: the ballots below want every lane)
        int4 rec[PT_U];
#pragma unroll
        for (int u = 0; u < PT_U; ++u) rec[u] = *reinterpret_cast<const int4*>(gate + min(j0 + 64 * u, n - 1));
        if (n_list + 64 * PT_U > PT_CAP) second_pass();
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
            const int j = j0 + 64 * u;
            bool pass = j < n && rec[u].w == g;
            if (pass) {
                const int oct = rec[u].z & 255;
                pass = tri::gate_geometry(l, q_stereo || (rec[u].z >> 8) != 0, e, (double)__int_as_float(rec[u].x), (double)__int_as_float(rec[u].y), (double)scale[oct & (LPSLAM_HIP_MAX_LEVELS - 1)]);
            }
            wave_append(list, n_list, pass, j);
        }
    }
    second_pass();
    cnt = wave_sum_i32(cnt);
    wave_topk_pop(top, [&](int r, unsigned long long m) { if (lane == 0) out_keys[tri::kListed * oq + r] = m; });      // keys are unique (index bits)
    if (lane == 0) out_count[oq] = cnt;
}

__device__ __forceinline__ tri::Keypoint slot_keypoint(const lpslam_hip_keypoint* kp, const float* xr, const float* depth, int i)
{
    // (a slot's octave comes from the extraction: the mask only keeps a planted value inside the scale table)
    return tri::Keypoint{kp[i].x, kp[i].y, kp[i].octave & (LPSLAM_HIP_MAX_LEVELS - 1), xr ? xr[i] : -1.0f, depth ? depth[i] : -1.0f};
}

// h_count / h_keys / h_code / h_X: page-locked host memory.  An entry beyond min(count, 8) of its query is not written, X only with a
// code other than 0: the host reads what the counts and codes tell it to.
__global__ __launch_bounds__(256) void k_tri_pairs(const uint8_t* __restrict__ blk, const lpslam_hip_keypoint* __restrict__ kp1, const float* __restrict__ xr1,
                                                   const float* __restrict__ depth1, const unsigned long long* __restrict__ keys, const int* __restrict__ count,
                                                   int* __restrict__ h_count, unsigned long long* __restrict__ h_keys, int* __restrict__ h_code, double* __restrict__ h_X,
                                                   unsigned* done_counter, int* done_flag, int done_seq)
{
    const TriHead* head = reinterpret_cast<const TriHead*>(blk);
    const int nq = head->nq;
    const size_t total = (size_t)head->n_sets * (size_t)nq * tri::kListed;
    const size_t ent = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ent < total) {
        const size_t oq = ent / tri::kListed;
        const int r = (int)(ent % tri::kListed), s = (int)(oq / (size_t)nq), q = (int)(oq % (size_t)nq);
        const int cnt = count[oq];
        if (r == 0) h_count[oq] = cnt;
        if (r < cnt) {                                                  // (a list holds min(count, 8) keys)
            const unsigned long long key = keys[ent];
            const TriSetDev* set = reinterpret_cast<const TriSetDev*>(blk + head->o_sets) + s;
            const int j = max(min((int)(key & 0xffffffffu), set->n - 1), 0);      // (a listed index is inside the set: the clamp is a seat belt)
            const GateRec gr = reinterpret_cast<const GateRec*>(blk + set->o_gate)[j];
            const tri::Keypoint k2{gr.x, gr.y, gr.oct_flags & (LPSLAM_HIP_MAX_LEVELS - 1), reinterpret_cast<const float*>(blk + set->o_xr)[j], reinterpret_cast<const float*>(blk + set->o_depth)[j]};
            const tri::Keypoint k1 = slot_keypoint(kp1, xr1, depth1, q);
            double X[3];
            const int code = tri::tri_pair(head->cam, head->scale, head->v1, set->v, k1, k2, X);
            h_keys[ent] = key;
            h_code[ent] = code;
            if (code) { h_X[3 * ent] = X[0]; h_X[3 * ent + 1] = X[1]; h_X[3 * ent + 2] = X[2]; }
        }
    }
    lp_signal_done(done_counter, done_flag, done_seq);
}

// tri_pair on caller-given pairs (the parity hook): device memory in, device memory out
struct PairsHead { tri::Camera cam; tri::View v1, v2; float scale[LPSLAM_HIP_MAX_LEVELS]; };
__global__ __launch_bounds__(256) void k_tri_pair_list(PairsHead head, const tri::Keypoint* __restrict__ k1, const tri::Keypoint* __restrict__ k2, int n,
                                                       const float* __restrict__ scale, int32_t* __restrict__ code, double* __restrict__ X)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    tri::Keypoint a = k1[i], b = k2[i];
    a.octave &= LPSLAM_HIP_MAX_LEVELS - 1; b.octave &= LPSLAM_HIP_MAX_LEVELS - 1;
    double x[3] = {NAN, NAN, NAN};
    code[i] = tri::tri_pair(head.cam, scale, head.v1, head.v2, a, b, x);
    X[3 * (size_t)i] = x[0]; X[3 * (size_t)i + 1] = x[1]; X[3 * (size_t)i + 2] = x[2];
}

bool camera_ok(const lpslam_hip_tri_camera* cam)
{
    const double v[6] = {cam->fx, cam->fy, cam->cx, cam->cy, cam->focal_x_baseline, cam->scale_factor};
    for (double d : v) if (!std::isfinite(d)) return false;
    return cam->fx > 0.0 && cam->fy > 0.0 && cam->focal_x_baseline >= 0.0 && cam->scale_factor >= 1.0;
}
bool finite_all(const double* p, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false; return true; }
bool pose_ok(const double* p) { return finite_all(p, 7) && p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3] > 0.0; }
tri::Camera to_camera(const lpslam_hip_tri_camera* c) { return tri::Camera{c->fx, c->fy, c->cx, c->cy, c->focal_x_baseline, c->scale_factor}; }
void fill_scale(float* dst, const float* scale, int n_levels) { for (int l = 0; l < LPSLAM_HIP_MAX_LEVELS; ++l) dst[l] = l < n_levels ? scale[l] : 1.0f; }

}  // namespace

extern "C" {

int lpslam_hip_triangulate_neighbours(lpslam_hip_ctx* c, int image, const int32_t* group1, const double* pose1, const lpslam_hip_tri_camera* cam,
                                      const lpslam_hip_tri_set* sets, int32_t n_sets, const float* scale, int32_t n_levels, int32_t capacity,
                                      int32_t* n_queries, int32_t* out_j, int32_t* out_dist, int32_t* out_code, double* out_X, int32_t* out_count)
{
    if (!c) { set_error("null context"); return LPSLAM_HIP_ERR_INVALID; }
    if (image < 0 || image >= c->cfg.max_images) { set_error("image slot %d out of range [0,%d)", image, c->cfg.max_images); return LPSLAM_HIP_ERR_CAPACITY; }
    if (!pose1 || !cam || !scale || !n_queries || n_sets < 0 || (n_sets > 0 && !sets) || capacity < 0) { set_error("triangulate_neighbours: null argument or negative count"); return LPSLAM_HIP_ERR_INVALID; }
    if (n_sets > tri::kMaxSets) { set_error("triangulate_neighbours: %d neighbours, at most %d", n_sets, tri::kMaxSets); return LPSLAM_HIP_ERR_CAPACITY; }
    if (n_levels < 1 || n_levels > LPSLAM_HIP_MAX_LEVELS) { set_error("triangulate_neighbours: %d levels outside 1 .. %d", n_levels, LPSLAM_HIP_MAX_LEVELS); return LPSLAM_HIP_ERR_INVALID; }
    if (!camera_ok(cam) || !pose_ok(pose1)) { set_error("triangulate_neighbours: camera or pose is not usable"); return LPSLAM_HIP_ERR_INVALID; }
    for (int l = 0; l < n_levels; ++l) if (!(scale[l] > 0.0f) || !std::isfinite(scale[l])) { set_error("triangulate_neighbours: scale[%d] is not positive", l); return LPSLAM_HIP_ERR_INVALID; }
    for (int i = 0; i < n_sets; ++i) {
        const lpslam_hip_tri_set& st = sets[i];
        if (st.n < 0 || (st.n > 0 && (!st.kpts || !st.desc32 || !st.group)) || ((st.x_right == nullptr) != (st.depth == nullptr))) { set_error("triangulate_neighbours: set %d has a null array or a negative count", i); return LPSLAM_HIP_ERR_INVALID; }
        if (st.n > c->slots_per_image || st.n > 65535) { set_error("triangulate_neighbours: set %d has %d keypoints, at most %d", i, st.n, c->slots_per_image); return LPSLAM_HIP_ERR_CAPACITY; }
        if (!pose_ok(st.pose) || !finite_all(st.F, 9) || (st.has_epipole && !finite_all(st.epipole, 2))) { set_error("triangulate_neighbours: set %d has a pose, F or epipole that is no number", i); return LPSLAM_HIP_ERR_INVALID; }
        for (int j = 0; j < st.n; ++j) if (st.kpts[j].octave < 0 || st.kpts[j].octave >= n_levels) { set_error("triangulate_neighbours: set %d, keypoint %d: octave %d outside the scale table", i, j, st.kpts[j].octave); return LPSLAM_HIP_ERR_INVALID; }
    }
    if ((size_t)image >= c->kp_written.size() || !c->kp_written[(size_t)image]) { set_error("triangulate_neighbours: image slot %d holds no extraction", image); return LPSLAM_HIP_ERR_INVALID; }
    LP_HIP(hipSetDevice(c->cfg.device));
    int32_t nq = 0;
    if (int rc = lpslam_hip_keypoint_count(c, image, &nq)) return rc;
    if (nq < 0 || nq > c->slots_per_image) { set_error("triangulate_neighbours: image slot %d holds no valid keypoint count (%d)", image, nq); return LPSLAM_HIP_ERR_INVALID; }
    *n_queries = nq;
    if (nq > capacity) { set_error("triangulate_neighbours: result rows too few (%d < %d)", capacity, nq); return LPSLAM_HIP_ERR_CAPACITY; }
    if (nq > 0 && n_sets > 0 && (!group1 || !out_j || !out_dist || !out_code || !out_X || !out_count)) { set_error("triangulate_neighbours: null argument"); return LPSLAM_HIP_ERR_INVALID; }
    if (nq == 0 || n_sets == 0) return LPSLAM_HIP_OK;
    hipStream_t s = c->stream;
    const LpMatchTrace tr;
    // page-locked block: flag | input (head, sets, group1, per set: gate records, descriptors, right-image columns, depths) | results
    // (counts, keys, codes, X); device block: the input, then the lists of k_epi_topk
    const size_t entries = (size_t)n_sets * (size_t)nq * tri::kListed, lists = (size_t)n_sets * (size_t)nq;
    const size_t o_in = 64;
    LpLayout dev;
    dev.take(sizeof(TriHead));
    const size_t o_sets = dev.take((size_t)n_sets * sizeof(TriSetDev)), o_group1 = dev.take((size_t)nq * 4);
    std::vector<TriSetDev> dev_sets((size_t)n_sets);
    for (int i = 0; i < n_sets; ++i) {
        TriSetDev& d = dev_sets[(size_t)i];
        const size_t n = (size_t)std::max(sets[i].n, 1);                 // (an empty set keeps one zeroed record: the clamped loads stay inside)
        d.o_gate = (unsigned)dev.take(n * sizeof(GateRec)); d.o_desc = (unsigned)dev.take(n * 32);
        d.o_xr = (unsigned)dev.take(n * 4); d.o_depth = (unsigned)dev.take(n * 4);
    }
    const size_t in_bytes = dev.at;
    const size_t d_keys_off = dev.take(entries * 8), d_cnt_off = dev.take(lists * 4);
    LpLayout host{o_in + in_bytes};
    const size_t h_cnt_off = host.take(lists * 4), h_keys_off = host.take(entries * 8), h_code_off = host.take(entries * 4), h_X_off = host.take(entries * 24);
    LpStagedCall call{c, s, "triangulate_neighbours"};
    if (int rc = call.open(host.at, dev.at, LP_DONE_TRIANGULATE)) return rc;
    uint8_t *hb = call.host, *base = call.dev(), *in = hb + o_in;
    const tri::Camera camera = to_camera(cam);
    TriHead head{};
    head.cam = camera; head.v1 = tri::view_from_pose(pose1);
    fill_scale(head.scale, scale, n_levels);
    head.o_sets = (unsigned)o_sets; head.o_group1 = (unsigned)o_group1; head.nq = nq; head.n_sets = n_sets;
    memcpy(in, &head, sizeof head);
    memcpy(in + o_group1, group1, (size_t)nq * 4);
    for (int i = 0; i < n_sets; ++i) {
        const lpslam_hip_tri_set& st = sets[i];
        TriSetDev& d = dev_sets[(size_t)i];
        memcpy(d.e.F, st.F, sizeof d.e.F);
        d.e.ex = st.has_epipole ? st.epipole[0] : 0.0; d.e.ey = st.has_epipole ? st.epipole[1] : 0.0; d.e.has_epipole = st.has_epipole ? 1 : 0; d.e.pad = 0;
        d.v = tri::view_from_pose(st.pose);
        d.n = st.n; d.pad[0] = d.pad[1] = d.pad[2] = 0;
        GateRec* gr = (GateRec*)(in + d.o_gate); float* xr = (float*)(in + d.o_xr); float* dep = (float*)(in + d.o_depth);
        if (st.n == 0) { gr[0] = GateRec{0.f, 0.f, 0, -1}; xr[0] = -1.f; dep[0] = -1.f; memset(in + d.o_desc, 0, 32); }
        for (int j = 0; j < st.n; ++j) {
            const float depth = st.depth ? st.depth[j] : -1.0f;
            gr[j] = GateRec{st.kpts[j].x, st.kpts[j].y, st.kpts[j].octave | (tri::is_stereo(camera, depth) ? 256 : 0), st.group[j]};
            xr[j] = st.x_right ? st.x_right[j] : -1.0f; dep[j] = depth;
        }
        if (st.n) memcpy(in + d.o_desc, st.desc32, (size_t)st.n * 32);
        memcpy(in + o_sets + (size_t)i * sizeof(TriSetDev), &d, sizeof d);
    }
    const double tr_staged = tr.us();
    const size_t o = (size_t)image * c->slots_per_image;
    const lpslam_hip_keypoint* kp1 = c->d_kpts + o;
    const float* xr1 = camera.fxb > 0.0 ? c->d_stereo + o * 2 : nullptr;            // the slot's last stereo match
    const float* depth1 = xr1 ? xr1 + c->slots_per_image : nullptr;
    if (int rc = call.upload(o_in, in_bytes)) return rc;
    unsigned long long* d_keys = (unsigned long long*)(base + d_keys_off); int* d_cnt = (int*)(base + d_cnt_off);
    hipLaunchKernelGGL(k_epi_topk, dim3((unsigned)((nq + 3) / 4), (unsigned)n_sets), dim3(256), 0, s, (const uint8_t*)base, kp1, (const uint8_t*)(c->d_desc + o * 32), depth1, d_keys, d_cnt);
    hipLaunchKernelGGL(k_tri_pairs, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, (const uint8_t*)base, kp1, xr1, depth1, (const unsigned long long*)d_keys, (const int*)d_cnt,
                       (int*)(hb + h_cnt_off), (unsigned long long*)(hb + h_keys_off), (int*)(hb + h_code_off), (double*)(hb + h_X_off), call.done.counter, call.done.flag, call.done.seq);
    if (int rc = call.finish()) return rc;
    const double tr_back = tr.us();
    const int* h_cnt = (const int*)(hb + h_cnt_off); const unsigned long long* h_keys = (const unsigned long long*)(hb + h_keys_off);
    const int* h_code = (const int*)(hb + h_code_off); const double* h_X = (const double*)(hb + h_X_off);
    for (int i = 0; i < n_sets; ++i)
        for (int q = 0; q < nq; ++q) {
            const size_t oq = (size_t)i * (size_t)nq + (size_t)q, dst = ((size_t)i * (size_t)capacity + (size_t)q) * tri::kListed;
            const int cnt = h_cnt[oq];
            out_count[(size_t)i * (size_t)capacity + (size_t)q] = cnt;
            for (int r = 0; r < tri::kListed; ++r) {
                const size_t ent = oq * tri::kListed + (size_t)r;
                const bool listed = r < cnt && h_keys[ent] != NONE;
                out_j[dst + r] = listed ? (int32_t)(h_keys[ent] & 0xffffffffu) : -1;
                out_dist[dst + r] = listed ? (int32_t)(h_keys[ent] >> 32) : 256;
                const int code = listed ? h_code[ent] : 0;
                out_code[dst + r] = code;
                for (int a = 0; a < 3; ++a) out_X[3 * (dst + r) + a] = code ? h_X[3 * ent + a] : (double)NAN;
            }
        }
    if (tr.on()) fprintf(stderr, "triangulate_neighbours: %d queries, %d neighbours; us: staged %.1f, results back %.1f, unpacked %.1f\n", nq, n_sets, tr_staged, tr_back, tr.us());
    return LPSLAM_HIP_OK;
}

int lpslam_hip_triangulate_pairs(lpslam_hip_ctx* c, const lpslam_hip_tri_camera* cam, const float* scale, int32_t n_levels, const double* pose1, const double* pose2,
                                 const lpslam_hip_tri_keypoint* kp1, const lpslam_hip_tri_keypoint* kp2, int32_t n, int32_t* code, double* X)
{
    if (!c) { set_error("null context"); return LPSLAM_HIP_ERR_INVALID; }
    if (!cam || !scale || !pose1 || !pose2 || n < 0 || (n && (!kp1 || !kp2 || !code || !X))) { set_error("triangulate_pairs: null argument or negative count"); return LPSLAM_HIP_ERR_INVALID; }
    if (n_levels < 1 || n_levels > LPSLAM_HIP_MAX_LEVELS || !camera_ok(cam) || !pose_ok(pose1) || !pose_ok(pose2)) { set_error("triangulate_pairs: camera, pose or level count is not usable"); return LPSLAM_HIP_ERR_INVALID; }
    for (int i = 0; i < n; ++i) if (kp1[i].octave < 0 || kp1[i].octave >= n_levels || kp2[i].octave < 0 || kp2[i].octave >= n_levels) { set_error("triangulate_pairs: pair %d: octave outside the scale table", i); return LPSLAM_HIP_ERR_INVALID; }
    if (n == 0) return LPSLAM_HIP_OK;
    LP_HIP(hipSetDevice(c->cfg.device));
    static_assert(sizeof(lpslam_hip_tri_keypoint) == sizeof(tri::Keypoint), "keypoint layout");
    // one block of the cache: keypoints of view 1 | of view 2 | scale table | X | codes
    LpLayout lay;
    lay.take((size_t)n * sizeof(tri::Keypoint));
    const size_t kb = lay.take((size_t)n * sizeof(tri::Keypoint)), o_scale = lay.take(sizeof(PairsHead::scale)), o_X = lay.take((size_t)n * 24), o_code = lay.at;
    LpPoolBlock blk(c);
    if (int rc = blk.alloc(o_code + (size_t)n * 4)) return rc;
    uint8_t* base = (uint8_t*)blk.ptr;
    PairsHead head{};
    head.cam = to_camera(cam); head.v1 = tri::view_from_pose(pose1); head.v2 = tri::view_from_pose(pose2);
    fill_scale(head.scale, scale, n_levels);
    hipStream_t s = c->stream;
    LP_HIP(hipMemcpyAsync(base, kp1, (size_t)n * sizeof(tri::Keypoint), hipMemcpyHostToDevice, s));
    LP_HIP(hipMemcpyAsync(base + kb, kp2, (size_t)n * sizeof(tri::Keypoint), hipMemcpyHostToDevice, s));
    LP_HIP(hipMemcpyAsync(base + o_scale, head.scale, sizeof head.scale, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tri_pair_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, head, (const tri::Keypoint*)base, (const tri::Keypoint*)(base + kb), n,
                       (const float*)(base + o_scale), (int32_t*)(base + o_code), (double*)(base + o_X));
    LP_HIP(hipGetLastError());
    LP_HIP(hipMemcpyAsync(X, base + o_X, (size_t)n * 24, hipMemcpyDeviceToHost, s));
    LP_HIP(hipMemcpyAsync(code, base + o_code, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    const hipError_t err = hipStreamSynchronize(s);
    if (err != hipSuccess) { blk.leak(); return hip_fail(err, "triangulate_pairs"); }
    return LPSLAM_HIP_OK;
}

}  // extern "C"
