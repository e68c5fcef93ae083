// monoinit.hip — the two-view geometry of MapInitialization::InitializeWithFrames on MI355X (gfx950).
//
// The reference (Core/MAGESLAM/Source/Tracking/MapInitialization.cpp:988-1094) collects the matches'
// points, runs FindPossiblePoses — 90 RANSAC iterations of a five-point solve, each of up to ten
// essential matrices scored over all matches and gated by cheirality — and hands the winner's four
// poses to FindCorrectPose.  Here that is a chain of launches on one stream, batched over frame
// pairs, with no host step:
//   mono_mask_kernel    (with descriptors) the octave-0 masks of :562-583 for both frames, the
//                       masked descriptors packed in keypoint order with their keypoint indices —
//                       the two sides the two-way matcher (match.hip) then reads;
//   mono_sample_kernel  one workgroup per pair: the matcher's indices back to keypoints, the limits
//                       and index checks, the result record, the match points staged in LDS and one
//                       lane running the serial sampler (one generator for all iterations);
//   mono_solve_kernel   one hypothesis per thread, 64 per workgroup; the 10 x 20 matrix and the
//                       fp64 work arrays lane-interleaved in LDS (bank-conflict free, no scratch
//                       for the runtime-indexed arrays);
//   mono_score_kernel   one lane per candidate essential matrix: the pair's match points staged in
//                       LDS and walked in match order by every lane (same address: a broadcast), so
//                       the in-order float sum costs nothing; the cheirality check on the same lane;
//   mono_pose_kernel    one workgroup per pair: the winner (maximum score among the consistent
//                       candidates, the earliest on ties), its four poses, a lane per match for
//                       FindCorrectPose's triangulation and flags, one lane's in-order score sum, the
//                       median through lds_sort.hpp, the verdict, and for MAGE_MI_OK the accepted
//                       matches compacted in match order with the bundle adjustment's inputs.
// All arithmetic is monoinit_math.hpp's, shared with the twin (monoinit.cpp).  No atomics; nothing
// depends on the order in which threads run; all loops are bounded by the counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "lds_sort.hpp"
#include "monoinit_math.hpp"
#include "ordered_take.hpp"

namespace mage {
namespace {

using namespace monoinit;

// The host-buffer entry's scratch slot, after stereoinit.hip's 7.
constexpr ScratchSlot SCRATCH_MONOINIT = static_cast<ScratchSlot>(8);

constexpr int MI_THREADS = 256;
constexpr int MI_WAVES = MI_THREADS / kWave;
constexpr int MI_SOLVE_THREADS = 64;
constexpr int MI_POSE_THREADS = SORT_THREADS;

struct MiParams {
    Consts c;
    TraceLayout L;
    const float* intr4;
    const mage_keypoint *kp0, *kp1;
    const uint8_t *desc0, *desc1;
    long long pitch0, pitch1;
    const uint32_t *n0, *n1;
    mage_dmatch* matches;
    uint32_t match_cap;
    const uint32_t* n_matches;
    mage_mono_init_result* result;
    mage_stereo_point* out;
    uint32_t cap;
    float *ba_points, *ba_uv;
    uint32_t *ba_cam, *ba_pt;
    float* ba_info;
    char* work;                // pairs x L.bytes: the trace, or the scratch's first part
    uint8_t *pack0, *pack1;    // masked descriptors in keypoint order; null when the matches are given
    uint32_t *pidx0, *pidx1;   // their keypoint indices
    uint32_t* n_masked;        // [2 pairs]: frame 0's counts, then frame 1's
};

struct Trace {
    int32_t *idx, *ncand;
    float *E, *score;
    uint32_t *inliers, *cheir;
};

__device__ __forceinline__ Trace trace_of(const MiParams& p, int pr)
{
    char* b = p.work + (size_t)pr * p.L.bytes;
    return Trace{reinterpret_cast<int32_t*>(b + p.L.idx),   reinterpret_cast<int32_t*>(b + p.L.ncand),
                 reinterpret_cast<float*>(b + p.L.E),       reinterpret_cast<float*>(b + p.L.score),
                 reinterpret_cast<uint32_t*>(b + p.L.inliers), reinterpret_cast<uint32_t*>(b + p.L.cheir)};
}

__device__ __forceinline__ bool over_limit(const MiParams& p, uint32_t n0, uint32_t n1)
{
    return n0 > (uint32_t)MI_MAX_KP || n1 > (uint32_t)MI_MAX_KP || (long long)n0 > p.pitch0 || (long long)n1 > p.pitch1;
}

// Match m's points; the indices were checked by mono_sample_kernel.
__device__ __forceinline__ Pt4 match_point(const MiParams& p, int pr, uint32_t m)
{
    const mage_dmatch d = p.matches[(long long)pr * p.match_cap + m];
    const mage_keypoint& a = p.kp0[pr * p.pitch0 + d.query_idx];
    const mage_keypoint& b = p.kp1[pr * p.pitch1 + d.train_idx];
    return Pt4{a.x, a.y, b.x, b.y};
}

// A pair the later kernels skip: stopped by mono_sample_kernel (its result record says why).
__device__ __forceinline__ bool stopped(const MiParams& p, int pr)
{
    const mage_mono_init_result& r = p.result[pr];
    return (r.status & (MI_STATUS_OVER_LIMIT | MI_STATUS_BAD_INDEX)) != 0 || r.verdict != MI_OK;
}

// grid (pairs, 2): frame blockIdx.y's octave-0 mask, packed descriptors and indices.
__global__ __launch_bounds__(MI_THREADS) void mono_mask_kernel(MiParams p)
{
    __shared__ uint32_t s_wsum[MI_WAVES];
    const int pr = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const uint32_t n0 = p.n0[pr], n1 = p.n1[pr];
    uint32_t* n_masked = p.n_masked + (size_t)f * gridDim.x + pr;
    if (over_limit(p, n0, n1)) {  // uniform over the workgroup
        if (tid == 0) *n_masked = 0;
        return;
    }
    const uint32_t n = f ? n1 : n0;
    const long long row = pr * (f ? p.pitch1 : p.pitch0);
    const mage_keypoint* kp = (f ? p.kp1 : p.kp0) + row;
    const uint8_t* desc = (f ? p.desc1 : p.desc0) + 32 * row;
    uint8_t* pack = (f ? p.pack1 : p.pack0) + 32 * row;
    uint32_t* pidx = (f ? p.pidx1 : p.pidx0) + row;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += MI_THREADS) {
        const uint32_t i = c0 + tid;
        const bool in = i < n && kp[i].octave == 0;
        uint32_t total;
        const uint32_t pos = base + block_prefix<MI_WAVES>(in, s_wsum, &total);  // pos < n <= pitch
        if (in) {
            const uint4* src = reinterpret_cast<const uint4*>(desc + 32ull * i);
            uint4* dst = reinterpret_cast<uint4*>(pack + 32ull * pos);
            dst[0] = src[0];
            dst[1] = src[1];
            pidx[pos] = i;
        }
        base += total;
    }
    if (tid == 0) *n_masked = base;
}

__global__ __launch_bounds__(MI_THREADS) void mono_sample_kernel(MiParams p)
{
    __shared__ Pt4 s_pts[MI_MAX_MATCHES];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const uint32_t n0 = p.n0[pr], n1 = p.n1[pr], nm = p.n_matches[pr];
    const bool over = over_limit(p, n0, n1) || nm > p.match_cap || nm > (uint32_t)MI_MAX_MATCHES;
    int bad = 0;
    if (!over) {
        mage_dmatch* mm = p.matches + (long long)pr * p.match_cap;
        const uint32_t m0 = p.pidx0 ? p.n_masked[pr] : 0u, m1 = p.pidx0 ? p.n_masked[gridDim.x + pr] : 0u;
        for (uint32_t m = tid; m < nm; m += MI_THREADS) {
            int q = mm[m].query_idx, t = mm[m].train_idx;
            if (p.pidx0) {  // the matcher counted the masked keypoints: back to the frames' indices
                q = q >= 0 && (uint32_t)q < m0 ? (int)p.pidx0[pr * p.pitch0 + q] : -1;
                t = t >= 0 && (uint32_t)t < m1 ? (int)p.pidx1[pr * p.pitch1 + t] : -1;
                mm[m].query_idx = q;
                mm[m].train_idx = t;
            }
            if (q < 0 || (uint32_t)q >= n0 || t < 0 || (uint32_t)t >= n1) bad = 1;
        }
    }
    bad = __syncthreads_or(bad);  // also orders the index stores before match_point's loads
    const uint32_t status = over ? MI_STATUS_OVER_LIMIT : (bad ? MI_STATUS_BAD_INDEX : 0u);
    const bool few = status == 0 && nm < p.c.min_matches;
    if (tid == 0) {
        mage_mono_init_result R{};
        R.win_iteration = R.win_root = R.selected_pose = -1;
        R.r9[0] = R.r9[4] = R.r9[8] = R.r9[9] = R.r9[13] = R.r9[17] = 1.f;
        R.n_matches = nm;
        R.status = status;
        R.verdict = few ? MI_FEW_MATCHES : MI_OK;
        p.result[pr] = R;
    }
    if (status != 0 || few) return;  // uniform over the workgroup
    for (uint32_t m = tid; m < nm; m += MI_THREADS) s_pts[m] = match_point(p, pr, m);
    __syncthreads();
    if (tid == 0) {
        const Pt4* pts = s_pts;
        sample_indices([pts](int m) { return pts[m]; }, nm, p.c.iters, p.c.min_spread_sq, trace_of(p, pr).idx);
    }
}

// grid (pairs, ceil(iters / 64)): one hypothesis per thread.
__global__ __launch_bounds__(MI_SOLVE_THREADS) void mono_solve_kernel(MiParams p)
{
    __shared__ double s_d[MI_WORK_D * MI_SOLVE_THREADS];
    __shared__ float s_a[MI_WORK_A * MI_SOLVE_THREADS];
    const int pr = blockIdx.x, tid = threadIdx.x;
    if (stopped(p, pr)) return;
    const uint32_t it = blockIdx.y * MI_SOLVE_THREADS + tid;
    if (it >= p.c.iters) return;
    const Trace T = trace_of(p, pr);
    float* E = T.E + 90ull * it;
    int cnt = 0;
    if (T.idx[5 * it] >= 0) {
        Pt4 p5[5];
        for (int k = 0; k < 5; k++) p5[k] = match_point(p, pr, (uint32_t)T.idx[5 * it + k]);
        const float* intr = p.intr4 + 8ll * pr;
        cnt = solve_five_point(p5, intr[0], intr[1], intr[2], intr[3], Strided<double>{s_d + tid, MI_SOLVE_THREADS},
                               Strided<float>{s_a + tid, MI_SOLVE_THREADS}, E);
    } else {
        for (int k = 0; k < 90; k++) E[k] = 0.f;
    }
    T.ncand[it] = cnt;
}

// grid (pairs, ceil(10 iters / 256)): one candidate per thread.
__global__ __launch_bounds__(MI_THREADS) void mono_score_kernel(MiParams p)
{
    __shared__ Pt4 s_pts[MI_MAX_MATCHES];
    const int pr = blockIdx.x, tid = threadIdx.x;
    if (stopped(p, pr)) return;
    const uint32_t nm = p.result[pr].n_matches;
    for (uint32_t m = tid; m < nm; m += MI_THREADS) s_pts[m] = match_point(p, pr, m);
    __syncthreads();
    const uint32_t slot = blockIdx.y * MI_THREADS + tid;
    if (slot >= 10 * p.c.iters) return;
    const Trace T = trace_of(p, pr);
    const uint32_t it = slot / 10, r = slot % 10;
    float score = 0.f;
    uint32_t inliers = 0, cheir = 0;
    if ((int)r < T.ncand[it]) {
        const float* intr = p.intr4 + 8ll * pr;
        Frame f0, k1;
        identity_frame(intr, f0);
        identity_frame(intr + 4, k1);
        const float* E = T.E + 90ull * it + 9 * r;
        float F12[9], F21[9];
        fundamental_from_essential(E, f0.Kinv, k1.Kinv, F12, F21);
        ScoreState s{0.f, 0};
        for (uint32_t m = 0; m < nm; m++) score_match(F12, F21, p.c.threshold, s_pts[m], s);
        score = score_gate(p.c, s, nm);
        inliers = s.inliers;
        float pos3[12], r9[36];
        decompose_poses(E, pos3, r9);
        Pt4 p5[5];
        for (int k = 0; k < 5; k++) p5[k] = s_pts[T.idx[5 * it + k]];
        cheir = consistent_cheirality(pos3, r9, f0, intr + 4, p5) ? 1u : 0u;
    }
    T.score[slot] = score;
    T.inliers[slot] = inliers;
    T.cheir[slot] = cheir;
}

__device__ __forceinline__ uint32_t next_pow2(uint32_t v)
{
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

__global__ __launch_bounds__(MI_POSE_THREADS) void mono_pose_kernel(MiParams p)
{
    __shared__ unsigned long long s_keys[MI_MAX_MATCHES];
    __shared__ float s_term[MI_MAX_MATCHES];
    __shared__ uint32_t s_wsum[MI_POSE_THREADS / kWave];
    __shared__ Frame s_f0;
    __shared__ PoseEval s_pe[4];
    __shared__ mage_mono_init_result s_r;
    __shared__ float s_cam_z[4];
    const int pr = blockIdx.x, tid = threadIdx.x;
    if (stopped(p, pr)) return;
    const Trace T = trace_of(p, pr);
    const uint32_t nm = p.result[pr].n_matches;
    const float* intr = p.intr4 + 8ll * pr;

    // the winner: the maximum score among the consistent candidates, the earliest on ties — what
    // the sequential "strictly better and consistent replaces" rule (:263-269) leaves
    unsigned long long key = 0ull;
    for (uint32_t slot = tid; slot < 10 * p.c.iters; slot += MI_POSE_THREADS) {
        const float sc = T.score[slot];
        if (T.cheir[slot] && sc > 0.f) {
            const unsigned long long k = ((unsigned long long)__float_as_uint(sc) << 32) | (0xFFFFFFFFu - slot);
            key = k > key ? k : key;
        }
    }
    s_keys[tid] = key;
    __syncthreads();
    for (int s = MI_POSE_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) s_keys[tid] = s_keys[tid] > s_keys[tid + s] ? s_keys[tid] : s_keys[tid + s];
        __syncthreads();
    }
    const unsigned long long win = s_keys[0];
    __syncthreads();
    if (win == 0ull) {  // uniform over the workgroup
        if (tid == 0) p.result[pr].verdict = MI_NO_HYPOTHESIS;
        return;
    }
    const uint32_t wslot = 0xFFFFFFFFu - (uint32_t)win;
    if (tid == 0) {
        s_r = p.result[pr];
        s_r.win_iteration = (int32_t)(wslot / 10);
        s_r.win_root = (int32_t)(wslot % 10);
        s_r.win_score = __uint_as_float((uint32_t)(win >> 32));
        for (int k = 0; k < 5; k++) s_r.win_indices[k] = T.idx[5 * (wslot / 10) + k];
        decompose_poses(T.E + 9ull * wslot, s_r.cand_pos3, s_r.cand_r9);
        identity_frame(intr, s_f0);
    }
    __syncthreads();
    if (tid < 4) {
        prepare_pose(s_f0, s_r.cand_pos3 + 3 * tid, s_r.cand_r9 + 9 * tid, intr + 4, s_pe[tid]);
        s_cam_z[tid] = s_pe[tid].f1.C[2];
    }
    __syncthreads();

    // FindCorrectPose's pose loop (:350-450)
    const uint32_t P = next_pow2(nm);
    for (int ps = 0; ps < 4; ps++) {
        if (s_pe[ps].twisted) {  // uniform
            if (tid == 0) s_r.cand_flags[ps] = MI_POSE_TWISTED;
            continue;
        }
        for (uint32_t m = tid; m < P; m += MI_POSE_THREADS) {
            float term = 0.f, X[3] = {0.f, 0.f, 0.f};
            bool parallel;
            if (m < nm) term = eval_match(p.c, s_f0, s_pe[ps], match_point(p, pr, m), X, parallel);
            if (m < nm) s_term[m] = term;
            // accepted depths sort above every rejected match's zero key
            s_keys[m] = term > 0.f ? ((unsigned long long)float_order_key(X[2]) << 32) | __float_as_uint(X[2]) : 0ull;
        }
        __syncthreads();
        if (tid == 0) {  // the score in match order
            float score = 0.f;
            uint32_t count = 0;
            for (uint32_t m = 0; m < nm; m++) {
                const float t = s_term[m];
                if (t > 0.f) {
                    score += t;
                    count++;
                }
            }
            s_r.cand_score[ps] = score;
            s_r.cand_count[ps] = count;
            s_r.cand_flags[ps] = pose_gate(p.c, count, nm);
        }
        __syncthreads();
        if (s_r.cand_flags[ps] & MI_POSE_ENOUGH) {  // uniform
            sort_desc(s_keys, (int)P);
            if (tid == 0) {
                // ascending order statistic count / 2 of the accepted depths = descending count - 1 - count / 2
                const uint32_t count = s_r.cand_count[ps];
                const float median = __uint_as_float((uint32_t)s_keys[count - 1 - count / 2]);
                s_r.cand_median[ps] = median;
                if (median <= p.c.max_median) s_r.cand_flags[ps] |= MI_POSE_MEDIAN_OK;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        s_r.verdict = final_verdict(p.c, s_r.cand_flags, s_r.cand_score, s_cam_z, s_r.selected_pose, s_r.next_best_score);
        if (s_r.verdict == MI_OK) {
            for (int k = 0; k < 3; k++) s_r.pos3[3 + k] = s_r.cand_pos3[3 * s_r.selected_pose + k];
            for (int k = 0; k < 9; k++) s_r.r9[9 + k] = s_r.cand_r9[9 * s_r.selected_pose + k];
        }
    }
    __syncthreads();
    if (s_r.verdict != MI_OK) {  // uniform
        if (tid == 0) p.result[pr] = s_r;
        return;
    }
    // the selected pose's accepted matches compacted in match order
    const int sp = s_r.selected_pose;
    const mage_dmatch* mm = p.matches + (long long)pr * p.match_cap;
    mage_stereo_point* out = p.out + (long long)pr * p.cap;
    uint32_t nacc = 0;
    for (uint32_t c0 = 0; c0 < nm; c0 += MI_POSE_THREADS) {
        const uint32_t m = c0 + tid;
        bool acc = false;
        mage_stereo_point o{};
        if (m < nm) {
            bool parallel;
            acc = eval_match(p.c, s_f0, s_pe[sp], match_point(p, pr, m), o.position, parallel) > 0.f;
            const mage_dmatch d = mm[m];
            o.query_idx = d.query_idx;
            o.train_idx = d.train_idx;
            o.distance = d.distance;
            o.near_parallel = parallel ? 1u : 0u;
        }
        uint32_t total;
        const uint32_t pos = nacc + block_prefix<MI_POSE_THREADS / kWave>(acc, s_wsum, &total);
        if (acc && pos < p.cap) out[pos] = o;
        nacc += total;
    }
    const uint32_t n = min(nacc, p.cap);
    if (tid == 0) {
        s_r.n_points = n;
        if (nacc > p.cap) s_r.status |= MI_STATUS_OVER_CAP;
        p.result[pr] = s_r;
    }
    // the bundler's inputs from the compacted records (this workgroup's own stores, visible after
    // the barrier): the points, then frame 0's observations, then frame 1's
    __syncthreads();
    const float info = track::refinement_confidence(1);
    float* bp = p.ba_points + 3ll * pr * p.cap;
    const long long ob = 2ll * pr * p.cap;
    const mage_keypoint* kp0 = p.kp0 + pr * p.pitch0;
    const mage_keypoint* kp1 = p.kp1 + pr * p.pitch1;
    for (uint32_t i = tid; i < n; i += MI_POSE_THREADS) {
        const mage_stereo_point r = out[i];
        for (int k = 0; k < 3; k++) bp[3 * i + k] = r.position[k];
        const mage_keypoint a = kp0[r.query_idx], b = kp1[r.train_idx];
        const long long o0 = ob + i, o1 = ob + n + i;
        p.ba_uv[2 * o0] = a.x;
        p.ba_uv[2 * o0 + 1] = a.y;
        p.ba_uv[2 * o1] = b.x;
        p.ba_uv[2 * o1 + 1] = b.y;
        p.ba_cam[o0] = 0u;
        p.ba_cam[o1] = 1u;
        p.ba_pt[o0] = i;
        p.ba_pt[o1] = i;
        p.ba_info[o0] = info;
        p.ba_info[o1] = info;
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct ScratchLayout {
    size_t work, n_masked, pack0, pack1, pidx0, pidx1, bytes;
};

ScratchLayout scratch_layout(uint32_t iters, uint32_t pairs, int64_t pitch0, int64_t pitch1, bool with_trace, bool with_matcher)
{
    ScratchLayout s{};
    s.work = 0;
    size_t at = with_trace ? 0 : align256((size_t)pairs * trace_layout(iters).bytes);
    if (with_matcher) {
        s.n_masked = at;
        at = align256(at + 8ull * pairs);
        s.pack0 = at;
        at = align256(at + 32ull * pairs * (size_t)pitch0);
        s.pack1 = at;
        at = align256(at + 32ull * pairs * (size_t)pitch1);
        s.pidx0 = at;
        at = align256(at + 4ull * pairs * (size_t)pitch0);
        s.pidx1 = at;
        at = align256(at + 4ull * pairs * (size_t)pitch1);
    }
    s.bytes = at;
    return s;
}

}  // namespace
}  // namespace mage

extern "C" uint64_t mage_mono_init_scratch_bytes(uint32_t iterations, uint32_t pairs, int64_t pitch0, int64_t pitch1,
                                                 int32_t with_trace, int32_t with_matcher)
{
    if (pitch0 < 0 || pitch1 < 0) return 0;
    return mage::scratch_layout(iterations, pairs, pitch0, pitch1, with_trace != 0, with_matcher != 0).bytes;
}

extern "C" mage_status mage_mono_init_two_view_batch_device(
    const mage_mono_init_settings* settings, uint32_t pairs, const float* d_intr4, const mage_keypoint* d_kp0,
    const uint8_t* d_desc0, int64_t pitch0, const uint32_t* d_n0, const mage_keypoint* d_kp1, const uint8_t* d_desc1,
    int64_t pitch1, const uint32_t* d_n1, mage_dmatch* d_matches, uint32_t match_cap, uint32_t* d_n_matches,
    mage_mono_init_result* d_result, mage_stereo_point* d_out, uint32_t cap, float* d_ba_points, float* d_ba_uv,
    uint32_t* d_ba_cam, uint32_t* d_ba_pt, float* d_ba_info, void* d_trace, void* d_scratch, mage_stream stream)
{
    using namespace mage;
    const char* why = monoinit::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    if (pairs == 0) return MAGE_OK;
    MAGE_REQUIRE(d_intr4 && d_kp0 && d_n0 && d_kp1 && d_n1 && d_matches && d_n_matches && d_result && d_out &&
                     d_ba_points && d_ba_uv && d_ba_cam && d_ba_pt && d_ba_info,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE((d_desc0 == nullptr) == (d_desc1 == nullptr), MAGE_EINVAL, "the matcher needs both descriptor sets");
    MAGE_REQUIRE(pitch0 > 0 && pitch1 > 0 && match_cap > 0 && cap > 0, MAGE_EINVAL,
                 "pitches and capacities must be positive");
    const bool match = d_desc0 != nullptr;
    const ScratchLayout S =
        scratch_layout(settings->ransac_iterations_for_models, pairs, pitch0, pitch1, d_trace != nullptr, match);
    MAGE_REQUIRE(S.bytes == 0 || d_scratch, MAGE_EINVAL, "null scratch");
    MAGE_REQUIRE(!match || (((uintptr_t)d_desc0 | (uintptr_t)d_desc1 | (uintptr_t)d_scratch) & 15) == 0, MAGE_EINVAL,
                 "descriptors and scratch must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    MiParams p{};
    p.c = monoinit::make_consts(*settings);
    p.L = monoinit::trace_layout(p.c.iters);
    p.intr4 = d_intr4;
    p.kp0 = d_kp0;
    p.kp1 = d_kp1;
    p.desc0 = d_desc0;
    p.desc1 = d_desc1;
    p.pitch0 = pitch0;
    p.pitch1 = pitch1;
    p.n0 = d_n0;
    p.n1 = d_n1;
    p.matches = d_matches;
    p.match_cap = match_cap;
    p.n_matches = d_n_matches;
    p.result = d_result;
    p.out = d_out;
    p.cap = cap;
    p.ba_points = d_ba_points;
    p.ba_uv = d_ba_uv;
    p.ba_cam = d_ba_cam;
    p.ba_pt = d_ba_pt;
    p.ba_info = d_ba_info;
    char* sb = static_cast<char*>(d_scratch);
    p.work = d_trace ? static_cast<char*>(d_trace) : sb + S.work;
    if (match) {
        p.n_masked = reinterpret_cast<uint32_t*>(sb + S.n_masked);
        p.pack0 = reinterpret_cast<uint8_t*>(sb + S.pack0);
        p.pack1 = reinterpret_cast<uint8_t*>(sb + S.pack1);
        p.pidx0 = reinterpret_cast<uint32_t*>(sb + S.pidx0);
        p.pidx1 = reinterpret_cast<uint32_t*>(sb + S.pidx1);
        launch("monoinit.mask", mono_mask_kernel, dim3(pairs, 2), dim3(MI_THREADS), 0, st, p);
        MAGE_HIP(hipGetLastError());
        const mage_status r = mage_hamming_match_batch_device(
            p.pack0, 32 * pitch0, p.n_masked, p.pack1, 32 * pitch1, p.n_masked + pairs, pairs,
            settings->five_point_max_hamming_distance, settings->five_point_min_hamming_difference, d_matches, match_cap,
            d_n_matches, stream);
        if (r != MAGE_OK) return r;
    }
    const uint32_t iters = p.c.iters;
    launch("monoinit.sample", mono_sample_kernel, dim3(pairs), dim3(MI_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    launch("monoinit.solve", mono_solve_kernel, dim3(pairs, (iters + MI_SOLVE_THREADS - 1) / MI_SOLVE_THREADS),
           dim3(MI_SOLVE_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    launch("monoinit.score", mono_score_kernel, dim3(pairs, (10 * iters + MI_THREADS - 1) / MI_THREADS), dim3(MI_THREADS), 0,
           st, p);
    MAGE_HIP(hipGetLastError());
    launch("monoinit.pose", mono_pose_kernel, dim3(pairs), dim3(MI_POSE_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

extern "C" mage_status mage_mono_init_two_view(const mage_mono_init_settings* settings, const float* intr4,
                                               const mage_keypoint* kp0, const uint8_t* desc0, uint32_t n0,
                                               const mage_keypoint* kp1, const uint8_t* desc1, uint32_t n1,
                                               mage_dmatch* matches, uint32_t match_cap, uint32_t* n_matches,
                                               mage_mono_init_result* result, mage_stereo_point* out, uint32_t cap,
                                               float* ba_points, float* ba_uv, uint32_t* ba_cam, uint32_t* ba_pt,
                                               float* ba_info, void* trace, int device)
{
    using namespace mage;
    const char* why = monoinit::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(intr4 && n_matches && result, MAGE_EINVAL, "null argument");
    const bool match = desc0 != nullptr;
    MAGE_REQUIRE(!match || (desc1 && match_cap > 0), MAGE_EINVAL,
                 "the matcher needs both descriptor sets and room for a match");
    const uint32_t n_in = match ? 0u : *n_matches;
    MAGE_REQUIRE(n_in <= match_cap, MAGE_EINVAL, "more matches than match_cap");
    MAGE_REQUIRE((n0 == 0 || kp0) && (n1 == 0 || kp1) && (match_cap == 0 || matches) &&
                     (cap == 0 || (out && ba_points && ba_uv && ba_cam && ba_pt && ba_info)),
                 MAGE_EINVAL, "null argument");
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    if (n0 > (uint32_t)monoinit::MI_MAX_KP || n1 > (uint32_t)monoinit::MI_MAX_KP) {  // nothing else is written
        mage_mono_init_result R{};
        R.win_iteration = R.win_root = R.selected_pose = -1;
        R.r9[0] = R.r9[4] = R.r9[8] = R.r9[9] = R.r9[13] = R.r9[17] = 1.f;
        R.n_matches = n_in;
        R.status = monoinit::MI_STATUS_OVER_LIMIT;
        *result = R;
        return MAGE_OK;
    }
    HostScratch* sp = host_scratch(device, SCRATCH_MONOINIT);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [intr][kp0][kp1][desc0][desc1][counts][matches] | [result][records][ba points, uv,
    // cam, pt, info][trace] | [scratch]: the inputs in one H2D copy, matches to trace back in one D2H copy
    const uint32_t iters = settings->ransac_iterations_for_models;
    const size_t tbytes = monoinit::trace_layout(iters).bytes;
    const uint32_t p0 = std::max(n0, 1u), p1 = std::max(n1, 1u), mc = std::max(match_cap, 1u), dcap = std::max(cap, 1u);
    const size_t sbytes = scratch_layout(iters, 1, p0, p1, true, match).bytes;
    const size_t ointr = 0, okp0 = align256(ointr + 32), okp1 = align256(okp0 + 28ull * p0),
                 od0 = align256(okp1 + 28ull * p1), od1 = align256(od0 + 32ull * p0), ocnt = align256(od1 + 32ull * p1),
                 omat = align256(ocnt + 4 * 3), ores = align256(omat + 16ull * mc),
                 oout = align256(ores + sizeof(mage_mono_init_result)),
                 obp = align256(oout + sizeof(mage_stereo_point) * (size_t)dcap), ouv = align256(obp + 12ull * dcap),
                 ocam = align256(ouv + 16ull * dcap), opt = align256(ocam + 8ull * dcap),
                 oinfo = align256(opt + 8ull * dcap), otr = align256(oinfo + 8ull * dcap),
                 oscr = align256(otr + tbytes), total = align256(oscr + sbytes);
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(oscr)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    std::memset(h, 0, ores);
    std::memcpy(h + ointr, intr4, 32);
    if (n0) std::memcpy(h + okp0, kp0, 28ull * n0);
    if (n1) std::memcpy(h + okp1, kp1, 28ull * n1);
    if (match && n0) std::memcpy(h + od0, desc0, 32ull * n0);
    if (match && n1) std::memcpy(h + od1, desc1, 32ull * n1);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(h + ocnt);  // n0, n1, n_matches
    cnt[0] = n0;
    cnt[1] = n1;
    cnt[2] = n_in;
    if (n_in) std::memcpy(h + omat, matches, 16ull * n_in);
    MAGE_HIP(hipMemcpyAsync(b, h, ores, hipMemcpyHostToDevice, S.st));
    uint32_t* dc = reinterpret_cast<uint32_t*>(b + ocnt);
    r = mage_mono_init_two_view_batch_device(
        settings, 1, reinterpret_cast<const float*>(b + ointr), reinterpret_cast<const mage_keypoint*>(b + okp0),
        match ? reinterpret_cast<const uint8_t*>(b + od0) : nullptr, p0, dc,
        reinterpret_cast<const mage_keypoint*>(b + okp1), match ? reinterpret_cast<const uint8_t*>(b + od1) : nullptr, p1,
        dc + 1, reinterpret_cast<mage_dmatch*>(b + omat), mc, dc + 2, reinterpret_cast<mage_mono_init_result*>(b + ores),
        reinterpret_cast<mage_stereo_point*>(b + oout), dcap, reinterpret_cast<float*>(b + obp),
        reinterpret_cast<float*>(b + ouv), reinterpret_cast<uint32_t*>(b + ocam), reinterpret_cast<uint32_t*>(b + opt),
        reinterpret_cast<float*>(b + oinfo), b + otr, sbytes ? b + oscr : nullptr, S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + ocnt, b + ocnt, oscr - ocnt, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    const mage_mono_init_result* R = reinterpret_cast<const mage_mono_init_result*>(h + ores);
    *result = *R;
    if (match) {
        const uint32_t nm = std::min(cnt[2], match_cap);
        *n_matches = nm;
        if (nm) std::memcpy(matches, h + omat, 16ull * nm);
    }
    const bool ran = (R->status & (monoinit::MI_STATUS_OVER_LIMIT | monoinit::MI_STATUS_BAD_INDEX)) == 0 &&
                     R->verdict != monoinit::MI_FEW_MATCHES;
    if (trace && ran) std::memcpy(trace, h + otr, tbytes);
    // cap == 0 ran with one spare record: every accepted match is then over the capacity
    const uint32_t n = cap ? R->n_points : 0;
    if (cap == 0 && R->n_points > 0) {
        result->n_points = 0;
        result->status |= monoinit::MI_STATUS_OVER_CAP;
    }
    if (n) {
        std::memcpy(out, h + oout, sizeof(mage_stereo_point) * (size_t)n);
        std::memcpy(ba_points, h + obp, 12ull * n);
        std::memcpy(ba_uv, h + ouv, 16ull * n);
        std::memcpy(ba_cam, h + ocam, 8ull * n);
        std::memcpy(ba_pt, h + opt, 8ull * n);
        std::memcpy(ba_info, h + oinfo, 8ull * n);
    }
    return MAGE_OK;
}
