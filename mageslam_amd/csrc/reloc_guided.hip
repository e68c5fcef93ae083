// reloc_guided.hip — the rest of PoseEstimator::TryEstimatePoseFromCandidates behind PNPRansac
// (Core/MAGESLAM/Source/Tracking/PoseEstimator.cpp:346-436) on MI355X (gfx950), batched over (lost
// frame, candidate keyframe) problems laid out frames x candidates: a chain of launches on one
// stream behind mage_reloc_pnp_batch_device, no host step:
//   pose BA 1             mage_ba_pose_batch_device on the PnP stage's arrays, as it is (:346);
//   reloc_query_kernel    one workgroup per problem: the limits, order and frame checks, the
//                         candidate's associations projected through the refined pose in the given
//                         order, several passes of the workgroup when there are more than its
//                         threads, those with Distance >= 0 compacted in order into the radius
//                         matcher's query layout (:351-371);
//   radius match          mage_radius_match_batch_device, as it is (:376-389);
//   reloc_gate_kernel     one workgroup per problem: the MinRadiusMatchCorrespondences gate (:391),
//                         the matches in query order as association records without the map points
//                         behind the camera (:396-405), the MinMapPoints gate (:406), the count
//                         that reaches the second bundle adjustment;
//   reloc_gpack_kernel    one workgroup per problem: its place in obs_start (the prefix of those
//                         counts, known only once every problem's gate has run: hence its own
//                         launch) and the second bundle adjustment's inputs gathered there;
//   pose BA 2             mage_ba_pose_batch_device with outlier flags (:419);
//   reloc_decide_kernel   one workgroup per frame: each candidate's outlier count, the
//                         BundleAdjustInliersPctRequired gate (:422), its result record; then the
//                         frame's record, the lowest candidate index that succeeded.
// All arithmetic is reloc_guided_math.hpp's, shared with the twin (reloc_guided.cpp).  No atomics;
// nothing depends on the order in which threads run; all loops are bounded by the counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "ordered_take.hpp"
#include "reloc_guided_math.hpp"

namespace mage {
namespace {

using namespace relocguided;

// The host-buffer entry's scratch slot, after reloc_pnp.hip's 10.
constexpr ScratchSlot SCRATCH_RELOCGUIDED = static_cast<ScratchSlot>(11);

constexpr int RG_THREADS = 256;
constexpr int RG_WAVES = RG_THREADS / kWave;

struct RgParams {
    Consts c;
    mage_reloc_guided_args a;
    uint32_t problems;
    float *pos1, *r91, *pos2, *r92;  // per problem: the poses the two bundle adjustments leave
    uint32_t* count2;                // per problem: the observations that reach the second
};

__global__ __launch_bounds__(RG_THREADS) void reloc_query_kernel(RgParams p)
{
    __shared__ uint32_t s_wsum[RG_WAVES];
    __shared__ float s_pose[16];
    const mage_reloc_guided_args& a = p.a;
    const int pr = blockIdx.x, tid = threadIdx.x;
    const uint32_t frame = (uint32_t)pr / a.candidates_per_frame, cand = (uint32_t)pr % a.candidates_per_frame;
    const bool present = cand < (a.d_n_candidates ? a.d_n_candidates[frame] : a.candidates_per_frame);
    const uint32_t nkf = a.d_n_kf[pr], nkp = a.d_n_kp[pr];
    const bool ordered = a.d_order != nullptr;
    const uint32_t nord = ordered ? a.d_n_order[pr] : 0u;
    const mage_reloc_pnp_result& pnp = a.d_pnp_result[pr];
    const bool pnp_ok = pnp.verdict == relocpnp::RP_OK &&
                        (pnp.status & (relocpnp::RP_STATUS_OVER_LIMIT | relocpnp::RP_STATUS_BAD_INDEX)) == 0;
    const bool over = present && over_limit(nkf, a.kf_pitch, nkp, a.kp_pitch, ordered, nord);
    const bool skip = !present || over || !pnp_ok || nkp < p.c.min_frame_kp;  // uniform over the workgroup
    const float* map = a.d_map_xyzi + 4 * pr * a.kf_pitch;
    const int32_t* order = ordered ? a.d_order + pr * a.kf_pitch : nullptr;
    const uint32_t slots = ordered ? nord : nkf;
    int bad = 0;
    if (!skip && ordered)
        for (uint32_t s = tid; s < slots; s += RG_THREADS)
            if (bad_order_entry(order[s], nkf, map)) bad = 1;
    bad = __syncthreads_or(bad);
    if (skip || bad) {
        if (tid == 0) {
            mage_reloc_guided_result R;
            init_result(R);
            R.verdict = RG_SKIPPED;
            R.status = over ? RG_STATUS_OVER_LIMIT : (bad ? RG_STATUS_BAD_ORDER : 0u);
            a.d_result[pr] = R;
            a.d_n_queries[pr] = 0;
        }
        return;
    }
    // the refined pose and the calibration in LDS: every lane reads the same words (a broadcast), and
    // the projection's run-time indexed reads need no per-lane copy
    if (tid < 3) s_pose[tid] = p.pos1[3ll * pr + tid];
    else if (tid < 12) s_pose[tid] = p.r91[9ll * pr + (tid - 3)];
    else if (tid < 16) s_pose[tid] = a.d_intr4[4ll * pr + (tid - 12)];
    __syncthreads();
    const float *pos3 = s_pose, *r9 = s_pose + 3, *intr = s_pose + 12;
    const mage_keypoint* kfkp = a.d_kf_kp + pr * a.kf_pitch;
    const uint4* kfdesc = reinterpret_cast<const uint4*>(a.d_kf_desc + 32 * pr * a.kf_pitch);
    const long long q0 = (long long)pr * a.cap;
    uint4* qdesc = reinterpret_cast<uint4*>(a.d_query_desc + 32 * q0);
    uint32_t n_assoc = 0, nq = 0;
    for (uint32_t s0 = 0; s0 < slots; s0 += RG_THREADS) {  // uniform over the workgroup
        const uint32_t s = s0 + tid;
        const int32_t k = s < slots ? slot_keypoint(order, map, s) : -1;
        float x = 0.f, y = 0.f;
        const bool keep = k >= 0 && predict(pos3, r9, intr, map + 4ll * k, x, y);
        n_assoc += (uint32_t)__syncthreads_count(k >= 0);
        uint32_t total;
        const uint32_t pos = nq + block_prefix<RG_WAVES>(keep, s_wsum, &total);
        if (keep && pos < a.cap) {
            a.d_query_kp[q0 + pos] = kfkp[k];
            a.d_query_pos[2 * (q0 + pos)] = x;
            a.d_query_pos[2 * (q0 + pos) + 1] = y;
            qdesc[2 * pos] = kfdesc[2 * k];
            qdesc[2 * pos + 1] = kfdesc[2 * k + 1];
            a.d_query_ref[q0 + pos] = k;
        }
        nq += total;
    }
    if (tid == 0) {
        mage_reloc_guided_result R;
        init_result(R);
        R.verdict = RG_OK;
        R.n_assoc = n_assoc;
        R.n_queries = min(nq, a.cap);
        if (nq > a.cap) R.status |= RG_STATUS_OVER_CAP;
        for (int k = 0; k < 3; k++) R.pos3_first[k] = pos3[k];
        for (int k = 0; k < 9; k++) R.r9_first[k] = r9[k];
        a.d_result[pr] = R;
        a.d_n_queries[pr] = R.n_queries;
    }
}

__global__ __launch_bounds__(RG_THREADS) void reloc_gate_kernel(RgParams p)
{
    __shared__ uint32_t s_wsum[RG_WAVES];
    const mage_reloc_guided_args& a = p.a;
    const int pr = blockIdx.x, tid = threadIdx.x;
    const mage_reloc_guided_result R0 = a.d_result[pr];
    __syncthreads();  // every thread has the record before thread 0 changes it
    if (R0.verdict != RG_OK) {  // uniform over the workgroup
        if (tid == 0) p.count2[pr] = 0;
        return;
    }
    const uint32_t nr = min(a.d_n_radius[pr], R0.n_queries);
    if (nr < p.c.min_radius) {
        if (tid == 0) {
            a.d_result[pr].n_radius_matches = nr;
            a.d_result[pr].verdict = RG_FEW_RADIUS;
            p.count2[pr] = 0;
        }
        return;
    }
    const float* map = a.d_map_xyzi + 4 * pr * a.kf_pitch;
    const long long q0 = (long long)pr * a.cap;
    const relocpnp::BehindFilter bf = relocpnp::behind_filter(R0.pos3_first, R0.r9_first);
    uint32_t n = 0;
    for (uint32_t m0 = 0; m0 < nr; m0 += RG_THREADS) {
        const uint32_t m = m0 + tid;
        int32_t k = 0, t = 0;
        bool keep = false;
        if (m < nr) {
            const mage_dmatch d = a.d_radius_matches[q0 + m];
            k = a.d_query_ref[q0 + d.query_idx];
            t = d.train_idx;
            keep = !point_behind(bf, map + 4ll * k);
        }
        uint32_t total;
        const uint32_t pos = n + block_prefix<RG_WAVES>(keep, s_wsum, &total);
        if (keep) {
            a.d_assoc[2 * (q0 + pos)] = k;
            a.d_assoc[2 * (q0 + pos) + 1] = t;
        }
        n += total;
    }
    if (tid == 0) {
        const bool few = n < p.c.min_points;
        a.d_result[pr].n_radius_matches = nr;
        a.d_result[pr].n_in_front = n;
        if (few) a.d_result[pr].verdict = RG_FEW_POINTS;
        p.count2[pr] = few ? 0u : n;
    }
}

__global__ __launch_bounds__(RG_THREADS) void reloc_gpack_kernel(RgParams p)
{
    __shared__ uint32_t s_part[RG_THREADS];
    const mage_reloc_guided_args& a = p.a;
    const int pr = blockIdx.x, tid = threadIdx.x;
    // the counts before this problem, summed (integers: any order)
    uint32_t part = 0;
    for (uint32_t k = tid; k < (uint32_t)pr; k += RG_THREADS) part += p.count2[k];
    s_part[tid] = part;
    __syncthreads();
    for (int s = RG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) s_part[tid] += s_part[tid + s];
        __syncthreads();
    }
    const uint32_t start = s_part[0], n = p.count2[pr];
    if (tid == 0) {
        a.d_ba_obs_start[pr] = start;
        if ((uint32_t)pr + 1 == p.problems) a.d_ba_obs_start[p.problems] = start + n;
    }
    const float* map = a.d_map_xyzi + 4 * pr * a.kf_pitch;
    const mage_keypoint* kp = a.d_kp + pr * a.kp_pitch;
    const int32_t* assoc = a.d_assoc + 2 * (long long)pr * a.cap;
    for (uint32_t i = tid; i < n; i += RG_THREADS) {
        const float* X = map + 4ll * assoc[2 * i];
        const mage_keypoint& f = kp[assoc[2 * i + 1]];
        const size_t o = (size_t)start + i;
        a.d_ba_points3[3 * o] = X[0];
        a.d_ba_points3[3 * o + 1] = X[1];
        a.d_ba_points3[3 * o + 2] = X[2];
        a.d_ba_uv[2 * o] = f.x;
        a.d_ba_uv[2 * o + 1] = f.y;
        a.d_ba_info[o] = X[3];
    }
}

__global__ __launch_bounds__(RG_THREADS) void reloc_decide_kernel(RgParams p)
{
    const mage_reloc_guided_args& a = p.a;
    const uint32_t frame = blockIdx.x, tid = threadIdx.x;
    mage_reloc_frame_result F;
    init_frame(F);
    for (uint32_t c = 0; c < a.candidates_per_frame; c++) {  // uniform over the workgroup
        const long long pr = (long long)frame * a.candidates_per_frame + c;
        const uint32_t verdict = a.d_result[pr].verdict, n = a.d_result[pr].n_in_front, e0 = a.d_ba_obs_start[pr];
        __syncthreads();  // every thread has the record before thread 0 changes it
        if (verdict != RG_OK) continue;
        uint32_t outliers = 0;
        for (uint32_t i0 = 0; i0 < n; i0 += RG_THREADS) {
            const uint32_t i = i0 + tid;
            outliers += (uint32_t)__syncthreads_count(i < n && a.d_ba_outlier[e0 + i] != 0);
        }
        const bool fails = ba_gate_fails(n, outliers, p.c.min_ba_pct);
        if (tid == 0) {
            mage_reloc_guided_result R = a.d_result[pr];
            R.n_outliers = outliers;
            for (int k = 0; k < 3; k++) R.pos3[k] = p.pos2[3 * pr + k];
            for (int k = 0; k < 9; k++) R.r9[k] = p.r92[9 * pr + k];
            if (fails) R.verdict = RG_FEW_BA_INLIERS;
            a.d_result[pr] = R;
            if (!fails && F.index < 0 && p.c.rounds >= 1 && (R.status & (RG_STATUS_OVER_LIMIT | RG_STATUS_BAD_ORDER)) == 0)
                take_candidate(F, c, R);
        }
    }
    if (tid == 0) a.d_frame_result[frame] = F;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct ScratchLayout {
    size_t pos1, r91, pos2, r92, mean1, mean2, outlier1, res, count2, status, bytes;
};

ScratchLayout scratch_layout(uint64_t problems, uint64_t cap, uint64_t pnp_cap)
{
    ScratchLayout s{};
    size_t at = 0;
    auto take = [&at](uint64_t n) {
        const size_t o = at;
        at = align256(at + (size_t)n);
        return o;
    };
    s.pos1 = take(12 * problems);
    s.r91 = take(36 * problems);
    s.pos2 = take(12 * problems);
    s.r92 = take(36 * problems);
    s.mean1 = take(4 * problems);
    s.mean2 = take(4 * problems);
    s.outlier1 = take(problems * pnp_cap);
    s.res = take(4 * problems * cap);
    s.count2 = take(4 * problems);
    s.status = take(4);
    s.bytes = at;
    return s;
}

}  // namespace
}  // namespace mage

extern "C" uint64_t mage_reloc_guided_scratch_bytes(uint32_t problems, uint32_t cap, uint32_t pnp_cap)
{
    return mage::scratch_layout(problems, cap, pnp_cap).bytes;
}

extern "C" mage_status mage_reloc_guided_batch_device(const mage_reloc_settings* settings,
                                                      const mage_reloc_guided_args* args, mage_stream stream)
{
    using namespace mage;
    const char* why = relocguided::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(args && args->struct_size == sizeof(mage_reloc_guided_args), MAGE_EINVAL,
                 "struct_size is not sizeof(mage_reloc_guided_args)");
    const mage_reloc_guided_args& a = *args;
    const uint64_t problems64 = (uint64_t)a.frames * a.candidates_per_frame;
    if (problems64 == 0) return MAGE_OK;
    MAGE_REQUIRE(problems64 <= 0x7fffffffull, MAGE_EINVAL, "too many problems");
    const uint32_t problems = (uint32_t)problems64;
    MAGE_REQUIRE(a.d_intr4 && a.d_map_xyzi && a.d_kf_kp && a.d_kf_desc && a.d_n_kf && a.d_kp && a.d_desc && a.d_n_kp &&
                     a.d_pnp_result && a.d_obs_start && a.d_points3 && a.d_uv && a.d_info && a.d_pos3 && a.d_r9 &&
                     a.d_query_kp && a.d_query_pos && a.d_query_desc && a.d_query_ref && a.d_n_queries &&
                     a.d_radius_matches && a.d_n_radius && a.d_assoc && a.d_ba_obs_start && a.d_ba_points3 && a.d_ba_uv &&
                     a.d_ba_info && a.d_ba_outlier && a.d_result && a.d_frame_result && a.d_scratch,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(!a.d_order || a.d_n_order, MAGE_EINVAL, "an order list needs its counts");
    MAGE_REQUIRE(a.kf_pitch > 0 && a.kp_pitch > 0 && a.cap > 0 && a.pnp_cap > 0, MAGE_EINVAL,
                 "pitches and capacities must be positive");
    MAGE_REQUIRE(a.pose_max_hamming_distance >= -1 && a.pose_max_hamming_distance <= 256, MAGE_EINVAL,
                 "pose_max_hamming_distance must be in [-1, 256]");
    MAGE_REQUIRE(((uintptr_t)a.d_scratch & 255) == 0 && ((uintptr_t)a.d_kf_desc & 15) == 0 && ((uintptr_t)a.d_query_desc & 15) == 0,
                 MAGE_EINVAL, "scratch must be 256-byte aligned, descriptors 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const ScratchLayout S = scratch_layout(problems, a.cap, a.pnp_cap);
    char* sb = static_cast<char*>(a.d_scratch);
    RgParams p{};
    p.c = relocguided::make_consts(*settings);
    p.a = a;
    p.problems = problems;
    p.pos1 = reinterpret_cast<float*>(sb + S.pos1);
    p.r91 = reinterpret_cast<float*>(sb + S.r91);
    p.pos2 = reinterpret_cast<float*>(sb + S.pos2);
    p.r92 = reinterpret_cast<float*>(sb + S.r92);
    p.count2 = reinterpret_cast<uint32_t*>(sb + S.count2);
    uint32_t* d_status = reinterpret_cast<uint32_t*>(sb + S.status);
    const float* ba_intr = a.d_ba_intr4 ? a.d_ba_intr4 : a.d_intr4;
    const float max_err = settings->max_bundle_adjust_reprojection_error;  // unsquared, as BundleAdjust.cpp:303 passes it
    mage_status r = mage_ba_pose_batch_device(problems, a.d_pos3, a.d_r9, ba_intr, a.d_obs_start, a.d_points3, a.d_uv,
                                              a.d_info, settings->bundle_adjust_iterations, RG_HUBER, max_err, p.pos1, p.r91,
                                              a.d_qt7_first, reinterpret_cast<uint8_t*>(sb + S.outlier1),
                                              reinterpret_cast<float*>(sb + S.mean1), nullptr, stream);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemsetAsync(d_status, 0, 4, st));
    launch("relocguided.query", reloc_query_kernel, dim3(problems), dim3(RG_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    r = mage_radius_match_batch_device(a.d_query_kp, a.d_query_pos, a.d_query_desc, a.cap, a.d_n_queries, a.d_kp, a.d_desc,
                                       a.kp_pitch, a.d_n_kp, problems, settings->search_radius,
                                       a.pose_max_hamming_distance, a.pose_min_hamming_difference,
                                       reinterpret_cast<int32_t*>(sb + S.res), a.d_radius_matches, a.cap, a.d_n_radius,
                                       d_status, stream);
    if (r != MAGE_OK) return r;
    launch("relocguided.gate", reloc_gate_kernel, dim3(problems), dim3(RG_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    launch("relocguided.pack", reloc_gpack_kernel, dim3(problems), dim3(RG_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    r = mage_ba_pose_batch_device(problems, p.pos1, p.r91, ba_intr, a.d_ba_obs_start, a.d_ba_points3, a.d_ba_uv,
                                  a.d_ba_info, settings->bundle_adjust_iterations, RG_HUBER, max_err, p.pos2, p.r92, a.d_qt7,
                                  a.d_ba_outlier, reinterpret_cast<float*>(sb + S.mean2), nullptr, stream);
    if (r != MAGE_OK) return r;
    launch("relocguided.decide", reloc_decide_kernel, dim3(a.frames), dim3(RG_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

extern "C" mage_status mage_reloc_candidates_batch_device(const mage_reloc_settings* settings,
                                                          const mage_reloc_candidates_args* cand,
                                                          const mage_reloc_guided_args* guided, mage_stream stream)
{
    using namespace mage;
    const char* why = relocguided::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(cand && cand->struct_size == sizeof(mage_reloc_candidates_args), MAGE_EINVAL,
                 "struct_size is not sizeof(mage_reloc_candidates_args)");
    MAGE_REQUIRE(guided && guided->struct_size == sizeof(mage_reloc_guided_args), MAGE_EINVAL,
                 "struct_size is not sizeof(mage_reloc_guided_args)");
    const mage_reloc_candidates_args& c = *cand;
    mage_reloc_guided_args a = *guided;
    const uint64_t problems64 = (uint64_t)a.frames * a.candidates_per_frame;
    if (problems64 == 0) return MAGE_OK;
    MAGE_REQUIRE(problems64 <= 0x7fffffffull, MAGE_EINVAL, "too many problems");
    const uint32_t problems = (uint32_t)problems64;
    MAGE_REQUIRE(c.d_leaf_kf && c.d_leaf && c.d_mask_kf && c.d_matches && c.d_n_matches && c.d_match_status &&
                     c.d_pnp_result && c.d_inlier_idx && c.d_obs_start && c.d_points3 && c.d_uv && c.d_info && c.d_pos3 &&
                     c.d_r9 && c.d_pnp_scratch && a.d_kf_desc && a.d_n_kf && a.d_desc && a.d_n_kp && a.d_intr4 &&
                     a.d_map_xyzi && a.d_kp,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(c.match_cap > 0 && a.kf_pitch > 0 && a.kp_pitch > 0, MAGE_EINVAL, "pitches and capacities must be positive");
    MAGE_HIP(hipMemsetAsync(c.d_match_status, 0, 4, (hipStream_t)stream));
    mage_status r = mage_indexed_match_batch_device(a.d_kf_desc, c.d_leaf_kf, c.d_mask_kf, a.kf_pitch, a.d_n_kf, a.d_desc,
                                                    c.d_leaf, nullptr, a.kp_pitch, a.d_n_kp, problems,
                                                    settings->max_hamming_distance, settings->min_hamming_difference,
                                                    c.d_matches, c.match_cap, c.d_n_matches, c.d_match_status, stream);
    if (r != MAGE_OK) return r;
    r = mage_reloc_pnp_batch_device(settings, problems, a.d_intr4, a.d_map_xyzi, a.kf_pitch, a.d_kp, a.kp_pitch, a.d_n_kp,
                                    c.d_matches, c.match_cap, c.d_n_matches, c.d_pnp_result, c.d_inlier_idx, c.match_cap,
                                    c.d_obs_start, c.d_points3, c.d_uv, c.d_info, c.d_pos3, c.d_r9, nullptr,
                                    c.d_pnp_scratch, stream);
    if (r != MAGE_OK) return r;
    a.pnp_cap = c.match_cap;
    a.d_pnp_result = c.d_pnp_result;
    a.d_obs_start = c.d_obs_start;
    a.d_points3 = c.d_points3;
    a.d_uv = c.d_uv;
    a.d_info = c.d_info;
    a.d_pos3 = c.d_pos3;
    a.d_r9 = c.d_r9;
    return mage_reloc_guided_batch_device(settings, &a, stream);
}

extern "C" mage_status mage_reloc_guided(const mage_reloc_settings* settings, int32_t pose_max_hamming_distance,
                                         int32_t pose_min_hamming_difference, uint32_t n_candidates, const float* intr4,
                                         const float* ba_intr4, const float* map_xyzi, const mage_keypoint* kf_kp,
                                         const uint8_t* kf_desc, uint32_t kf_pitch, const uint32_t* n_kf,
                                         const int32_t* order, const uint32_t* n_order, const mage_keypoint* kp,
                                         const uint8_t* desc, uint32_t n_kp, const mage_dmatch* matches, uint32_t match_cap,
                                         const uint32_t* n_matches, uint32_t cap, mage_reloc_guided_result* results,
                                         mage_reloc_pnp_result* pnp_results, mage_reloc_frame_result* frame,
                                         int32_t* assoc, int device)
{
    using namespace mage;
    const char* why = relocguided::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(intr4 && frame, MAGE_EINVAL, "null argument");
    if (n_candidates == 0) {
        relocguided::init_frame(*frame);
        return MAGE_OK;
    }
    MAGE_REQUIRE(map_xyzi && kf_kp && kf_desc && n_kf && n_matches && matches && results && assoc && (n_kp == 0 || (kp && desc)),
                 MAGE_EINVAL, "null argument");
    MAGE_REQUIRE(!order || n_order, MAGE_EINVAL, "an order list needs its counts");
    MAGE_REQUIRE(kf_pitch > 0 && match_cap > 0 && cap > 0, MAGE_EINVAL, "pitches and capacities must be positive");
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    HostScratch* sp = host_scratch(device, SCRATCH_RELOCGUIDED);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    const size_t P = n_candidates, KF = (size_t)P * kf_pitch, E = (size_t)P * cap, M = (size_t)P * match_cap;
    // the frame's keypoints per candidate, as the batched entries index them; a frame over the limit
    // is refused by its counts, so its pitch need not hold it
    const uint32_t kp_pitch = std::max(std::min(n_kp, (uint32_t)relocguided::RG_MAX_KEYPOINTS), 1u);
    const size_t KP = (size_t)P * kp_pitch;
    size_t at = 0;
    auto take = [&at](size_t n) {
        const size_t o = at;
        at = align256(at + n);
        return o;
    };
    // inputs (one H2D copy), outputs (one D2H copy), then what stays on the device
    const size_t ointr = take(16 * P), obai = take(16 * P), omap = take(16 * KF), okfkp = take(sizeof(mage_keypoint) * KF),
                 okfd = take(32 * KF), onkf = take(4 * P), oord = take(4 * KF), onord = take(4 * P),
                 okp = take(sizeof(mage_keypoint) * KP), odesc = take(32 * KP), onkp = take(4 * P),
                 omat = take(sizeof(mage_dmatch) * M), onmat = take(4 * P), in_end = at;
    const size_t ores = take(sizeof(mage_reloc_guided_result) * P), opnp = take(sizeof(mage_reloc_pnp_result) * P),
                 ofr = take(sizeof(mage_reloc_frame_result)), oassoc = take(8 * E), out_end = at;
    const size_t oidx = take(4 * M), oobs = take(4 * (P + 1)), opts = take(12 * M), ouv = take(8 * M), oinfo = take(4 * M),
                 opos = take(12 * P), or9 = take(36 * P),
                 opscr = take(mage_reloc_pnp_scratch_bytes(settings->ransac_iterations, n_candidates, match_cap, 0)),
                 oqkp = take(sizeof(mage_keypoint) * E), oqpos = take(8 * E), oqd = take(32 * E), oqref = take(4 * E),
                 onq = take(4 * P), orm = take(sizeof(mage_dmatch) * E), onr = take(4 * P), obobs = take(4 * (P + 1)),
                 obpts = take(12 * E), obuv = take(8 * E), obinfo = take(4 * E), obout = take(E),
                 ogscr = take(mage_reloc_guided_scratch_bytes(n_candidates, cap, match_cap)), total = at;
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(out_end)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    std::memset(h, 0, in_end);
    const uint32_t nkp_copy = std::min(n_kp, kp_pitch);
    for (size_t c = 0; c < P; c++) {
        std::memcpy(h + ointr + 16 * c, intr4, 16);
        std::memcpy(h + obai + 16 * c, ba_intr4 ? ba_intr4 + 4 * c : intr4, 16);
        if (n_kp) {
            std::memcpy(h + okp + sizeof(mage_keypoint) * c * kp_pitch, kp, sizeof(mage_keypoint) * (size_t)nkp_copy);
            std::memcpy(h + odesc + 32 * c * kp_pitch, desc, 32 * (size_t)nkp_copy);
        }
        reinterpret_cast<uint32_t*>(h + onkp)[c] = n_kp;
    }
    std::memcpy(h + omap, map_xyzi, 16 * KF);
    std::memcpy(h + okfkp, kf_kp, sizeof(mage_keypoint) * KF);
    std::memcpy(h + okfd, kf_desc, 32 * KF);
    std::memcpy(h + onkf, n_kf, 4 * P);
    if (order) {
        std::memcpy(h + oord, order, 4 * KF);
        std::memcpy(h + onord, n_order, 4 * P);
    }
    std::memcpy(h + omat, matches, sizeof(mage_dmatch) * M);
    std::memcpy(h + onmat, n_matches, 4 * P);
    MAGE_HIP(hipMemcpyAsync(b, h, in_end, hipMemcpyHostToDevice, S.st));
    auto f32 = [b](size_t o) { return reinterpret_cast<float*>(b + o); };
    auto u32 = [b](size_t o) { return reinterpret_cast<uint32_t*>(b + o); };
    r = mage_reloc_pnp_batch_device(settings, n_candidates, f32(ointr), f32(omap), kf_pitch,
                                    reinterpret_cast<const mage_keypoint*>(b + okp), kp_pitch, u32(onkp),
                                    reinterpret_cast<const mage_dmatch*>(b + omat), match_cap, u32(onmat),
                                    reinterpret_cast<mage_reloc_pnp_result*>(b + opnp), u32(oidx), match_cap, u32(oobs),
                                    f32(opts), f32(ouv), f32(oinfo), f32(opos), f32(or9), nullptr, b + opscr, S.st);
    if (r != MAGE_OK) return r;
    mage_reloc_guided_args a{};
    a.struct_size = sizeof(a);
    a.frames = 1;
    a.candidates_per_frame = n_candidates;
    a.cap = cap;
    a.pnp_cap = match_cap;
    a.pose_max_hamming_distance = pose_max_hamming_distance;
    a.pose_min_hamming_difference = pose_min_hamming_difference;
    a.kf_pitch = kf_pitch;
    a.kp_pitch = kp_pitch;
    a.d_intr4 = f32(ointr);
    a.d_ba_intr4 = f32(obai);
    a.d_map_xyzi = f32(omap);
    a.d_kf_kp = reinterpret_cast<const mage_keypoint*>(b + okfkp);
    a.d_kf_desc = reinterpret_cast<const uint8_t*>(b + okfd);
    a.d_n_kf = u32(onkf);
    a.d_order = order ? reinterpret_cast<const int32_t*>(b + oord) : nullptr;
    a.d_n_order = order ? u32(onord) : nullptr;
    a.d_kp = reinterpret_cast<const mage_keypoint*>(b + okp);
    a.d_desc = reinterpret_cast<const uint8_t*>(b + odesc);
    a.d_n_kp = u32(onkp);
    a.d_pnp_result = reinterpret_cast<const mage_reloc_pnp_result*>(b + opnp);
    a.d_obs_start = u32(oobs);
    a.d_points3 = f32(opts);
    a.d_uv = f32(ouv);
    a.d_info = f32(oinfo);
    a.d_pos3 = f32(opos);
    a.d_r9 = f32(or9);
    a.d_query_kp = reinterpret_cast<mage_keypoint*>(b + oqkp);
    a.d_query_pos = f32(oqpos);
    a.d_query_desc = reinterpret_cast<uint8_t*>(b + oqd);
    a.d_query_ref = reinterpret_cast<int32_t*>(b + oqref);
    a.d_n_queries = u32(onq);
    a.d_radius_matches = reinterpret_cast<mage_dmatch*>(b + orm);
    a.d_n_radius = u32(onr);
    a.d_assoc = reinterpret_cast<int32_t*>(b + oassoc);
    a.d_ba_obs_start = u32(obobs);
    a.d_ba_points3 = f32(obpts);
    a.d_ba_uv = f32(obuv);
    a.d_ba_info = f32(obinfo);
    a.d_ba_outlier = reinterpret_cast<uint8_t*>(b + obout);
    a.d_result = reinterpret_cast<mage_reloc_guided_result*>(b + ores);
    a.d_frame_result = reinterpret_cast<mage_reloc_frame_result*>(b + ofr);
    a.d_scratch = b + ogscr;
    r = mage_reloc_guided_batch_device(settings, &a, S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + ores, b + ores, out_end - ores, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    const mage_reloc_guided_result* R = reinterpret_cast<const mage_reloc_guided_result*>(h + ores);
    std::memcpy(results, R, sizeof(mage_reloc_guided_result) * P);
    if (pnp_results) std::memcpy(pnp_results, h + opnp, sizeof(mage_reloc_pnp_result) * P);
    std::memcpy(frame, h + ofr, sizeof(mage_reloc_frame_result));
    for (size_t c = 0; c < P; c++)
        if (R[c].n_in_front) std::memcpy(assoc + 2 * c * cap, h + oassoc + 8 * c * cap, 8ull * R[c].n_in_front);
    return MAGE_OK;
}
