// reloc_pnp.hip — PoseEstimator::PNPRansac with the steps around it in TryEstimatePoseFromCandidates
// (Core/MAGESLAM/Source/Tracking/PoseEstimator.cpp:291-342, :610-638) on MI355X (gfx950), batched
// over (lost frame, candidate keyframe) problems: a chain of launches on one stream, no host step:
//   reloc_sample_kernel  one workgroup per problem: the limits and index checks, the result record,
//                        the correspondences gathered in match order, one lane running the serial
//                        sampler (one generator for all iterations);
//   reloc_solve_kernel   one hypothesis per thread, 64 per workgroup: EPnP on five points; the packed
//                        12 x 12 matrix, its eigenvectors and L lane-interleaved in LDS
//                        (bank-conflict free, no scratch for the runtime-indexed arrays);
//   reloc_score_kernel   one hypothesis per wave: the inlier rule over all matches, a lane per match,
//                        the ballot stored as the hypothesis's bit word, the popcounts summed;
//   reloc_select_kernel  one workgroup per problem: one lane replays the adaptive loop over the
//                        counts; the winner's inliers compacted in match order without those behind
//                        the camera, the gate, the result record;
//   reloc_pack_kernel    one workgroup per problem: its place in obs_start (the prefix of the kept
//                        counts before it) and the pose bundle adjustment's inputs gathered there.
// All arithmetic is reloc_pnp_math.hpp's, shared with the twin (reloc_pnp.cpp).  No atomics;
// nothing depends on the order in which threads run; all loops are bounded by the counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "ordered_take.hpp"
#include "reloc_pnp_math.hpp"

namespace mage {
namespace {

using namespace relocpnp;

// The host-buffer entry's scratch slot, after monoinit_third.hip's 9.
constexpr ScratchSlot SCRATCH_RELOCPNP = static_cast<ScratchSlot>(10);

constexpr int RP_THREADS = 256;
constexpr int RP_WAVES = RP_THREADS / kWave;
constexpr int RP_SOLVE_THREADS = 64;

struct RpParams {
    Consts c;
    TraceLayout L;
    const float* intr4;
    const float* map;
    long long kf_pitch;
    const mage_keypoint* kp;
    long long kp_pitch;
    const uint32_t* n_kp;
    const mage_dmatch* matches;
    uint32_t match_cap;
    const uint32_t* n_matches;
    mage_reloc_pnp_result* result;
    uint32_t* inlier_idx;
    uint32_t cap;
    uint32_t* obs_start;
    float *points3, *uv, *info, *pos3, *r9;
    char* work;                // problems x L.bytes: the trace, or the scratch's first part
    Corr* corr;                // problems x match_cap gathered correspondences
    unsigned long long* bits;  // problems x iters x words: bit m % 64 of word m / 64 = match m is an inlier
    uint32_t words;
    uint32_t* kept;            // problems: the observations a problem contributes
    uint32_t problems;
};

__device__ __forceinline__ Trace trace_of(const RpParams& p, int pr) { return trace_at(p.work + (size_t)pr * p.L.bytes, p.L); }

// A problem the later kernels skip: stopped by reloc_sample_kernel (its result record says why).
__device__ __forceinline__ bool stopped(const RpParams& p, int pr)
{
    const mage_reloc_pnp_result& r = p.result[pr];
    return (r.status & (RP_STATUS_OVER_LIMIT | RP_STATUS_BAD_INDEX)) != 0 || r.verdict != RP_OK;
}

__global__ __launch_bounds__(RP_THREADS) void reloc_sample_kernel(RpParams p)
{
    const int pr = blockIdx.x, tid = threadIdx.x;
    const uint32_t nk = p.n_kp[pr], nm = p.n_matches[pr];
    const bool over = nm > p.match_cap || nm > (uint32_t)RP_MAX_MATCHES || (long long)nk > p.kp_pitch;
    const mage_dmatch* mm = p.matches + (long long)pr * p.match_cap;
    const float* map = p.map + 4 * pr * p.kf_pitch;
    int bad = 0;
    if (!over)
        for (uint32_t m = tid; m < nm; m += RP_THREADS) {
            const int q = mm[m].query_idx, t = mm[m].train_idx;
            if (q < 0 || (long long)q >= p.kf_pitch || t < 0 || (uint32_t)t >= nk)
                bad = 1;
            else if (!(map[4ll * q + 3] > 0.f))
                bad = 1;
        }
    bad = __syncthreads_or(bad);
    const uint32_t status = over ? RP_STATUS_OVER_LIMIT : (bad ? RP_STATUS_BAD_INDEX : 0u);
    const uint32_t verdict = status != 0 ? RP_OK : (nm < p.c.min_matches ? RP_FEW_MATCHES : (nm < 5u ? RP_NO_MODEL : RP_OK));
    if (tid == 0) {
        mage_reloc_pnp_result R;
        init_result(R, nm);
        R.status = status;
        R.verdict = verdict;
        p.result[pr] = R;
        for (int k = 0; k < 3; k++) p.pos3[3ll * pr + k] = R.pos3[k];
        for (int k = 0; k < 9; k++) p.r9[9ll * pr + k] = R.r9[k];
        p.kept[pr] = 0;
    }
    if (status != 0 || verdict != RP_OK) return;  // uniform over the workgroup
    const mage_keypoint* kp = p.kp + pr * p.kp_pitch;
    Corr* corr = p.corr + (size_t)pr * p.match_cap;
    for (uint32_t m = tid; m < nm; m += RP_THREADS) {
        const mage_dmatch d = mm[m];
        const float* x = map + 4ll * d.query_idx;
        const mage_keypoint& k = kp[d.train_idx];
        corr[m] = Corr{x[0], x[1], x[2], x[3], k.x, k.y, d.query_idx, d.train_idx};
    }
    if (tid == 0) {
        const Trace T = trace_of(p, pr);
        if (nm > 5u) {
            sample_indices(nm, p.c.iters, T.idx);
        } else {
            for (uint32_t k = 0; k < 5 * p.c.iters; k++) T.idx[k] = k < 5 ? (int32_t)k : -1;
        }
    }
}

// grid (problems, ceil(iters / 64)): one hypothesis per thread.
__global__ __launch_bounds__(RP_SOLVE_THREADS) void reloc_solve_kernel(RpParams p)
{
    __shared__ double s_w[RP_WORK_D * RP_SOLVE_THREADS];
    const int pr = blockIdx.x, tid = threadIdx.x;
    if (stopped(p, pr)) return;
    const uint32_t it = blockIdx.y * RP_SOLVE_THREADS + tid;
    if (it >= p.c.iters) return;
    const Trace T = trace_of(p, pr);
    double* R = T.R + 9ull * it;
    double* t = T.t + 3ull * it;
    double* err = T.err + 3ull * it;
    int solved = 0;
    if (T.idx[5 * it] >= 0) {
        const Corr* corr = p.corr + (size_t)pr * p.match_cap;
        Corr c5[5];
        for (int k = 0; k < 5; k++) c5[k] = corr[T.idx[5 * it + k]];
        double Rm[9], tm[3], em[3];
        solved = solve_epnp5(c5, p.intr4 + 4ll * pr, Strided<double>{s_w + tid, RP_SOLVE_THREADS}, Rm, tm, em) ? 1 : 0;
        for (int k = 0; k < 9; k++) R[k] = Rm[k];
        for (int k = 0; k < 3; k++) {
            t[k] = tm[k];
            err[k] = em[k];
        }
    } else {
        for (int k = 0; k < 9; k++) R[k] = 0.0;
        for (int k = 0; k < 3; k++) {
            t[k] = 0.0;
            err[k] = -1.0;
        }
    }
    T.solved[it] = solved;
}

// grid (problems, ceil(iters / 4)): one hypothesis per wave, a lane per match.
__global__ __launch_bounds__(RP_THREADS) void reloc_score_kernel(RpParams p)
{
    const int pr = blockIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (stopped(p, pr)) return;
    const uint32_t it = blockIdx.y * RP_WAVES + wave;
    if (it >= p.c.iters) return;  // uniform over the wave
    const Trace T = trace_of(p, pr);
    const uint32_t nm = p.result[pr].n_matches;
    unsigned long long* bits = p.bits + ((size_t)pr * p.c.iters + it) * p.words;
    uint32_t count = 0;
    if (T.solved[it]) {
        double R[9], t[3];
        for (int k = 0; k < 9; k++) R[k] = T.R[9ull * it + k];
        for (int k = 0; k < 3; k++) t[k] = T.t[3ull * it + k];
        const float* intr = p.intr4 + 4ll * pr;
        const Corr* corr = p.corr + (size_t)pr * p.match_cap;
        for (uint32_t m0 = 0; m0 < nm; m0 += kWave) {  // uniform over the wave
            const uint32_t m = m0 + lane;
            const bool in = m < nm && (nm == 5u || is_inlier(R, t, intr, corr[m], p.c.thr_sq));
            const unsigned long long b = __ballot(in);
            if (lane == 0) bits[m0 / kWave] = b;
            count += (uint32_t)__builtin_popcountll(b);
        }
    }
    if (lane == 0) T.count[it] = count;
}

__global__ __launch_bounds__(RP_THREADS) void reloc_select_kernel(RpParams p)
{
    __shared__ uint32_t s_wsum[RP_WAVES];
    __shared__ mage_reloc_pnp_result s_r;
    __shared__ BehindFilter s_bf;
    const int pr = blockIdx.x, tid = threadIdx.x;
    if (stopped(p, pr)) return;
    const Trace T = trace_of(p, pr);
    if (tid == 0) {
        s_r = p.result[pr];
        const uint32_t nm = s_r.n_matches;
        const LoopResult loop = replay_loop(T.idx, T.solved, T.count, p.c.iters, nm, p.c.confidence, nm > 5u);
        s_r.iterations = loop.niters;
        s_r.iterations_run = loop.run;
        s_r.win_iteration = loop.win;
        if (loop.win >= 0) {
            s_r.n_inliers = loop.best;
            for (int k = 0; k < 5; k++) s_r.win_indices[k] = T.idx[5 * loop.win + k];
            float_pose(T.R + 9ull * loop.win, T.t + 3ull * loop.win, s_r.pos3, s_r.r9);
            s_bf = behind_filter(s_r.pos3, s_r.r9);
        } else {
            s_r.verdict = RP_NO_MODEL;
        }
    }
    __syncthreads();
    if (s_r.win_iteration < 0) {  // uniform over the workgroup
        if (tid == 0) p.result[pr] = s_r;
        return;
    }
    const uint32_t nm = s_r.n_matches;
    const unsigned long long* bits = p.bits + ((size_t)pr * p.c.iters + (uint32_t)s_r.win_iteration) * p.words;
    const Corr* corr = p.corr + (size_t)pr * p.match_cap;
    uint32_t* out = p.inlier_idx + (size_t)pr * p.cap;
    uint32_t in_front = 0;
    for (uint32_t c0 = 0; c0 < nm; c0 += RP_THREADS) {
        const uint32_t m = c0 + tid;
        const bool keep = m < nm && ((bits[m / 64] >> (m % 64)) & 1ull) != 0 && !is_behind(s_bf, corr[m]);
        uint32_t total;
        const uint32_t pos = in_front + block_prefix<RP_WAVES>(keep, s_wsum, &total);
        if (keep && pos < p.cap) out[pos] = m;
        in_front += total;
    }
    if (tid == 0) {
        s_r.n_in_front = in_front;
        s_r.n_kept = min(in_front, p.cap);
        if (in_front > p.cap) s_r.status |= RP_STATUS_OVER_CAP;
        if (gate_fails(in_front, nm, p.c.min_pct)) s_r.verdict = RP_FEW_INLIERS;
        p.result[pr] = s_r;
        for (int k = 0; k < 3; k++) p.pos3[3ll * pr + k] = s_r.pos3[k];
        for (int k = 0; k < 9; k++) p.r9[9ll * pr + k] = s_r.r9[k];
        p.kept[pr] = s_r.verdict == RP_OK ? s_r.n_kept : 0u;
    }
}

__global__ __launch_bounds__(RP_THREADS) void reloc_pack_kernel(RpParams p)
{
    __shared__ uint32_t s_part[RP_THREADS];
    const int pr = blockIdx.x, tid = threadIdx.x;
    // the kept counts before this problem, summed (integers: any order)
    uint32_t part = 0;
    for (uint32_t k = tid; k < (uint32_t)pr; k += RP_THREADS) part += p.kept[k];
    s_part[tid] = part;
    __syncthreads();
    for (int s = RP_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) s_part[tid] += s_part[tid + s];
        __syncthreads();
    }
    const uint32_t start = s_part[0], n = p.kept[pr];
    if (tid == 0) {
        p.obs_start[pr] = start;
        if ((uint32_t)pr + 1 == p.problems) p.obs_start[p.problems] = start + n;
    }
    const Corr* corr = p.corr + (size_t)pr * p.match_cap;
    const uint32_t* idx = p.inlier_idx + (size_t)pr * p.cap;
    for (uint32_t i = tid; i < n; i += RP_THREADS) {
        const Corr c = corr[idx[i]];
        const size_t o = (size_t)start + i;
        p.points3[3 * o] = c.x;
        p.points3[3 * o + 1] = c.y;
        p.points3[3 * o + 2] = c.z;
        p.uv[2 * o] = c.u;
        p.uv[2 * o + 1] = c.v;
        p.info[o] = c.info;
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct ScratchLayout {
    size_t work, corr, bits, kept, bytes;
    uint32_t words;
};

ScratchLayout scratch_layout(uint32_t iters, uint32_t problems, uint32_t match_cap, bool with_trace)
{
    ScratchLayout s{};
    s.words = (match_cap + 63) / 64;
    size_t at = with_trace ? 0 : align256((size_t)problems * trace_layout(iters).bytes);
    s.corr = at;
    at = align256(at + sizeof(Corr) * (size_t)problems * match_cap);
    s.bits = at;
    at = align256(at + 8ull * problems * iters * s.words);
    s.kept = at;
    at = align256(at + 4ull * problems);
    s.bytes = at;
    return s;
}

}  // namespace
}  // namespace mage

extern "C" uint64_t mage_reloc_pnp_scratch_bytes(uint32_t iterations, uint32_t problems, uint32_t match_cap, int32_t with_trace)
{
    return mage::scratch_layout(iterations, problems, match_cap, with_trace != 0).bytes;
}

extern "C" mage_status mage_reloc_pnp_batch_device(const mage_reloc_settings* settings, uint32_t problems,
                                                   const float* d_intr4, const float* d_map_xyzi, int64_t kf_pitch,
                                                   const mage_keypoint* d_kp, int64_t kp_pitch, const uint32_t* d_n_kp,
                                                   const mage_dmatch* d_matches, uint32_t match_cap,
                                                   const uint32_t* d_n_matches, mage_reloc_pnp_result* d_result,
                                                   uint32_t* d_inlier_idx, uint32_t cap, uint32_t* d_obs_start,
                                                   float* d_points3, float* d_uv, float* d_info, float* d_pos3,
                                                   float* d_r9, void* d_trace, void* d_scratch, mage_stream stream)
{
    using namespace mage;
    const char* why = relocpnp::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    if (problems == 0) return MAGE_OK;
    MAGE_REQUIRE(d_intr4 && d_map_xyzi && d_kp && d_n_kp && d_matches && d_n_matches && d_result && d_inlier_idx &&
                     d_obs_start && d_points3 && d_uv && d_info && d_pos3 && d_r9 && d_scratch,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(kf_pitch > 0 && kp_pitch > 0 && match_cap > 0 && cap > 0, MAGE_EINVAL,
                 "pitches and capacities must be positive");
    MAGE_REQUIRE((((uintptr_t)d_scratch | (uintptr_t)d_trace) & 7) == 0, MAGE_EINVAL, "scratch and trace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    RpParams p{};
    p.c = relocpnp::make_consts(*settings);
    p.L = relocpnp::trace_layout(p.c.iters);
    const ScratchLayout S = scratch_layout(p.c.iters, problems, match_cap, d_trace != nullptr);
    p.intr4 = d_intr4;
    p.map = d_map_xyzi;
    p.kf_pitch = kf_pitch;
    p.kp = d_kp;
    p.kp_pitch = kp_pitch;
    p.n_kp = d_n_kp;
    p.matches = d_matches;
    p.match_cap = match_cap;
    p.n_matches = d_n_matches;
    p.result = d_result;
    p.inlier_idx = d_inlier_idx;
    p.cap = cap;
    p.obs_start = d_obs_start;
    p.points3 = d_points3;
    p.uv = d_uv;
    p.info = d_info;
    p.pos3 = d_pos3;
    p.r9 = d_r9;
    char* sb = static_cast<char*>(d_scratch);
    p.work = d_trace ? static_cast<char*>(d_trace) : sb + S.work;
    p.corr = reinterpret_cast<Corr*>(sb + S.corr);
    p.bits = reinterpret_cast<unsigned long long*>(sb + S.bits);
    p.words = S.words;
    p.kept = reinterpret_cast<uint32_t*>(sb + S.kept);
    p.problems = problems;
    const uint32_t iters = p.c.iters;
    launch("relocpnp.sample", reloc_sample_kernel, dim3(problems), dim3(RP_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    launch("relocpnp.solve", reloc_solve_kernel, dim3(problems, (iters + RP_SOLVE_THREADS - 1) / RP_SOLVE_THREADS),
           dim3(RP_SOLVE_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    launch("relocpnp.score", reloc_score_kernel, dim3(problems, (iters + RP_WAVES - 1) / RP_WAVES), dim3(RP_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    launch("relocpnp.select", reloc_select_kernel, dim3(problems), dim3(RP_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    launch("relocpnp.pack", reloc_pack_kernel, dim3(problems), dim3(RP_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

extern "C" mage_status mage_reloc_pnp(const mage_reloc_settings* settings, const float* intr4, const float* map_xyzi,
                                      uint32_t n_kf, const mage_keypoint* kp, uint32_t n_kp, const mage_dmatch* matches,
                                      uint32_t n_matches, mage_reloc_pnp_result* result, uint32_t* inlier_idx,
                                      uint32_t cap, float* points3, float* uv, float* info, void* trace, int device)
{
    using namespace mage;
    const char* why = relocpnp::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(intr4 && result, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE((n_kf == 0 || map_xyzi) && (n_kp == 0 || kp) && (n_matches == 0 || matches) &&
                     (cap == 0 || (inlier_idx && points3 && uv && info)),
                 MAGE_EINVAL, "null argument");
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    if (n_matches > (uint32_t)relocpnp::RP_MAX_MATCHES) {  // nothing else is written
        mage_reloc_pnp_result R;
        relocpnp::init_result(R, n_matches);
        R.status = relocpnp::RP_STATUS_OVER_LIMIT;
        *result = R;
        return MAGE_OK;
    }
    HostScratch* sp = host_scratch(device, SCRATCH_RELOCPNP);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [intr][map][kp][counts][matches] | [result][inlier idx][obs_start][points, uv, info]
    // [pos3][r9][trace] | [scratch]: the inputs in one H2D copy, result to trace back in one D2H copy
    const uint32_t iters = settings->ransac_iterations;
    const size_t tbytes = relocpnp::trace_layout(iters).bytes;
    const uint32_t pkf = std::max(n_kf, 1u), pkp = std::max(n_kp, 1u), mc = std::max(n_matches, 1u), dcap = std::max(cap, 1u);
    const size_t sbytes = scratch_layout(iters, 1, mc, true).bytes;
    const size_t ointr = 0, omap = align256(ointr + 16), okp = align256(omap + 16ull * pkf),
                 ocnt = align256(okp + sizeof(mage_keypoint) * (size_t)pkp), omat = align256(ocnt + 8),
                 ores = align256(omat + sizeof(mage_dmatch) * (size_t)mc),
                 oidx = align256(ores + sizeof(mage_reloc_pnp_result)), oobs = align256(oidx + 4ull * dcap),
                 opts = align256(oobs + 8), ouv = align256(opts + 12ull * dcap), oinfo = align256(ouv + 8ull * dcap),
                 opos = align256(oinfo + 4ull * dcap), or9 = align256(opos + 12), otr = align256(or9 + 36),
                 oscr = align256(otr + tbytes), total = align256(oscr + sbytes);
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(oscr)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    std::memset(h, 0, ores);
    std::memcpy(h + ointr, intr4, 16);
    if (n_kf) std::memcpy(h + omap, map_xyzi, 16ull * n_kf);
    if (n_kp) std::memcpy(h + okp, kp, sizeof(mage_keypoint) * (size_t)n_kp);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(h + ocnt);  // n_kp, n_matches
    cnt[0] = n_kp;
    cnt[1] = n_matches;
    if (n_matches) std::memcpy(h + omat, matches, sizeof(mage_dmatch) * (size_t)n_matches);
    MAGE_HIP(hipMemcpyAsync(b, h, ores, hipMemcpyHostToDevice, S.st));
    uint32_t* dc = reinterpret_cast<uint32_t*>(b + ocnt);
    r = mage_reloc_pnp_batch_device(settings, 1, reinterpret_cast<const float*>(b + ointr),
                                    reinterpret_cast<const float*>(b + omap), pkf,
                                    reinterpret_cast<const mage_keypoint*>(b + okp), pkp, dc,
                                    reinterpret_cast<const mage_dmatch*>(b + omat), mc, dc + 1,
                                    reinterpret_cast<mage_reloc_pnp_result*>(b + ores), reinterpret_cast<uint32_t*>(b + oidx),
                                    dcap, reinterpret_cast<uint32_t*>(b + oobs), reinterpret_cast<float*>(b + opts),
                                    reinterpret_cast<float*>(b + ouv), reinterpret_cast<float*>(b + oinfo),
                                    reinterpret_cast<float*>(b + opos), reinterpret_cast<float*>(b + or9), b + otr, b + oscr,
                                    S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + ores, b + ores, oscr - ores, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    const mage_reloc_pnp_result* R = reinterpret_cast<const mage_reloc_pnp_result*>(h + ores);
    *result = *R;
    // the candidate has n_kf keypoints, the device form's bound is its pitch: the same here, as pkf
    // is n_kf unless that is 0, when every match is bad either way
    const bool ran = (R->status & (relocpnp::RP_STATUS_OVER_LIMIT | relocpnp::RP_STATUS_BAD_INDEX)) == 0 &&
                     R->verdict != relocpnp::RP_FEW_MATCHES && n_matches >= 5;
    if (trace && ran) std::memcpy(trace, h + otr, tbytes);
    // cap == 0 ran with one spare entry: every kept inlier is then over the capacity
    if (cap == 0) {
        if (R->n_in_front > 0) result->status |= relocpnp::RP_STATUS_OVER_CAP;
        result->n_kept = 0;
    }
    const uint32_t n = cap ? R->n_kept : 0;
    if (n) {
        std::memcpy(inlier_idx, h + oidx, 4ull * n);
        if (R->verdict == relocpnp::RP_OK) {
            std::memcpy(points3, h + opts, 12ull * n);
            std::memcpy(uv, h + ouv, 8ull * n);
            std::memcpy(info, h + oinfo, 4ull * n);
        }
    }
    return MAGE_OK;
}
