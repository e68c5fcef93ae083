// monoinit_third.hip — the third frame of the monocular map initialisation on MI355X (gfx950).
//
// The reference (Core/MAGESLAM/Source/Tracking/MapInitialization.cpp:695-840) places the middle
// frame half way between the initialisation pair, offers every map point to it in order — projected,
// then looked up twice against one mask of unassociated keypoints, frame 0's descriptor under
// ExtraFrameMatchingSettings and frame 1's under FivePointMatchingSettings, the better match taking
// the keypoint — gives up below MinThirdFrameMatchPercentage, runs a pose-only bundle adjustment
// (TrackLocalMap::OptimizeCameraPose), culls its outliers and applies the gate again.  Four launches
// on one stream, no host step between them:
//   match    one workgroup per problem.  Lane 0 builds the midpoint pose; the octave-0 keypoints (the
//            query octave is 0) are staged in LDS and listed by horizontal band as newpoints_assoc.hip
//            lists them; the points go 256 at a time: one thread per point projects it, the points in
//            front are compacted in point order, 64 of them at a time 4 lanes per point gather up to
//            8 candidates (keypoint, both distances) of either query, and one wave takes them in order
//            with ordered_take.hpp's resolve_pairs_in_order (the exactness argument is there).  Then
//            the matched points' indices in point order, the first gate and the mask.
//   pack     pose_ba_kernel reads observations obs_start[k] .. obs_start[k + 1]: a scan of the
//            problems' counts and the gather of (point, keypoint position, info) into one
//            prefix-packed array.  A problem that failed the first gate contributes none.
//   pose BA  mage_ba_pose_batch_device, as it is.
//   finish   the outlier flags cull associations, the second gate, the surviving associations
//            compacted in point order as bundle-adjustment observations, the record.
// Only commuting integer atomics, barriers and plain stores; nothing in the results depends on the
// order in which threads run, and every loop is bounded by the counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "monoinit_third_math.hpp"
#include "ordered_take.hpp"
// the twin's HIP-free copy of MAGE_REQUIRE and set_error must stay common.hpp's: a differing macro
// is a build error here (an identical redefinition is none)
#pragma clang diagnostic push
#pragma clang diagnostic error "-Wmacro-redefined"
#include "require.hpp"
#pragma clang diagnostic pop

namespace mage {
namespace {

using namespace monothird;

// The host-buffer entry's scratch slot, after monoinit.hip's (common.hpp stays as it is).
constexpr ScratchSlot SCRATCH_MONOTHIRD = static_cast<ScratchSlot>(9);

constexpr int M3_THREADS = 256;
constexpr int M3_WAVES = M3_THREADS / kWave;
constexpr int M3_CAP = 8;     // candidates kept per point (more: the point rescans its bands)
constexpr int M3_GROUP = 4;   // lanes per point in the gather
constexpr int M3_CHUNK = 64;  // points per gather + resolve round
constexpr int M3_BANDS = 32;  // horizontal bands of the keypoint list
static_assert(M3_MAX_KP <= OT_MAX_TARGETS, "keypoint indices must fit the resolver's packings");

struct M3Params {
    Consts c;
    const float *intr4, *pos3, *r9, *points;
    uint32_t cap;
    const uint32_t* n_points;
    const int32_t *idx0, *idx1;
    const uint8_t *desc0, *desc1;
    long long pitch0, pitch1, pitch2;
    const uint32_t *n0, *n1, *n2;
    const mage_keypoint* kp2;
    const uint8_t* desc2;
    uint32_t cam_index;
    mage_mono_init_third_result* result;
    int32_t* keypoint;
    uint8_t* verdict;
    int32_t* dist;
    float* proj;
    uint8_t* mask;
    float* obs_uv;
    uint32_t *obs_pt, *obs_cam;
    float* obs_info;
    // the scratch (monothird::Layout)
    uint32_t *obs_start, *ba_count;
    float *ba_pos3, *ba_r9;
    uint32_t* matched;
    float *ba_points, *ba_uv, *ba_info;
    const uint8_t* outlier;
    const float *opt_pos3, *opt_r9, *mean_sq;
};

// The band of row y: monotone in y (a product with a positive constant, then a clamp), so every
// keypoint with y0 <= y <= y1 lies in bands band_of(y0) .. band_of(y1).  NaN goes to band 0.
__device__ __forceinline__ int band_of(float y, float scale)
{
    const float f = y * scale;
    return f >= 0.f ? (f < (float)M3_BANDS ? (int)f : M3_BANDS - 1) : 0;
}

struct M3Shared {
    float x[M3_MAX_KP], y[M3_MAX_KP];
    uint16_t key[M3_MAX_KP];  // the octave-0 keypoints by band, ascending keypoint within a band
    int bstart[M3_BANDS + 1], brun[M3_BANDS];
    int wband[M3_WAVES][M3_BANDS];
    uint32_t m[M3_MAX_KP / 32];
    int taker[M3_MAX_KP];
    float px[M3_THREADS], py[M3_THREADS];
    int pi[M3_THREADS];              // the points in front of the camera, in point order
    uint32_t ent[M3_CHUNK][M3_CAP];  // kept_entry2(keypoint, d0, d1)
    int n[M3_CHUNK];
    uint32_t wsum[M3_WAVES];
    float pose[12];  // the midpoint pose: pos3, r9
    int bad;
};

// One problem's arrays.
struct M3Problem {
    uint32_t np, n2;
    float band_scale;  // M3_BANDS / (2 cy); any positive scale is correct, the bands only have to be monotone in y
    const float *pts, *intr;
    const int32_t *idx0, *idx1;
    const uint8_t *d0, *d1, *d2;
    const mage_keypoint* kp;
    int32_t* keypoint;
    uint8_t* verdict;
    int32_t* dist;
    float* proj;
};

// The third frame's positions in LDS and its octave-0 keypoints listed by band; every keypoint
// starts unassociated (:717).
__device__ __forceinline__ void stage_frame(const M3Problem& v, M3Shared& s)
{
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < M3_BANDS) s.bstart[tid + 1] = 0;
    if (tid == 0) s.bstart[0] = 0;
    __syncthreads();
    for (int i = tid; i < (int)v.n2; i += M3_THREADS) {
        const float y = v.kp[i].y;
        s.x[i] = v.kp[i].x;
        s.y[i] = y;
        if (v.kp[i].octave == 0) atomicAdd(&s.bstart[band_of(y, v.band_scale) + 1], 1);
    }
    for (int i = tid; i < M3_MAX_KP; i += M3_THREADS) s.taker[i] = OT_NO_TAKER;
    for (int c0 = 0; c0 < M3_MAX_KP; c0 += M3_THREADS) {  // a wave's 64 mask bits are two words (all 128 are written)
        const int t = c0 + tid;
        const unsigned long long bal = __ballot(t < (int)v.n2);
        if (lane == 0) {
            s.m[t >> 5] = (uint32_t)bal;
            s.m[(t >> 5) + 1] = (uint32_t)(bal >> 32);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int b = 0; b < M3_BANDS; b++) {
            s.brun[b] = acc;
            acc += s.bstart[b + 1];
            s.bstart[b + 1] = acc;
        }
    }
    __syncthreads();
    // the list: 256 keypoints at a time, each octave-0 keypoint at its band's running base plus its
    // rank among the band's keypoints of the chunk
    for (int c0 = 0; c0 < (int)v.n2; c0 += M3_THREADS) {
        const int t = c0 + tid;
        const int b = t < (int)v.n2 && v.kp[t].octave == 0 ? band_of(s.y[t], v.band_scale) : -1;
        const int pos = rank_by_key<M3_WAVES>(b, true, M3_BANDS, s.brun, &s.wband[0][0], M3_BANDS);
        int add = 0;
        if (tid < M3_BANDS)
            for (int w = 0; w < M3_WAVES; w++) add += s.wband[w][tid];
        if (b >= 0) s.key[pos] = (uint16_t)t;
        __syncthreads();  // wband and brun are read: the next chunk may write them
        if (tid < M3_BANDS) s.brun[tid] += add;  // read again only after the next chunk's first barrier
    }
    __syncthreads();
}

// Points c0 .. c0 + 255, one thread each: a point behind the camera is final, the others are
// compacted in point order into px, py, pi.  Returns their count.
__device__ __forceinline__ int project_and_compact(const M3Problem& v, M3Shared& s, uint32_t c0)
{
    const uint32_t i = c0 + threadIdx.x;
    bool pass = false;
    float px = 0.f, py = 0.f;
    if (i < v.np) {
        const float X[3] = {v.pts[3 * i], v.pts[3 * i + 1], v.pts[3 * i + 2]};
        pass = !(project(s.pose, s.pose + 3, v.intr, X, px, py) < 0);
        v.proj[2 * i] = px;
        v.proj[2 * i + 1] = py;
        if (!pass) {
            v.keypoint[i] = -1;
            v.verdict[i] = M3_PT_BEHIND;
            v.dist[2 * i] = v.dist[2 * i + 1] = -1;
        }
    }
    uint32_t cnt;
    const uint32_t pos = block_prefix<M3_WAVES>(pass, s.wsum, &cnt);
    if (pass) {
        s.px[pos] = px;
        s.py[pos] = py;
        s.pi[pos] = (int)i;
    }
    __syncthreads();
    return (int)cnt;
}

// A point's search: its box, its run of the band list, its two descriptors.
struct Box {
    float x0, x1, y0, y1;
    int lo, hi;
    uint4 a0, a1, b0, b1;
};

__device__ __forceinline__ Box load_box(const M3Params& p, const M3Problem& v, const M3Shared& s, int i)
{
    const float r = p.c.radius, qx = s.px[i], qy = s.py[i];
    Box b;
    b.x0 = qx - r, b.x1 = qx + r, b.y0 = qy - r, b.y1 = qy + r;
    b.lo = s.bstart[band_of(b.y0, v.band_scale)];
    b.hi = s.bstart[band_of(b.y1, v.band_scale) + 1];
    const uint8_t* q0 = v.d0 + 32ll * v.idx0[s.pi[i]];
    const uint8_t* q1 = v.d1 + 32ll * v.idx1[s.pi[i]];
    b.a0 = *reinterpret_cast<const uint4*>(q0);
    b.a1 = *reinterpret_cast<const uint4*>(q0 + 16);
    b.b0 = *reinterpret_cast<const uint4*>(q1);
    b.b1 = *reinterpret_cast<const uint4*>(q1 + 16);
    return b;
}

// Entries lo, lo + 1, ... < hi of the band list: `visit(t, d0, d1)` for every keypoint in the box
// that is available under the current mask and within either query's maxDist.
template <typename F>
__device__ __forceinline__ void scan(const M3Params& p, const M3Problem& v, const M3Shared& s, const Box& b, int lo,
                                     int hi, F visit)
{
    for (int i = lo; i < hi; i++) {
        const int t = s.key[i];
        const float tx = s.x[t], ty = s.y[t];
        if (!(tx >= b.x0 && tx <= b.x1 && ty >= b.y0 && ty <= b.y1) || !mask_bit(s.m, t)) continue;
        const uint8_t* td = v.d2 + 32ll * t;
        const int d0 = (int)hamming256(b.a0, b.a1, td), d1 = (int)hamming256(b.b0, b.b1, td);
        if (d0 <= p.c.max_dist[0] || d1 <= p.c.max_dist[1]) visit(t, d0, d1);
    }
}

// Compacted points s0 .. s0 + 63, 4 lanes per point walking the point's run 4 entries at a time: up
// to 8 candidates per point into ent, their number into n.
__device__ __forceinline__ void gather(const M3Params& p, const M3Problem& v, M3Shared& s, int s0, int cnt)
{
    const int j = threadIdx.x / M3_GROUP, sub = threadIdx.x % M3_GROUP;
    const bool act = s0 + j < cnt;
    Box b = {};
    if (act) b = load_box(p, v, s, s0 + j);
    int n = 0;
    for (int i0 = b.lo; __any(i0 < b.hi); i0 += M3_GROUP) {
        bool f = false;
        uint32_t ent = 0;
        if (i0 + sub < b.hi)
            scan(p, v, s, b, i0 + sub, i0 + sub + 1, [&](int t, int d0, int d1) {
                f = true;
                ent = kept_entry2(t, d0, d1);
            });
        const int pos = group_append<M3_GROUP>(f, sub, n);
        if (f && pos < M3_CAP) s.ent[j][pos] = ent;
    }
    if (act && sub == 0) s.n[j] = n;
}

// One wave: the chunk's cc points take their keypoints in order; every point's outputs.
__device__ __forceinline__ void resolve(const M3Params& p, const M3Problem& v, M3Shared& s, int s0, int cc)
{
    resolve_pairs_in_order(
        cc, p.c.max_dist, p.c.min_diff, s.m, s.taker,
        [&](int j, bool act) {
            const int n = act ? s.n[j] : 0;
            Box b = {};
            if (n > M3_CAP) b = load_box(p, v, s, s0 + j);
            // every candidate of the lane that is still available (overflow: the bands rescanned)
            return [=, &p, &v, &s](auto fn) {
                if (n <= M3_CAP) {
                    for (int e = 0; e < n; e++) {
                        const uint32_t c = s.ent[j][e];
                        if (mask_bit(s.m, kept_target2(c))) fn(kept_target2(c), kept_dist2(c, 0), kept_dist2(c, 1));
                    }
                } else {
                    scan(p, v, s, b, b.lo, b.hi, fn);
                }
            };
        },
        [&](int j, int which, int t, int best0, int best1) {
            const int i = s.pi[s0 + j];
            v.keypoint[i] = which >= 0 ? t : -1;
            v.verdict[i] = which < 0 ? (uint8_t)M3_PT_NO_MATCH : (which ? (uint8_t)M3_PT_FRAME1 : (uint8_t)M3_PT_FRAME0);
            v.dist[2 * i] = best0;
            v.dist[2 * i + 1] = best1;
        });
}

// The record of a problem that stops before the matching, or the zeroed start of any other.
__device__ __forceinline__ mage_mono_init_third_result blank_record(uint32_t np, uint32_t status)
{
    mage_mono_init_third_result r = {};
    r.n_points = np;
    r.status = status;
    return r;
}

__global__ __launch_bounds__(M3_THREADS) void mono_third_match_kernel(M3Params p)
{
    __shared__ M3Shared s;
    const int tid = threadIdx.x;
    const long long prob = blockIdx.x;
    M3Problem v;
    v.np = p.n_points[prob];
    v.n2 = p.n2[prob];
    const uint32_t n0 = p.n0[prob], n1 = p.n1[prob];
    // uniform over the workgroup
    if (v.np > p.cap || v.np > (uint32_t)M3_MAX_POINTS || v.n2 > (uint32_t)M3_MAX_KP || (long long)v.n2 > p.pitch2 ||
        (long long)n0 > p.pitch0 || (long long)n1 > p.pitch1) {
        if (tid == 0) {
            p.result[prob] = blank_record(v.np, M3_STATUS_OVER_LIMIT);
            p.ba_count[prob] = 0;
        }
        return;
    }
    v.pts = p.points + 3ll * prob * p.cap;
    v.intr = p.intr4 + 4 * prob;
    v.idx0 = p.idx0 + prob * p.cap;
    v.idx1 = p.idx1 + prob * p.cap;
    v.d0 = p.desc0 + 32ll * prob * p.pitch0;
    v.d1 = p.desc1 + 32ll * prob * p.pitch1;
    v.d2 = p.desc2 + 32ll * prob * p.pitch2;
    v.kp = p.kp2 + prob * p.pitch2;
    v.band_scale = v.intr[1] > 1.f ? (float)M3_BANDS / (2.f * v.intr[1]) : 1.f;
    v.keypoint = p.keypoint + prob * p.cap;
    v.verdict = p.verdict + prob * p.cap;
    v.dist = p.dist + 2ll * prob * p.cap;
    v.proj = p.proj + 2ll * prob * p.cap;

    if (tid == 0) s.bad = 0;
    __syncthreads();
    bool bad = false;
    for (uint32_t i = tid; i < v.np; i += M3_THREADS) {
        const int a = v.idx0[i], b = v.idx1[i];
        bad |= a < 0 || (uint32_t)a >= n0 || b < 0 || (uint32_t)b >= n1;
    }
    if (bad) s.bad = 1;  // every writer stores the same value
    __syncthreads();
    if (s.bad) {
        if (tid == 0) {
            p.result[prob] = blank_record(v.np, M3_STATUS_BAD_INDEX);
            p.ba_count[prob] = 0;
        }
        return;
    }
    if (tid == 0) {
        float mp[3], mr[9];
        midpoint_pose(p.pos3 + 6 * prob, p.r9 + 18 * prob, mp, mr);
        for (int i = 0; i < 3; i++) s.pose[i] = p.ba_pos3[3 * prob + i] = mp[i];
        for (int i = 0; i < 9; i++) s.pose[3 + i] = p.ba_r9[9 * prob + i] = mr[i];
    }
    stage_frame(v, s);  // its barriers publish the pose

    for (uint32_t c0 = 0; c0 < v.np; c0 += M3_THREADS) {
        const int cnt = project_and_compact(v, s, c0);
        for (int s0 = 0; s0 < cnt; s0 += M3_CHUNK) {
            gather(p, v, s, s0, cnt);
            __syncthreads();
            if (tid < kWave) resolve(p, v, s, s0, min(M3_CHUNK, cnt - s0));
            __syncthreads();
        }
    }
    // the matched points in point order (the barrier above made the wave's stores visible)
    uint32_t nm = 0, nb = 0;
    uint32_t* matched = p.matched + prob * p.cap;
    for (uint32_t c0 = 0; c0 < v.np; c0 += M3_THREADS) {
        const uint32_t i = c0 + tid;
        const uint8_t vd = i < v.np ? v.verdict[i] : (uint8_t)M3_PT_NO_MATCH;
        const bool took = vd == M3_PT_FRAME0 || vd == M3_PT_FRAME1;
        uint32_t cnt, cb;
        const uint32_t pos = block_prefix<M3_WAVES>(took, s.wsum, &cnt);
        (void)block_prefix<M3_WAVES>(vd == M3_PT_BEHIND, s.wsum, &cb);
        if (took) matched[nm + pos] = i;
        nm += cnt;
        nb += cb;
    }
    if (tid == 0) {
        mage_mono_init_third_result r = blank_record(v.np, 0);
        r.n_behind = nb;
        r.n_matched = r.n_associated = nm;
        const bool fails = gate_fails(nm, v.np, p.c.min_pct);
        r.verdict = fails ? M3_FEW_MATCHES : M3_OK;
        for (int i = 0; i < 3; i++) r.pos3[i] = s.pose[i];
        for (int i = 0; i < 9; i++) r.r9[i] = s.pose[3 + i];
        p.result[prob] = r;
        p.ba_count[prob] = fails ? 0u : nm;
    }
    uint8_t* mask = p.mask + prob * p.pitch2;
    for (int t = tid; t < (int)v.n2; t += M3_THREADS) mask[t] = mask_bit(s.m, t) ? 1 : 0;
}

// The problems' observation counts scanned into obs_start, and every problem's matches gathered
// behind its offset.  One workgroup per problem; the scan is a strided sum over the problems before
// it (a batch is a few hundred problems).
__global__ __launch_bounds__(M3_THREADS) void mono_third_pack_kernel(M3Params p, uint32_t problems)
{
    __shared__ uint32_t part[M3_THREADS];
    const int tid = threadIdx.x;
    const long long prob = blockIdx.x;
    uint32_t acc = 0;
    for (uint32_t k = tid; k < (uint32_t)prob; k += M3_THREADS) acc += p.ba_count[k];
    part[tid] = acc;
    __syncthreads();
    for (int h = M3_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    const uint32_t base = part[0], n = p.ba_count[prob];
    if (tid == 0) {
        p.obs_start[prob] = base;
        if (prob + 1 == (long long)problems) p.obs_start[problems] = base + n;
    }
    const uint32_t* matched = p.matched + prob * p.cap;
    const int32_t* keypoint = p.keypoint + prob * p.cap;
    const float* pts = p.points + 3ll * prob * p.cap;
    const mage_keypoint* kp = p.kp2 + prob * p.pitch2;
    for (uint32_t j = tid; j < n; j += M3_THREADS) {
        const uint32_t i = matched[j], o = base + j;
        const int t = keypoint[i];
        for (int a = 0; a < 3; a++) p.ba_points[3ll * o + a] = pts[3 * i + a];
        p.ba_uv[2ll * o] = kp[t].x;
        p.ba_uv[2ll * o + 1] = kp[t].y;
        p.ba_info[o] = p.c.info;
    }
}

// :829-838 and the outputs: the flagged associations are dropped, the gate runs again, the
// surviving associations are compacted in point order.  One workgroup per problem.
__global__ __launch_bounds__(M3_THREADS) void mono_third_finish_kernel(M3Params p)
{
    __shared__ uint32_t wsum[M3_WAVES];
    const int tid = threadIdx.x;
    const long long prob = blockIdx.x;
    mage_mono_init_third_result* R = p.result + prob;
    if (R->status != 0) return;  // uniform
    const uint32_t np = R->n_points, nm = R->n_matched;
    const bool ran = R->verdict == M3_OK;
    const uint32_t base = p.obs_start[prob];
    const uint32_t* matched = p.matched + prob * p.cap;
    int32_t* keypoint = p.keypoint + prob * p.cap;
    uint8_t* verdict = p.verdict + prob * p.cap;
    uint32_t nout = 0;
    if (ran)
        for (uint32_t c0 = 0; c0 < nm; c0 += M3_THREADS) {
            const uint32_t j = c0 + tid;
            const bool out = j < nm && p.outlier[base + j] != 0;
            if (out) {
                keypoint[matched[j]] = -1;
                verdict[matched[j]] = M3_PT_CULLED;
            }
            uint32_t cnt;
            (void)block_prefix<M3_WAVES>(out, wsum, &cnt);
            nout += cnt;
        }
    __syncthreads();  // the culled points' keypoints are read below by other threads
    const mage_keypoint* kp = p.kp2 + prob * p.pitch2;
    float* uv = p.obs_uv + 2ll * prob * p.cap;
    uint32_t* opt = p.obs_pt + prob * p.cap;
    uint32_t* ocam = p.obs_cam + prob * p.cap;
    float* oinfo = p.obs_info + prob * p.cap;
    uint32_t na = 0;
    for (uint32_t c0 = 0; c0 < np; c0 += M3_THREADS) {
        const uint32_t i = c0 + tid;
        const int t = i < np ? keypoint[i] : -1;
        uint32_t cnt;
        const uint32_t o = na + block_prefix<M3_WAVES>(t >= 0, wsum, &cnt);
        if (t >= 0) {
            uv[2 * o] = kp[t].x;
            uv[2 * o + 1] = kp[t].y;
            opt[o] = i;
            ocam[o] = p.cam_index;
            oinfo[o] = p.c.info;
        }
        na += cnt;
    }
    if (tid == 0 && ran) {
        R->n_outliers = nout;
        R->n_associated = na;
        R->mean_sq = p.mean_sq[prob];
        for (int i = 0; i < 3; i++) R->opt_pos3[i] = p.opt_pos3[3 * prob + i];
        for (int i = 0; i < 9; i++) R->opt_r9[i] = p.opt_r9[9 * prob + i];
        if (gate_fails(na, np, p.c.min_pct)) R->verdict = M3_FEW_AFTER_CULL;
    }
}

}  // namespace
}  // namespace mage

extern "C" {

uint64_t mage_mono_init_third_scratch_bytes(uint32_t problems, uint32_t cap, uint64_t* offsets)
{
    const mage::monothird::Layout l = mage::monothird::layout(problems, cap);
    if (offsets) {
        const size_t o[13] = {l.obs_start, l.ba_count, l.ba_pos3,  l.ba_r9,  l.matched, l.ba_points, l.ba_uv,
                              l.ba_info,   l.outlier,  l.opt_pos3, l.opt_r9, l.mean_sq, l.opt_qt7};
        for (int i = 0; i < 13; i++) offsets[i] = o[i];
    }
    return l.bytes;
}

mage_status mage_mono_init_third_frame_batch_device(
    const mage_mono_init_settings* settings, uint32_t problems, const float* d_intr4, const float* d_pos3,
    const float* d_r9, const float* d_points, uint32_t cap, const uint32_t* d_n_points, const int32_t* d_idx0,
    const int32_t* d_idx1, const uint8_t* d_desc0, int64_t pitch0, const uint32_t* d_n0, const uint8_t* d_desc1,
    int64_t pitch1, const uint32_t* d_n1, const mage_keypoint* d_kp2, const uint8_t* d_desc2, int64_t pitch2,
    const uint32_t* d_n2, uint32_t cam_index, mage_mono_init_third_result* d_result, int32_t* d_keypoint,
    uint8_t* d_verdict, int32_t* d_dist, float* d_proj, uint8_t* d_mask, float* d_obs_uv, uint32_t* d_obs_pt,
    uint32_t* d_obs_cam, float* d_obs_info, void* d_scratch, mage_stream stream)
{
    using namespace mage;
    const char* why = monothird::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    if (problems == 0) return MAGE_OK;
    MAGE_REQUIRE(d_intr4 && d_pos3 && d_r9 && d_points && d_n_points && d_idx0 && d_idx1 && d_desc0 && d_n0 && d_desc1 &&
                     d_n1 && d_kp2 && d_desc2 && d_n2 && d_result && d_keypoint && d_verdict && d_dist && d_proj && d_mask &&
                     d_obs_uv && d_obs_pt && d_obs_cam && d_obs_info && d_scratch,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(pitch0 > 0 && pitch1 > 0 && pitch2 > 0 && cap > 0, MAGE_EINVAL, "pitches and capacities must be positive");
    MAGE_REQUIRE((uint64_t)problems * cap <= 0x7FFFFFFFull, MAGE_EINVAL, "too many points in the batch");
    MAGE_REQUIRE(reinterpret_cast<uintptr_t>(d_desc0) % 16 == 0 && reinterpret_cast<uintptr_t>(d_desc1) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(d_desc2) % 16 == 0,
                 MAGE_EINVAL, "descriptor pointers must be 16-byte aligned");
    MAGE_REQUIRE(reinterpret_cast<uintptr_t>(d_scratch) % 256 == 0, MAGE_EINVAL, "the scratch must be 256-byte aligned");
    const monothird::Layout l = monothird::layout(problems, cap);
    char* sc = static_cast<char*>(d_scratch);
    M3Params p{};
    p.c = monothird::make_consts(*settings);
    p.intr4 = d_intr4;
    p.pos3 = d_pos3;
    p.r9 = d_r9;
    p.points = d_points;
    p.cap = cap;
    p.n_points = d_n_points;
    p.idx0 = d_idx0;
    p.idx1 = d_idx1;
    p.desc0 = d_desc0;
    p.desc1 = d_desc1;
    p.pitch0 = pitch0;
    p.pitch1 = pitch1;
    p.pitch2 = pitch2;
    p.n0 = d_n0;
    p.n1 = d_n1;
    p.n2 = d_n2;
    p.kp2 = d_kp2;
    p.desc2 = d_desc2;
    p.cam_index = cam_index;
    p.result = d_result;
    p.keypoint = d_keypoint;
    p.verdict = d_verdict;
    p.dist = d_dist;
    p.proj = d_proj;
    p.mask = d_mask;
    p.obs_uv = d_obs_uv;
    p.obs_pt = d_obs_pt;
    p.obs_cam = d_obs_cam;
    p.obs_info = d_obs_info;
    p.obs_start = reinterpret_cast<uint32_t*>(sc + l.obs_start);
    p.ba_count = reinterpret_cast<uint32_t*>(sc + l.ba_count);
    p.ba_pos3 = reinterpret_cast<float*>(sc + l.ba_pos3);
    p.ba_r9 = reinterpret_cast<float*>(sc + l.ba_r9);
    p.matched = reinterpret_cast<uint32_t*>(sc + l.matched);
    p.ba_points = reinterpret_cast<float*>(sc + l.ba_points);
    p.ba_uv = reinterpret_cast<float*>(sc + l.ba_uv);
    p.ba_info = reinterpret_cast<float*>(sc + l.ba_info);
    uint8_t* outlier = reinterpret_cast<uint8_t*>(sc + l.outlier);
    float* opt_pos3 = reinterpret_cast<float*>(sc + l.opt_pos3);
    float* opt_r9 = reinterpret_cast<float*>(sc + l.opt_r9);
    float* mean_sq = reinterpret_cast<float*>(sc + l.mean_sq);
    p.outlier = outlier;
    p.opt_pos3 = opt_pos3;
    p.opt_r9 = opt_r9;
    p.mean_sq = mean_sq;
    hipStream_t st = (hipStream_t)stream;
    // a problem that stops before the matching leaves its pose slot alone: the bundle adjustment
    // reads every problem's start
    MAGE_HIP(hipMemsetAsync(sc + l.ba_pos3, 0, l.matched - l.ba_pos3, st));
    launch("monoinit.third_match", mono_third_match_kernel, dim3(problems), dim3(M3_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    launch("monoinit.third_pack", mono_third_pack_kernel, dim3(problems), dim3(M3_THREADS), 0, st, p, problems);
    MAGE_HIP(hipGetLastError());
    const mage_status r =
        mage_ba_pose_batch_device(problems, p.ba_pos3, p.ba_r9, d_intr4, p.obs_start, p.ba_points, p.ba_uv, p.ba_info,
                                  p.c.steps, p.c.huber, p.c.max_error_sq, opt_pos3, opt_r9,
                                  reinterpret_cast<double*>(sc + l.opt_qt7), outlier, mean_sq, nullptr, stream);
    if (r != MAGE_OK) return r;
    launch("monoinit.third_finish", mono_third_finish_kernel, dim3(problems), dim3(M3_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

mage_status mage_mono_init_third_frame(const mage_mono_init_settings* settings, const float* intr4, const float* pos3,
                                       const float* r9, const float* points, uint32_t n_points, const int32_t* idx0,
                                       const int32_t* idx1, const uint8_t* desc0, uint32_t n0, const uint8_t* desc1,
                                       uint32_t n1, const mage_keypoint* kp2, const uint8_t* desc2, uint32_t n2,
                                       uint32_t cam_index, mage_mono_init_third_result* result, int32_t* keypoint,
                                       uint8_t* verdict, int32_t* dist, float* proj, uint8_t* mask, float* obs_uv,
                                       uint32_t* obs_pt, uint32_t* obs_cam, float* obs_info, uint8_t* outlier, int device)
{
    using namespace mage;
    const char* why = monothird::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(intr4 && pos3 && r9 && result, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE(n_points == 0 || (points && idx0 && idx1 && keypoint && verdict && dist && proj && obs_uv && obs_pt &&
                                   obs_cam && obs_info),
                 MAGE_EINVAL, "null argument");
    MAGE_REQUIRE((n0 == 0 || desc0) && (n1 == 0 || desc1) && (n2 == 0 || (kp2 && desc2 && mask)), MAGE_EINVAL,
                 "null argument");
    // over a limit: the kernel would say the same without the data
    if (n_points > (uint32_t)monothird::M3_MAX_POINTS || n2 > (uint32_t)monothird::M3_MAX_KP) {
        *result = mage_mono_init_third_result{};
        result->n_points = n_points;
        result->status = MAGE_M3_STATUS_OVER_LIMIT;
        return MAGE_OK;
    }
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    HostScratch* sp = host_scratch(device, SCRATCH_MONOTHIRD);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [inputs] | [outputs] | [scratch]: one copy each way
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t np = std::max(n_points, 1u), p0 = std::max(n0, 1u), p1 = std::max(n1, 1u), p2 = std::max(n2, 1u);
    const size_t ocnt = 0, opose = al(ocnt + 16), opts = al(opose + 4 * (4 + 6 + 18)), oi0 = al(opts + 12 * np),
                 oi1 = al(oi0 + 4 * np), od0 = al(oi1 + 4 * np), od1 = al(od0 + 32 * p0), okp = al(od1 + 32 * p1),
                 od2 = al(okp + 28 * p2), ores = al(od2 + 32 * p2), okey = al(ores + sizeof(mage_mono_init_third_result)),
                 over = al(okey + 4 * np), odist = al(over + np), oproj = al(odist + 8 * np), omask = al(oproj + 8 * np),
                 ouv = al(omask + p2),
                 oopt = al(ouv + 8 * np), ocam = al(oopt + 4 * np), oinfo = al(ocam + 4 * np), osc = al(oinfo + 4 * np);
    const monothird::Layout l = monothird::layout(1, np);
    const size_t total = osc + l.bytes;
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(total)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    uint32_t* cnt = reinterpret_cast<uint32_t*>(h + ocnt);
    cnt[0] = n_points;
    cnt[1] = n0;
    cnt[2] = n1;
    cnt[3] = n2;
    float* hp = reinterpret_cast<float*>(h + opose);
    std::memcpy(hp, intr4, 16);
    std::memcpy(hp + 4, pos3, 24);
    std::memcpy(hp + 10, r9, 72);
    if (n_points) {
        std::memcpy(h + opts, points, 12ull * n_points);
        std::memcpy(h + oi0, idx0, 4ull * n_points);
        std::memcpy(h + oi1, idx1, 4ull * n_points);
    }
    if (n0) std::memcpy(h + od0, desc0, 32ull * n0);
    if (n1) std::memcpy(h + od1, desc1, 32ull * n1);
    if (n2) {
        std::memcpy(h + okp, kp2, 28ull * n2);
        std::memcpy(h + od2, desc2, 32ull * n2);
    }
    MAGE_HIP(hipMemcpyAsync(b, h, ores, hipMemcpyHostToDevice, S.st));
    const uint32_t* dc = reinterpret_cast<const uint32_t*>(b + ocnt);
    const float* dp = reinterpret_cast<const float*>(b + opose);
    r = mage_mono_init_third_frame_batch_device(
        settings, 1, dp, dp + 4, dp + 10, reinterpret_cast<const float*>(b + opts), (uint32_t)np, dc,
        reinterpret_cast<const int32_t*>(b + oi0), reinterpret_cast<const int32_t*>(b + oi1),
        reinterpret_cast<const uint8_t*>(b + od0), (int64_t)p0, dc + 1, reinterpret_cast<const uint8_t*>(b + od1),
        (int64_t)p1, dc + 2, reinterpret_cast<const mage_keypoint*>(b + okp), reinterpret_cast<const uint8_t*>(b + od2),
        (int64_t)p2, dc + 3, cam_index, reinterpret_cast<mage_mono_init_third_result*>(b + ores),
        reinterpret_cast<int32_t*>(b + okey), reinterpret_cast<uint8_t*>(b + over), reinterpret_cast<int32_t*>(b + odist),
        reinterpret_cast<float*>(b + oproj),
        reinterpret_cast<uint8_t*>(b + omask), reinterpret_cast<float*>(b + ouv), reinterpret_cast<uint32_t*>(b + oopt),
        reinterpret_cast<uint32_t*>(b + ocam), reinterpret_cast<float*>(b + oinfo), b + osc, S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + ores, b + ores, osc + l.outlier + np - ores, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    const mage_mono_init_third_result R = *reinterpret_cast<const mage_mono_init_third_result*>(h + ores);
    *result = R;
    if (R.status != 0) return MAGE_OK;
    if (n_points) {
        std::memcpy(keypoint, h + okey, 4ull * n_points);
        std::memcpy(verdict, h + over, n_points);
        std::memcpy(dist, h + odist, 8ull * n_points);
        std::memcpy(proj, h + oproj, 8ull * n_points);
    }
    if (n2) std::memcpy(mask, h + omask, n2);
    const size_t na = R.n_associated;
    if (na) {
        std::memcpy(obs_uv, h + ouv, 8 * na);
        std::memcpy(obs_pt, h + oopt, 4 * na);
        std::memcpy(obs_cam, h + ocam, 4 * na);
        std::memcpy(obs_info, h + oinfo, 4 * na);
    }
    if (outlier && R.verdict != MAGE_M3_FEW_MATCHES && R.n_matched) std::memcpy(outlier, h + osc + l.outlier, R.n_matched);
    return MAGE_OK;
}

}  // extern "C"
