// newpoints_assoc.hip — NewMapPointsCreation's LocallyAssociateNewAssociations on MI355X (gfx950).
//
// The reference (Core/MAGESLAM/Source/Mapping/NewMapPointsCreation.cpp:337-424) offers every new
// point, in push_back order, to every covisible keyframe it is not yet associated with: project,
// gate (TrackLocalMap::IsGoodCandidate), predict the octave, then the single-query RadiusMatch
// against the keyframe's still-unassociated keypoints; a success takes the keypoint for the later
// points.  State flows only through one keyframe's mask, so the keyframes are independent: one
// workgroup per (problem, keyframe).  It stages the keyframe's x, y and mask bits in LDS, lists the
// keypoints by horizontal band (32 bands over the image height, a counting sort with ballot ranks, so
// the list is in ascending keypoint index within a band), clears the keypoints
// CreateInitialAssociations took (:314), and takes the points 256 at a time:
//   gate      one thread per point (newpoints_math.hpp project_gate); a refused point's record and
//             verdict are final, the others are compacted in point order (ballot prefix);
//   gather    64 surviving points at a time, 4 lanes per point: a scan of the bands the point's box
//             touches (box, octave, available under the current mask, distance <= maxDist) into up
//             to 8 candidates per point — a superset of what the point can ever be offered, since
//             the mask only loses bits;
//   resolve   one wave, as localmap.hip's lm_resolve_kernel: each lane's result under the current
//             mask, the wanted keypoints marked with the lowest wanting lane (LDS atomicMin), the
//             lanes before the first one that sees an earlier lane's keypoint among its candidates
//             are final and commit, and the chunk restarts at that lane.  A point with more than 8
//             candidates rescans its bands instead of reading its list.
// The first build scanned all of the keyframe's keypoints per point (no index): 0.656 ms per launch
// on the shape of tools/bench_new_points_assoc.py (256 problems x 8 keyframes x 2000 keypoints), the
// ~nkp / 4 box tests per lane twice over (72 points are two rounds of 64) being nearly all of it.
// The bands cut the scan to the ~8 % of the keypoints near the point's row; they are a counting sort
// and not the 64-bit key sort of band_index.hpp, which would not fit beside the taker table in 64 KiB
// of LDS.  Only commuting integer atomics, barriers and plain stores; nothing in the results depends
// on the order in which threads run, and every loop is bounded by the counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "newpoints_math.hpp"

namespace mage {
namespace {

using namespace newpoints;

// The host-buffer entry's scratch slot, after newpoints.hip's (common.hpp stays as it is).
constexpr ScratchSlot SCRATCH_NEWPOINTS_ASSOC = static_cast<ScratchSlot>(6);

constexpr int NA_THREADS = 256;
constexpr int NA_WAVES = NA_THREADS / kWave;
constexpr int NA_CAP = 8;     // candidates kept per point (more: the point rescans its bands)
constexpr int NA_GROUP = 4;   // lanes per point in the gather
constexpr int NA_CHUNK = 64;  // points per gather + resolve round
constexpr int NA_BANDS = 32;  // horizontal bands of the keypoint list
constexpr int NA_BAD_OCT = 15;  // key octave of a keypoint no point can predict (predictions are 0..8)

struct NaParams {
    AssocConsts c;
    float band_scale;  // NA_BANDS / image height
    uint32_t kf_slots;
    const mage_new_point* points;
    uint32_t cap;
    const uint32_t* n_points;
    const uint8_t* ki_desc;
    long long ki_pitch;
    const uint32_t* n_ki;
    const uint32_t* n_kf;
    const float *kf_pos3, *kf_r9, *kf_intr4;
    const mage_keypoint* kf_kp;
    const uint8_t* kf_desc;
    uint8_t* kf_mask;
    long long kf_pitch;
    const uint32_t* n_kf_kp;
    const int32_t* kf_slot;
    mage_new_point_assoc* out;
    uint8_t* verdict;
    uint32_t* status;
};

__device__ __forceinline__ uint32_t hamming32(const uint4& a0, const uint4& a1, const uint8_t* b)
{
    const uint4 b0 = *reinterpret_cast<const uint4*>(b), b1 = *reinterpret_cast<const uint4*>(b + 16);
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

__device__ __forceinline__ bool bit(const uint32_t* w, int t) { return (w[t >> 5] >> (t & 31)) & 1u; }

// The band of row y: monotone in y (a product with a positive constant, then a clamp), so every
// keypoint with y0 <= y <= y1 lies in bands band_of(y0) .. band_of(y1).  NaN goes to band 0.
__device__ __forceinline__ int band_of(float y, float scale)
{
    const float f = y * scale;
    return f >= 0.f ? (f < (float)NA_BANDS ? (int)f : NA_BANDS - 1) : 0;
}

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(NA_THREADS) void new_points_assoc_kernel(NaParams p)
{
    __shared__ float s_x[NA_MAX_KP], s_y[NA_MAX_KP];
    __shared__ uint16_t s_key[NA_MAX_KP];  // by band, ascending keypoint within a band: octave << 12 | keypoint
    __shared__ int s_bstart[NA_BANDS + 1], s_brun[NA_BANDS];
    __shared__ int s_wband[NA_WAVES][NA_BANDS];
    __shared__ uint32_t s_m[NA_MAX_KP / 32];
    __shared__ int s_taker[NA_MAX_KP];
    __shared__ Frame s_frame;
    __shared__ float s_px[NA_THREADS], s_py[NA_THREADS];
    __shared__ int s_pi[NA_THREADS];  // the surviving points: index, octave
    __shared__ signed char s_po[NA_THREADS];
    __shared__ uint32_t s_ent[NA_CHUNK][NA_CAP];        // keypoint << 9 | distance
    __shared__ int s_n[NA_CHUNK];
    __shared__ uint32_t s_wsum[NA_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t prob = blockIdx.x / p.kf_slots, k = blockIdx.x % p.kf_slots;
    const long long pair = blockIdx.x;
    const uint32_t nkf = p.n_kf[prob], npts = min(p.n_points[prob], p.cap);
    if (nkf <= p.kf_slots && k >= nkf) return;
    const uint32_t nkp = p.n_kf_kp[pair];
    const long long stride = p.kf_slots, o0 = (long long)prob * p.cap * stride + k;
    mage_new_point_assoc* out = p.out + o0;
    uint8_t* verdict = p.verdict + o0;
    if (nkf > p.kf_slots || nkp > (uint32_t)NA_MAX_KP || (long long)nkp > p.kf_pitch) {  // uniform over the workgroup
        if (tid == 0) atomicOr(p.status, 1u);
        for (uint32_t i = tid; i < npts; i += NA_THREADS) out[i * stride] = mage_new_point_assoc{0.f, 0.f, 0, -1};
        return;
    }
    const mage_new_point* pts = p.points + (long long)prob * p.cap;
    const mage_keypoint* kp = p.kf_kp + pair * p.kf_pitch;
    const uint8_t* kdesc = p.kf_desc + 32ll * pair * p.kf_pitch;
    uint8_t* mask = p.kf_mask + pair * p.kf_pitch;
    const uint8_t* kidesc = p.ki_desc + 32ll * prob * p.ki_pitch;
    const uint32_t nki = (uint32_t)min((long long)p.n_ki[prob], p.ki_pitch);
    const int slot = p.kf_slot[pair];
    const float* intr = p.kf_intr4 + 4 * pair;

    // the keyframe in LDS, and the band populations
    if (tid < NA_BANDS) s_bstart[tid + 1] = 0;
    if (tid == 0) s_bstart[0] = 0;
    __syncthreads();
    for (int i = tid; i < (int)nkp; i += NA_THREADS) {
        const float y = kp[i].y;
        s_x[i] = kp[i].x;
        s_y[i] = y;
        atomicAdd(&s_bstart[band_of(y, p.band_scale) + 1], 1);
    }
    for (int i = tid; i < NA_MAX_KP; i += NA_THREADS) s_taker[i] = 64;
    for (int c0 = 0; c0 < NA_MAX_KP; c0 += NA_THREADS) {  // a wave's 64 mask bytes are two words (all 128 are written)
        const int t = c0 + tid;
        const unsigned long long bal = __ballot(t < (int)nkp && mask[t] != 0);
        if (lane == 0) {
            s_m[t >> 5] = (uint32_t)bal;
            s_m[(t >> 5) + 1] = (uint32_t)(bal >> 32);
        }
    }
    if (tid == 0) {
        Frame f;
        make_frame(p.kf_pos3 + 3 * pair, p.kf_r9 + 9 * pair, intr, f);
        s_frame = f;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int b = 0; b < NA_BANDS; b++) {
            s_brun[b] = acc;
            acc += s_bstart[b + 1];
            s_bstart[b + 1] = acc;
        }
    }
    __syncthreads();
    // the list: 256 keypoints at a time, each one's rank among its band's keypoints of the chunk by
    // wave ballots plus the band's running base
    for (int c0 = 0; c0 < (int)nkp; c0 += NA_THREADS) {
        const int t = c0 + tid;
        const int b = t < (int)nkp ? band_of(s_y[t], p.band_scale) : -1;
        const int o = b >= 0 ? kp[t].octave : 0;  // in flight over the ballots
        int rank = 0;
        for (int c = 0; c < NA_BANDS; c++) {
            const unsigned long long bal = __ballot(b == c);
            if (lane == 0) s_wband[wave][c] = __popcll(bal);
            if (b == c) rank = __popcll(bal & ((1ull << lane) - 1ull));
        }
        __syncthreads();
        int add = 0;
        if (tid < NA_BANDS)
            for (int w = 0; w < NA_WAVES; w++) add += s_wband[w][tid];
        if (b >= 0) {
            int pos = s_brun[b] + rank;
            for (int w = 0; w < wave; w++) pos += s_wband[w][b];
            s_key[pos] = (uint16_t)((o >= 0 && o < NA_BAD_OCT ? o : NA_BAD_OCT) << 12 | t);
        }
        __syncthreads();  // s_wband and s_brun are read: the next chunk may write them
        if (tid < NA_BANDS) s_brun[tid] += add;  // read again only after the next chunk's first barrier
    }
    __syncthreads();
    // CreateInitialAssociations' own associations with this keyframe (:314)
    if (slot >= 0)
        for (uint32_t i = tid; i < npts; i += NA_THREADS) {
            const uint32_t s = pts[i].kc_slot, q = pts[i].kc_index;
            if (s == (uint32_t)slot && q < nkp) atomicAnd(&s_m[q >> 5], ~(1u << (q & 31)));
        }
    __syncthreads();

    const float r = p.c.radius;
    const int maxd = p.c.max_dist, mind = p.c.min_diff;
    for (uint32_t c0 = 0; c0 < npts; c0 += NA_THREADS) {
        // gate: one thread per point
        const uint32_t i = c0 + tid;
        bool pass = false;
        float px = 0.f, py = 0.f;
        int oc = 0;
        if (i < npts) {
            const mage_new_point pt = pts[i];
            uint8_t v;
            if (pt.ki_index >= nki || pt.kc_slot >= (uint32_t)NP_MAX_SLOTS)
                v = NA_BAD_INDEX;
            else if (slot >= 0 && pt.kc_slot == (uint32_t)slot)
                v = pt.kc_index < nkp ? NA_SAME_FRAME : NA_BAD_INDEX;
            else {
                v = project_gate(p.c, s_frame, intr, pt, px, py, oc);
                pass = v == NA_NO_MATCH;
            }
            if (!pass) {
                out[i * stride] = mage_new_point_assoc{px, py, oc, -1};
                verdict[i * stride] = v;
            }
        }
        const unsigned long long bal = __ballot(pass);
        if (lane == 0) s_wsum[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        int off = 0, cnt = 0;
        for (int w = 0; w < NA_WAVES; w++) {
            off += w < wave ? (int)s_wsum[w] : 0;
            cnt += (int)s_wsum[w];
        }
        if (pass) {
            const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
            s_px[pos] = px;
            s_py[pos] = py;
            s_pi[pos] = (int)i;
            s_po[pos] = (signed char)oc;
        }
        __syncthreads();

        for (int s0 = 0; s0 < cnt; s0 += NA_CHUNK) {
            // gather: 4 lanes per point walk the point's bands 4 keypoints at a time
            {
                const int j = tid / NA_GROUP, sub = tid % NA_GROUP, gbase = lane & ~(NA_GROUP - 1);
                const bool act = s0 + j < cnt;
                float x0 = 0.f, x1 = 0.f, y0 = 0.f, y1 = 0.f;
                int qo = -2, lo = 0, hi = 0;
                uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
                if (act) {
                    const float qx = s_px[s0 + j], qy = s_py[s0 + j];
                    x0 = qx - r, x1 = qx + r, y0 = qy - r, y1 = qy + r;
                    qo = s_po[s0 + j];
                    lo = s_bstart[band_of(y0, p.band_scale)];
                    hi = s_bstart[band_of(y1, p.band_scale) + 1];
                    const uint8_t* qd = kidesc + 32ll * pts[s_pi[s0 + j]].ki_index;
                    a0 = *reinterpret_cast<const uint4*>(qd);
                    a1 = *reinterpret_cast<const uint4*>(qd + 16);
                }
                int n = 0;
                for (int i0 = lo; __any(i0 < hi); i0 += NA_GROUP) {
                    const int e = i0 + sub;
                    bool f = false;
                    uint32_t ent = 0;
                    if (e < hi) {
                        const int key = s_key[e], t = key & 0xFFF;
                        const float tx = s_x[t], ty = s_y[t];
                        if (tx >= x0 && tx <= x1 && ty >= y0 && ty <= y1 && (key >> 12) == qo && bit(s_m, t)) {
                            const uint32_t d = hamming32(a0, a1, kdesc + 32ll * t);
                            if ((int)d <= maxd) {
                                f = true;
                                ent = (uint32_t)t << 9 | d;
                            }
                        }
                    }
                    const unsigned long long b = __ballot(f);
                    const uint32_t gb = (uint32_t)(b >> gbase) & ((1u << NA_GROUP) - 1u);
                    const int pos = n + __popc(gb & ((1u << sub) - 1u));
                    if (f && pos < NA_CAP) s_ent[j][pos] = ent;
                    n += __popc(gb);
                }
                if (act && sub == 0) s_n[j] = n;
            }
            __syncthreads();
            // resolve: one wave, the chunk's points in order
            if (wave == 0) {
                const int cc = min(NA_CHUNK, cnt - s0);
                int r0 = 0;
                while (r0 < cc) {
                    const int j = r0 + lane;
                    const bool act = j < cc;
                    const int n = act ? s_n[j] : 0;
                    const bool over = n > NA_CAP;
                    float x0 = 0.f, x1 = 0.f, y0 = 0.f, y1 = 0.f;
                    int qo = -2, lo = 0, hi = 0;
                    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
                    if (over) {
                        const float qx = s_px[s0 + j], qy = s_py[s0 + j];
                        x0 = qx - r, x1 = qx + r, y0 = qy - r, y1 = qy + r;
                        qo = s_po[s0 + j];
                        lo = s_bstart[band_of(y0, p.band_scale)];
                        hi = s_bstart[band_of(y1, p.band_scale) + 1];
                        const uint8_t* qd = kidesc + 32ll * pts[s_pi[s0 + j]].ki_index;
                        a0 = *reinterpret_cast<const uint4*>(qd);
                        a1 = *reinterpret_cast<const uint4*>(qd + 16);
                    }
                    // every candidate of the lane that is still available (overflow: the bands rescanned)
                    auto each = [&](auto fn) {
                        if (!act) return;
                        if (!over) {
                            for (int e = 0; e < n; e++) {
                                const uint32_t v = s_ent[j][e];
                                const int t = (int)(v >> 9);
                                if (bit(s_m, t)) fn(t, (int)(v & 0x1FFu));
                            }
                        } else {
                            for (int i = lo; i < hi; i++) {
                                const int key = s_key[i], t = key & 0xFFF;
                                const float tx = s_x[t], ty = s_y[t];
                                if (!(tx >= x0 && tx <= x1 && ty >= y0 && ty <= y1) || (key >> 12) != qo || !bit(s_m, t))
                                    continue;
                                const int d = (int)hamming32(a0, a1, kdesc + 32ll * t);
                                if (d <= maxd) fn(t, d);
                            }
                        }
                    };
                    uint32_t bestk = 0xFFFFFFFFu;
                    each([&](int t, int d) { bestk = min(bestk, (uint32_t)d << 12 | (uint32_t)t); });
                    const int tb = (int)(bestk & 0xFFFu), best = (int)(bestk >> 12);
                    int sec = maxd + 1;
                    each([&](int t, int d) {
                        if (t < tb) sec = min(sec, d);
                    });
                    const bool ok = bestk != 0xFFFFFFFFu && sec - best > mind;
                    if (ok) atomicMin(&s_taker[tb], lane);
                    wave_sync();
                    bool conflict = false;
                    each([&](int t, int) {
                        if (s_taker[t] < lane) conflict = true;
                    });
                    const unsigned long long cb = __ballot(conflict);
                    const int f = cb ? __builtin_ctzll(cb) : 64;
                    if (act && lane < f) {
                        if (ok) atomicAnd(&s_m[tb >> 5], ~(1u << (tb & 31)));
                        const long long o = (long long)s_pi[s0 + j] * stride;
                        out[o] = mage_new_point_assoc{s_px[s0 + j], s_py[s0 + j], s_po[s0 + j], ok ? tb : -1};
                        verdict[o] = ok ? (uint8_t)NA_ASSOCIATED : (uint8_t)NA_NO_MATCH;
                    }
                    wave_sync();
                    if (ok) s_taker[tb] = 64;
                    wave_sync();
                    r0 += f;
                }
            }
            __syncthreads();
        }
    }
    // the taken keypoints (the claims included) back to the mask bytes
    for (int t = tid; t < (int)nkp; t += NA_THREADS)
        if (!bit(s_m, t)) mask[t] = 0;
}

}  // namespace
}  // namespace mage

extern "C" {

mage_status mage_new_points_associate_batch_device(
    const mage_new_points_settings* settings, const mage_new_points_assoc_settings* assoc, uint32_t problems,
    uint32_t kf_slots, const mage_new_point* d_points, uint32_t cap, const uint32_t* d_n_points, const uint8_t* d_ki_desc,
    int64_t ki_pitch, const uint32_t* d_n_ki, const uint32_t* d_n_kf, const float* d_kf_pos3, const float* d_kf_r9,
    const float* d_kf_intr4, const mage_keypoint* d_kf_kp, const uint8_t* d_kf_desc, uint8_t* d_kf_mask, int64_t kf_pitch,
    const uint32_t* d_n_kf_kp, const int32_t* d_kf_slot, mage_new_point_assoc* d_assoc, uint8_t* d_verdict,
    uint32_t* d_status, mage_stream stream)
{
    using namespace mage;
    const char* why = newpoints::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    why = newpoints::check_assoc_settings(assoc);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    if (problems == 0 || kf_slots == 0) return MAGE_OK;
    MAGE_REQUIRE(d_points && d_n_points && d_ki_desc && d_n_ki && d_n_kf && d_kf_pos3 && d_kf_r9 && d_kf_intr4 &&
                     d_kf_kp && d_kf_desc && d_kf_mask && d_n_kf_kp && d_kf_slot && d_assoc && d_verdict && d_status,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(ki_pitch > 0 && kf_pitch > 0 && cap > 0, MAGE_EINVAL, "pitches and capacities must be positive");
    MAGE_REQUIRE((uint64_t)problems * kf_slots <= 0x7FFFFFFFull, MAGE_EINVAL, "too many (problem, keyframe) pairs");
    MAGE_REQUIRE(reinterpret_cast<uintptr_t>(d_ki_desc) % 16 == 0 && reinterpret_cast<uintptr_t>(d_kf_desc) % 16 == 0,
                 MAGE_EINVAL, "descriptor pointers must be 16-byte aligned");
    NaParams p{};
    p.c = newpoints::make_assoc_consts(*settings, *assoc);
    p.band_scale = (float)NA_BANDS / p.c.image_h;
    p.kf_slots = kf_slots;
    p.points = d_points;
    p.cap = cap;
    p.n_points = d_n_points;
    p.ki_desc = d_ki_desc;
    p.ki_pitch = ki_pitch;
    p.n_ki = d_n_ki;
    p.n_kf = d_n_kf;
    p.kf_pos3 = d_kf_pos3;
    p.kf_r9 = d_kf_r9;
    p.kf_intr4 = d_kf_intr4;
    p.kf_kp = d_kf_kp;
    p.kf_desc = d_kf_desc;
    p.kf_mask = d_kf_mask;
    p.kf_pitch = kf_pitch;
    p.n_kf_kp = d_n_kf_kp;
    p.kf_slot = d_kf_slot;
    p.out = d_assoc;
    p.verdict = d_verdict;
    p.status = d_status;
    launch("newpoints.associate", new_points_assoc_kernel, dim3(problems * kf_slots), dim3(NA_THREADS), 0,
           (hipStream_t)stream, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

mage_status mage_new_points_associate(const mage_new_points_settings* settings,
                                      const mage_new_points_assoc_settings* assoc, const mage_new_point* points,
                                      uint32_t n_points, const uint8_t* ki_desc, uint32_t n_ki, uint32_t n_kf,
                                      const float* kf_pos3, const float* kf_r9, const float* kf_intr4,
                                      const mage_keypoint* kf_kp, const uint8_t* kf_desc, const uint32_t* kf_start,
                                      const int32_t* kf_slot, uint8_t* kf_mask, mage_new_point_assoc* out,
                                      uint8_t* verdict, uint32_t* status, int device)
{
    using namespace mage;
    const char* why = newpoints::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    why = newpoints::check_assoc_settings(assoc);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(status, MAGE_EINVAL, "null argument");
    *status = 0;
    if (n_points == 0 || n_kf == 0) return MAGE_OK;
    MAGE_REQUIRE(points && out && verdict && kf_pos3 && kf_r9 && kf_intr4 && kf_start && kf_slot && (n_ki == 0 || ki_desc),
                 MAGE_EINVAL, "null argument");
    uint32_t pitch = 1;
    for (uint32_t k = 0; k < n_kf; k++) {
        MAGE_REQUIRE(kf_start[k] <= kf_start[k + 1], MAGE_EINVAL, "start offsets must not decrease");
        MAGE_REQUIRE(kf_slot[k] >= -1 && kf_slot[k] < newpoints::NP_MAX_SLOTS, MAGE_EINVAL, "kf_slot must be in [-1, 7]");
        const uint32_t nk = kf_start[k + 1] - kf_start[k];
        if (nk <= (uint32_t)newpoints::NA_MAX_KP) pitch = std::max(pitch, nk);
    }
    MAGE_REQUIRE(kf_start[n_kf] == kf_start[0] || (kf_kp && kf_desc && kf_mask), MAGE_EINVAL, "null argument");
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    HostScratch* sp = host_scratch(device, SCRATCH_NEWPOINTS_ASSOC);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [points][ki desc][counts][poses][kf kp][kf desc] | [masks][status][verdicts] | [records]:
    // everything up to the records in one H2D copy (the verdict bytes of a keyframe over the limit
    // are the caller's), the masks and outputs back in one D2H copy.  A keyframe over the limit keeps
    // its count and sends no data.
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t nkf = n_kf, np = n_points, kip = std::max(n_ki, 1u);
    const size_t opts = 0, okid = al(opts + 48 * np), ocnt = al(okid + 32 * kip), opose = al(ocnt + 4 * (3 + 2 * nkf)),
                 okp = al(opose + 64 * nkf), okd = al(okp + 28 * nkf * pitch), omask = al(okd + 32 * nkf * pitch),
                 ost = al(omask + nkf * pitch), over = al(ost + 4), orec = al(over + np * nkf),
                 total = al(orec + 16 * np * nkf);
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(total)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    std::memset(h, 0, over);
    std::memcpy(h + opts, points, 48 * np);
    if (n_ki) std::memcpy(h + okid, ki_desc, 32ull * n_ki);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(h + ocnt);  // [n_points, n_ki, n_kf, n_kf_kp x n_kf, kf_slot x n_kf]
    cnt[0] = n_points;
    cnt[1] = n_ki;
    cnt[2] = n_kf;
    float* hp = reinterpret_cast<float*>(h + opose);  // [pos3 x n_kf | r9 x n_kf | intr4 x n_kf]
    std::memcpy(hp, kf_pos3, 12 * nkf);
    std::memcpy(hp + 3 * nkf, kf_r9, 36 * nkf);
    std::memcpy(hp + 12 * nkf, kf_intr4, 16 * nkf);
    for (uint32_t k = 0; k < n_kf; k++) {
        const uint32_t nk = kf_start[k + 1] - kf_start[k];
        cnt[3 + k] = nk;
        cnt[3 + nkf + k] = (uint32_t)kf_slot[k];
        if (nk == 0 || nk > (uint32_t)newpoints::NA_MAX_KP) continue;
        std::memcpy(h + okp + 28 * (k * (size_t)pitch), kf_kp + kf_start[k], 28ull * nk);
        std::memcpy(h + okd + 32 * (k * (size_t)pitch), kf_desc + 32ull * kf_start[k], 32ull * nk);
        std::memcpy(h + omask + k * (size_t)pitch, kf_mask + kf_start[k], nk);
    }
    std::memcpy(h + over, verdict, np * nkf);
    MAGE_HIP(hipMemcpyAsync(b, h, orec, hipMemcpyHostToDevice, S.st));
    const uint32_t* dc = reinterpret_cast<const uint32_t*>(b + ocnt);
    const float* dp = reinterpret_cast<const float*>(b + opose);
    r = mage_new_points_associate_batch_device(
        settings, assoc, 1, n_kf, reinterpret_cast<const mage_new_point*>(b + opts), n_points, dc,
        reinterpret_cast<const uint8_t*>(b + okid), (int64_t)kip, dc + 1, dc + 2, dp, dp + 3 * nkf, dp + 12 * nkf,
        reinterpret_cast<const mage_keypoint*>(b + okp), reinterpret_cast<const uint8_t*>(b + okd),
        reinterpret_cast<uint8_t*>(b + omask), pitch, dc + 3, reinterpret_cast<const int32_t*>(dc + 3 + nkf),
        reinterpret_cast<mage_new_point_assoc*>(b + orec), reinterpret_cast<uint8_t*>(b + over),
        reinterpret_cast<uint32_t*>(b + ost), S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + omask, b + omask, total - omask, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    *status = *reinterpret_cast<const uint32_t*>(h + ost);
    std::memcpy(verdict, h + over, np * nkf);
    std::memcpy(out, h + orec, 16 * np * nkf);
    for (uint32_t k = 0; k < n_kf; k++) {
        const uint32_t nk = kf_start[k + 1] - kf_start[k];
        if (nk && nk <= (uint32_t)newpoints::NA_MAX_KP) std::memcpy(kf_mask + kf_start[k], h + omask + k * (size_t)pitch, nk);
    }
    return MAGE_OK;
}

}  // extern "C"
