// keyframe_take.hpp — "points take keypoints of one keyframe, in order" on gfx950: the staging, the
// candidate gather and the in-order take that LocallyAssociateNewAssociations (newpoints_assoc.hip)
// and the cheap loop closure (loopclose.hip) run around TrackLocalMap::ProjectMapPointIntoCurrentFrame.
// One workgroup of KT_THREADS threads owns one keyframe at a time:
//   stage    the keyframe's x, y and mask bits in LDS and its keypoints listed by horizontal band (32
//            bands over the image height, a counting sort with ballot ranks, so the list is in
//            ascending keypoint index within a band);
//   gather   64 surviving points at a time, 4 lanes per point: a scan of the bands the point's box
//            touches (box, octave, available under the current mask, distance <= maxDist) into up
//            to 8 candidates per point — a superset of what the point can ever be offered, since
//            the mask only loses bits;
//   resolve  one wave takes the chunk's points in order with ordered_take.hpp's resolve_in_order
//            (the argument for its exactness is there).  A point with more than 8 candidates
//            rescans its bands instead of reading its list.
// The caller gates its points (one thread per point) and compacts the survivors in point order into
// px, py, pi, po between the two.  The bands are a counting sort and not the 64-bit key sort of
// band_index.hpp, which would not fit beside the taker table in 64 KiB of LDS.  Only commuting
// integer atomics, barriers and plain stores; nothing in the results depends on the order in which
// threads run, and every loop is bounded by the counts.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "ordered_take.hpp"

namespace mage {
namespace kt {

constexpr int KT_THREADS = 256;
constexpr int KT_WAVES = KT_THREADS / kWave;
constexpr int KT_MAX_KP = OT_MAX_TARGETS;  // keypoints per keyframe (mask bits in LDS)
constexpr int KT_CAP = 8;     // candidates kept per point (more: the point rescans its bands)
constexpr int KT_GROUP = 4;   // lanes per point in the gather
constexpr int KT_CHUNK = 64;  // points per gather + resolve round
constexpr int KT_BANDS = 32;  // horizontal bands of the keypoint list
constexpr int KT_BAD_OCT = 15;  // key octave of a keypoint no point can predict (predictions are 0..8)

// What the descriptor search reads of the settings.
struct Search {
    float radius;
    float band_scale;  // KT_BANDS / image height
    int max_dist, min_diff;
};

// The band of row y: monotone in y (a product with a positive constant, then a clamp), so every
// keypoint with y0 <= y <= y1 lies in bands band_of(y0) .. band_of(y1).  NaN goes to band 0.
__device__ __forceinline__ int band_of(float y, float scale)
{
    const float f = y * scale;
    return f >= 0.f ? (f < (float)KT_BANDS ? (int)f : KT_BANDS - 1) : 0;
}

// The workgroup's LDS arrays.
struct Shared {
    float x[KT_MAX_KP], y[KT_MAX_KP];
    uint16_t key[KT_MAX_KP];  // by band, ascending keypoint within a band: octave << 12 | keypoint
    int bstart[KT_BANDS + 1], brun[KT_BANDS];
    int wband[KT_WAVES][KT_BANDS];
    uint32_t m[KT_MAX_KP / 32];
    int taker[KT_MAX_KP];
    float px[KT_THREADS], py[KT_THREADS];
    int pi[KT_THREADS];  // the surviving points: index, octave
    signed char po[KT_THREADS];
    uint32_t ent[KT_CHUNK][KT_CAP];  // kept_entry(keypoint, distance)
    int n[KT_CHUNK];
    uint32_t wsum[KT_WAVES];
};

// The keyframe's nkp <= KT_MAX_KP keypoints in LDS, listed by band; available(t) says whether
// keypoint t < nkp is unassociated.  `extra` runs on thread 0 between the first two barriers (the
// caller's own per-keyframe LDS state).
template <typename Available, typename Extra>
__device__ __forceinline__ void stage_keyframe(float band_scale, int nkp, const mage_keypoint* kp, Shared& s,
                                               Available available, Extra extra)
{
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < KT_BANDS) s.bstart[tid + 1] = 0;
    if (tid == 0) s.bstart[0] = 0;
    __syncthreads();
    for (int i = tid; i < nkp; i += KT_THREADS) {
        const float y = kp[i].y;
        s.x[i] = kp[i].x;
        s.y[i] = y;
        atomicAdd(&s.bstart[band_of(y, band_scale) + 1], 1);
    }
    for (int i = tid; i < KT_MAX_KP; i += KT_THREADS) s.taker[i] = OT_NO_TAKER;
    for (int c0 = 0; c0 < KT_MAX_KP; c0 += KT_THREADS) {  // a wave's 64 mask bytes are two words (all 128 are written)
        const int t = c0 + tid;
        const unsigned long long bal = __ballot(t < nkp && available(t));
        if (lane == 0) {
            s.m[t >> 5] = (uint32_t)bal;
            s.m[(t >> 5) + 1] = (uint32_t)(bal >> 32);
        }
    }
    if (tid == 0) extra();
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int b = 0; b < KT_BANDS; b++) {
            s.brun[b] = acc;
            acc += s.bstart[b + 1];
            s.bstart[b + 1] = acc;
        }
    }
    __syncthreads();
    // the list: 256 keypoints at a time, each at its band's running base plus its rank among the
    // band's keypoints of the chunk
    for (int c0 = 0; c0 < nkp; c0 += KT_THREADS) {
        const int t = c0 + tid;
        const int b = t < nkp ? band_of(s.y[t], band_scale) : -1;
        const int o = b >= 0 ? kp[t].octave : 0;  // in flight over the ballots
        const int pos = rank_by_key<KT_WAVES>(b, true, KT_BANDS, s.brun, &s.wband[0][0], KT_BANDS);
        int add = 0;
        if (tid < KT_BANDS)
            for (int w = 0; w < KT_WAVES; w++) add += s.wband[w][tid];
        if (b >= 0) s.key[pos] = (uint16_t)((o >= 0 && o < KT_BAD_OCT ? o : KT_BAD_OCT) << 12 | t);
        __syncthreads();  // wband and brun are read: the next chunk may write them
        if (tid < KT_BANDS) s.brun[tid] += add;  // read again only after the next chunk's first barrier
    }
    __syncthreads();
}

// Compacts the gated points of one 256-point chunk in point order: thread's point i passed with
// projection (px, py) and octave oc.  Returns the survivors' count (a barrier inside).
__device__ __forceinline__ int compact(Shared& s, bool pass, float px, float py, int i, int oc)
{
    uint32_t cnt;
    const uint32_t pos = block_prefix<KT_WAVES>(pass, s.wsum, &cnt);
    if (pass) {
        s.px[pos] = px;
        s.py[pos] = py;
        s.pi[pos] = i;
        s.po[pos] = (signed char)oc;
    }
    __syncthreads();
    return (int)cnt;
}

// A surviving point's search: its box, its octave, its run of the band list, its descriptor.
struct Box {
    float x0, x1, y0, y1;
    int qo, lo, hi;
    uint4 a0, a1;
};

// desc_of(point index) -> the point's 32-byte query descriptor, 16-byte aligned.
template <typename DescOf>
__device__ __forceinline__ Box load_box(const Search& c, const Shared& s, int i, DescOf desc_of)
{
    const float r = c.radius, qx = s.px[i], qy = s.py[i];
    Box b;
    b.x0 = qx - r, b.x1 = qx + r, b.y0 = qy - r, b.y1 = qy + r;
    b.qo = s.po[i];
    b.lo = s.bstart[band_of(b.y0, c.band_scale)];
    b.hi = s.bstart[band_of(b.y1, c.band_scale) + 1];
    const uint8_t* qd = desc_of(s.pi[i]);
    b.a0 = *reinterpret_cast<const uint4*>(qd);
    b.a1 = *reinterpret_cast<const uint4*>(qd + 16);
    return b;
}

// Entries lo + first, lo + first + step, ... of the box's run: `visit(t, d)` for every keypoint in
// the box with the box's octave that is available under the current mask and within maxDist.
template <typename F>
__device__ __forceinline__ void scan(const Search& c, const uint8_t* kdesc, const Shared& s, const Box& b, int first,
                                     int step, F visit)
{
    for (int i = b.lo + first; i < b.hi; i += step) {
        const int key = s.key[i], t = key & 0xFFF;
        const float tx = s.x[t], ty = s.y[t];
        if (!(tx >= b.x0 && tx <= b.x1 && ty >= b.y0 && ty <= b.y1) || (key >> 12) != b.qo || !mask_bit(s.m, t)) continue;
        const int d = (int)hamming256(b.a0, b.a1, kdesc + 32ll * t);
        if (d <= c.max_dist) visit(t, d);
    }
}

// Surviving points s0 .. s0 + 63, 4 lanes per point walking the point's run 4 entries at a time: up
// to 8 candidates per point into ent, their number into n.
template <typename DescOf>
__device__ __forceinline__ void gather(const Search& c, const uint8_t* kdesc, Shared& s, int s0, int cnt, DescOf desc_of)
{
    const int j = threadIdx.x / KT_GROUP, sub = threadIdx.x % KT_GROUP;
    const bool act = s0 + j < cnt;
    Box b = {};
    if (act) b = load_box(c, s, s0 + j, desc_of);
    int n = 0;
    for (int i0 = b.lo; __any(i0 < b.hi); i0 += KT_GROUP) {
        bool f = false;
        uint32_t ent = 0;
        if (i0 + sub < b.hi) {
            Box one = b;  // this lane's entry alone
            one.lo = i0 + sub;
            one.hi = one.lo + 1;
            scan(c, kdesc, s, one, 0, 1, [&](int t, int d) {
                f = true;
                ent = kept_entry(t, d);
            });
        }
        const int pos = group_append<KT_GROUP>(f, sub, n);
        if (f && pos < KT_CAP) s.ent[j][pos] = ent;
    }
    if (act && sub == 0) s.n[j] = n;
}

// One wave: the chunk's cc points take their keypoints in order; commit(i, ok, t) once per point,
// i its place among the survivors (s.px[i], s.py[i], s.pi[i], s.po[i]).
template <typename DescOf, typename Commit>
__device__ __forceinline__ void resolve(const Search& c, const uint8_t* kdesc, Shared& s, int s0, int cc, DescOf desc_of,
                                        Commit commit)
{
    resolve_in_order(
        cc, c.max_dist, c.min_diff, s.m, s.taker,
        [&](int j, bool act) {
            const int n = act ? s.n[j] : 0;
            Box b = {};
            if (n > KT_CAP) b = load_box(c, s, s0 + j, desc_of);
            // every candidate of the lane that is still available (overflow: the bands rescanned)
            return [=, &c, &s](auto fn) {
                if (n <= KT_CAP) {
                    for (int e = 0; e < n; e++) {
                        const uint32_t v = s.ent[j][e];
                        if (mask_bit(s.m, kept_target(v))) fn(kept_target(v), kept_dist(v));
                    }
                } else {
                    scan(c, kdesc, s, b, 0, 1, fn);
                }
            };
        },
        [&](int j, bool ok, int t) { commit(s0 + j, ok, t); });
}

// The survivors of one gated chunk take their keypoints, 64 at a time (every thread calls it).
template <typename DescOf, typename Commit>
__device__ __forceinline__ void take_in_order(const Search& c, const uint8_t* kdesc, Shared& s, int cnt, DescOf desc_of,
                                              Commit commit)
{
    for (int s0 = 0; s0 < cnt; s0 += KT_CHUNK) {
        gather(c, kdesc, s, s0, cnt, desc_of);
        __syncthreads();
        if (threadIdx.x < kWave) resolve(c, kdesc, s, s0, min(KT_CHUNK, cnt - s0), desc_of, commit);
        __syncthreads();
    }
}

}  // namespace kt
}  // namespace mage
