// ordered_take.hpp — device helpers for "items take from a pool in order" on gfx950 (wave64).
//
// TrackLocalMap (localmap.hip) and LocallyAssociateNewAssociations (newpoints_assoc.hip) are the same
// sequential loop in the reference: items are offered, in order, to a pool of still-unassociated
// keypoints; each item takes its best keypoint under the single-query RadiusMatch rule
// (FeatureMatcher.cpp:386-446), and every later item sees that keypoint gone.  resolve_in_order runs
// that loop exactly and in parallel, one wave, 64 items per round:
//   1. every lane computes its item's result under the current mask;
//   2. a lane that would take keypoint t marks it with its lane number (LDS atomicMin: the lowest
//      taking lane stays);
//   3. a lane that finds a lower lane's mark on any of its own candidates is in conflict: that
//      earlier item may take a keypoint this lane's result was computed with;
//   4. the lanes before the first conflicting lane are final and commit (a taken keypoint leaves the
//      mask); the marks are reset and the next round starts at the conflicting lane.
// This is the sequential outcome: an item's result depends on the earlier items only through the
// keypoints they take out of its candidate set.  A final lane has no earlier lane's mark among its
// candidates, so no earlier lane of the round takes from its set, and all items before the round
// are committed already: its result is what the sequential loop computes.  Lane r0 never conflicts
// (no lower lane is active), so every round commits at least one item and the loop ends.
// The reference's "second best = the previous best" rule (:425-437) is taken in ascending keypoint
// order (the R*-tree's visiting order is unspecified), where it is order-free:
// best = min (distance, index), second = min(maxDist + 1, min distance over lower indices).
// Only commuting integer atomics, wave barriers and plain stores: nothing depends on the order in
// which lanes run.
//
// The other helpers are the ordered compactions around that loop.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mage {

// The two packings.  Best key d << OT_TARGET_BITS | t: unsigned min is min (distance, index).  Kept
// candidate t << OT_DIST_BITS | d.  Callers assert their keypoint limit against OT_MAX_TARGETS.
constexpr int OT_TARGET_BITS = 12, OT_DIST_BITS = 9;
constexpr int OT_MAX_TARGETS = 1 << OT_TARGET_BITS;  // keypoints in the pool (mask bits, taker entries)
constexpr int OT_MAX_DIST = 256;                     // a 256-bit descriptor's largest distance
constexpr uint32_t OT_NO_BEST = 0xFFFFFFFFu;
constexpr int OT_NO_TAKER = 64;  // the taker table's idle value: above every lane
static_assert(OT_MAX_DIST < (1 << OT_DIST_BITS), "a distance must fit the kept entry's low bits");
static_assert(((uint64_t)OT_MAX_DIST << OT_TARGET_BITS | (OT_MAX_TARGETS - 1)) < OT_NO_BEST, "best key overflows");
static_assert(((uint64_t)(OT_MAX_TARGETS - 1) << OT_DIST_BITS | OT_MAX_DIST) <= 0xFFFFFFFFull, "kept entry overflows");

__device__ __forceinline__ uint32_t kept_entry(int t, int d) { return (uint32_t)t << OT_DIST_BITS | (uint32_t)d; }
__device__ __forceinline__ int kept_target(uint32_t v) { return (int)(v >> OT_DIST_BITS); }
__device__ __forceinline__ int kept_dist(uint32_t v) { return (int)(v & ((1u << OT_DIST_BITS) - 1u)); }

// Hamming distance of two 256-bit descriptors (16-byte aligned); a0, a1: the first one's halves.
__device__ __forceinline__ uint32_t hamming256(const uint4& a0, const uint4& a1, const uint8_t* b)
{
    const uint4 b0 = *reinterpret_cast<const uint4*>(b), b1 = *reinterpret_cast<const uint4*>(b + 16);
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

__device__ __forceinline__ uint32_t hamming256(const uint8_t* a, const uint8_t* b)
{
    return hamming256(*reinterpret_cast<const uint4*>(a), *reinterpret_cast<const uint4*>(a + 16), b);
}

__device__ __forceinline__ bool mask_bit(const uint32_t* w, int t) { return (w[t >> 5] >> (t & 31)) & 1u; }
__device__ __forceinline__ void mask_clear(uint32_t* w, int t) { atomicAnd(&w[t >> 5], ~(1u << (t & 31))); }

// The wave's LDS writes before this point are visible to its lanes after it.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Exclusive position of this thread's item among the block's items with pred set, in thread order;
// *total = their count.  A block of WAVES waves, all of which call it; wsum: WAVES words of LDS.
// The second barrier makes back-to-back calls safe.
template <int WAVES>
__device__ __forceinline__ uint32_t block_prefix(bool pred, uint32_t* wsum, uint32_t* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t b = __ballot(pred);
    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (lane == 0) wsum[wave] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t woff = 0, tot = 0;
    for (int w = 0; w < WAVES; w++) {
        if (w < wave) woff += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();
    *total = tot;
    return woff + before;
}

// GROUP adjacent lanes (lane % GROUP == sub) append their found candidates to the group's list of n
// entries: the position of this lane's candidate, in lane order; n advances by the group's count.
// Every lane of the wave calls it.
template <int GROUP>
__device__ __forceinline__ int group_append(bool found, int sub, int& n)
{
    static_assert(GROUP <= 32 && 64 % GROUP == 0, "a group is part of one wave");
    const int gbase = (threadIdx.x & 63) - sub;
    const uint32_t gb = (uint32_t)(__ballot(found) >> gbase) & (uint32_t)((1ull << GROUP) - 1ull);
    const int pos = n + __popc(gb & ((1u << sub) - 1u));
    n += __popc(gb);
    return pos;
}

// Stable rank by a small key in 0..nkeys-1: this thread's position among the block's threads with
// the same key and `counted` set, in thread order, on top of base[key]; 0 for a negative key (a
// thread without one).  wcount: WAVES rows of `stride` >= nkeys ints of LDS, left holding each
// wave's count per key; the caller adds them to base[] once every thread has its rank (a barrier
// later).  One barrier inside.
template <int WAVES>
__device__ __forceinline__ int rank_by_key(int key, bool counted, int nkeys, const int* base, int* wcount, int stride)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rank = 0;
    for (int c = 0; c < nkeys; c++) {
        const uint64_t bal = __ballot(counted && key == c);
        if (lane == 0) wcount[wave * stride + c] = __popcll(bal);
        if (key == c) rank = __popcll(bal & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (key >= 0) {
        rank += base[key];
        for (int w = 0; w < wave; w++) rank += wcount[w * stride + key];
    }
    return rank;
}

// The in-order take of `count` items by one wave (all 64 lanes call it; see the file header).
//   mask   LDS bit words of the pool, a set bit = available; a taken keypoint's bit is cleared here
//   taker  LDS, one int per keypoint, all OT_NO_TAKER on entry and on return
//   load(k, act) -> each   called once per round for the lane's item k (act: k < count); returns a
//                  callable each(fn) that calls fn(t, d) for every candidate t of the item that is
//                  available under the current mask, d <= max_dist its distance; nothing if !act.
//                  It is run three times per round and must visit the same set while the mask
//                  does not change.
//   commit(k, ok, t)   called once per item, in a round where the item is final: it took t (ok) or
//                  nothing.
template <typename Load, typename Commit>
__device__ __forceinline__ void resolve_in_order(int count, int max_dist, int min_diff, uint32_t* mask, int* taker,
                                                 Load load, Commit commit)
{
    const int lane = threadIdx.x & 63;
    int r0 = 0;
    while (r0 < count) {
        const int k = r0 + lane;
        const bool act = k < count;
        auto each = load(k, act);
        uint32_t bestk = OT_NO_BEST;
        each([&](int t, int d) { bestk = min(bestk, (uint32_t)d << OT_TARGET_BITS | (uint32_t)t); });
        const int tb = (int)(bestk & (uint32_t)(OT_MAX_TARGETS - 1)), best = (int)(bestk >> OT_TARGET_BITS);
        int sec = max_dist + 1;
        each([&](int t, int d) {
            if (t < tb) sec = min(sec, d);
        });
        const bool ok = bestk != OT_NO_BEST && sec - best > min_diff;
        if (ok) atomicMin(&taker[tb], lane);
        wave_sync();
        bool conflict = false;
        each([&](int t, int) {
            if (taker[t] < lane) conflict = true;
        });
        const uint64_t cb = __ballot(conflict);
        const int f = cb ? __builtin_ctzll(cb) : 64;
        if (act && lane < f) {
            if (ok) mask_clear(mask, tb);
            commit(k, ok, tb);
        }
        wave_sync();
        if (ok) taker[tb] = OT_NO_TAKER;
        wave_sync();
        r0 += f;
    }
}

// ---------------------------------------------------------------------------------------------
// Two queries per item (the third frame of the monocular map initialisation,
// MapInitialization.cpp:730-799): every item looks its position up twice against the same mask
// state, each query under its own maxDist / minDiff, and takes the keypoint of the better match —
// query 1's only when both matched and its distance is strictly smaller, or when it alone matched.
// The round protocol is resolve_in_order's, and so is the argument: an item's outcome (both queries'
// results and hence the keypoint it takes) depends on the earlier items only through the keypoints
// they take out of the union of its two candidate sets.  A lane is therefore in conflict when a
// lower lane's mark sits on a candidate of EITHER query; a final lane has no earlier lane's mark in
// that union, all items before the round are committed, and its outcome is the sequential loop's.
// A lane marks only the one keypoint it would take (the winner's): the loser's match stays in the
// pool, as in the reference.  Lane r0 never conflicts, so every round commits at least one item.
// ---------------------------------------------------------------------------------------------

// A kept candidate of a two-query item: t << 18 | d0 << 9 | d1.
static_assert(OT_TARGET_BITS + 2 * OT_DIST_BITS <= 32, "a two-query kept entry must fit a word");
__device__ __forceinline__ uint32_t kept_entry2(int t, int d0, int d1)
{
    return (uint32_t)t << (2 * OT_DIST_BITS) | (uint32_t)d0 << OT_DIST_BITS | (uint32_t)d1;
}
__device__ __forceinline__ int kept_target2(uint32_t v) { return (int)(v >> (2 * OT_DIST_BITS)); }
__device__ __forceinline__ int kept_dist2(uint32_t v, int q)
{
    return (int)(v >> (q ? 0 : OT_DIST_BITS) & ((1u << OT_DIST_BITS) - 1u));
}

// The in-order take of `count` two-query items by one wave (all 64 lanes call it).  mask, taker: as
// resolve_in_order.
//   load(k, act) -> each   as resolve_in_order's, but fn(t, d0, d1) gets the candidate's distance to
//                  both queries, for every available candidate with d0 <= max_dist[0] or
//                  d1 <= max_dist[1] (a candidate within neither bound may be visited or not).
//   commit(k, which, t, best0, best1)   once per item, in the round where it is final: it took t by
//                  query `which` (0 / 1), or nothing (-1); best0 / best1: each query's best distance
//                  within its bound under the mask the item saw, or -1.
template <typename Load, typename Commit>
__device__ __forceinline__ void resolve_pairs_in_order(int count, const int (&max_dist)[2], const int (&min_diff)[2],
                                                       uint32_t* mask, int* taker, Load load, Commit commit)
{
    const int lane = threadIdx.x & 63;
    int r0 = 0;
    while (r0 < count) {
        const int k = r0 + lane;
        const bool act = k < count;
        auto each = load(k, act);
        uint32_t bk0 = OT_NO_BEST, bk1 = OT_NO_BEST;
        each([&](int t, int d0, int d1) {
            if (d0 <= max_dist[0]) bk0 = min(bk0, (uint32_t)d0 << OT_TARGET_BITS | (uint32_t)t);
            if (d1 <= max_dist[1]) bk1 = min(bk1, (uint32_t)d1 << OT_TARGET_BITS | (uint32_t)t);
        });
        const int t0 = (int)(bk0 & (uint32_t)(OT_MAX_TARGETS - 1)), b0 = (int)(bk0 >> OT_TARGET_BITS);
        const int t1 = (int)(bk1 & (uint32_t)(OT_MAX_TARGETS - 1)), b1 = (int)(bk1 >> OT_TARGET_BITS);
        int s0 = max_dist[0] + 1, s1 = max_dist[1] + 1;
        each([&](int t, int d0, int d1) {
            if (t < t0 && d0 <= max_dist[0]) s0 = min(s0, d0);
            if (t < t1 && d1 <= max_dist[1]) s1 = min(s1, d1);
        });
        const bool ok0 = bk0 != OT_NO_BEST && s0 - b0 > min_diff[0];
        const bool ok1 = bk1 != OT_NO_BEST && s1 - b1 > min_diff[1];
        const int which = ok0 && ok1 ? (b1 < b0 ? 1 : 0) : (ok1 ? 1 : (ok0 ? 0 : -1));
        const int tw = which == 1 ? t1 : t0;
        if (which >= 0) atomicMin(&taker[tw], lane);
        wave_sync();
        bool conflict = false;
        each([&](int t, int, int) {
            if (taker[t] < lane) conflict = true;
        });
        const uint64_t cb = __ballot(conflict);
        const int f = cb ? __builtin_ctzll(cb) : 64;
        if (act && lane < f) {
            if (which >= 0) mask_clear(mask, tw);
            commit(k, which, tw, bk0 != OT_NO_BEST ? b0 : -1, bk1 != OT_NO_BEST ? b1 : -1);
        }
        wave_sync();
        if (which >= 0) taker[tw] = OT_NO_TAKER;
        wave_sync();
        r0 += f;
    }
}

}  // namespace mage
