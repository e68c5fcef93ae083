// track_bufs.hpp — the device loop's state (track.hip): control words, kernel arguments and the
// one table of the per-call device block (track_block_visit): each buffer once, with its element
// type and count; the pointers, the block's size, the keyframe ring's byte range and the host
// mirror's views all come from running it.  No device code, so a host program can include it.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "../../include/mage_hot.h"

namespace mage {
namespace track {

constexpr int NKMAX = 8;  // keyframes of the local map
// RadiusMatch band-index ring of mage_track_sequence_device: chunks of BAND_CHUNK frames, two
// chunks resident (the host runs at most a few frames ahead of the device)
constexpr uint32_t BAND_CHUNK = 16, BAND_SLOTS = 2 * BAND_CHUNK;

struct Ctl {              // per-call control words (device)
    uint32_t exec[3];     // radius pass k ran
    uint32_t ns;          // queries (keyframe points in front of the predicted camera)
    uint32_t lost;
    uint32_t kf_first;    // keyframe ring: oldest slot, slots in use (ascending keyframe id)
    uint32_t kf_count;
    uint32_t kf_n[NKMAX]; // keyframe feature counts per slot
    uint32_t lm_nq;       // local-map queries of the frame
    uint32_t kf_id[NKMAX];  // frame index of the keyframe in each slot
    uint32_t kf_an[NKMAX];  // associations per slot (the keyframe frame's pass-2 inliers)
    uint32_t halt;        // local BA pending: every frame kernel is a no-op until the host clears it
};

struct TrackBufs {  // the kernels' buffer argument (member order = kernel argument layout)
    Ctl* ctl;
    double* pred;  // 12
    // keyframe ring (NKMAX slots of cap entries; the reference keyframe is the newest slot): points,
    // mean viewing directions (3 per point), scale-invariance distances, pose (12 per slot)
    mage_keypoint* kf_kp;
    uint8_t* kf_desc;
    float *kf_pts, *kf_mvd, *kf_dmin, *kf_dmax;
    double* kf_pose;
    // mapping side (local BA): per point its refinement count and own-observation flag, per slot
    // the associations (owner keyframe id, point index, keypoint x, y bits) and their flags
    uint32_t* kf_ref;
    uint8_t* kf_own;
    int4* kf_assoc;
    uint8_t* kf_aalive;
    int2 *src1, *src2;     // pose-BA observation sources (owner keyframe id, point index)
    float *info1, *info2;  // per observation: MapPointRefinementConfidence of the point
    int2* lm_qsrc;
    float* lm_qinfo;
    uint32_t* prog;  // mapped host words {frame done, frame that requested a local BA}; not in the block
    // local-map search
    uint32_t* lm_mask;    // unassociated keypoints (bit words)
    uint8_t* lm_visited;  // reference-keyframe points associated as pass-1 inliers
    int32_t* lm_hide;     // reference-keyframe points of pass-1 outliers: their keypoint
    float* lm_qpos;
    int32_t *lm_qoct, *lm_qhide;
    uint8_t* lm_qdesc;
    float* lm_qpt;  // the queries' map point positions
    int32_t* lm_res;
    uint32_t* lm_status;
    uint8_t* lm_scratch;
    mage_keypoint* qkp;
    uint8_t* qdesc;
    float* qpos;
    uint32_t *sel, *nq;  // nq: query count of each radius pass
    mage_dmatch* m;      // 3 x cap
    uint32_t* mn;
    // pose BA
    float *pos3, *r9, *intr4;
    uint32_t *os1, *os2;  // 2 each
    float *pts1, *uv1, *pts2, *uv2, *pos3_o1, *r9_o1, *pos3_o2, *r9_o2;
    uint8_t *out1, *out2;
    float* msq;
};

struct TrackConst {
    float fx, fy, cx, cy;  // (float)K
    double K[4];
    double plane_z;
    mage_track_settings s;
    uint32_t cap;          // keypoints per frame slot
    uint32_t nk;           // keyframe ring slots (max(local_map_keyframes, 1))
    uint32_t qcap;         // local-map queries per frame (nk x cap)
    uint32_t acap;         // associations per keyframe slot (cap + qcap)
    float fmax[8], fmin[8];  // ComputeDMax / ComputeDMin factors per octave (powf on the host)
    float log2s;           // log2(scale factor)
};

// The block: what the kernels take (b) and what only the host driver's launches name.
struct TrackBlock {
    TrackBufs b;
    int32_t* rscratch;  // RadiusMatch
    uint32_t* rstatus;
    double* poses;      // the outputs, 12 / 1 / 1 / 1 per frame
    uint32_t* matches;
    uint32_t* inliers;
    uint8_t* keyframe;
    // RadiusMatch band indices, built once per frame: a ring of BAND_SLOTS frames, BAND_CHUNK at a
    // time by the enqueue of a chunk's first frame (the loop runs at most DEPTH frames ahead, so a
    // chunk's slots are free again when the chunk two ahead is built)
    unsigned long long* bkeys;
    float* bxy;
    uint32_t* bdesc;
};

// Walks the table: binds each member to base + its offset (256-byte aligned, in table order) and
// measures the block and its keyframe-ring part.  At base 0 the members hold the offsets.
struct BlockBinder {
    enum Part { REST, RING, RING_MOVED };  // RING_MOVED: the ring fields a local BA changes
    uintptr_t base = 0;
    size_t bytes = 0;  // the block's size so far
    size_t ring_begin = 0, moved_begin = 0, ring_end = 0;
    bool ring_contiguous = true;
    Part last = REST;
    template <class T>
    void operator()(T*& member, size_t count, Part part = REST)
    {
        member = reinterpret_cast<T*>(base + bytes);
        if (part != REST) {
            // one byte range (one copy each way per window): consecutive entries, the moved ones last
            if (ring_end == 0) ring_begin = bytes;
            else if (part < last || last == REST) ring_contiguous = false;
            if (part == RING_MOVED && last != RING_MOVED) moved_begin = bytes;
            ring_end = bytes + count * sizeof(T);
        }
        last = part;
        bytes = (bytes + count * sizeof(T) + 255) & ~(size_t)255;
    }
};

// The table, in the block's order (c: cap, nk, qcap, acap; local_map_scratch_bytes(c.qcap)).
template <class V>
void track_block_visit(TrackBlock& k, const TrackConst& c, size_t frames, size_t lm_scratch_bytes, V& v)
{
    TrackBufs& b = k.b;
    const size_t cap = c.cap, nk = c.nk, ring = cap * nk, qcap = c.qcap;
    const size_t c2 = c.acap;  // pose-BA 2 observations = associations per keyframe slot
    const size_t band = cap * BAND_SLOTS;
    v(b.ctl, 1);
    v(b.pred, 12);
    v(b.kf_kp, ring, BlockBinder::RING);
    v(b.kf_desc, 32 * ring, BlockBinder::RING);
    v(b.kf_pts, 3 * ring, BlockBinder::RING_MOVED);
    v(b.kf_mvd, 3 * ring, BlockBinder::RING_MOVED);
    v(b.kf_dmin, ring, BlockBinder::RING_MOVED);
    v(b.kf_dmax, ring, BlockBinder::RING_MOVED);
    v(b.kf_pose, 12 * nk, BlockBinder::RING_MOVED);
    v(b.kf_ref, ring, BlockBinder::RING_MOVED);
    v(b.kf_own, ring, BlockBinder::RING_MOVED);
    v(b.kf_assoc, c2 * nk, BlockBinder::RING_MOVED);
    v(b.kf_aalive, c2 * nk, BlockBinder::RING_MOVED);
    v(b.src1, cap);
    v(b.src2, c2);
    v(b.info1, cap);
    v(b.lm_qsrc, qcap);
    v(b.lm_qinfo, qcap);
    v(b.qkp, cap);
    v(b.qdesc, 32 * cap);
    v(b.qpos, 2 * cap);
    v(b.sel, cap);
    v(b.nq, 4);
    v(b.m, 3 * cap);
    v(b.mn, 4);
    v(k.rscratch, cap);
    v(k.rstatus, 1);
    v(b.pos3, 3);
    v(b.r9, 9);
    v(b.intr4, 4);
    v(b.os1, 2);
    v(b.os2, 2);
    v(b.pts1, 3 * cap);
    v(b.uv1, 2 * cap);
    v(b.pts2, 3 * c2);
    v(b.uv2, 2 * c2);
    v(b.info2, c2);
    v(b.pos3_o1, 3);
    v(b.r9_o1, 9);
    v(b.pos3_o2, 3);
    v(b.r9_o2, 9);
    v(b.out1, cap);
    v(b.out2, c2);
    v(b.msq, 2);
    v(b.lm_mask, 4096 / 32);
    v(b.lm_visited, cap);
    v(b.lm_hide, cap);
    v(b.lm_qpos, 2 * qcap);
    v(b.lm_qoct, qcap);
    v(b.lm_qhide, qcap);
    v(b.lm_qdesc, 32 * qcap);
    v(b.lm_qpt, 3 * qcap);
    v(b.lm_res, qcap);
    v(b.lm_status, 1);
    v(b.lm_scratch, lm_scratch_bytes);
    v(k.poses, 12 * frames);
    v(k.matches, frames);
    v(k.inliers, frames);
    v(k.keyframe, frames);
    v(k.bkeys, band);
    v(k.bxy, 2 * band);
    v(k.bdesc, 8 * band);
}

inline BlockBinder track_block(TrackBlock& k, const TrackConst& c, size_t frames, size_t lm_scratch_bytes, void* base)
{
    BlockBinder v{reinterpret_cast<uintptr_t>(base)};
    track_block_visit(k, c, frames, lm_scratch_bytes, v);
    return v;
}

// The keyframe ring on the host: control words, kf_* views into a mirror of the block's ring range
struct HostRing {
    uint32_t nk = 0, cap = 0, acap = 0;
    Ctl ctl{};  // kf_first, kf_count, and per slot kf_n, kf_id, kf_an
    TrackBufs v{};
};

// The same table bound so that the ring range starts at `mirror`.
inline HostRing host_ring(const TrackConst& c, size_t frames, size_t lm_scratch_bytes, void* mirror, const Ctl& ctl)
{
    TrackBlock k{};
    const size_t ring_begin = track_block(k, c, frames, lm_scratch_bytes, nullptr).ring_begin;
    track_block(k, c, frames, lm_scratch_bytes, reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(mirror) - ring_begin));
    return HostRing{c.nk, c.cap, c.acap, ctl, k.b};
}

}  // namespace track
}  // namespace mage
