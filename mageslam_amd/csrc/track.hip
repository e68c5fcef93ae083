// track.hip — the C4 tracking loop device-resident: the same specification as csrc/track.cpp
// (PoseEstimator::TryEstimatePoseFromKeyframe, PoseEstimator.cpp:439-607; TrackLocalMap's two
// OptimizeCameraPose passes, TrackLocalMap.cpp:37-140; NewKeyFrameDecision.cpp:196) with every
// per-frame decision taken on the device, so the host enqueues the whole sequence and
// synchronises once.  trk_init makes frame 0's keyframe; then per frame, in one stream:
//   trk_project        prediction (constant velocity on SE3, fp64) + ProjectUndistorted of the
//                      keyframe's map points (f32), ordered compaction of the points in front
//                      (a launch of its own only for the first frame and after a local BA)
//   radius x 3         RadiusMatch at SearchRadius / WiderSearchRadius (position overrides) /
//                      ExtraWiderSearchRadius (keypoint positions); pass k+1 gets a zero query
//                      count unless pass k ran and was weak (RadiusFollow, in pass k's kernel)
//   trk_gather         the last pass's matches -> pose-BA observations, "lost" when too few
//   pose BA 1          mage_ba_pose_batch_device (3 steps, Huber 4, 6^2)
//   trk_filter[_lm]    ordered compaction of pass 1's inliers [+ the local map's candidate queries,
//                      then the local-map search (localmap.hip) and trk_lm_assemble]
//   pose BA 2          (4 steps, Huber 0.9, 4.5^2)
//   trk_finish_project the frame's pose / counts, keyframe decision, new keyframe's map points,
//                      then the next frame's trk_project part
// Arithmetic: csrc/track_math.hpp, shared with track.cpp (identical results); buffers: track_bufs.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <vector>

#include "common.hpp"
#include "ordered_take.hpp"
#include "track_window.hpp"

namespace mage {
namespace {

using namespace track;

constexpr int TT = 1024;  // threads of the per-frame control kernels

// Keyframe slot <- frame features (kp, desc, n) with map points back-projected at pose P onto the
// plane and their MapPoint::UpdateMeanViewDirectionAndDistances attributes.
__device__ void make_keyframe(const TrackBufs& b, const TrackConst& c, uint32_t slot, const mage_keypoint* fk,
                              const uint8_t* fd, uint32_t nf, const Pose& P, uint32_t fid)
{
    float R32[9], t32[3], Cf[3];
    pose_f32(P.R, P.t, R32, t32);
    world_position(R32, t32, Cf);
    const size_t o = (size_t)slot * c.cap;
    if (threadIdx.x < 12) b.kf_pose[12 * slot + threadIdx.x] = threadIdx.x < 9 ? P.R[threadIdx.x] : P.t[threadIdx.x - 9];
    for (uint32_t i = threadIdx.x; i < nf; i += TT) {
        b.kf_ref[o + i] = 0;
        b.kf_own[o + i] = 1;
        b.kf_kp[o + i] = fk[i];
        const uint4* s = reinterpret_cast<const uint4*>(fd + 32ull * i);
        uint4* d = reinterpret_cast<uint4*>(b.kf_desc + 32ull * (o + i));
        d[0] = s[0];
        d[1] = s[1];
        float Pp[3], mvd[3], dmin, dmax;
        backproject_to_plane(fk[i].x, fk[i].y, P, c.K, c.plane_z, fid, i, c.s.map_point_depth_noise, Pp);
        for (int j = 0; j < 3; j++) b.kf_pts[3 * (o + i) + j] = Pp[j];
        point_attributes(Pp, Cf, fk[i].octave, c.fmin, c.fmax, mvd, dmin, dmax);
        for (int j = 0; j < 3; j++) b.kf_mvd[3 * (o + i) + j] = mvd[j];
        b.kf_dmin[o + i] = dmin;
        b.kf_dmax[o + i] = dmax;
    }
}

__device__ __forceinline__ uint32_t ref_slot(const Ctl* ctl, const TrackConst& c)
{
    return (ctl->kf_first + ctl->kf_count - 1) % c.nk;
}

// Frame 0: its keyframe at the first pose (already in poses[0]).
// A frame's keypoint count, clamped to the frame slot (`cap` keypoints): a larger count would copy
// the next frame's (or unallocated) entries into the keyframe buffers, which hold `cap`; the
// overflow is reported through status bit 1 (MAGE_ECAPACITY on return).
__device__ uint32_t frame_count(const TrackConst& c, const uint32_t* nf, uint32_t* status)
{
    const uint32_t n = *nf;
    if (n > c.cap) {
        if (threadIdx.x == 0) atomicOr(status, 2u);
        return c.cap;
    }
    return n;
}

__global__ __launch_bounds__(TT) void trk_init(TrackBufs b, TrackConst c, const mage_keypoint* fk, const uint8_t* fd,
                                               const uint32_t* nf, double* poses, uint32_t* matches,
                                               uint32_t* inliers, uint8_t* keyframe, uint32_t* status)
{
    const uint32_t n = frame_count(c, nf, status);
    make_keyframe(b, c, 0, fk, fd, n, load_pose(poses), 0u);
    if (threadIdx.x == 0) {
        b.ctl->kf_first = 0;
        b.ctl->kf_count = 1;
        b.ctl->kf_n[0] = n;
        b.ctl->kf_id[0] = 0;
        b.ctl->kf_an[0] = 0;
        b.ctl->halt = 0;
        matches[0] = inliers[0] = n;
        keyframe[0] = 1;
        b.intr4[0] = c.cx;  // BundlerLib's {cx, cy, fx, fy}
        b.intr4[1] = c.cy;
        b.intr4[2] = c.fx;
        b.intr4[3] = c.fy;
    }
}

__device__ void project_frame(const TrackBufs& b, const TrackConst& c, int f, const double* poses)
{
    __shared__ float R32[9], t32[3];
    __shared__ uint32_t wsum[TT / 64];
    if (b.ctl->halt) {  // a local BA is pending: this frame runs again after it (zero counts downstream)
        if (threadIdx.x == 0) {
            b.ctl->ns = 0;
            for (int k = 0; k < 3; k++) b.ctl->exec[k] = b.nq[k] = 0;
        }
        return;
    }
    if (threadIdx.x == 0) {
        const Pose p1 = load_pose(poses + 12ll * (f - 1));
        const Pose pred = f < 2 ? p1 : predict(p1, load_pose(poses + 12ll * (f - 2)));
        store_pose(b.pred, pred);
        pose_f32(pred.R, pred.t, R32, t32);
    }
    __syncthreads();
    const uint32_t slot = ref_slot(b.ctl, c), nk = b.ctl->kf_n[slot];
    const size_t o = (size_t)slot * c.cap;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < nk; c0 += TT) {
        const uint32_t i = c0 + threadIdx.x;
        bool front = false;
        float u = 0.f, v = 0.f;
        if (i < nk) {
            const float X[3] = {b.kf_pts[3 * (o + i)], b.kf_pts[3 * (o + i) + 1], b.kf_pts[3 * (o + i) + 2]};
            front = project_front(R32, t32, c.fx, c.fy, c.cx, c.cy, X, u, v);
        }
        uint32_t tot;
        const uint32_t pos = base + block_prefix<TT / 64>(front, wsum, &tot);
        if (front) {
            b.qkp[pos] = b.kf_kp[o + i];
            const uint4* s = reinterpret_cast<const uint4*>(b.kf_desc + 32ull * (o + i));
            uint4* d = reinterpret_cast<uint4*>(b.qdesc + 32ull * pos);
            d[0] = s[0];
            d[1] = s[1];
            b.qpos[2 * pos] = u;
            b.qpos[2 * pos + 1] = v;
            b.sel[pos] = i;
        }
        base += tot;
    }
    if (threadIdx.x == 0) {
        b.ctl->ns = base;
        b.ctl->exec[0] = 1;
        b.ctl->exec[1] = b.ctl->exec[2] = 0;
        b.nq[0] = base;
        b.nq[1] = b.nq[2] = 0;
    }
}

__global__ __launch_bounds__(TT) void trk_gather(TrackBufs b, TrackConst c, const mage_keypoint* fk, int f,
                                                 uint32_t* matches)
{
    if (b.ctl->halt) {
        if (threadIdx.x == 0) {
            b.ctl->lost = 1;
            b.os1[0] = b.os1[1] = 0;
        }
        return;
    }
    const int fin = b.ctl->exec[2] ? 2 : (b.ctl->exec[1] ? 1 : 0);
    const uint32_t n = b.mn[fin];
    const bool lost = n < c.s.min_matches;
    const mage_dmatch* m = b.m + (size_t)fin * c.cap;
    if (!lost) {
        const uint32_t slot = ref_slot(b.ctl, c);
        const size_t o = (size_t)slot * c.cap;
        const int kid = (int)b.ctl->kf_id[slot];
        for (uint32_t k = threadIdx.x; k < n; k += TT) {
            const uint32_t q = b.sel[m[k].query_idx], t = (uint32_t)m[k].train_idx;
            for (int j = 0; j < 3; j++) b.pts1[3 * k + j] = b.kf_pts[3 * (o + q) + j];
            b.uv1[2 * k] = fk[t].x;
            b.uv1[2 * k + 1] = fk[t].y;
            b.info1[k] = refinement_confidence(b.kf_ref[o + q]);  // TrackLocalMap.cpp:473-475
            b.src1[k] = make_int2(kid, (int)q);
        }
    }
    if (threadIdx.x == 0) {
        matches[f] = n;
        b.ctl->lost = lost;
        b.os1[0] = 0;
        b.os1[1] = lost ? 0u : n;
        to_bundler(b.pred, b.pred + 9, b.pos3, b.r9);
    }
}

// Pass-1 inliers -> the pose-BA 2 observations (ordered compaction); with the local map on, the
// frame's associations after TrackLocalMap unassociates the outliers (:116-147): the unassociated
// keypoint mask, the reference points associated as inliers (visited) and each outlier point's
// keypoint (hidden from its own local-map search).
__device__ void filter_frame(const TrackBufs& b, const TrackConst& c, const uint32_t* nf_ptr)
{
    __shared__ uint32_t wsum[TT / 64];
    const uint32_t n = b.os1[1];
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += TT) {
        const uint32_t k = c0 + threadIdx.x;
        const bool keep = k < n && !b.out1[k];
        uint32_t tot;
        const uint32_t pos = base + block_prefix<TT / 64>(keep, wsum, &tot);
        if (keep) {
            for (int j = 0; j < 3; j++) b.pts2[3 * pos + j] = b.pts1[3 * k + j];
            b.uv2[2 * pos] = b.uv1[2 * k];
            b.uv2[2 * pos + 1] = b.uv1[2 * k + 1];
            b.info2[pos] = b.info1[k];
            b.src2[pos] = b.src1[k];
        }
        base += tot;
    }
    if (threadIdx.x == 0) {
        b.os2[0] = 0;
        b.os2[1] = base;
    }
    if (c.s.local_map_keyframes == 0 || b.ctl->lost) return;
    // the unassociated-keypoint mask is built in LDS (2000 atomics on ~63 global words serialised
    // at the L2) and written out once
    __shared__ uint32_t smask[4096 / 32];
    const uint32_t nf = min(min(*nf_ptr, c.cap), 4096u);
    const uint32_t nk = b.ctl->kf_n[ref_slot(b.ctl, c)];
    for (uint32_t w = threadIdx.x; w < (nf + 31) / 32; w += TT)
        smask[w] = (32 * w + 32 <= nf) ? 0xFFFFFFFFu : ((1u << (nf - 32 * w)) - 1u);
    for (uint32_t i = threadIdx.x; i < nk; i += TT) {
        b.lm_visited[i] = 0;
        b.lm_hide[i] = -1;
    }
    __syncthreads();
    const int fin = b.ctl->exec[2] ? 2 : (b.ctl->exec[1] ? 1 : 0);
    const mage_dmatch* m = b.m + (size_t)fin * c.cap;
    for (uint32_t k = threadIdx.x; k < n; k += TT) {
        const uint32_t q = b.sel[m[k].query_idx], t = (uint32_t)m[k].train_idx;
        if (!b.out1[k]) {
            if (t < nf) atomicAnd(&smask[t >> 5], ~(1u << (t & 31)));
            b.lm_visited[q] = 1;
        } else {
            b.lm_hide[q] = (int32_t)t;
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < (nf + 31) / 32; w += TT) b.lm_mask[w] = smask[w];
}

// TrackLocalMap.cpp:149-223: the local map's unvisited points, keyframe by keyframe in ascending id,
// through ProjectMapPointIntoCurrentFrame / IsGoodCandidate / ComputeOctave with the pass-1 pose
// (tracking.py local_map_queries, track.cpp): ordered compaction of the candidates into queries.
// No pass-1 inlier left (mapPoints.empty(), :149-150) is a lost frame.
__device__ void lm_project_frame(const TrackBufs& b, const TrackConst& c)
{
    __shared__ uint32_t wsum[TT / 64];
    const bool off = c.s.local_map_keyframes == 0 || b.ctl->lost;
    if (off || b.os2[1] == 0) {
        if (threadIdx.x == 0) {
            if (!off) b.ctl->lost = 1;
            b.ctl->lm_nq = 0;
        }
        return;
    }
    // the pass-1 pose as pose BA 1 left it: its floats are the float view matrix (track.cpp casts
    // the double pose made of them back to float: the same values)
    float R[9], t[3], C[3];
    from_bundler(b.pos3_o1, b.r9_o1, R, t);
    world_position(R, t, C);
    const uint32_t first = b.ctl->kf_first, count = b.ctl->kf_count;
    uint32_t base = 0;
    for (uint32_t si = 0; si < count; si++) {
        const uint32_t slot = (first + si) % c.nk, n = b.ctl->kf_n[slot];
        const bool is_ref = si + 1 == count;
        const size_t o = (size_t)slot * c.cap;
        for (uint32_t c0 = 0; c0 < n; c0 += TT) {
            const uint32_t i = c0 + threadIdx.x;
            bool ok = i < n && !(is_ref && b.lm_visited[i]);
            float px = 0.f, py = 0.f;
            int oc = 0;
            if (ok)
                ok = local_map_candidate(R, t, C, c.fx, c.fy, c.cx, c.cy, c.s, c.log2s, b.kf_pts + 3 * (o + i),
                                         b.kf_mvd + 3 * (o + i), b.kf_dmin[o + i], b.kf_dmax[o + i], px, py, oc);
            uint32_t tot;
            const uint32_t pos = base + block_prefix<TT / 64>(ok, wsum, &tot);
            if (ok && pos < c.qcap) {
                b.lm_qpos[2 * pos] = px;
                b.lm_qpos[2 * pos + 1] = py;
                b.lm_qoct[pos] = oc;
                b.lm_qhide[pos] = is_ref ? b.lm_hide[i] : -1;
                const uint4* sd = reinterpret_cast<const uint4*>(b.kf_desc + 32ull * (o + i));
                uint4* dd = reinterpret_cast<uint4*>(b.lm_qdesc + 32ull * pos);
                dd[0] = sd[0];
                dd[1] = sd[1];
                for (int j = 0; j < 3; j++) b.lm_qpt[3 * pos + j] = b.kf_pts[3 * (o + i) + j];
                b.lm_qsrc[pos] = make_int2((int)b.ctl->kf_id[slot], (int)i);
                b.lm_qinfo[pos] = refinement_confidence(b.kf_ref[o + i]);
            }
            base += tot;
        }
    }
    if (threadIdx.x == 0) b.ctl->lm_nq = min(base, c.qcap);
}

// The local map's new associations appended to the pass-2 observations in query order.
__global__ __launch_bounds__(TT) void trk_lm_assemble(TrackBufs b, const mage_keypoint* fk)
{
    __shared__ uint32_t wsum[TT / 64];
    const uint32_t nq = b.ctl->lm_nq;
    if (b.ctl->lost || nq == 0) return;
    const uint32_t base0 = b.os2[1];
    uint32_t base = base0;
    for (uint32_t c0 = 0; c0 < nq; c0 += TT) {
        const uint32_t q = c0 + threadIdx.x;
        const int r = q < nq ? b.lm_res[q] : -1;
        uint32_t tot;
        const uint32_t pos = base + block_prefix<TT / 64>(r >= 0, wsum, &tot);
        if (r >= 0) {
            for (int j = 0; j < 3; j++) b.pts2[3 * pos + j] = b.lm_qpt[3 * q + j];
            b.uv2[2 * pos] = fk[r].x;
            b.uv2[2 * pos + 1] = fk[r].y;
            b.info2[pos] = b.lm_qinfo[q];
            b.src2[pos] = b.lm_qsrc[q];
        }
        base += tot;
    }
    if (threadIdx.x == 0) b.os2[1] = base;
}

__device__ void finish_frame(const TrackBufs& b, const TrackConst& c, int f, const mage_keypoint* fk,
                             const uint8_t* fd, const uint32_t* nf, double* poses, uint32_t* inliers,
                             uint8_t* keyframe, uint32_t* status)
{
    __shared__ uint32_t wsum[TT / 64];
    __shared__ int s_kf;
    __shared__ uint32_t s_slot;
    __shared__ double sP[12];
    if (b.ctl->halt) return;  // re-run after the pending local BA
    bool lost = b.ctl->lost != 0;
    uint32_t n_in = 0;
    if (!lost) {
        const uint32_t n2 = b.os2[1];
        for (uint32_t c0 = 0; c0 < n2; c0 += TT) {
            const uint32_t k = c0 + threadIdx.x;
            uint32_t tot;
            (void)block_prefix<TT / 64>(k < n2 && !b.out2[k], wsum, &tot);
            n_in += tot;
        }
        // TrackLocalMap.cpp:309-314: too few associations after the second pass
        if (c.s.local_map_keyframes > 0 && n_in < c.s.min_tracked) lost = true;
    }
    if (threadIdx.x == 0) {
        Pose P;  // pose BA 2's, or the prediction when lost (this order keeps the count loop above in VGPRs)
        from_bundler(b.pos3_o2, b.r9_o2, P.R, P.t);
        if (lost) P = load_pose(b.pred);
        store_pose(poses + 12ll * f, P);
        store_pose(sP, P);
        inliers[f] = lost ? 0u : n_in;
        const uint32_t nk = b.ctl->kf_n[ref_slot(b.ctl, c)];
        s_kf = !lost && (double)n_in < c.s.keyframe_ratio * (double)nk + (double)c.s.keyframe_min;
        keyframe[f] = (uint8_t)s_kf;
        if (s_kf) {  // the keyframe ring: a free slot, or the oldest keyframe's
            if (b.ctl->kf_count < c.nk) {
                s_slot = (b.ctl->kf_first + b.ctl->kf_count) % c.nk;
                b.ctl->kf_count++;
            } else {
                s_slot = b.ctl->kf_first;
                b.ctl->kf_first = (b.ctl->kf_first + 1) % c.nk;
            }
        }
    }
    __syncthreads();
    if (s_kf) {
        const uint32_t n = frame_count(c, nf, status);
        make_keyframe(b, c, s_slot, fk, fd, n, load_pose(sP), f);
        // its associations: the pass-2 inliers in observation order (ordered compaction)
        const uint32_t n2 = b.os2[1];
        int4* as = b.kf_assoc + (size_t)s_slot * c.acap;
        uint8_t* aa = b.kf_aalive + (size_t)s_slot * c.acap;
        uint32_t base = 0;
        for (uint32_t c0 = 0; c0 < n2; c0 += TT) {
            const uint32_t k = c0 + threadIdx.x;
            const bool in = k < n2 && !b.out2[k];
            uint32_t tot;
            const uint32_t pos = base + block_prefix<TT / 64>(in, wsum, &tot);
            if (in && pos < c.acap) {
                as[pos] = make_int4(b.src2[k].x, b.src2[k].y, __float_as_int(b.uv2[2 * k]), __float_as_int(b.uv2[2 * k + 1]));
                aa[pos] = 1;
            }
            base += tot;
        }
        if (threadIdx.x == 0) {
            b.ctl->kf_n[s_slot] = n;
            b.ctl->kf_id[s_slot] = (uint32_t)f;
            b.ctl->kf_an[s_slot] = min(base, c.acap);
            // a window needs two keyframes: halt the queued frames until the host ran the local BA
            if (c.s.local_ba && b.ctl->kf_count >= 2) b.ctl->halt = 1;
        }
    }
    if (b.prog && threadIdx.x == 0) {  // progress for the host (local BA): request word, then frame
        if (s_kf && c.s.local_ba && b.ctl->kf_count >= 2) *reinterpret_cast<volatile uint32_t*>(b.prog + 1) = (uint32_t)f;
        __threadfence_system();
        *reinterpret_cast<volatile uint32_t*>(b.prog) = (uint32_t)f;
    }
}

// The per-frame control kernels, and two fused pairs that save a dependent launch each per frame
// (the parts are separated by a workgroup barrier: what one part writes to global memory the next
// reads in the same workgroup).
__global__ __launch_bounds__(TT) void trk_project(TrackBufs b, TrackConst c, int f, const double* poses)
{
    project_frame(b, c, f, poses);
}

__global__ __launch_bounds__(TT) void trk_filter(TrackBufs b, TrackConst c, const uint32_t* nf_ptr)
{
    filter_frame(b, c, nf_ptr);
}

// trk_filter + trk_lm_project (the local map's candidate queries of the frame)
__global__ __launch_bounds__(TT) void trk_filter_lm(TrackBufs b, TrackConst c, const uint32_t* nf_ptr)
{
    filter_frame(b, c, nf_ptr);
    __syncthreads();
    lm_project_frame(b, c);
}

// trk_finish of frame f + trk_project of frame f + 1 (its prediction needs f's pose and ring)
__global__ __launch_bounds__(TT) void trk_finish_project(TrackBufs b, TrackConst c, int f, const mage_keypoint* fk,
                                                         const uint8_t* fd, const uint32_t* nf, double* poses,
                                                         uint32_t* inliers, uint8_t* keyframe, uint32_t* status,
                                                         int project_next)
{
    finish_frame(b, c, f, fk, fd, nf, poses, inliers, keyframe, status);
    if (!project_next) return;
    __syncthreads();
    project_frame(b, c, f + 1, poses);
}

}  // namespace
}  // namespace mage

namespace mage {
namespace {

// ---- Local BA of the device loop (host side, between frames: MappingWorker's BundleAdjustTask) ----
// The same window / schedule / write-back as tracking.py build_ba_window + apply_ba_window, over the
// keyframe ring copied from the device; BundlerLib through the C-ABI (one instance per call of the
// loop, the lambda persisted across windows as MappingWorker does).
// MAGE_TRACK_PROFILE=1 in the environment: per-window phase times of the local BA on stderr
// (development; tools/track_kernels.py)
struct PhaseClock {
    bool on = false;
    std::chrono::steady_clock::time_point t;
    char line[512];
    int len = 0;
    void start()
    {
        if (!on) return;
        t = std::chrono::steady_clock::now();
        len = 0;
    }
    void mark(const char* name)
    {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        len += snprintf(line + len, sizeof(line) - len, " %s %.3f", name,
                        std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
    void flush()
    {
        if (on) fprintf(stderr, "local BA window ms:%s\n", line);
    }
};

// Page-locked host array (the ring's host copy): DMA copies in both directions, queued with
// hipMemcpyAsync on the loop's stream instead of one synchronous pageable copy per field.
template <class T>
struct Pinned {
    T* p = nullptr;
    size_t n = 0;
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned()
    {
        if (p) (void)hipHostFree(p);
    }
    bool resize(size_t m)
    {
        if (m <= n) return true;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(m, 1) * sizeof(T), hipHostMallocDefault) != hipSuccess)
            return false;
        n = m;
        return true;
    }
    T* data() { return p; }
};

struct BundlerHandle {  // a fresh BundlerLib per window (BundleAdjust.cpp MakeBundler)
    mage_ba* ba = nullptr;
    ~BundlerHandle()
    {
        if (ba) mage_ba_destroy(ba);
    }
};

struct BaSolution {
    std::vector<uint32_t> outl;  // outlier observations (indices into the window's), nout of them
    uint32_t nout = 0;
    std::vector<float> pos, r9, xyz;  // GetPose / GetPoint
};

// BundlerLib on one window (tracking.py run_bundler); the lambda persisted across windows
mage_status solve_window(const BaWindow& w, const TrackConst& c, LocalBA& L, int device, BundlerHandle& H, BaSolution& o,
                         PhaseClock& prof)
{
    const uint32_t nr = w.nr, P = (uint32_t)w.keys.size(), E = (uint32_t)w.kept.size();
    const std::vector<float> hw(std::max(w.steps, 1u), w.huber);
    mage_status st;
    if ((st = mage_ba_create(0, device, &H.ba)) != MAGE_OK) return st;
    prof.mark("create");
    if (L.have_lambda && (st = mage_ba_set_lambda(H.ba, L.lambda)) != MAGE_OK) return st;
    if ((st = mage_ba_set_cameras(H.ba, nr, w.pos3.data(), w.r9.data(), w.intr.data(), w.fixed.data())) != MAGE_OK ||
        (st = mage_ba_set_points(H.ba, P, w.xyz.data())) != MAGE_OK ||
        (st = mage_ba_set_observations(H.ba, E, w.uv.data(), w.cam.data(), w.pt.data(), w.info.data())) != MAGE_OK)
        return st;
    prof.mark("setters");
    o.outl.resize(E);
    float ms = 0.f;
    if ((st = mage_ba_step(H.ba, hw.data(), (uint32_t)hw.size(), c.s.ba_max_outlier_error, o.outl.data(), E, &o.nout,
                           &ms)) != MAGE_OK)
        return st;
    prof.mark("step");
    o.pos.resize(3 * nr);
    o.r9.resize(9 * nr);
    o.xyz.resize(3ull * P);
    float lam = 0.f;
    if ((st = mage_ba_get_poses(H.ba, o.pos.data(), o.r9.data())) != MAGE_OK ||
        (st = mage_ba_get_points(H.ba, o.xyz.data())) != MAGE_OK || (st = mage_ba_get_lambda(H.ba, &lam)) != MAGE_OK)
        return st;
    L.have_lambda = true;
    L.lambda = std::max(lam, c.s.min_lambda);
    return MAGE_OK;
}

}  // namespace
}  // namespace mage

extern "C" mage_status mage_track_sequence_device(const mage_keypoint* d_kp, const uint8_t* d_desc, uint32_t pitch,
                                                  const uint32_t* d_n, uint32_t frames, const double K[4],
                                                  const double first_pose[12], double plane_z,
                                                  const mage_track_settings* s, double* poses, uint32_t* matches,
                                                  uint32_t* inliers, uint8_t* keyframe, uint32_t* ba_outliers,
                                                  mage_stream stream)
{
    using namespace mage;
    MAGE_REQUIRE(K && first_pose && s && poses && matches && inliers && keyframe, MAGE_EINVAL, "null argument");
    if (frames == 0) return MAGE_OK;
    MAGE_REQUIRE(d_kp && d_desc && d_n, MAGE_EINVAL, "null features");
    MAGE_REQUIRE(pitch > 0 && pitch <= 4096, MAGE_EINVAL, "frame pitch must be in [1, 4096] keypoints");
    hipStream_t st = (hipStream_t)stream;
    MAGE_REQUIRE(s->local_map_keyframes <= (uint32_t)NKMAX, MAGE_EINVAL, "local_map_keyframes must be <= 8");
    // the observations' information is MapPointRefinementConfidence of each point's refinement
    // count (TrackLocalMap.cpp:473-475); the setting only names its count-0 value
    MAGE_REQUIRE(s->refinement_info == refinement_confidence(0), MAGE_EINVAL,
                 "refinement_info must be MapPointRefinementConfidence(0) = 1 - 1/1.5^2");
    const uint32_t NK = std::max(s->local_map_keyframes, 1u);
    const size_t qcap = s->local_map_keyframes > 0 ? (size_t)NK * pitch : 0;  // local-map queries
    TrackConst c{};
    c.fx = (float)K[0];
    c.fy = (float)K[1];
    c.cx = (float)K[2];
    c.cy = (float)K[3];
    for (int i = 0; i < 4; i++) c.K[i] = K[i];
    c.plane_z = plane_z;
    c.s = *s;
    c.cap = pitch;
    c.nk = NK;
    c.qcap = (uint32_t)qcap;
    c.acap = (uint32_t)(pitch + qcap);  // associations per keyframe = pose-BA 2 observations
    octave_factors(s->scale_factor, s->num_levels, c.fmax, c.fmin, &c.log2s);
    // one device allocation for the per-call scratch and outputs: track_bufs.hpp's table, run
    // once at base 0 for the size and the ring's range, once at the allocation
    const size_t lm_bytes = local_map_scratch_bytes(c.qcap);
    TrackBlock blk{};
    const BlockBinder lay = track_block(blk, c, frames, lm_bytes, nullptr);
    MAGE_REQUIRE(lay.ring_contiguous, MAGE_EINVAL, "track block: the keyframe ring's buffers are not consecutive");
    DeviceBuffer buf;
    mage_status r = buf.reserve(lay.bytes);
    if (r != MAGE_OK) return r;
    char* d = buf.as<char>();
    track_block(blk, c, frames, lm_bytes, d);
    TrackBufs& b = blk.b;
    const float e1 = (float)(s->initial_max_error * s->initial_max_error);
    const float e2 = (float)(s->final_max_error * s->final_max_error);

    auto fail = [&](mage_status st2) {
        (void)hipStreamSynchronize(st);
        buf.release();
        return st2;
    };
    if (hipMemsetAsync(d, 0, lay.bytes, st) != hipSuccess ||
        hipMemcpyAsync(blk.poses, first_pose, 96, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(MAGE_EDEVICE);
    hipLaunchKernelGGL(trk_init, dim3(1), dim3(TT), 0, st, b, c, d_kp, d_desc, d_n, blk.poses, blk.matches,
                       blk.inliers, blk.keyframe, blk.rstatus);
    const float radius[3] = {s->search_radius, s->wider_search_radius, s->extra_wider_search_radius};
    // project: frame f's prediction is its own launch (first frame, first frame after a local BA);
    // otherwise the previous frame's trk_finish_project made it
    auto enqueue = [&](uint32_t f, bool project) -> mage_status {
        const mage_keypoint* fk = d_kp + (size_t)f * pitch;
        const uint8_t* fd = d_desc + 32ull * f * pitch;
        const uint32_t* nf = d_n + f;
        const size_t slot = (size_t)(f % BAND_SLOTS);
        mage_status rr;
        if (f == 1 || f % BAND_CHUNK == 0) {  // build the band indices of frames [f, next chunk)
            const uint32_t end = std::min(frames, (f / BAND_CHUNK + 1) * BAND_CHUNK);
            if ((rr = radius_band_index_launch(fk, fd, nf, (int64_t)pitch, end - f, blk.bkeys + slot * pitch,
                                               blk.bxy + 2 * slot * pitch, blk.bdesc + 8 * slot * pitch, st)) !=
                MAGE_OK)
                return rr;
        }
        if (project)
            launch("track.project", trk_project, dim3(1), dim3(TT), 0, st, b, c, (int)f, (const double*)blk.poses);
        for (int k = 0; k < 3; k++) {
            // passes 0 and 1 end with the fallback decision for the next (radius_pass_weak, in the
            // pass's last workgroup: one dependent launch less per pass)
            const RadiusFollow follow{&b.ctl->ns, b.ctl->exec, b.nq + k + 1, k, s->min_matches, s->small_match_ratio};
            rr = radius_match_indexed(b.qkp, k < 2 ? b.qpos : nullptr, b.qdesc, (int64_t)pitch, b.nq + k, fk, fd,
                                      (int64_t)pitch, nf, blk.bkeys + slot * pitch, blk.bxy + 2 * slot * pitch,
                                      blk.bdesc + 8 * slot * pitch, 1, radius[k], s->max_hamming,
                                      s->min_hamming_difference, blk.rscratch, b.m + (size_t)k * pitch, pitch,
                                      b.mn + k, blk.rstatus, st, k < 2 ? &follow : nullptr);
            if (rr != MAGE_OK) return rr;
        }
        launch("track.gather", trk_gather, dim3(1), dim3(TT), 0, st, b, c, fk, (int)f, blk.matches);
        rr = mage_ba_pose_batch_device(1, b.pos3, b.r9, b.intr4, b.os1, b.pts1, b.uv1, b.info1, s->initial_steps,
                                       s->initial_huber, e1, b.pos3_o1, b.r9_o1, nullptr, b.out1, b.msq, nullptr,
                                       stream);
        if (rr != MAGE_OK) return rr;
        if (s->local_map_keyframes > 0) {
            launch("track.filter_lm", trk_filter_lm, dim3(1), dim3(TT), 0, st, b, c, nf);
            LocalMapArgs la{};
            la.qpos = b.lm_qpos;
            la.qoct = b.lm_qoct;
            la.qhide = b.lm_qhide;
            la.qdesc = b.lm_qdesc;
            la.nq = &b.ctl->lm_nq;
            la.q_cap = (uint32_t)qcap;
            la.tkp = fk;
            la.tdesc = fd;
            la.nt = nf;
            la.mask_words = b.lm_mask;
            la.radius = s->match_search_radius;
            la.max_dist = s->local_max_hamming;
            la.min_diff = s->local_min_hamming_difference;
            la.result = b.lm_res;
            la.status = b.lm_status;
            la.keys = blk.bkeys + slot * pitch;
            if ((rr = local_map_match_launch(la, b.lm_scratch, st)) != MAGE_OK) return rr;
            launch("track.lm_assemble", trk_lm_assemble, dim3(1), dim3(TT), 0, st, b, fk);
        } else {
            launch("track.filter", trk_filter, dim3(1), dim3(TT), 0, st, b, c, nf);
        }
        rr = mage_ba_pose_batch_device(1, b.pos3_o1, b.r9_o1, b.intr4, b.os2, b.pts2, b.uv2, b.info2, s->final_steps,
                                       s->final_huber, e2, b.pos3_o2, b.r9_o2, nullptr, b.out2, b.msq + 1, nullptr,
                                       stream);
        if (rr != MAGE_OK) return rr;
        launch("track.finish", trk_finish_project, dim3(1), dim3(TT), 0, st, b, c, (int)f, fk, fd, nf, blk.poses,
               blk.inliers, blk.keyframe, blk.rstatus, (int)(f + 1 < frames));
        return MAGE_OK;
    };
    if (ba_outliers)
        for (uint32_t f = 0; f < frames; f++) ba_outliers[f] = 0xFFFFFFFFu;
    if (!s->local_ba) {
        for (uint32_t f = 1; f < frames; f++)
            if ((r = enqueue(f, f == 1)) != MAGE_OK) return fail(r);
    } else {
        // Local BA after every new keyframe (MappingWorker; tracking.py local_bundle_adjust).  The
        // host stays up to two frames ahead; trk_finish of a keyframe frame sets ctl->halt (the
        // queued frames become no-ops) and reports it in mapped memory: the host drains the stream,
        // runs the BA on its copy of the keyframe ring, writes the ring back, clears the halt and
        // enqueues the following frames again.
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return fail(MAGE_EDEVICE);
        MappedBuffer prog;
        if ((r = prog.reserve(64)) != MAGE_OK) return fail(r);
        volatile uint32_t* hp = prog.host<volatile uint32_t>();
        hp[0] = 0;
        hp[1] = 0;
        b.prog = prog.device<uint32_t>();
        // a page-locked mirror of the device ring (one DMA copy each way per window), the halt-clear word
        Pinned<uint8_t> mirror;
        Pinned<uint32_t> zero;
        const size_t mbytes = lay.ring_end - lay.ring_begin;
        LocalBA L;
        PhaseClock prof;
        {
            const char* e = getenv("MAGE_TRACK_PROFILE");
            prof.on = e && *e == '1';
        }
        std::vector<uint8_t> changed(NK);
        uint32_t next = 1;
        bool need_project = true;  // the next enqueued frame makes its own prediction
        constexpr uint32_t DEPTH = 2;
        for (uint32_t f = 1; f < frames; f++) {
            while (next < frames && next <= f + DEPTH) {
                if ((r = enqueue(next, need_project)) != MAGE_OK) return fail(r);
                need_project = false;
                next++;
            }
            const auto t0 = std::chrono::steady_clock::now();
            while (hp[0] < f) {  // frame f done (trk_finish writes its index last)
                if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) {
                    if (hipStreamSynchronize(st) != hipSuccess) return fail(MAGE_EDEVICE);
                    if (hp[0] < f) return fail(MAGE_EDEVICE);
                }
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            if (hp[1] != f) continue;
            // a local BA: the halted frames drain, the ring comes to the host
            prof.start();
            if (hipStreamSynchronize(st) != hipSuccess) return fail(MAGE_EDEVICE);
            prof.mark("drain");
            Ctl hc;
            if (hipMemcpy(&hc, b.ctl, sizeof(Ctl), hipMemcpyDeviceToHost) != hipSuccess) return fail(MAGE_EDEVICE);
            if (!mirror.resize(mbytes) || !zero.resize(1)) return fail(MAGE_ENOMEM);
            *zero.data() = 0;
            if (hipMemcpyAsync(mirror.data(), d + lay.ring_begin, mbytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return fail(MAGE_EDEVICE);
            HostRing R = host_ring(c, frames, lm_bytes, mirror.data(), hc);
            prof.mark("ring D2H");
            std::fill(changed.begin(), changed.end(), 0);
            const BaWindow w = build_window(R, c, L);  // tracking.py local_bundle_adjust, on the host copy
            if (w.valid) {
                prof.mark("window");
                BundlerHandle H;  // destroyed at the end of this block, after the apply
                BaSolution o;
                if ((r = solve_window(w, c, L, dev, H, o, prof)) != MAGE_OK) return fail(r);
                apply_window(R, c, w, o.outl.data(), o.nout, o.pos.data(), o.r9.data(), o.xyz.data(), changed);
                prof.mark("get + apply");
                if (ba_outliers) ba_outliers[f] = o.nout;
            }
            // write back the changed slots, the frame's pose (= its keyframe's) and clear the halt:
            // queued on the stream ahead of the next frames (the ring's host copy is not touched
            // again before the next window's drain)
            bool any = false;
            for (uint32_t k = 0; k < NK; k++) any = any || changed[k];
            // one copy of the mirror from the points on (kf_pts .. kf_aalive: every field the window
            // changes; the unchanged slots and the associations go back as they came)
            if (any && hipMemcpyAsync(d + lay.moved_begin, mirror.data() + (lay.moved_begin - lay.ring_begin),
                                      lay.ring_end - lay.moved_begin, hipMemcpyHostToDevice, st) != hipSuccess)
                return fail(MAGE_EDEVICE);
            const uint32_t newest = (hc.kf_first + hc.kf_count - 1) % NK;
            if (hipMemcpyAsync(blk.poses + 12ull * f, &R.v.kf_pose[12 * newest], 96, hipMemcpyHostToDevice, st) !=
                    hipSuccess ||
                hipMemcpyAsync(&b.ctl->halt, zero.data(), 4, hipMemcpyHostToDevice, st) != hipSuccess)
                return fail(MAGE_EDEVICE);
            prof.mark("write-back");
            prof.flush();
            next = f + 1;
            need_project = true;
        }
        // the last window's write-back reads the pinned ring: done before the ring is freed
        if (hipStreamSynchronize(st) != hipSuccess) return fail(MAGE_EDEVICE);
    }
    if (hipGetLastError() != hipSuccess) return fail(MAGE_EDEVICE);
    uint32_t rst = 0, lst = 0;
    if (hipMemcpyAsync(poses, blk.poses, 96ull * frames, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(matches, blk.matches, 4ull * frames, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(inliers, blk.inliers, 4ull * frames, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(keyframe, blk.keyframe, frames, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&rst, blk.rstatus, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&lst, b.lm_status, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(MAGE_EDEVICE);
    buf.release();
    MAGE_REQUIRE(!(rst & 1u), MAGE_ECAPACITY, "a frame has more than 4096 keypoints");
    MAGE_REQUIRE(!(rst & 2u), MAGE_ECAPACITY, "a frame's keypoint count exceeds the frame pitch");
    MAGE_REQUIRE(lst == 0, MAGE_ECAPACITY, "local-map search: a frame has more than 4096 keypoints");
    return MAGE_OK;
}
