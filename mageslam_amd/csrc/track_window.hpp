// track_window.hpp — the device loop's local BA between frames (MappingWorker's BundleAdjustTask),
// its two pure host halves: build_window / apply_window, the twins of tracking.py build_ba_window /
// apply_ba_window over the keyframe ring copied from the device.  No HIP or BundlerLib call
// (track.hip's solve_window makes those), so a plain host program can run them.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "track_bufs.hpp"
#include "track_math.hpp"

namespace mage {
namespace track {

struct LocalBA {  // MappingWorker's CurrentLambda and CosVisThreashold, persisted across the windows
    bool have_lambda = false;
    float lambda = 0.f;
    bool have_theta = false;
    uint32_t theta = 0;
};

struct BaObs {
    uint32_t cam, owner, idx;  // ring positions of the observer and the point's owner, point index
    float u, v;
    uint32_t kind, src;  // 0: own (point index), 1: association (entry)
};

// One local BA problem in BundlerLib's boundary layout and how it maps back to the ring.
struct BaWindow {
    bool valid = false;  // false: no window (fewer than two keyframes, nothing kept or nothing free)
    uint32_t nr = 0;     // cameras: the ring's keyframes, ascending id
    uint32_t slot_of[NKMAX] = {};
    uint32_t freemask = 0;
    std::vector<BaObs> kept;     // the observations, per camera: own points, then associations
    std::vector<uint32_t> cam, pt;
    std::vector<float> uv, info, xyz;
    std::vector<uint64_t> keys;  // the points (xyz), ascending (owner ring position << 32 | index)
    std::vector<float> pos3, r9, intr;  // view-space t, Eigen column-major R, {cx, cy, fx, fy}
    std::vector<uint8_t> fixed;
    uint32_t steps = 0;  // NumStepsPerRun and the Huber width after the connectivity scaling
    float huber = 0.f;
    uint32_t theta = 0;  // the covisibility threshold to persist (also left in LocalBA)
};

inline float bits_float(int v)
{
    float f;
    std::memcpy(&f, &v, 4);
    return f;
}

// GetMapPointsAndDistantKeyframes + BuildDataForG2O over the ring (tracking.build_ba_window).
inline BaWindow build_window(const HostRing& R, const TrackConst& c, LocalBA& L)
{
    BaWindow w;
    w.theta = L.have_theta ? L.theta : c.s.covis_min_threshold;
    const uint32_t nr = R.ctl.kf_count;
    if (nr < 2) return w;
    w.nr = nr;
    uint32_t* slot_of = w.slot_of;
    for (uint32_t r = 0; r < nr; r++) slot_of[r] = (R.ctl.kf_first + r) % R.nk;
    auto pos_of = [&](int id) -> int {
        for (uint32_t r = 0; r < nr; r++)
            if ((int)R.ctl.kf_id[slot_of[r]] == id) return (int)r;
        return -1;
    };
    std::vector<BaObs> obs;
    obs.reserve((size_t)nr * R.cap * 2);
    for (uint32_t r = 0; r < nr; r++) {
        const uint32_t sl = slot_of[r];
        const size_t o = (size_t)sl * R.cap;
        for (uint32_t i = 0; i < R.ctl.kf_n[sl]; i++)
            if (R.v.kf_own[o + i]) obs.push_back({r, r, i, R.v.kf_kp[o + i].x, R.v.kf_kp[o + i].y, 0, i});
        const size_t ao = (size_t)sl * R.acap;
        for (uint32_t a = 0; a < R.ctl.kf_an[sl]; a++) {
            const int4 e = R.v.kf_assoc[ao + a];
            const int ow = pos_of(e.x);
            if (R.v.kf_aalive[ao + a] && ow >= 0)
                obs.push_back({r, (uint32_t)ow, (uint32_t)e.y, bits_float(e.z), bits_float(e.w), 1, a});
        }
    }
    // the window's points, ascending (owner, index): a dense (ring position, index) map instead of
    // a sorted key list (the window build runs between frames, on the loop's critical path)
    std::vector<int32_t> pmap((size_t)nr * R.cap, -1);
    uint32_t freemask = 0;
    if (c.s.ba_free_keyframes > 0) {
        // the newest ba_free_keyframes free, the oldest fixed (at least one); the points they observe
        const uint32_t nfix = nr > c.s.ba_free_keyframes ? nr - c.s.ba_free_keyframes : 1u;
        for (uint32_t r = nfix; r < nr; r++) freemask |= 1u << r;
        for (const BaObs& ob : obs)
            if (ob.cam >= nfix) pmap[(size_t)ob.owner * R.cap + ob.idx] = 0;
    } else {
        // GetMapPointsAndDistantKeyframes (ThreadSafeMap.cpp:888-957; tracking.py covisible_window):
        // per point the mask of ring keyframes observing it; the covisibility weight of keyframe r
        // to the newest one is the count of points both observe (CovisibilityGraph.cpp:131-170)
        std::vector<uint8_t> seen((size_t)nr * R.cap, 0);
        for (const BaObs& ob : obs) seen[(size_t)ob.owner * R.cap + ob.idx] |= (uint8_t)(1u << ob.cam);
        const uint32_t last = nr - 1;
        uint32_t weight[NKMAX] = {};
        for (uint8_t m : seen)
            if (m >> last & 1u)
                for (uint32_t r = 0; r < last; r++) weight[r] += m >> r & 1u;
        uint32_t theta = w.theta, kc = 0;
        for (uint32_t step = 0; step <= c.s.covis_max_steps; step++) {
            kc = 1u << last;
            for (uint32_t r = 0; r < last; r++)
                if (weight[r] >= theta) kc |= 1u << r;
            size_t n_assoc = 0;
            for (const BaObs& ob : obs) n_assoc += (seen[(size_t)ob.owner * R.cap + ob.idx] & kc) != 0;
            if (n_assoc > c.s.ba_upper_connections) {
                theta += c.s.covis_ba_step;
                continue;
            }
            if (n_assoc < c.s.ba_lower_connections && theta > c.s.covis_min_threshold) {
                theta -= c.s.covis_ba_step;
                continue;
            }
            break;
        }
        w.theta = L.theta = theta;
        L.have_theta = true;
        for (size_t q = 0; q < seen.size(); q++)
            if (seen[q] & kc) pmap[q] = 0;
        for (uint32_t r = 0; r < nr; r++)  // the map's first keyframe stays fixed (ThreadSafeMap.cpp:89)
            if ((kc >> r & 1u) && R.ctl.kf_id[slot_of[r]] != 0) freemask |= 1u << r;
    }
    w.freemask = freemask;
    std::vector<uint64_t>& keys = w.keys;
    for (uint32_t r = 0; r < nr; r++)
        for (uint32_t i = 0; i < R.cap; i++)
            if (pmap[(size_t)r * R.cap + i] == 0) {
                pmap[(size_t)r * R.cap + i] = (int32_t)keys.size();
                keys.push_back((uint64_t)r << 32 | i);
            }
    w.kept.reserve(obs.size());
    w.cam.reserve(obs.size());
    w.pt.reserve(obs.size());
    w.uv.reserve(2 * obs.size());
    for (const BaObs& ob : obs) {
        const int32_t p = pmap[(size_t)ob.owner * R.cap + ob.idx];
        if (p < 0) continue;
        w.kept.push_back(ob);
        w.cam.push_back(ob.cam);
        w.pt.push_back((uint32_t)p);
        w.uv.push_back(ob.u);
        w.uv.push_back(ob.v);
    }
    if (w.kept.empty() || freemask == 0) return w;
    const uint32_t P = (uint32_t)keys.size(), E = (uint32_t)w.kept.size();
    w.xyz.resize(3ull * P);
    std::vector<uint32_t> pref(P);
    for (uint32_t q = 0; q < P; q++) {
        const uint32_t sl = slot_of[keys[q] >> 32], i = (uint32_t)(keys[q] & 0xFFFFFFFFu);
        const size_t o = (size_t)sl * R.cap + i;
        for (int j = 0; j < 3; j++) w.xyz[3 * q + j] = R.v.kf_pts[3 * o + j];
        pref[q] = R.v.kf_ref[o];
    }
    for (uint32_t e = 0; e < E; e++) w.info.push_back(refinement_confidence(pref[w.pt[e]]));
    w.pos3.resize(3 * nr);
    w.r9.resize(9 * nr);
    w.intr.resize(4 * nr);
    w.fixed.assign(nr, 0);
    for (uint32_t r = 0; r < nr; r++) w.fixed[r] = (freemask >> r & 1u) ? 0 : 1;
    for (uint32_t r = 0; r < nr; r++) {
        const double* ps = &R.v.kf_pose[12 * slot_of[r]];
        to_bundler(ps, ps + 9, &w.pos3[3 * r], &w.r9[9 * r]);
        w.intr[4 * r] = (float)c.K[2];
        w.intr[4 * r + 1] = (float)c.K[3];
        w.intr[4 * r + 2] = (float)c.K[0];
        w.intr[4 * r + 3] = (float)c.K[1];
    }
    // NumStepsPerRun / Huber width by the connectivity ratio (MappingWorker.cpp:254-263)
    const uint32_t ratio = c.s.ba_upper_connections / E;
    w.steps = c.s.ba_steps_per_run;
    w.huber = c.s.ba_huber;
    if (ratio > 0) {
        w.steps = w.steps * (uint32_t)((float)ratio * c.s.ba_low_connectivity_scale);
        w.huber = w.huber * powf(c.s.ba_huber_scale, (float)ratio);
    }
    w.valid = true;
    return w;
}

// AdjustPosesAndMapPoints (tracking.apply_ba_window): the outliers (indices into w.kept)
// unassociated, free poses, points (+ refinement), attributes; slot_changed[slot] = 1 where written.
inline void apply_window(HostRing& R, const TrackConst& c, const BaWindow& w, const uint32_t* outl, uint32_t nout,
                         const float* pos_o, const float* r9_o, const float* xyz_o, std::vector<uint8_t>& slot_changed)
{
    const uint32_t* slot_of = w.slot_of;
    const uint32_t P = (uint32_t)w.keys.size(), E = (uint32_t)w.kept.size();
    for (uint32_t k = 0; k < std::min(nout, E); k++) {
        const BaObs& ob = w.kept[outl[k]];
        const uint32_t sl = slot_of[ob.cam];
        if (ob.kind == 0)
            R.v.kf_own[(size_t)sl * R.cap + ob.src] = 0;
        else
            R.v.kf_aalive[(size_t)sl * R.acap + ob.src] = 0;
        slot_changed[sl] = 1;
    }
    for (uint32_t r = 0; r < w.nr; r++) {
        if (!(w.freemask >> r & 1u)) continue;
        double* ps = &R.v.kf_pose[12 * slot_of[r]];
        from_bundler(&pos_o[3 * r], &r9_o[9 * r], ps, ps + 9);
        slot_changed[slot_of[r]] = 1;
    }
    for (uint32_t q = 0; q < P; q++) {
        const uint32_t sl = slot_of[w.keys[q] >> 32], i = (uint32_t)(w.keys[q] & 0xFFFFFFFFu);
        const size_t o = (size_t)sl * R.cap + i;
        for (int j = 0; j < 3; j++) R.v.kf_pts[3 * o + j] = xyz_o[3 * q + j];
        R.v.kf_ref[o] += 1;
        slot_changed[sl] = 1;
    }
    for (uint32_t q = 0; q < P; q++) {  // a loop of its own: fused with the one above it runs 2.4x slower
        const uint32_t sl = slot_of[w.keys[q] >> 32], i = (uint32_t)(w.keys[q] & 0xFFFFFFFFu);
        const size_t o = (size_t)sl * R.cap + i;
        float R32[9], t32[3], C[3];
        pose_f32(&R.v.kf_pose[12 * sl], &R.v.kf_pose[12 * sl + 9], R32, t32);
        world_position(R32, t32, C);
        point_attributes(&R.v.kf_pts[3 * o], C, R.v.kf_kp[o].octave, c.fmin, c.fmax, &R.v.kf_mvd[3 * o], R.v.kf_dmin[o],
                         R.v.kf_dmax[o]);
    }
}

}  // namespace track
}  // namespace mage
