// loopclose_math.hpp — the map-point refresh of the mapping thread's cheap loop closure, shared by
// the kernel (loopclose.hip) and its plain C++ twin (loopclose.cpp).  MapPoint::AddKeyframeAssociation
// (Map/MapPoint.cpp:35-46) runs UpdateRepresentativeDescriptor (:80-130) and
// UpdateMeanViewDirectionAndDistances (:132-155) after every association that CheapLoopClosure
// (Tasks/MappingWorker.cpp:20-73, through InsertKeyframe, Map/ThreadSafeMap.cpp:242-249) and
// TryConnectMapPoints (ThreadSafeMap.cpp:715-787) make.  float32 throughout, in the reference's
// expression order, the conventions those of track_math.hpp's one-keyframe case (point_attributes):
// Normalize (Utils/cv.h:287-296) takes the norm as sqrtf of the float dot product and divides by
// multiplying with the float reciprocal.  Both translation units are built with -ffp-contract=off,
// and +, -, *, / and sqrtf are correctly rounded on host and device, so the two sides give the same
// bits.  No HIP header: the twin also builds as plain host C++ on its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include "newpoints_math.hpp"  // NP_HD, dot3: the same expressions, not written again

namespace mage {
namespace loopclose {

using newpoints::dot3;

constexpr int LC_MAX_LEVELS = 8;      // pyramid levels (MAGE_MAX_LEVELS)
constexpr int LC_MAX_POINTS = 1024;   // sampled points per closure
static_assert(sizeof(mage_map_point_obs) == 64 && alignof(mage_map_point_obs) >= 4, "mage_map_point_obs is 64 bytes");
static_assert(sizeof(mage_map_point_state) == 40, "mage_map_point_state is 40 bytes");

// ComputeDMax / ComputeDMin factors per octave (Map/MappingMath.h:32-40), the tables of
// track_math.hpp's octave_factors.  Host only: powf stays on the host.
struct Tables {
    float fmin[LC_MAX_LEVELS], fmax[LC_MAX_LEVELS];
};

// nullptr when the settings can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_settings(const mage_loop_closure_settings* s)
{
    if (!s) return "null settings";
    if (s->struct_size != sizeof(mage_loop_closure_settings)) return "struct_size is not sizeof(mage_loop_closure_settings)";
    if (s->max_map_points < 1 || s->max_map_points > (uint32_t)LC_MAX_POINTS) return "max_map_points must be in 1..1024";
    if (!(s->search_radius >= 0.f)) return "search_radius must be >= 0";
    if (s->width < 1 || s->height < 1) return "image size must be positive";
    if (s->num_levels < 1 || s->num_levels > (uint32_t)LC_MAX_LEVELS) return "num_levels must be in 1..8";
    if (!(s->pyramid_scale > 1.f)) return "pyramid_scale must be > 1";
    if (s->closure_max_hamming_distance < -1 || s->closure_max_hamming_distance > 256 ||
        s->connect_max_hamming_distance < -1 || s->connect_max_hamming_distance > 256)
        return "max_hamming_distance must be in [-1, 256]";
    return nullptr;
}

inline Tables make_tables(const mage_loop_closure_settings& s)
{
    Tables t{};
    for (int o = 0; o < LC_MAX_LEVELS; o++) {
        t.fmax[o] = powf(s.pyramid_scale, (float)s.num_levels - ((float)o + 0.5f));
        t.fmin[o] = powf(s.pyramid_scale, 0.f - ((float)o + 0.5f));
    }
    return t;
}

// Normalize (Utils/cv.h:287-296) in place.
NP_HD void normalize3(float v[3])
{
    const float d = sqrtf(dot3(v, v));
    if (d != 0) {
        const float inv = 1.f / d;
        for (int j = 0; j < 3; j++) v[j] = v[j] * inv;
    }
}

// Normalize(CalculateDeltaWorldPositionFromKeyframe) (MapPoint.cpp:143-144, 157-162): P - C, unit.
NP_HD void view_direction(const float P[3], const float C[3], float out[3])
{
    for (int j = 0; j < 3; j++) out[j] = P[j] - C[j];
    normalize3(out);
}

// The state of a point with n > 0 observations once its representative observation `rep` (centre C,
// keypoint octave) and the sum `m` of its view directions are known (MapPoint.cpp:146-154).
NP_HD void finish_state(const Tables& t, const float P[3], const float m[3], const float C[3], int octave, int rep, int n,
                        mage_map_point_state& st)
{
    float v[3] = {m[0], m[1], m[2]};
    normalize3(v);
    const float dl[3] = {C[0] - P[0], C[1] - P[1], C[2] - P[2]};
    const float dist = sqrtf((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]);
    const int o = octave < 0 ? 0 : (octave > LC_MAX_LEVELS - 1 ? LC_MAX_LEVELS - 1 : octave);
    for (int j = 0; j < 3; j++) {
        st.pos[j] = P[j];
        st.mvd[j] = v[j];
    }
    st.dmin = dist * t.fmin[o];
    st.dmax = dist * t.fmax[o];
    st.rep = rep;
    st.n_obs = n;
}

// A point without observations (MapPoint.cpp:85-88, 136-139).
NP_HD void empty_state(const float P[3], mage_map_point_state& st)
{
    for (int j = 0; j < 3; j++) {
        st.pos[j] = P[j];
        st.mvd[j] = 0.f;
    }
    st.dmin = 0.f;
    st.dmax = 0.f;
    st.rep = -1;
    st.n_obs = 0;
}

// ------------------------------------------------------------------------------------------
// CheapLoopClosure (Tasks/MappingWorker.cpp:20-73) and TryConnectMapPoints
// (Map/ThreadSafeMap.cpp:715-787): the sampling and what a point and a keyframe decide before
// the descriptor search.
// ------------------------------------------------------------------------------------------
constexpr int LC_MAX_KP = 4096;  // keypoints per keyframe (OT_MAX_TARGETS)

enum LcVerdict : uint8_t {
    LC_ASSOCIATED = MAGE_LC_ASSOCIATED,
    LC_NOT_SAMPLED = MAGE_LC_NOT_SAMPLED,
    LC_HAS_POINT = MAGE_LC_HAS_POINT,
    LC_BEHIND = MAGE_LC_BEHIND,
    LC_BORDER = MAGE_LC_BORDER,
    LC_ANGLE = MAGE_LC_ANGLE,
    LC_DISTANCE = MAGE_LC_DISTANCE,
    LC_OCTAVE = MAGE_LC_OCTAVE,
    LC_NO_MATCH = MAGE_LC_NO_MATCH,
};
static_assert(LC_BEHIND == newpoints::NA_BEHIND + 1 && LC_NO_MATCH == newpoints::NA_NO_MATCH + 1,
              "the gate's verdicts are newpoints' shifted by one");

// The settings as the loops use them: the gate of both stages (they differ in the matcher pair
// only), the octave tables, the limits.
struct Consts {
    newpoints::AssocConsts gate;  // max_dist / min_diff: the closure's
    int connect_max_dist, connect_min_diff;
    Tables tables;
    uint32_t max_points, min_keyframes;
};

inline Consts make_consts(const mage_loop_closure_settings& s)
{
    Consts c{};
    c.gate.radius = s.search_radius;
    c.gate.border = s.image_border - s.search_radius / 2.0f;
    c.gate.cos_max_angle = cosf(s.min_view_degrees * (3.14159265358979323846f / 180.f));
    c.gate.log2s = (float)log2((double)s.pyramid_scale);
    c.gate.image_w = (float)s.width;
    c.gate.image_h = (float)s.height;
    c.gate.num_levels = (int)s.num_levels;
    c.gate.max_dist = s.closure_max_hamming_distance;
    c.gate.min_diff = s.closure_min_hamming_difference;
    c.connect_max_dist = s.connect_max_hamming_distance;
    c.connect_min_diff = s.connect_min_hamming_difference;
    c.tables = make_tables(s);
    c.max_points = s.max_map_points;
    c.min_keyframes = s.min_keyframes;
    return c;
}

// nullptr when the problem's arguments can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_problem(const mage_loop_closure_problem* p)
{
    if (!p) return "null problem";
    if (p->struct_size != sizeof(mage_loop_closure_problem)) return "struct_size is not sizeof(mage_loop_closure_problem)";
    if (p->obs_pitch < 1 || p->obs_pitch > (int64_t)MAGE_MP_MAX_OBS) return "obs_pitch must be in 1..65536";
    if (!p->counts || !p->status) return "null argument";
    if (p->n_map && !(p->state && p->obs && p->sample_index && p->closure && p->closure_verdict)) return "null argument";
    if (!p->ki_pos3 || !p->ki_r9 || !p->ki_intr4) return "null argument";
    if (p->n_ki && !(p->ki_kp && p->ki_desc && p->ki_point && p->ki_mask)) return "null argument";
    if (p->n_kf) {
        if (!(p->kf_id && p->kf_pos3 && p->kf_r9 && p->kf_intr4 && p->kf_start && p->kf_modified)) return "null argument";
        if (p->n_map && !(p->connect && p->connect_verdict)) return "null argument";
        for (uint32_t k = 0; k < p->n_kf; k++)
            if (p->kf_start[k] > p->kf_start[k + 1]) return "start offsets must not decrease";
        if (p->kf_start[p->n_kf] != p->kf_start[0] && !(p->kf_kp && p->kf_desc && p->kf_point && p->kf_mask))
            return "null argument";
    }
    return nullptr;
}

// GetSampleOfMapPoints (Map/Map.cpp:319-333) by index arithmetic.  The reference's counter is
// v(i) = (uint32)(offset + 1 + i) and point i is sampled iff v(i) % step == 0.  Over i = 0 .. n - 1
// the counter wraps at most once: it runs c0, c0 + 1, ... for the first w = min(n, 2^32 - c0)
// points and 0, 1, ... for the rest.  In the first run the sampled points are i0, i0 + step, ...
// with i0 = (step - c0 % step) % step; in the second w, w + step, ... (v = 0 is a multiple).
// Without a wrap the sample has at most ceil(n / step) <= max points; at the wrap both runs can end
// and start on a multiple, one more than max, and the sample is cut at max.
struct Sampler {
    uint32_t step, i0, w, n_a, count;
};

NP_HD Sampler make_sampler(uint32_t n, uint32_t max, uint32_t offset)
{
    Sampler s;
    s.step = n / max + 1u;
    const uint32_t c0 = offset + 1u;
    const uint64_t room = 0x100000000ull - (uint64_t)c0;
    s.w = (uint64_t)n < room ? n : (uint32_t)room;
    s.i0 = (s.step - c0 % s.step) % s.step;
    s.n_a = s.i0 < s.w ? (s.w - 1u - s.i0) / s.step + 1u : 0u;
    const uint32_t n_b = s.w < n ? (n - s.w - 1u) / s.step + 1u : 0u;
    const uint64_t all = (uint64_t)s.n_a + n_b;
    s.count = all < max ? (uint32_t)all : max;
    return s;
}

// The map index of sample j < count.
NP_HD uint32_t sample_index(const Sampler& s, uint32_t j)
{
    return j < s.n_a ? s.i0 + j * s.step : s.w + (j - s.n_a) * s.step;
}

// The place of map point i < n in the sample, or -1.
NP_HD int sample_slot(const Sampler& s, uint32_t i)
{
    uint32_t j;
    if (i < s.w) {
        if (i < s.i0 || (i - s.i0) % s.step != 0) return -1;
        j = (i - s.i0) / s.step;
    } else {
        if ((i - s.w) % s.step != 0) return -1;
        j = s.n_a + (i - s.w) / s.step;
    }
    return j < s.count ? (int)j : -1;
}

// ProjectMapPointIntoCurrentFrame (TrackLocalMap.cpp:325-370) up to the descriptor search for a
// point in state st: newpoints' project_gate (the same gate) with the verdicts renamed.  A point
// that passes but has no representative observation cannot be matched: LC_NO_MATCH, pass false.
NP_HD uint8_t gate_point(const newpoints::AssocConsts& c, const newpoints::Frame& f, const float* intr4,
                         const mage_map_point_state& st, float& x, float& y, int& octave, bool& pass)
{
    mage_new_point pt{};
    for (int j = 0; j < 3; j++) {
        pt.position[j] = st.pos[j];
        pt.mean_view_dir[j] = st.mvd[j];
    }
    pt.d_min = st.dmin;
    pt.d_max = st.dmax;
    const uint8_t v = newpoints::project_gate(c, f, intr4, pt, x, y, octave);
    pass = v == newpoints::NA_NO_MATCH && st.rep >= 0 && st.rep < st.n_obs;
    return (uint8_t)(v + 1);
}

// The observation keyframe (centre C, id) makes of keypoint kp with descriptor desc.
NP_HD mage_map_point_obs make_obs(const uint8_t* desc, const float C[3], int octave, int keyframe_id)
{
    mage_map_point_obs o{};
    for (int b = 0; b < 32; b++) o.desc[b] = desc[b];
    for (int j = 0; j < 3; j++) o.centre[j] = C[j];
    o.octave = octave;
    o.keyframe_id = keyframe_id;
    return o;
}

}  // namespace loopclose
}  // namespace mage
