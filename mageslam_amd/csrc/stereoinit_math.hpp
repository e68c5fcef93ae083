// stereoinit_math.hpp — what StereoMapInit's device stage decides per keypoint and per match, shared
// by the kernels (stereoinit.hip) and their plain C++ twin (stereoinit.cpp): IsWithinArea
// (Utils/cv.h:421-427) for the crop mask and the filter sequence of MapInitialization::
// TriangulatePoints (Tracking/MapInitialization.cpp:945-984) over the arithmetic of
// newpoints_math.hpp, which is used as it is.  float32 throughout, in the reference's expression
// order; both translation units are built with -ffp-contract=off, so the two sides give the same
// bits.
#pragma once

#include "newpoints_math.hpp"
#include "track_math.hpp"

namespace mage {
namespace stereoinit {

using newpoints::Frame;

constexpr int ST_MAX_KP = 4096;  // keypoints per frame (the two-way matcher's limit)

enum Verdict : uint8_t {
    ST_ACCEPTED = MAGE_ST_ACCEPTED,
    ST_EPIPOLAR = MAGE_ST_EPIPOLAR,
    ST_BEHIND = MAGE_ST_BEHIND,
    ST_DISTANCE_RATIO = MAGE_ST_DISTANCE_RATIO,
    ST_OCTAVE = MAGE_ST_OCTAVE,
    ST_BAD_INDEX = MAGE_ST_BAD_INDEX,
};

enum : uint32_t { ST_STATUS_OVER_LIMIT = 1u, ST_STATUS_OVER_CAP = 2u };

// nullptr when the settings can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_settings(const mage_stereo_init_settings* s)
{
    if (!s) return "null settings";
    if (s->struct_size != sizeof(mage_stereo_init_settings)) return "struct_size is not sizeof(mage_stereo_init_settings)";
    if (!(s->max_epipolar_error >= 0.f)) return "max_epipolar_error must be >= 0";
    if (!(s->min_accepted_distance_ratio >= 0.f)) return "min_accepted_distance_ratio must be >= 0";
    if (!(s->max_outlier_error > 0.f)) return "max_outlier_error must be > 0";
    if (!(s->initialization_tether_strength >= 0.f)) return "initialization_tether_strength must be >= 0";
    if (!(s->max_pose_contribution_z >= 0.f)) return "max_pose_contribution_z must be >= 0";
    if (!(s->amount_ba_can_change_pose >= 1.f)) return "amount_ba_can_change_pose must be >= 1";
    if (!(s->max_depth_meters > 0.f)) return "max_depth_meters must be > 0";
    if (s->max_hamming_distance < -1 || s->max_hamming_distance > 256) return "max_hamming_distance must be in [-1, 256]";
    if (s->min_hamming_difference < 0 || s->min_hamming_difference > 256) return "min_hamming_difference must be in [0, 256]";
    if (s->ba_num_steps_per_run < 1) return "ba_num_steps_per_run must be >= 1";
    if (s->ba_min_steps > s->ba_num_steps) return "ba_min_steps must be <= ba_num_steps";
    if (!(s->ba_huber_width > 0.f) || !(s->ba_huber_width_scale > 0.f)) return "ba_huber_width and its scale must be > 0";
    if (!(s->ba_max_outlier_error > 0.f) || !(s->ba_max_outlier_error_scale_factor > 0.f))
        return "ba_max_outlier_error and its scale factor must be > 0";
    if (!(s->ba_min_mean_square_error >= 0.f)) return "ba_min_mean_square_error must be >= 0";
    return nullptr;
}

// IsWithinArea (Utils/cv.h:421-427), literally: the right edge is outside the area, the bottom
// edge is inside it.  The int sums convert to float for the comparisons, as in the reference.
NP_HD bool within_area(float x, float y, const int32_t* crop)
{
    return (x >= (float)crop[0] && x < (float)(crop[0] + crop[2])) && (y >= (float)crop[1] && y <= (float)(crop[1] + crop[3]));
}

// Everything the matches of a stereo pair share: frame 0 is TriangulatePoints' reference frame
// (the matches' queryIdx side), frame 1 its current frame (trainIdx).
struct StereoPair {
    Frame f0, f1;
    float f_1_to_0[9];  // fundamentalMatrixKcToKi: current -> reference (:928)
    float f_0_to_1[9];  // fundamentalMatrixKiToKc: reference -> current (:929)
    float baseline;     // |C0 - C1| (:968-969)
};

// pos3 / r9 / intr4: frame 0 then frame 1 (6 / 18 / 8 floats), as mage_ba_set_cameras takes them.
NP_HD void make_stereo_pair(const float* pos3, const float* r9, const float* intr4, StereoPair& p)
{
    newpoints::make_frame(pos3, r9, intr4, p.f0);
    newpoints::make_frame(pos3 + 3, r9 + 9, intr4 + 4, p.f1);
    newpoints::fundamental(p.f1, p.f0, p.f_1_to_0);
    newpoints::fundamental(p.f0, p.f1, p.f_0_to_1);
    const float d[3] = {p.f0.C[0] - p.f1.C[0], p.f0.C[1] - p.f1.C[1], p.f0.C[2] - p.f1.C[2]};
    p.baseline = sqrtf(newpoints::dot3(d, d));
}

// One match through TriangulatePoints' filters (:945-984): the first failing check's verdict, or
// ST_ACCEPTED with the point in X.  (x0, y0, o0) is frame 0's keypoint, (x1, y1, o1) frame 1's.
// TriangulatePointWorldSpace gets the reference frame first (:952), where new-points passes Kc.
NP_HD uint8_t stereo_match_geometry(const StereoPair& p, float two_max_epipolar, float min_ratio, float x0, float y0,
                                    int o0, float x1, float y1, int o1, float* X, bool& parallel)
{
    const float d_kc_ki = newpoints::epipolar_distance(p.f_1_to_0, x1, y1, x0, y0);
    const float d_ki_kc = newpoints::epipolar_distance(p.f_0_to_1, x0, y0, x1, y1);
    parallel = false;
    if (d_ki_kc + d_kc_ki > two_max_epipolar) return ST_EPIPOLAR;
    newpoints::triangulate(p.f0, p.f1, x0, y0, x1, y1, X, parallel);
    if (newpoints::depth_of(p.f0, X) <= 0.f || newpoints::depth_of(p.f1, X) <= 0.f) return ST_BEHIND;
    const float v[3] = {X[0] - p.f0.C[0], X[1] - p.f0.C[1], X[2] - p.f0.C[2]};
    const float d0 = sqrtf(newpoints::dot3(v, v));
    if (d0 / p.baseline < min_ratio) return ST_DISTANCE_RATIO;
    if (o0 != o1) return ST_OCTAVE;
    return ST_ACCEPTED;
}

}  // namespace stereoinit
}  // namespace mage
