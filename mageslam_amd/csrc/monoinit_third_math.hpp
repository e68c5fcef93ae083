// monoinit_third_math.hpp — the third frame of TryIntializeMapWithProvidedFrames
// (Tracking/MapInitialization.cpp:695-840), shared by the kernels (monoinit_third.hip) and their plain
// C++ twin (monoinit_third.cpp): the midpoint pose (:711-714), ProjectUndistorted
// (Tracking/Reprojection.cpp:26-42), the choice between the two queries' matches (:766-798), the two
// gates (:803, :835) and the layout of the device chain's scratch.
//
// Only + - * / and sqrtf appear here, every sum is written in one fixed order, and both translation
// units are built with -ffp-contract=off, so host and gfx950 give the same bits (the rule of
// monoinit_math.hpp).
#pragma once

#include "newpoints_math.hpp"
#include "track_math.hpp"

namespace mage {
namespace monothird {

constexpr int M3_MAX_KP = 4096;      // third-frame keypoints per problem (mask bits and taker entries in LDS)
constexpr int M3_MAX_POINTS = 4096;  // map points per problem

enum : uint32_t { M3_OK = MAGE_M3_OK, M3_FEW_MATCHES = MAGE_M3_FEW_MATCHES, M3_FEW_AFTER_CULL = MAGE_M3_FEW_AFTER_CULL };
enum : uint32_t { M3_STATUS_OVER_LIMIT = MAGE_M3_STATUS_OVER_LIMIT, M3_STATUS_BAD_INDEX = MAGE_M3_STATUS_BAD_INDEX };
enum : uint8_t {
    M3_PT_BEHIND = MAGE_M3_PT_BEHIND,
    M3_PT_NO_MATCH = MAGE_M3_PT_NO_MATCH,
    M3_PT_FRAME0 = MAGE_M3_PT_FRAME0,
    M3_PT_FRAME1 = MAGE_M3_PT_FRAME1,
    M3_PT_CULLED = MAGE_M3_PT_CULLED,
};

// nullptr when the third frame's settings can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_settings(const mage_mono_init_settings* s)
{
    if (!s) return "null settings";
    if (s->struct_size != sizeof(mage_mono_init_settings)) return "struct_size is not sizeof(mage_mono_init_settings)";
    if (!(s->extra_frame_search_radius >= 0.f)) return "extra_frame_search_radius must be >= 0";
    if (!(s->extra_frame_huber_width >= 0.f)) return "extra_frame_huber_width must be >= 0";
    if (!(s->extra_frame_max_outlier_error >= 0.f)) return "extra_frame_max_outlier_error must be >= 0";
    if (!(s->min_third_frame_match_percentage == s->min_third_frame_match_percentage))
        return "min_third_frame_match_percentage must be a number";
    if (s->five_point_max_hamming_distance < -1 || s->five_point_max_hamming_distance > 256 ||
        s->extra_frame_max_hamming_distance < -1 || s->extra_frame_max_hamming_distance > 256)
        return "the maximal Hamming distances must be in [-1, 256]";
    if (s->five_point_min_hamming_difference < 0 || s->five_point_min_hamming_difference > 256 ||
        s->extra_frame_min_hamming_difference < 0 || s->extra_frame_min_hamming_difference > 256)
        return "the minimal Hamming differences must be in [0, 256]";
    return nullptr;
}

// The settings as the loops read them.  Query 0 is frame 0's descriptor under
// ExtraFrameMatchingSettings (:734-746), query 1 frame 1's under FivePointMatchingSettings (:751-763).
struct Consts {
    float radius;   // ExtraFrame_SearchRadius
    float min_pct;  // MinThirdFrameMatchPercentage
    int max_dist[2], min_diff[2];
    float info;     // MapPointRefinementConfidence(1) (:773)
    uint32_t steps;
    float huber, max_error_sq;
};

inline Consts make_consts(const mage_mono_init_settings& s)
{
    Consts c{};
    c.radius = s.extra_frame_search_radius;
    c.min_pct = s.min_third_frame_match_percentage;
    c.max_dist[0] = s.extra_frame_max_hamming_distance;
    c.min_diff[0] = s.extra_frame_min_hamming_difference;
    c.max_dist[1] = s.five_point_max_hamming_distance;
    c.min_diff[1] = s.five_point_min_hamming_difference;
    c.info = track::refinement_confidence(1);
    c.steps = s.extra_frame_bundle_adjustment_steps;
    c.huber = s.extra_frame_huber_width;
    c.max_error_sq = s.extra_frame_max_outlier_error * s.extra_frame_max_outlier_error;
    return c;
}

// Eigen's Quaternion(Matrix3f) followed by normalize() (Utils/cv.h ToQuat): m row-major, q = x, y, z, w.
NP_HD void quat_from_rotation(const float* m, float* q)
{
    const float tr = (m[0] + m[4]) + m[8];
    if (tr > 0.f) {
        float t = sqrtf(tr + 1.0f);
        q[3] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        float t = sqrtf(((m[i * 4] - m[j * 4]) - m[k * 4]) + 1.0f);
        q[i] = 0.5f * t;
        t = 0.5f / t;
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
    const float n = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int a = 0; a < 4; a++) q[a] = q[a] / n;
}

// The midpoint pose (:711-714) from the two frames' poses in the bundler form (view-space t,
// column-major R): the world position is the mean of the two camera centres C = -(R^T t), the world
// rotation the slerp at 1/2 of the two world rotations R^T.  Eigen's slerp weighs both ends equally
// at t = 1/2 (sin(theta / 2) / sin(theta) each, the second negated when the dot product is negative),
// so the result is normalize(q0 +- q1): the closed form used here, whose last bits against Eigen's
// acos / sin form are unpinned.  Pose(To4x4(ToMat(q), C)) keeps that world matrix and
// inverts it by Utils/cv.h Invert: the transposed rotation, and t = R^T (-C) summed as cv::Matx's
// product sums it.  Output in the bundler form again.
NP_HD void midpoint_pose(const float* pos3, const float* r9, float* mpos3, float* mr9)
{
    float q[2][4], C[2][3];
    for (int f = 0; f < 2; f++) {
        const float* r = r9 + 9 * f;  // column-major R = row-major R^T, the world rotation
        const float* t = pos3 + 3 * f;
        for (int i = 0; i < 3; i++) C[f][i] = -newpoints::dot3(&r[i * 3], t);
        quat_from_rotation(r, q[f]);
    }
    const float d = ((q[0][0] * q[1][0] + q[0][1] * q[1][1]) + q[0][2] * q[1][2]) + q[0][3] * q[1][3];
    float h[4];
    for (int a = 0; a < 4; a++) h[a] = d < 0.f ? q[0][a] - q[1][a] : q[0][a] + q[1][a];
    const float n = sqrtf(((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]) + h[3] * h[3]);
    for (int a = 0; a < 4; a++) h[a] = h[a] / n;
    // Eigen's toRotationMatrix: the world rotation W, row-major
    const float tx = 2.f * h[0], ty = 2.f * h[1], tz = 2.f * h[2];
    const float twx = tx * h[3], twy = ty * h[3], twz = tz * h[3];
    const float txx = tx * h[0], txy = ty * h[0], txz = tz * h[0];
    const float tyy = ty * h[1], tyz = tz * h[1], tzz = tz * h[2];
    const float W[9] = {1.f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.f - (txx + tzz),
                        tyz - twx,         txz - twy, tyz + twx, 1.f - (txx + tyy)};
    float c[3];
    for (int i = 0; i < 3; i++) c[i] = (C[0][i] + C[1][i]) / 2.f;
    // view rotation R = W^T: column-major R is row-major W
    for (int i = 0; i < 9; i++) mr9[i] = W[i];
    for (int i = 0; i < 3; i++)
        mpos3[i] = (((0.f + W[i] * -c[0]) + W[3 + i] * -c[1]) + W[6 + i] * -c[2]) + 0.f * 1.f;
}

// ProjectUndistorted (Reprojection.cpp:26-42) through the pose in the bundler form: returns the
// depth.  A depth of exactly zero divides by 1 (:32).
NP_HD float project(const float* pos3, const float* r9, const float* intr4, const float* X, float& x, float& y)
{
    float cs[3];
    for (int r = 0; r < 3; r++) cs[r] = (((0.f + r9[r] * X[0]) + r9[3 + r] * X[1]) + r9[6 + r] * X[2]) + pos3[r] * 1.f;
    const float depth = cs[2], div = depth != 0 ? depth : 1.f;
    x = (cs[0] / div) * intr4[2] + intr4[0];
    y = (cs[1] / div) * intr4[3] + intr4[1];
    return depth;
}

// :766-798 — which query's match takes the keypoint: 1 only when both matched and frame 1's
// distance is strictly smaller, or when frame 1's alone matched; -1 when neither did.
NP_HD int choose(bool ok0, int best0, bool ok1, int best1)
{
    if (ok0 && ok1) return best1 < best0 ? 1 : 0;
    return ok1 ? 1 : (ok0 ? 0 : -1);
}

// The gates of :803 and :835: the frame gives up.  No map points at all give up as well (the
// reference never arrives with fewer than MinInitialMapPoints, :690).
NP_HD bool gate_fails(uint32_t associated, uint32_t n_points, float min_pct)
{
    return n_points == 0 || (float)associated / (float)n_points < min_pct;
}

// The device chain's scratch for `problems` problems of up to `cap` points, offsets in bytes.
struct Layout {
    size_t obs_start;  // problems + 1 words: the prefix of ba_count
    size_t ba_count;   // per problem: observations handed to the pose BA (the matches, 0 after a failed first gate)
    size_t ba_pos3, ba_r9;  // per problem: the midpoint pose, the BA's start
    size_t matched;    // problems x cap words: the matched points' indices in point order
    size_t ba_points, ba_uv, ba_info;  // the BA's observations, prefix-packed over the problems
    size_t outlier;    // its flags, packed the same way
    size_t opt_pos3, opt_r9, mean_sq, opt_qt7;  // its outputs per problem (qt7: the fp64 state, 7 doubles)
    size_t bytes;
};
inline Layout layout(uint64_t problems, uint64_t cap)
{
    const uint64_t P = problems, E = problems * cap;
    Layout l;
    size_t o = 0;
    auto take = [&o](uint64_t n) {
        const size_t at = o;
        o = (size_t)((o + n + 255) & ~(uint64_t)255);
        return at;
    };
    l.obs_start = take(4 * (P + 1));
    l.ba_count = take(4 * P);
    l.ba_pos3 = take(12 * P);
    l.ba_r9 = take(36 * P);
    l.matched = take(4 * E);
    l.ba_points = take(12 * E);
    l.ba_uv = take(8 * E);
    l.ba_info = take(4 * E);
    l.outlier = take(E);
    l.opt_pos3 = take(12 * P);
    l.opt_r9 = take(36 * P);
    l.mean_sq = take(4 * P);
    l.opt_qt7 = take(56 * P);
    l.bytes = o;
    return l;
}

}  // namespace monothird
}  // namespace mage
