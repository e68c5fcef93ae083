// reloc_guided_math.hpp — the rest of PoseEstimator::TryEstimatePoseFromCandidates behind PNPRansac
// (Tracking/PoseEstimator.cpp:346-436): the guided query set (:351-371, ProjectUndistorted of
// Reprojection.cpp:26-42), the gates of :391, :406 and :422, RemoveMapPointsThatAreBehind (:405) and
// the choice of the candidate.  Shared by the kernels (reloc_guided.hip) and their plain C++ twin
// (reloc_guided.cpp).  Float arithmetic in one written order, both built with -ffp-contract=off.
#pragma once

#include "reloc_pnp_math.hpp"

namespace mage {
namespace relocguided {

constexpr int RG_MAX_KEYPOINTS = 4096;  // a side's keypoints (the matchers' limit), so the queries too

enum : uint32_t {
    RG_OK = MAGE_RG_OK,
    RG_SKIPPED = MAGE_RG_SKIPPED,
    RG_FEW_RADIUS = MAGE_RG_FEW_RADIUS_MATCHES,
    RG_FEW_POINTS = MAGE_RG_FEW_MAP_POINTS,
    RG_FEW_BA_INLIERS = MAGE_RG_FEW_BA_INLIERS,
};
enum : uint32_t {
    RG_STATUS_OVER_LIMIT = MAGE_RG_STATUS_OVER_LIMIT,
    RG_STATUS_OVER_CAP = MAGE_RG_STATUS_OVER_CAP,
    RG_STATUS_BAD_ORDER = MAGE_RG_STATUS_BAD_ORDER,
};

constexpr float RG_HUBER = 1.8f;  // BundleAdjustSettings' default HuberWidth

// nullptr when the settings can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_settings(const mage_reloc_settings* s)
{
    if (const char* why = relocpnp::check_settings(s)) return why;
    if (!(s->bundle_adjust_inliers_pct_required >= 0.f)) return "bundle_adjust_inliers_pct_required must be >= 0";
    if (!(s->search_radius >= 0.f) || !(s->search_radius <= FLT_MAX)) return "search_radius must be finite and >= 0";
    if (!(s->max_bundle_adjust_reprojection_error >= 0.f) || !(s->max_bundle_adjust_reprojection_error <= FLT_MAX))
        return "max_bundle_adjust_reprojection_error must be finite and >= 0";
    return nullptr;
}

struct Consts {
    uint32_t min_frame_kp;  // MinBruteForceCorrespondences (:233)
    uint32_t min_radius;    // MinRadiusMatchCorrespondences
    uint32_t min_points;    // MinMapPoints
    float min_ba_pct;       // BundleAdjustInliersPctRequired
    uint32_t rounds;        // RoundRobinIterations
};
inline Consts make_consts(const mage_reloc_settings& s)
{
    return Consts{s.min_brute_force_correspondences, s.min_radius_match_correspondences, s.min_map_points,
                  s.bundle_adjust_inliers_pct_required, s.round_robin_iterations};
}

NP_HD void init_result(mage_reloc_guided_result& r)
{
    r = mage_reloc_guided_result{};
    r.r9_first[0] = r.r9_first[4] = r.r9_first[8] = 1.f;
    r.r9[0] = r.r9[4] = r.r9[8] = 1.f;
}

NP_HD void init_frame(mage_reloc_frame_result& f)
{
    f = mage_reloc_frame_result{};
    f.index = -1;
    f.r9[0] = f.r9[4] = f.r9[8] = 1.f;
}

// The counts alone: a side over the matchers' limit or a count over its pitch.
NP_HD bool over_limit(uint32_t n_kf, long long kf_pitch, uint32_t n_kp, long long kp_pitch, bool ordered, uint32_t n_order)
{
    return n_kf > (uint32_t)RG_MAX_KEYPOINTS || (long long)n_kf > kf_pitch || n_kp > (uint32_t)RG_MAX_KEYPOINTS ||
           (long long)n_kp > kp_pitch || (ordered && (n_order > (uint32_t)RG_MAX_KEYPOINTS || (long long)n_order > kf_pitch));
}

// An order entry that names no association of the candidate.
NP_HD bool bad_order_entry(int32_t k, uint32_t n_kf, const float* map_xyzi)
{
    return k < 0 || (uint32_t)k >= n_kf || !(map_xyzi[4ll * k + 3] > 0.f);
}

// Slot s of the iteration (:360): the candidate keypoint it visits, or -1 when the slot holds no
// association (no order list: the keypoints in ascending index, those without a map point passed over).
NP_HD int32_t slot_keypoint(const int32_t* order, const float* map_xyzi, uint32_t s)
{
    if (order) return order[s];
    return map_xyzi[4ll * s + 3] > 0.f ? (int32_t)s : -1;
}

// :362-363, ProjectUndistorted (Reprojection.cpp:26-42) through the pose in the bundler form, each
// row summed as cv::Matx's product sums it: the predicted position; true when Distance >= 0.  A depth
// of exactly zero stays and divides by 1 (:32).  Written out row by row: no array indexed at run time.
NP_HD bool predict(const float* pos3, const float* r9, const float* intr4, const float* X, float& x, float& y)
{
    const float c0 = (((0.f + r9[0] * X[0]) + r9[3] * X[1]) + r9[6] * X[2]) + pos3[0] * 1.f;
    const float c1 = (((0.f + r9[1] * X[0]) + r9[4] * X[1]) + r9[7] * X[2]) + pos3[1] * 1.f;
    const float depth = (((0.f + r9[2] * X[0]) + r9[5] * X[1]) + r9[8] * X[2]) + pos3[2] * 1.f;
    const float div = depth != 0 ? depth : 1.f;
    x = (c0 / div) * intr4[2] + intr4[0];
    y = (c1 / div) * intr4[3] + intr4[1];
    return depth >= 0;
}

// RemoveMapPointsThatAreBehind's rule (:213) on a map point.
NP_HD bool point_behind(const relocpnp::BehindFilter& f, const float* X)
{
    const relocpnp::Corr c{X[0], X[1], X[2], 0.f, 0.f, 0.f, 0, 0};
    return relocpnp::is_behind(f, c);
}

// The gate of :421-422 in float as written: baInlierCount / (float)n < BundleAdjustInliersPctRequired.
NP_HD bool ba_gate_fails(uint32_t n, uint32_t outliers, float min_pct) { return (float)(n - outliers) / (float)n < min_pct; }

// A problem whose pass succeeded (:428-432).
NP_HD bool succeeded(const mage_reloc_guided_result& r)
{
    return r.verdict == RG_OK && (r.status & (RG_STATUS_OVER_LIMIT | RG_STATUS_BAD_ORDER)) == 0;
}

// The frame's record from candidate c's record, when it is the first that succeeded.
NP_HD void take_candidate(mage_reloc_frame_result& f, uint32_t c, const mage_reloc_guided_result& r)
{
    f.index = (int32_t)c;
    f.n_assoc = r.n_in_front;
    for (int k = 0; k < 3; k++) f.pos3[k] = r.pos3[k];
    for (int k = 0; k < 9; k++) f.r9[k] = r.r9[k];
}

}  // namespace relocguided
}  // namespace mage
