// reloc_guided.cpp — the plain C++ twin of reloc_guided.hip: the rest of
// PoseEstimator::TryEstimatePoseFromCandidates behind PNPRansac (Tracking/PoseEstimator.cpp:346-436)
// for one problem, in three phases over the arithmetic of reloc_guided_math.hpp.  The library has
// neither a host pose bundle adjustment nor a host RadiusMatch: their outcomes are inputs.  Same
// records, arrays and bytes as the kernels.
//
// This file includes no HIP header, so that it also builds as plain host C++ on its own
// (tests/cpp/reloc_guided_host_check.cpp): set_error and the argument check are declared here as
// common.hpp declares them.
#include <algorithm>
#include <cstring>
#include <string>

#include "reloc_guided_math.hpp"

namespace mage {
void set_error(const std::string& msg);
}

#define MAGE_REQUIRE(cond, code, msg) \
    do {                              \
        if (!(cond)) {                \
            ::mage::set_error(msg);   \
            return (code);            \
        }                             \
    } while (0)

extern "C" mage_status mage_reloc_guided_host(const mage_reloc_settings* settings, int32_t pnp_ok, const float* intr4,
                                              const float* map_xyzi, const mage_keypoint* kf_kp, const uint8_t* kf_desc,
                                              uint32_t n_kf, const int32_t* order, uint32_t n_order,
                                              const mage_keypoint* kp, uint32_t n_kp, const float* pos3_first,
                                              const float* r9_first, uint32_t cap, mage_reloc_guided_result* result,
                                              mage_keypoint* query_kp, float* query_pos, uint8_t* query_desc,
                                              int32_t* query_ref, const mage_dmatch* radius_matches,
                                              uint32_t n_radius_matches, int32_t* assoc, float* ba_points3, float* ba_uv,
                                              float* ba_info, const uint8_t* outlier, const float* pos3_second,
                                              const float* r9_second)
{
    using namespace mage;
    using namespace mage::relocguided;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(intr4 && result && pos3_first && r9_first, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE((n_kf == 0 || (map_xyzi && kf_kp && kf_desc)) && (n_kp == 0 || kp) && (!order || n_order == 0 || map_xyzi) &&
                     (cap == 0 || (query_kp && query_pos && query_desc && query_ref)),
                 MAGE_EINVAL, "null argument");
    MAGE_REQUIRE(!radius_matches || cap == 0 || (assoc && ba_points3 && ba_uv && ba_info), MAGE_EINVAL, "null argument");
    MAGE_REQUIRE(!outlier || (radius_matches && pos3_second && r9_second), MAGE_EINVAL, "null argument");
    const Consts c = make_consts(*settings);
    mage_reloc_guided_result R;
    init_result(R);
    R.verdict = RG_SKIPPED;
    // phase 1: the checks, the query set
    if (over_limit(n_kf, RG_MAX_KEYPOINTS, n_kp, RG_MAX_KEYPOINTS, order != nullptr, n_order)) {  // no pitches here
        R.status = RG_STATUS_OVER_LIMIT;
        *result = R;
        return MAGE_OK;
    }
    if (!pnp_ok || n_kp < c.min_frame_kp) {
        *result = R;
        return MAGE_OK;
    }
    const uint32_t slots = order ? n_order : n_kf;
    if (order)
        for (uint32_t s = 0; s < slots; s++)
            if (bad_order_entry(order[s], n_kf, map_xyzi)) R.status = RG_STATUS_BAD_ORDER;
    if (R.status != 0) {
        *result = R;
        return MAGE_OK;
    }
    for (int k = 0; k < 3; k++) R.pos3_first[k] = pos3_first[k];
    for (int k = 0; k < 9; k++) R.r9_first[k] = r9_first[k];
    uint32_t nq = 0;
    for (uint32_t s = 0; s < slots; s++) {
        const int32_t k = slot_keypoint(order, map_xyzi, s);
        if (k < 0) continue;
        R.n_assoc++;
        float x, y;
        if (!predict(pos3_first, r9_first, intr4, map_xyzi + 4ll * k, x, y)) continue;
        if (nq < cap) {
            query_kp[nq] = kf_kp[k];
            query_pos[2 * nq] = x;
            query_pos[2 * nq + 1] = y;
            std::memcpy(query_desc + 32ull * nq, kf_desc + 32ull * k, 32);
            query_ref[nq] = k;
        }
        nq++;
    }
    R.n_queries = std::min(nq, cap);
    if (nq > cap) R.status |= RG_STATUS_OVER_CAP;
    R.verdict = RG_OK;
    if (!radius_matches) {
        *result = R;
        return MAGE_OK;
    }
    // phase 2: the gates, the associations, the second bundle adjustment's inputs
    MAGE_REQUIRE(n_radius_matches <= R.n_queries, MAGE_EINVAL, "more radius matches than queries");
    for (uint32_t m = 0; m < n_radius_matches; m++)
        MAGE_REQUIRE(radius_matches[m].query_idx >= 0 && (uint32_t)radius_matches[m].query_idx < R.n_queries &&
                         radius_matches[m].train_idx >= 0 && (uint32_t)radius_matches[m].train_idx < n_kp,
                     MAGE_EINVAL, "a radius match names no query or no keypoint");
    R.n_radius_matches = n_radius_matches;
    if (n_radius_matches < c.min_radius) {
        R.verdict = RG_FEW_RADIUS;
        *result = R;
        return MAGE_OK;
    }
    const relocpnp::BehindFilter bf = relocpnp::behind_filter(pos3_first, r9_first);
    uint32_t n = 0;
    for (uint32_t m = 0; m < n_radius_matches; m++) {
        const int32_t k = query_ref[radius_matches[m].query_idx], t = radius_matches[m].train_idx;
        const float* X = map_xyzi + 4ll * k;
        if (point_behind(bf, X)) continue;
        assoc[2 * n] = k;
        assoc[2 * n + 1] = t;
        n++;
    }
    R.n_in_front = n;
    if (n < c.min_points) {
        R.verdict = RG_FEW_POINTS;
        *result = R;
        return MAGE_OK;
    }
    for (uint32_t i = 0; i < n; i++) {
        const float* X = map_xyzi + 4ll * assoc[2 * i];
        const mage_keypoint& f = kp[assoc[2 * i + 1]];
        ba_points3[3 * i] = X[0];
        ba_points3[3 * i + 1] = X[1];
        ba_points3[3 * i + 2] = X[2];
        ba_uv[2 * i] = f.x;
        ba_uv[2 * i + 1] = f.y;
        ba_info[i] = X[3];
    }
    if (!outlier) {
        *result = R;
        return MAGE_OK;
    }
    // phase 3: the outlier share, the final record
    for (uint32_t i = 0; i < n; i++) R.n_outliers += outlier[i] ? 1u : 0u;
    for (int k = 0; k < 3; k++) R.pos3[k] = pos3_second[k];
    for (int k = 0; k < 9; k++) R.r9[k] = r9_second[k];
    if (ba_gate_fails(n, R.n_outliers, c.min_ba_pct)) R.verdict = RG_FEW_BA_INLIERS;
    *result = R;
    return MAGE_OK;
}

extern "C" mage_status mage_reloc_guided_choose_host(const mage_reloc_settings* settings,
                                                     const mage_reloc_guided_result* results, uint32_t n_candidates,
                                                     mage_reloc_frame_result* frame)
{
    using namespace mage::relocguided;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(frame && (n_candidates == 0 || results), MAGE_EINVAL, "null argument");
    mage_reloc_frame_result F;
    init_frame(F);
    if (settings->round_robin_iterations >= 1)
        for (uint32_t c = 0; c < n_candidates; c++)
            if (succeeded(results[c])) {
                take_candidate(F, c, results[c]);
                break;
            }
    *frame = F;
    return MAGE_OK;
}
