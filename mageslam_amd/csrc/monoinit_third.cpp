// monoinit_third.cpp — the plain C++ twin of monoinit_third.hip: the third frame of
// TryIntializeMapWithProvidedFrames (Tracking/MapInitialization.cpp:695-840) as the reference's
// sequential loop, literally — per map point the projection, two single-query RadiusMatch calls
// (FeatureMatcher.cpp:386-446) against one mask, the choice of :766-798 — then the first gate, and,
// given the pose bundle adjustment's outlier flags, the cull, the second gate and the compaction,
// over the arithmetic of monoinit_third_math.hpp.  The CPU backend.
//
// This file includes no HIP header, so that it also builds as plain host C++ on its own
// (tests/cpp/mono_third_host_check.cpp); set_error and MAGE_REQUIRE come from require.hpp, which the
// build holds equal to common.hpp's (monoinit_third.hip).
#include <cstring>
#include <string>
#include <vector>

#include "monoinit_third_math.hpp"
#include "require.hpp"

namespace mage {
namespace monothird {
namespace {

int hamming256(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int w = 0; w < 4; w++) {
        uint64_t x, y;
        std::memcpy(&x, a + 8 * w, 8);
        std::memcpy(&y, b + 8 * w, 8);
        d += __builtin_popcountll(x ^ y);
    }
    return d;
}

// The single-query RadiusMatch at octave 0 (FeatureMatcher.cpp:386-446), candidates in ascending
// keypoint index: the keypoint, or -1; *best_out the best distance seen within max_dist, or -1.
int radius_match_one(float radius, int max_dist, int min_diff, float qx, float qy, const uint8_t* qd,
                     const mage_keypoint* kp, const uint8_t* desc, uint32_t n, const uint8_t* mask, int* best_out)
{
    int best = max_dist + 1, second = 0x7FFFFFFF, train = -1;
    for (uint32_t t = 0; t < n; t++) {
        if (!(kp[t].x >= qx - radius && kp[t].x <= qx + radius && kp[t].y >= qy - radius && kp[t].y <= qy + radius) ||
            kp[t].octave != 0 || !mask[t])
            continue;
        const int d = hamming256(qd, desc + 32ull * t);
        if (d < best) {
            train = (int)t;
            second = best;
            best = d;
        }
    }
    *best_out = train >= 0 ? best : -1;
    return train >= 0 && second - best > min_diff ? train : -1;
}

}  // namespace
}  // namespace monothird
}  // namespace mage

extern "C" mage_status mage_mono_init_third_frame_host(
    const mage_mono_init_settings* settings, const float* intr4, const float* pos3, const float* r9, const float* points,
    uint32_t n_points, const int32_t* idx0, const int32_t* idx1, const uint8_t* desc0, uint32_t n0, const uint8_t* desc1,
    uint32_t n1, const mage_keypoint* kp2, const uint8_t* desc2, uint32_t n2, uint32_t cam_index, const uint8_t* outlier,
    const float* opt_pos3, const float* opt_r9, float mean_sq, mage_mono_init_third_result* result, int32_t* keypoint,
    uint8_t* verdict, int32_t* dist, float* proj, uint8_t* mask, float* obs_uv, uint32_t* obs_pt, uint32_t* obs_cam,
    float* obs_info, float* ba_points, float* ba_uv, float* ba_info)
{
    using namespace mage;
    using namespace mage::monothird;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(intr4 && pos3 && r9 && result, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE(n_points == 0 || (points && idx0 && idx1 && keypoint && verdict && dist && proj && obs_uv && obs_pt &&
                                   obs_cam && obs_info),
                 MAGE_EINVAL, "null argument");
    MAGE_REQUIRE((n0 == 0 || desc0) && (n1 == 0 || desc1) && (n2 == 0 || (kp2 && desc2 && mask)), MAGE_EINVAL,
                 "null argument");
    MAGE_REQUIRE(!outlier || (opt_pos3 && opt_r9), MAGE_EINVAL, "the outlier flags come with the optimised pose");
    const Consts c = make_consts(*settings);
    mage_mono_init_third_result R{};
    R.n_points = n_points;
    if (n_points > (uint32_t)M3_MAX_POINTS || n2 > (uint32_t)M3_MAX_KP)
        R.status = M3_STATUS_OVER_LIMIT;
    else
        for (uint32_t i = 0; i < n_points; i++)
            if (idx0[i] < 0 || (uint32_t)idx0[i] >= n0 || idx1[i] < 0 || (uint32_t)idx1[i] >= n1)
                R.status = M3_STATUS_BAD_INDEX;
    if (R.status != 0) {
        *result = R;
        return MAGE_OK;
    }
    midpoint_pose(pos3, r9, R.pos3, R.r9);
    for (uint32_t t = 0; t < n2; t++) mask[t] = 1;
    // :723-799
    std::vector<uint32_t> matched;
    for (uint32_t i = 0; i < n_points; i++) {
        float x, y;
        keypoint[i] = -1;
        dist[2 * i] = dist[2 * i + 1] = -1;
        const float depth = project(R.pos3, R.r9, intr4, points + 3ull * i, x, y);
        proj[2 * i] = x;
        proj[2 * i + 1] = y;
        if (depth < 0) {
            verdict[i] = M3_PT_BEHIND;
            R.n_behind++;
            continue;
        }
        int best[2];
        const int t0 = radius_match_one(c.radius, c.max_dist[0], c.min_diff[0], x, y, desc0 + 32ull * idx0[i], kp2, desc2, n2,
                                        mask, &best[0]);
        const int t1 = radius_match_one(c.radius, c.max_dist[1], c.min_diff[1], x, y, desc1 + 32ull * idx1[i], kp2, desc2, n2,
                                        mask, &best[1]);
        dist[2 * i] = best[0];
        dist[2 * i + 1] = best[1];
        const int which = choose(t0 >= 0, best[0], t1 >= 0, best[1]);
        verdict[i] = which < 0 ? M3_PT_NO_MATCH : (which ? M3_PT_FRAME1 : M3_PT_FRAME0);
        if (which < 0) continue;
        keypoint[i] = which ? t1 : t0;
        mask[keypoint[i]] = 0;
        matched.push_back(i);
    }
    R.n_matched = R.n_associated = (uint32_t)matched.size();
    const bool gate1 = gate_fails(R.n_matched, n_points, c.min_pct);  // :803
    R.verdict = gate1 ? M3_FEW_MATCHES : M3_OK;
    for (size_t j = 0; j < matched.size(); j++) {
        const uint32_t i = matched[j];
        if (ba_points) std::memcpy(ba_points + 3 * j, points + 3ull * i, 12);
        if (ba_uv) {
            ba_uv[2 * j] = kp2[keypoint[i]].x;
            ba_uv[2 * j + 1] = kp2[keypoint[i]].y;
        }
        if (ba_info) ba_info[j] = c.info;
    }
    if (!outlier && !gate1) {  // the bundle adjustment is the caller's
        *result = R;
        return MAGE_OK;
    }
    if (!gate1) {
        // :829-838
        for (size_t j = 0; j < matched.size(); j++)
            if (outlier[j]) {
                keypoint[matched[j]] = -1;
                verdict[matched[j]] = M3_PT_CULLED;
                R.n_outliers++;
            }
        R.n_associated = R.n_matched - R.n_outliers;
        std::memcpy(R.opt_pos3, opt_pos3, 12);
        std::memcpy(R.opt_r9, opt_r9, 36);
        R.mean_sq = mean_sq;
        if (gate_fails(R.n_associated, n_points, c.min_pct)) R.verdict = M3_FEW_AFTER_CULL;
    }
    uint32_t o = 0;
    for (uint32_t i = 0; i < n_points; i++) {
        if (keypoint[i] < 0) continue;
        obs_uv[2 * o] = kp2[keypoint[i]].x;
        obs_uv[2 * o + 1] = kp2[keypoint[i]].y;
        obs_pt[o] = i;
        obs_cam[o] = cam_index;
        obs_info[o] = c.info;
        o++;
    }
    *result = R;
    return MAGE_OK;
}
