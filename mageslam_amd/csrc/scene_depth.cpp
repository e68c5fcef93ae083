// scene_depth.cpp — the plain C++ twin of scene_depth.hip: CalculateBoundingPlaneDepthsForKeyframe
// (Tracking/BoundingPlaneDepths.cpp:16-87) for one frame over the arithmetic of scene_math.hpp, the
// two order statistics by std::nth_element as the reference takes them.  Same records and bytes as
// the kernel.
//
// This file includes no HIP header, so that it also builds as plain host C++ on its own
// (tests/cpp/scene_host_check.cpp): set_error and the argument check are declared here as common.hpp
// declares them.
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "scene_math.hpp"

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

extern "C" mage_status mage_bounding_plane_depths_host(const mage_bounding_depth_settings* settings, const float* pos3,
                                                       const float* r9, const float* intr4, uint32_t width,
                                                       uint32_t height, const mage_keypoint* kp, uint32_t n_kp,
                                                       const float* map_xyzi, const int32_t* kp_index, uint32_t n_points,
                                                       uint32_t cap, mage_depth_result* result,
                                                       mage_projected_point* sparse)
{
    using namespace mage::scene;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(pos3 && r9 && intr4 && result, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE((n_kp == 0 || kp) && (n_points == 0 || (map_xyzi && kp_index)) && (cap == 0 || sparse), MAGE_EINVAL,
                 "null argument");
    if (over_limit(n_points, cap)) {
        *result = over_limit_result(n_points);
        return MAGE_OK;
    }
    const Camera cam = make_camera(*settings, pos3, r9, width, height);
    std::vector<uint32_t> keys;  // validDepths (:30), as their order-preserving keys
    keys.reserve(n_points);
    uint32_t status = 0;
    for (uint32_t i = 0; i < n_points; i++) {
        const float* p = map_xyzi + 4ull * i;
        const int32_t k = kp_index[i];
        if (k < 0 || (uint32_t)k >= n_kp) {
            status |= BD_STATUS_BAD_INDEX;
        } else if (in_region(cam, kp[k].x, kp[k].y)) {
            const float depth = depth_of(cam, p);
            if (!(depth > 0.f)) status |= BD_STATUS_NONPOSITIVE;
            uint32_t u;
            std::memcpy(&u, &depth, 4);
            keys.push_back(key_of_bits(u));
        }
        int32_t id;
        std::memcpy(&id, p + 3, 4);
        sparse[i] = sparse_of(pos3, r9, intr4, p, id);
    }
    const uint32_t nv = (uint32_t)keys.size();
    float sel[2] = {0.f, 0.f};
    if (nv) {
        const uint32_t rn = soft_rank(settings->near_depth_softness, nv), rf = soft_rank(settings->far_depth_softness, nv);
        std::nth_element(keys.begin(), keys.begin() + rn, keys.end());
        uint32_t u = bits_of_key(keys[rn]);
        std::memcpy(&sel[0], &u, 4);
        std::nth_element(keys.begin(), keys.begin() + rf, keys.end(), std::greater<uint32_t>{});
        u = bits_of_key(keys[rf]);
        std::memcpy(&sel[1], &u, 4);
    }
    *result = make_result(nv, n_points, status, sel[0], sel[1]);
    return MAGE_OK;
}
