// scene_voi.cpp — the plain C++ twin of scene_voi.hip: CalculateVolumeOfInterest
// (VolumeOfInterest/VolumeOfInterest.cpp:45-259) for one problem as the reference's sequential loops
// over the arithmetic of scene_math.hpp.  Same records, trace and bytes as the kernels.
//
// This file includes no HIP header, so that it also builds as plain host C++ on its own
// (tests/cpp/scene_host_check.cpp): set_error and the argument check are declared here as common.hpp
// declares them.
#include <cstring>
#include <string>
#include <vector>

#include "scene_math.hpp"

namespace mage {
void set_error(const std::string& msg);
}

#ifndef MAGE_REQUIRE
#define MAGE_REQUIRE(cond, code, msg) \
    do {                              \
        if (!(cond)) {                \
            ::mage::set_error(msg);   \
            return (code);            \
        }                             \
    } while (0)
#endif

extern "C" mage_status mage_voi_settings_prepare(mage_voi_settings* settings)
{
    const char* why = mage::scene::check_voi_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    mage::scene::voi_prepare(*settings);
    return MAGE_OK;
}

extern "C" mage_status mage_voi_teardrop_host(const mage_voi_settings* settings, const float* kf_world, const float* near_far,
                                              uint32_t n_kf, const float* points, uint32_t n_points, float* scores)
{
    using namespace mage::scene;
    const char* why = check_voi_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE((n_kf == 0 || (kf_world && near_far)) && (n_points == 0 || points) && (n_kf == 0 || n_points == 0 || scores),
                 MAGE_EINVAL, "null argument");
    mage_voi_settings s = *settings;
    voi_prepare(s);
    std::vector<VoiKf> kf(n_kf);
    float corners[8][3];
    for (uint32_t k = 0; k < n_kf; k++) voi_keyframe(s, kf_world + 12ull * k, near_far[2 * k], near_far[2 * k + 1], kf[k], corners);
    for (uint32_t p = 0; p < n_points; p++)
        for (uint32_t k = 0; k < n_kf; k++) scores[(size_t)p * n_kf + k] = voi_teardrop(s, kf[k], points + 3ull * p);
    return MAGE_OK;
}

extern "C" mage_status mage_volume_of_interest_host(const mage_voi_settings* settings, const float* kf_world,
                                                    const float* near_far, const mage_depth_result* depth_records,
                                                    uint32_t n_depth_records, const uint32_t* depth_index, uint32_t n_kf,
                                                    mage_voi_result* result, mage_voi_level* trace)
{
    using namespace mage::scene;
    const char* why = check_voi_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(result && (n_kf == 0 || (kf_world && (near_far || (depth_index && (depth_records || n_depth_records == 0))))),
                 MAGE_EINVAL, "null argument");
    if (n_kf == 0) {  // :91-94, the bounds untouched
        result->status = VOI_NO_KEYFRAMES;
        result->levels_done = 0;
        return MAGE_OK;
    }
    mage_voi_settings s = *settings;
    voi_prepare(s);
    const int levels = s.iterations;
    if (trace && levels) std::memset(trace, 0, sizeof(mage_voi_level) * (size_t)levels);
    // :99-136 — the keyframes and the box of their frusta
    std::vector<VoiKf> kf(n_kf);
    float bmin[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, bmax[3] = {FLT_MIN, FLT_MIN, FLT_MIN};
    for (uint32_t k = 0; k < n_kf; k++) {
        float nd, fd, corners[8][3];
        voi_depths(near_far, depth_records, n_depth_records, depth_index, k, nd, fd);
        voi_keyframe(s, kf_world + 12ull * k, nd, fd, kf[k], corners);
        for (int c = 0; c < 8; c++)
            for (int i = 0; i < 3; i++) {
                bmin[i] = min_total(bmin[i], corners[c][i]);
                bmax[i] = max_total(bmax[i], corners[c][i]);
            }
    }
    // :138-157 — every centroid's score, the seeds of the voxel minimum and maximum
    float vmin = FLT_MAX, vmax = FLT_MIN;
    std::vector<float> kf_score(n_kf);
    for (uint32_t a = 0; a < n_kf; a++) {
        float v = 0.f;
        for (uint32_t b = 0; b < n_kf; b++) v += voi_teardrop(s, kf[b], kf[a].centroid);
        kf_score[a] = v;
        vmin = min_total(v, vmin);
        vmax = max_total(v, vmax);
    }
    mage_voi_result R;
    for (int i = 0; i < 3; i++) {
        R.min[i] = bmin[i];
        R.max[i] = bmax[i];
    }
    R.status = VOI_OK;
    R.levels_done = 0;
    // :159-240
    for (int li = 0; li < levels; li++) {
        const int lod = levels - li;
        mage_voi_level L;
        std::memset(&L, 0, sizeof(L));
        const VoiGrid g = voi_grid(s, lod, R.min, R.max);
        if (!g.ok) {
            R.status = VOI_DEGENERATE;
            break;
        }
        L.side = g.side;
        for (int i = 0; i < 3; i++) L.dims[i] = g.dims[i];
        for (uint32_t v = 0; v < g.count; v++) {
            float p[3], value = 0.f;
            voi_voxel_point(g, v, p);
            for (uint32_t k = 0; k < n_kf; k++) value += voi_teardrop(s, kf[k], p);
            vmin = min_total(vmin, value);
            vmax = max_total(vmax, value);
        }
        L.voxel_min = vmin;
        L.voxel_max = vmax;
        if (!finite_f(vmin) || !finite_f(vmax)) {
            R.status = VOI_DEGENERATE;
            if (trace) trace[li] = L;
            break;
        }
        const float thr = voi_threshold(s, lod, vmin, vmax);
        L.threshold = thr;
        float nmin[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, nmax[3] = {FLT_MIN, FLT_MIN, FLT_MIN};
        for (uint32_t v = 0; v < g.count; v++) {
            float p[3], value = 0.f;
            voi_voxel_point(g, v, p);
            for (uint32_t k = 0; k < n_kf; k++) value += voi_teardrop(s, kf[k], p);
            if (value > thr) {
                L.n_voxels++;
                for (int i = 0; i < 3; i++) {
                    nmin[i] = min_total(nmin[i], p[i] - g.half);
                    nmax[i] = max_total(nmax[i], p[i] + g.half);
                }
            }
        }
        for (uint32_t k = 0; k < n_kf; k++)
            if (kf_score[k] > thr) {
                L.n_centroids++;
                for (int i = 0; i < 3; i++) {
                    nmin[i] = min_total(nmin[i], kf[k].centroid[i] - g.half);
                    nmax[i] = max_total(nmax[i], kf[k].centroid[i] + g.half);
                }
            }
        for (int i = 0; i < 3; i++) {
            L.box_min[i] = nmin[i];
            L.box_max[i] = nmax[i];
        }
        if (trace) trace[li] = L;
        if (L.n_voxels == 0 && L.n_centroids == 0) {
            R.status = VOI_EMPTY;
            break;
        }
        for (int i = 0; i < 3; i++) {
            R.min[i] = nmin[i];
            R.max[i] = nmax[i];
        }
        R.levels_done = (uint32_t)li + 1;
    }
    *result = R;
    return MAGE_OK;
}
