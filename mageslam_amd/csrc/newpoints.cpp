// newpoints.cpp — the plain C++ twin of newpoints.hip: CreateInitialAssociations' sequential loop
// (Core/MAGESLAM/Source/Mapping/NewMapPointsCreation.cpp:187-201, 290-321) over the per-match
// arithmetic of newpoints_math.hpp.  The CPU backend of mage_new_map_points, like track.cpp is the
// tracker's: same verdicts, same points, same bits.
#include <cstring>
#include <vector>

#include "common.hpp"
#include "newpoints_math.hpp"

extern "C" mage_status mage_new_map_points_host(const mage_new_points_settings* settings, const float* ki_pos3,
                                                const float* ki_r9, const float* ki_intr4, const mage_keypoint* ki_kp,
                                                uint32_t n_ki, const uint8_t* ki_associated, uint32_t n_kc,
                                                const float* kc_pos3, const float* kc_r9, const float* kc_intr4,
                                                const mage_keypoint* kc_kp, const uint32_t* kc_kp_start,
                                                const mage_dmatch* matches, const uint32_t* match_start,
                                                mage_new_point* out, uint32_t cap, uint32_t* n_out, uint8_t* verdict,
                                                uint32_t* status)
{
    using namespace mage;
    using namespace mage::newpoints;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(n_kc <= (uint32_t)NP_MAX_SLOTS, MAGE_EINVAL, "more than 8 Kc slots");
    MAGE_REQUIRE(n_out && status && ki_pos3 && ki_r9 && ki_intr4 && (n_ki == 0 || ki_kp), MAGE_EINVAL, "null argument");
    *n_out = 0;
    *status = 0;
    MAGE_REQUIRE(n_kc == 0 || (kc_pos3 && kc_r9 && kc_intr4 && kc_kp_start && match_start), MAGE_EINVAL, "null argument");
    for (uint32_t s = 0; s < n_kc; s++)
        MAGE_REQUIRE(kc_kp_start[s] <= kc_kp_start[s + 1] && match_start[s] <= match_start[s + 1], MAGE_EINVAL,
                     "start offsets must not decrease");
    const uint32_t n_matches = n_kc ? match_start[n_kc] - match_start[0] : 0;
    MAGE_REQUIRE((n_kc == 0 || kc_kp_start[n_kc] == kc_kp_start[0] || kc_kp) &&
                     (n_matches == 0 || (matches && verdict)) && (cap == 0 || out),
                 MAGE_EINVAL, "null argument");
    if (n_matches == 0) return MAGE_OK;
    if (n_ki > (uint32_t)NP_MAX_KI) {  // over a limit: no points, verdicts untouched
        *status = 1u;
        return MAGE_OK;
    }
    const Consts c = make_consts(*settings);
    Frame ki;
    make_frame(ki_pos3, ki_r9, ki_intr4, ki);
    std::vector<uint32_t> grid(c.grid_w * c.grid_h, 0u);
    if (ki_associated)
        for (uint32_t i = 0; i < n_ki; i++)
            if (ki_associated[i]) {
                const int cell = count_cell(c, ki_kp[i].x, ki_kp[i].y);
                if (cell >= 0) grid[cell]++;
            }
    std::vector<uint8_t> taken(n_ki, 0);  // KiAssociatedDescriptors
    uint32_t accepted = 0;
    for (uint32_t s = 0; s < n_kc; s++) {
        Frame kc;
        Pair pair;
        make_frame(kc_pos3 + 3 * s, kc_r9 + 9 * s, kc_intr4 + 4 * s, kc);
        make_pair(ki, kc, pair);
        const uint32_t nk = kc_kp_start[s + 1] - kc_kp_start[s];
        for (uint32_t mi = match_start[s]; mi < match_start[s + 1]; mi++) {
            const int q = matches[mi].query_idx, t = matches[mi].train_idx;
            if (q < 0 || (uint32_t)q >= nk || t < 0 || (uint32_t)t >= n_ki || ki_kp[t].octave < 0 ||
                ki_kp[t].octave >= NP_MAX_LEVELS) {
                verdict[mi] = NP_BAD_INDEX;
                continue;
            }
            const mage_keypoint& a = kc_kp[kc_kp_start[s] + q];
            const mage_keypoint& b = ki_kp[t];
            const int cell = test_cell(c, b.x, b.y);
            if (grid[cell] >= c.max_grid_count) {
                verdict[mi] = NP_GRID_FULL;
                continue;
            }
            if (taken[t]) {
                verdict[mi] = NP_KI_TAKEN;
                continue;
            }
            Geometry g{};
            const uint8_t v = match_geometry(c, ki, pair, a.x, a.y, a.octave, b.x, b.y, b.octave, g);
            verdict[mi] = v;
            if (v != NP_ACCEPTED) continue;
            taken[t] = 1;
            grid[cell]++;
            if (accepted < cap) {
                mage_new_point& o = out[accepted];
                for (int i = 0; i < 3; i++) {
                    o.position[i] = g.X[i];
                    o.mean_view_dir[i] = g.dir[i];
                }
                o.d_min = g.d_min;
                o.d_max = g.d_max;
                o.ki_index = (uint32_t)t;
                o.kc_slot = s;
                o.kc_index = (uint32_t)q;
                o.match_index = mi - match_start[s];
            }
            accepted++;
        }
    }
    *n_out = accepted < cap ? accepted : cap;
    if (accepted > cap) *status |= 2u;
    return MAGE_OK;
}

// ------------------------------------------------------------------------------------------
// LocallyAssociateNewAssociations (NewMapPointsCreation.cpp:337-424): the twin of
// newpoints_assoc.hip and the CPU backend of mage_new_points_associate.
// ------------------------------------------------------------------------------------------
extern "C" mage_status mage_new_points_associate_host(
    const mage_new_points_settings* settings, const mage_new_points_assoc_settings* assoc, const mage_new_point* points,
    uint32_t n_points, const uint8_t* ki_desc, uint32_t n_ki, uint32_t n_kf, const float* kf_pos3, const float* kf_r9,
    const float* kf_intr4, const mage_keypoint* kf_kp, const uint8_t* kf_desc, const uint32_t* kf_start,
    const int32_t* kf_slot, uint8_t* kf_mask, mage_new_point_assoc* out, uint8_t* verdict, uint32_t* status)
{
    using namespace mage;
    using namespace mage::newpoints;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    why = check_assoc_settings(assoc);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(status, MAGE_EINVAL, "null argument");
    *status = 0;
    if (n_points == 0 || n_kf == 0) return MAGE_OK;
    MAGE_REQUIRE(points && out && verdict && kf_pos3 && kf_r9 && kf_intr4 && kf_start && kf_slot && (n_ki == 0 || ki_desc),
                 MAGE_EINVAL, "null argument");
    for (uint32_t k = 0; k < n_kf; k++) {
        MAGE_REQUIRE(kf_start[k] <= kf_start[k + 1], MAGE_EINVAL, "start offsets must not decrease");
        MAGE_REQUIRE(kf_slot[k] >= -1 && kf_slot[k] < NP_MAX_SLOTS, MAGE_EINVAL, "kf_slot must be in [-1, 7]");
    }
    MAGE_REQUIRE(kf_start[n_kf] == kf_start[0] || (kf_kp && kf_desc && kf_mask), MAGE_EINVAL, "null argument");
    const AssocConsts c = make_assoc_consts(*settings, *assoc);
    std::vector<Frame> frames(n_kf);
    for (uint32_t k = 0; k < n_kf; k++) {
        make_frame(kf_pos3 + 3ull * k, kf_r9 + 9ull * k, kf_intr4 + 4ull * k, frames[k]);
        const uint32_t nk = kf_start[k + 1] - kf_start[k];
        if (nk > (uint32_t)NA_MAX_KP) {
            *status |= 1u;
            continue;
        }
        // CreateInitialAssociations' own associations (:314)
        for (uint32_t p = 0; p < n_points; p++)
            if (kf_slot[k] >= 0 && points[p].kc_slot == (uint32_t)kf_slot[k] && points[p].kc_index < nk)
                kf_mask[kf_start[k] + points[p].kc_index] = 0;
    }
    for (uint32_t p = 0; p < n_points; p++) {
        const mage_new_point& pt = points[p];
        for (uint32_t k = 0; k < n_kf; k++) {
            const uint32_t nk = kf_start[k + 1] - kf_start[k];
            mage_new_point_assoc& o = out[(size_t)p * n_kf + k];
            o = mage_new_point_assoc{0.f, 0.f, 0, -1};
            if (nk > (uint32_t)NA_MAX_KP) continue;  // over the limit: the verdict byte stays
            uint8_t& v = verdict[(size_t)p * n_kf + k];
            if (pt.ki_index >= n_ki || pt.kc_slot >= (uint32_t)NP_MAX_SLOTS) {
                v = NA_BAD_INDEX;
                continue;
            }
            if (kf_slot[k] >= 0 && pt.kc_slot == (uint32_t)kf_slot[k]) {
                v = pt.kc_index < nk ? NA_SAME_FRAME : NA_BAD_INDEX;
                continue;
            }
            v = project_gate(c, frames[k], kf_intr4 + 4ull * k, pt, o.x, o.y, o.octave);
            if (v != NA_NO_MATCH) continue;
            uint8_t* mask = kf_mask + kf_start[k];
            const int t = host_radius_match_one(c, o.x, o.y, o.octave, ki_desc + 32ull * pt.ki_index, kf_kp + kf_start[k],
                                                kf_desc + 32ull * kf_start[k], nk, mask);
            if (t >= 0) {
                o.keypoint = t;
                mask[t] = 0;
                v = NA_ASSOCIATED;
            }
        }
    }
    return MAGE_OK;
}
