// monoinit.cpp — the plain C++ twin of monoinit.hip: MapInitialization::InitializeWithFrames' two-view
// geometry (Tracking/MapInitialization.cpp:988-1094) as the reference's sequential loops —
// FindPossiblePoses' RANSAC loop with its running best (:210-274), FindCorrectPose's pose loop
// (:350-450) — over the arithmetic of monoinit_math.hpp.  The CPU backend: same verdicts, poses,
// scores, records, trace and bits as the kernels.
//
// This file includes no HIP header, so that it also builds as plain host C++ on its own
// (tests/cpp/mono_init_host_check.cpp): set_error and the argument check are declared here as
// common.hpp declares them.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "monoinit_math.hpp"

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

extern "C" uint64_t mage_mono_init_trace_bytes(uint32_t iterations)
{
    return mage::monoinit::trace_layout(iterations).bytes;
}

extern "C" mage_status mage_mono_init_two_view_host(const mage_mono_init_settings* settings, const float* intr4,
                                                    const mage_keypoint* kp0, uint32_t n0, const mage_keypoint* kp1,
                                                    uint32_t n1, const mage_dmatch* matches, uint32_t n_matches,
                                                    mage_mono_init_result* result, mage_stereo_point* out,
                                                    uint32_t cap, float* ba_points, float* ba_uv, uint32_t* ba_cam,
                                                    uint32_t* ba_pt, float* ba_info, void* trace)
{
    using namespace mage;
    using namespace mage::monoinit;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(intr4 && result, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE((n0 == 0 || kp0) && (n1 == 0 || kp1) && (n_matches == 0 || matches) &&
                     (cap == 0 || (out && ba_points && ba_uv && ba_cam && ba_pt && ba_info)),
                 MAGE_EINVAL, "null argument");
    const Consts c = make_consts(*settings);
    mage_mono_init_result R{};
    R.win_iteration = R.win_root = R.selected_pose = -1;
    R.r9[0] = R.r9[4] = R.r9[8] = R.r9[9] = R.r9[13] = R.r9[17] = 1.f;
    R.n_matches = n_matches;
    if (n0 > (uint32_t)MI_MAX_KP || n1 > (uint32_t)MI_MAX_KP || n_matches > (uint32_t)MI_MAX_MATCHES)
        R.status = MI_STATUS_OVER_LIMIT;
    else
        for (uint32_t m = 0; m < n_matches; m++) {
            const int q = matches[m].query_idx, t = matches[m].train_idx;
            if (q < 0 || (uint32_t)q >= n0 || t < 0 || (uint32_t)t >= n1) R.status = MI_STATUS_BAD_INDEX;
        }
    if (R.status == 0 && n_matches < c.min_matches) R.verdict = MI_FEW_MATCHES;
    if (R.status != 0 || R.verdict != MI_OK) {
        *result = R;
        return MAGE_OK;
    }
    // CollectMatchPoints (:889-909)
    const uint32_t n = n_matches;
    std::vector<Pt4> pts(n);
    for (uint32_t m = 0; m < n; m++) {
        const mage_keypoint &a = kp0[matches[m].query_idx], &b = kp1[matches[m].train_idx];
        pts[m] = Pt4{a.x, a.y, b.x, b.y};
    }
    const TraceLayout L = trace_layout(c.iters);
    std::vector<char> own;
    if (!trace) {
        own.resize(L.bytes);
        trace = own.data();
    }
    char* tb = static_cast<char*>(trace);
    int32_t* t_idx = reinterpret_cast<int32_t*>(tb + L.idx);
    int32_t* t_ncand = reinterpret_cast<int32_t*>(tb + L.ncand);
    float* t_E = reinterpret_cast<float*>(tb + L.E);
    float* t_score = reinterpret_cast<float*>(tb + L.score);
    uint32_t* t_inl = reinterpret_cast<uint32_t*>(tb + L.inliers);
    uint32_t* t_cheir = reinterpret_cast<uint32_t*>(tb + L.cheir);

    Frame f0, k1;
    identity_frame(intr4, f0);
    identity_frame(intr4 + 4, k1);  // frame 1's inverse calibration
    sample_indices([&](int m) { return pts[m]; }, n, c.iters, c.min_spread_sq, t_idx);

    // FindPossiblePoses' loop (:210-274) with its running best
    float best = 0.f;
    for (uint32_t it = 0; it < c.iters; it++) {
        float* E = t_E + 90ull * it;
        Pt4 p5[5];
        int cnt = 0;
        if (t_idx[5 * it] >= 0) {
            for (int k = 0; k < 5; k++) p5[k] = pts[t_idx[5 * it + k]];
            double D[MI_WORK_D];
            float A[MI_WORK_A];
            cnt = solve_five_point(p5, intr4[0], intr4[1], intr4[2], intr4[3], Strided<double>{D, 1}, Strided<float>{A, 1}, E);
        } else {
            std::memset(E, 0, 360);
        }
        t_ncand[it] = cnt;
        for (int r = 0; r < MI_MAX_ROOTS; r++) {
            const uint32_t slot = 10 * it + r;
            t_score[slot] = 0.f;
            t_inl[slot] = 0;
            t_cheir[slot] = 0;
            if (r >= cnt) continue;
            float F12[9], F21[9];
            fundamental_from_essential(E + 9 * r, f0.Kinv, k1.Kinv, F12, F21);
            ScoreState s{0.f, 0};
            for (uint32_t m = 0; m < n; m++) score_match(F12, F21, c.threshold, pts[m], s);
            const float score = score_gate(c, s, n);
            float pos3[12], r9[36];
            decompose_poses(E + 9 * r, pos3, r9);
            const bool ok = consistent_cheirality(pos3, r9, f0, intr4 + 4, p5);
            t_score[slot] = score;
            t_inl[slot] = s.inliers;
            t_cheir[slot] = ok ? 1u : 0u;
            if (score > best && ok) {
                best = score;
                R.win_iteration = (int32_t)it;
                R.win_root = r;
            }
        }
    }
    if (R.win_iteration < 0) {
        R.verdict = MI_NO_HYPOTHESIS;
        *result = R;
        return MAGE_OK;
    }
    R.win_score = best;
    for (int k = 0; k < 5; k++) R.win_indices[k] = t_idx[5 * R.win_iteration + k];
    decompose_poses(t_E + 90ull * R.win_iteration + 9 * R.win_root, R.cand_pos3, R.cand_r9);

    // FindCorrectPose (:324-480)
    float cam_z[4] = {0.f, 0.f, 0.f, 0.f};
    std::vector<float> depth;
    depth.reserve(n);
    PoseEval pe[4];
    for (int p = 0; p < 4; p++) {
        prepare_pose(f0, R.cand_pos3 + 3 * p, R.cand_r9 + 9 * p, intr4 + 4, pe[p]);
        cam_z[p] = pe[p].f1.C[2];
        if (pe[p].twisted) {
            R.cand_flags[p] = MI_POSE_TWISTED;
            continue;
        }
        float score = 0.f;
        depth.clear();
        for (uint32_t m = 0; m < n; m++) {
            float X[3];
            bool parallel;
            const float term = eval_match(c, f0, pe[p], pts[m], X, parallel);
            if (term > 0.f) {
                score += term;
                depth.push_back(X[2]);
            }
        }
        R.cand_score[p] = score;
        R.cand_count[p] = (uint32_t)depth.size();
        R.cand_flags[p] = pose_gate(c, R.cand_count[p], n);
        if (R.cand_flags[p] & MI_POSE_ENOUGH) {
            const size_t mid = depth.size() / 2;
            std::nth_element(depth.begin(), depth.begin() + mid, depth.end());
            R.cand_median[p] = depth[mid];
            if (R.cand_median[p] <= c.max_median) R.cand_flags[p] |= MI_POSE_MEDIAN_OK;
        }
    }
    R.verdict = final_verdict(c, R.cand_flags, R.cand_score, cam_z, R.selected_pose, R.next_best_score);
    if (R.verdict != MI_OK) {
        *result = R;
        return MAGE_OK;
    }
    const int sp = R.selected_pose;
    std::memcpy(R.pos3 + 3, R.cand_pos3 + 3 * sp, 12);
    std::memcpy(R.r9 + 9, R.cand_r9 + 9 * sp, 36);
    // the selected pose's accepted matches in match order, then the bundle adjustment's inputs
    uint32_t accepted = 0;
    for (uint32_t m = 0; m < n; m++) {
        float X[3];
        bool parallel;
        if (!(eval_match(c, f0, pe[sp], pts[m], X, parallel) > 0.f)) continue;
        if (accepted < cap)
            out[accepted] = mage_stereo_point{matches[m].query_idx, matches[m].train_idx, matches[m].distance,
                                              {X[0], X[1], X[2]}, parallel ? 1u : 0u};
        accepted++;
    }
    const uint32_t np = accepted < cap ? accepted : cap;
    R.n_points = np;
    if (accepted > cap) R.status |= MI_STATUS_OVER_CAP;
    const float info = track::refinement_confidence(1);
    for (uint32_t i = 0; i < np; i++) {
        for (int k = 0; k < 3; k++) ba_points[3 * i + k] = out[i].position[k];
        for (uint32_t f = 0; f < 2; f++) {
            const uint32_t o = f * np + i;
            const mage_keypoint& kp = f == 0 ? kp0[out[i].query_idx] : kp1[out[i].train_idx];
            ba_uv[2 * o] = kp.x;
            ba_uv[2 * o + 1] = kp.y;
            ba_cam[o] = f;
            ba_pt[o] = i;
            ba_info[o] = info;
        }
    }
    *result = R;
    return MAGE_OK;
}
