// stereoinit.cpp — the plain C++ twin of stereoinit.hip: CreateFilteredDescriptorMask
// (Core/MAGESLAM/Source/Stereo/StereoMapInit.cpp:28-45) and MapInitialization::TriangulatePoints'
// sequential loop (Tracking/MapInitialization.cpp:931-985) over the per-match arithmetic of
// stereoinit_math.hpp, then the bundle adjustment's inputs in BundleAdjustInitializationData's
// order (:1099-1110).  The CPU backend: same masks, verdicts, points and bits as the kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "stereoinit_math.hpp"

extern "C" mage_status mage_stereo_init_triangulate_host(const mage_stereo_init_settings* settings, const float* pos3,
                                                         const float* r9, const float* intr4,
                                                         const int32_t crop_xywh[4], const mage_keypoint* kp0,
                                                         uint32_t n0, const mage_keypoint* kp1, uint32_t n1,
                                                         const mage_dmatch* matches, uint32_t n_matches,
                                                         uint8_t* mask0, uint32_t* n_masked, uint8_t* verdict,
                                                         mage_stereo_point* out, uint32_t cap, uint32_t* n_out,
                                                         float* ba_points, float* ba_uv, uint32_t* ba_cam,
                                                         uint32_t* ba_pt, float* ba_info, uint32_t* status)
{
    using namespace mage;
    using namespace mage::stereoinit;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(pos3 && r9 && intr4 && crop_xywh && n_masked && n_out && status, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE((n0 == 0 || (kp0 && mask0)) && (n1 == 0 || kp1) && (n_matches == 0 || (matches && verdict)) &&
                     (cap == 0 || (out && ba_points && ba_uv && ba_cam && ba_pt && ba_info)),
                 MAGE_EINVAL, "null argument");
    *n_masked = 0;
    *n_out = 0;
    *status = 0;
    if (n0 > (uint32_t)ST_MAX_KP || n1 > (uint32_t)ST_MAX_KP) {  // over the limit: nothing else is written
        *status = ST_STATUS_OVER_LIMIT;
        return MAGE_OK;
    }
    uint32_t masked = 0;
    for (uint32_t i = 0; i < n0; i++) {
        mask0[i] = within_area(kp0[i].x, kp0[i].y, crop_xywh) ? 1 : 0;
        masked += mask0[i];
    }
    *n_masked = masked;
    StereoPair pair;
    make_stereo_pair(pos3, r9, intr4, pair);
    const float two_max = 2 * settings->max_epipolar_error;
    uint32_t accepted = 0;
    for (uint32_t m = 0; m < n_matches; m++) {
        const int q = matches[m].query_idx, t = matches[m].train_idx;
        if (q < 0 || (uint32_t)q >= n0 || t < 0 || (uint32_t)t >= n1) {
            verdict[m] = ST_BAD_INDEX;
            continue;
        }
        float X[3] = {0.f, 0.f, 0.f};
        bool parallel = false;
        const uint8_t v = stereo_match_geometry(pair, two_max, settings->min_accepted_distance_ratio, kp0[q].x, kp0[q].y,
                                                kp0[q].octave, kp1[t].x, kp1[t].y, kp1[t].octave, X, parallel);
        verdict[m] = v;
        if (v != ST_ACCEPTED) continue;
        if (accepted < cap) out[accepted] = mage_stereo_point{q, t, matches[m].distance, {X[0], X[1], X[2]}, parallel ? 1u : 0u};
        accepted++;
    }
    const uint32_t n = accepted < cap ? accepted : cap;
    *n_out = n;
    if (accepted > cap) *status |= ST_STATUS_OVER_CAP;
    const float info = track::refinement_confidence(1);
    for (uint32_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) ba_points[3 * i + k] = out[i].position[k];
        for (uint32_t f = 0; f < 2; f++) {
            const uint32_t o = f * n + i;
            const mage_keypoint& kp = f == 0 ? kp0[out[i].query_idx] : kp1[out[i].train_idx];
            ba_uv[2 * o] = kp.x;
            ba_uv[2 * o + 1] = kp.y;
            ba_cam[o] = f;
            ba_pt[o] = i;
            ba_info[o] = info;
        }
    }
    return MAGE_OK;
}

// ------------------------------------------------------------------------------------------
// StereoMapInit::Initialize as one call (Stereo/StereoMapInit.cpp:97-194): the host part around the
// device stage.  Everything is float as the reference evaluates it; cv::Matx44f products, the LU
// inverse and Invert (Utils/cv.h:226-262) are image.hip's restatements.
// ------------------------------------------------------------------------------------------
namespace mage {
void matx44f_mul(const float* a, const float* b, float* out);
void matx44f_inverse(const float* a, float* out);
void matx44f_rigid_inverse(const float* t, float* out);

namespace stereoinit {

// Eigen::Quaternionf(Matrix3f) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other,
// 3, 3>) followed by normalize(), as ToQuat does (Utils/cv.h:22-32).  m row-major, q = x, y, z, w.
// The squared norm is summed left to right (Eigen's packet order is not pinned).
void to_quat(const float* m, float* q)
{
    float t = (m[0] + m[4]) + m[8];
    if (t > 0.f) {
        t = sqrtf(t + 1.0f);
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
        t = sqrtf(((m[i * 4] - m[j * 4]) - m[k * 4]) + 1.0f);
        q[i] = 0.5f * t;
        t = 0.5f / t;
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
    const float n = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int c = 0; c < 4; c++) q[c] /= n;
}

// Quaternionf::toRotationMatrix, as ToMat does (Utils/cv.h:89-94).  m row-major.
void quat_to_mat(const float* q, float* m)
{
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
                tyz = tz * y, tzz = tz * z;
    m[0] = 1.f - (tyy + tzz);
    m[1] = txy - twz;
    m[2] = txz + twy;
    m[3] = txy + twz;
    m[4] = 1.f - (txx + tzz);
    m[5] = tyz - twx;
    m[6] = txz - twy;
    m[7] = tyz + twx;
    m[8] = 1.f - (txx + tyy);
}

struct HostScalars {
    bool zero_displacement;
    float length;          // |translation| of frame0ToFrame1
    float normalized[16];  // frame0ToFrame1 with the translation scaled to length 1 (:135-148)
    float world1[16];      // normalized.inv(): frame 1's inverse view matrix (:157)
    float pos3[3], r9[9];  // frame 1's view matrix Invert(world1): t and column-major R
    float tether[7];       // SetRelativeTransformConstraint's position and quaternion x, y, z, w
};

// StereoMapInit.cpp:135-157 and the extrinsic tether of :168 as KeyframeBuilder::AddExtrinsicTether
// (KeyframeBuilder.h:38-48) stores it and BuildDataForG2O hands it on (BundleAdjust.cpp:177-192).
void host_scalars(const float* f0_to_f1, HostScalars& h)
{
    std::memcpy(h.normalized, f0_to_f1, sizeof(h.normalized));
    const double x = h.normalized[3], y = h.normalized[7], z = h.normalized[11];
    h.length = (float)std::sqrt((x * x + y * y) + z * z);  // cv::norm(Vec3f, NORM_L2) accumulates in double
    h.zero_displacement = h.length < 0.00001f;
    if (h.zero_displacement) return;
    const float one_over = 1 / h.length;
    h.normalized[3] *= one_over;
    h.normalized[7] *= one_over;
    h.normalized[11] *= one_over;
    // Pose{world}: the inverse view matrix is the world matrix itself, the view matrix Invert(world)
    matx44f_inverse(h.normalized, h.world1);
    float view[16];
    matx44f_rigid_inverse(h.world1, view);
    for (int i = 0; i < 3; i++) {
        h.pos3[i] = view[i * 4 + 3];
        for (int j = 0; j < 3; j++) h.r9[j * 3 + i] = view[i * 4 + j];
    }
    // transform = frame 0's view matrix (identity) * frame 1's inverse view matrix
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float tr[16], rot[9], q[4], tm[16], tinv[16];
    matx44f_mul(eye, h.world1, tr);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) rot[i * 3 + j] = tr[i * 4 + j];
    to_quat(rot, q);
    // Tether::TransformMatrix() (Tether.h:73-82), inverted again for the bundler
    quat_to_mat(q, rot);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) tm[i * 4 + j] = rot[i * 3 + j];
        tm[i * 4 + 3] = tr[i * 4 + 3];
        tm[12 + i] = 0.f;
    }
    tm[15] = 1.f;
    matx44f_inverse(tm, tinv);
    for (int i = 0; i < 3; i++) {
        h.tether[i] = tinv[i * 4 + 3];
        for (int j = 0; j < 3; j++) rot[i * 3 + j] = tinv[i * 4 + j];
    }
    to_quat(rot, h.tether + 3);
}

// BundleAdjustInitializationData's culling (MapInitialization.cpp:1166-1222) for n points with one
// association in each of the two frames; observation o < n is point o in frame 0, o >= n point
// o - n in frame 1.  order: the surviving points' original indices in the reference's order after
// its swap-with-back removals.  An outlier listed twice removes its association once.
void cull(uint32_t n, const uint32_t* outliers, uint32_t n_outliers, std::vector<uint32_t>& order)
{
    std::vector<int> count(n, 2);
    std::vector<uint8_t> present(2 * (size_t)n, 1);
    for (uint32_t k = 0; k < n_outliers; k++) {
        const uint32_t o = outliers[k];
        if (o >= 2 * n || !present[o]) continue;
        present[o] = 0;
        count[o < n ? o : o - n]--;
    }
    order.resize(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    for (uint32_t i = 0; i < n; i++)
        if (count[i] < 2)
            for (size_t k = 0; k < order.size(); k++)
                if (order[k] == i) {
                    std::swap(order[k], order.back());
                    order.pop_back();
                    break;
                }
}

// ValidateInitializationData (MapInitialization.cpp:1228-1268) for two frames: frame 1's pose as the
// bundler returned it (view-space t, column-major R).
bool validate(const mage_stereo_init_settings& s, uint32_t n_points, const float* pos3, const float* r9)
{
    if (n_points < s.min_init_map_points) return false;
    // Pose{position, rotation}: GetWorldSpacePosition is column 3 of Invert(view)
    float view[16] = {r9[0], r9[3], r9[6], pos3[0], r9[1], r9[4], r9[7], pos3[1], r9[2], r9[5], r9[8], pos3[2], 0, 0, 0, 1};
    float inv[16];
    matx44f_rigid_inverse(view, inv);
    const float w[3] = {inv[3], inv[7], inv[11]};
    const float dot = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const float len = sqrtf(dot);
    const float nz = len == 0 ? w[2] : w[2] / len;
    if (fabsf(nz) > s.max_pose_contribution_z) return false;
    const float scale = len, a = s.amount_ba_can_change_pose;
    if (a != 0 && (scale < 1.0f / a || scale > 1.0f * a)) return false;
    return true;
}

}  // namespace stereoinit
}  // namespace mage

extern "C" mage_status mage_debug_stereo_init_host(const mage_stereo_init_settings* settings, const float frame0_to_frame1[16],
                                                   int32_t* zero_displacement, float normalized[16], float pos3[3],
                                                   float r9[9], float tether7[7], uint32_t n_points,
                                                   const uint32_t* outliers, uint32_t n_outliers, uint32_t* order,
                                                   uint32_t* n_left, const float* ba_pos3, const float* ba_r9,
                                                   int32_t* valid)
{
    using namespace mage;
    using namespace mage::stereoinit;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    if (frame0_to_frame1) {
        MAGE_REQUIRE(zero_displacement && normalized && pos3 && r9 && tether7, MAGE_EINVAL, "null argument");
        HostScalars h{};
        host_scalars(frame0_to_frame1, h);
        *zero_displacement = h.zero_displacement;
        std::memcpy(normalized, h.normalized, sizeof(h.normalized));
        std::memcpy(pos3, h.pos3, sizeof(h.pos3));
        std::memcpy(r9, h.r9, sizeof(h.r9));
        std::memcpy(tether7, h.tether, sizeof(h.tether));
    }
    std::vector<uint32_t> left;
    if (order) {
        MAGE_REQUIRE(n_left && (n_outliers == 0 || outliers), MAGE_EINVAL, "null argument");
        cull(n_points, outliers, n_outliers, left);
        *n_left = (uint32_t)left.size();
        if (!left.empty()) std::memcpy(order, left.data(), 4 * left.size());
    }
    if (valid) {
        MAGE_REQUIRE(ba_pos3 && ba_r9, MAGE_EINVAL, "null argument");
        *valid = validate(*settings, order ? (uint32_t)left.size() : n_points, ba_pos3, ba_r9);
    }
    return MAGE_OK;
}

extern "C" mage_status mage_stereo_map_init(const mage_stereo_init_settings* settings, const float frame0_to_frame1[16],
                                            const mage_camera_config* camera0, const mage_camera_config* camera1,
                                            const mage_keypoint* kp0, const uint8_t* desc0, uint32_t n0,
                                            const mage_keypoint* kp1, const uint8_t* desc1, uint32_t n1,
                                            mage_stereo_map_init_result* result, uint8_t* mask0, mage_dmatch* matches,
                                            uint8_t* verdict, mage_stereo_point* points, uint32_t* ba_outliers,
                                            int device)
{
    using namespace mage;
    using namespace mage::stereoinit;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(frame0_to_frame1 && camera0 && camera1 && result, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE(n0 == 0 || (kp0 && desc0 && mask0 && matches && verdict && points && ba_outliers), MAGE_EINVAL,
                 "null argument");
    MAGE_REQUIRE(n1 == 0 || (kp1 && desc1), MAGE_EINVAL, "null argument");
    MAGE_REQUIRE(n0 <= (uint32_t)ST_MAX_KP && n1 <= (uint32_t)ST_MAX_KP, MAGE_EUNSUPPORTED,
                 "more than 4096 keypoints in a frame");
    const mage_stereo_init_settings& s = *settings;
    *result = mage_stereo_map_init_result{};
    result->frame1_r9[0] = result->frame1_r9[4] = result->frame1_r9[8] = 1.f;
    // 1. crop (:100), mask (:104-105), match (:112) — and, with them, the triangulation of :159, whose
    // results count only if the two checks below pass
    mage_status r = mage_overlap_crop_source_in_target(frame0_to_frame1, camera0, camera1, s.max_depth_meters, result->crop);
    if (r != MAGE_OK) return r;
    HostScalars h{};
    host_scalars(frame0_to_frame1, h);
    const float eye9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    float pos3[6] = {0, 0, 0, 0, 0, 0}, r9[18];
    std::memcpy(r9, eye9, sizeof(eye9));
    std::memcpy(r9 + 9, eye9, sizeof(eye9));
    if (!h.zero_displacement) {
        std::memcpy(pos3 + 3, h.pos3, sizeof(h.pos3));
        std::memcpy(r9 + 9, h.r9, sizeof(h.r9));
    }
    const float intr[8] = {camera0->cx, camera0->cy, camera0->fx, camera0->fy,
                           camera1->cx, camera1->cy, camera1->fx, camera1->fy};
    const uint32_t cap = std::max(n0, 1u);
    std::vector<float> bp(3 * (size_t)cap), uv(4 * (size_t)cap), info(2 * (size_t)cap);
    std::vector<uint32_t> cam(2 * (size_t)cap), pt(2 * (size_t)cap);
    std::vector<mage_stereo_point> acc(cap);
    std::vector<mage_dmatch> mm(cap);
    std::vector<uint8_t> vv(cap), mk(cap);
    uint32_t n_matches = 0, n_acc = 0, status = 0;
    const uint8_t none[32] = {};  // an empty frame may come without descriptors; the matcher still runs
    r = mage_stereo_init_triangulate(settings, pos3, r9, intr, result->crop, kp0, desc0 ? desc0 : none, n0, kp1,
                                     desc1 ? desc1 : none, n1, mm.data(), cap, &n_matches, mk.data(),
                                     &result->n_masked, vv.data(), acc.data(), cap, &n_acc, bp.data(), uv.data(),
                                     cam.data(), pt.data(), info.data(), &status, device);
    if (r != MAGE_OK) return r;
    result->n_matches = n_matches;
    if (n0) std::memcpy(mask0, mk.data(), n0);
    if (n_matches) std::memcpy(matches, mm.data(), sizeof(mage_dmatch) * (size_t)n_matches);
    // 2. zero displacement (:139), 3. match count (:151)
    if (h.zero_displacement) {
        result->code = MAGE_STEREO_INIT_ZERO_DISPLACEMENT;
        return MAGE_OK;
    }
    if (n_matches < s.min_feature_matches) {
        result->code = MAGE_STEREO_INIT_FEW_MATCHES;
        return MAGE_OK;
    }
    // 4. triangulate (:159), 5. point count (:161)
    if (n_matches) std::memcpy(verdict, vv.data(), n_matches);
    result->n_verdicts = n_matches;
    std::memcpy(result->frame1_pos3, h.pos3, sizeof(h.pos3));
    std::memcpy(result->frame1_r9, h.r9, sizeof(h.r9));
    if (n_acc < s.min_init_map_points) {
        result->code = MAGE_STEREO_INIT_FEW_POINTS;
        return MAGE_OK;
    }
    // 6. tether (:168), bundle adjustment and culling (:181)
    mage_ba* ba = nullptr;
    if ((r = mage_ba_create(0, device, &ba)) != MAGE_OK) return r;
    const uint8_t fixed[2] = {1, 0};
    const uint32_t c0 = 0, c1 = 1;
    std::vector<float> huber(s.ba_num_steps_per_run, s.ba_huber_width);
    std::vector<uint32_t> outl(2 * (size_t)cap * ((size_t)s.ba_num_steps / s.ba_num_steps_per_run + 2));
    uint32_t total = 0, count = 0, runs = 0;
    float resid = 0.f, max_err_sq = s.ba_max_outlier_error;  // BundleAdjustSettings', as the reference passes it
    const float scale_sq = s.ba_max_outlier_error_scale_factor * s.ba_max_outlier_error_scale_factor;
    r = mage_ba_set_cameras(ba, 2, pos3, r9, intr, fixed);
    if (r == MAGE_OK) r = mage_ba_set_points(ba, n_acc, bp.data());
    if (r == MAGE_OK) r = mage_ba_set_observations(ba, 2 * n_acc, uv.data(), cam.data(), pt.data(), info.data());
    if (r == MAGE_OK)
        r = mage_ba_set_tethers(ba, MAGE_TETHER_TRANSFORM, 1, &c0, &c1, h.tether, &s.initialization_tether_strength);
    // RunBundleAdjustment's schedule with the NoOpScheduler (BundleAdjust.cpp:300-345)
    while (r == MAGE_OK) {
        uint32_t n = 0;
        r = mage_ba_step(ba, huber.data(), s.ba_num_steps_per_run, max_err_sq, outl.data() + total,
                         (uint32_t)(outl.size() - total), &n, &resid);
        if (r != MAGE_OK) break;
        total += std::min<uint32_t>(n, (uint32_t)(outl.size() - total));
        count += s.ba_num_steps_per_run;
        max_err_sq *= scale_sq;
        runs++;
        if (!(count < s.ba_num_steps && (resid > s.ba_min_mean_square_error || count < s.ba_min_steps))) break;
    }
    float bpos[6], br9[18];
    if (r == MAGE_OK) r = mage_ba_get_poses(ba, bpos, br9);
    if (r == MAGE_OK) r = mage_ba_get_points(ba, bp.data());
    (void)mage_ba_destroy(ba);
    if (r != MAGE_OK) return r;
    result->ba_runs = runs;
    result->n_ba_outliers = total;
    if (total) std::memcpy(ba_outliers, outl.data(), 4ull * total);
    std::memcpy(result->frame1_pos3, bpos + 3, 12);  // the fixed frame 0 keeps its pose (:1143)
    std::memcpy(result->frame1_r9, br9 + 9, 36);
    std::vector<uint32_t> order;
    cull(n_acc, outl.data(), total, order);
    result->n_points = (uint32_t)order.size();
    for (size_t k = 0; k < order.size(); k++) {
        points[k] = acc[order[k]];
        for (int c = 0; c < 3; c++) points[k].position[c] = bp[3 * (size_t)order[k] + c];
    }
    // 7. validation (:183)
    result->code = validate(s, result->n_points, result->frame1_pos3, result->frame1_r9) ? MAGE_STEREO_INIT_OK
                                                                                          : MAGE_STEREO_INIT_FAILED_VALIDATION;
    return MAGE_OK;
}
