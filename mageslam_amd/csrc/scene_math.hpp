// scene_math.hpp — CalculateBoundingPlaneDepthsForKeyframe (Tracking/BoundingPlaneDepths.cpp:16-87),
// shared by the kernel (scene_depth.hip) and its plain C++ twin (scene_depth.cpp): the camera's world
// position and forward (Data/Pose.cpp:110-118 over Utils/cv.h Invert), the region of interest
// (:35-38, :45-46), a point's depth (:48), its sparse record (:56-60), the ranks of the two order
// statistics (:69, :73) and the order under which depths compare.
//
// Only + - * / appear here, every sum is written in one fixed order, and both translation units are
// built with -ffp-contract=off, so host and gfx950 give the same bits (the rule of monoinit_math.hpp).
#pragma once

#include <cfloat>

#include "newpoints_math.hpp"

namespace mage {
namespace scene {

constexpr uint32_t BD_MAX_POINTS = MAGE_BD_MAX_POINTS;

enum : uint32_t {
    BD_STATUS_BAD_INDEX = MAGE_BD_STATUS_BAD_INDEX,
    BD_STATUS_NONPOSITIVE = MAGE_BD_STATUS_NONPOSITIVE,
    BD_STATUS_OVER_LIMIT = MAGE_BD_STATUS_OVER_LIMIT,
};

// nullptr when the settings can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_settings(const mage_bounding_depth_settings* s)
{
    if (!s) return "null settings";
    if (s->struct_size != sizeof(mage_bounding_depth_settings)) return "struct_size is not sizeof(mage_bounding_depth_settings)";
    if (!(s->near_depth_softness >= 0.f && s->near_depth_softness < 1.f) ||
        !(s->far_depth_softness >= 0.f && s->far_depth_softness < 1.f))
        return "the depth softness values must be in [0, 1)";
    return nullptr;
}

// What a frame's threads read of its pose and settings.
struct Camera {
    float c[3], f[3];              // world position and forward
    float min_x, min_y, max_x, max_y;  // the region of interest in pixels
};

// Invert(view) = invRotation * invTranslation (Utils/cv.h:227-263): column 3 is the position,
// column 2 the forward.  The position is formed as the third-frame stage forms its camera centres
// (monoinit_third_math.hpp midpoint_pose): C = -(R^T t), each component the negated sum
// ((0 + r0 t0) + r1 t1) + r2 t2.  cv::Matx's product sums the same products of -t from 0 and so
// gives the same value, apart from the sign of a component that is exactly zero.  The forward is
// summed as the product sums it, from 0 over the four terms.  The region's bounds are float
// products of the share and the converted size.
NP_HD Camera make_camera(const mage_bounding_depth_settings& s, const float* pos3, const float* r9, uint32_t width,
                         uint32_t height)
{
    Camera k;
    for (int i = 0; i < 3; i++) {
        const float* rt = r9 + 3 * i;  // row i of R^T (r9 is column-major R)
        k.c[i] = -newpoints::dot3(rt, pos3);
        k.f[i] = (((0.f + rt[0] * 0.f) + rt[1] * 0.f) + rt[2] * 1.f) + 0.f * 0.f;
    }
    const float w = (float)width, h = (float)height;
    k.min_x = s.region_of_interest_min_x * w;
    k.min_y = s.region_of_interest_min_y * h;
    k.max_x = s.region_of_interest_max_x * w;
    k.max_y = s.region_of_interest_max_y * h;
    return k;
}

// :45-46 — the closed region.
NP_HD bool in_region(const Camera& k, float x, float y)
{
    return x >= k.min_x && x <= k.max_x && y >= k.min_y && y <= k.max_y;
}

// :48 — (p - c).dot(f), cv::Point3f's dot.
NP_HD float depth_of(const Camera& k, const float* p)
{
    const float d0 = p[0] - k.c[0], d1 = p[1] - k.c[1], d2 = p[2] - k.c[2];
    return (d0 * k.f[0] + d1 * k.f[1]) + d2 * k.f[2];
}

// :56-60 — the sparse record of a point {x, y, z, id bits}.
NP_HD mage_projected_point sparse_of(const float* pos3, const float* r9, const float* intr4, const float* xyzi, int32_t id)
{
    // ProjectUndistorted (Reprojection.cpp:26-42) as monoinit_third_math.hpp's project writes it (that
    // header is not included: it brings HIP's in, and the twin builds as plain host C++)
    float cs[3];
    for (int r = 0; r < 3; r++) cs[r] = (((0.f + r9[r] * xyzi[0]) + r9[3 + r] * xyzi[1]) + r9[6 + r] * xyzi[2]) + pos3[r] * 1.f;
    const float div = cs[2] != 0 ? cs[2] : 1.f;  // prevent division by zero (:32)
    mage_projected_point q;
    q.x = (cs[0] / div) * intr4[2] + intr4[0];
    q.y = (cs[1] / div) * intr4[3] + intr4[1];
    q.depth = cs[2];
    q.id = id;
    return q;
}

// Depths compare through these keys: ascending as unsigned words is ascending as floats, with
// -0 < +0 and every bit pattern distinct, so a selection's result does not depend on how it is done.
NP_HD uint32_t key_of_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
NP_HD uint32_t bits_of_key(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

// :69, :73 — (size_t)(softness * size) with the product in float; a product that rounds up to the
// size itself is held at the last element.
NP_HD uint32_t soft_rank(float softness, uint32_t n_valid)
{
    const uint32_t r = (uint32_t)(softness * (float)n_valid);
    return r < n_valid ? r : n_valid - 1u;
}

// :24, :79-83 — the record from the two selected depths (unused without a valid depth, where near
// keeps numeric_limits<float>::max() and far numeric_limits<float>::min(), the smallest positive normal).
NP_HD mage_depth_result make_result(uint32_t n_valid, uint32_t n_points, uint32_t status, float near_sel, float far_sel)
{
    mage_depth_result r;
    r.near_plane = n_valid ? near_sel : FLT_MAX;
    r.far_plane = n_valid ? far_sel : FLT_MIN;
    if (r.near_plane > r.far_plane) r.near_plane = r.far_plane = MAGE_INVALID_DEPTH;
    r.n_valid = n_valid;
    r.n_points = n_points;
    r.status = status;
    return r;
}

NP_HD mage_depth_result over_limit_result(uint32_t n_points)
{
    mage_depth_result r;
    r.near_plane = r.far_plane = MAGE_INVALID_DEPTH;
    r.n_valid = 0;
    r.n_points = n_points;
    r.status = BD_STATUS_OVER_LIMIT;
    return r;
}

NP_HD bool over_limit(uint32_t n_points, uint32_t cap) { return n_points > cap || cap > BD_MAX_POINTS; }

// ------------------------------------------------------------------------------------------------
// CalculateVolumeOfInterest (VolumeOfInterest/VolumeOfInterest.cpp:45-259), shared by the kernels
// (scene_voi.hip) and their twin (scene_voi.cpp).  acos, exp and the cube root cannot be libm's on
// the device, so they are written here from + - * / and sqrtf (correctly rounded on both sides),
// integer conversions and bit patterns, in one fixed order; the twin uses the same three functions.
// ------------------------------------------------------------------------------------------------

enum : uint32_t {
    VOI_OK = MAGE_VOI_OK,
    VOI_NO_KEYFRAMES = MAGE_VOI_NO_KEYFRAMES,
    VOI_DEGENERATE = MAGE_VOI_DEGENERATE,
    VOI_EMPTY = MAGE_VOI_EMPTY,
};
constexpr int VOI_MAX_ITERATIONS = MAGE_VOI_MAX_ITERATIONS;
constexpr float VOI_PI = 3.14159274f, VOI_HALF_PI = 1.57079637f;  // mira::PI<float>, mira::HALF_PI<float>

NP_HD float float_of_bits(uint32_t u)
{
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
NP_HD uint32_t bits_of_float(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
NP_HD uint32_t key_of(float f) { return key_of_bits(bits_of_float(f)); }
NP_HD float float_of_key(uint32_t k) { return float_of_bits(bits_of_key(k)); }
// min and max under the total order of the keys (-0 < +0); they differ from std::min / std::max in
// the sign of a zero and in where a NaN goes (it is kept and ends as VOI_DEGENERATE)
NP_HD float min_total(float a, float b) { return key_of(b) < key_of(a) ? b : a; }
NP_HD float max_total(float a, float b) { return key_of(b) > key_of(a) ? b : a; }
NP_HD bool finite_f(float f) { return (bits_of_float(f) & 0x7F800000u) != 0x7F800000u; }

// acos of x clamped to [-1, 1] (dot / distance can round past 1 on the view axis, where libm gives
// NaN): the rational approximation of asin of FreeBSD msun's e_acosf.c on the three ranges.
NP_HD float voi_acosf(float x)
{
    const float pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f, pi = 3.1415925026e+00f;
    const float pS0 = 1.6666586697e-01f, pS1 = -4.2743422091e-02f, pS2 = -8.6563630030e-03f, qS1 = -7.0662963390e-01f;
    if (x != x) return x;
    if (x >= 1.f) return 0.f;
    if (x <= -1.f) return pi + 2.f * pio2_lo;
    if (x > -0.5f && x < 0.5f) {
        const float z = x * x;
        const float r = (z * (pS0 + z * (pS1 + z * pS2))) / (1.f + z * qS1);
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (x < 0.f) {
        const float z = (1.f + x) * 0.5f;
        const float r = (z * (pS0 + z * (pS1 + z * pS2))) / (1.f + z * qS1);
        const float s = sqrtf(z);
        const float w = r * s - pio2_lo;
        return pi - 2.f * (s + w);
    }
    const float z = (1.f - x) * 0.5f;
    const float s = sqrtf(z);
    const float df = float_of_bits(bits_of_float(s) & 0xFFFFF000u);
    const float c = (z - df * df) / (s + df);
    const float r = (z * (pS0 + z * (pS1 + z * pS2))) / (1.f + z * qS1);
    const float w = r * s + c;
    return 2.f * (df + w);
}

// exp(x): x = k ln2 + r with ln2 split so that k ln2_hi is exact, a degree-7 Taylor polynomial on
// |r| <= ln2 / 2, the scaling by 2^k as one multiplication (two into the subnormal range, the last
// one rounding).  Below -104 the result is +0, above 88.73 +inf.
NP_HD float voi_expf(float x)
{
    if (x != x) return x;
    if (x < -104.f) return 0.f;
    if (x > 88.73f) return float_of_bits(0x7F800000u);
    const float t = x * 1.44269504f;
    const int k = (int)(t < 0.f ? t - 0.5f : t + 0.5f);
    const float kf = (float)k;
    const float r = (x - kf * 0.693145751953125f) - kf * 1.42860682030941723212e-6f;
    float p = 1.f / 5040.f;
    p = 1.f / 720.f + r * p;
    p = 1.f / 120.f + r * p;
    p = 1.f / 24.f + r * p;
    p = 1.f / 6.f + r * p;
    p = 0.5f + r * p;
    p = 1.f + r * p;
    p = 1.f + r * p;
    if (k >= -126) return p * float_of_bits((uint32_t)(k + 127) << 23);
    return (p * float_of_bits((uint32_t)(k + 100 + 127) << 23)) * float_of_bits((uint32_t)(127 - 100) << 23);
}

// The cube root: the exponent divided by three on the bit pattern (fdlibm's start, 5 bits), two
// Halley steps and one Newton step.  The reference writes pow(v, 1.f / 3.f), whose float exponent
// is not a third; the two differ within float rounding.
NP_HD float voi_cbrtf(float v)
{
    if (v != v || v == 0.f || !finite_f(v)) return v;
    float a = v < 0.f ? -v : v, scale = 1.f;
    // the steps' products stay in range for a in [2^-60, 2^60]: outside it the root of 2^+-72 a,
    // times 2^-+24 (both exact)
    if (a < 8.67361737988403547e-19f) {
        a *= 4722366482869645213696.f;
        scale = 5.9604644775390625e-8f;
    } else if (a > 1152921504606846976.f) {
        a *= 2.11758236813575084767e-22f;
        scale = 16777216.f;
    }
    float t = float_of_bits(bits_of_float(a) / 3u + 709958130u);
    for (int i = 0; i < 2; i++) {
        const float r = (t * t) * t;
        t = (t * ((a + a) + r)) / ((r + r) + a);
    }
    t = t - (t - a / (t * t)) / 3.f;
    t *= scale;
    return v < 0.f ? -t : t;
}

// nullptr when the settings can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_voi_settings(const mage_voi_settings* s)
{
    if (!s) return "null settings";
    if (s->struct_size != sizeof(mage_voi_settings)) return "struct_size is not sizeof(mage_voi_settings)";
    if (s->iterations < 0 || s->iterations > VOI_MAX_ITERATIONS) return "iterations must be in 0..30";
    return nullptr;
}

// The constants that depend on the settings only, with libm on the host (the rule powf follows
// elsewhere in the tree): ToMat (Utils/cv.h:96-116), :59, :103-104.
inline void voi_prepare(mage_voi_settings& s)
{
    const float a = s.kernel_pitch_rads, b = s.kernel_yaw_rads, c = s.kernel_roll_rads;
    const float sa = sinf(a), sb = sinf(b), sc = sinf(c), ca = cosf(a), cb = cosf(b), cc = cosf(c);
    const float m[9] = {cc * cb, -sc, cc * sb, ca * sc * cb + sa * sb, ca * cc, ca * sc * sb - sa * cb,
                        sa * sc * cb - ca * sb, sa * cc, sa * sc * sb + ca * cb};
    for (int i = 0; i < 9; i++) s.kernel_rotation[i] = m[i];
    s.tan_min_angle = tanf(s.kernel_angle_x_rads < s.kernel_angle_y_rads ? s.kernel_angle_x_rads : s.kernel_angle_y_rads);
    s.tan_half_angle_x = tanf(s.kernel_angle_x_rads / 2);
    s.tan_half_angle_y = tanf(s.kernel_angle_y_rads / 2);
}

// Keyframe k's depths: the pair given, or the depth stage's record by index.
NP_HD void voi_depths(const float* near_far, const mage_depth_result* records, uint32_t n_records, const uint32_t* index,
                      uint32_t k, float& near_d, float& far_d)
{
    if (near_far) {
        near_d = near_far[2 * k];
        far_d = near_far[2 * k + 1];
    } else if (index[k] < n_records) {
        near_d = records[index[k]].near_plane;
        far_d = records[index[k]].far_plane;
    } else {
        near_d = far_d = MAGE_INVALID_DEPTH;
    }
}

// A keyframe as the scores read it (VOIKeyframe, :45-61).
struct VoiKf {
    float centroid[3], forward[3];
    float alpha_xi;     // DistanceAlphaToXi
    float mod_omega;    // ModifiedDistanceAlphaToOmega
};

// cv::Matx / cv::Vec sums: from 0, the terms in order.
NP_HD float dot3z(const float* a, const float* b) { return ((0.f + a[0] * b[0]) + a[1] * b[1]) + a[2] * b[2]; }

// :45-61 and :103-117 — the keyframe's record and its eight frustum corners from the
// world-from-camera matrix m (3 x 4, row-major), its depths and the prepared settings.
NP_HD void voi_keyframe(const mage_voi_settings& s, const float* m, float near_d, float far_d, VoiKf& k, float (*corners)[3])
{
    float rot[9];  // Rotation(inverse view) * ToMat(pitch, roll, yaw)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const float col[3] = {s.kernel_rotation[j], s.kernel_rotation[3 + j], s.kernel_rotation[6 + j]};
            rot[3 * i + j] = dot3z(m + 4 * i, col);
        }
    float pos[3], right[3], up[3];
    for (int i = 0; i < 3; i++) {
        pos[i] = m[4 * i + 3];
        right[i] = rot[3 * i];
        up[i] = rot[3 * i + 1];
        k.forward[i] = rot[3 * i + 2];
        k.centroid[i] = pos[i] + (k.forward[i] * near_d) * s.kernel_depth_modifier;
    }
    k.alpha_xi = near_d * s.tan_min_angle;
    k.mod_omega = (far_d - near_d) * s.away_prominence;
    float ox = near_d * s.tan_half_angle_x, oy = near_d * s.tan_half_angle_y;
    for (int pl = 0; pl < 2; pl++) {
        const float d = pl ? far_d : near_d;
        if (pl) {
            ox *= far_d / near_d;
            oy *= far_d / near_d;
        }
        for (int c = 0; c < 4; c++)
            for (int i = 0; i < 3; i++) {
                const float a = (pos[i] + k.forward[i] * d), bx = ox * right[i], by = oy * up[i];
                const float ab = (c & 2) ? a - bx : a + bx;
                corners[4 * pl + c][i] = (c & 1) ? ab - by : ab + by;
            }
    }
}

// TeardropScore (:63-86).
NP_HD float voi_teardrop(const mage_voi_settings& s, const VoiKf& k, const float* point)
{
    const float a[3] = {point[0] - k.centroid[0], point[1] - k.centroid[1], point[2] - k.centroid[2]};
    const float dist = sqrtf(dot3z(a, a));
    if (dist == 0.f) return 1.f;
    const float angle = voi_acosf(dot3z(a, k.forward) / dist);
    const float dev = angle - VOI_HALF_PI;
    const float bias = (2.f * (dev < 0.f ? -dev : dev)) / VOI_PI;
    const float slope = 1.f / k.mod_omega + (angle * (1.f / s.toward_prominence - 1.f)) / (k.mod_omega * VOI_PI);
    const float factor = bias * slope + (1.f - bias) / (k.alpha_xi * s.side_prominence);
    const float x = factor * dist;
    return voi_expf((-2.f * x) * x);
}

// A level's grid (:161-169) from the box it starts with.
struct VoiGrid {
    float min_point[3], side, half;
    int dims[3];
    uint32_t count;  // dims' product
    bool ok;         // false: VOI_DEGENERATE
};
NP_HD VoiGrid voi_grid(const mage_voi_settings& s, int lod, const float* bmin, const float* bmax)
{
    VoiGrid g;
    g.ok = false;
    g.side = g.half = 0.f;
    g.count = 0;
    float diag[3];
    for (int i = 0; i < 3; i++) {
        g.min_point[i] = bmin[i];
        g.dims[i] = 0;
        diag[i] = bmax[i] - bmin[i];
    }
    const int voxels = s.voxel_count_floor / (1 << lod);
    if (voxels <= 0) return g;
    for (int i = 0; i < 3; i++)
        if (!(diag[i] > 0.f) || !finite_f(diag[i])) return g;
    g.side = voi_cbrtf(((diag[0] * diag[1]) * diag[2]) / (float)voxels);
    g.half = g.side / 2.f;
    uint64_t count = 1;
    for (int i = 0; i < 3; i++) {
        const float q = ceilf(diag[i] / g.side);
        if (!(q >= 1.f && q <= 2147483520.f)) return g;
        g.dims[i] = (int)q;
        count *= (uint64_t)g.dims[i];
        if (count > 2147483647ull) return g;
    }
    g.count = (uint32_t)count;
    g.ok = true;
    return g;
}
// Voxel v of the grid in x-fastest order (:172-178).
NP_HD void voi_voxel_point(const VoiGrid& g, uint32_t v, float* p)
{
    const uint32_t dx = (uint32_t)g.dims[0], dy = (uint32_t)g.dims[1];
    const int x = (int)(v % dx), y = (int)((v / dx) % dy), z = (int)(v / (dx * dy));
    p[0] = g.min_point[0] + (float)x * g.side;
    p[1] = g.min_point[1] + (float)y * g.side;
    p[2] = g.min_point[2] + (float)z * g.side;
}
// :200
NP_HD float voi_threshold(const mage_voi_settings& s, int lod, float vmin, float vmax)
{
    return (vmax - vmin) * (s.threshold / (float)lod) + vmin;
}

}  // namespace scene
}  // namespace mage
