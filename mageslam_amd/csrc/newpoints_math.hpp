// newpoints_math.hpp — the per-match arithmetic of NewMapPointsCreation, shared by the kernel
// (newpoints.hip) and its plain C++ twin (newpoints.cpp).  One function per reference function,
// float32 throughout, in the reference's expression order; every sum of products starts at 0 and
// adds its terms in ascending index, as cv::Matx's product and cv::Vec::dot do.  Both translation
// units are built with -ffp-contract=off, and +, -, *, / and sqrtf are correctly rounded on host
// and device, so the two sides give the same bits.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mage_hot.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NP_HD __host__ __device__ inline
#else
#define NP_HD inline
#endif

namespace mage {
namespace newpoints {

constexpr int NP_MAX_SLOTS = 8;     // Kc keyframes per problem (MaxFramesForNewPointsCreation is 5)
constexpr int NP_MAX_KI = 4096;     // Ki keypoints per problem
constexpr int NP_MAX_LEVELS = 8;    // pyramid levels (MAGE_MAX_LEVELS)
constexpr int NP_MAX_CELLS = 64;    // grid_width x grid_height

enum Verdict : uint8_t {
    NP_ACCEPTED = 0,
    NP_EPIPOLAR = 1,
    NP_BEHIND = 2,
    NP_DISTANCE_RATIO = 3,
    NP_SCALE = 4,
    NP_PARALLAX = 5,
    NP_GRID_FULL = 6,
    NP_KI_TAKEN = 7,
    NP_BAD_INDEX = 8,
};

// The settings as the loops use them: the host computes the transcendental parts once.
struct Consts {
    float two_max_epipolar;  // 2 * MaxEpipolarError
    float min_ratio;
    float cos_min_parallax;  // cosf(deg2rad(MinParallaxDegrees))
    float fmin[NP_MAX_LEVELS], fmax[NP_MAX_LEVELS];  // ComputeDMin / ComputeDMax factors per octave
    float log2s;             // (float)log2((double)scale)
    uint32_t num_levels;
    uint32_t grid_w, grid_h, max_grid_count;
    uint32_t image_w, image_h;
    float cell_w, cell_h;    // (float)gridWidth / (float)imageWidth, likewise the height (:287-288)
};

// nullptr when the settings can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_settings(const mage_new_points_settings* s)
{
    if (!s) return "null settings";
    if (s->struct_size != sizeof(mage_new_points_settings)) return "struct_size is not sizeof(mage_new_points_settings)";
    if (s->num_levels < 1 || s->num_levels > (uint32_t)NP_MAX_LEVELS) return "num_levels must be in 1..8";
    if (!(s->pyramid_scale > 1.f)) return "pyramid_scale must be > 1";
    if (s->grid_width < 1 || s->grid_height < 1 || (uint64_t)s->grid_width * s->grid_height > (uint64_t)NP_MAX_CELLS)
        return "the grid must have 1..64 cells";
    if (s->image_width < 1 || s->image_height < 1) return "image size must be positive";
    return nullptr;
}

inline Consts make_consts(const mage_new_points_settings& s)
{
    Consts c{};
    c.two_max_epipolar = 2 * s.max_epipolar_error;
    c.min_ratio = s.min_accepted_distance_ratio;
    c.cos_min_parallax = cosf(s.min_parallax_degrees * (3.14159265358979323846f / 180.f));
    for (int o = 0; o < NP_MAX_LEVELS; o++) {
        c.fmax[o] = powf(s.pyramid_scale, (float)s.num_levels - ((float)o + 0.5f));
        c.fmin[o] = powf(s.pyramid_scale, 0.f - ((float)o + 0.5f));
    }
    c.log2s = (float)log2((double)s.pyramid_scale);
    c.num_levels = s.num_levels;
    c.grid_w = s.grid_width;
    c.grid_h = s.grid_height;
    c.max_grid_count = s.max_grid_count;
    c.image_w = s.image_width;
    c.image_h = s.image_height;
    c.cell_w = (float)s.grid_width / (float)s.image_width;
    c.cell_h = (float)s.grid_height / (float)s.image_height;
    return c;
}

// One keyframe as the checks read it: the 3x4 view matrix [R | t], its inverse [R^T | C] with
// C = -(R^T t) the world-space position, and the inverse calibration.
struct Frame {
    float R[9];     // row-major view rotation
    float t[3];
    float Rt[9];    // row-major R^T
    float C[3];     // camera centre
    float Kinv[9];  // row-major inverse camera matrix
};

// Everything a (Kc, Ki) pair's matches share.
struct Pair {
    Frame kc;
    float f_kc_to_ki[9], f_ki_to_kc[9];
    float baseline;  // |Ci - Cc|
};

NP_HD void mat3_mul(const float* a, const float* b, float* o)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float s = 0.f;
            for (int k = 0; k < 3; k++) s += a[i * 3 + k] * b[k * 3 + j];
            o[i * 3 + j] = s;
        }
}

NP_HD float dot3(const float* a, const float* b)
{
    float s = 0.f;
    for (int k = 0; k < 3; k++) s += a[k] * b[k];
    return s;
}

// Pose (view-space t, column-major R as mage_ba_set_cameras takes them) and {cx, cy, fx, fy}.
// The inverse view matrix is the closed form R^T, -(R^T t) (the reference inverts the 4x4 with
// cv::Matx::inv; parity unpinned); the inverse calibration is {1/fx, 0, -cx/fx; 0, 1/fy, -cy/fy;
// 0, 0, 1} with -cx/fx evaluated as -(cx / fx).
NP_HD void make_frame(const float* pos3, const float* r9, const float* intr4, Frame& f)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            f.R[i * 3 + j] = r9[j * 3 + i];
            f.Rt[i * 3 + j] = r9[i * 3 + j];
        }
    for (int i = 0; i < 3; i++) f.t[i] = pos3[i];
    for (int i = 0; i < 3; i++) f.C[i] = -dot3(&f.Rt[i * 3], f.t);
    const float cx = intr4[0], cy = intr4[1], fx = intr4[2], fy = intr4[3];
    f.Kinv[0] = 1.f / fx;
    f.Kinv[1] = 0.f;
    f.Kinv[2] = -(cx / fx);
    f.Kinv[3] = 0.f;
    f.Kinv[4] = 1.f / fy;
    f.Kinv[5] = -(cy / fy);
    f.Kinv[6] = 0.f;
    f.Kinv[7] = 0.f;
    f.Kinv[8] = 1.f;
}

// ComputeFundamentalMatrix / ComputeEssentialMatrix (Utils/Epipolar.cpp:14-48):
// Mji = V_to * inverse(V_from), E = [t]x * R of Mji, F = Kinv_to^T * E * Kinv_from.
NP_HD void fundamental(const Frame& from, const Frame& to, float* F)
{
    float Rji[9], tji[3];
    mat3_mul(to.R, from.Rt, Rji);
    for (int i = 0; i < 3; i++) tji[i] = dot3(&to.R[i * 3], from.C) + to.t[i];
    const float T[9] = {0.f, -tji[2], tji[1], tji[2], 0.f, -tji[0], -tji[1], tji[0], 0.f};
    float E[9], KtT[9], M[9];
    mat3_mul(T, Rji, E);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) KtT[i * 3 + j] = to.Kinv[j * 3 + i];
    mat3_mul(KtT, E, M);
    mat3_mul(M, from.Kinv, F);
}

NP_HD void make_pair(const Frame& ki, const Frame& kc, Pair& p)
{
    p.kc = kc;
    fundamental(kc, ki, p.f_kc_to_ki);
    fundamental(ki, kc, p.f_ki_to_kc);
    const float d[3] = {ki.C[0] - kc.C[0], ki.C[1] - kc.C[1], ki.C[2] - kc.C[2]};
    p.baseline = sqrtf(dot3(d, d));
}

// DistanceFromEpipolarLine (Epipolar.cpp:94-107).
NP_HD float epipolar_distance(const float* f, float x1, float y1, float x2, float y2)
{
    const float a = f[0] * x1 + f[1] * y1 + f[2];
    const float b = f[3] * x1 + f[4] * y1 + f[5];
    const float c = f[6] * x1 + f[7] * y1 + f[8];
    float nu = a * a + b * b;
    nu = nu ? 1.f / sqrtf(nu) : 1.f;
    return fabsf(x2 * a + y2 * b + c) * nu;
}

// TriangulatePointWorldSpace (Tracking/Triangulation.cpp:24-60); frame 1 is Kc, frame 2 is Ki.
// `parallel` reports the D < 0.00001f branch.
NP_HD void triangulate(const Frame& f1, const Frame& f2, float x1, float y1, float x2, float y2, float* X, bool& parallel)
{
    const float p1[3] = {x1, y1, 1.f}, p2[3] = {x2, y2, 1.f};
    float c1[3], c2[3], u[3], v[3], w[3];
    for (int i = 0; i < 3; i++) {
        c1[i] = dot3(&f1.Kinv[i * 3], p1);
        c2[i] = dot3(&f2.Kinv[i * 3], p2);
    }
    for (int i = 0; i < 3; i++) {
        u[i] = (dot3(&f1.Rt[i * 3], c1) + f1.C[i] * 1.f) - f1.C[i];
        v[i] = (dot3(&f2.Rt[i * 3], c2) + f2.C[i] * 1.f) - f2.C[i];
        w[i] = f1.C[i] - f2.C[i];
    }
    const float a = dot3(u, u), b = dot3(u, v), c = dot3(v, v), d = dot3(u, w), e = dot3(v, w);
    const float D = a * c - b * b;
    float sc, tc;
    parallel = D < 0.00001f;
    if (parallel) {
        sc = 0.f;
        tc = b > c ? d / b : e / c;
    } else {
        sc = (b * e - c * d) / D;
        tc = (a * e - b * d) / D;
    }
    for (int i = 0; i < 3; i++) X[i] = (((f1.C[i] + sc * u[i]) + f2.C[i]) + tc * v[i]) * 0.5f;
}

// ProjectUndistorted's depth (Tracking/Reprojection.cpp:26-42): row 2 of [R | t] times {X, 1}.
NP_HD float depth_of(const Frame& f, const float* X) { return dot3(&f.R[6], X) + f.t[2] * 1.f; }

// ComputeOctave (Map/MappingMath.h:13-16) in the tracker's convention (track.hip): the logarithm
// in double, the rest in float.
NP_HD int compute_octave(float distance, float dmin, float log2s)
{
    const float r = distance / dmin;
    return (int)roundf((float)log2((double)r) / log2s - 0.5f);
}

struct Geometry {
    float X[3], dir[3];
    float d_min, d_max;
    bool parallel;
};

// TryCreateNewAssociatedMapPointForMatch (NewMapPointsCreation.cpp:74-160) up to the point's
// creation: the first failing check's verdict, or NP_ACCEPTED with the outputs in g.
NP_HD uint8_t match_geometry(const Consts& c, const Frame& ki, const Pair& p, float kcx, float kcy, int kc_octave,
                             float kix, float kiy, int ki_octave, Geometry& g)
{
    const float d_kc_ki = epipolar_distance(p.f_kc_to_ki, kcx, kcy, kix, kiy);
    const float d_ki_kc = epipolar_distance(p.f_ki_to_kc, kix, kiy, kcx, kcy);
    if (d_ki_kc + d_kc_ki > c.two_max_epipolar) return NP_EPIPOLAR;
    triangulate(p.kc, ki, kcx, kcy, kix, kiy, g.X, g.parallel);
    if (depth_of(ki, g.X) <= 0.f || depth_of(p.kc, g.X) <= 0.f) return NP_BEHIND;
    const float vc[3] = {g.X[0] - p.kc.C[0], g.X[1] - p.kc.C[1], g.X[2] - p.kc.C[2]};
    const float dc = sqrtf(dot3(vc, vc));
    const float vi[3] = {g.X[0] - ki.C[0], g.X[1] - ki.C[1], g.X[2] - ki.C[2]};
    const float di = sqrtf(dot3(vi, vi));
    if (di / p.baseline < c.min_ratio) return NP_DISTANCE_RATIO;
    const float dmin = di * c.fmin[ki_octave];
    if (compute_octave(dc, dmin, c.log2s) != kc_octave) return NP_SCALE;  // |predicted - octave| >= 1
    const float nc[3] = {vc[0] / dc, vc[1] / dc, vc[2] / dc};
    const float ni[3] = {vi[0] / di, vi[1] / di, vi[2] / di};
    if (dot3(nc, ni) > c.cos_min_parallax) return NP_PARALLAX;
    const float m[3] = {nc[0] + ni[0], nc[1] + ni[1], nc[2] + ni[2]};
    const float mn = sqrtf(dot3(m, m));  // cv::normalize takes the norm in double; float here
    for (int i = 0; i < 3; i++) g.dir[i] = m[i] / mn;
    g.d_max = di * c.fmax[ki_octave];
    g.d_min = dmin;
    return NP_ACCEPTED;
}

// The initial grid count's cell (:197-199): (int)(pt.x * gridWidth / imageWidth), the size_t
// operands promoted to float; -1 when the cell is outside the grid (the reference would write
// out of bounds).
NP_HD int count_cell(const Consts& c, float x, float y)
{
    const int cx = (int)(x * (float)c.grid_w / (float)c.image_w);
    const int cy = (int)(y * (float)c.grid_h / (float)c.image_h);
    if (cx < 0 || cy < 0 || cx >= (int)c.grid_w || cy >= (int)c.grid_h) return -1;
    return cx + cy * (int)c.grid_w;
}

// The cell a match is tested against (:287-300): clamp((size_t)floor(pt.x * gridWidthPixels), 0,
// gridWidth - 1).  A negative value converts to a huge size_t and clamps to the last cell on the
// reference's platforms; NaN and negatives go to the last cell here too.
NP_HD int test_cell(const Consts& c, float x, float y)
{
    const float fx = floorf(x * c.cell_w), fy = floorf(y * c.cell_h);
    const int gx = fx >= 0.f && fx < (float)c.grid_w ? (int)fx : (int)c.grid_w - 1;
    const int gy = fy >= 0.f && fy < (float)c.grid_h ? (int)fy : (int)c.grid_h - 1;
    return gx + gy * (int)c.grid_w;
}

// ------------------------------------------------------------------------------------------
// LocallyAssociateNewAssociations (NewMapPointsCreation.cpp:337-424): what a new point and a
// covisible keyframe decide before the descriptor search, shared by newpoints_assoc.hip and the
// twin in newpoints.cpp.
// ------------------------------------------------------------------------------------------
constexpr int NA_MAX_KP = 4096;  // keypoints per keyframe (mask bits in LDS)

enum AssocVerdict : uint8_t {
    NA_ASSOCIATED = 0,
    NA_SAME_FRAME = 1,
    NA_BEHIND = 2,
    NA_BORDER = 3,
    NA_ANGLE = 4,
    NA_DISTANCE = 5,
    NA_OCTAVE = 6,
    NA_NO_MATCH = 7,
    NA_BAD_INDEX = 8,
};

struct AssocConsts {
    float radius;         // NewMapPointsSearchRadius
    float border;         // KiImageBorder - NewMapPointsSearchRadius / 2 (:345)
    float cos_max_angle;  // cosf(deg2rad(MaxKeyframeAngleDegrees))
    float log2s;          // (float)log2((double)scale)
    float image_w, image_h;
    int num_levels;
    int max_dist, min_diff;
};

inline const char* check_assoc_settings(const mage_new_points_assoc_settings* a)
{
    if (!a) return "null association settings";
    if (a->struct_size != sizeof(mage_new_points_assoc_settings))
        return "struct_size is not sizeof(mage_new_points_assoc_settings)";
    if (!(a->search_radius >= 0.f)) return "search_radius must be >= 0";
    if (a->max_hamming_distance < -1 || a->max_hamming_distance > 256) return "max_hamming_distance must be in [-1, 256]";
    return nullptr;
}

inline AssocConsts make_assoc_consts(const mage_new_points_settings& s, const mage_new_points_assoc_settings& a)
{
    AssocConsts c{};
    c.radius = a.search_radius;
    c.border = a.image_border - a.search_radius / 2.0f;
    c.cos_max_angle = cosf(a.max_keyframe_angle_degrees * (3.14159265358979323846f / 180.f));
    c.log2s = (float)log2((double)s.pyramid_scale);
    c.image_w = (float)s.image_width;
    c.image_h = (float)s.image_height;
    c.num_levels = (int)s.num_levels;
    c.max_dist = a.max_hamming_distance;
    c.min_diff = a.min_hamming_difference;
    return c;
}

// ProjectUndistorted (Tracking/Reprojection.cpp:26-42), TrackLocalMap::IsGoodCandidate
// (Tracking/TrackLocalMap.cpp:519-554) and the octave test of :387-395 for one point against one
// keyframe, in the reference's order.  Returns the first refusal, or NA_NO_MATCH when the point
// goes on to the descriptor search.  x, y are always set; octave is 0 unless the octave was
// computed (NA_OCTAVE, NA_NO_MATCH).  A point whose dMin is not positive or whose squared distance
// is not finite has no octave (the reference's conversion would be undefined): NA_OCTAVE, octave -1.
NP_HD uint8_t project_gate(const AssocConsts& c, const Frame& f, const float* intr4, const mage_new_point& pt, float& x,
                           float& y, int& octave)
{
    const float* X = pt.position;
    float cs[3];
    for (int r = 0; r < 3; r++)
        cs[r] = (((0.f + f.R[3 * r] * X[0]) + f.R[3 * r + 1] * X[1]) + f.R[3 * r + 2] * X[2]) + f.t[r] * 1.f;
    const float depth = cs[2], div = depth != 0 ? depth : 1.f;
    x = (cs[0] / div) * intr4[2] + intr4[0];
    y = (cs[1] / div) * intr4[3] + intr4[1];
    octave = 0;
    if (depth < 0) return NA_BEHIND;
    if (!(c.border <= x && c.border <= y && x < c.image_w - c.border && y < c.image_h - c.border)) return NA_BORDER;
    if (dot3(pt.mean_view_dir, &f.R[6]) < c.cos_max_angle) return NA_ANGLE;
    const float dl[3] = {X[0] - f.C[0], X[1] - f.C[1], X[2] - f.C[2]};
    const float d2 = (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2];
    if (d2 < pt.d_min * pt.d_min || pt.d_max * pt.d_max < d2) return NA_DISTANCE;
    if (!(pt.d_min > 0.f) || !(d2 <= 3.402823466e+38f)) {
        octave = -1;
        return NA_OCTAVE;
    }
    octave = compute_octave(sqrtf(d2), pt.d_min, c.log2s);
    if (octave < 0 || octave > c.num_levels) return NA_OCTAVE;
    return NA_NO_MATCH;
}

// The host twins' descriptor search (newpoints.cpp, loopclose.cpp).
inline int host_hamming256(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int i = 0; i < 4; i++) {
        uint64_t x, y;
        memcpy(&x, a + 8 * i, 8);
        memcpy(&y, b + 8 * i, 8);
        d += __builtin_popcountll(x ^ y);
    }
    return d;
}

// The single-query RadiusMatch (FeatureMatcher.cpp:386-446) against the available keypoints, the
// candidates in ascending keypoint index: the keypoint, or -1.
inline int host_radius_match_one(const AssocConsts& c, float px, float py, int octave, const uint8_t* desc,
                                 const mage_keypoint* kp, const uint8_t* kdesc, uint32_t n, const uint8_t* mask)
{
    const float r = c.radius;
    int best = c.max_dist + 1, second = 2147483647, train = -1;
    for (uint32_t t = 0; t < n; t++) {
        const float tx = kp[t].x, ty = kp[t].y;
        if (!(tx >= px - r && tx <= px + r && ty >= py - r && ty <= py + r) || kp[t].octave != octave || !mask[t])
            continue;
        const int d = host_hamming256(desc, kdesc + 32ull * t);
        if (d < best) {
            train = (int)t;
            second = best;
            best = d;
        }
    }
    return train != -1 && second - best > c.min_diff ? train : -1;
}

}  // namespace newpoints
}  // namespace mage
