// track_math.hpp — the arithmetic of the C4 tracking loop, once: shared by the host-driven loop
// (track.cpp), the device loop's kernels (track.hip) and its host local BA (track_window.hpp);
// tracking.py is the same specification in numpy.  Elementwise products, left-to-right sums,
// float32 projection, float64 poses; built with -ffp-contract=off, and +, -, *, / and sqrtf are
// correctly rounded on host and device, so all sides give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "depth_noise.hpp"
#include "newpoints_math.hpp"  // dot3 and compute_octave: the same expressions, not written again

namespace mage {
namespace track {

using newpoints::compute_octave;
using newpoints::dot3;

struct Pose {
    double R[9];  // world -> camera, row-major
    double t[3];
};

__host__ __device__ inline void mv(const double* R, const double* v, double* out)
{
    for (int i = 0; i < 3; i++) out[i] = (R[3 * i] * v[0] + R[3 * i + 1] * v[1]) + R[3 * i + 2] * v[2];
}

__host__ __device__ inline Pose inverse(const Pose& p)
{
    Pose q;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) q.R[3 * r + c] = p.R[3 * c + r];
    double m[3];
    mv(q.R, p.t, m);
    for (int i = 0; i < 3; i++) q.t[i] = -m[i];
    return q;
}

__host__ __device__ inline Pose mul(const Pose& a, const Pose& b)
{
    Pose o;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            o.R[3 * i + j] = (a.R[3 * i] * b.R[j] + a.R[3 * i + 1] * b.R[3 + j]) + a.R[3 * i + 2] * b.R[6 + j];
    double m[3];
    mv(a.R, b.t, m);
    for (int i = 0; i < 3; i++) o.t[i] = m[i] + a.t[i];
    return o;
}

// motion model: constant velocity on SE3, P[f-1] * P[f-2]^-1 * P[f-1]
__host__ __device__ inline Pose predict(const Pose& prev, const Pose& prev2) { return mul(mul(prev, inverse(prev2)), prev); }

__host__ __device__ inline Pose load_pose(const double* p)  // 12 doubles: R row-major, then t
{
    Pose q;
    for (int i = 0; i < 9; i++) q.R[i] = p[i];
    for (int i = 0; i < 3; i++) q.t[i] = p[9 + i];
    return q;
}

__host__ __device__ inline void store_pose(double* p, const Pose& q)
{
    for (int i = 0; i < 9; i++) p[i] = q.R[i];
    for (int i = 0; i < 3; i++) p[9 + i] = q.t[i];
}

// fp64 row-major pose -> BundlerLib's float view-space position and Eigen column-major rotation
__host__ __device__ inline void to_bundler(const double* R, const double* t, float pos3[3], float r9[9])
{
    for (int i = 0; i < 3; i++) pos3[i] = (float)t[i];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) r9[3 * c + r] = (float)R[3 * r + c];
}

// ... and back (exact in T = double; T = float is what a cast of that double pose gives again)
template <class T>
__host__ __device__ inline void from_bundler(const float pos3[3], const float r9[9], T* R, T* t)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[3 * r + c] = (T)r9[3 * c + r];
    for (int i = 0; i < 3; i++) t[i] = (T)pos3[i];
}

// The float view matrix of the float32 steps (cast per term or into arrays first: the same values)
__host__ __device__ inline void pose_f32(const double* R, const double* t, float R32[9], float t32[3])
{
    for (int i = 0; i < 9; i++) R32[i] = (float)R[i];
    for (int i = 0; i < 3; i++) t32[i] = (float)t[i];
}

// Pose::GetWorldSpacePosition of the float view matrix: column 3 of its inverse (Utils/cv.h:226-262)
__host__ __device__ inline void world_position(const float R[9], const float t[3], float C[3])
{
    for (int i = 0; i < 3; i++) {
        float s = 0.f;
        for (int k = 0; k < 3; k++) s = s + R[3 * k + i] * -t[k];
        C[i] = s + 0.f;
    }
}

// MapPointRefinementConfidence (Map/MappingMath.h:42-49): 1 - 1 / powf(1.5 + count, 2); the square
// of 1.5 + count is exact in float, so x * x is powf's result
__host__ __device__ inline float refinement_confidence(uint32_t count)
{
    const float x = 1.5f + (float)count;
    return 1.f - 1.f / (x * x);
}

// MapPoint::UpdateMeanViewDirectionAndDistances (Map/MapPoint.cpp:131-154) for a point P seen by
// one keyframe with centre C: Normalize(Normalize(P - C)), dmax / dmin from |C - P| and the
// factors of the keypoint's octave (clamped to the tables' 0..7)
__host__ __device__ inline void point_attributes(const float P[3], const float C[3], int octave, const float fmin[8],
                                                 const float fmax[8], float mvd[3], float& dmin, float& dmax)
{
    float v[3] = {P[0] - C[0], P[1] - C[1], P[2] - C[2]};
    const float d = sqrtf(dot3(v, v));
    if (d != 0) {
        const float inv = 1.f / d;
        for (int j = 0; j < 3; j++) v[j] = v[j] * inv;
    }
    const float d2 = sqrtf(dot3(v, v));
    if (d2 != 0) {
        const float inv = 1.f / d2;
        for (int j = 0; j < 3; j++) v[j] = v[j] * inv;
    }
    for (int j = 0; j < 3; j++) mvd[j] = v[j];
    const float dl[3] = {C[0] - P[0], C[1] - P[1], C[2] - P[2]};
    const float dist = sqrtf((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]);
    const int o = octave < 0 ? 0 : (octave > 7 ? 7 : octave);
    dmin = dist * fmin[o];
    dmax = dist * fmax[o];
}

// The ray of keypoint (x, y) of `pose` meets the plane Z = plane_z, the ray parameter scaled by
// the seeded depth error of keypoint i of keyframe `fid` when sigma != 0 (depth_noise.hpp).
__host__ __device__ inline void backproject_to_plane(float x, float y, const Pose& pose, const double K[4], double plane_z,
                                                     uint32_t fid, uint32_t i, float sigma, float out[3])
{
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    const double* R = pose.R;
    double C[3];
    for (int j = 0; j < 3; j++) C[j] = -((R[j] * pose.t[0] + R[3 + j] * pose.t[1]) + R[6 + j] * pose.t[2]);
    const double u = ((double)x - cx) / fx, v = ((double)y - cy) / fy;
    double d[3];
    for (int j = 0; j < 3; j++) d[j] = (u * R[j] + v * R[3 + j]) + R[6 + j];
    double lam = (plane_z - C[2]) / d[2];
    if (sigma != 0.f) lam = lam * depth_noise_factor(fid, i, sigma);
    for (int j = 0; j < 3; j++) out[j] = (float)(C[j] + lam * d[j]);
}

// ProjectUndistorted of map point X (float32 view and camera matrices): true when in front; u, v
// are evaluated either way (the host loop drops them when false: no other effect).
__host__ __device__ inline bool project_front(const float R32[9], const float t32[3], float fx, float fy, float cx,
                                              float cy, const float X[3], float& u, float& v)
{
    float xc[3];
    for (int r = 0; r < 3; r++) xc[r] = ((R32[3 * r] * X[0] + R32[3 * r + 1] * X[1]) + R32[3 * r + 2] * X[2]) + t32[r];
    u = (xc[0] / xc[2]) * fx + cx;
    v = (xc[1] / xc[2]) * fy + cy;
    return xc[2] > 0.f;
}

// ProjectMapPointIntoCurrentFrame + IsGoodCandidate + ComputeOctave (TrackLocalMap.cpp:325-370,
// 519-554; MappingMath.h:13-16) of map point P (mean viewing direction mvd, dmin, dmax) under the
// float view matrix R, t with centre C: in front, inside the border, viewing angle,
// scale-invariance distance, octave in 0..num_levels (every test evaluated: they have no side
// effects, so leaving at the first failing one gives the same).
__host__ __device__ inline bool local_map_candidate(const float R[9], const float t[3], const float C[3], float fx,
                                                    float fy, float cx, float cy, const mage_track_settings& s,
                                                    float log2s, const float P[3], const float mvd[3], float dmin,
                                                    float dmax, float& px, float& py, int& oc)
{
    const float border = s.image_border, W = (float)s.width, H = (float)s.height;
    float cs[3];
    for (int r = 0; r < 3; r++)
        cs[r] = (((0.f + R[3 * r] * P[0]) + R[3 * r + 1] * P[1]) + R[3 * r + 2] * P[2]) + t[r] * 1.f;
    const float depth = cs[2], div = depth != 0 ? depth : 1.f;
    px = (cs[0] / div) * fx + cx;
    py = (cs[1] / div) * fy + cy;
    bool ok = !(depth < 0) && border <= px && border <= py && px < W - border && py < H - border;
    ok = ok && !(dot3(mvd, &R[6]) < s.min_view_cos);  // GetWorldSpaceForward: row 2 of the view rotation
    const float dl[3] = {P[0] - C[0], P[1] - C[1], P[2] - C[2]};
    const float d2 = (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2];
    ok = ok && !(d2 < dmin * dmin || dmax * dmax < d2);
    oc = 0;
    if (ok) {
        oc = compute_octave(sqrtf(d2), dmin, log2s);
        ok = oc >= 0 && oc <= (int)s.num_levels;
    }
    return ok;
}

// ComputeDMax / ComputeDMin factors per octave (MappingMath.h:32-40) and ComputeOctave's
// log2f(scale).  Host only: powf stays on the host.
inline void octave_factors(float scale, uint32_t num_levels, float fmax[8], float fmin[8], float* log2s)
{
    for (int o = 0; o < 8; o++) {
        fmax[o] = powf(scale, (float)num_levels - ((float)o + 0.5f));
        fmin[o] = powf(scale, 0.f - ((float)o + 0.5f));
    }
    *log2s = (float)log2((double)scale);
}

}  // namespace track
}  // namespace mage
