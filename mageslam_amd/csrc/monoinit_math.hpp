// monoinit_math.hpp — the two-view geometry of MapInitialization::InitializeWithFrames
// (Tracking/MapInitialization.cpp:988-1094), shared by the kernels (monoinit.hip) and their plain
// C++ twin (monoinit.cpp): the RANSAC sampler of FindPossiblePoses (:196-249), the five-point
// solver (Tracking/ComputeEssential.cpp:357-514) as polynomial arithmetic over coefficient arrays,
// ScoreFundamentalMatrix (:279-322), HasConsistentCheirality (:129-179),
// FindEssentialPotientialPoses (:85-114) and FindCorrectPose's per-pose and final decisions
// (:324-480) over the arithmetic of newpoints_math.hpp, which is used as it is.
//
// Only + - * /, sqrt / sqrtf and fabs / fabsf appear here, every sum is written in one fixed order,
// and both translation units are built with -ffp-contract=off, so host and gfx950 give the same
// bits in fp32 and fp64.  The big per-hypothesis arrays live behind Strided<T>: plain arrays on
// the host, lane-interleaved LDS on the device.
#pragma once

#include <float.h>

#include "cv_rng.hpp"
#include "newpoints_math.hpp"
#include "track_math.hpp"

#if defined(__clang__)
#define MI_UNROLL _Pragma("unroll")
#else
#define MI_UNROLL
#endif

namespace mage {
namespace monoinit {

using newpoints::dot3;
using newpoints::Frame;
using newpoints::mat3_mul;

constexpr int MI_MAX_KP = 4096;       // keypoints per frame (the two-way matcher's limit)
constexpr int MI_MAX_MATCHES = 4096;  // matches per pair (LDS staging and the median's sort)
constexpr int MI_MAX_ITERS = 256;     // RansacIterationsForModels
constexpr int MI_MAX_ROOTS = 10;      // essential matrices per hypothesis
constexpr int MI_WORK_D = 81;         // doubles of per-hypothesis workspace
constexpr int MI_WORK_A = 200;        // floats of per-hypothesis workspace (the 10 x 20 matrix)

enum : uint32_t {
    MI_OK = MAGE_MI_OK,
    MI_FEW_MATCHES = MAGE_MI_FEW_MATCHES,
    MI_NO_HYPOTHESIS = MAGE_MI_NO_HYPOTHESIS,
    MI_NO_VALID_POSE = MAGE_MI_NO_VALID_POSE,
    MI_TOO_SIMILAR = MAGE_MI_TOO_SIMILAR,
    MI_Z_BIASED = MAGE_MI_Z_BIASED,
};
enum : uint32_t {
    MI_STATUS_OVER_LIMIT = MAGE_MI_STATUS_OVER_LIMIT,
    MI_STATUS_OVER_CAP = MAGE_MI_STATUS_OVER_CAP,
    MI_STATUS_BAD_INDEX = MAGE_MI_STATUS_BAD_INDEX,
};
enum : uint32_t { MI_POSE_TWISTED = 1u, MI_POSE_ENOUGH = 2u, MI_POSE_MEDIAN_OK = 4u };

// nullptr when the settings can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_settings(const mage_mono_init_settings* s)
{
    if (!s) return "null settings";
    if (s->struct_size != sizeof(mage_mono_init_settings)) return "struct_size is not sizeof(mage_mono_init_settings)";
    if (!(s->fundamental_transfer_error_threshold > 0.f)) return "fundamental_transfer_error_threshold must be > 0";
    if (s->min_feature_matches < 5) return "min_feature_matches must be >= 5 (a sample is five matches)";
    if (!(s->min_inlier_percentage >= 0.f)) return "min_inlier_percentage must be >= 0";
    if (!(s->max_parallax_3d_distance > 0.f) || !(s->max_parallax_3d_median_distance > 0.f))
        return "the parallax distances must be > 0";
    if (!(s->max_pose_contribution_z >= 0.f)) return "max_pose_contribution_z must be >= 0";
    if (s->ransac_iterations_for_models < 1 || s->ransac_iterations_for_models > (uint32_t)MI_MAX_ITERS)
        return "ransac_iterations_for_models must be in 1..256";
    if (!(s->max_epipolar_error >= 0.f)) return "max_epipolar_error must be >= 0";
    if (!(s->min_pixel_spread >= 0.f)) return "min_pixel_spread must be >= 0";
    if (s->five_point_max_hamming_distance < -1 || s->five_point_max_hamming_distance > 256)
        return "five_point_max_hamming_distance must be in [-1, 256]";
    if (s->five_point_min_hamming_difference < 0 || s->five_point_min_hamming_difference > 256)
        return "five_point_min_hamming_difference must be in [0, 256]";
    return nullptr;
}

// The settings as the loops read them.
struct Consts {
    float threshold;      // FundamentalTransferErrorThreshold
    float min_pct;        // MinInlierPercentage
    float max_dist;       // MaxParallax3dDistance
    float max_median;     // MaxParallax3dMedianDistance
    float min_dissim;     // MinCandidatePoseDisimilarity
    float max_z;          // MaxPoseContributionZ
    float two_max_epi;    // 2 * MaxEpipolarError
    float min_spread_sq;  // MinPixelSpread^2
    uint32_t min_matches, min_inliers, iters;
};

inline Consts make_consts(const mage_mono_init_settings& s)
{
    Consts c{};
    c.threshold = s.fundamental_transfer_error_threshold;
    c.min_pct = s.min_inlier_percentage;
    c.max_dist = s.max_parallax_3d_distance;
    c.max_median = s.max_parallax_3d_median_distance;
    c.min_dissim = s.min_candidate_pose_disimilarity;
    c.max_z = s.max_pose_contribution_z;
    c.two_max_epi = 2 * s.max_epipolar_error;
    c.min_spread_sq = s.min_pixel_spread * s.min_pixel_spread;
    c.min_matches = s.min_feature_matches;
    c.min_inliers = s.min_scoring_inliers;
    c.iters = s.ransac_iterations_for_models;
    return c;
}

// The trace / work buffer of one pair, `iters` RANSAC iterations (see mage_hot.h): offsets in bytes.
struct TraceLayout {
    size_t idx, ncand, E, score, inliers, cheir, bytes;
};
NP_HD TraceLayout trace_layout(uint32_t iters)
{
    TraceLayout t;
    t.idx = 0;
    t.ncand = t.idx + 20ull * iters;
    t.E = t.ncand + 4ull * iters;
    t.score = t.E + 360ull * iters;
    t.inliers = t.score + 40ull * iters;
    t.cheir = t.inliers + 40ull * iters;
    t.bytes = t.cheir + 40ull * iters;
    return t;
}

template <class T>
struct Strided {
    T* p;
    int s;
    NP_HD T& operator[](int i) const { return p[(long)i * s]; }
};

struct Pt4 {
    float x0, y0, x1, y1;  // frame 0's keypoint, frame 1's keypoint
};

// ------------------------------------------------------------------------------------------
// Sampling (:196-249): serial by nature, one generator for all iterations.  idx: 5 ints per
// iteration in ascending order (std::set's iteration order), or -1 five times for an iteration that
// found no five points in 100 tries (it has still consumed its draws).
// ------------------------------------------------------------------------------------------
template <class Points>
NP_HD void sample_indices(const Points& pts, uint32_t n, uint32_t iters, float min_sq, int32_t* idx)
{
    CvRng rng(12345);
    for (uint32_t it = 0; it < iters; it++) {
        // the set in draw order, every index written by a constant subscript (registers on the
        // device); sorted once it is complete
        int32_t set[5] = {-1, -1, -1, -1, -1};
        Pt4 sp[5] = {};
        int cnt = 0;
        for (int tries = 0; cnt < 5 && tries < 100; tries++) {
            const int c = rng.uniform(0, (int)n);
            const Pt4 pc = pts(c);
            bool close = false, have = false;
            MI_UNROLL
            for (int k = 0; k < 5; k++) {
                if (k >= cnt) continue;
                const float dx0 = sp[k].x0 - pc.x0, dy0 = sp[k].y0 - pc.y0;
                const float dx1 = sp[k].x1 - pc.x1, dy1 = sp[k].y1 - pc.y1;
                const float d0 = dx0 * dx0 + dy0 * dy0, d1 = dx1 * dx1 + dy1 * dy1;
                close = close || d0 < min_sq || d1 < min_sq;
                have = have || set[k] == c;
            }
            if (close || have) continue;  // a repeated index is a no-op insert
            MI_UNROLL
            for (int k = 0; k < 5; k++)
                if (k == cnt) {
                    set[k] = c;
                    sp[k] = pc;
                }
            cnt++;
        }
        MI_UNROLL
        for (int a = 0; a < 4; a++)
            MI_UNROLL
            for (int b = 0; b < 4 - a; b++)
                if (set[b] > set[b + 1]) {
                    const int32_t t = set[b];
                    set[b] = set[b + 1];
                    set[b + 1] = t;
                }
        for (int k = 0; k < 5; k++) idx[5 * it + k] = cnt == 5 ? set[k] : -1;
    }
}

// ------------------------------------------------------------------------------------------
// Polynomials in (x, y, z): linear over {x, y, z, 1}, quadratic over {x2, y2, z2, xy, xz, yz, x, y,
// z, 1}, cubic in Nister's order {x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1}.
// The product tables are built at compile time from the exponents.
// ------------------------------------------------------------------------------------------
struct MonoTables {
    int t11[4][4];   // linear x linear -> quadratic
    int t21[10][4];  // quadratic x linear -> cubic
    constexpr MonoTables() : t11{}, t21{}
    {
        const int e1[4][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
        const int e2[10][3] = {{2, 0, 0}, {0, 2, 0}, {0, 0, 2}, {1, 1, 0}, {1, 0, 1},
                               {0, 1, 1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
        const int e3[20][3] = {{3, 0, 0}, {0, 3, 0}, {2, 1, 0}, {1, 2, 0}, {2, 0, 1}, {2, 0, 0}, {0, 2, 1},
                               {0, 2, 0}, {1, 1, 1}, {1, 1, 0}, {1, 0, 2}, {1, 0, 1}, {1, 0, 0}, {0, 1, 2},
                               {0, 1, 1}, {0, 1, 0}, {0, 0, 3}, {0, 0, 2}, {0, 0, 1}, {0, 0, 0}};
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++)
                for (int q = 0; q < 10; q++)
                    if (e2[q][0] == e1[i][0] + e1[j][0] && e2[q][1] == e1[i][1] + e1[j][1] &&
                        e2[q][2] == e1[i][2] + e1[j][2])
                        t11[i][j] = q;
        for (int q = 0; q < 10; q++)
            for (int l = 0; l < 4; l++)
                for (int c = 0; c < 20; c++)
                    if (e3[c][0] == e2[q][0] + e1[l][0] && e3[c][1] == e2[q][1] + e1[l][1] &&
                        e3[c][2] == e2[q][2] + e1[l][2])
                        t21[q][l] = c;
    }
};

// o (quadratic) += or -= a * b, a and b linear; the terms in ascending (i, j).
template <bool SUB>
NP_HD void mul11(const double* a, const double* b, double* o)
{
    constexpr MonoTables T{};
MI_UNROLL
    for (int i = 0; i < 4; i++)
MI_UNROLL
        for (int j = 0; j < 4; j++) {
            const double v = a[i] * b[j];
            if (SUB)
                o[T.t11[i][j]] -= v;
            else
                o[T.t11[i][j]] += v;
        }
}

// o (cubic) += a * b, a quadratic and b linear; the terms in ascending (q, l).
NP_HD void mul21(const double* a, const double* b, double* o)
{
    constexpr MonoTables T{};
MI_UNROLL
    for (int q = 0; q < 10; q++)
MI_UNROLL
        for (int l = 0; l < 4; l++) o[T.t21[q][l]] += a[q] * b[l];
}

// The ten cubic constraints on E = xX + yY + zZ + W as a 10 x 20 float matrix: rows 0..8 are
// (E E^T - tr(E E^T) / 2) E entry by entry (half of 2 E E^T E - tr(E E^T) E), row 9 is det E.  e[k]
// holds entry k's {X, Y, Z, W} coefficients.  Computed in fp64, stored as float.
NP_HD void constraint_matrix(const double (&e)[9][4], const Strided<float>& A)
{
    double S[6][10];  // E E^T: 00 01 02 11 12 22
MI_UNROLL
    for (int s = 0; s < 6; s++) {
        const int i = s < 3 ? 0 : (s < 5 ? 1 : 2), j = s < 3 ? s : (s < 5 ? s - 2 : 2);
MI_UNROLL
        for (int m = 0; m < 10; m++) S[s][m] = 0.0;
MI_UNROLL
        for (int k = 0; k < 3; k++) mul11<false>(e[3 * i + k], e[3 * j + k], S[s]);
    }
MI_UNROLL
    for (int m = 0; m < 10; m++) {
        const double half = 0.5 * ((S[0][m] + S[3][m]) + S[5][m]);
        S[0][m] -= half;
        S[3][m] -= half;
        S[5][m] -= half;
    }
MI_UNROLL
    for (int i = 0; i < 3; i++)
MI_UNROLL
        for (int j = 0; j < 3; j++) {
            double c[20];
MI_UNROLL
            for (int m = 0; m < 20; m++) c[m] = 0.0;
MI_UNROLL
            for (int k = 0; k < 3; k++) {
                const int lo = i < k ? i : k, hi = i < k ? k : i;
                const int s = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
                mul21(S[s], e[3 * k + j], c);
            }
MI_UNROLL
            for (int m = 0; m < 20; m++) A[(3 * i + j) * 20 + m] = (float)c[m];
        }
    // det E = e0 (e4 e8 - e5 e7) + e1 (e5 e6 - e3 e8) + e2 (e3 e7 - e4 e6)
    double c[20];
MI_UNROLL
    for (int m = 0; m < 20; m++) c[m] = 0.0;
    const int co[3][4] = {{4, 8, 5, 7}, {5, 6, 3, 8}, {3, 7, 4, 6}};
MI_UNROLL
    for (int t = 0; t < 3; t++) {
        double q[10];
MI_UNROLL
        for (int m = 0; m < 10; m++) q[m] = 0.0;
        mul11<false>(e[co[t][0]], e[co[t][1]], q);
        mul11<true>(e[co[t][2]], e[co[t][3]], q);
        mul21(q, e[t], c);
    }
MI_UNROLL
    for (int m = 0; m < 20; m++) A[9 * 20 + m] = (float)c[m];
}

// A2 = inv(left) * right in float, in place: Gauss-Jordan with partial pivoting (the first row of
// the largest magnitude).  false when a pivot is zero or not finite: no solutions.
NP_HD bool gauss_jordan_10x20(const Strided<float>& A)
{
    for (int c = 0; c < 10; c++) {
        int pr = c;
        float best = fabsf(A[c * 20 + c]);
        for (int r = c + 1; r < 10; r++) {
            const float v = fabsf(A[r * 20 + c]);
            if (v > best) {
                best = v;
                pr = r;
            }
        }
        if (!(best > 0.f) || !(best <= FLT_MAX)) return false;
        if (pr != c)
            for (int m = 0; m < 20; m++) {
                const float t = A[c * 20 + m];
                A[c * 20 + m] = A[pr * 20 + m];
                A[pr * 20 + m] = t;
            }
        const float piv = A[c * 20 + c];
        for (int m = 0; m < 20; m++) A[c * 20 + m] = A[c * 20 + m] / piv;
        for (int r = 0; r < 10; r++) {
            if (r == c) continue;
            const float f = A[r * 20 + c];
            if (f == 0.f) continue;
            for (int m = 0; m < 20; m++) A[r * 20 + m] = A[r * 20 + m] - f * A[c * 20 + m];
        }
    }
    return true;
}

// An orthonormal basis of the null space of the 5 x 9 matrix in rows 0..4 of B (9 x 9, row-major),
// left in rows 5..8, as the orthogonal complement of the row space: the rows are orthonormalised
// (modified Gram-Schmidt, two passes; a row that vanishes to 1e-24 of its length is dropped), then
// four times the unit vector e_j with the largest remainder outside the span so far (the first on
// ties) is projected, re-projected and normalised; last, the four are mixed (see below).
NP_HD void null_space_basis(const Strided<double>& B)
{
    for (int k = 0; k < 9; k++) {
        if (k >= 5) {
            int bj = 0;
            double br = -1.0;
            for (int j = 0; j < 9; j++) {
                double r = 1.0;
                for (int i = 0; i < k; i++) r -= B[i * 9 + j] * B[i * 9 + j];
                if (r > br) {
                    br = r;
                    bj = j;
                }
            }
            for (int m = 0; m < 9; m++) B[k * 9 + m] = m == bj ? 1.0 : 0.0;
        }
        double n0 = 0.0;
        for (int m = 0; m < 9; m++) n0 += B[k * 9 + m] * B[k * 9 + m];
        for (int pass = 0; pass < 2; pass++)
            for (int i = 0; i < k; i++) {
                double d = 0.0;
                for (int m = 0; m < 9; m++) d += B[i * 9 + m] * B[k * 9 + m];
                for (int m = 0; m < 9; m++) B[k * 9 + m] -= d * B[i * 9 + m];
            }
        double n1 = 0.0;
        for (int m = 0; m < 9; m++) n1 += B[k * 9 + m] * B[k * 9 + m];
        if (n1 > n0 * 1e-24) {
            const double inv = 1.0 / sqrt(n1);
            for (int m = 0; m < 9; m++) B[k * 9 + m] *= inv;
        } else {
            for (int m = 0; m < 9; m++) B[k * 9 + m] = 0.0;
        }
    }
    // the four vectors so far each lean on one coordinate axis, which conditions the elimination
    // several times worse than a generic basis of the same space: mix them with the orthogonal
    // 4 x 4 Hadamard matrix / 2 (exact scaling, still orthonormal)
    for (int m = 0; m < 9; m++) {
        const double a = B[45 + m], b = B[54 + m], c = B[63 + m], d = B[72 + m];
        B[45 + m] = ((a + b) + (c + d)) * 0.5;
        B[54 + m] = ((a - b) + (c - d)) * 0.5;
        B[63 + m] = ((a + b) - (c + d)) * 0.5;
        B[72 + m] = ((a - b) - (c - d)) * 0.5;
    }
}

// Durand-Kerner (ComputeEssential.cpp:307-348) on c[0..10] (ascending powers), complex arithmetic
// written out as cv::Complex<double> computes it.  W: c at [0..10] on entry, roots at [11 + 2i],
// [12 + 2i] on exit.  Returns the number of roots (the degree left after dropping leading
// coefficients with |re| + |im| <= DBL_EPSILON).
NP_HD int durand_kerner(const Strided<double>& W)
{
    int n = 10;
    for (; n > 1; n--)
        if (fabs(W[n]) + 0.0 > DBL_EPSILON) break;
    double pre = 1.0, pim = 0.0;
    for (int i = 0; i < n; i++) {
        W[11 + 2 * i] = pre;
        W[12 + 2 * i] = pim;
        const double re = pre * 1.0 - pim * 1.0, im = pre * 1.0 + pim * 1.0;
        pre = re;
        pim = im;
    }
    for (int iter = 0; iter < 100; iter++) {
        double max_diff = 0.0;
        for (int i = 0; i < n; i++) {
            pre = W[11 + 2 * i];
            pim = W[12 + 2 * i];
            double nre = W[n], nim = 0.0, dre = W[n], dim = 0.0;
            for (int j = 0; j < n; j++) {
                const double tre = nre * pre - nim * pim, tim = nre * pim + nim * pre;
                nre = tre + W[n - j - 1];
                nim = tim + 0.0;
                if (j != i) {
                    const double qre = pre - W[11 + 2 * j], qim = pim - W[12 + 2 * j];
                    const double ure = dre * qre - dim * qim, uim = dre * qim + dim * qre;
                    dre = ure;
                    dim = uim;
                }
            }
            const double t = 1.0 / (dre * dre + dim * dim);
            const double qre = (nre * dre + nim * dim) * t, qim = (-nre * dim + nim * dre) * t;
            W[11 + 2 * i] = pre - qre;
            W[12 + 2 * i] = pim - qim;
            const double a = sqrt(qre * qre + qim * qim);
            if (a > max_diff) max_diff = a;
        }
        if (max_diff <= 1e-6) break;
    }
    for (int i = 0; i < n; i++)
        if (fabs(W[12 + 2 * i]) < 1e-100) W[12 + 2 * i] = 0.0;
    return n;
}

// c (ascending, length la + lb - 1) += or -= a * b over Strided / plain arrays.
template <bool SUB, class TA, class TB, class TC>
NP_HD void poly_mul_acc(const TA& a, int la, const TB& b, int lb, const TC& c)
{
    for (int i = 0; i < la; i++)
        for (int j = 0; j < lb; j++) {
            const double v = (double)a[i] * (double)b[j];
            if (SUB)
                c[i + j] = c[i + j] - v;
            else
                c[i + j] = c[i + j] + v;
        }
}

template <class T>
struct Offset {
    Strided<T> s;
    int o;
    NP_HD T& operator[](int i) const { return s[o + i]; }
};

// One hypothesis (ComputeEssential.cpp:357-514): the five matches' points -> up to ten essential
// matrices, row-major floats at E[9 r .. 9 r + 8] in root order; slots past the count are zeroed.
// pp / focal are frame 0's for both frames, as the reference passes them (:252).  D: MI_WORK_D
// doubles, A: MI_WORK_A floats of workspace.
NP_HD int solve_five_point(const Pt4* p5, float ppx, float ppy, float fx, float fy, const Strided<double>& D,
                           const Strided<float>& A, float* E)
{
    for (int k = 0; k < 90; k++) E[k] = 0.f;
    const double ifx = fx != 0 ? 1. / fx : 1., ify = fy != 0 ? 1. / fy : 1.;
    for (int i = 0; i < 5; i++) {
        const double x1 = ((double)p5[i].x0 - ppx) * ifx, y1 = ((double)p5[i].y0 - ppy) * ify;
        const double x2 = ((double)p5[i].x1 - ppx) * ifx, y2 = ((double)p5[i].y1 - ppy) * ify;
        D[i * 9 + 0] = x1 * x2;
        D[i * 9 + 1] = y1 * x2;
        D[i * 9 + 2] = x2 * 1.0;
        D[i * 9 + 3] = x1 * y2;
        D[i * 9 + 4] = y1 * y2;
        D[i * 9 + 5] = y2 * 1.0;
        D[i * 9 + 6] = x1 * 1.0;
        D[i * 9 + 7] = y1 * 1.0;
        D[i * 9 + 8] = 1.0;
    }
    null_space_basis(D);
    {
        double e[9][4];
MI_UNROLL
        for (int k = 0; k < 9; k++)
MI_UNROLL
            for (int b = 0; b < 4; b++) e[k][b] = D[(5 + b) * 9 + k];
        constraint_matrix(e, A);
    }
    if (!gauss_jordan_10x20(A)) return 0;
    // B(z): row i = (row 4 + 2i) - z (row 5 + 2i) of A2, grouped by x, y, 1: ascending coefficients
    // in float at A[13 i + {0..3, 4..7, 8..12}] (rows 0 and 1 of A are dead; rows 4..9 start at 80)
    for (int i = 0; i < 3; i++) {
        const int r4 = (4 + 2 * i) * 20 + 10, r5 = (5 + 2 * i) * 20 + 10;
        for (int g = 0; g < 3; g++) {
            const int len = g < 2 ? 3 : 4, src = 3 * g, dst = 13 * i + 4 * g;
            for (int k = 0; k <= len; k++) {
                const float lo = k < len ? A[r4 + src + (len - 1 - k)] : 0.f;  // z^k of row 4 + 2i
                const float hi = k > 0 ? A[r5 + src + (len - k)] : 0.f;        // z^(k-1) of row 5 + 2i
                A[dst + k] = lo - hi;
            }
        }
    }
    // det B(z), degree 10, in fp64 by polynomial multiplication: c at D[0..10], a 2 x 2 minor
    // (degree 7) at D[31..38]; rows 0..4 of D are dead, the basis stays in rows 5..8
    for (int k = 0; k < 11; k++) D[k] = 0.0;
    const Offset<double> c{D, 0}, t{D, 31};
    for (int g = 0; g < 3; g++) {
        // cofactor of column g in row 0 from rows 1 and 2: columns (u, v) = the other two
        const int u = g == 0 ? 1 : 0, v = g == 2 ? 1 : 2;
        const int lu = u < 2 ? 4 : 5, lv = v < 2 ? 4 : 5, lg = g < 2 ? 4 : 5;
        for (int k = 0; k < 8; k++) t[k] = 0.0;
        poly_mul_acc<false>(Offset<float>{A, 13 + 4 * u}, lu, Offset<float>{A, 26 + 4 * v}, lv, t);
        poly_mul_acc<true>(Offset<float>{A, 13 + 4 * v}, lv, Offset<float>{A, 26 + 4 * u}, lu, t);
        if (g == 1)
            poly_mul_acc<true>(Offset<float>{A, 4 * g}, lg, t, lu + lv - 1, c);
        else
            poly_mul_acc<false>(Offset<float>{A, 4 * g}, lg, t, lu + lv - 1, c);
    }
    const int nroots = durand_kerner(D);
    int count = 0;
    for (int i = 0; i < nroots; i++) {
        if (!(fabs(D[12 + 2 * i]) <= 1e-6)) continue;
        const float z1 = (float)D[11 + 2 * i];
        const float z2 = z1 * z1, z3 = z2 * z1, z4 = z3 * z1;
        float bz[3][3];
MI_UNROLL
        for (int j = 0; j < 3; j++) {
            const int o = 13 * j;
            bz[j][0] = A[o + 3] * z3 + A[o + 2] * z2 + A[o + 1] * z1 + A[o + 0];
            bz[j][1] = A[o + 7] * z3 + A[o + 6] * z2 + A[o + 5] * z1 + A[o + 4];
            bz[j][2] = A[o + 12] * z4 + A[o + 11] * z3 + A[o + 10] * z2 + A[o + 9] * z1 + A[o + 8];
        }
        // the null vector of B(z): of the row cross products 0x1, 0x2, 1x2 the longest (the first on ties)
        float v[3] = {0.f, 0.f, 0.f}, best = -1.f;
MI_UNROLL
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const float cx = bz[p][1] * bz[q][2] - bz[p][2] * bz[q][1];
            const float cy = bz[p][2] * bz[q][0] - bz[p][0] * bz[q][2];
            const float cz = bz[p][0] * bz[q][1] - bz[p][1] * bz[q][0];
            const float n = (cx * cx + cy * cy) + cz * cz;
            if (n > best) {
                best = n;
                v[0] = cx;
                v[1] = cy;
                v[2] = cz;
            }
        }
        if (fabs((double)v[2]) < 1e-10) continue;
        const float x = v[0] / v[2], y = v[1] / v[2];
        double ev[9], nn = 0.0;
MI_UNROLL
        for (int k = 0; k < 9; k++) {
            ev[k] = ((D[45 + k] * (double)x + D[54 + k] * (double)y) + D[63 + k] * (double)z1) + D[72 + k];
            nn += ev[k] * ev[k];
        }
        const double norm = sqrt(nn);
MI_UNROLL
        for (int k = 0; k < 9; k++) E[9 * count + k] = (float)(ev[k] / norm);
        count++;
    }
    return count;
}

// ------------------------------------------------------------------------------------------
// Scoring (:259-261, :279-322)
// ------------------------------------------------------------------------------------------
// F12 = K2inv^T * E * K1inv in cv::Matx order; F21 is its transpose.
NP_HD void fundamental_from_essential(const float* E, const float* k1inv, const float* k2inv, float* F12, float* F21)
{
    float k2t[9], m[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) k2t[i * 3 + j] = k2inv[j * 3 + i];
    mat3_mul(k2t, E, m);
    mat3_mul(m, k1inv, F12);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) F21[i * 3 + j] = F12[j * 3 + i];
}

// ComputePerpDistanceSquared (:38-52) of the point (x, y) from the line F * (lx, ly, 1).
NP_HD float perp_distance_sq(const float* F, float lx, float ly, float x, float y)
{
    const float l[3] = {lx, ly, 1.f};
    const float a = dot3(F, l), b = dot3(F + 3, l), c = dot3(F + 6, l);
    const float num = (a * x + b * y) + c;
    const float den = a * a + b * b;
    return num * num / den;
}

struct ScoreState {
    float sum;
    uint32_t inliers;
};

NP_HD void score_match(const float* F12, const float* F21, float thr, const Pt4& p, ScoreState& s)
{
    const float d12 = perp_distance_sq(F12, p.x0, p.y0, p.x1, p.y1);
    const float d21 = perp_distance_sq(F21, p.x1, p.y1, p.x0, p.y0);
    if (d12 < thr && d21 < thr) {
        s.sum += thr - d12;
        s.sum += thr - d21;
        s.inliers++;
    }
}

NP_HD float score_gate(const Consts& c, const ScoreState& s, uint32_t n)
{
    return s.inliers >= c.min_inliers && (float)s.inliers / (float)n > c.min_pct ? s.sum : 0.f;
}

// ------------------------------------------------------------------------------------------
// Pose candidates (:85-114): cv::decomposeEssentialMat's semantics in fp64.  The SVD E = U S V^T
// comes from cyclic Jacobi on E^T E (12 sweeps at most): V's columns by descending eigenvalue with
// v3 = v1 x v2 (det V = +1), u_i = E v_i normalised for the two large singular values and u3 = u1 x
// u2 (det U = +1, the reference's sign fixes).  R1 = U W V^T, R2 = U W^T V^T, t = u3.  Poses in the
// reference's order {tn, R1}, {-tn, R1}, {t, R2}, {-tn, R2}: the third takes t un-normalised.
// pos3: 4 x 3 view-space translations, r9: 4 x 9 column-major rotations.
// ------------------------------------------------------------------------------------------
NP_HD void jacobi_eigen3(double (&a)[3][3], double (&v)[3][3])
{
MI_UNROLL
    for (int i = 0; i < 3; i++)
MI_UNROLL
        for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; sweep++) {
        if (fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]) == 0.0) break;
MI_UNROLL
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double at = fabs(theta) + sqrt(theta * theta + 1.0);
            const double t = theta < 0.0 ? -1.0 / at : 1.0 / at;
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            const int r = 3 - p - q;
            const double arp = a[r][p], arq = a[r][q];
            a[p][p] = a[p][p] - t * apq;
            a[q][q] = a[q][q] + t * apq;
            a[p][q] = a[q][p] = 0.0;
            a[r][p] = a[p][r] = c * arp - s * arq;
            a[r][q] = a[q][r] = s * arp + c * arq;
MI_UNROLL
            for (int k = 0; k < 3; k++) {
                const double vp = v[k][p], vq = v[k][q];
                v[k][p] = c * vp - s * vq;
                v[k][q] = s * vp + c * vq;
            }
        }
    }
}

NP_HD void cross3d(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

NP_HD void decompose_poses(const float* Ef, float* pos3, float* r9)
{
    double E[3][3], a[3][3], v[3][3];
MI_UNROLL
    for (int i = 0; i < 3; i++)
MI_UNROLL
        for (int j = 0; j < 3; j++) E[i][j] = (double)Ef[3 * i + j];
MI_UNROLL
    for (int i = 0; i < 3; i++)
MI_UNROLL
        for (int j = 0; j < 3; j++) a[i][j] = (E[0][i] * E[0][j] + E[1][i] * E[1][j]) + E[2][i] * E[2][j];
    jacobi_eigen3(a, v);
    // the two largest eigenvalues' columns, the larger first (the lower column on ties); picked by
    // selects, so that no array is indexed by a runtime value
    const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
    int i0 = 0;
    double m0 = d0;
    if (d1 > m0) {
        i0 = 1;
        m0 = d1;
    }
    if (d2 > m0) i0 = 2;
    const int i1 = i0 == 0 ? (d2 > d1 ? 2 : 1) : (i0 == 1 ? (d2 > d0 ? 2 : 0) : (d1 > d0 ? 1 : 0));
    double V[3][3], U[3][3];  // columns as rows: V[c] is column c
MI_UNROLL
    for (int k = 0; k < 3; k++) {
        V[0][k] = i0 == 0 ? v[k][0] : (i0 == 1 ? v[k][1] : v[k][2]);
        V[1][k] = i1 == 0 ? v[k][0] : (i1 == 1 ? v[k][1] : v[k][2]);
    }
    cross3d(V[0], V[1], V[2]);
MI_UNROLL
    for (int c = 0; c < 2; c++) {
        double n = 0.0;
MI_UNROLL
        for (int i = 0; i < 3; i++) {
            U[c][i] = (E[i][0] * V[c][0] + E[i][1] * V[c][1]) + E[i][2] * V[c][2];
            n += U[c][i] * U[c][i];
        }
        n = sqrt(n);
MI_UNROLL
        for (int i = 0; i < 3; i++) U[c][i] = U[c][i] / n;
    }
    cross3d(U[0], U[1], U[2]);
    // U W V^T = -u2 v1^T + u1 v2^T + u3 v3^T;  U W^T V^T = u2 v1^T - u1 v2^T + u3 v3^T
    float R1[9], R2[9], T[3];
MI_UNROLL
    for (int i = 0; i < 3; i++) {
MI_UNROLL
        for (int j = 0; j < 3; j++) {
            const double m = U[0][i] * V[1][j] - U[1][i] * V[0][j], w = U[2][i] * V[2][j];
            R1[3 * i + j] = (float)(m + w);
            R2[3 * i + j] = (float)(w - m);
        }
        T[i] = (float)U[2][i];
    }
    const float tn = sqrtf(dot3(T, T));
MI_UNROLL
    for (int p = 0; p < 4; p++) {
        const float* R = p < 2 ? R1 : R2;
MI_UNROLL
        for (int i = 0; i < 3; i++) {
            pos3[3 * p + i] = p == 2 ? T[i] : (p == 0 ? T[i] / tn : -1.f * (T[i] / tn));
MI_UNROLL
            for (int j = 0; j < 3; j++) r9[9 * p + j * 3 + i] = R[3 * i + j];
        }
    }
}

// ------------------------------------------------------------------------------------------
// Cheirality (:129-179) on the hypothesis's own five points, frame 0 at the identity.
// ------------------------------------------------------------------------------------------
NP_HD void identity_frame(const float* intr4, Frame& f)
{
    const float z3[3] = {0.f, 0.f, 0.f}, eye[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    newpoints::make_frame(z3, eye, intr4, f);
}

NP_HD bool consistent_cheirality(const float* pos3, const float* r9, const Frame& f0, const float* intr1, const Pt4* p5)
{
    bool found = false;
    float t[3] = {0.f, 0.f, 0.f}, r[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    MI_UNROLL
    for (int p = 3; p >= 0; p--)
        if (r9[9 * p] > 0.f) {  // GetWorldSpaceRight()[0] is R(0, 0); the lowest such pose is kept
            found = true;
            MI_UNROLL
            for (int k = 0; k < 3; k++) t[k] = pos3[3 * p + k];
            MI_UNROLL
            for (int k = 0; k < 9; k++) r[k] = r9[9 * p + k];
        }
    if (!found) return false;
    Frame f1;
    newpoints::make_frame(t, r, intr1, f1);
    const float fwd0[3] = {f0.Rt[2], f0.Rt[5], f0.Rt[8]}, fwd1[3] = {f1.Rt[2], f1.Rt[5], f1.Rt[8]};
    int consensus = 1;
    bool ok = true;
    MI_UNROLL
    for (int i = 0; i < 5; i++) {
        float X[3];
        bool parallel;
        newpoints::triangulate(f0, f1, p5[i].x0, p5[i].y0, p5[i].x1, p5[i].y1, X, parallel);
        const float a[3] = {X[0] - f0.C[0], X[1] - f0.C[1], X[2] - f0.C[2]};
        const float b[3] = {X[0] - f1.C[0], X[1] - f1.C[1], X[2] - f1.C[2]};
        const float d0 = dot3(fwd0, a), d1 = dot3(fwd1, b);
        if (i == 0) {
            if (d0 <= 0.f || d1 <= 0.f) consensus = -1;
        } else if ((float)consensus * d0 <= 0.f || (float)consensus * d1 <= 0.f) {
            ok = false;
        }
    }
    return ok;
}

// ------------------------------------------------------------------------------------------
// FindCorrectPose (:324-480)
// ------------------------------------------------------------------------------------------
struct PoseEval {
    Frame f1;
    float F01[9], F10[9];  // ComputeFundamentalMatrix(reference -> pose), (pose -> reference)
    float scale;           // 1 / |C|^2
    bool twisted;
};

NP_HD void prepare_pose(const Frame& f0, const float* pos3, const float* r9, const float* intr1, PoseEval& e)
{
    newpoints::make_frame(pos3, r9, intr1, e.f1);
    const float right1[3] = {e.f1.Rt[0], e.f1.Rt[3], e.f1.Rt[6]}, right0[3] = {f0.Rt[0], f0.Rt[3], f0.Rt[6]};
    e.twisted = dot3(right1, right0) <= 0.f;
    newpoints::fundamental(f0, e.f1, e.F01);
    newpoints::fundamental(e.f1, f0, e.F10);
    e.scale = 1.0f / dot3(e.f1.C, e.f1.C);
}

// One match against one pose: the score term (> 0) when accepted with the point in X, else 0.
NP_HD float eval_match(const Consts& c, const Frame& f0, const PoseEval& e, const Pt4& p, float* X, bool& parallel)
{
    newpoints::triangulate(f0, e.f1, p.x0, p.y0, p.x1, p.y1, X, parallel);
    if (X[2] < 0.f) return 0.f;
    if (X[2] * e.scale > c.max_dist) return 0.f;
    const float a = newpoints::epipolar_distance(e.F01, p.x0, p.y0, p.x1, p.y1);
    const float b = newpoints::epipolar_distance(e.F10, p.x1, p.y1, p.x0, p.y0);
    const float temp = b + a;
    if (temp < c.two_max_epi) return c.two_max_epi - temp;
    return 0.f;
}

NP_HD uint32_t pose_gate(const Consts& c, uint32_t count, uint32_t n)
{
    return count >= c.min_inliers && (float)count / (float)n > c.min_pct ? MI_POSE_ENOUGH : 0u;
}

// The best / next-best bookkeeping in pose order and the three final rejections (:435-472).
// flags / score / median per pose; cz the selected pose's world-space position z.
NP_HD uint32_t final_verdict(const Consts& c, const uint32_t* flags, const float* score, const float* cam_z,
                             int32_t& selected, float& next_best)
{
    float sel_score = 0.f;
    next_best = 0.f;
    selected = -1;
    for (int p = 0; p < 4; p++) {
        if ((flags[p] & (MI_POSE_TWISTED | MI_POSE_ENOUGH | MI_POSE_MEDIAN_OK)) != (MI_POSE_ENOUGH | MI_POSE_MEDIAN_OK))
            continue;
        if (selected == -1 || score[p] > sel_score) {
            next_best = sel_score;
            sel_score = score[p];
            selected = p;
        } else if (score[p] > next_best) {
            next_best = score[p];
        }
    }
    if (sel_score <= 0.f) return MI_NO_VALID_POSE;
    const float ratio = (sel_score - next_best) / sel_score;
    if (ratio < c.min_dissim) return MI_TOO_SIMILAR;
    if (fabsf(cam_z[selected]) > c.max_z) return MI_Z_BIASED;
    return MI_OK;
}

// The keys of the median's sort: an order-preserving map of a float to 32 bits.
NP_HD uint32_t float_order_key(float z)
{
    union {
        float f;
        uint32_t u;
    } b;
    b.f = z;
    return (b.u & 0x80000000u) ? ~b.u : (b.u | 0x80000000u);
}

}  // namespace monoinit
}  // namespace mage
