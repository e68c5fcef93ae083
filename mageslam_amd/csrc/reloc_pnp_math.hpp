// reloc_pnp_math.hpp — PoseEstimator::PNPRansac (Tracking/PoseEstimator.cpp:610-638) as the
// relocalisation uses it (:219-437): cv::solvePnPRansac(SOLVEPNP_ITERATIVE) of OpenCV 3.4.0 restated
// — RANSACPointSetRegistrator::run's sampler, inlier rule and RANSACUpdateNumIters (ptsetreg.cpp),
// EPnP on five points (epnp.cpp, Lepetit / Moreno-Noguer / Fua) — then RemoveMapPointsThatAreBehind
// (:209-216) and the RansacInliersPctRequired gate (:339).  Shared by the kernels (reloc_pnp.hip)
// and their plain C++ twin (reloc_pnp.cpp).
//
// Only + - * /, sqrt and fabs appear here (the logarithm of the update is written out below), every
// sum is written in one fixed order, and both translation units are built with -ffp-contract=off,
// so host and gfx950 give the same bits.  The arrays that are indexed at run time (the packed
// 12 x 12 matrix, its eigenvectors, L) live behind Strided<double>: a plain array on the host,
// lane-interleaved LDS on the device; so do the five points, pixels and barycentric coordinates,
// which leaves the device's registers to the rest.  Everything else is indexed by unrolled loops.
#pragma once

#include <float.h>

#include "cv_rng.hpp"
#include "monoinit_math.hpp"

#if defined(__clang__)
#define RP_NOUNROLL _Pragma("clang loop unroll(disable)")
#else
#define RP_NOUNROLL
#endif

namespace mage {
namespace relocpnp {

using monoinit::Strided;

constexpr int RP_MAX_MATCHES = 4096;  // matches per problem
constexpr int RP_MAX_ITERS = 256;     // RansacIterations
constexpr int RP_WORK_D = 78 + 144 + 45;  // doubles of per-hypothesis workspace: packed M^T M (then L), eigenvectors, points
constexpr int RP_JACOBI_SWEEPS = 30;  // sweep limit of the 12 x 12 eigenproblem
constexpr int RP_MAX_REDRAWS = 4096;  // draws one sample may take (OpenCV has no bound; n >= 6 needs a handful)

enum : uint32_t {
    RP_OK = MAGE_RP_OK,
    RP_FEW_MATCHES = MAGE_RP_FEW_MATCHES,
    RP_NO_MODEL = MAGE_RP_NO_MODEL,
    RP_FEW_INLIERS = MAGE_RP_FEW_INLIERS,
};
enum : uint32_t {
    RP_STATUS_OVER_LIMIT = MAGE_RP_STATUS_OVER_LIMIT,
    RP_STATUS_OVER_CAP = MAGE_RP_STATUS_OVER_CAP,
    RP_STATUS_BAD_INDEX = MAGE_RP_STATUS_BAD_INDEX,
};

// nullptr when the settings can be used, else what is wrong with them (MAGE_EINVAL).
inline const char* check_settings(const mage_reloc_settings* s)
{
    if (!s) return "null settings";
    if (s->struct_size != sizeof(mage_reloc_settings)) return "struct_size is not sizeof(mage_reloc_settings)";
    if (!(s->ransac_confidence > 0.f) || !(s->ransac_confidence < 1.f)) return "ransac_confidence must be in (0, 1)";
    if (s->ransac_iterations < 1 || s->ransac_iterations > (uint32_t)RP_MAX_ITERS) return "ransac_iterations must be in 1..256";
    if (!(s->ransac_inliers_pct_required >= 0.f)) return "ransac_inliers_pct_required must be >= 0";
    if (!(s->max_bundle_pnp_reprojection_error >= 0.f) || !(s->max_bundle_pnp_reprojection_error <= FLT_MAX))
        return "max_bundle_pnp_reprojection_error must be finite and >= 0";
    return nullptr;
}

// The settings as the loops read them.
struct Consts {
    double confidence;   // RansacConfidence
    float thr_sq;        // (float)(MaxBundlePnPReprojectionError^2), the square taken in double (findInliers)
    float min_pct;       // RansacInliersPctRequired
    uint32_t min_matches, iters;
};

inline Consts make_consts(const mage_reloc_settings& s)
{
    Consts c{};
    c.confidence = (double)s.ransac_confidence;
    const double t = (double)s.max_bundle_pnp_reprojection_error;
    c.thr_sq = (float)(t * t);
    c.min_pct = s.ransac_inliers_pct_required;
    c.min_matches = s.min_brute_force_correspondences;
    c.iters = s.ransac_iterations;
    return c;
}

// One gathered correspondence (32 bytes): the candidate's map point with its information value,
// the current frame's keypoint, the match's indices.
struct Corr {
    float x, y, z, info, u, v;
    int32_t query_idx, train_idx;
};

// The trace / work buffer of one problem, `iters` RANSAC iterations (see mage_hot.h): offsets in bytes.
struct TraceLayout {
    size_t R, t, err, idx, solved, count, bytes;
};
NP_HD TraceLayout trace_layout(uint32_t iters)
{
    TraceLayout L;
    L.R = 0;
    L.t = L.R + 72ull * iters;
    L.err = L.t + 24ull * iters;
    L.idx = L.err + 24ull * iters;
    L.solved = L.idx + 20ull * iters;
    L.count = L.solved + 4ull * iters;
    L.bytes = (L.count + 4ull * iters + 7ull) & ~7ull;
    return L;
}

struct Trace {
    double *R, *t, *err;
    int32_t *idx, *solved;
    uint32_t* count;
};
NP_HD Trace trace_at(char* b, const TraceLayout& L)
{
    return Trace{reinterpret_cast<double*>(b + L.R),    reinterpret_cast<double*>(b + L.t),
                 reinterpret_cast<double*>(b + L.err),  reinterpret_cast<int32_t*>(b + L.idx),
                 reinterpret_cast<int32_t*>(b + L.solved), reinterpret_cast<uint32_t*>(b + L.count)};
}

// ------------------------------------------------------------------------------------------
// Sampling (RANSACPointSetRegistrator::getSubset): cv::RNG(2^64 - 1), five uniform(0, n) draws per
// iteration, a draw equal to an earlier index of the same sample redrawn, the indices kept in draw
// order.  The draws depend on n alone: one serial generator for all iterations.  n > 5.
// ------------------------------------------------------------------------------------------
NP_HD void sample_indices(uint32_t n, uint32_t iters, int32_t* idx)
{
    CvRng rng(0xffffffffffffffffull);
    for (uint32_t it = 0; it < iters; it++) {
        int32_t set[5] = {-1, -1, -1, -1, -1};
        int cnt = 0;
        for (int tries = 0; cnt < 5 && tries < RP_MAX_REDRAWS; tries++) {
            const int c = rng.uniform(0, (int)n);
            bool have = false;
            MI_UNROLL
            for (int k = 0; k < 5; k++) have = have || (k < cnt && set[k] == c);
            if (have) continue;
            MI_UNROLL
            for (int k = 0; k < 5; k++)
                if (k == cnt) set[k] = c;
            cnt++;
        }
        MI_UNROLL
        for (int k = 0; k < 5; k++) idx[5 * it + k] = cnt == 5 ? set[k] : -1;
    }
}

// ------------------------------------------------------------------------------------------
// RANSACUpdateNumIters (ptsetreg.cpp): the logarithm written out — exponent by bit operations, the
// mantissa folded into [sqrt(1/2), sqrt(2)), log m = 2 atanh((m - 1) / (m + 1)) by its series to
// s^23 (|s| <= 0.1716: the first dropped term is below 1e-20).  Not correctly rounded; good to a
// few ulp, which leaves the rounded quotient below equal to the libm formula's.
// ------------------------------------------------------------------------------------------
NP_HD double log_pos(double x)  // x > 0, finite, normal
{
    union {
        double d;
        uint64_t u;
    } b;
    b.d = x;
    int e = (int)((b.u >> 52) & 0x7ffull) - 1023;
    b.u = (b.u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m = b.d;  // [1, 2)
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        e = e + 1;
    }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    return (double)e * 0.6931471805599453 + 2.0 * s * p;
}

NP_HD int update_num_iters(double p, double ep, int max_iters)
{
    p = p > 0.0 ? p : 0.0;
    p = p < 1.0 ? p : 1.0;
    ep = ep > 0.0 ? ep : 0.0;
    ep = ep < 1.0 ? ep : 1.0;
    double num = 1.0 - p > DBL_MIN ? 1.0 - p : DBL_MIN;
    const double q = 1.0 - ep;
    double denom = 1.0 - (((q * q) * q) * q) * q;
    if (denom < DBL_MIN) return 0;
    num = log_pos(num);
    denom = log_pos(denom);
    if (denom >= 0.0 || -num >= (double)max_iters * (-denom)) return max_iters;
    // cvRound: to nearest, ties to even; 0 <= v < max_iters here
    const double v = num / denom;
    int k = (int)(v + 0.5);
    if ((double)k - v == 0.5 && (k & 1)) k--;
    return k;
}

// What the adaptive loop of run() leaves.
struct LoopResult {
    int32_t win;        // the best hypothesis's iteration, or -1
    uint32_t best;      // its inlier count (maxGoodCount)
    uint32_t niters;    // the final niters
    uint32_t run;       // iterations the loop went through
};

// The loop replayed over all hypotheses' outcomes: solved[i] != 0 when iteration i has a model,
// count[i] its inlier count, sampled[i] != 0 when it has a sample at all (getSubset's failure ends
// the loop).  With adaptive == false (n == 5) no update is made.
NP_HD LoopResult replay_loop(const int32_t* first_idx, const int32_t* solved, const uint32_t* count, uint32_t max_iters,
                             uint32_t n, double confidence, bool adaptive)
{
    LoopResult r{-1, 0u, max_iters > 1u ? max_iters : 1u, 0u};
    if (!adaptive) r.niters = 1u;
    uint32_t it = 0;
    for (; it < r.niters; it++) {
        if (first_idx[5 * it] < 0) break;
        if (!solved[it]) continue;
        const uint32_t good = count[it];
        if (good > (r.best > 4u ? r.best : 4u)) {
            r.best = good;
            r.win = (int32_t)it;
            if (adaptive) r.niters = (uint32_t)update_num_iters(confidence, (double)(n - good) / (double)n, (int)r.niters);
        }
    }
    r.run = it;
    return r;
}

// ------------------------------------------------------------------------------------------
// Small dense pieces
// ------------------------------------------------------------------------------------------
NP_HD bool finite_d(double v) { return fabs(v) <= DBL_MAX; }

// Column k (by selects) of a 3 x 3 array.
NP_HD double pick3(const double (&v)[3][3], int row, int k) { return k == 0 ? v[row][0] : (k == 1 ? v[row][1] : v[row][2]); }

// The sign rule of every eigenvector here: its component of the largest magnitude (the first on
// ties) is positive.
NP_HD void sign_rule3(double* v)
{
    double big = v[0];
    if (fabs(v[1]) > fabs(big)) big = v[1];
    if (fabs(v[2]) > fabs(big)) big = v[2];
    if (big < 0.0) {
        v[0] = -v[0];
        v[1] = -v[1];
        v[2] = -v[2];
    }
}

// The eigenvalues' order: i0 the largest (the lower column on ties), i2 the smallest, i1 the other.
NP_HD void order3(double d0, double d1, double d2, int& i0, int& i1, int& i2)
{
    i0 = 0;
    double m0 = d0;
    if (d1 > m0) {
        i0 = 1;
        m0 = d1;
    }
    if (d2 > m0) i0 = 2;
    i1 = i0 == 0 ? (d2 > d1 ? 2 : 1) : (i0 == 1 ? (d2 > d0 ? 2 : 0) : (d1 > d0 ? 1 : 0));
    i2 = 3 - i0 - i1;
}

// Least squares min |A x - b| for a 6 x N matrix by Householder QR (epnp.cpp's qr_solve in spirit;
// A and b are destroyed).  false on a zero column or a non-finite result.
template <int N>
NP_HD bool qr_lsq(double (&A)[6][N], double (&b)[6], double (&x)[N])
{
    bool ok = true;
    MI_UNROLL
    for (int k = 0; k < N; k++) {
        double sigma = 0.0;
        MI_UNROLL
        for (int i = k; i < 6; i++) sigma += A[i][k] * A[i][k];
        if (!(sigma > 0.0) || !finite_d(sigma)) ok = false;
        double alpha = sqrt(sigma);
        if (A[k][k] > 0.0) alpha = -alpha;
        const double vk = A[k][k] - alpha;
        const double vn = 2.0 * (sigma - A[k][k] * alpha);  // |v|^2
        MI_UNROLL
        for (int j = k + 1; j < N; j++) {
            double d = vk * A[k][j];
            MI_UNROLL
            for (int i = k + 1; i < 6; i++) d += A[i][k] * A[i][j];
            const double tau = 2.0 * d / vn;
            A[k][j] -= tau * vk;
            MI_UNROLL
            for (int i = k + 1; i < 6; i++) A[i][j] -= tau * A[i][k];
        }
        {
            double d = vk * b[k];
            MI_UNROLL
            for (int i = k + 1; i < 6; i++) d += A[i][k] * b[i];
            const double tau = 2.0 * d / vn;
            b[k] -= tau * vk;
            MI_UNROLL
            for (int i = k + 1; i < 6; i++) b[i] -= tau * A[i][k];
        }
        A[k][k] = alpha;
    }
    MI_UNROLL
    for (int k = N - 1; k >= 0; k--) {
        double s = b[k];
        MI_UNROLL
        for (int j = k + 1; j < N; j++) s -= A[k][j] * x[j];
        x[k] = s / A[k][k];
        if (!finite_d(x[k])) ok = false;
    }
    return ok;
}

// Packed upper triangle of a symmetric 12 x 12 matrix: entry (i, j), i <= j.
NP_HD int sym12(int i, int j)
{
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return lo * 12 - lo * (lo - 1) / 2 + (hi - lo);
}

// Cyclic Jacobi on the packed symmetric matrix at W[0..77]; the eigenvectors are left as the
// columns of the row-major 12 x 12 matrix at W[78..221], the eigenvalues on the diagonal.  A
// rotation is skipped (and the entry cleared) once 100 |a_pq| vanishes against both diagonal
// entries; the sweeps end when every off-diagonal entry is zero, or at the sweep limit.
NP_HD void jacobi_eigen12(const Strided<double>& W)
{
    for (int i = 0; i < 12; i++)
        for (int j = 0; j < 12; j++) W[78 + i * 12 + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < RP_JACOBI_SWEEPS; sweep++) {
        double off = 0.0;
        for (int p = 0; p < 11; p++)
            for (int q = p + 1; q < 12; q++) off += fabs(W[sym12(p, q)]);
        if (off == 0.0) break;
        for (int p = 0; p < 11; p++)
            for (int q = p + 1; q < 12; q++) {
                const int ipq = sym12(p, q), ipp = sym12(p, p), iqq = sym12(q, q);
                const double apq = W[ipq];
                if (apq == 0.0) continue;
                const double app = W[ipp], aqq = W[iqq];
                const double g = 100.0 * fabs(apq);
                if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
                    W[ipq] = 0.0;
                    continue;
                }
                const double theta = (aqq - app) / (2.0 * apq);
                const double at = fabs(theta) + sqrt(theta * theta + 1.0);
                const double t = theta < 0.0 ? -1.0 / at : 1.0 / at;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                W[ipp] = app - t * apq;
                W[iqq] = aqq + t * apq;
                W[ipq] = 0.0;
                for (int r = 0; r < 12; r++) {
                    if (r != p && r != q) {
                        const int irp = sym12(r, p), irq = sym12(r, q);
                        const double arp = W[irp], arq = W[irq];
                        W[irp] = c * arp - s * arq;
                        W[irq] = s * arp + c * arq;
                    }
                    const double vp = W[78 + r * 12 + p], vq = W[78 + r * 12 + q];
                    W[78 + r * 12 + p] = c * vp - s * vq;
                    W[78 + r * 12 + q] = s * vp + c * vq;
                }
            }
    }
}

// ------------------------------------------------------------------------------------------
// EPnP on five points (epnp.cpp), all fp64.
// ------------------------------------------------------------------------------------------
struct Epnp5 {
    double cx, cy, fx, fy;
    double cws[4][3];
    int col[4];  // the columns of the eigenvector matrix (W[78..221]) with the four smallest eigenvalues, the smallest first
    double rho[6];
};

// The five world points, pixels and barycentric coordinates, kept in the workspace behind the matrices.
#define RP_PW(i, k) W[222 + 3 * (i) + (k)]
#define RP_UV(i, k) W[237 + 2 * (i) + (k)]
#define RP_AL(i, j) W[247 + 4 * (i) + (j)]

// Component r of eigenvector k (sign rule applied in place).
NP_HD double evec(const Strided<double>& W, const Epnp5& e, int k, int r) { return W[78 + r * 12 + e.col[k]]; }

// Camera-frame points from the betas, then R, t by absolute orientation (estimate_R_and_t) and the
// summed reprojection error.  false when anything is not finite.
NP_HD bool pose_from_betas(const Strided<double>& W, const Epnp5& e, const double (&beta)[4], double* R, double* t, double& err)
{
    double ccs[4][3], pcs[5][3];
    MI_UNROLL
    for (int j = 0; j < 4; j++)
        MI_UNROLL
        for (int k = 0; k < 3; k++)
            ccs[j][k] = ((beta[0] * evec(W, e, 0, 3 * j + k) + beta[1] * evec(W, e, 1, 3 * j + k)) +
                         beta[2] * evec(W, e, 2, 3 * j + k)) +
                        beta[3] * evec(W, e, 3, 3 * j + k);
    MI_UNROLL
    for (int i = 0; i < 5; i++)
        MI_UNROLL
        for (int k = 0; k < 3; k++)
            pcs[i][k] = ((RP_AL(i, 0) * ccs[0][k] + RP_AL(i, 1) * ccs[1][k]) + RP_AL(i, 2) * ccs[2][k]) +
                        RP_AL(i, 3) * ccs[3][k];
    if (pcs[0][2] < 0.0) {  // solve_for_sign
        MI_UNROLL
        for (int i = 0; i < 5; i++)
            MI_UNROLL
            for (int k = 0; k < 3; k++) pcs[i][k] = -pcs[i][k];
    }
    double pc0[3], pw0[3];
    MI_UNROLL
    for (int k = 0; k < 3; k++) {
        pc0[k] = ((((pcs[0][k] + pcs[1][k]) + pcs[2][k]) + pcs[3][k]) + pcs[4][k]) / 5.0;
        pw0[k] = ((((RP_PW(0, k) + RP_PW(1, k)) + RP_PW(2, k)) + RP_PW(3, k)) + RP_PW(4, k)) / 5.0;
    }
    double A[3][3];  // ABt: sum (pc - pc0)(pw - pw0)^T
    MI_UNROLL
    for (int j = 0; j < 3; j++)
        MI_UNROLL
        for (int k = 0; k < 3; k++) {
            double s = 0.0;
            MI_UNROLL
            for (int i = 0; i < 5; i++) s += (pcs[i][j] - pc0[j]) * (RP_PW(i, k) - pw0[k]);
            A[j][k] = s;
        }
    // SVD A = U S V^T from cyclic Jacobi on A^T A: v1, v2 by descending eigenvalue, v3 = v1 x v2,
    // u_i = A v_i normalised, u3 = sign(det A) u1 x u2 — the third singular pair's sign, which is all
    // of it that R = U V^T depends on.  det R < 0 is fixed by negating R's third row, as the original.
    double a[3][3], ev[3][3];
    MI_UNROLL
    for (int i = 0; i < 3; i++)
        MI_UNROLL
        for (int j = 0; j < 3; j++) a[i][j] = (A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j];
    monoinit::jacobi_eigen3(a, ev);
    int i0, i1, i2;
    order3(a[0][0], a[1][1], a[2][2], i0, i1, i2);
    double V[3][3], U[3][3];  // V[c], U[c]: column c
    MI_UNROLL
    for (int k = 0; k < 3; k++) {
        V[0][k] = pick3(ev, k, i0);
        V[1][k] = pick3(ev, k, i1);
    }
    monoinit::cross3d(V[0], V[1], V[2]);
    MI_UNROLL
    for (int c = 0; c < 2; c++) {
        double n = 0.0;
        MI_UNROLL
        for (int i = 0; i < 3; i++) {
            U[c][i] = (A[i][0] * V[c][0] + A[i][1] * V[c][1]) + A[i][2] * V[c][2];
            n += U[c][i] * U[c][i];
        }
        n = sqrt(n);
        MI_UNROLL
        for (int i = 0; i < 3; i++) U[c][i] = U[c][i] / n;
    }
    monoinit::cross3d(U[0], U[1], U[2]);
    const double det = (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    const double sg = det < 0.0 ? -1.0 : 1.0;
    MI_UNROLL
    for (int i = 0; i < 3; i++)
        MI_UNROLL
        for (int j = 0; j < 3; j++) {
            const double r = (U[0][i] * V[0][j] + U[1][i] * V[1][j]) + sg * (U[2][i] * V[2][j]);
            R[3 * i + j] = i == 2 && det < 0.0 ? -r : r;
        }
    MI_UNROLL
    for (int i = 0; i < 3; i++) t[i] = pc0[i] - ((R[3 * i] * pw0[0] + R[3 * i + 1] * pw0[1]) + R[3 * i + 2] * pw0[2]);
    double sum = 0.0;
    MI_UNROLL
    for (int i = 0; i < 5; i++) {
        const double X = ((R[0] * RP_PW(i, 0) + R[1] * RP_PW(i, 1)) + R[2] * RP_PW(i, 2)) + t[0];
        const double Y = ((R[3] * RP_PW(i, 0) + R[4] * RP_PW(i, 1)) + R[5] * RP_PW(i, 2)) + t[1];
        const double Z = ((R[6] * RP_PW(i, 0) + R[7] * RP_PW(i, 1)) + R[8] * RP_PW(i, 2)) + t[2];
        const double iz = 1.0 / Z;
        const double du = RP_UV(i, 0) - (e.cx + e.fx * X * iz), dv = RP_UV(i, 1) - (e.cy + e.fy * Y * iz);
        sum += sqrt(du * du + dv * dv);
    }
    err = sum;
    bool ok = finite_d(sum);
    MI_UNROLL
    for (int k = 0; k < 9; k++) ok = ok && finite_d(R[k]);
    MI_UNROLL
    for (int k = 0; k < 3; k++) ok = ok && finite_d(t[k]);
    return ok;
}

// Five Gauss-Newton iterations on the four betas (gauss_newton): L at W[0..59] (6 x 10, row-major).
NP_HD bool gauss_newton(const Strided<double>& W, const double (&rho)[6], double (&beta)[4])
{
    bool ok = true;
    RP_NOUNROLL
    for (int iter = 0; iter < 5; iter++) {
        double A[6][4], b[6], x[4];
        MI_UNROLL
        for (int i = 0; i < 6; i++) {
            double l[10];
            MI_UNROLL
            for (int k = 0; k < 10; k++) l[k] = W[10 * i + k];
            A[i][0] = ((2.0 * l[0] * beta[0] + l[1] * beta[1]) + l[3] * beta[2]) + l[6] * beta[3];
            A[i][1] = ((l[1] * beta[0] + 2.0 * l[2] * beta[1]) + l[4] * beta[2]) + l[7] * beta[3];
            A[i][2] = ((l[3] * beta[0] + l[4] * beta[1]) + 2.0 * l[5] * beta[2]) + l[8] * beta[3];
            A[i][3] = ((l[6] * beta[0] + l[7] * beta[1]) + l[8] * beta[2]) + 2.0 * l[9] * beta[3];
            b[i] = rho[i] - (((((((((l[0] * beta[0] * beta[0] + l[1] * beta[0] * beta[1]) + l[2] * beta[1] * beta[1]) +
                                   l[3] * beta[0] * beta[2]) + l[4] * beta[1] * beta[2]) + l[5] * beta[2] * beta[2]) +
                                l[6] * beta[0] * beta[3]) + l[7] * beta[1] * beta[3]) + l[8] * beta[2] * beta[3]) +
                             l[9] * beta[3] * beta[3]);
        }
        ok = qr_lsq<4>(A, b, x) && ok;
        MI_UNROLL
        for (int k = 0; k < 4; k++) beta[k] += x[k];
    }
    return ok;
}

// The three linearised starts (find_betas_approx_1 / _2 / _3) with their sign rules.
NP_HD bool betas_start(const Strided<double>& W, const double (&rho)[6], int start, double (&beta)[4])
{
    double b[6];
    MI_UNROLL
    for (int i = 0; i < 6; i++) b[i] = rho[i];
    bool ok;
    if (start == 0) {  // [B11 B12 B13 B14]
        double A[6][4], x[4];
        MI_UNROLL
        for (int i = 0; i < 6; i++) {
            A[i][0] = W[10 * i + 0];
            A[i][1] = W[10 * i + 1];
            A[i][2] = W[10 * i + 3];
            A[i][3] = W[10 * i + 6];
        }
        ok = qr_lsq<4>(A, b, x);
        if (x[0] < 0.0) {
            beta[0] = sqrt(-x[0]);
            beta[1] = -x[1] / beta[0];
            beta[2] = -x[2] / beta[0];
            beta[3] = -x[3] / beta[0];
        } else {
            beta[0] = sqrt(x[0]);
            beta[1] = x[1] / beta[0];
            beta[2] = x[2] / beta[0];
            beta[3] = x[3] / beta[0];
        }
    } else if (start == 1) {  // [B11 B12 B22]
        double A[6][3], x[3];
        MI_UNROLL
        for (int i = 0; i < 6; i++)
            MI_UNROLL
            for (int k = 0; k < 3; k++) A[i][k] = W[10 * i + k];
        ok = qr_lsq<3>(A, b, x);
        if (x[0] < 0.0) {
            beta[0] = sqrt(-x[0]);
            beta[1] = x[2] < 0.0 ? sqrt(-x[2]) : 0.0;
        } else {
            beta[0] = sqrt(x[0]);
            beta[1] = x[2] > 0.0 ? sqrt(x[2]) : 0.0;
        }
        if (x[1] < 0.0) beta[0] = -beta[0];
        beta[2] = 0.0;
        beta[3] = 0.0;
    } else {  // [B11 B12 B22 B13 B23]
        double A[6][5], x[5];
        MI_UNROLL
        for (int i = 0; i < 6; i++)
            MI_UNROLL
            for (int k = 0; k < 5; k++) A[i][k] = W[10 * i + k];
        ok = qr_lsq<5>(A, b, x);
        if (x[0] < 0.0) {
            beta[0] = sqrt(-x[0]);
            beta[1] = x[2] < 0.0 ? sqrt(-x[2]) : 0.0;
        } else {
            beta[0] = sqrt(x[0]);
            beta[1] = x[2] > 0.0 ? sqrt(x[2]) : 0.0;
        }
        if (x[1] < 0.0) beta[0] = -beta[0];
        beta[2] = x[3] / beta[0];
        beta[3] = 0.0;
    }
    MI_UNROLL
    for (int k = 0; k < 4; k++) ok = ok && finite_d(beta[k]);
    return ok;
}

// One hypothesis: five correspondences -> R (row-major, 9), t (3) and the three starts' summed
// reprojection errors (-1 where a start failed).  false when no start gives a finite pose: no model.
// intr4 = {cx, cy, fx, fy}.  W: RP_WORK_D doubles of workspace.
NP_HD bool solve_epnp5(const Corr* c5, const float* intr4, const Strided<double>& W, double* R, double* t, double* err3)
{
    Epnp5 e;
    e.cx = (double)intr4[0];
    e.cy = (double)intr4[1];
    e.fx = (double)intr4[2];
    e.fy = (double)intr4[3];
    MI_UNROLL
    for (int i = 0; i < 5; i++) {
        RP_PW(i, 0) = (double)c5[i].x;
        RP_PW(i, 1) = (double)c5[i].y;
        RP_PW(i, 2) = (double)c5[i].z;
        RP_UV(i, 0) = (double)c5[i].u;
        RP_UV(i, 1) = (double)c5[i].v;
    }
    MI_UNROLL
    for (int k = 0; k < 9; k++) R[k] = 0.0;
    MI_UNROLL
    for (int k = 0; k < 3; k++) {
        t[k] = 0.0;
        err3[k] = -1.0;
    }
    // choose_control_points: the centroid and the principal directions scaled by sqrt(lambda / 5)
    MI_UNROLL
    for (int k = 0; k < 3; k++) e.cws[0][k] = ((((RP_PW(0, k) + RP_PW(1, k)) + RP_PW(2, k)) + RP_PW(3, k)) + RP_PW(4, k)) / 5.0;
    {
        double a[3][3], ev[3][3];
        MI_UNROLL
        for (int j = 0; j < 3; j++)
            MI_UNROLL
            for (int k = 0; k < 3; k++) {
                double s = 0.0;
                MI_UNROLL
                for (int i = 0; i < 5; i++) s += (RP_PW(i, j) - e.cws[0][j]) * (RP_PW(i, k) - e.cws[0][k]);
                a[j][k] = s;
            }
        monoinit::jacobi_eigen3(a, ev);
        int o[3];
        order3(a[0][0], a[1][1], a[2][2], o[0], o[1], o[2]);
        MI_UNROLL
        for (int c = 0; c < 3; c++) {
            const double lam = o[c] == 0 ? a[0][0] : (o[c] == 1 ? a[1][1] : a[2][2]);
            const double k = sqrt((lam > 0.0 ? lam : 0.0) / 5.0);
            double d[3] = {pick3(ev, 0, o[c]), pick3(ev, 1, o[c]), pick3(ev, 2, o[c])};
            sign_rule3(d);
            MI_UNROLL
            for (int j = 0; j < 3; j++) e.cws[c + 1][j] = e.cws[0][j] + k * d[j];
        }
    }
    // compute_barycentric_coordinates: the inverse of the control-point difference matrix by cofactors
    {
        double cc[3][3], ci[3][3];
        MI_UNROLL
        for (int i = 0; i < 3; i++)
            MI_UNROLL
            for (int j = 0; j < 3; j++) cc[i][j] = e.cws[j + 1][i] - e.cws[0][i];
        const double c00 = cc[1][1] * cc[2][2] - cc[1][2] * cc[2][1], c01 = cc[1][2] * cc[2][0] - cc[1][0] * cc[2][2],
                     c02 = cc[1][0] * cc[2][1] - cc[1][1] * cc[2][0];
        const double det = (cc[0][0] * c00 + cc[0][1] * c01) + cc[0][2] * c02;
        if (det == 0.0 || !finite_d(det)) return false;
        ci[0][0] = c00 / det;
        ci[1][0] = c01 / det;
        ci[2][0] = c02 / det;
        ci[0][1] = (cc[0][2] * cc[2][1] - cc[0][1] * cc[2][2]) / det;
        ci[1][1] = (cc[0][0] * cc[2][2] - cc[0][2] * cc[2][0]) / det;
        ci[2][1] = (cc[0][1] * cc[2][0] - cc[0][0] * cc[2][1]) / det;
        ci[0][2] = (cc[0][1] * cc[1][2] - cc[0][2] * cc[1][1]) / det;
        ci[1][2] = (cc[0][2] * cc[1][0] - cc[0][0] * cc[1][2]) / det;
        ci[2][2] = (cc[0][0] * cc[1][1] - cc[0][1] * cc[1][0]) / det;
        MI_UNROLL
        for (int i = 0; i < 5; i++) {
            MI_UNROLL
            for (int j = 0; j < 3; j++)
                RP_AL(i, 1 + j) = (ci[j][0] * (RP_PW(i, 0) - e.cws[0][0]) + ci[j][1] * (RP_PW(i, 1) - e.cws[0][1])) +
                                    ci[j][2] * (RP_PW(i, 2) - e.cws[0][2]);
            RP_AL(i, 0) = ((1.0 - RP_AL(i, 1)) - RP_AL(i, 2)) - RP_AL(i, 3);
        }
    }
    // M^T M (fill_M's rows {a fu, 0, a (uc - u)}, {0, a fv, a (vc - v)} per point and control point),
    // entry (3 a + c, 3 b + d) = sum over the points of (alpha_a alpha_b) g_cd, packed at W[0..77]
    {
        double g[5][6];  // g00 g02 g11 g12 g22 (g01 = 0)
        MI_UNROLL
        for (int i = 0; i < 5; i++) {
            const double du = e.cx - RP_UV(i, 0), dv = e.cy - RP_UV(i, 1);
            g[i][0] = e.fx * e.fx;
            g[i][1] = e.fx * du;
            g[i][2] = e.fy * e.fy;
            g[i][3] = e.fy * dv;
            g[i][4] = du * du + dv * dv;
            g[i][5] = 0.0;
        }
        MI_UNROLL
        for (int a = 0; a < 4; a++)
            MI_UNROLL
            for (int b = a; b < 4; b++) {
                double w[5];
                MI_UNROLL
                for (int i = 0; i < 5; i++) w[i] = RP_AL(i, a) * RP_AL(i, b);
                MI_UNROLL
                for (int c = 0; c < 3; c++)
                    MI_UNROLL
                    for (int d = 0; d < 3; d++) {
                        if (a == b && d < c) continue;
                        const int lo = c < d ? c : d, hi = c < d ? d : c;
                        // (0,0) g00, (0,1) 0, (0,2) g02, (1,1) g11, (1,2) g12, (2,2) g22
                        const int gi = lo == 0 ? (hi == 0 ? 0 : (hi == 1 ? 5 : 1)) : (lo == 1 ? (hi == 1 ? 2 : 3) : 4);
                        double s = 0.0;
                        if (gi != 5) {
                            MI_UNROLL
                            for (int i = 0; i < 5; i++) s += w[i] * g[i][gi];
                        }
                        W[sym12(3 * a + c, 3 * b + d)] = s;
                    }
            }
    }
    jacobi_eigen12(W);
    // the four smallest eigenvalues' vectors, the smallest first (the lower column on ties), each
    // under the sign rule
    {
        uint32_t used = 0;
        RP_NOUNROLL
        for (int k = 0; k < 4; k++) {
            int best = -1;
            double bv = 0.0;
            for (int j = 0; j < 12; j++) {
                if (used & (1u << j)) continue;
                const double d = W[sym12(j, j)];
                if (best < 0 || d < bv) {
                    best = j;
                    bv = d;
                }
            }
            used |= 1u << best;
            double big = 0.0;
            for (int r = 0; r < 12; r++) {
                const double x = W[78 + r * 12 + best];
                if (fabs(x) > fabs(big)) big = x;
            }
            if (big < 0.0)
                for (int r = 0; r < 12; r++) W[78 + r * 12 + best] = -W[78 + r * 12 + best];
            MI_UNROLL
            for (int kk = 0; kk < 4; kk++)
                if (kk == k) e.col[kk] = best;
        }
    }
    // compute_L_6x10 into W[0..59] (the packed matrix is dead) and compute_rho
    MI_UNROLL
    for (int i = 0; i < 6; i++) {
        const int a = i < 3 ? 0 : (i < 5 ? 1 : 2), b = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);
        double dv[4][3];
        MI_UNROLL
        for (int k = 0; k < 4; k++)
            MI_UNROLL
            for (int j = 0; j < 3; j++) dv[k][j] = evec(W, e, k, 3 * a + j) - evec(W, e, k, 3 * b + j);
        auto dot = [&dv](int p, int q) { return (dv[p][0] * dv[q][0] + dv[p][1] * dv[q][1]) + dv[p][2] * dv[q][2]; };
        W[10 * i + 0] = dot(0, 0);
        W[10 * i + 1] = 2.0 * dot(0, 1);
        W[10 * i + 2] = dot(1, 1);
        W[10 * i + 3] = 2.0 * dot(0, 2);
        W[10 * i + 4] = 2.0 * dot(1, 2);
        W[10 * i + 5] = dot(2, 2);
        W[10 * i + 6] = 2.0 * dot(0, 3);
        W[10 * i + 7] = 2.0 * dot(1, 3);
        W[10 * i + 8] = 2.0 * dot(2, 3);
        W[10 * i + 9] = dot(3, 3);
        const double d0 = e.cws[a][0] - e.cws[b][0], d1 = e.cws[a][1] - e.cws[b][1], d2 = e.cws[a][2] - e.cws[b][2];
        e.rho[i] = (d0 * d0 + d1 * d1) + d2 * d2;
    }
    // the three starts, each refined; the smallest error wins, the first on ties
    bool any = false;
    double best = 0.0;
    RP_NOUNROLL
    for (int s = 0; s < 3; s++) {
        double beta[4], Rs[9], ts[3], es;
        bool ok = betas_start(W, e.rho, s, beta);
        ok = gauss_newton(W, e.rho, beta) && ok;
        ok = pose_from_betas(W, e, beta, Rs, ts, es) && ok;
        if (!ok) continue;
        MI_UNROLL
        for (int k = 0; k < 3; k++)
            if (k == s) err3[k] = es;
        if (!any || es < best) {
            any = true;
            best = es;
            MI_UNROLL
            for (int k = 0; k < 9; k++) R[k] = Rs[k];
            MI_UNROLL
            for (int k = 0; k < 3; k++) t[k] = ts[k];
        }
    }
    return any;
}

// ------------------------------------------------------------------------------------------
// The inlier rule (PnPRansacCallback::computeError over cv::projectPoints, findInliers): the
// projection in fp64 rounded to float, the squared error in float, <= the threshold's square.
// ------------------------------------------------------------------------------------------
NP_HD bool is_inlier(const double* R, const double* t, const float* intr4, const Corr& c, float thr_sq)
{
    const double px = (double)c.x, py = (double)c.y, pz = (double)c.z;
    const double X = ((R[0] * px + R[1] * py) + R[2] * pz) + t[0];
    const double Y = ((R[3] * px + R[4] * py) + R[5] * pz) + t[1];
    const double Z = ((R[6] * px + R[7] * py) + R[8] * pz) + t[2];
    const double iz = Z == 0.0 ? 1.0 : 1.0 / Z;
    const float u = (float)((double)intr4[2] * (X * iz) + (double)intr4[0]);
    const float v = (float)((double)intr4[3] * (Y * iz) + (double)intr4[1]);
    const float du = c.u - u, dv = c.v - v;
    const float e = du * du + dv * dv;
    return e <= thr_sq;
}

// The float pose of a model: view-space t and column-major R, as mage_ba_pose_batch takes them.
NP_HD void float_pose(const double* R, const double* t, float* pos3, float* r9)
{
    for (int i = 0; i < 3; i++) {
        pos3[i] = (float)t[i];
        for (int j = 0; j < 3; j++) r9[j * 3 + i] = (float)R[3 * i + j];
    }
}

// RemoveMapPointsThatAreBehind's camera (:209-216, Data/Pose.cpp:110-118): the world-space position
// C = -(R^T t) and forward vector (R's third row), in float from the float pose.
struct BehindFilter {
    float C[3], fwd[3];
};
NP_HD BehindFilter behind_filter(const float* pos3, const float* r9)
{
    BehindFilter f;
    for (int i = 0; i < 3; i++) {
        const float col[3] = {r9[i * 3], r9[i * 3 + 1], r9[i * 3 + 2]};  // row i of R^T
        f.C[i] = -newpoints::dot3(col, pos3);
        f.fwd[i] = r9[i * 3 + 2];
    }
    return f;
}
NP_HD bool is_behind(const BehindFilter& f, const Corr& c)
{
    const float d[3] = {c.x - f.C[0], c.y - f.C[1], c.z - f.C[2]};
    return newpoints::dot3(d, f.fwd) <= 0.f;
}

// The gate of :339: inFront / (float)n < RansacInliersPctRequired fails (n counts all matches).
NP_HD bool gate_fails(uint32_t in_front, uint32_t n, float min_pct) { return (float)in_front / (float)n < min_pct; }

NP_HD void init_result(mage_reloc_pnp_result& r, uint32_t n_matches)
{
    r = mage_reloc_pnp_result{};
    r.n_matches = n_matches;
    r.win_iteration = -1;
    for (int k = 0; k < 5; k++) r.win_indices[k] = -1;
    r.r9[0] = r.r9[4] = r.r9[8] = 1.f;
}

#undef RP_PW
#undef RP_UV
#undef RP_AL

}  // namespace relocpnp
}  // namespace mage
