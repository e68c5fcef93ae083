// reloc_pnp.cpp — the plain C++ twin of reloc_pnp.hip: PoseEstimator::PNPRansac
// (Tracking/PoseEstimator.cpp:610-638) with the steps around it in TryEstimatePoseFromCandidates
// (:291-342) as the sequential loop of RANSACPointSetRegistrator::run — sample, solve, count, update
// niters, one iteration after the other — over the arithmetic of reloc_pnp_math.hpp.  The CPU
// backend: same verdicts, poses, indices, arrays, trace and bits as the kernels.
//
// This file includes no HIP header, so that it also builds as plain host C++ on its own
// (tests/cpp/reloc_pnp_host_check.cpp): set_error and the argument check are declared here as
// common.hpp declares them.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "reloc_pnp_math.hpp"

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

namespace mage {
namespace relocpnp {
namespace {

// RANSACPointSetRegistrator::run's loop: hypothesis(it) makes iteration it's model and returns its
// inlier count, -1 without a model, -2 without a sample.  Nothing past the loop's end is asked for.
template <class Hypothesis>
LoopResult sequential_loop(uint32_t max_iters, uint32_t n, double confidence, bool adaptive, const Hypothesis& hypothesis)
{
    uint32_t niters = adaptive ? std::max(max_iters, 1u) : 1u, best = 0, iter = 0;
    int32_t win = -1;
    for (; iter < niters; iter++) {
        const int good = hypothesis(iter);
        if (good == -2) break;
        if (good < 0) continue;
        if ((uint32_t)good > std::max(best, 4u)) {
            best = (uint32_t)good;
            win = (int32_t)iter;
            if (adaptive) niters = (uint32_t)update_num_iters(confidence, (double)(n - best) / (double)n, (int)niters);
        }
    }
    return LoopResult{win, best, niters, iter};
}

}  // namespace
}  // namespace relocpnp
}  // namespace mage

extern "C" uint64_t mage_reloc_pnp_trace_bytes(uint32_t iterations)
{
    return mage::relocpnp::trace_layout(iterations).bytes;
}

extern "C" mage_status mage_debug_reloc_pnp_update(double confidence, uint32_t n, uint32_t max_iters, int32_t* out)
{
    MAGE_REQUIRE(out && n > 0, MAGE_EINVAL, "null argument");
    for (uint32_t g = 0; g <= n; g++)
        out[g] = mage::relocpnp::update_num_iters(confidence, (double)(n - g) / (double)n, (int)max_iters);
    return MAGE_OK;
}

extern "C" mage_status mage_debug_reloc_pnp_loop(const int32_t* solved, const uint32_t* inliers, uint32_t max_iters,
                                                 uint32_t n, double confidence, int32_t sequential, int32_t* out)
{
    using namespace mage::relocpnp;
    MAGE_REQUIRE(solved && inliers && out && n > 0 && max_iters >= 1 && max_iters <= (uint32_t)RP_MAX_ITERS, MAGE_EINVAL,
                 "bad argument");
    LoopResult r;
    if (sequential) {
        r = sequential_loop(max_iters, n, confidence, true, [&](uint32_t it) { return solved[it] ? (int)inliers[it] : -1; });
    } else {
        const std::vector<int32_t> idx(5 * (size_t)max_iters, 0);
        r = replay_loop(idx.data(), solved, inliers, max_iters, n, confidence, true);
    }
    out[0] = r.win;
    out[1] = (int32_t)r.best;
    out[2] = (int32_t)r.niters;
    out[3] = (int32_t)r.run;
    return MAGE_OK;
}

extern "C" mage_status mage_reloc_pnp_host(const mage_reloc_settings* settings, const float* intr4, const float* map_xyzi,
                                           uint32_t n_kf, const mage_keypoint* kp, uint32_t n_kp,
                                           const mage_dmatch* matches, uint32_t n_matches, mage_reloc_pnp_result* result,
                                           uint32_t* inlier_idx, uint32_t cap, float* points3, float* uv, float* info,
                                           void* trace)
{
    using namespace mage;
    using namespace mage::relocpnp;
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(intr4 && result, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE((n_kf == 0 || map_xyzi) && (n_kp == 0 || kp) && (n_matches == 0 || matches) &&
                     (cap == 0 || (inlier_idx && points3 && uv && info)),
                 MAGE_EINVAL, "null argument");
    const Consts c = make_consts(*settings);
    mage_reloc_pnp_result R;
    init_result(R, n_matches);
    const uint32_t n = n_matches;
    if (n > (uint32_t)RP_MAX_MATCHES)
        R.status = RP_STATUS_OVER_LIMIT;
    else
        for (uint32_t m = 0; m < n; m++) {
            const int q = matches[m].query_idx, t = matches[m].train_idx;
            if (q < 0 || (uint32_t)q >= n_kf || t < 0 || (uint32_t)t >= n_kp || !(map_xyzi[4 * q + 3] > 0.f))
                R.status = RP_STATUS_BAD_INDEX;
        }
    if (R.status == 0 && n < c.min_matches) R.verdict = RP_FEW_MATCHES;
    if (R.status == 0 && R.verdict == RP_OK && n < 5) R.verdict = RP_NO_MODEL;
    if (R.status != 0 || R.verdict != RP_OK) {
        *result = R;
        return MAGE_OK;
    }
    // the matched map points and keypoints (:301-308)
    std::vector<Corr> pts(n);
    for (uint32_t m = 0; m < n; m++) {
        const float* p = map_xyzi + 4 * (size_t)matches[m].query_idx;
        const mage_keypoint& k = kp[matches[m].train_idx];
        pts[m] = Corr{p[0], p[1], p[2], p[3], k.x, k.y, matches[m].query_idx, matches[m].train_idx};
    }
    const TraceLayout L = trace_layout(c.iters);
    std::vector<char> own;
    const bool want_trace = trace != nullptr;
    if (!trace) {
        own.resize(L.bytes);
        trace = own.data();
    }
    const Trace T = trace_at(static_cast<char*>(trace), L);
    const bool adaptive = n > 5;
    if (adaptive) {
        sample_indices(n, c.iters, T.idx);
    } else {
        for (uint32_t k = 0; k < 5 * c.iters; k++) T.idx[k] = k < 5 ? (int32_t)k : -1;
    }
    std::vector<uint8_t> mask(n), best_mask(n);
    const auto hypothesis = [&](uint32_t it) -> int {
        double* Rm = T.R + 9ull * it;
        double* tm = T.t + 3ull * it;
        T.solved[it] = 0;
        T.count[it] = 0;
        if (T.idx[5 * it] < 0) {
            std::memset(Rm, 0, 72);
            std::memset(tm, 0, 24);
            for (int k = 0; k < 3; k++) T.err[3ull * it + k] = -1.0;
            return -2;
        }
        Corr c5[5];
        for (int k = 0; k < 5; k++) c5[k] = pts[T.idx[5 * it + k]];
        double W[RP_WORK_D];
        if (!solve_epnp5(c5, intr4, Strided<double>{W, 1}, Rm, tm, T.err + 3ull * it)) return -1;
        T.solved[it] = 1;
        uint32_t good = 0;
        for (uint32_t m = 0; m < n; m++) {
            mask[m] = !adaptive || is_inlier(Rm, tm, intr4, pts[m], c.thr_sq);
            good += mask[m];
        }
        T.count[it] = good;
        return (int)good;
    };
    uint32_t best_seen = 0;
    const LoopResult loop = sequential_loop(c.iters, n, c.confidence, adaptive, [&](uint32_t it) {
        const int good = hypothesis(it);
        if (good > (int)std::max(best_seen, 4u)) {  // the loop takes it: keep its mask
            best_seen = (uint32_t)good;
            best_mask = mask;
        }
        return good;
    });
    // the trace holds every iteration, as the kernels compute them
    if (want_trace)
        for (uint32_t it = loop.run; it < c.iters; it++) hypothesis(it);
    R.iterations = loop.niters;
    R.iterations_run = loop.run;
    if (loop.win < 0) {
        R.verdict = RP_NO_MODEL;
        *result = R;
        return MAGE_OK;
    }
    R.win_iteration = loop.win;
    R.n_inliers = loop.best;
    for (int k = 0; k < 5; k++) R.win_indices[k] = T.idx[5 * loop.win + k];
    float_pose(T.R + 9ull * loop.win, T.t + 3ull * loop.win, R.pos3, R.r9);
    // the inliers in match order without those behind the camera (:329-338), the gate (:339)
    const BehindFilter bf = behind_filter(R.pos3, R.r9);
    uint32_t in_front = 0;
    for (uint32_t m = 0; m < n; m++) {
        if (!best_mask[m] || is_behind(bf, pts[m])) continue;
        if (in_front < cap) inlier_idx[in_front] = m;
        in_front++;
    }
    R.n_in_front = in_front;
    R.n_kept = std::min(in_front, cap);
    if (in_front > cap) R.status |= RP_STATUS_OVER_CAP;
    if (gate_fails(in_front, n, c.min_pct)) {
        R.verdict = RP_FEW_INLIERS;
        *result = R;
        return MAGE_OK;
    }
    for (uint32_t i = 0; i < R.n_kept; i++) {
        const Corr& p = pts[inlier_idx[i]];
        points3[3 * i] = p.x;
        points3[3 * i + 1] = p.y;
        points3[3 * i + 2] = p.z;
        uv[2 * i] = p.u;
        uv[2 * i + 1] = p.v;
        info[i] = p.info;
    }
    *result = R;
    return MAGE_OK;
}
