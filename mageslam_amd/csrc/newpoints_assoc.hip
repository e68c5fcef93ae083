// newpoints_assoc.hip — NewMapPointsCreation's LocallyAssociateNewAssociations on MI355X (gfx950).
//
// The reference (Core/MAGESLAM/Source/Mapping/NewMapPointsCreation.cpp:337-424) offers every new
// point, in push_back order, to every covisible keyframe it is not yet associated with: project,
// gate (TrackLocalMap::IsGoodCandidate), predict the octave, then the single-query RadiusMatch
// against the keyframe's still-unassociated keypoints; a success takes the keypoint for the later
// points.  State flows only through one keyframe's mask, so the keyframes are independent: one
// workgroup per (problem, keyframe).  It stages the keyframe's x, y and mask bits in LDS and lists
// the keypoints by horizontal band (keyframe_take.hpp, shared with the cheap loop closure), clears
// the keypoints CreateInitialAssociations took (:314), and takes the points 256 at a time:
//   gate      one thread per point (newpoints_math.hpp project_gate); a refused point's record and
//             verdict are final, the others are compacted in point order (ballot prefix);
//   gather    64 surviving points at a time, 4 lanes per point, up to 8 candidates per point;
//   resolve   one wave takes the chunk's points in order with ordered_take.hpp's resolve_in_order
//             (the resolver TrackLocalMap's matching uses; the argument for its exactness is there).
// The first build scanned all of the keyframe's keypoints per point (no index): 0.656 ms per launch
// on the shape of tools/bench_new_points_assoc.py (256 problems x 8 keyframes x 2000 keypoints), the
// ~nkp / 4 box tests per lane twice over (72 points are two rounds of 64) being nearly all of it.
// The bands cut the scan to the ~8 % of the keypoints near the point's row.  Only commuting integer
// atomics, barriers and plain stores; nothing in the results depends on the order in which threads
// run, and every loop is bounded by the counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "keyframe_take.hpp"
#include "newpoints_math.hpp"

namespace mage {
namespace {

using namespace newpoints;

// The host-buffer entry's scratch slot, after newpoints.hip's (common.hpp stays as it is).
constexpr ScratchSlot SCRATCH_NEWPOINTS_ASSOC = static_cast<ScratchSlot>(6);

constexpr int NA_THREADS = kt::KT_THREADS;
constexpr int NA_BANDS = kt::KT_BANDS;
static_assert(NA_MAX_KP <= kt::KT_MAX_KP, "keypoint indices must fit resolve_in_order's packings");

struct NaParams {
    AssocConsts c;
    kt::Search search;
    uint32_t kf_slots;
    const mage_new_point* points;
    uint32_t cap;
    const uint32_t* n_points;
    const uint8_t* ki_desc;
    long long ki_pitch;
    const uint32_t* n_ki;
    const uint32_t* n_kf;
    const float *kf_pos3, *kf_r9, *kf_intr4;
    const mage_keypoint* kf_kp;
    const uint8_t* kf_desc;
    uint8_t* kf_mask;
    long long kf_pitch;
    const uint32_t* n_kf_kp;
    const int32_t* kf_slot;
    mage_new_point_assoc* out;
    uint8_t* verdict;
    uint32_t* status;
};

// The workgroup's (problem, keyframe) pair.
struct NaPair {
    uint32_t nkp, npts, nki;
    int slot;          // the keyframe's Kc slot, or -1
    long long stride;  // between a keyframe's records (and verdicts) of consecutive points
    const mage_new_point* pts;
    const mage_keypoint* kp;
    const uint8_t *kdesc, *kidesc;
    uint8_t* mask;
    const float* intr;
    mage_new_point_assoc* out;
    uint8_t* verdict;
};

// CreateInitialAssociations' own associations with this keyframe (:314) leave the mask.
__device__ __forceinline__ void clear_claims(const NaPair& v, kt::Shared& s)
{
    if (v.slot >= 0)
        for (uint32_t i = threadIdx.x; i < v.npts; i += NA_THREADS) {
            const uint32_t sl = v.pts[i].kc_slot, q = v.pts[i].kc_index;
            if (sl == (uint32_t)v.slot && q < v.nkp) mask_clear(s.m, (int)q);
        }
    __syncthreads();
}

// Points c0 .. c0 + 255, one thread each: a refused point's record and verdict are final, the others
// are compacted in point order into px, py, pi, po.  Returns their count.
__device__ __forceinline__ int gate_and_compact(const NaParams& p, const NaPair& v, kt::Shared& s, const Frame& frame,
                                                uint32_t c0)
{
    const uint32_t i = c0 + threadIdx.x;
    bool pass = false;
    float px = 0.f, py = 0.f;
    int oc = 0;
    if (i < v.npts) {
        const mage_new_point pt = v.pts[i];
        uint8_t vd;
        if (pt.ki_index >= v.nki || pt.kc_slot >= (uint32_t)NP_MAX_SLOTS)
            vd = NA_BAD_INDEX;
        else if (v.slot >= 0 && pt.kc_slot == (uint32_t)v.slot)
            vd = pt.kc_index < v.nkp ? NA_SAME_FRAME : NA_BAD_INDEX;
        else {
            vd = project_gate(p.c, frame, v.intr, pt, px, py, oc);
            pass = vd == NA_NO_MATCH;
        }
        if (!pass) {
            v.out[i * v.stride] = mage_new_point_assoc{px, py, oc, -1};
            v.verdict[i * v.stride] = vd;
        }
    }
    return kt::compact(s, pass, px, py, (int)i, oc);
}

// The taken keypoints (the claims included) back to the mask bytes.
__device__ __forceinline__ void write_mask(const NaPair& v, const kt::Shared& s)
{
    for (int t = threadIdx.x; t < (int)v.nkp; t += NA_THREADS)
        if (!mask_bit(s.m, t)) v.mask[t] = 0;
}

__global__ __launch_bounds__(NA_THREADS) void new_points_assoc_kernel(NaParams p)
{
    __shared__ kt::Shared s;
    __shared__ Frame s_frame;  // beside the arrays: on its own the compiler drops the members project_gate never reads
    const int tid = threadIdx.x;
    const uint32_t prob = blockIdx.x / p.kf_slots, k = blockIdx.x % p.kf_slots;
    const long long pair = blockIdx.x;
    const uint32_t nkf = p.n_kf[prob];
    if (nkf <= p.kf_slots && k >= nkf) return;
    NaPair v;
    v.nkp = p.n_kf_kp[pair];
    v.npts = min(p.n_points[prob], p.cap);
    v.stride = p.kf_slots;
    v.out = p.out + (long long)prob * p.cap * v.stride + k;
    v.verdict = p.verdict + (long long)prob * p.cap * v.stride + k;
    if (nkf > p.kf_slots || v.nkp > (uint32_t)NA_MAX_KP || (long long)v.nkp > p.kf_pitch) {  // uniform over the workgroup
        if (tid == 0) atomicOr(p.status, 1u);
        for (uint32_t i = tid; i < v.npts; i += NA_THREADS) v.out[i * v.stride] = mage_new_point_assoc{0.f, 0.f, 0, -1};
        return;
    }
    v.pts = p.points + (long long)prob * p.cap;
    v.kp = p.kf_kp + pair * p.kf_pitch;
    v.kdesc = p.kf_desc + 32ll * pair * p.kf_pitch;
    v.mask = p.kf_mask + pair * p.kf_pitch;
    v.kidesc = p.ki_desc + 32ll * prob * p.ki_pitch;
    v.nki = (uint32_t)min((long long)p.n_ki[prob], p.ki_pitch);
    v.slot = p.kf_slot[pair];
    v.intr = p.kf_intr4 + 4 * pair;

    kt::stage_keyframe(
        p.search.band_scale, (int)v.nkp, v.kp, s, [&](int t) { return v.mask[t] != 0; },
        [&] {
            Frame f;
            make_frame(p.kf_pos3 + 3 * pair, p.kf_r9 + 9 * pair, v.intr, f);
            s_frame = f;
        });
    clear_claims(v, s);
    const auto desc_of = [&](int i) { return v.kidesc + 32ll * v.pts[i].ki_index; };
    for (uint32_t c0 = 0; c0 < v.npts; c0 += NA_THREADS) {
        const int cnt = gate_and_compact(p, v, s, s_frame, c0);
        kt::take_in_order(p.search, v.kdesc, s, cnt, desc_of, [&](int i, bool ok, int t) {
            const long long o = (long long)s.pi[i] * v.stride;
            v.out[o] = mage_new_point_assoc{s.px[i], s.py[i], s.po[i], ok ? t : -1};
            v.verdict[o] = ok ? (uint8_t)NA_ASSOCIATED : (uint8_t)NA_NO_MATCH;
        });
    }
    write_mask(v, s);
}

}  // namespace
}  // namespace mage

extern "C" {

mage_status mage_new_points_associate_batch_device(
    const mage_new_points_settings* settings, const mage_new_points_assoc_settings* assoc, uint32_t problems,
    uint32_t kf_slots, const mage_new_point* d_points, uint32_t cap, const uint32_t* d_n_points, const uint8_t* d_ki_desc,
    int64_t ki_pitch, const uint32_t* d_n_ki, const uint32_t* d_n_kf, const float* d_kf_pos3, const float* d_kf_r9,
    const float* d_kf_intr4, const mage_keypoint* d_kf_kp, const uint8_t* d_kf_desc, uint8_t* d_kf_mask, int64_t kf_pitch,
    const uint32_t* d_n_kf_kp, const int32_t* d_kf_slot, mage_new_point_assoc* d_assoc, uint8_t* d_verdict,
    uint32_t* d_status, mage_stream stream)
{
    using namespace mage;
    const char* why = newpoints::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    why = newpoints::check_assoc_settings(assoc);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    if (problems == 0 || kf_slots == 0) return MAGE_OK;
    MAGE_REQUIRE(d_points && d_n_points && d_ki_desc && d_n_ki && d_n_kf && d_kf_pos3 && d_kf_r9 && d_kf_intr4 &&
                     d_kf_kp && d_kf_desc && d_kf_mask && d_n_kf_kp && d_kf_slot && d_assoc && d_verdict && d_status,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(ki_pitch > 0 && kf_pitch > 0 && cap > 0, MAGE_EINVAL, "pitches and capacities must be positive");
    MAGE_REQUIRE((uint64_t)problems * kf_slots <= 0x7FFFFFFFull, MAGE_EINVAL, "too many (problem, keyframe) pairs");
    MAGE_REQUIRE(reinterpret_cast<uintptr_t>(d_ki_desc) % 16 == 0 && reinterpret_cast<uintptr_t>(d_kf_desc) % 16 == 0,
                 MAGE_EINVAL, "descriptor pointers must be 16-byte aligned");
    NaParams p{};
    p.c = newpoints::make_assoc_consts(*settings, *assoc);
    p.search = kt::Search{p.c.radius, (float)NA_BANDS / p.c.image_h, p.c.max_dist, p.c.min_diff};
    p.kf_slots = kf_slots;
    p.points = d_points;
    p.cap = cap;
    p.n_points = d_n_points;
    p.ki_desc = d_ki_desc;
    p.ki_pitch = ki_pitch;
    p.n_ki = d_n_ki;
    p.n_kf = d_n_kf;
    p.kf_pos3 = d_kf_pos3;
    p.kf_r9 = d_kf_r9;
    p.kf_intr4 = d_kf_intr4;
    p.kf_kp = d_kf_kp;
    p.kf_desc = d_kf_desc;
    p.kf_mask = d_kf_mask;
    p.kf_pitch = kf_pitch;
    p.n_kf_kp = d_n_kf_kp;
    p.kf_slot = d_kf_slot;
    p.out = d_assoc;
    p.verdict = d_verdict;
    p.status = d_status;
    launch("newpoints.associate", new_points_assoc_kernel, dim3(problems * kf_slots), dim3(NA_THREADS), 0,
           (hipStream_t)stream, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

mage_status mage_new_points_associate(const mage_new_points_settings* settings,
                                      const mage_new_points_assoc_settings* assoc, const mage_new_point* points,
                                      uint32_t n_points, const uint8_t* ki_desc, uint32_t n_ki, uint32_t n_kf,
                                      const float* kf_pos3, const float* kf_r9, const float* kf_intr4,
                                      const mage_keypoint* kf_kp, const uint8_t* kf_desc, const uint32_t* kf_start,
                                      const int32_t* kf_slot, uint8_t* kf_mask, mage_new_point_assoc* out,
                                      uint8_t* verdict, uint32_t* status, int device)
{
    using namespace mage;
    const char* why = newpoints::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    why = newpoints::check_assoc_settings(assoc);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(status, MAGE_EINVAL, "null argument");
    *status = 0;
    if (n_points == 0 || n_kf == 0) return MAGE_OK;
    MAGE_REQUIRE(points && out && verdict && kf_pos3 && kf_r9 && kf_intr4 && kf_start && kf_slot && (n_ki == 0 || ki_desc),
                 MAGE_EINVAL, "null argument");
    uint32_t pitch = 1;
    for (uint32_t k = 0; k < n_kf; k++) {
        MAGE_REQUIRE(kf_start[k] <= kf_start[k + 1], MAGE_EINVAL, "start offsets must not decrease");
        MAGE_REQUIRE(kf_slot[k] >= -1 && kf_slot[k] < newpoints::NP_MAX_SLOTS, MAGE_EINVAL, "kf_slot must be in [-1, 7]");
        const uint32_t nk = kf_start[k + 1] - kf_start[k];
        if (nk <= (uint32_t)newpoints::NA_MAX_KP) pitch = std::max(pitch, nk);
    }
    MAGE_REQUIRE(kf_start[n_kf] == kf_start[0] || (kf_kp && kf_desc && kf_mask), MAGE_EINVAL, "null argument");
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    HostScratch* sp = host_scratch(device, SCRATCH_NEWPOINTS_ASSOC);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [points][ki desc][counts][poses][kf kp][kf desc] | [masks][status][verdicts] | [records]:
    // everything up to the records in one H2D copy (the verdict bytes of a keyframe over the limit
    // are the caller's), the masks and outputs back in one D2H copy.  A keyframe over the limit keeps
    // its count and sends no data.
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t nkf = n_kf, np = n_points, kip = std::max(n_ki, 1u);
    const size_t opts = 0, okid = al(opts + 48 * np), ocnt = al(okid + 32 * kip), opose = al(ocnt + 4 * (3 + 2 * nkf)),
                 okp = al(opose + 64 * nkf), okd = al(okp + 28 * nkf * pitch), omask = al(okd + 32 * nkf * pitch),
                 ost = al(omask + nkf * pitch), over = al(ost + 4), orec = al(over + np * nkf),
                 total = al(orec + 16 * np * nkf);
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(total)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    std::memset(h, 0, over);
    std::memcpy(h + opts, points, 48 * np);
    if (n_ki) std::memcpy(h + okid, ki_desc, 32ull * n_ki);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(h + ocnt);  // [n_points, n_ki, n_kf, n_kf_kp x n_kf, kf_slot x n_kf]
    cnt[0] = n_points;
    cnt[1] = n_ki;
    cnt[2] = n_kf;
    float* hp = reinterpret_cast<float*>(h + opose);  // [pos3 x n_kf | r9 x n_kf | intr4 x n_kf]
    std::memcpy(hp, kf_pos3, 12 * nkf);
    std::memcpy(hp + 3 * nkf, kf_r9, 36 * nkf);
    std::memcpy(hp + 12 * nkf, kf_intr4, 16 * nkf);
    for (uint32_t k = 0; k < n_kf; k++) {
        const uint32_t nk = kf_start[k + 1] - kf_start[k];
        cnt[3 + k] = nk;
        cnt[3 + nkf + k] = (uint32_t)kf_slot[k];
        if (nk == 0 || nk > (uint32_t)newpoints::NA_MAX_KP) continue;
        std::memcpy(h + okp + 28 * (k * (size_t)pitch), kf_kp + kf_start[k], 28ull * nk);
        std::memcpy(h + okd + 32 * (k * (size_t)pitch), kf_desc + 32ull * kf_start[k], 32ull * nk);
        std::memcpy(h + omask + k * (size_t)pitch, kf_mask + kf_start[k], nk);
    }
    std::memcpy(h + over, verdict, np * nkf);
    MAGE_HIP(hipMemcpyAsync(b, h, orec, hipMemcpyHostToDevice, S.st));
    const uint32_t* dc = reinterpret_cast<const uint32_t*>(b + ocnt);
    const float* dp = reinterpret_cast<const float*>(b + opose);
    r = mage_new_points_associate_batch_device(
        settings, assoc, 1, n_kf, reinterpret_cast<const mage_new_point*>(b + opts), n_points, dc,
        reinterpret_cast<const uint8_t*>(b + okid), (int64_t)kip, dc + 1, dc + 2, dp, dp + 3 * nkf, dp + 12 * nkf,
        reinterpret_cast<const mage_keypoint*>(b + okp), reinterpret_cast<const uint8_t*>(b + okd),
        reinterpret_cast<uint8_t*>(b + omask), pitch, dc + 3, reinterpret_cast<const int32_t*>(dc + 3 + nkf),
        reinterpret_cast<mage_new_point_assoc*>(b + orec), reinterpret_cast<uint8_t*>(b + over),
        reinterpret_cast<uint32_t*>(b + ost), S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + omask, b + omask, total - omask, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    *status = *reinterpret_cast<const uint32_t*>(h + ost);
    std::memcpy(verdict, h + over, np * nkf);
    std::memcpy(out, h + orec, 16 * np * nkf);
    for (uint32_t k = 0; k < n_kf; k++) {
        const uint32_t nk = kf_start[k + 1] - kf_start[k];
        if (nk && nk <= (uint32_t)newpoints::NA_MAX_KP) std::memcpy(kf_mask + kf_start[k], h + omask + k * (size_t)pitch, nk);
    }
    return MAGE_OK;
}

}  // extern "C"
