// stereoinit.hip — the device stage of StereoMapInit::Initialize on MI355X (gfx950).
//
// The reference (Core/MAGESLAM/Source/Stereo/StereoMapInit.cpp:97-194) masks frame 0's keypoints to
// the overlap crop (:28-45, :104-105), matches the masked frame 0 against frame 1 (:112) and walks
// the matches in order through MapInitialization::TriangulatePoints (Tracking/MapInitialization.cpp:
// 911-986); the accepted matches become the map points and the two keyframes' associations that
// BundleAdjustInitializationData hands to the bundler (:1099-1110).  Here that is three launches on
// one stream, batched over stereo pairs, one workgroup per pair in the two kernels of this file:
//   stereo_crop_mask_kernel    the mask bytes, their count, and the masked descriptors packed in
//                              keypoint order with their keypoint indices — the A side the two-way
//                              matcher (match.hip) then reads, as Match packs descriptorMatrixA;
//   stereo_triangulate_kernel  the matcher's records, 256 at a time in match order: queryIdx back
//                              to frame 0's keypoint, the geometry per thread (stereoinit_math.hpp),
//                              the accepted matches compacted in match order, then the bundler's
//                              inputs from the compacted records.
// A match's verdict depends on the match alone, so only the output positions need an order: wave
// ballots, a prefix over the wave counts and a running base across chunks (block_prefix).  No
// atomics; nothing depends on the order in which threads run; all loops are bounded by the counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "ordered_take.hpp"
#include "stereoinit_math.hpp"

namespace mage {
namespace {

using namespace stereoinit;

// The host-buffer entry's scratch slot, after common.hpp's ScratchSlot values and the new-points
// entries' 5 and 6 (declared here for the same reason as there: common.hpp stays as it is).
constexpr ScratchSlot SCRATCH_STEREOINIT = static_cast<ScratchSlot>(7);

constexpr int ST_THREADS = 256;
constexpr int ST_WAVES = ST_THREADS / kWave;

struct StParams {
    float two_max_epipolar, min_ratio;
    const float *pos3, *r9, *intr4;
    const int32_t* crop;
    const mage_keypoint *kp0, *kp1;
    const uint8_t* desc0;
    long long pitch0, pitch1;
    const uint32_t *n0, *n1;
    uint8_t* mask0;
    uint32_t* n_masked;
    uint8_t* pack_desc;    // masked descriptors in keypoint order, pitch0 x 32 bytes per pair; or null
    uint32_t* pack_index;  // their keypoint indices, pitch0 per pair; null when the matches are given
    mage_dmatch* matches;
    uint32_t match_cap;
    const uint32_t* n_matches;
    uint8_t* verdict;
    mage_stereo_point* out;
    uint32_t cap;
    uint32_t* n_out;
    float *ba_points, *ba_uv;
    uint32_t *ba_cam, *ba_pt;
    float* ba_info;
    uint32_t* status;
};

// A pair either kernel leaves alone: a frame over the matcher's limit or over its pitch.
__device__ __forceinline__ bool over_limit(const StParams& p, uint32_t n0, uint32_t n1)
{
    return n0 > (uint32_t)ST_MAX_KP || n1 > (uint32_t)ST_MAX_KP || (long long)n0 > p.pitch0 || (long long)n1 > p.pitch1;
}

__global__ __launch_bounds__(ST_THREADS) void stereo_crop_mask_kernel(StParams p)
{
    __shared__ uint32_t s_wsum[ST_WAVES];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const uint32_t n0 = p.n0[pr], n1 = p.n1[pr];
    if (over_limit(p, n0, n1)) {  // uniform over the workgroup
        if (tid == 0) p.n_masked[pr] = 0;
        return;
    }
    const int32_t crop[4] = {p.crop[4 * pr], p.crop[4 * pr + 1], p.crop[4 * pr + 2], p.crop[4 * pr + 3]};
    const long long row0 = pr * p.pitch0;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < n0; c0 += ST_THREADS) {
        const uint32_t i = c0 + tid;
        bool in = false;
        if (i < n0) {
            const mage_keypoint& kp = p.kp0[row0 + i];
            in = within_area(kp.x, kp.y, crop);
            p.mask0[row0 + i] = in ? 1 : 0;
        }
        uint32_t total;
        const uint32_t pos = base + block_prefix<ST_WAVES>(in, s_wsum, &total);  // pos < n0 <= pitch0
        if (in && p.pack_index) {
            const uint4* src = reinterpret_cast<const uint4*>(p.desc0 + 32 * (row0 + i));
            uint4* dst = reinterpret_cast<uint4*>(p.pack_desc + 32 * (row0 + pos));
            dst[0] = src[0];
            dst[1] = src[1];
            p.pack_index[row0 + pos] = i;
        }
        base += total;
    }
    if (tid == 0) p.n_masked[pr] = base;
}

__global__ __launch_bounds__(ST_THREADS) void stereo_triangulate_kernel(StParams p)
{
    __shared__ StereoPair s_pair;
    __shared__ uint32_t s_wsum[ST_WAVES];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const uint32_t n0 = p.n0[pr], n1 = p.n1[pr];
    if (over_limit(p, n0, n1)) {  // uniform over the workgroup
        if (tid == 0) {
            p.n_out[pr] = 0;
            p.status[pr] = ST_STATUS_OVER_LIMIT;
        }
        return;
    }
    if (tid == 0) make_stereo_pair(p.pos3 + 6ll * pr, p.r9 + 18ll * pr, p.intr4 + 8ll * pr, s_pair);
    __syncthreads();
    const uint32_t nm = min(p.n_matches[pr], p.match_cap), n_masked = p.n_masked[pr];
    const mage_keypoint* kp0 = p.kp0 + pr * p.pitch0;
    const mage_keypoint* kp1 = p.kp1 + pr * p.pitch1;
    mage_stereo_point* out = p.out + (long long)pr * p.cap;
    uint32_t nacc = 0;
    for (uint32_t c0 = 0; c0 < nm; c0 += ST_THREADS) {
        const uint32_t g = c0 + tid;
        bool acc = false;
        mage_stereo_point o{};
        if (g < nm) {
            const long long mi = (long long)pr * p.match_cap + g;
            const mage_dmatch m = p.matches[mi];
            int q = m.query_idx;
            const int t = m.train_idx;
            if (p.pack_index) {  // the matcher counted the masked keypoints: back to frame 0's index
                q = q >= 0 && (uint32_t)q < n_masked ? (int)p.pack_index[pr * p.pitch0 + q] : -1;
                p.matches[mi].query_idx = q;
            }
            uint8_t v = ST_BAD_INDEX;
            if (q >= 0 && (uint32_t)q < n0 && t >= 0 && (uint32_t)t < n1) {
                const mage_keypoint a = kp0[q], b = kp1[t];
                bool parallel;
                v = stereo_match_geometry(s_pair, p.two_max_epipolar, p.min_ratio, a.x, a.y, a.octave, b.x, b.y, b.octave,
                                          o.position, parallel);
                o.query_idx = q;
                o.train_idx = t;
                o.distance = m.distance;
                o.near_parallel = parallel ? 1u : 0u;
            }
            p.verdict[mi] = v;
            acc = v == ST_ACCEPTED;
        }
        uint32_t total;
        const uint32_t pos = nacc + block_prefix<ST_WAVES>(acc, s_wsum, &total);
        if (acc && pos < p.cap) out[pos] = o;
        nacc += total;
    }
    const uint32_t n = min(nacc, p.cap);
    if (tid == 0) {
        p.n_out[pr] = n;
        p.status[pr] = nacc > p.cap ? ST_STATUS_OVER_CAP : 0u;
    }
    // the bundler's inputs from the compacted records (this workgroup's own stores, visible after
    // the barrier): the points, then frame 0's observations, then frame 1's
    __syncthreads();
    const float info = track::refinement_confidence(1);
    float* bp = p.ba_points + 3ll * pr * p.cap;
    const long long ob = 2ll * pr * p.cap;
    for (uint32_t i = tid; i < n; i += ST_THREADS) {
        const mage_stereo_point r = out[i];
        for (int k = 0; k < 3; k++) bp[3 * i + k] = r.position[k];
        const mage_keypoint a = kp0[r.query_idx], b = kp1[r.train_idx];
        const long long o0 = ob + i, o1 = ob + n + i;
        p.ba_uv[2 * o0] = a.x;
        p.ba_uv[2 * o0 + 1] = a.y;
        p.ba_uv[2 * o1] = b.x;
        p.ba_uv[2 * o1 + 1] = b.y;
        p.ba_cam[o0] = 0u;
        p.ba_cam[o1] = 1u;
        p.ba_pt[o0] = i;
        p.ba_pt[o1] = i;
        p.ba_info[o0] = info;
        p.ba_info[o1] = info;
    }
}

}  // namespace
}  // namespace mage

extern "C" mage_status mage_stereo_init_triangulate_batch_device(
    const mage_stereo_init_settings* settings, uint32_t pairs, const float* d_pos3, const float* d_r9,
    const float* d_intr4, const int32_t* d_crop, const mage_keypoint* d_kp0, const uint8_t* d_desc0, int64_t pitch0,
    const uint32_t* d_n0, const mage_keypoint* d_kp1, const uint8_t* d_desc1, int64_t pitch1, const uint32_t* d_n1,
    uint8_t* d_mask0, uint32_t* d_n_masked, mage_dmatch* d_matches, uint32_t match_cap, uint32_t* d_n_matches,
    uint8_t* d_verdict, mage_stereo_point* d_out, uint32_t cap, uint32_t* d_n_out, float* d_ba_points, float* d_ba_uv,
    uint32_t* d_ba_cam, uint32_t* d_ba_pt, float* d_ba_info, uint32_t* d_status, void* d_scratch, mage_stream stream)
{
    using namespace mage;
    const char* why = stereoinit::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    if (pairs == 0) return MAGE_OK;
    MAGE_REQUIRE(d_pos3 && d_r9 && d_intr4 && d_crop && d_kp0 && d_n0 && d_kp1 && d_n1 && d_mask0 && d_n_masked &&
                     d_matches && d_n_matches && d_verdict && d_out && d_n_out && d_ba_points && d_ba_uv && d_ba_cam &&
                     d_ba_pt && d_ba_info && d_status,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(!d_desc0 || (d_desc1 && d_scratch), MAGE_EINVAL, "the matcher needs both descriptor sets and the scratch");
    MAGE_REQUIRE(pitch0 > 0 && pitch1 > 0 && match_cap > 0 && cap > 0, MAGE_EINVAL,
                 "pitches and capacities must be positive");
    MAGE_REQUIRE(!d_desc0 || (((uintptr_t)d_desc0 | (uintptr_t)d_desc1 | (uintptr_t)d_scratch) & 15) == 0, MAGE_EINVAL,
                 "descriptors and scratch must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    StParams p{};
    p.two_max_epipolar = 2 * settings->max_epipolar_error;
    p.min_ratio = settings->min_accepted_distance_ratio;
    p.pos3 = d_pos3;
    p.r9 = d_r9;
    p.intr4 = d_intr4;
    p.crop = d_crop;
    p.kp0 = d_kp0;
    p.kp1 = d_kp1;
    p.desc0 = d_desc0;
    p.pitch0 = pitch0;
    p.pitch1 = pitch1;
    p.n0 = d_n0;
    p.n1 = d_n1;
    p.mask0 = d_mask0;
    p.n_masked = d_n_masked;
    if (d_desc0) {  // scratch: [pairs x pitch0 x 32 bytes of descriptors][pairs x pitch0 indices]
        p.pack_desc = static_cast<uint8_t*>(d_scratch);
        p.pack_index = reinterpret_cast<uint32_t*>(p.pack_desc + 32ull * pairs * (uint64_t)pitch0);
    }
    p.matches = d_matches;
    p.match_cap = match_cap;
    p.n_matches = d_n_matches;
    p.verdict = d_verdict;
    p.out = d_out;
    p.cap = cap;
    p.n_out = d_n_out;
    p.ba_points = d_ba_points;
    p.ba_uv = d_ba_uv;
    p.ba_cam = d_ba_cam;
    p.ba_pt = d_ba_pt;
    p.ba_info = d_ba_info;
    p.status = d_status;
    launch("stereoinit.crop_mask", stereo_crop_mask_kernel, dim3(pairs), dim3(ST_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    if (d_desc0) {
        const mage_status r = mage_hamming_match_batch_device(p.pack_desc, 32 * pitch0, d_n_masked, d_desc1, 32 * pitch1,
                                                              d_n1, pairs, settings->max_hamming_distance,
                                                              settings->min_hamming_difference, d_matches, match_cap,
                                                              d_n_matches, stream);
        if (r != MAGE_OK) return r;
    }
    launch("stereoinit.triangulate", stereo_triangulate_kernel, dim3(pairs), dim3(ST_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

extern "C" mage_status mage_stereo_init_triangulate(const mage_stereo_init_settings* settings, const float* pos3,
                                                    const float* r9, const float* intr4, const int32_t crop_xywh[4],
                                                    const mage_keypoint* kp0, const uint8_t* desc0, uint32_t n0,
                                                    const mage_keypoint* kp1, const uint8_t* desc1, uint32_t n1,
                                                    mage_dmatch* matches, uint32_t match_cap, uint32_t* n_matches,
                                                    uint8_t* mask0, uint32_t* n_masked, uint8_t* verdict,
                                                    mage_stereo_point* out, uint32_t cap, uint32_t* n_out,
                                                    float* ba_points, float* ba_uv, uint32_t* ba_cam, uint32_t* ba_pt,
                                                    float* ba_info, uint32_t* status, int device)
{
    using namespace mage;
    const char* why = stereoinit::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(pos3 && r9 && intr4 && crop_xywh && n_matches && n_masked && n_out && status, MAGE_EINVAL, "null argument");
    const bool match = desc0 != nullptr;
    MAGE_REQUIRE(!match || (desc1 && match_cap > 0), MAGE_EINVAL,
                 "the matcher needs both descriptor sets and room for a match");
    const uint32_t n_in = match ? 0u : *n_matches;
    MAGE_REQUIRE(n_in <= match_cap, MAGE_EINVAL, "more matches than match_cap");
    MAGE_REQUIRE((n0 == 0 || (kp0 && mask0)) && (n1 == 0 || kp1) && (match_cap == 0 || (matches && verdict)) &&
                     (cap == 0 || (out && ba_points && ba_uv && ba_cam && ba_pt && ba_info)),
                 MAGE_EINVAL, "null argument");
    *n_masked = 0;
    *n_out = 0;
    *status = 0;
    if (match) *n_matches = 0;
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    if (n0 > (uint32_t)stereoinit::ST_MAX_KP || n1 > (uint32_t)stereoinit::ST_MAX_KP) {  // nothing else is written
        *status = stereoinit::ST_STATUS_OVER_LIMIT;
        return MAGE_OK;
    }
    HostScratch* sp = host_scratch(device, SCRATCH_STEREOINIT);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [poses][crop][kp0][kp1][desc0][desc1][counts][matches] | [mask][verdicts][records]
    // [ba points, uv, cam, pt, info] | [matcher scratch]: the inputs in one H2D copy, counts to ba
    // info back in one D2H copy
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint32_t p0 = std::max(n0, 1u), p1 = std::max(n1, 1u), mc = std::max(match_cap, 1u), dcap = std::max(cap, 1u);
    const size_t opose = 0, ocrop = al(opose + 4 * 32), okp0 = al(ocrop + 16), okp1 = al(okp0 + 28ull * p0),
                 od0 = al(okp1 + 28ull * p1), od1 = al(od0 + 32ull * p0), ocnt = al(od1 + 32ull * p1),
                 omat = al(ocnt + 4 * 6), omask = al(omat + 16ull * mc), over = al(omask + p0), oout = al(over + mc),
                 obp = al(oout + sizeof(mage_stereo_point) * (size_t)dcap), ouv = al(obp + 12ull * dcap),
                 ocam = al(ouv + 16ull * dcap), opt = al(ocam + 8ull * dcap), oinfo = al(opt + 8ull * dcap),
                 oscr = al(oinfo + 8ull * dcap), total = al(oscr + 36ull * p0);
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(oscr)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    std::memset(h, 0, omask);
    float* hp = reinterpret_cast<float*>(h + opose);
    std::memcpy(hp, pos3, 4 * 6);
    std::memcpy(hp + 6, r9, 4 * 18);
    std::memcpy(hp + 24, intr4, 4 * 8);
    std::memcpy(h + ocrop, crop_xywh, 16);
    if (n0) std::memcpy(h + okp0, kp0, 28ull * n0);
    if (n1) std::memcpy(h + okp1, kp1, 28ull * n1);
    if (match && n0) std::memcpy(h + od0, desc0, 32ull * n0);
    if (match && n1) std::memcpy(h + od1, desc1, 32ull * n1);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(h + ocnt);  // n0, n1, n_masked, n_matches, n_out, status
    cnt[0] = n0;
    cnt[1] = n1;
    cnt[3] = n_in;
    if (n_in) std::memcpy(h + omat, matches, 16ull * n_in);
    MAGE_HIP(hipMemcpyAsync(b, h, omask, hipMemcpyHostToDevice, S.st));
    const float* dp = reinterpret_cast<const float*>(b + opose);
    uint32_t* dc = reinterpret_cast<uint32_t*>(b + ocnt);
    r = mage_stereo_init_triangulate_batch_device(
        settings, 1, dp, dp + 6, dp + 24, reinterpret_cast<const int32_t*>(b + ocrop),
        reinterpret_cast<const mage_keypoint*>(b + okp0), match ? reinterpret_cast<const uint8_t*>(b + od0) : nullptr, p0,
        dc, reinterpret_cast<const mage_keypoint*>(b + okp1), match ? reinterpret_cast<const uint8_t*>(b + od1) : nullptr,
        p1, dc + 1, reinterpret_cast<uint8_t*>(b + omask), dc + 2, reinterpret_cast<mage_dmatch*>(b + omat), mc, dc + 3,
        reinterpret_cast<uint8_t*>(b + over), reinterpret_cast<mage_stereo_point*>(b + oout), dcap, dc + 4,
        reinterpret_cast<float*>(b + obp), reinterpret_cast<float*>(b + ouv), reinterpret_cast<uint32_t*>(b + ocam),
        reinterpret_cast<uint32_t*>(b + opt), reinterpret_cast<float*>(b + oinfo), dc + 5, match ? b + oscr : nullptr, S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + ocnt, b + ocnt, oscr - ocnt, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    *n_masked = cnt[2];
    if (n0) std::memcpy(mask0, h + omask, n0);
    // match_cap == 0 ran with one spare record; a matcher that found more than match_cap kept the first
    const uint32_t nm = std::min(cnt[3], match_cap);
    if (match) {
        *n_matches = nm;
        if (nm) std::memcpy(matches, h + omat, 16ull * nm);
    }
    if (nm) std::memcpy(verdict, h + over, nm);
    // cap == 0 ran with one spare record: every accepted match is then over the capacity
    const uint32_t n = cap ? cnt[4] : 0;
    *status = cnt[5] | (cap == 0 && cnt[4] > 0 ? stereoinit::ST_STATUS_OVER_CAP : 0u);
    *n_out = n;
    if (n) {
        std::memcpy(out, h + oout, sizeof(mage_stereo_point) * (size_t)n);
        std::memcpy(ba_points, h + obp, 12ull * n);
        std::memcpy(ba_uv, h + ouv, 16ull * n);
        std::memcpy(ba_cam, h + ocam, 8ull * n);
        std::memcpy(ba_pt, h + opt, 8ull * n);
        std::memcpy(ba_info, h + oinfo, 8ull * n);
    }
    return MAGE_OK;
}
