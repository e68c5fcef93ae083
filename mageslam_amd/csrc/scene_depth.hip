// scene_depth.hip — CalculateBoundingPlaneDepthsForKeyframe (Core/MAGESLAM/Source/Tracking/
// BoundingPlaneDepths.cpp:16-87) on MI355X (gfx950), batched over frames: one launch, one workgroup
// per frame.
//   a. the threads stride over the frame's map points: each writes its point's sparse record
//      (ProjectUndistorted, :56-60) and, when the point's keypoint lies inside the region of interest
//      (:45-46), appends the depth (p - c) . f (:48) as an order-preserving key to the list in LDS.
//      The list's order depends on how the threads run; the two order statistics do not.
//   b. NearPlaneDepth and FarPlaneDepth (:69-75) are the keys of rank r_near ascending and r_far
//      descending: a most-significant-digit radix selection over the list, 8 bits per pass, both
//      ranks in the same four passes.  Each pass counts the keys that still carry a selection's
//      prefix into 256 bins with LDS atomics, scans the bins (a wave scan per 64 bins) and the one
//      bin that holds the rank extends the prefix.  After four passes the prefix is the key.  The
//      selection is exact, so the twin's std::nth_element (scene_depth.cpp) gives the same bits.
// All arithmetic is scene_math.hpp's, shared with the twin.  The only atomics are on LDS words;
// every loop is bounded by the frame's counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "scene_math.hpp"

namespace mage {
namespace {

using namespace scene;

// The host-buffer entry's scratch slot, after reloc_guided.hip's 11.
constexpr ScratchSlot SCRATCH_SCENEDEPTH = static_cast<ScratchSlot>(12);

constexpr int SD_THREADS = 1024;
constexpr int SD_BINS = 256;             // one radix digit
constexpr int SD_SCAN = 2 * SD_BINS;     // threads of the bin scan: one per (selection, bin)
constexpr int SD_SCAN_WAVES = SD_SCAN / kWave;
static_assert(SD_SCAN <= SD_THREADS && SD_BINS % kWave == 0, "the bin scan is one thread per bin, whole waves per selection");

struct SdParams {
    mage_bounding_depth_settings s;
    const float *pos3, *r9, *intr4;
    const uint32_t* size;
    const mage_keypoint* kp;
    int64_t kp_pitch;
    const uint32_t* n_kp;
    const float* map_xyzi;
    const int32_t* kp_index;
    int64_t point_pitch;
    const uint32_t* n_points;
    uint32_t cap;
    mage_depth_result* result;
    mage_projected_point* sparse;
};

__global__ __launch_bounds__(SD_THREADS) void scene_depth_kernel(SdParams p)
{
    __shared__ uint32_t s_keys[BD_MAX_POINTS];
    __shared__ uint32_t s_hist[2][SD_BINS];
    __shared__ uint32_t s_wsum[SD_SCAN_WAVES];
    __shared__ uint32_t s_prefix[2], s_rank[2];
    __shared__ uint32_t s_nvalid, s_status;
    const int64_t fr = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t n = p.n_points[fr];
    if (over_limit(n, p.cap)) {  // uniform over the workgroup
        if (tid == 0) p.result[fr] = over_limit_result(n);
        return;
    }
    if (tid == 0) {
        s_nvalid = 0;
        s_status = 0;
    }
    __syncthreads();
    const float* pos3 = p.pos3 + 3 * fr;
    const float* r9 = p.r9 + 9 * fr;
    const float* intr4 = p.intr4 + 4 * fr;
    const Camera cam = make_camera(p.s, pos3, r9, p.size[2 * fr], p.size[2 * fr + 1]);
    const uint32_t nkp = (uint32_t)min((int64_t)p.n_kp[fr], p.kp_pitch);
    const mage_keypoint* kp = p.kp + fr * p.kp_pitch;
    const float* map = p.map_xyzi + 4 * fr * p.point_pitch;
    const int32_t* kpi = p.kp_index + fr * p.point_pitch;
    mage_projected_point* sparse = p.sparse + fr * p.point_pitch;
    uint32_t flags = 0;
    for (uint32_t i = tid; i < n; i += SD_THREADS) {  // n <= cap <= min(point_pitch, BD_MAX_POINTS)
        const float xyzi[4] = {map[4 * i], map[4 * i + 1], map[4 * i + 2], map[4 * i + 3]};
        const int32_t k = kpi[i];
        if (k < 0 || (uint32_t)k >= nkp) {
            flags |= BD_STATUS_BAD_INDEX;
        } else if (in_region(cam, kp[k].x, kp[k].y)) {
            const float depth = depth_of(cam, xyzi);
            if (!(depth > 0.f)) flags |= BD_STATUS_NONPOSITIVE;
            s_keys[atomicAdd(&s_nvalid, 1u)] = key_of_bits(__float_as_uint(depth));  // at most one slot per point
        }
        sparse[i] = sparse_of(pos3, r9, intr4, xyzi, (int32_t)__float_as_uint(xyzi[3]));
    }
    if (flags) atomicOr(&s_status, flags);
    __syncthreads();
    const uint32_t nv = s_nvalid;
    if (nv == 0) {  // uniform
        if (tid == 0) p.result[fr] = make_result(0, n, s_status, 0.f, 0.f);
        return;
    }
    if (tid == 0) {
        s_prefix[0] = s_prefix[1] = 0;
        s_rank[0] = soft_rank(p.s.near_depth_softness, nv);
        s_rank[1] = nv - 1u - soft_rank(p.s.far_depth_softness, nv);  // rank r descending is rank nv - 1 - r ascending
    }
    __syncthreads();
    const int sel = tid / SD_BINS, bin = tid % SD_BINS, lane = tid % kWave, wave = tid / kWave;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int t = tid; t < 2 * SD_BINS; t += SD_THREADS) (&s_hist[0][0])[t] = 0;
        const uint32_t mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);  // the digits already chosen
        const uint32_t pre0 = s_prefix[0], pre1 = s_prefix[1];
        __syncthreads();
        for (uint32_t i = tid; i < nv; i += SD_THREADS) {
            const uint32_t k = s_keys[i], d = (k >> shift) & (SD_BINS - 1);
            if ((k & mask) == pre0) atomicAdd(&s_hist[0][d], 1u);
            if ((k & mask) == pre1) atomicAdd(&s_hist[1][d], 1u);
        }
        __syncthreads();
        // thread (sel, bin): the inclusive count of its selection's bins up to its own
        uint32_t h = 0, incl = 0, rank = 0;
        if (tid < SD_SCAN) {  // whole waves
            h = incl = s_hist[sel][bin];
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            if (lane == kWave - 1) s_wsum[wave] = incl;
            rank = s_rank[sel];
        }
        __syncthreads();
        if (tid < SD_SCAN) {
            for (int w = sel * (SD_BINS / kWave); w < wave; w++) incl += s_wsum[w];
            const uint32_t excl = incl - h;
            if (excl <= rank && rank < incl) {  // exactly one bin per selection: the rank is under the matching count
                s_prefix[sel] = (sel ? pre1 : pre0) | ((uint32_t)bin << shift);
                s_rank[sel] = rank - excl;
            }
        }
        __syncthreads();
    }
    if (tid == 0)
        p.result[fr] = make_result(nv, n, s_status, __uint_as_float(bits_of_key(s_prefix[0])),
                                   __uint_as_float(bits_of_key(s_prefix[1])));
}

}  // namespace
}  // namespace mage

extern "C" mage_status mage_bounding_plane_depths_batch_device(
    const mage_bounding_depth_settings* settings, uint32_t frames, const float* d_pos3, const float* d_r9,
    const float* d_intr4, const uint32_t* d_size, const mage_keypoint* d_kp, int64_t kp_pitch, const uint32_t* d_n_kp,
    const float* d_map_xyzi, const int32_t* d_kp_index, int64_t point_pitch, const uint32_t* d_n_points, uint32_t cap,
    mage_depth_result* d_result, mage_projected_point* d_sparse, mage_stream stream)
{
    using namespace mage;
    const char* why = scene::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    if (frames == 0) return MAGE_OK;
    MAGE_REQUIRE(d_pos3 && d_r9 && d_intr4 && d_size && d_kp && d_n_kp && d_map_xyzi && d_kp_index && d_n_points &&
                     d_result && d_sparse,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(kp_pitch > 0 && point_pitch > 0, MAGE_EINVAL, "pitches must be positive");
    MAGE_REQUIRE((int64_t)cap <= point_pitch, MAGE_EINVAL, "cap is over point_pitch");
    SdParams p{};
    p.s = *settings;
    p.pos3 = d_pos3;
    p.r9 = d_r9;
    p.intr4 = d_intr4;
    p.size = d_size;
    p.kp = d_kp;
    p.kp_pitch = kp_pitch;
    p.n_kp = d_n_kp;
    p.map_xyzi = d_map_xyzi;
    p.kp_index = d_kp_index;
    p.point_pitch = point_pitch;
    p.n_points = d_n_points;
    p.cap = cap;
    p.result = d_result;
    p.sparse = d_sparse;
    launch("scene.depth", scene_depth_kernel, dim3(frames), dim3(SD_THREADS), 0, (hipStream_t)stream, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

extern "C" mage_status mage_bounding_plane_depths(const mage_bounding_depth_settings* settings, const float* pos3,
                                                  const float* r9, const float* intr4, uint32_t width, uint32_t height,
                                                  const mage_keypoint* kp, uint32_t n_kp, const float* map_xyzi,
                                                  const int32_t* kp_index, uint32_t n_points, uint32_t cap,
                                                  mage_depth_result* result, mage_projected_point* sparse, int device)
{
    using namespace mage;
    const char* why = scene::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(pos3 && r9 && intr4 && result, MAGE_EINVAL, "null argument");
    MAGE_REQUIRE((n_kp == 0 || kp) && (n_points == 0 || (map_xyzi && kp_index)) && (cap == 0 || sparse), MAGE_EINVAL,
                 "null argument");
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    if (scene::over_limit(n_points, cap)) {  // nothing else is written
        *result = scene::over_limit_result(n_points);
        return MAGE_OK;
    }
    HostScratch* sp = host_scratch(device, SCRATCH_SCENEDEPTH);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [pose, intr, size, counts][kp][map][kp index] | [result][sparse]: the inputs in one
    // H2D copy, the outputs back in one D2H copy
    auto align256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint32_t pkp = std::max(n_kp, 1u), ppt = std::max(n_points, 1u);
    const size_t ohead = 0, okp = align256(ohead + 80), omap = align256(okp + sizeof(mage_keypoint) * (size_t)pkp),
                 oidx = align256(omap + 16ull * ppt), ores = align256(oidx + 4ull * ppt),
                 osp = align256(ores + sizeof(mage_depth_result)),
                 total = align256(osp + sizeof(mage_projected_point) * (size_t)ppt);
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(total)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    float* hf = reinterpret_cast<float*>(h + ohead);  // pos3, r9, intr4, then {width, height, n_kp, n_points}
    std::memcpy(hf, pos3, 12);
    std::memcpy(hf + 3, r9, 36);
    std::memcpy(hf + 12, intr4, 16);
    const uint32_t words[4] = {width, height, n_kp, n_points};
    std::memcpy(hf + 16, words, 16);
    if (n_kp) std::memcpy(h + okp, kp, sizeof(mage_keypoint) * (size_t)n_kp);
    if (n_points) {
        std::memcpy(h + omap, map_xyzi, 16ull * n_points);
        std::memcpy(h + oidx, kp_index, 4ull * n_points);
    }
    MAGE_HIP(hipMemcpyAsync(b, h, ores, hipMemcpyHostToDevice, S.st));
    const float* df = reinterpret_cast<const float*>(b + ohead);
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(df + 16);
    r = mage_bounding_plane_depths_batch_device(settings, 1, df, df + 3, df + 12, dw,
                                                reinterpret_cast<const mage_keypoint*>(b + okp), pkp, dw + 2,
                                                reinterpret_cast<const float*>(b + omap),
                                                reinterpret_cast<const int32_t*>(b + oidx), ppt, dw + 3, n_points,
                                                reinterpret_cast<mage_depth_result*>(b + ores),
                                                reinterpret_cast<mage_projected_point*>(b + osp), S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + ores, b + ores, total - ores, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    *result = *reinterpret_cast<const mage_depth_result*>(h + ores);
    if (n_points) std::memcpy(sparse, h + osp, sizeof(mage_projected_point) * (size_t)n_points);
    return MAGE_OK;
}
