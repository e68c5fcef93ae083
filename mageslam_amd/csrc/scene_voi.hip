// scene_voi.hip — CalculateVolumeOfInterest (Core/MAGESLAM/Source/VolumeOfInterest/
// VolumeOfInterest.cpp:45-259) on MI355X (gfx950), batched over problems (pose histories): one chain
// of launches on one stream, no host step, the grid's dimensions computed on the device.
//   voi_setup_kernel    one workgroup per problem: the keyframes' records (:45-61) into scratch, the
//                       box of their frusta (:99-136), every centroid's score against every keyframe
//                       in order (:144-157) and with them the seeds of the voxel minimum / maximum;
//   voi_minmax_kernel   per level, VOI_WGS workgroups per problem: workgroup 0 first writes the
//                       outcome of the level before (its box, counts, the result's bounds); every
//                       workgroup derives the level's grid from that box (:161-169) and walks the
//                       voxels with a grid-stride loop, one thread summing a voxel's keyframes in
//                       keyframe order (:172-191); the minimum and maximum go through integer
//                       atomics on order-preserving keys;
//   voi_box_kernel      per level: the threshold (:200) from the minimum and maximum, which need
//                       every workgroup's voxels, hence the kernel boundary; the voxels' values are
//                       computed again (no voxel array is kept), those above the threshold and, in
//                       workgroup 0, the centroids above it (:202-239) give the next box, again
//                       through key atomics;
//   voi_finish_kernel   one workgroup per problem: the last level's outcome.
// The next level needs the whole box, hence the boundary behind voi_box_kernel too: 2 + 2 x
// Iterations launches.  The box accumulators are double-buffered by level parity, so the workgroup
// that clears one set never races the workgroups that read the other.  The keyframes' records are
// staged through LDS VOI_CHUNK at a time, so n_kf is unbounded.  The trace records in the caller's
// memory are written as the chain goes; all arithmetic is scene_math.hpp's, shared with the twin
// (scene_voi.cpp), and min / max are order-independent on the keys, so the bytes are the twin's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "scene_math.hpp"

namespace mage {
namespace {

using namespace scene;

// The host-buffer entry's scratch slot, after scene_depth.hip's 12.
constexpr ScratchSlot SCRATCH_SCENEVOI = static_cast<ScratchSlot>(13);

constexpr int VOI_THREADS = 256;
constexpr int VOI_WGS = 64;     // workgroups per problem in the level kernels
constexpr int VOI_CHUNK = 128;  // keyframe records staged in LDS at a time (4 KB)

// A problem's accumulators in scratch.
struct VoiState {
    uint32_t vmin_key, vmax_key;  // minVoxelValue / maxVoxelValue, running on across the levels
    uint32_t stop;                // the level loop has ended
    uint32_t pad;
    uint32_t box[2][8];           // by level parity: 3 minimum keys, 3 maximum keys, voxels, centroids above
};

struct VoiParams {
    mage_voi_settings s;
    const float* kf_world;
    int64_t kf_pitch;
    const uint32_t* n_kf;
    const float* near_far;
    const mage_depth_result* depth_records;
    uint32_t n_depth_records;
    const uint32_t* depth_index;
    mage_voi_result* result;
    mage_voi_level* trace;
    VoiKf* kf;        // problems x kf_pitch
    float* kf_score;  // problems x kf_pitch
    VoiState* state;
    int level;        // the level index li of this launch; lod = iterations - li
};

__device__ inline uint32_t kf_count(const VoiParams& p, int pr) { return (uint32_t)min((int64_t)p.n_kf[pr], p.kf_pitch); }

// The sum of the n keyframes' scores at `point`, in keyframe order, for every thread that is
// `active`; the records go through LDS a chunk at a time (all threads of the workgroup call this).
__device__ inline float sum_scores(const VoiParams& p, const VoiKf* kf, uint32_t n, const float* point, bool active, VoiKf* s_kf)
{
    float v = 0.f;
    for (uint32_t base = 0; base < n; base += VOI_CHUNK) {
        const uint32_t m = min((uint32_t)VOI_CHUNK, n - base);
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < m * (sizeof(VoiKf) / 4); w += VOI_THREADS)
            reinterpret_cast<uint32_t*>(s_kf)[w] = reinterpret_cast<const uint32_t*>(kf + base)[w];
        __syncthreads();
        if (active)
            for (uint32_t k = 0; k < m; k++) v += voi_teardrop(p.s, s_kf[k], point);
    }
    return v;
}

__global__ __launch_bounds__(VOI_THREADS) void voi_setup_kernel(VoiParams p)
{
    __shared__ VoiKf s_kf[VOI_CHUNK];
    __shared__ uint32_t s_box[6], s_v[2];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = kf_count(p, pr);
    VoiState& st = p.state[pr];
    if (n == 0) {  // :91-94, the bounds and the trace untouched
        if (tid == 0) {
            p.result[pr].status = VOI_NO_KEYFRAMES;
            p.result[pr].levels_done = 0;
            st.stop = 1;
        }
        return;
    }
    VoiKf* kf = p.kf + pr * p.kf_pitch;
    float* score = p.kf_score + pr * p.kf_pitch;
    if (tid < 3) {
        s_box[tid] = key_of(FLT_MAX);
        s_box[3 + tid] = key_of(FLT_MIN);
    }
    if (tid < 2) s_v[tid] = key_of(tid ? FLT_MIN : FLT_MAX);
    if (p.trace)
        for (uint32_t w = tid; w < (uint32_t)p.s.iterations * (sizeof(mage_voi_level) / 4); w += VOI_THREADS)
            reinterpret_cast<uint32_t*>(p.trace + (int64_t)pr * p.s.iterations)[w] = 0;
    __syncthreads();
    for (uint32_t k = tid; k < n; k += VOI_THREADS) {
        float nd, fd, corners[8][3];
        const int64_t g = pr * p.kf_pitch + k;
        voi_depths(p.near_far ? p.near_far + 2 * pr * p.kf_pitch : nullptr, p.depth_records, p.n_depth_records,
                   p.depth_index ? p.depth_index + pr * p.kf_pitch : nullptr, k, nd, fd);
        VoiKf rec;
        voi_keyframe(p.s, p.kf_world + 12 * g, nd, fd, rec, corners);
        kf[k] = rec;
        for (int c = 0; c < 8; c++)
            for (int i = 0; i < 3; i++) {
                atomicMin(&s_box[i], key_of(corners[c][i]));
                atomicMax(&s_box[3 + i], key_of(corners[c][i]));
            }
    }
    __syncthreads();  // the records, written by this workgroup, are read back below
    for (uint32_t base = 0; base < n; base += VOI_THREADS) {
        const uint32_t a = base + tid;
        const bool active = a < n;
        float c[3] = {0.f, 0.f, 0.f};
        if (active)
            for (int i = 0; i < 3; i++) c[i] = kf[a].centroid[i];
        const float v = sum_scores(p, kf, n, c, active, s_kf);
        if (active) {
            score[a] = v;
            atomicMin(&s_v[0], key_of(v));
            atomicMax(&s_v[1], key_of(v));
        }
    }
    __syncthreads();
    if (tid == 0) {
        st.vmin_key = s_v[0];
        st.vmax_key = s_v[1];
        st.stop = 0;
        for (int i = 0; i < 6; i++) st.box[0][i] = s_box[i];
        st.box[0][6] = 1;  // level 0 starts from the frustum box as from a level that passed
        st.box[0][7] = 0;
        mage_voi_result r;
        for (int i = 0; i < 3; i++) {
            r.min[i] = float_of_key(s_box[i]);
            r.max[i] = float_of_key(s_box[3 + i]);
        }
        r.status = VOI_OK;
        r.levels_done = 0;
        p.result[pr] = r;
    }
}

// What level li starts from: false when the level loop has ended (before this launch, or because
// level li - 1 left nothing).  Workgroup 0's thread 0 writes level li - 1's outcome.
__device__ inline bool voi_enter_level(const VoiParams& p, int pr, int li, bool writer, float* bmin, float* bmax)
{
    VoiState& st = p.state[pr];
    if (st.stop) return false;
    const uint32_t* acc = st.box[li & 1];
    for (int i = 0; i < 3; i++) {
        bmin[i] = float_of_key(acc[i]);
        bmax[i] = float_of_key(acc[3 + i]);
    }
    const bool empty = acc[6] == 0 && acc[7] == 0;
    if (writer && li > 0) {
        if (p.trace) {
            mage_voi_level& L = p.trace[(int64_t)pr * p.s.iterations + li - 1];
            for (int i = 0; i < 3; i++) {
                L.box_min[i] = bmin[i];
                L.box_max[i] = bmax[i];
            }
            L.n_voxels = acc[6];
            L.n_centroids = acc[7];
        }
        if (empty) {
            p.result[pr].status = VOI_EMPTY;
            st.stop = 1;
        } else {
            for (int i = 0; i < 3; i++) {
                p.result[pr].min[i] = bmin[i];
                p.result[pr].max[i] = bmax[i];
            }
            p.result[pr].levels_done = (uint32_t)li;
        }
    }
    return !empty;
}

__global__ __launch_bounds__(VOI_THREADS) void voi_minmax_kernel(VoiParams p)
{
    __shared__ VoiKf s_kf[VOI_CHUNK];
    __shared__ uint32_t s_v[2];
    const int pr = blockIdx.y, tid = threadIdx.x, li = p.level;
    const bool writer = blockIdx.x == 0 && tid == 0;
    VoiState& st = p.state[pr];
    float bmin[3], bmax[3];
    if (!voi_enter_level(p, pr, li, writer, bmin, bmax)) return;  // uniform over the problem's workgroups
    const VoiGrid g = voi_grid(p.s, p.s.iterations - li, bmin, bmax);
    if (!g.ok) {
        if (writer) {
            p.result[pr].status = VOI_DEGENERATE;
            st.stop = 1;
        }
        return;
    }
    if (writer) {
        if (p.trace) {
            mage_voi_level& L = p.trace[(int64_t)pr * p.s.iterations + li];
            L.side = g.side;
            for (int i = 0; i < 3; i++) L.dims[i] = g.dims[i];
        }
        uint32_t* next = st.box[(li + 1) & 1];  // cleared for voi_box_kernel; nobody reads it in this launch
        for (int i = 0; i < 3; i++) {
            next[i] = key_of(FLT_MAX);
            next[3 + i] = key_of(FLT_MIN);
        }
        next[6] = next[7] = 0;
    }
    if (tid < 2) s_v[tid] = key_of(tid ? FLT_MIN : FLT_MAX);
    const uint32_t n = kf_count(p, pr);
    const VoiKf* kf = p.kf + pr * p.kf_pitch;
    for (uint32_t base = blockIdx.x * VOI_THREADS; base < g.count; base += VOI_WGS * VOI_THREADS) {  // uniform per workgroup
        const uint32_t v = base + tid;
        const bool active = v < g.count;
        float pt[3] = {0.f, 0.f, 0.f};
        if (active) voi_voxel_point(g, v, pt);
        const float value = sum_scores(p, kf, n, pt, active, s_kf);  // its first barrier orders s_v's initialisation
        if (active) {
            atomicMin(&s_v[0], key_of(value));
            atomicMax(&s_v[1], key_of(value));
        }
    }
    __syncthreads();
    if (tid == 0) {
        atomicMin(&st.vmin_key, s_v[0]);
        atomicMax(&st.vmax_key, s_v[1]);
    }
}

__global__ __launch_bounds__(VOI_THREADS) void voi_box_kernel(VoiParams p)
{
    __shared__ VoiKf s_kf[VOI_CHUNK];
    __shared__ uint32_t s_acc[8];
    const int pr = blockIdx.y, tid = threadIdx.x, li = p.level;
    const bool writer = blockIdx.x == 0 && tid == 0;
    VoiState& st = p.state[pr];
    if (st.stop) return;  // set by an earlier launch, or below by this one: the same decision either way
    const float vmin = float_of_key(st.vmin_key), vmax = float_of_key(st.vmax_key);
    const bool bad = !finite_f(vmin) || !finite_f(vmax);
    const int lod = p.s.iterations - li;
    const float thr = voi_threshold(p.s, lod, vmin, vmax);
    if (writer) {
        if (p.trace) {
            mage_voi_level& L = p.trace[(int64_t)pr * p.s.iterations + li];
            L.voxel_min = vmin;
            L.voxel_max = vmax;
            if (!bad) L.threshold = thr;
        }
        if (bad) {
            p.result[pr].status = VOI_DEGENERATE;
            st.stop = 1;
        }
    }
    if (bad) return;
    const uint32_t* acc = st.box[li & 1];  // the box this level started from
    float bmin[3], bmax[3];
    for (int i = 0; i < 3; i++) {
        bmin[i] = float_of_key(acc[i]);
        bmax[i] = float_of_key(acc[3 + i]);
    }
    const VoiGrid g = voi_grid(p.s, lod, bmin, bmax);  // ok: voi_minmax_kernel went through it
    if (tid < 8) s_acc[tid] = tid < 3 ? key_of(FLT_MAX) : (tid < 6 ? key_of(FLT_MIN) : 0u);
    const uint32_t n = kf_count(p, pr);
    const VoiKf* kf = p.kf + pr * p.kf_pitch;
    for (uint32_t base = blockIdx.x * VOI_THREADS; base < g.count; base += VOI_WGS * VOI_THREADS) {
        const uint32_t v = base + tid;
        const bool active = v < g.count;
        float pt[3] = {0.f, 0.f, 0.f};
        if (active) voi_voxel_point(g, v, pt);
        const float value = sum_scores(p, kf, n, pt, active, s_kf);
        if (active && value > thr) {
            atomicAdd(&s_acc[6], 1u);
            for (int i = 0; i < 3; i++) {
                atomicMin(&s_acc[i], key_of(pt[i] - g.half));
                atomicMax(&s_acc[3 + i], key_of(pt[i] + g.half));
            }
        }
    }
    __syncthreads();  // also orders s_acc's initialisation when the workgroup has no voxel
    if (blockIdx.x == 0) {  // :224-239, the centroids
        const float* score = p.kf_score + pr * p.kf_pitch;
        for (uint32_t k = tid; k < n; k += VOI_THREADS)
            if (score[k] > thr) {
                atomicAdd(&s_acc[7], 1u);
                for (int i = 0; i < 3; i++) {
                    atomicMin(&s_acc[i], key_of(kf[k].centroid[i] - g.half));
                    atomicMax(&s_acc[3 + i], key_of(kf[k].centroid[i] + g.half));
                }
            }
        __syncthreads();
    }
    uint32_t* next = st.box[(li + 1) & 1];
    if (tid < 3) atomicMin(&next[tid], s_acc[tid]);
    else if (tid < 6) atomicMax(&next[tid], s_acc[tid]);
    else if (tid < 8 && s_acc[tid]) atomicAdd(&next[tid], s_acc[tid]);
}

__global__ __launch_bounds__(kWave) void voi_finish_kernel(VoiParams p)
{
    float bmin[3], bmax[3];
    if (threadIdx.x == 0) voi_enter_level(p, blockIdx.x, p.level, true, bmin, bmax);
}

struct ScratchLayout {
    size_t kf, score, state, bytes;
};
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline ScratchLayout scratch_layout(uint64_t problems, uint64_t kf_pitch)
{
    ScratchLayout l;
    l.kf = 0;
    l.score = align256(l.kf + sizeof(VoiKf) * problems * kf_pitch);
    l.state = align256(l.score + 4 * problems * kf_pitch);
    l.bytes = align256(l.state + sizeof(VoiState) * problems);
    return l;
}

}  // namespace
}  // namespace mage

extern "C" uint64_t mage_volume_of_interest_scratch_bytes(uint32_t problems, uint32_t kf_pitch)
{
    return mage::scratch_layout(problems, kf_pitch).bytes;
}

extern "C" mage_status mage_volume_of_interest_batch_device(const mage_voi_settings* settings, uint32_t problems,
                                                            const float* d_kf_world, int64_t kf_pitch, const uint32_t* d_n_kf,
                                                            const float* d_near_far, const mage_depth_result* d_depth_records,
                                                            uint32_t n_depth_records, const uint32_t* d_depth_index,
                                                            mage_voi_result* d_result, mage_voi_level* d_trace,
                                                            void* d_scratch, mage_stream stream)
{
    using namespace mage;
    const char* why = scene::check_voi_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    if (problems == 0) return MAGE_OK;
    MAGE_REQUIRE(d_kf_world && d_n_kf && d_result && d_scratch, MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(d_near_far || (d_depth_index && (d_depth_records || n_depth_records == 0)), MAGE_EINVAL,
                 "depths are needed: pairs, or the depth stage's records and indices");
    MAGE_REQUIRE(kf_pitch > 0 && kf_pitch <= 0xFFFFFFFFll && problems <= 65535u, MAGE_EINVAL,
                 "kf_pitch must be positive and the problems at most 65535");
    MAGE_REQUIRE(((uintptr_t)d_scratch & 255) == 0, MAGE_EINVAL, "scratch must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    VoiParams p{};
    p.s = *settings;
    scene::voi_prepare(p.s);
    const ScratchLayout L = scratch_layout(problems, (uint64_t)kf_pitch);
    char* sb = static_cast<char*>(d_scratch);
    p.kf_world = d_kf_world;
    p.kf_pitch = kf_pitch;
    p.n_kf = d_n_kf;
    p.near_far = d_near_far;
    p.depth_records = d_depth_records;
    p.n_depth_records = n_depth_records;
    p.depth_index = d_near_far ? nullptr : d_depth_index;
    p.result = d_result;
    p.trace = d_trace;
    p.kf = reinterpret_cast<VoiKf*>(sb + L.kf);
    p.kf_score = reinterpret_cast<float*>(sb + L.score);
    p.state = reinterpret_cast<VoiState*>(sb + L.state);
    launch("voi.setup", voi_setup_kernel, dim3(problems), dim3(VOI_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    for (int li = 0; li < p.s.iterations; li++) {
        p.level = li;
        launch("voi.minmax", voi_minmax_kernel, dim3(VOI_WGS, problems), dim3(VOI_THREADS), 0, st, p);
        MAGE_HIP(hipGetLastError());
        launch("voi.box", voi_box_kernel, dim3(VOI_WGS, problems), dim3(VOI_THREADS), 0, st, p);
        MAGE_HIP(hipGetLastError());
    }
    p.level = p.s.iterations;
    launch("voi.finish", voi_finish_kernel, dim3(problems), dim3(kWave), 0, st, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

extern "C" mage_status mage_volume_of_interest(const mage_voi_settings* settings, const float* kf_world, const float* near_far,
                                               const mage_depth_result* depth_records, uint32_t n_depth_records,
                                               const uint32_t* depth_index, uint32_t n_kf, mage_voi_result* result,
                                               mage_voi_level* trace, int device)
{
    using namespace mage;
    const char* why = scene::check_voi_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(result && (n_kf == 0 || (kf_world && (near_far || (depth_index && (depth_records || n_depth_records == 0))))),
                 MAGE_EINVAL, "null argument");
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    if (n_kf == 0) {  // the bounds and the trace untouched
        result->status = scene::VOI_NO_KEYFRAMES;
        result->levels_done = 0;
        return MAGE_OK;
    }
    HostScratch* sp = host_scratch(device, SCRATCH_SCENEVOI);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // the depths as pairs on the host; device layout [count][matrices][pairs] | [result][trace] | [scratch]
    std::vector<float> pairs(2 * (size_t)n_kf);
    for (uint32_t k = 0; k < n_kf; k++)
        scene::voi_depths(near_far, depth_records, n_depth_records, depth_index, k, pairs[2 * k], pairs[2 * k + 1]);
    const size_t levels = (size_t)settings->iterations;
    const size_t ocnt = 0, okf = align256(ocnt + 4), onf = align256(okf + 48ull * n_kf), ores = align256(onf + 8ull * n_kf),
                 otr = align256(ores + sizeof(mage_voi_result)), oscr = align256(otr + sizeof(mage_voi_level) * levels),
                 total = oscr + scratch_layout(1, n_kf).bytes;
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(oscr)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    std::memcpy(h + ocnt, &n_kf, 4);
    std::memcpy(h + okf, kf_world, 48ull * n_kf);
    std::memcpy(h + onf, pairs.data(), 8ull * n_kf);
    MAGE_HIP(hipMemcpyAsync(b, h, ores, hipMemcpyHostToDevice, S.st));
    r = mage_volume_of_interest_batch_device(settings, 1, reinterpret_cast<const float*>(b + okf), n_kf,
                                             reinterpret_cast<const uint32_t*>(b + ocnt),
                                             reinterpret_cast<const float*>(b + onf), nullptr, 0, nullptr,
                                             reinterpret_cast<mage_voi_result*>(b + ores),
                                             reinterpret_cast<mage_voi_level*>(b + otr), b + oscr, S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + ores, b + ores, oscr - ores, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    *result = *reinterpret_cast<const mage_voi_result*>(h + ores);
    if (trace && levels) std::memcpy(trace, h + otr, sizeof(mage_voi_level) * levels);
    return MAGE_OK;
}
