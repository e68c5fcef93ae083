// loopclose.hip — the mapping thread's cheap loop closure on MI355X (gfx950): CheapLoopClosure
// (Tasks/MappingWorker.cpp:20-73), InsertKeyframe's effect on the points it associated
// (Map/ThreadSafeMap.cpp:242-249) and TryConnectMapPoints (ThreadSafeMap.cpp:715-787), three launches
// chained on one stream, and the map-point refresh they share.
//
// MapPoint::AddKeyframeAssociation (Map/MapPoint.cpp:35-46) recomputes a point's representative
// descriptor (:80-130), mean viewing direction and dMin / dMax (:132-155) after every association; a
// point taken in one keyframe is offered to the next one with that new state.  refresh_point is
// that recomputation by one wave:
//   representative   lane a sums the Hamming distances of observation a to all n observations (an
//                    integer sum: the reference's float sum of integers is exact below 2^24, which
//                    MAGE_MP_MAX_OBS keeps); the first strictly smallest sum is the unsigned minimum
//                    of sum << 16 | a over the wave (xor shuffles: min commutes, every lane ends
//                    with the same key);
//   view direction   a float sum is not associative, so it is taken in observation order: the
//                    lanes normalise 64 observations' P - C at once, then every lane adds the 64
//                    vectors in lane order (a broadcast shuffle per term) — each lane holds the
//                    sequential loop's sum;
//   dMin / dMax      lane 0, from the representative observation (loopclose_math.hpp finish_state).
// The launches:
//   close    one workgroup per problem: the sample by index arithmetic (loopclose_math.hpp
//            make_sampler), the refusal of a problem whose observation pitch is too small, the
//            places whose point the new keyframe already holds, then keyframe_take.hpp's staging,
//            gate (one thread per point, compacted in order), gather and in-order take;
//   apply    one wave per (problem, place): a point the closure associated gains the new keyframe's
//            observation and is refreshed;
//   connect  one workgroup per problem walks the covisible keyframes in order: stage the keyframe,
//            gate the closure's points under their current states, gather and take in order, then a
//            wave per taken point appends the observation and refreshes, and a barrier ends the
//            keyframe.  The keyframes of a problem depend on each other through those states, so
//            they are not spread over workgroups.
// Only commuting integer atomics, barriers, wave shuffles and plain stores: nothing depends on the
// order in which threads run.  Every loop is bounded by the counts, which the entries bound by the
// pitches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "keyframe_take.hpp"
#include "loopclose_math.hpp"

namespace mage {
namespace {

using namespace loopclose;

// The host-buffer entry's scratch slot, after scene_voi.hip's (common.hpp stays as it is).
constexpr ScratchSlot SCRATCH_LOOPCLOSE = static_cast<ScratchSlot>(14);

constexpr int LC_THREADS = 256;
constexpr int LC_WAVES = LC_THREADS / kWave;  // points per workgroup
static_assert(MAGE_MP_MAX_OBS <= (1 << 16), "an observation index must fit the key's low 16 bits");
static_assert((uint64_t)MAGE_MP_MAX_OBS * 256 <= (1ull << 24), "the summed distance must stay exact in float");

struct RefreshParams {
    Tables t;
    uint32_t n_points;
    const float* positions;
    const mage_map_point_obs* obs;
    long long obs_pitch;
    const uint32_t* n_obs;
    mage_map_point_state* state;
    uint32_t* status;
};

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v)
{
    for (int off = 32; off; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
        const unsigned long long o = (unsigned long long)hi << 32 | lo;
        v = o < v ? o : v;
    }
    return v;
}

// The refresh of one point by one wave (all 64 lanes call it; see the file header): position P, its
// n observations o[0 .. n), 16-byte aligned; lane 0 writes *out.
__device__ __forceinline__ void refresh_point(const Tables& t, const float* P, const mage_map_point_obs* o, int n,
                                              mage_map_point_state* out)
{
    const int lane = threadIdx.x & 63;
    const float Pv[3] = {P[0], P[1], P[2]};
    mage_map_point_state st;
    if (n == 0) {
        empty_state(Pv, st);
        if (lane == 0) *out = st;
        return;
    }
    unsigned long long key = ~0ull;
    float m[3] = {0.f, 0.f, 0.f};
    for (int a0 = 0; a0 < n; a0 += kWave) {
        const int a = a0 + lane;
        float v[3] = {0.f, 0.f, 0.f};
        if (a < n) {
            const uint4 d0 = *reinterpret_cast<const uint4*>(o[a].desc), d1 = *reinterpret_cast<const uint4*>(o[a].desc + 16);
            uint32_t sum = 0;
            for (int b = 0; b < n; b++) sum += hamming256(d0, d1, o[b].desc);
            const unsigned long long k = (unsigned long long)sum << 16 | (uint32_t)a;
            key = k < key ? k : key;
            const float C[3] = {o[a].centre[0], o[a].centre[1], o[a].centre[2]};
            view_direction(Pv, C, v);
        }
        const int cnt = min(kWave, n - a0);
        for (int l = 0; l < cnt; l++)
            for (int j = 0; j < 3; j++) m[j] = m[j] + __shfl(v[j], l);
    }
    const int rep = (int)(wave_min(key) & 0xFFFFull);
    if (lane == 0) {
        const float C[3] = {o[rep].centre[0], o[rep].centre[1], o[rep].centre[2]};
        finish_state(t, Pv, m, C, o[rep].octave, rep, n, st);
        *out = st;
    }
}

__global__ __launch_bounds__(LC_THREADS) void map_points_refresh_kernel(RefreshParams p)
{
    const uint32_t i = blockIdx.x * LC_WAVES + (threadIdx.x >> 6);  // uniform over the wave
    if (i >= p.n_points) return;
    const uint32_t n = p.n_obs[i];
    if ((long long)n > p.obs_pitch) {
        if ((threadIdx.x & 63) == 0) atomicOr(p.status, 1u);
        return;
    }
    refresh_point(p.t, p.positions + 3ll * i, p.obs + (long long)i * p.obs_pitch, (int)n, p.state + i);
}

// ------------------------------------------------------------------------------------------
// The whole step: closure, its refresh, connect (see the file header).
// ------------------------------------------------------------------------------------------
using newpoints::Frame;

struct LcParams {
    Consts c;
    kt::Search closure, connect;
    mage_loop_closure_batch b;
};

// The workgroup's LDS: the staged keyframe and, by place in the sample, whether the keyframe
// already holds the point and the keypoint the point took in it.  About 74 KiB of the CU's 160.
struct LcShared {
    kt::Shared k;
    int took[LC_MAX_POINTS];
    int lst[LC_MAX_POINTS];  // connect: the places the closure associated, in order
    uint8_t has[LC_MAX_POINTS];
    uint32_t n_taken;
};

// One problem's slice of the batch.
struct LcProblem {
    uint32_t n_map, n_kf, L;
    Sampler sm;
    mage_map_point_state* state;
    mage_map_point_obs* obs;
    long long obs_pitch;
};

__device__ __forceinline__ LcProblem problem_of(const LcParams& p, uint32_t prob, uint32_t n_map)
{
    const mage_loop_closure_batch& b = p.b;
    LcProblem q;
    q.n_map = n_map;
    q.n_kf = b.d_n_kf[prob];
    q.sm = make_sampler(n_map, p.c.max_points, b.d_offset[prob]);
    q.L = q.sm.count;
    q.state = b.d_state + (long long)prob * b.map_pitch;
    q.obs = b.d_obs + (long long)prob * b.map_pitch * b.obs_pitch;
    q.obs_pitch = b.obs_pitch;
    return q;
}

// Per place: the staged keyframe holds the point (HasMapPoint / IsAssociatedToMapPoint), nothing
// taken yet.  Plain stores of the same value: commuting.  The caller's next barriers (the
// staging's) publish them.
__device__ __forceinline__ void mark_held(const LcProblem& q, LcShared& s, const int32_t* point, uint32_t nkp)
{
    for (int j = threadIdx.x; j < LC_MAX_POINTS; j += kt::KT_THREADS) {
        s.has[j] = 0;
        s.took[j] = -1;
    }
    if (threadIdx.x == 0) s.n_taken = 0;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < nkp; t += kt::KT_THREADS) {
        const int32_t i = point[t];
        if (i < 0 || (uint32_t)i >= q.n_map) continue;
        const int j = sample_slot(q.sm, (uint32_t)i);
        if (j >= 0) s.has[j] = 1;
    }
}

// The staged keyframe is offered `count` points in order, point i of them at place places[i] of the
// sample (places == nullptr: place i): ProjectMapPointIntoCurrentFrame for each under the mask the
// earlier ones left.  Records and verdicts at rec[place * stride]; s.took[place] and s.n_taken.
__device__ __forceinline__ void offer_points(const LcParams& p, const kt::Search& search, const LcProblem& q, LcShared& s,
                                             const Frame& frame, const float* intr, const uint8_t* kdesc, int count,
                                             const int* places, long long stride, mage_loop_closure_assoc* rec,
                                             uint8_t* verdict)
{
    const auto desc_of = [&](int j) {
        const long long idx = sample_index(q.sm, (uint32_t)j);
        return q.obs[idx * q.obs_pitch + q.state[idx].rep].desc;
    };
    for (int c0 = 0; c0 < count; c0 += kt::KT_THREADS) {
        const int i = c0 + threadIdx.x;
        bool pass = false;
        float px = 0.f, py = 0.f;
        int oc = 0, j = 0;
        if (i < count) {
            j = places ? places[i] : i;
            uint8_t vd = LC_HAS_POINT;
            if (!s.has[j]) {
                const mage_map_point_state st = q.state[sample_index(q.sm, (uint32_t)j)];
                vd = gate_point(p.c.gate, frame, intr, st, px, py, oc, pass);
            }
            if (!pass) {
                rec[j * stride] = mage_loop_closure_assoc{px, py, oc, -1};
                verdict[j * stride] = vd;
            }
        }
        const int cnt = kt::compact(s.k, pass, px, py, j, oc);
        kt::take_in_order(search, kdesc, s.k, cnt, desc_of, [&](int i, bool ok, int t) {
            const int j = s.k.pi[i];
            rec[j * stride] = mage_loop_closure_assoc{s.k.px[i], s.k.py[i], s.k.po[i], ok ? t : -1};
            verdict[j * stride] = ok ? (uint8_t)LC_ASSOCIATED : (uint8_t)LC_NO_MATCH;
            if (ok) {
                s.took[j] = t;
                atomicAdd(&s.n_taken, 1u);
            }
        });
    }
}

// MapPoint::AddKeyframeAssociation (MapPoint.cpp:35-46) by one wave: the keyframe's observation
// (descriptor, centre C, octave, id) becomes the point's last one, then the refresh.  The record's
// 16 words are written by 16 lanes; the fence and the wave barrier publish them to the lanes that
// read them back.
__device__ __forceinline__ void append_and_refresh(const Tables& t, mage_map_point_state* st, mage_map_point_obs* o,
                                                   const uint8_t* desc, const float* C, int octave, int id)
{
    const int lane = threadIdx.x & 63, n = st->n_obs;
    if (lane < 16) {
        uint32_t w = 0;
        if (lane < 8)
            w = reinterpret_cast<const uint32_t*>(desc)[lane];
        else if (lane < 11)
            w = __float_as_uint(lane == 8 ? C[0] : lane == 9 ? C[1] : C[2]);  // no indexed read: C may be in registers
        else if (lane == 11)
            w = (uint32_t)octave;
        else if (lane == 12)
            w = (uint32_t)id;
        reinterpret_cast<uint32_t*>(o + n)[lane] = w;
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    refresh_point(t, st->pos, o, n + 1, st);
}

// Closure: one workgroup per problem.  Samples by index arithmetic, refuses a problem whose
// observation pitch is too small, offers the sample to the new keyframe.
__global__ __launch_bounds__(kt::KT_THREADS) void loop_close_kernel(LcParams p)
{
    __shared__ LcShared s;
    __shared__ Frame s_frame;
    const mage_loop_closure_batch& b = p.b;
    const int tid = threadIdx.x;
    const uint32_t prob = blockIdx.x;
    const uint32_t n_map = b.d_n_map[prob], n_ki = b.d_n_ki[prob];
    uint32_t status = 0;
    bool run = b.d_n_keyframes[prob] >= p.c.min_keyframes;  // MappingWorker.cpp:22-25
    if (run && ((long long)n_map > b.map_pitch || b.d_n_kf[prob] > b.kf_slots)) {
        status = MAGE_LC_STATUS_OVER_LIMIT;
        run = false;
    }
    LcProblem q = problem_of(p, prob, run ? n_map : 0u);
    int full = 0;
    for (uint32_t j = tid; j < q.L; j += kt::KT_THREADS) {
        const long long n = q.state[sample_index(q.sm, j)].n_obs;
        if (n < 0 || n + 1 + (long long)q.n_kf > q.obs_pitch) full = 1;
    }
    if (__syncthreads_or(full)) {
        status |= MAGE_LC_STATUS_OBS_FULL;
        q.L = 0;
    }
    const bool ki_over = n_ki > (uint32_t)LC_MAX_KP || (long long)n_ki > b.ki_pitch;
    if (q.L && ki_over) status |= MAGE_LC_STATUS_OVER_LIMIT;  // nothing sampled: nothing is looked at
    uint32_t* counts = b.d_counts + 3ll * prob;
    if (tid == 0) {
        counts[0] = q.L;
        counts[1] = 0;
        counts[2] = 0;
        b.d_status[prob] = status;
    }
    if (q.L == 0) return;  // uniform over the workgroup
    const long long out0 = (long long)prob * p.c.max_points;
    for (uint32_t j = tid; j < q.L; j += kt::KT_THREADS) {
        b.d_sample_index[out0 + j] = sample_index(q.sm, j);
        if (ki_over) b.d_closure[out0 + j] = mage_loop_closure_assoc{0.f, 0.f, 0, -1};
    }
    if (ki_over) return;
    const int32_t* point = b.d_ki_point + (long long)prob * b.ki_pitch;
    const mage_keypoint* kp = b.d_ki_kp + (long long)prob * b.ki_pitch;
    const float* intr = b.d_ki_intr4 + 4ll * prob;
    mark_held(q, s, point, n_ki);
    kt::stage_keyframe(
        p.closure.band_scale, (int)n_ki, kp, s.k, [&](int t) { return point[t] < 0; },
        [&] {
            Frame f;
            newpoints::make_frame(b.d_ki_pos3 + 3ll * prob, b.d_ki_r9 + 9ll * prob, intr, f);
            s_frame = f;
        });
    offer_points(p, p.closure, q, s, s_frame, intr, b.d_ki_desc + 32ll * prob * b.ki_pitch, (int)q.L, nullptr, 1,
                 b.d_closure + out0, b.d_closure_verdict + out0);
    uint8_t* mask = b.d_ki_mask + (long long)prob * b.ki_pitch;
    for (uint32_t t = tid; t < n_ki; t += kt::KT_THREADS) mask[t] = mask_bit(s.k.m, (int)t) ? 1 : 0;
    if (tid == 0) counts[1] = s.n_taken;
}

// InsertKeyframe's associations (ThreadSafeMap.cpp:242-249): one wave per (problem, place); a point
// the closure associated gains the new keyframe's observation and is refreshed.
__global__ __launch_bounds__(LC_THREADS) void loop_close_apply_kernel(LcParams p)
{
    const mage_loop_closure_batch& b = p.b;
    const uint32_t prob = blockIdx.y, j = blockIdx.x * LC_WAVES + (threadIdx.x >> 6);  // uniform over the wave
    if (j >= b.d_counts[3ll * prob]) return;
    const int t = b.d_closure[(long long)prob * p.c.max_points + j].keypoint;
    if (t < 0) return;
    const LcProblem q = problem_of(p, prob, b.d_n_map[prob]);
    const long long idx = sample_index(q.sm, j), k0 = (long long)prob * b.ki_pitch;
    Frame f;
    newpoints::make_frame(b.d_ki_pos3 + 3ll * prob, b.d_ki_r9 + 9ll * prob, b.d_ki_intr4 + 4ll * prob, f);
    append_and_refresh(p.c.tables, q.state + idx, q.obs + idx * q.obs_pitch, b.d_ki_desc + 32ll * (k0 + t), f.C,
                       b.d_ki_kp[k0 + t].octave, b.d_ki_id[prob]);
}

// Connect: one workgroup per problem walks its covisible keyframes in order.  A keyframe reads the
// states the keyframes before it left (global memory, published by the barrier that ends each
// keyframe), so the order across keyframes is the reference's; within a keyframe the in-order take
// is resolve_in_order's, and the refreshes of one keyframe touch distinct points.
__global__ __launch_bounds__(kt::KT_THREADS) void loop_connect_kernel(LcParams p)
{
    __shared__ LcShared s;
    __shared__ Frame s_frame;
    const mage_loop_closure_batch& b = p.b;
    const int tid = threadIdx.x;
    const uint32_t prob = blockIdx.x;
    uint32_t* counts = b.d_counts + 3ll * prob;
    if (counts[0] == 0) return;  // refused, or nothing sampled
    const LcProblem q = problem_of(p, prob, b.d_n_map[prob]);
    if (q.n_kf == 0) return;
    const long long out0 = (long long)prob * p.c.max_points;
    const mage_loop_closure_assoc* closure = b.d_closure + out0;
    int n_closed = 0;
    for (uint32_t c0 = 0; c0 < q.L; c0 += kt::KT_THREADS) {
        const uint32_t j = c0 + tid;
        const bool closed = j < q.L && closure[j].keypoint >= 0;
        uint32_t cnt;
        const uint32_t pos = block_prefix<kt::KT_WAVES>(closed, s.k.wsum, &cnt);
        if (closed) s.lst[n_closed + pos] = (int)j;
        n_closed += (int)cnt;
    }
    uint32_t total = 0;  // thread 0's
    for (uint32_t k = 0; k < q.n_kf; k++) {
        const long long pair = (long long)prob * b.kf_slots + k, k0 = pair * b.kf_pitch;
        const uint32_t nkp = b.d_n_kf_kp[pair];
        const bool over = nkp > (uint32_t)LC_MAX_KP || (long long)nkp > b.kf_pitch;
        mage_loop_closure_assoc* rec = b.d_connect + out0 * b.kf_slots + k;
        uint8_t* verdict = b.d_connect_verdict + out0 * b.kf_slots + k;
        for (uint32_t j = tid; j < q.L; j += kt::KT_THREADS) {
            const bool closed = closure[j].keypoint >= 0;
            if (over || !closed) rec[(long long)j * b.kf_slots] = mage_loop_closure_assoc{0.f, 0.f, 0, -1};
            if (!over && !closed) verdict[(long long)j * b.kf_slots] = LC_NOT_SAMPLED;
        }
        if (over) {  // uniform over the workgroup
            if (tid == 0) {
                atomicOr(b.d_status + prob, MAGE_LC_STATUS_OVER_LIMIT);
                b.d_kf_modified[pair] = 0;
            }
            continue;
        }
        const float* intr = b.d_kf_intr4 + 4 * pair;
        const mage_keypoint* kp = b.d_kf_kp + k0;
        const uint8_t* kdesc = b.d_kf_desc + 32 * k0;
        uint8_t* mask = b.d_kf_mask + k0;
        mark_held(q, s, b.d_kf_point + k0, nkp);
        kt::stage_keyframe(
            p.connect.band_scale, (int)nkp, kp, s.k, [&](int t) { return mask[t] != 0; },
            [&] {
                Frame f;
                newpoints::make_frame(b.d_kf_pos3 + 3 * pair, b.d_kf_r9 + 9 * pair, intr, f);
                s_frame = f;
            });
        offer_points(p, p.connect, q, s, s_frame, intr, kdesc, n_closed, s.lst, b.kf_slots, rec, verdict);
        for (int t = tid; t < (int)nkp; t += kt::KT_THREADS)
            if (!mask_bit(s.k.m, t)) mask[t] = 0;
        // apply any found associations to the keyframe (:771-774), a wave per point
        for (int i = tid >> 6; i < n_closed; i += kt::KT_WAVES) {
            const int j = s.lst[i], t = s.took[j];
            if (t < 0) continue;
            const long long idx = sample_index(q.sm, (uint32_t)j);
            append_and_refresh(p.c.tables, q.state + idx, q.obs + idx * q.obs_pitch, kdesc + 32ll * t, s_frame.C,
                               kp[t].octave, b.d_kf_id[pair]);
        }
        if (tid == 0) {
            b.d_kf_modified[pair] = s.n_taken > 0;
            total += s.n_taken;
        }
        __syncthreads();  // the refreshed states and the LDS flags, before the next keyframe
    }
    if (tid == 0) counts[2] = total;
}

}  // namespace
}  // namespace mage

extern "C" {

mage_status mage_map_points_refresh_batch_device(const mage_loop_closure_settings* settings, uint32_t n_points,
                                                 const float* d_positions, const mage_map_point_obs* d_obs,
                                                 int64_t obs_pitch, const uint32_t* d_n_obs, mage_map_point_state* d_state,
                                                 uint32_t* d_status, mage_stream stream)
{
    using namespace mage;
    const char* why = loopclose::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(obs_pitch >= 1 && obs_pitch <= (int64_t)MAGE_MP_MAX_OBS, MAGE_EINVAL, "obs_pitch must be in 1..65536");
    if (n_points == 0) return MAGE_OK;
    MAGE_REQUIRE(d_positions && d_obs && d_n_obs && d_state && d_status, MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(reinterpret_cast<uintptr_t>(d_obs) % 16 == 0, MAGE_EINVAL, "the observations must be 16-byte aligned");
    RefreshParams p{};
    p.t = loopclose::make_tables(*settings);
    p.n_points = n_points;
    p.positions = d_positions;
    p.obs = d_obs;
    p.obs_pitch = obs_pitch;
    p.n_obs = d_n_obs;
    p.state = d_state;
    p.status = d_status;
    launch("loopclose.refresh", map_points_refresh_kernel, dim3((n_points + LC_WAVES - 1) / LC_WAVES), dim3(LC_THREADS), 0,
           (hipStream_t)stream, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

mage_status mage_map_points_refresh(const mage_loop_closure_settings* settings, uint32_t n_points, const float* positions,
                                    const mage_map_point_obs* obs, int64_t obs_pitch, const uint32_t* n_obs,
                                    mage_map_point_state* state, int device)
{
    using namespace mage;
    const char* why = loopclose::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(obs_pitch >= 1 && obs_pitch <= (int64_t)MAGE_MP_MAX_OBS, MAGE_EINVAL, "obs_pitch must be in 1..65536");
    if (n_points == 0) return MAGE_OK;
    MAGE_REQUIRE(positions && obs && n_obs && state, MAGE_EINVAL, "null argument");
    uint32_t most = 1;  // the device pitch: the largest count
    for (uint32_t i = 0; i < n_points; i++) {
        MAGE_REQUIRE((int64_t)n_obs[i] <= obs_pitch, MAGE_EINVAL, "a point has more observations than obs_pitch");
        most = std::max(most, n_obs[i]);
    }
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    HostScratch* sp = host_scratch(device, SCRATCH_LOOPCLOSE);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [observations][positions][counts][status] | [states]: the inputs in one H2D copy,
    // the states back in one D2H copy
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t np = n_points, oobs = 0, opos = al(oobs + 64 * np * most), ocnt = al(opos + 12 * np),
                 ost = al(ocnt + 4 * np), ostate = al(ost + 4), total = al(ostate + sizeof(mage_map_point_state) * np);
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(total)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    for (uint32_t i = 0; i < n_points; i++)
        if (n_obs[i]) std::memcpy(h + oobs + 64 * (i * (size_t)most), obs + (size_t)i * (size_t)obs_pitch, 64ull * n_obs[i]);
    std::memcpy(h + opos, positions, 12 * np);
    std::memcpy(h + ocnt, n_obs, 4 * np);
    std::memset(h + ost, 0, 4);
    MAGE_HIP(hipMemcpyAsync(b, h, ostate, hipMemcpyHostToDevice, S.st));
    r = mage_map_points_refresh_batch_device(settings, n_points, reinterpret_cast<const float*>(b + opos),
                                             reinterpret_cast<const mage_map_point_obs*>(b + oobs), (int64_t)most,
                                             reinterpret_cast<const uint32_t*>(b + ocnt),
                                             reinterpret_cast<mage_map_point_state*>(b + ostate),
                                             reinterpret_cast<uint32_t*>(b + ost), S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + ostate, b + ostate, total - ostate, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    std::memcpy(state, h + ostate, sizeof(mage_map_point_state) * np);
    return MAGE_OK;
}

mage_status mage_cheap_loop_closure_batch_device(const mage_loop_closure_settings* settings,
                                                 const mage_loop_closure_batch* batch, mage_stream stream)
{
    using namespace mage;
    const char* why = loopclose::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(batch, MAGE_EINVAL, "null batch");
    const mage_loop_closure_batch& b = *batch;
    MAGE_REQUIRE(b.struct_size == sizeof(mage_loop_closure_batch), MAGE_EINVAL,
                 "struct_size is not sizeof(mage_loop_closure_batch)");
    if (b.problems == 0) return MAGE_OK;
    MAGE_REQUIRE(b.map_pitch > 0 && b.ki_pitch > 0 && b.kf_pitch > 0 && b.obs_pitch >= 1 &&
                     b.obs_pitch <= (int64_t)MAGE_MP_MAX_OBS,
                 MAGE_EINVAL, "pitches must be positive and obs_pitch at most 65536");
    MAGE_REQUIRE(b.d_n_map && b.d_state && b.d_obs && b.d_offset && b.d_n_keyframes && b.d_ki_id && b.d_n_ki &&
                     b.d_ki_pos3 && b.d_ki_r9 && b.d_ki_intr4 && b.d_ki_kp && b.d_ki_desc && b.d_ki_point && b.d_n_kf &&
                     b.d_sample_index && b.d_closure && b.d_closure_verdict && b.d_ki_mask && b.d_counts && b.d_status,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(b.kf_slots == 0 || (b.d_kf_id && b.d_kf_pos3 && b.d_kf_r9 && b.d_kf_intr4 && b.d_kf_kp && b.d_kf_desc &&
                                     b.d_kf_point && b.d_n_kf_kp && b.d_kf_mask && b.d_connect && b.d_connect_verdict &&
                                     b.d_kf_modified),
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE((uint64_t)b.problems * std::max(b.kf_slots, 1u) <= 0x7FFFFFFFull && b.problems <= 65535u, MAGE_EINVAL,
                 "too many problems");
    MAGE_REQUIRE(reinterpret_cast<uintptr_t>(b.d_obs) % 16 == 0 && reinterpret_cast<uintptr_t>(b.d_ki_desc) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(b.d_kf_desc) % 16 == 0,
                 MAGE_EINVAL, "descriptor and observation pointers must be 16-byte aligned");
    LcParams p{};
    p.c = loopclose::make_consts(*settings);
    const float band_scale = (float)kt::KT_BANDS / p.c.gate.image_h;
    p.closure = kt::Search{p.c.gate.radius, band_scale, p.c.gate.max_dist, p.c.gate.min_diff};
    p.connect = kt::Search{p.c.gate.radius, band_scale, p.c.connect_max_dist, p.c.connect_min_diff};
    p.b = b;
    hipStream_t st = (hipStream_t)stream;
    launch("loopclose.close", loop_close_kernel, dim3(b.problems), dim3(kt::KT_THREADS), 0, st, p);
    launch("loopclose.apply", loop_close_apply_kernel, dim3((p.c.max_points + LC_WAVES - 1) / LC_WAVES, b.problems),
           dim3(LC_THREADS), 0, st, p);
    if (b.kf_slots) launch("loopclose.connect", loop_connect_kernel, dim3(b.problems), dim3(kt::KT_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

mage_status mage_cheap_loop_closure(const mage_loop_closure_settings* settings, const mage_loop_closure_problem* problem,
                                    int device)
{
    using namespace mage;
    const char* why = loopclose::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    why = loopclose::check_problem(problem);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    const mage_loop_closure_problem& q = *problem;
    const uint32_t max = settings->max_map_points;
    uint32_t pitch = 1;  // of the covisible keyframes that are within the limit
    for (uint32_t k = 0; k < q.n_kf; k++) {
        const uint32_t nk = q.kf_start[k + 1] - q.kf_start[k];
        if (nk <= (uint32_t)loopclose::LC_MAX_KP) pitch = std::max(pitch, nk);
    }
    const bool ki_over = q.n_ki > (uint32_t)loopclose::LC_MAX_KP;
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    HostScratch* sp = host_scratch(device, SCRATCH_LOOPCLOSE);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [observations][states] | [Ki mask][kf masks][modified][verdicts] | [counts, status]
    // [sample][records] || [scalars][poses][Ki kp, desc, point][kf kp, desc, point]: the whole map
    // travels both ways (the batch form is the one for maps that live on the device), the inputs
    // in one H2D copy, everything up to the records back in one D2H copy.  The verdict bytes of a
    // keyframe over the limit are the caller's; such a keyframe keeps its count and sends no data.
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t nm = std::max(q.n_map, 1u), nkf = q.n_kf, slots = std::max(q.n_kf, 1u), nki = ki_over ? 1 : std::max(q.n_ki, 1u),
                 op = (size_t)q.obs_pitch;
    const size_t oobs = 0, ostate = al(oobs + 64 * nm * op), okim = al(ostate + 40 * nm), okfm = al(okim + nki),
                 omod = al(okfm + slots * pitch), ocv = al(omod + slots), onv = al(ocv + max),
                 ocnt = al(onv + (size_t)max * slots), osmp = al(ocnt + 16), ocr = al(osmp + 4 * (size_t)max),
                 onr = al(ocr + 16 * (size_t)max), oout = al(onr + 16 * (size_t)max * slots),
                 oscal = oout, opose = al(oscal + 4 * (6 + 2 * slots)), okikp = al(opose + 64 * (1 + slots)),
                 okid = al(okikp + 28 * nki), okip = al(okid + 32 * nki), okfkp = al(okip + 4 * nki),
                 okfd = al(okfkp + 28 * slots * pitch), okfp = al(okfd + 32 * slots * pitch),
                 total = al(okfp + 4 * slots * pitch);
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(total)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    std::memset(h + okim, 0, ocnt - okim);
    if (q.n_map) {
        std::memcpy(h + oobs, q.obs, 64 * (size_t)q.n_map * op);
        std::memcpy(h + ostate, q.state, 40 * (size_t)q.n_map);
        std::memcpy(h + ocv, q.closure_verdict, max);
        if (nkf) std::memcpy(h + onv, q.connect_verdict, (size_t)max * nkf);
    }
    if (q.n_ki && !ki_over) std::memcpy(h + okim, q.ki_mask, q.n_ki);
    uint32_t* sc = reinterpret_cast<uint32_t*>(h + oscal);  // [n_map, offset, n_keyframes, ki_id, n_ki, n_kf, n_kf_kp x, kf_id x]
    sc[0] = q.n_map;
    sc[1] = q.offset;
    sc[2] = q.n_keyframes;
    sc[3] = (uint32_t)q.ki_id;
    sc[4] = q.n_ki;
    sc[5] = q.n_kf;
    float* hp = reinterpret_cast<float*>(h + opose);  // [pos3 x (1 + slots) | r9 x | intr4 x], Ki first
    std::memcpy(hp, q.ki_pos3, 12);
    std::memcpy(hp + 3 * (1 + slots), q.ki_r9, 36);
    std::memcpy(hp + 12 * (1 + slots), q.ki_intr4, 16);
    if (nkf) {
        std::memcpy(hp + 3, q.kf_pos3, 12 * nkf);
        std::memcpy(hp + 3 * (1 + slots) + 9, q.kf_r9, 36 * nkf);
        std::memcpy(hp + 12 * (1 + slots) + 4, q.kf_intr4, 16 * nkf);
    }
    if (q.n_ki && !ki_over) {
        std::memcpy(h + okikp, q.ki_kp, 28ull * q.n_ki);
        std::memcpy(h + okid, q.ki_desc, 32ull * q.n_ki);
        std::memcpy(h + okip, q.ki_point, 4ull * q.n_ki);
    }
    for (uint32_t k = 0; k < q.n_kf; k++) {
        const uint32_t s0 = q.kf_start[k], nk = q.kf_start[k + 1] - s0;
        sc[6 + k] = nk;
        sc[6 + slots + k] = (uint32_t)q.kf_id[k];
        if (nk == 0 || nk > (uint32_t)loopclose::LC_MAX_KP) continue;
        std::memcpy(h + okfkp + 28 * (k * (size_t)pitch), q.kf_kp + s0, 28ull * nk);
        std::memcpy(h + okfd + 32 * (k * (size_t)pitch), q.kf_desc + 32ull * s0, 32ull * nk);
        std::memcpy(h + okfp + 4 * (k * (size_t)pitch), q.kf_point + s0, 4ull * nk);
        std::memcpy(h + okfm + k * (size_t)pitch, q.kf_mask + s0, nk);
    }
    MAGE_HIP(hipMemcpyAsync(b, h, onv + (size_t)max * slots, hipMemcpyHostToDevice, S.st));
    MAGE_HIP(hipMemcpyAsync(b + oscal, h + oscal, total - oscal, hipMemcpyHostToDevice, S.st));
    const uint32_t* dsc = reinterpret_cast<const uint32_t*>(b + oscal);
    const float* dp = reinterpret_cast<const float*>(b + opose);
    mage_loop_closure_batch B{};
    B.struct_size = (uint32_t)sizeof(B);
    B.problems = 1;
    B.kf_slots = q.n_kf;
    B.map_pitch = (int64_t)nm;
    B.obs_pitch = q.obs_pitch;
    B.ki_pitch = (int64_t)nki;
    B.kf_pitch = pitch;
    B.d_n_map = dsc;
    B.d_state = reinterpret_cast<mage_map_point_state*>(b + ostate);
    B.d_obs = reinterpret_cast<mage_map_point_obs*>(b + oobs);
    B.d_offset = dsc + 1;
    B.d_n_keyframes = dsc + 2;
    B.d_ki_id = reinterpret_cast<const int32_t*>(dsc + 3);
    B.d_n_ki = dsc + 4;
    B.d_n_kf = dsc + 5;
    B.d_n_kf_kp = dsc + 6;
    B.d_kf_id = reinterpret_cast<const int32_t*>(dsc + 6 + slots);
    B.d_ki_pos3 = dp;
    B.d_kf_pos3 = dp + 3;
    B.d_ki_r9 = dp + 3 * (1 + slots);
    B.d_kf_r9 = B.d_ki_r9 + 9;
    B.d_ki_intr4 = dp + 12 * (1 + slots);
    B.d_kf_intr4 = B.d_ki_intr4 + 4;
    B.d_ki_kp = reinterpret_cast<const mage_keypoint*>(b + okikp);
    B.d_ki_desc = reinterpret_cast<const uint8_t*>(b + okid);
    B.d_ki_point = reinterpret_cast<const int32_t*>(b + okip);
    B.d_kf_kp = reinterpret_cast<const mage_keypoint*>(b + okfkp);
    B.d_kf_desc = reinterpret_cast<const uint8_t*>(b + okfd);
    B.d_kf_point = reinterpret_cast<const int32_t*>(b + okfp);
    B.d_kf_mask = reinterpret_cast<uint8_t*>(b + okfm);
    B.d_sample_index = reinterpret_cast<uint32_t*>(b + osmp);
    B.d_closure = reinterpret_cast<mage_loop_closure_assoc*>(b + ocr);
    B.d_closure_verdict = reinterpret_cast<uint8_t*>(b + ocv);
    B.d_connect = reinterpret_cast<mage_loop_closure_assoc*>(b + onr);
    B.d_connect_verdict = reinterpret_cast<uint8_t*>(b + onv);
    B.d_ki_mask = reinterpret_cast<uint8_t*>(b + okim);
    B.d_kf_modified = reinterpret_cast<uint8_t*>(b + omod);
    B.d_counts = reinterpret_cast<uint32_t*>(b + ocnt);
    B.d_status = B.d_counts + 3;
    r = mage_cheap_loop_closure_batch_device(settings, &B, S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h, b, oout, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(h + ocnt);
    std::memcpy(q.counts, cnt, 12);
    *q.status = cnt[3];
    if (cnt[3] & MAGE_LC_STATUS_OBS_FULL) {
        set_error("a sampled point's observation list cannot hold n_obs + 1 + n_kf entries");
        return MAGE_ECAPACITY;
    }
    const uint32_t L = cnt[0];
    if (L == 0) return MAGE_OK;
    std::memcpy(q.obs, h + oobs, 64 * (size_t)q.n_map * op);
    std::memcpy(q.state, h + ostate, 40 * (size_t)q.n_map);
    std::memcpy(q.sample_index, h + osmp, 4ull * L);
    std::memcpy(q.closure, h + ocr, 16ull * L);
    if (!ki_over) {
        std::memcpy(q.closure_verdict, h + ocv, L);
        if (q.n_ki) std::memcpy(q.ki_mask, h + okim, q.n_ki);
    }
    if (nkf) {
        std::memcpy(q.connect, h + onr, 16ull * L * nkf);
        std::memcpy(q.connect_verdict, h + onv, (size_t)L * nkf);
        std::memcpy(q.kf_modified, h + omod, nkf);
    }
    for (uint32_t k = 0; k < q.n_kf; k++) {
        const uint32_t s0 = q.kf_start[k], nk = q.kf_start[k + 1] - s0;
        if (nk && nk <= (uint32_t)loopclose::LC_MAX_KP) std::memcpy(q.kf_mask + s0, h + okfm + k * (size_t)pitch, nk);
    }
    return MAGE_OK;
}

}  // extern "C"
