// newpoints.hip — NewMapPointsCreation's CreateInitialAssociations on MI355X (gfx950).
//
// The reference (Core/MAGESLAM/Source/Mapping/NewMapPointsCreation.cpp:171-329) walks the matches
// of each covisible keyframe Kc against the new keyframe Ki in order: a match whose Ki keypoint
// lies in a full grid cell is skipped (:301), one whose Ki keypoint already made a point is skipped
// (:309), the others are triangulated and validated (:74-160) and, when valid, make a point, mark
// the Ki keypoint and count in its cell (:312-315).  The geometry (newpoints_math.hpp) depends on
// the match alone; the bookkeeping has an exact parallel form, because a Ki keypoint lies in one
// cell, cell counts only grow and the cap is tested before the duplicate test:
//   U = the matches that pass the geometry and are the first such match of their Ki keypoint;
//   rank(m) = initial_count[cell(m)] + the members of U before m in cell(m);
//   m is GRID_FULL when rank(m) >= max_grid_count, else KI_TAKEN when a member of U with its Ki
//   keypoint precedes it, else its geometry verdict — accepted exactly when it is in U.
// (An earlier member of U that was itself refused was refused by a full cell, which is still full.)
// One workgroup per problem takes the matches 256 at a time in processing order: the geometry per
// thread, the first match per Ki keypoint by an LDS atomicMin of the match's sequence number (later
// chunks only hold larger numbers), the per-cell ranks and the output positions by wave ballots plus
// running bases.  Nothing depends on the order in which threads run; all loops are bounded by the
// counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "newpoints_math.hpp"
#include "ordered_take.hpp"

namespace mage {
namespace {

using namespace newpoints;

// The host-buffer entry's scratch slot, after common.hpp's ScratchSlot values.  Declared here so
// that common.hpp, whose hash the committed profiler counters of every other kernel are keyed on
// (build.kernel_file_shas), stays as it is.
constexpr ScratchSlot SCRATCH_NEWPOINTS = static_cast<ScratchSlot>(5);

constexpr int NP_THREADS = 256;
constexpr int NP_WAVES = NP_THREADS / kWave;

struct NpParams {
    Consts c;
    uint32_t kc_slots;
    const float *ki_pos3, *ki_r9, *ki_intr4;
    const mage_keypoint* ki_kp;
    long long ki_pitch;
    const uint32_t* n_ki;
    const uint8_t* ki_assoc;
    const uint32_t* n_kc;
    const float *kc_pos3, *kc_r9, *kc_intr4;
    const mage_keypoint* kc_kp;
    long long kc_pitch;
    const uint32_t* n_kc_kp;
    const mage_dmatch* matches;
    uint32_t match_cap;
    const uint32_t* n_matches;
    mage_new_point* out;
    uint32_t cap;
    uint32_t* n_out;
    uint8_t* verdict;
    uint32_t* status;
};

__global__ __launch_bounds__(NP_THREADS) void new_points_kernel(NpParams p)
{
    __shared__ Frame s_ki;
    __shared__ Pair s_pair[NP_MAX_SLOTS];
    __shared__ uint32_t s_first[NP_MAX_KI];
    __shared__ int s_count[NP_MAX_CELLS];
    __shared__ int s_wcell[NP_WAVES][NP_MAX_CELLS];
    __shared__ int s_wacc[NP_WAVES];
    __shared__ uint32_t s_mstart[NP_MAX_SLOTS + 1];
    const int pr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nki = p.n_ki[pr], nkc = p.n_kc[pr];
    const long long pair0 = (long long)pr * p.kc_slots;
    bool bad = nki > (uint32_t)NP_MAX_KI || (long long)nki > p.ki_pitch || nkc > p.kc_slots;
    for (uint32_t s = 0; !bad && s < nkc; s++) bad = (long long)p.n_kc_kp[pair0 + s] > p.kc_pitch;
    if (bad) {  // uniform over the workgroup
        if (tid == 0) {
            p.n_out[pr] = 0;
            atomicOr(p.status, 1u);
        }
        return;
    }
    const int ncells = (int)(p.c.grid_w * p.c.grid_h);
    const mage_keypoint* kikp = p.ki_kp + pr * p.ki_pitch;

    // setup: one thread per Kc slot builds the pair's matrices; grid counts from Ki's associated mask
    if ((uint32_t)tid < nkc || tid == 0) {
        Frame ki, kc;
        make_frame(p.ki_pos3 + 3ll * pr, p.ki_r9 + 9ll * pr, p.ki_intr4 + 4ll * pr, ki);
        if (tid == 0) s_ki = ki;
        if ((uint32_t)tid < nkc) {
            const long long pair = pair0 + tid;
            make_frame(p.kc_pos3 + 3 * pair, p.kc_r9 + 9 * pair, p.kc_intr4 + 4 * pair, kc);
            make_pair(ki, kc, s_pair[tid]);
        }
    }
    if (tid == 0) {
        uint32_t acc = 0;
        for (uint32_t s = 0; s < nkc; s++) {
            s_mstart[s] = acc;
            acc += min(p.n_matches[pair0 + s], p.match_cap);
        }
        s_mstart[nkc] = acc;
    }
    for (int i = tid; i < (int)nki; i += NP_THREADS) s_first[i] = 0xFFFFFFFFu;
    if (tid < NP_MAX_CELLS) s_count[tid] = 0;
    __syncthreads();
    if (p.ki_assoc) {
        const uint8_t* as = p.ki_assoc + pr * p.ki_pitch;
        for (int i = tid; i < (int)nki; i += NP_THREADS)
            if (as[i]) {
                const int cell = count_cell(p.c, kikp[i].x, kikp[i].y);
                if (cell >= 0) atomicAdd(&s_count[cell], 1);
            }
    }
    __syncthreads();

    const uint32_t total = s_mstart[nkc];
    uint32_t nacc = 0;
    for (uint32_t c0 = 0; c0 < total; c0 += NP_THREADS) {
        const uint32_t g = c0 + tid;
        const bool live = g < total;
        int slot = 0, cell = -1, t = 0, q = 0;
        uint32_t idx = 0;
        long long mi = 0;
        bool valid = false;
        uint8_t gv = NP_BAD_INDEX;
        Geometry geo{};
        if (live) {
            while (slot + 1 < (int)nkc && s_mstart[slot + 1] <= g) slot++;
            idx = g - s_mstart[slot];
            const long long pair = pair0 + slot;
            mi = pair * p.match_cap + idx;
            const mage_dmatch m = p.matches[mi];
            q = m.query_idx;
            t = m.train_idx;
            if (q >= 0 && (uint32_t)q < p.n_kc_kp[pair] && t >= 0 && (uint32_t)t < nki) {
                const mage_keypoint a = p.kc_kp[pair * p.kc_pitch + q], b = kikp[t];
                if (b.octave >= 0 && b.octave < NP_MAX_LEVELS) {
                    valid = true;
                    cell = test_cell(p.c, b.x, b.y);
                    gv = match_geometry(p.c, s_ki, s_pair[slot], a.x, a.y, a.octave, b.x, b.y, b.octave, geo);
                    if (gv == NP_ACCEPTED) atomicMin(&s_first[t], g);
                }
            }
        }
        __syncthreads();
        const bool u = valid && gv == NP_ACCEPTED && s_first[t] == g;
        // the match's rank in its cell: the cell's count plus the members of U before it
        const int r = rank_by_key<NP_WAVES>(cell, u, ncells, s_count, &s_wcell[0][0], NP_MAX_CELLS);
        uint8_t verdict = NP_BAD_INDEX;
        if (valid)
            verdict = (uint32_t)r >= p.c.max_grid_count ? (uint8_t)NP_GRID_FULL
                      : s_first[t] < g                  ? (uint8_t)NP_KI_TAKEN
                                                        : gv;
        const bool acc = valid && verdict == NP_ACCEPTED;
        // the accepted points in match order.  Open-coded: block_prefix's second barrier (the next write
        // of s_wacc is two barriers away already) measured +1 % on this kernel.
        const unsigned long long abal = __ballot(acc);
        if (lane == 0) s_wacc[wave] = __popcll(abal);
        if (live) p.verdict[mi] = verdict;
        __syncthreads();
        uint32_t pos = nacc + __popcll(abal & ((1ull << lane) - 1ull));
        for (int w = 0; w < NP_WAVES; w++) {
            if (w < wave) pos += s_wacc[w];
            nacc += s_wacc[w];
        }
        if (acc && pos < p.cap) {
            mage_new_point o;
            for (int i = 0; i < 3; i++) {
                o.position[i] = geo.X[i];
                o.mean_view_dir[i] = geo.dir[i];
            }
            o.d_min = geo.d_min;
            o.d_max = geo.d_max;
            o.ki_index = (uint32_t)t;
            o.kc_slot = (uint32_t)slot;
            o.kc_index = (uint32_t)q;
            o.match_index = idx;
            p.out[(long long)pr * p.cap + pos] = o;
        }
        if (tid < ncells) {
            int add = 0;
            for (int w = 0; w < NP_WAVES; w++) add += s_wcell[w][tid];
            s_count[tid] += add;  // read again only after the next chunk's barriers
        }
    }
    if (tid == 0) {
        p.n_out[pr] = min(nacc, p.cap);
        if (nacc > p.cap) atomicOr(p.status, 2u);
    }
}

mage_status new_points_launch(const NpParams& p, uint32_t problems, hipStream_t st)
{
    launch("newpoints.create", new_points_kernel, dim3(problems), dim3(NP_THREADS), 0, st, p);
    MAGE_HIP(hipGetLastError());
    return MAGE_OK;
}

}  // namespace
}  // namespace mage

extern "C" {

mage_status mage_new_map_points_batch_device(const mage_new_points_settings* settings, uint32_t problems,
                                             uint32_t kc_slots, const float* d_ki_pos3, const float* d_ki_r9,
                                             const float* d_ki_intr4, const mage_keypoint* d_ki_kp, int64_t ki_pitch,
                                             const uint32_t* d_n_ki, const uint8_t* d_ki_associated,
                                             const uint32_t* d_n_kc, const float* d_kc_pos3, const float* d_kc_r9,
                                             const float* d_kc_intr4, const mage_keypoint* d_kc_kp, int64_t kc_pitch,
                                             const uint32_t* d_n_kc_kp, const mage_dmatch* d_matches,
                                             uint32_t match_cap, const uint32_t* d_n_matches, mage_new_point* d_out,
                                             uint32_t cap, uint32_t* d_n_out, uint8_t* d_verdict, uint32_t* d_status,
                                             mage_stream stream)
{
    using namespace mage;
    const char* why = newpoints::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(kc_slots >= 1 && kc_slots <= (uint32_t)newpoints::NP_MAX_SLOTS, MAGE_EINVAL, "kc_slots must be in 1..8");
    if (problems == 0) return MAGE_OK;
    MAGE_REQUIRE(d_ki_pos3 && d_ki_r9 && d_ki_intr4 && d_ki_kp && d_n_ki && d_n_kc && d_kc_pos3 && d_kc_r9 &&
                     d_kc_intr4 && d_kc_kp && d_n_kc_kp && d_matches && d_n_matches && d_out && d_n_out &&
                     d_verdict && d_status,
                 MAGE_EINVAL, "null buffer");
    MAGE_REQUIRE(ki_pitch > 0 && kc_pitch > 0 && match_cap > 0 && cap > 0, MAGE_EINVAL,
                 "pitches and capacities must be positive");
    NpParams p{};
    p.c = newpoints::make_consts(*settings);
    p.kc_slots = kc_slots;
    p.ki_pos3 = d_ki_pos3;
    p.ki_r9 = d_ki_r9;
    p.ki_intr4 = d_ki_intr4;
    p.ki_kp = d_ki_kp;
    p.ki_pitch = ki_pitch;
    p.n_ki = d_n_ki;
    p.ki_assoc = d_ki_associated;
    p.n_kc = d_n_kc;
    p.kc_pos3 = d_kc_pos3;
    p.kc_r9 = d_kc_r9;
    p.kc_intr4 = d_kc_intr4;
    p.kc_kp = d_kc_kp;
    p.kc_pitch = kc_pitch;
    p.n_kc_kp = d_n_kc_kp;
    p.matches = d_matches;
    p.match_cap = match_cap;
    p.n_matches = d_n_matches;
    p.out = d_out;
    p.cap = cap;
    p.n_out = d_n_out;
    p.verdict = d_verdict;
    p.status = d_status;
    return new_points_launch(p, problems, (hipStream_t)stream);
}

mage_status mage_new_map_points(const mage_new_points_settings* settings, const float* ki_pos3, const float* ki_r9,
                                const float* ki_intr4, const mage_keypoint* ki_kp, uint32_t n_ki,
                                const uint8_t* ki_associated, uint32_t n_kc, const float* kc_pos3, const float* kc_r9,
                                const float* kc_intr4, const mage_keypoint* kc_kp, const uint32_t* kc_kp_start,
                                const mage_dmatch* matches, const uint32_t* match_start, mage_new_point* out,
                                uint32_t cap, uint32_t* n_out, uint8_t* verdict, uint32_t* status, int device)
{
    using namespace mage;
    const char* why = newpoints::check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(n_kc <= (uint32_t)newpoints::NP_MAX_SLOTS, MAGE_EINVAL, "more than 8 Kc slots");
    MAGE_REQUIRE(n_out && status && ki_pos3 && ki_r9 && ki_intr4 && (n_ki == 0 || ki_kp), MAGE_EINVAL, "null argument");
    *n_out = 0;
    *status = 0;
    MAGE_REQUIRE(n_kc == 0 || (kc_pos3 && kc_r9 && kc_intr4 && kc_kp_start && match_start), MAGE_EINVAL, "null argument");
    uint32_t kc_pitch = 1, match_cap = 1;
    for (uint32_t s = 0; s < n_kc; s++) {
        MAGE_REQUIRE(kc_kp_start[s] <= kc_kp_start[s + 1] && match_start[s] <= match_start[s + 1], MAGE_EINVAL,
                     "start offsets must not decrease");
        kc_pitch = std::max(kc_pitch, kc_kp_start[s + 1] - kc_kp_start[s]);
        match_cap = std::max(match_cap, match_start[s + 1] - match_start[s]);
    }
    const uint32_t n_matches = n_kc ? match_start[n_kc] - match_start[0] : 0;
    MAGE_REQUIRE((n_kc == 0 || kc_kp_start[n_kc] == kc_kp_start[0] || kc_kp) &&
                     (n_matches == 0 || (matches && verdict)) && (cap == 0 || out),
                 MAGE_EINVAL, "null argument");
    if (n_matches == 0) return MAGE_OK;
    mage_status r = bind_device(device);
    if (r != MAGE_OK) return r;
    HostScratch* sp = host_scratch(device, SCRATCH_NEWPOINTS);
    if (!sp) return MAGE_EDEVICE;
    HostScratch& S = *sp;
    // device layout [poses][ki kp][ki mask][kc kp][matches][counts] | [status, n_out][verdicts][points]:
    // the inputs in one H2D copy, the outputs back in one D2H copy
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint32_t slots = std::max(n_kc, 1u), ki_pitch = std::max(n_ki, 1u), dcap = std::max(cap, 1u);
    const size_t opose = 0, okikp = al(opose + 4ull * 16 * (1 + slots)), omask = al(okikp + 28ull * ki_pitch),
                 okckp = al(omask + ki_pitch), omat = al(okckp + 28ull * slots * kc_pitch),
                 ocnt = al(omat + 16ull * slots * match_cap), ores = al(ocnt + 4ull * (2 + 2 * slots)),
                 over = al(ores + 8), opts = al(over + (size_t)slots * match_cap), total = al(opts + 48ull * dcap);
    if ((r = S.buf.reserve(total)) != MAGE_OK || (r = S.host.reserve(total)) != MAGE_OK) return r;
    char* b = S.buf.as<char>();
    char* h = S.host.as<char>();
    std::memset(h, 0, ores + 8);
    // poses: [ki pos3 | ki r9 | ki intr4 | kc pos3 x slots | kc r9 x slots | kc intr4 x slots]
    float* hp = reinterpret_cast<float*>(h + opose);
    std::memcpy(hp, ki_pos3, 12);
    std::memcpy(hp + 3, ki_r9, 36);
    std::memcpy(hp + 12, ki_intr4, 16);
    std::memcpy(hp + 16, kc_pos3, 12ull * n_kc);
    std::memcpy(hp + 16 + 3 * slots, kc_r9, 36ull * n_kc);
    std::memcpy(hp + 16 + 12 * slots, kc_intr4, 16ull * n_kc);
    if (n_ki) std::memcpy(h + okikp, ki_kp, 28ull * n_ki);
    if (ki_associated && n_ki) std::memcpy(h + omask, ki_associated, n_ki);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(h + ocnt);  // [n_ki, n_kc, n_kc_kp x slots, n_matches x slots]
    cnt[0] = n_ki;
    cnt[1] = n_kc;
    for (uint32_t s = 0; s < n_kc; s++) {
        const uint32_t nk = kc_kp_start[s + 1] - kc_kp_start[s], nm = match_start[s + 1] - match_start[s];
        cnt[2 + s] = nk;
        cnt[2 + slots + s] = nm;
        if (nk) std::memcpy(h + okckp + 28ull * s * kc_pitch, kc_kp + kc_kp_start[s], 28ull * nk);
        if (nm) std::memcpy(h + omat + 16ull * s * match_cap, matches + match_start[s], 16ull * nm);
    }
    MAGE_HIP(hipMemcpyAsync(b, h, ores + 8, hipMemcpyHostToDevice, S.st));
    const float* dp = reinterpret_cast<const float*>(b + opose);
    const uint32_t* dc = reinterpret_cast<const uint32_t*>(b + ocnt);
    uint32_t* dres = reinterpret_cast<uint32_t*>(b + ores);
    r = mage_new_map_points_batch_device(
        settings, 1, slots, dp, dp + 3, dp + 12, reinterpret_cast<const mage_keypoint*>(b + okikp), ki_pitch, dc,
        ki_associated ? reinterpret_cast<const uint8_t*>(b + omask) : nullptr, dc + 1, dp + 16, dp + 16 + 3 * slots,
        dp + 16 + 12 * slots, reinterpret_cast<const mage_keypoint*>(b + okckp), kc_pitch, dc + 2,
        reinterpret_cast<const mage_dmatch*>(b + omat), match_cap, dc + 2 + slots,
        reinterpret_cast<mage_new_point*>(b + opts), dcap, dres + 1, reinterpret_cast<uint8_t*>(b + over), dres, S.st);
    if (r != MAGE_OK) return r;
    MAGE_HIP(hipMemcpyAsync(h + ores, b + ores, total - ores, hipMemcpyDeviceToHost, S.st));
    MAGE_HIP(hipStreamSynchronize(S.st));
    const uint32_t* hres = reinterpret_cast<const uint32_t*>(h + ores);
    *status = hres[0];
    if (hres[0] & 1u) return MAGE_OK;  // over a limit: no points, verdicts untouched
    // cap == 0 ran with one spare record: every accepted point is then over the capacity
    const uint32_t got = cap ? hres[1] : 0;
    if (cap == 0 && hres[1] > 0) *status |= 2u;
    *n_out = got;
    if (got) std::memcpy(out, h + opts, 48ull * got);
    for (uint32_t s = 0; s < n_kc; s++) {
        const uint32_t nm = match_start[s + 1] - match_start[s];
        if (nm) std::memcpy(verdict + match_start[s], h + over + (size_t)s * match_cap, nm);
    }
    return MAGE_OK;
}

}  // extern "C"
