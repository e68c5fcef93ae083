// loopclose.cpp — the plain C++ twin of loopclose.hip: the mapping task's CheapLoopClosure
// (Tasks/MappingWorker.cpp:20-73), InsertKeyframe's effect on the points it associated
// (Map/ThreadSafeMap.cpp:242-249), TryConnectMapPoints (ThreadSafeMap.cpp:715-787) and the map-point
// refresh after an association (MapPoint::UpdateRepresentativeDescriptor and
// UpdateMeanViewDirectionAndDistances, Map/MapPoint.cpp:80-155) as the reference's literal loops
// over the arithmetic of loopclose_math.hpp.  Same states, records and bytes as the kernels.
//
// This file includes no HIP header, so that it also builds as plain host C++ on its own
// (tests/cpp/loop_closure_host_check.cpp): set_error and the argument check are declared here as
// common.hpp declares them.
#include <cstring>
#include <string>
#include <vector>

#include "loopclose_math.hpp"

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

namespace {

using namespace mage::loopclose;
using mage::newpoints::AssocConsts;
using mage::newpoints::Frame;
using mage::newpoints::host_hamming256;
using mage::newpoints::host_radius_match_one;

// MapPoint.cpp:80-155 for one point with observations o[0 .. n).
void refresh_one(const Tables& t, const float* P, const mage_map_point_obs* o, uint32_t n, mage_map_point_state& st)
{
    if (n == 0) {
        empty_state(P, st);
        return;
    }
    // UpdateRepresentativeDescriptor (:105-125); one observation compares with itself alone (:90-95)
    float least = 3.402823466e+38f;
    int rep = -1;
    for (uint32_t a = 0; a < n; a++) {
        float sum = 0;
        for (uint32_t b = 0; b < n; b++) sum += (float)host_hamming256(o[a].desc, o[b].desc);
        if (sum < least) {
            rep = (int)a;
            least = sum;
        }
    }
    // UpdateMeanViewDirectionAndDistances (:134-154)
    float m[3] = {0.f, 0.f, 0.f};
    for (uint32_t a = 0; a < n; a++) {
        float v[3];
        view_direction(P, o[a].centre, v);
        for (int j = 0; j < 3; j++) m[j] = m[j] + v[j];
    }
    finish_state(t, P, m, o[rep].centre, o[rep].octave, rep, (int)n, st);
}

// One keyframe of the problem as both stages read it.
struct Keyframe {
    int32_t id;
    uint32_t n;
    const float* intr4;
    const mage_keypoint* kp;
    const uint8_t* desc;
    const int32_t* point;
    Frame frame;
};

bool holds(const Keyframe& k, uint32_t index)
{
    for (uint32_t t = 0; t < k.n; t++)
        if (k.point[t] >= 0 && (uint32_t)k.point[t] == index) return true;
    return false;
}

// ProjectMapPointIntoCurrentFrame (TrackLocalMap.cpp:325-388) of map point `index` into keyframe k
// under `mask`: the record and the verdict; a success leaves the mask.
uint8_t offer(const AssocConsts& c, const mage_loop_closure_problem& p, const Keyframe& k, uint32_t index, uint8_t* mask,
              mage_loop_closure_assoc& rec)
{
    rec = mage_loop_closure_assoc{0.f, 0.f, 0, -1};
    if (holds(k, index)) return LC_HAS_POINT;
    const mage_map_point_state& st = p.state[index];
    bool pass;
    const uint8_t v = gate_point(c, k.frame, k.intr4, st, rec.x, rec.y, rec.octave, pass);
    if (!pass) return v;
    const uint8_t* desc = p.obs[(size_t)index * (size_t)p.obs_pitch + (size_t)st.rep].desc;
    const int t = host_radius_match_one(c, rec.x, rec.y, rec.octave, desc, k.kp, k.desc, k.n, mask);
    if (t < 0) return LC_NO_MATCH;
    rec.keypoint = t;
    mask[t] = 0;
    return LC_ASSOCIATED;
}

// MapPoint::AddKeyframeAssociation (MapPoint.cpp:35-46): keyframe k's keypoint t becomes the last
// observation of map point `index`, which is refreshed.
void associate(const Tables& tables, const mage_loop_closure_problem& p, const Keyframe& k, uint32_t index, int t)
{
    mage_map_point_state& st = p.state[index];
    mage_map_point_obs* o = p.obs + (size_t)index * (size_t)p.obs_pitch;
    o[st.n_obs] = make_obs(k.desc + 32ull * t, k.frame.C, k.kp[t].octave, k.id);
    refresh_one(tables, st.pos, o, (uint32_t)st.n_obs + 1u, st);
}

}  // namespace

extern "C" mage_status mage_map_points_refresh_host(const mage_loop_closure_settings* settings, uint32_t n_points,
                                                    const float* positions, const mage_map_point_obs* obs,
                                                    int64_t obs_pitch, const uint32_t* n_obs, mage_map_point_state* state)
{
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    MAGE_REQUIRE(obs_pitch >= 1 && obs_pitch <= (int64_t)MAGE_MP_MAX_OBS, MAGE_EINVAL, "obs_pitch must be in 1..65536");
    if (n_points == 0) return MAGE_OK;
    MAGE_REQUIRE(positions && obs && n_obs && state, MAGE_EINVAL, "null argument");
    for (uint32_t i = 0; i < n_points; i++)
        MAGE_REQUIRE((int64_t)n_obs[i] <= obs_pitch, MAGE_EINVAL, "a point has more observations than obs_pitch");
    const Tables t = make_tables(*settings);
    for (uint32_t i = 0; i < n_points; i++)
        refresh_one(t, positions + 3ull * i, obs + (size_t)i * (size_t)obs_pitch, n_obs[i], state[i]);
    return MAGE_OK;
}

extern "C" mage_status mage_cheap_loop_closure_host(const mage_loop_closure_settings* settings,
                                                    const mage_loop_closure_problem* problem)
{
    const char* why = check_settings(settings);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    why = check_problem(problem);
    MAGE_REQUIRE(!why, MAGE_EINVAL, why);
    const mage_loop_closure_problem& p = *problem;
    const Consts c = make_consts(*settings);
    p.counts[0] = p.counts[1] = p.counts[2] = 0;
    *p.status = 0;
    if (p.n_keyframes < c.min_keyframes) return MAGE_OK;  // MappingWorker.cpp:22-25

    // GetSampleOfMapPoints (Map.cpp:319-333), cut at max
    std::vector<uint32_t> sample;
    const uint32_t step = p.n_map / c.max_points + 1u;
    uint32_t count = p.offset;
    for (uint32_t i = 0; i < p.n_map && sample.size() < c.max_points; i++) {
        count++;
        if (count % step != 0) continue;
        sample.push_back(i);
    }
    const uint32_t L = (uint32_t)sample.size();
    for (uint32_t j = 0; j < L; j++) {
        const mage_map_point_state& st = p.state[sample[j]];
        if (st.n_obs < 0 || (int64_t)st.n_obs + 1 + (int64_t)p.n_kf > p.obs_pitch) {
            *p.status = MAGE_LC_STATUS_OBS_FULL;
            mage::set_error("a sampled point's observation list cannot hold n_obs + 1 + n_kf entries");
            return MAGE_ECAPACITY;
        }
    }
    p.counts[0] = L;
    if (L == 0) return MAGE_OK;  // nothing sampled: nothing else is written
    for (uint32_t j = 0; j < L; j++) p.sample_index[j] = sample[j];

    // CheapLoopClosure's loop (MappingWorker.cpp:49-70) and InsertKeyframe's associations
    Keyframe ki{p.ki_id, p.n_ki, p.ki_intr4, p.ki_kp, p.ki_desc, p.ki_point, {}};
    if (p.n_ki > (uint32_t)LC_MAX_KP) {
        *p.status |= MAGE_LC_STATUS_OVER_LIMIT;
        for (uint32_t j = 0; j < L; j++) p.closure[j] = mage_loop_closure_assoc{0.f, 0.f, 0, -1};
    } else {
        mage::newpoints::make_frame(p.ki_pos3, p.ki_r9, p.ki_intr4, ki.frame);
        for (uint32_t t = 0; t < p.n_ki; t++) p.ki_mask[t] = p.ki_point[t] < 0;
        for (uint32_t j = 0; j < L; j++) {
            p.closure_verdict[j] = offer(c.gate, p, ki, sample[j], p.ki_mask, p.closure[j]);
            p.counts[1] += p.closure_verdict[j] == LC_ASSOCIATED;
        }
        for (uint32_t j = 0; j < L; j++)
            if (p.closure[j].keypoint >= 0) associate(c.tables, p, ki, sample[j], p.closure[j].keypoint);
    }

    // TryConnectMapPoints (ThreadSafeMap.cpp:733-780)
    AssocConsts cc = c.gate;
    cc.max_dist = c.connect_max_dist;
    cc.min_diff = c.connect_min_diff;
    for (uint32_t k = 0; k < p.n_kf; k++) {
        const uint32_t s0 = p.kf_start[k], nk = p.kf_start[k + 1] - s0;
        p.kf_modified[k] = 0;
        if (nk > (uint32_t)LC_MAX_KP) {
            *p.status |= MAGE_LC_STATUS_OVER_LIMIT;
            for (uint32_t j = 0; j < L; j++) p.connect[(size_t)j * p.n_kf + k] = mage_loop_closure_assoc{0.f, 0.f, 0, -1};
            continue;
        }
        Keyframe kf{p.kf_id[k], nk, p.kf_intr4 + 4ull * k, p.kf_kp + s0, p.kf_desc + 32ull * s0, p.kf_point + s0, {}};
        mage::newpoints::make_frame(p.kf_pos3 + 3ull * k, p.kf_r9 + 9ull * k, kf.intr4, kf.frame);
        for (uint32_t j = 0; j < L; j++) {
            mage_loop_closure_assoc& rec = p.connect[(size_t)j * p.n_kf + k];
            uint8_t& v = p.connect_verdict[(size_t)j * p.n_kf + k];
            if (p.closure[j].keypoint < 0) {
                rec = mage_loop_closure_assoc{0.f, 0.f, 0, -1};
                v = LC_NOT_SAMPLED;
                continue;
            }
            v = offer(cc, p, kf, sample[j], p.kf_mask + s0, rec);
        }
        // apply any found associations to the keyframe (:771-774)
        for (uint32_t j = 0; j < L; j++) {
            const int t = p.connect[(size_t)j * p.n_kf + k].keypoint;
            if (t < 0) continue;
            associate(c.tables, p, kf, sample[j], t);
            p.kf_modified[k] = 1;
            p.counts[2]++;
        }
    }
    return MAGE_OK;
}
