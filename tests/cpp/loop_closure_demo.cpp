// loop_closure_demo — mage::hot::CheapLoopClosureAndConnect and UpdateMapPoint through
// include/mage/mage.hpp (tests/test_loop_closure_facade.py).  Usage: loop_closure_demo IN OUT DEVICE
// (DEVICE < 0: the CPU backend).  IN is the input file of tests/cpp/loop_closure_host_check.cpp.
// OUT: uint32 sample size, the sample; uint32 count and the closure's {map point, keypoint} pairs;
// per covisible keyframe a uint32 count, its pairs and its modified byte; per map point its state and
// its observations; the covisible keyframes' masks; UpdateMapPoint's state of map point 0 (if any).
// Exit code 5 when the facade throws Error(MAGE_EUNSUPPORTED).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mage/mage.hpp"

using namespace mage::hot;

template <class T>
static bool take(FILE* f, std::vector<T>& v)
{
    return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

static void put_pairs(FILE* o, const std::vector<LoopClosureAssociation>& a)
{
    const uint32_t n = (uint32_t)a.size();
    fwrite(&n, 4, 1, o);
    if (n) fwrite(a.data(), sizeof(LoopClosureAssociation), n, o);
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    mage_loop_closure_settings s;
    uint32_t h[8];
    if (fread(&s, sizeof(s), 1, in) != 1 || fread(h, 4, 8, in) != 8) return 2;
    const uint32_t n_map = h[0], obs_pitch = h[1], n_ki = h[5], n_kf = h[6];
    std::vector<mage_map_point_state> state(n_map);
    std::vector<mage_map_point_obs> obs((size_t)n_map * obs_pitch);
    std::vector<float> ki_pose(16);
    std::vector<KeyPoint> ki_kp(n_ki);
    std::vector<Descriptor> ki_desc(n_ki);
    std::vector<int32_t> ki_point(n_ki);
    std::vector<uint32_t> start(n_kf + 1);
    std::vector<int32_t> kf_id(n_kf);
    std::vector<float> kf_pos3(3 * (size_t)n_kf), kf_r9(9 * (size_t)n_kf), kf_intr4(4 * (size_t)n_kf);
    if (!take(in, state) || !take(in, obs) || !take(in, ki_pose) || !take(in, ki_kp) || !take(in, ki_desc) ||
        !take(in, ki_point) || !take(in, start) || !take(in, kf_id) || !take(in, kf_pos3) || !take(in, kf_r9) ||
        !take(in, kf_intr4))
        return 2;
    const uint32_t total = start[n_kf];
    std::vector<KeyPoint> all_kp(total);
    std::vector<Descriptor> all_desc(total);
    std::vector<int32_t> all_point(total);
    std::vector<uint8_t> all_mask(total);
    if (!take(in, all_kp) || !take(in, all_desc) || !take(in, all_point) || !take(in, all_mask)) return 2;
    fclose(in);

    CheapLoopClosureSettings settings;
    settings.MaxMapPoints = s.max_map_points;
    settings.MinKeyframe = s.min_keyframes;
    settings.MatchSearchRadius = s.search_radius;
    settings.MinDegreesBetweenCurrentViewAndMapPointView = s.min_view_degrees;
    settings.ImageBorder = s.image_border;
    settings.ImageWidth = s.width;
    settings.ImageHeight = s.height;
    settings.NumLevels = s.num_levels;
    settings.PyramidScale = s.pyramid_scale;
    settings.CheapLoopClosureMaxHammingDistance = s.closure_max_hamming_distance;
    settings.CheapLoopClosureMinHammingDifference = s.closure_min_hamming_difference;
    settings.ConnectMaxHammingDistance = s.connect_max_hamming_distance;
    settings.ConnectMinHammingDifference = s.connect_min_hamming_difference;

    std::vector<MapPointView> map(n_map);
    for (uint32_t i = 0; i < n_map; i++) {
        map[i].State = state[i];
        map[i].Observations.assign(obs.begin() + (size_t)i * obs_pitch, obs.begin() + (size_t)i * obs_pitch + state[i].n_obs);
    }
    auto view = [](const float* pos3, const float* r9, const float* intr4, const std::vector<KeyPoint>* kp) {
        KeyframeView v;
        std::copy(pos3, pos3 + 3, v.Position.begin());
        std::copy(r9, r9 + 9, v.Rotation.begin());
        std::copy(intr4, intr4 + 4, v.Intrinsics.begin());
        v.KeyPoints = kp;
        return v;
    };
    LoopClosureKeyframe Ki;
    Ki.Id = (int)h[4];
    Ki.View = view(ki_pose.data(), ki_pose.data() + 3, ki_pose.data() + 12, &ki_kp);
    Ki.Descriptors = &ki_desc;
    Ki.KeypointMapPoints = &ki_point;
    std::vector<std::vector<KeyPoint>> kps(n_kf);
    std::vector<std::vector<Descriptor>> descs(n_kf);
    std::vector<std::vector<int32_t>> points(n_kf);
    std::vector<std::vector<bool>> masks(n_kf);
    std::vector<LoopClosureKeyframe> kfs(n_kf);
    for (uint32_t k = 0; k < n_kf; k++) {
        kps[k].assign(all_kp.begin() + start[k], all_kp.begin() + start[k + 1]);
        descs[k].assign(all_desc.begin() + start[k], all_desc.begin() + start[k + 1]);
        points[k].assign(all_point.begin() + start[k], all_point.begin() + start[k + 1]);
        for (uint32_t t = start[k]; t < start[k + 1]; t++) masks[k].push_back(all_mask[t] != 0);
        kfs[k].Id = kf_id[k];
        kfs[k].View = view(&kf_pos3[3 * k], &kf_r9[9 * k], &kf_intr4[4 * k], &kps[k]);
        kfs[k].Descriptors = &descs[k];
        kfs[k].KeypointMapPoints = &points[k];
        kfs[k].UnassociatedKeypointMask = &masks[k];
    }
    const int device = atoi(argv[3]);
    CheapLoopClosureResult r;
    try {
        r = CheapLoopClosureAndConnect(settings, map, h[2], h[3], Ki, kfs, device);
    } catch (const Error& e) {
        fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const uint32_t L = (uint32_t)r.Sample.size();
    fwrite(&L, 4, 1, o);
    if (L) fwrite(r.Sample.data(), 4, L, o);
    put_pairs(o, r.Associations);
    for (uint32_t k = 0; k < n_kf; k++) {
        put_pairs(o, r.Connected[k]);
        const uint8_t m = r.Modified[k];
        fwrite(&m, 1, 1, o);
    }
    for (const MapPointView& p : map) {
        fwrite(&p.State, sizeof(p.State), 1, o);
        if (!p.Observations.empty()) fwrite(p.Observations.data(), sizeof(MapPointObservation), p.Observations.size(), o);
    }
    for (uint32_t k = 0; k < n_kf; k++)
        for (bool b : masks[k]) {
            const uint8_t m = b;
            fwrite(&m, 1, 1, o);
        }
    if (n_map) {
        const MapPointState st = UpdateMapPoint(settings, {map[0].State.pos[0], map[0].State.pos[1], map[0].State.pos[2]},
                                                map[0].Observations, device);
        fwrite(&st, sizeof(st), 1, o);
    }
    fclose(o);
    return 0;
}
