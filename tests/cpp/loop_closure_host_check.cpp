// loop_closure_host_check — mage_cheap_loop_closure_host's code as a stand-alone program
// (tests/test_loop_closure_sanitize.py builds it with -fsanitize=address,undefined): the twin's
// translation unit is compiled in, no library and no GPU.
// Usage: loop_closure_host_check IN OUT, or loop_closure_host_check sampler (the kernels' sampling by
// index arithmetic, loopclose_math.hpp make_sampler, against the reference's counter loop).
// IN: mage_loop_closure_settings; uint32 n_map, obs_pitch, offset, n_keyframes, ki_id, n_ki, n_kf, L
// (the sample's size, which sizes the per-place buffers); the states, the observations; Ki's pos3[3],
// r9[9], intr4[4], keypoints, descriptors, ki_point; kf_start[n_kf + 1], kf_id, the poses (pos3 x n_kf,
// r9 x, intr4 x), the keypoints, descriptors, kf_point and mask bytes of all keyframes.
// OUT: uint32 return code, counts[3], status; the states, the observations; sample_index, closure,
// closure_verdict, connect, connect_verdict (L places each); ki_mask, the keyframes' masks, kf_modified.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "loopclose.cpp"

namespace mage {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace mage

template <class T>
static bool take(FILE* f, std::vector<T>& v)
{
    return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

template <class T>
static void put(FILE* f, const std::vector<T>& v)
{
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

template <class T>
static std::vector<T> filled(size_t n)
{
    std::vector<T> v(n);
    if (n) std::memset(static_cast<void*>(v.data()), 0xA5, sizeof(T) * n);
    return v;
}

static int sampler_main()
{
    using namespace mage::loopclose;
    const uint32_t offsets[] = {0u, 1u, 2u, 5u, 41u, 199u, 200u, 0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFDBu, 0xFFFFFF00u, 0xFFFFFC00u};
    long bad = 0;
    for (uint32_t max : {1u, 2u, 3u, 7u, 200u, 1024u})
        for (uint32_t n = 0; n < 1500; n += n < 40 ? 1 : 37)
            for (uint32_t offset : offsets) {
                std::vector<uint32_t> sample;  // Map.cpp:319-333, cut at max
                const uint32_t step = n / max + 1;
                uint32_t count = offset;
                for (uint32_t i = 0; i < n && sample.size() < max; i++) {
                    count++;
                    if (count % step != 0) continue;
                    sample.push_back(i);
                }
                const Sampler s = make_sampler(n, max, offset);
                std::vector<int> slot(n, -1);
                for (size_t j = 0; j < sample.size(); j++) slot[sample[j]] = (int)j;
                bool ok = s.count == sample.size();
                for (uint32_t j = 0; ok && j < s.count; j++) ok = sample_index(s, j) == sample[j];
                for (uint32_t i = 0; ok && i < n; i++) ok = sample_slot(s, i) == slot[i];
                if (!ok) {
                    fprintf(stderr, "sampler differs: n %u max %u offset %u\n", n, max, offset);
                    bad++;
                }
            }
    return bad ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "sampler") return sampler_main();
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    mage_loop_closure_settings s;
    uint32_t h[8];
    if (fread(&s, sizeof(s), 1, in) != 1 || fread(h, 4, 8, in) != 8) return 2;
    const uint32_t n_map = h[0], obs_pitch = h[1], n_ki = h[5], n_kf = h[6], L = h[7];
    // exact sizes, so that a step past a count is a step past an allocation
    std::vector<mage_map_point_state> state(n_map);
    std::vector<mage_map_point_obs> obs((size_t)n_map * obs_pitch);
    std::vector<float> ki_pose(16);
    std::vector<mage_keypoint> ki_kp(n_ki);
    std::vector<uint8_t> ki_desc(32 * (size_t)n_ki);
    std::vector<int32_t> ki_point(n_ki);
    std::vector<uint32_t> kf_start(n_kf + 1);
    std::vector<int32_t> kf_id(n_kf);
    std::vector<float> kf_pos3(3 * (size_t)n_kf), kf_r9(9 * (size_t)n_kf), kf_intr4(4 * (size_t)n_kf);
    if (!take(in, state) || !take(in, obs) || !take(in, ki_pose) || !take(in, ki_kp) || !take(in, ki_desc) ||
        !take(in, ki_point) || !take(in, kf_start) || !take(in, kf_id) || !take(in, kf_pos3) || !take(in, kf_r9) ||
        !take(in, kf_intr4))
        return 2;
    const uint32_t total = kf_start[n_kf];
    std::vector<mage_keypoint> kf_kp(total);
    std::vector<uint8_t> kf_desc(32 * (size_t)total), kf_mask(total);
    std::vector<int32_t> kf_point(total);
    if (!take(in, kf_kp) || !take(in, kf_desc) || !take(in, kf_point) || !take(in, kf_mask)) return 2;
    fclose(in);
    auto sample = filled<uint32_t>(L);
    auto closure = filled<mage_loop_closure_assoc>(L), connect = filled<mage_loop_closure_assoc>((size_t)L * n_kf);
    auto closure_verdict = filled<uint8_t>(L), connect_verdict = filled<uint8_t>((size_t)L * n_kf);
    auto ki_mask = filled<uint8_t>(n_ki), kf_modified = filled<uint8_t>(n_kf);
    uint32_t counts[3], status;
    mage_loop_closure_problem p{};
    p.struct_size = (uint32_t)sizeof(p);
    p.n_map = n_map;
    p.state = state.data();
    p.obs = obs.data();
    p.obs_pitch = obs_pitch;
    p.offset = h[2];
    p.n_keyframes = h[3];
    p.ki_id = (int32_t)h[4];
    p.n_ki = n_ki;
    p.ki_pos3 = ki_pose.data();
    p.ki_r9 = ki_pose.data() + 3;
    p.ki_intr4 = ki_pose.data() + 12;
    p.ki_kp = ki_kp.data();
    p.ki_desc = ki_desc.data();
    p.ki_point = ki_point.data();
    p.n_kf = n_kf;
    p.kf_id = kf_id.data();
    p.kf_pos3 = kf_pos3.data();
    p.kf_r9 = kf_r9.data();
    p.kf_intr4 = kf_intr4.data();
    p.kf_kp = kf_kp.data();
    p.kf_desc = kf_desc.data();
    p.kf_point = kf_point.data();
    p.kf_start = kf_start.data();
    p.kf_mask = kf_mask.data();
    // a buffer of no elements has no address to give: the entry wants non-null pointers for a map
    static uint32_t none[4];
    p.sample_index = L ? sample.data() : none;
    p.closure = L ? closure.data() : reinterpret_cast<mage_loop_closure_assoc*>(none);
    p.closure_verdict = L ? closure_verdict.data() : reinterpret_cast<uint8_t*>(none);
    p.connect = L && n_kf ? connect.data() : reinterpret_cast<mage_loop_closure_assoc*>(none);
    p.connect_verdict = L && n_kf ? connect_verdict.data() : reinterpret_cast<uint8_t*>(none);
    p.ki_mask = ki_mask.data();
    p.kf_modified = kf_modified.data();
    p.counts = counts;
    p.status = &status;
    const uint32_t rc = (uint32_t)mage_cheap_loop_closure_host(&s, &p);
    if (rc != MAGE_OK && rc != MAGE_ECAPACITY) {
        fprintf(stderr, "status %u: %s\n", rc, mage::g_error.c_str());
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&rc, 4, 1, o);
    fwrite(counts, 4, 3, o);
    fwrite(&status, 4, 1, o);
    put(o, state);
    put(o, obs);
    put(o, sample);
    put(o, closure);
    put(o, closure_verdict);
    put(o, connect);
    put(o, connect_verdict);
    put(o, ki_mask);
    put(o, kf_mask);
    put(o, kf_modified);
    fclose(o);
    return 0;
}
