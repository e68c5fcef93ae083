// reloc_guided_host_check — mage_reloc_guided_host's code as a stand-alone program
// (tests/test_reloc_guided_sanitize.py builds it with -fsanitize=address,undefined): the twin's
// translation unit is compiled in, no library and no GPU.  Usage: reloc_guided_host_check IN OUT.
// IN: mage_reloc_settings; uint32 pnp_ok, n_kf, has_order, n_order, n_kp, cap, has_radius, n_radius,
// has_flags, n_flags; intr4[4], the first pose (3 + 9 floats), the second pose (3 + 9 floats);
// map_xyzi, kf_kp, kf_desc, order, kp, radius matches, flags.
// OUT: mage_reloc_guided_result, the queries (keypoints, positions, descriptors, reference indices;
// n_queries each), the association records (n_in_front), the bundle adjustment's inputs (n_in_front
// when the second bundle adjustment is reached).
#include <cstdio>
#include <string>
#include <vector>

#include "reloc_guided.cpp"

namespace mage {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace mage

template <class T>
static bool take(FILE* f, T* p, size_t n)
{
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}

template <class T>
static void put(FILE* f, const T* p, size_t n)
{
    if (n) fwrite(p, sizeof(T), n, f);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    mage_reloc_settings s;
    uint32_t h[10];
    float intr[4], first[12], second[12];
    if (!take(in, &s, 1) || !take(in, h, 10) || !take(in, intr, 4) || !take(in, first, 12) || !take(in, second, 12)) return 2;
    const uint32_t pnp_ok = h[0], n_kf = h[1], has_order = h[2], n_order = h[3], n_kp = h[4], cap = h[5], has_radius = h[6],
                   n_radius = h[7], has_flags = h[8], n_flags = h[9];
    std::vector<float> map(4 * (size_t)n_kf);
    std::vector<mage_keypoint> kfkp(n_kf), kp(n_kp);
    std::vector<uint8_t> kfd(32 * (size_t)n_kf), flags(n_flags);
    std::vector<int32_t> order(n_order);
    std::vector<mage_dmatch> rm(n_radius);
    if (!take(in, map.data(), map.size()) || !take(in, kfkp.data(), n_kf) || !take(in, kfd.data(), kfd.size()) ||
        !take(in, order.data(), n_order) || !take(in, kp.data(), n_kp) || !take(in, rm.data(), n_radius) ||
        !take(in, flags.data(), n_flags))
        return 2;
    fclose(in);
    // exact sizes, so that a step past a count is a step past an allocation; never a null pointer
    // for a present input (an empty vector's data() may be null)
    static const mage_dmatch no_match{};
    static const uint8_t no_flag = 0;
    static const int32_t no_order = 0;
    mage_reloc_guided_result r;
    std::vector<mage_keypoint> qkp(cap);
    std::vector<float> qpos(2 * (size_t)cap), p3(3 * (size_t)cap), uv(2 * (size_t)cap), info(cap);
    std::vector<uint8_t> qd(32 * (size_t)cap);
    std::vector<int32_t> qref(cap), assoc(2 * (size_t)cap);
    const mage_status st = mage_reloc_guided_host(
        &s, (int32_t)pnp_ok, intr, map.data(), kfkp.data(), kfd.data(), n_kf,
        has_order ? (n_order ? order.data() : &no_order) : nullptr, n_order, kp.data(), n_kp, first, first + 3, cap, &r,
        qkp.data(), qpos.data(), qd.data(), qref.data(), has_radius ? (n_radius ? rm.data() : &no_match) : nullptr, n_radius,
        assoc.data(), p3.data(), uv.data(), info.data(), has_flags ? (n_flags ? flags.data() : &no_flag) : nullptr,
        has_flags ? second : nullptr, has_flags ? second + 3 : nullptr);
    if (st != MAGE_OK) {
        fprintf(stderr, "status %d: %s\n", (int)st, mage::g_error.c_str());
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const size_t nq = r.n_queries, n = r.n_in_front;
    const size_t nb = has_radius && (r.verdict == MAGE_RG_OK || r.verdict == MAGE_RG_FEW_BA_INLIERS) ? n : 0;
    put(o, &r, 1);
    put(o, qkp.data(), nq);
    put(o, qpos.data(), 2 * nq);
    put(o, qd.data(), 32 * nq);
    put(o, qref.data(), nq);
    put(o, assoc.data(), 2 * n);
    put(o, p3.data(), 3 * nb);
    put(o, uv.data(), 2 * nb);
    put(o, info.data(), nb);
    fclose(o);
    return 0;
}
