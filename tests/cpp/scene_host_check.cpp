// scene_host_check — mage_bounding_plane_depths_host's code as a stand-alone program
// (tests/test_scene_sanitize.py builds it with -fsanitize=address,undefined): the twin's translation
// unit is compiled in, no library and no GPU.  Usage: scene_host_check IN OUT, or scene_host_check voi IN
// OUT for mage_volume_of_interest_host (IN: mage_voi_settings; uint32 n_kf; the matrices, 12 floats
// each; the {near, far} pairs.  OUT: mage_voi_result, then `iterations` trace records).
// IN: mage_bounding_depth_settings; uint32 width, height, n_kp, n_points, cap; pos3[3], r9[9],
// intr4[4]; the keypoints, the map points (4 floats each), the keypoint indices.
// OUT: mage_depth_result, then the sparse records (n_points, none for an OVER_LIMIT frame).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "scene_depth.cpp"
#include "scene_voi.cpp"

namespace mage {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace mage

template <class T>
static bool take(FILE* f, T* p, size_t n)
{
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}

static int voi_main(const char* fin, const char* fout)
{
    FILE* in = fopen(fin, "rb");
    if (!in) return 2;
    mage_voi_settings s;
    uint32_t n_kf;
    if (!take(in, &s, 1) || !take(in, &n_kf, 1)) return 2;
    std::vector<float> m(12 * (size_t)n_kf), nf(2 * (size_t)n_kf);  // exact sizes
    if (!take(in, m.data(), m.size()) || !take(in, nf.data(), nf.size())) return 2;
    fclose(in);
    mage_voi_result r;
    std::memset(&r, 0xA5, sizeof(r));
    std::vector<mage_voi_level> trace((size_t)(s.iterations > 0 ? s.iterations : 0));
    if (!trace.empty()) std::memset(trace.data(), 0xA5, sizeof(mage_voi_level) * trace.size());
    const mage_status st = mage_volume_of_interest_host(&s, m.data(), nf.data(), nullptr, 0, nullptr, n_kf, &r, trace.data());
    if (st != MAGE_OK) {
        fprintf(stderr, "status %d: %s\n", (int)st, mage::g_error.c_str());
        return 1;
    }
    FILE* o = fopen(fout, "wb");
    if (!o) return 2;
    fwrite(&r, sizeof(r), 1, o);
    if (!trace.empty()) fwrite(trace.data(), sizeof(mage_voi_level), trace.size(), o);
    fclose(o);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && std::string(argv[1]) == "voi") return voi_main(argv[2], argv[3]);
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    mage_bounding_depth_settings s;
    uint32_t h[5];
    float pose[12], intr[4];
    if (!take(in, &s, 1) || !take(in, h, 5) || !take(in, pose, 12) || !take(in, intr, 4)) return 2;
    const uint32_t width = h[0], height = h[1], n_kp = h[2], n_points = h[3], cap = h[4];
    // exact sizes, so that a step past a count is a step past an allocation
    std::vector<mage_keypoint> kp(n_kp);
    std::vector<float> map(4 * (size_t)n_points);
    std::vector<int32_t> index(n_points);
    if (!take(in, kp.data(), n_kp) || !take(in, map.data(), map.size()) || !take(in, index.data(), n_points)) return 2;
    fclose(in);
    mage_depth_result r;
    std::vector<mage_projected_point> sparse(cap);
    const mage_status st = mage_bounding_plane_depths_host(&s, pose, pose + 3, intr, width, height, kp.data(), n_kp, map.data(),
                                                           index.data(), n_points, cap, &r, sparse.data());
    if (st != MAGE_OK) {
        fprintf(stderr, "status %d: %s\n", (int)st, mage::g_error.c_str());
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&r, sizeof(r), 1, o);
    const size_t n = (r.status & MAGE_BD_STATUS_OVER_LIMIT) ? 0 : r.n_points;
    if (n) fwrite(sparse.data(), sizeof(mage_projected_point), n, o);
    fclose(o);
    return 0;
}
