// Drives mage::hot::CreateInitialAssociations (include/mage/mage.hpp) on a problem read from a file:
//   u32 n_ki, n_kc, has_mask, device_plus_one; Ki pose (3 + 9 + 4 floats); n_ki keypoints; [n_ki mask bytes];
//   per Kc: pose (16 floats), u32 n_kp, keypoints, u32 n_matches, matches.
// Writes u32 n_points, the points, then per Kc the verdict bytes.  Exit 3: no usable device.
#include <cstdio>
#include <cstring>
#include <vector>

#include "mage/mage.hpp"

using namespace mage::hot;

template <typename T>
static bool rd(FILE* f, T* p, size_t n)
{
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}

static bool read_pose(FILE* f, KeyframeView& k)
{
    return rd(f, k.Position.data(), 3) && rd(f, k.Rotation.data(), 9) && rd(f, k.Intrinsics.data(), 4);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[4];
    if (!rd(f, hdr, 4)) return 2;
    KeyframeView ki{};
    std::vector<KeyPoint> ki_kp(hdr[0]);
    if (!read_pose(f, ki) || !rd(f, ki_kp.data(), ki_kp.size())) return 2;
    ki.KeyPoints = &ki_kp;
    std::vector<uint8_t> mask_bytes(hdr[2] ? hdr[0] : 0);
    if (!rd(f, mask_bytes.data(), mask_bytes.size())) return 2;
    std::vector<bool> mask(mask_bytes.begin(), mask_bytes.end());
    std::vector<KeyframeView> kc(hdr[1]);
    std::vector<std::vector<KeyPoint>> kc_kp(hdr[1]);
    std::vector<std::vector<DMatch>> matches(hdr[1]);
    for (uint32_t k = 0; k < hdr[1]; k++) {
        uint32_t n = 0;
        if (!read_pose(f, kc[k]) || !rd(f, &n, 1)) return 2;
        kc_kp[k].resize(n);
        if (!rd(f, kc_kp[k].data(), n) || !rd(f, &n, 1)) return 2;
        matches[k].resize(n);
        if (!rd(f, matches[k].data(), n)) return 2;
        kc[k].KeyPoints = &kc_kp[k];
    }
    fclose(f);
    std::vector<std::vector<uint8_t>> verdicts;
    std::vector<NewMapPoint> pts;
    try {
        pts = CreateInitialAssociations(NewMapPointsCreationSettings{}, ki, mask, kc, matches, &verdicts, (int)hdr[3] - 1);
    } catch (const Error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == MAGE_EDEVICE ? 3 : 4;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const uint32_t n = (uint32_t)pts.size();
    fwrite(&n, 4, 1, o);
    if (n) fwrite(pts.data(), sizeof(NewMapPoint), n, o);
    for (auto& v : verdicts)
        if (!v.empty()) fwrite(v.data(), 1, v.size(), o);
    fclose(o);
    return 0;
}
