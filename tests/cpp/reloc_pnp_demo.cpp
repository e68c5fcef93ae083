// Drives mage::hot::PoseEstimator::PNPRansac (include/mage/mage.hpp) on 2D-3D points read from a file:
//   u32 n, device_plus_one, iterations; float confidence, max_error, intr[4] = {cx, cy, fx, fy};
//   n x 3 floats points3d; n x 2 floats points2d.
// Writes the mage_reloc_pnp_result, u32 found, n_inliers, and when found the pose (3 + 9 floats) and
// the inliers (int32).  Exit 3: no usable device; 6: over a limit.
#include <cstdio>
#include <vector>

#include "mage/mage.hpp"

using namespace mage::hot;

template <typename T>
static bool rd(FILE* f, T* p, size_t n)
{
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[3];
    float par[2];
    std::array<float, 4> intr;
    if (!rd(f, hdr, 3) || !rd(f, par, 2) || !rd(f, intr.data(), 4)) return 2;
    std::vector<std::array<float, 3>> p3(hdr[0]);
    std::vector<std::array<float, 2>> p2(hdr[0]);
    if (!rd(f, p3.data(), p3.size()) || !rd(f, p2.data(), p2.size())) return 2;
    fclose(f);
    PoseEstimator estimator(RelocalizationSettings{}, (int)hdr[1] - 1);
    ViewPose pose;
    std::vector<int> inliers;
    bool found = false;
    try {
        found = estimator.PNPRansac(intr, p3, p2, false, par[1], par[0], hdr[2], pose, inliers);
    } catch (const Error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == MAGE_EDEVICE ? 3 : (e.status == MAGE_EUNSUPPORTED ? 6 : 4);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&estimator.LastResult(), sizeof(mage_reloc_pnp_result), 1, o);
    const uint32_t n[2] = {found ? 1u : 0u, (uint32_t)inliers.size()};
    fwrite(n, 4, 2, o);
    if (found) {
        fwrite(pose.Position.data(), 4, 3, o);
        fwrite(pose.Rotation.data(), 4, 9, o);
        if (!inliers.empty()) fwrite(inliers.data(), 4, inliers.size(), o);
    }
    fclose(o);
    return 0;
}
