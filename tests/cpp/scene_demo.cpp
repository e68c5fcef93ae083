// Drives mage::hot::CalculateBoundingPlaneDepthsForKeyframe (include/mage/mage.hpp) on a frame read
// from a file:
//   u32 n_kp, n_points, width, height, device_plus_one; the six BoundingDepthSettings floats;
//   pos3[3], r9[9], intr[4] = {cx, cy, fx, fy}; n_kp keypoints; n_points x 4 floats; n_points int32.
// Writes NearPlaneDepth, FarPlaneDepth, the mage_depth_result and the sparse records.
// Exit 3: no usable device; 5: a bad keypoint index; 6: over the limit.
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
    uint32_t hdr[5];
    float set[6];
    ViewPose pose;
    std::array<float, 4> intr;
    if (!rd(f, hdr, 5) || !rd(f, set, 6) || !rd(f, pose.Position.data(), 3) || !rd(f, pose.Rotation.data(), 9) ||
        !rd(f, intr.data(), 4))
        return 2;
    std::vector<KeyPoint> kp(hdr[0]);
    std::vector<std::array<float, 4>> points(hdr[1]);
    std::vector<int32_t> index(hdr[1]);
    if (!rd(f, kp.data(), kp.size()) || !rd(f, points.data(), points.size()) || !rd(f, index.data(), index.size())) return 2;
    fclose(f);
    BoundingDepthSettings s;
    s.RegionOfInterestMinX = set[0];
    s.RegionOfInterestMinY = set[1];
    s.RegionOfInterestMaxX = set[2];
    s.RegionOfInterestMaxY = set[3];
    s.NearDepthSoftness = set[4];
    s.FarDepthSoftness = set[5];
    InternalDepth d;
    try {
        d = CalculateBoundingPlaneDepthsForKeyframe(pose, intr, hdr[2], hdr[3], kp, points, index, s, (int)hdr[4] - 1);
    } catch (const Error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == MAGE_EDEVICE ? 3 : (e.status == MAGE_EUNSUPPORTED ? 6 : 4);
    } catch (const std::out_of_range& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&d.NearPlaneDepth, 4, 1, o);
    fwrite(&d.FarPlaneDepth, 4, 1, o);
    fwrite(&d.Result, sizeof(mage_depth_result), 1, o);
    if (!d.SparseDepth.empty()) fwrite(d.SparseDepth.data(), sizeof(ProjectedPoint), d.SparseDepth.size(), o);
    fclose(o);
    return 0;
}
