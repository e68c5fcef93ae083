// Drives mage::hot::PoseEstimator::TryEstimatePoseFromCandidates (include/mage/mage.hpp) on one lost
// frame with its candidates read from a file:
//   u32 n_candidates, device_plus_one, n_kp; float intr[4] = {cx, cy, fx, fy};
//   n_kp keypoints, n_kp x 32 bytes descriptors; then per candidate
//   u32 n_kf, n_order, n_matches; n_kf x 4 floats map points, n_kf keypoints, n_kf x 32 bytes
//   descriptors, n_order int32 order, n_matches DMatch.
// Writes int32 index, u32 n_associations, the pose (3 + 9 floats), the associations (2 x int32
// each), then the candidates' mage_reloc_guided_result records.  Exit 3: no usable device; 6: not
// supported (the CPU backend).
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
    std::array<float, 4> intr;
    if (!rd(f, hdr, 3) || !rd(f, intr.data(), 4)) return 2;
    std::vector<KeyPoint> kp(hdr[2]);
    std::vector<Descriptor> desc(hdr[2]);
    if (!rd(f, kp.data(), kp.size()) || !rd(f, desc.data(), desc.size())) return 2;
    std::vector<PoseEstimator::Candidate> cands(hdr[0]);
    std::vector<std::vector<DMatch>> matches(hdr[0]);
    for (uint32_t c = 0; c < hdr[0]; c++) {
        uint32_t n[3];
        if (!rd(f, n, 3)) return 2;
        PoseEstimator::Candidate& k = cands[c];
        k.MapPoints.resize(n[0]);
        k.KeyPoints.resize(n[0]);
        k.Descriptors.resize(n[0]);
        k.Order.resize(n[1]);
        matches[c].resize(n[2]);
        if (!rd(f, k.MapPoints.data(), n[0]) || !rd(f, k.KeyPoints.data(), n[0]) || !rd(f, k.Descriptors.data(), n[0]) ||
            !rd(f, k.Order.data(), n[1]) || !rd(f, matches[c].data(), n[2]))
            return 2;
    }
    fclose(f);
    PoseEstimator estimator(RelocalizationSettings{}, (int)hdr[1] - 1);
    ViewPose pose;
    std::vector<PoseEstimator::Association> assoc;
    int index = -1;
    try {
        index = estimator.TryEstimatePoseFromCandidates(intr, cands, matches, kp, desc, pose, assoc);
    } catch (const Error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == MAGE_EDEVICE ? 3 : (e.status == MAGE_EUNSUPPORTED ? 6 : 4);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t i32 = index;
    const uint32_t na = (uint32_t)assoc.size();
    fwrite(&i32, 4, 1, o);
    fwrite(&na, 4, 1, o);
    fwrite(pose.Position.data(), 4, 3, o);
    fwrite(pose.Rotation.data(), 4, 9, o);
    if (na) fwrite(assoc.data(), sizeof(PoseEstimator::Association), na, o);
    const auto& rs = estimator.LastCandidates();
    if (!rs.empty()) fwrite(rs.data(), sizeof(mage_reloc_guided_result), rs.size(), o);
    fclose(o);
    return 0;
}
