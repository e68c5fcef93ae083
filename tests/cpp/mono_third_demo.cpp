// Drives mage::hot::MonoMapInit::LocateThirdFrame (include/mage/mage.hpp) on a problem read from a file:
//   u32 n, n0, n1, n2, device_plus_one, n_flags_plus_one (0: no bundle-adjustment outcome); float intr[4], pos3[6],
//   r9[18], points[3 n]; i32 idx0[n], idx1[n]; desc0, desc1 (32 bytes each); n2 keypoints and descriptors;
//   then n_flags outlier bytes, float opt_pos3[3], opt_r9[9], mean_sq.
// Writes the mage_mono_init_third_result and, when a frame is returned, u32 n_observations, the per-point
// arrays (keypoints, verdict bytes, distances, projections), the mask and the observations (uv, point,
// camera, information).  Exit 3: no usable device; 5: std::out_of_range; 6: over a limit.
#include <cstdio>
#include <vector>

#include "mage/mage.hpp"

using namespace mage::hot;

template <typename T>
static bool rd(FILE* f, T* p, size_t n)
{
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}

template <typename T>
static void wr(FILE* f, const std::vector<T>& v)
{
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[6];
    if (!rd(f, hdr, 6)) return 2;
    const uint32_t n = hdr[0], n0 = hdr[1], n1 = hdr[2], n2 = hdr[3];
    MonoFrame third;
    std::array<float, 6> pos;
    std::array<float, 18> rot;
    std::vector<float> points(3 * (size_t)n);
    std::vector<int32_t> idx0(n), idx1(n);
    std::vector<uint8_t> d0(32 * (size_t)n0), d1(32 * (size_t)n1), d2(32 * (size_t)n2);
    std::vector<KeyPoint> kp(n2);
    if (!rd(f, third.Intrinsics.data(), 4) || !rd(f, pos.data(), 6) || !rd(f, rot.data(), 18) ||
        !rd(f, points.data(), points.size()) || !rd(f, idx0.data(), n) || !rd(f, idx1.data(), n) ||
        !rd(f, d0.data(), d0.size()) || !rd(f, d1.data(), d1.size()) || !rd(f, kp.data(), n2) || !rd(f, d2.data(), d2.size()))
        return 2;
    MonoMapInit::ThirdFrameBA ba;
    if (hdr[5]) {
        ba.Outlier.resize(hdr[5] - 1);
        if (!rd(f, ba.Outlier.data(), ba.Outlier.size()) || !rd(f, ba.Position.data(), 3) || !rd(f, ba.Rotation.data(), 9) ||
            !rd(f, &ba.MeanSquareError, 1))
            return 2;
    }
    fclose(f);
    third.KeyPoints = &kp;
    third.Descriptors = d2.data();
    MonoMapInit init(MonoMapInitializationSettings{}, (int)hdr[4] - 1);
    std::optional<MonoThirdFrame> t;
    try {
        t = init.LocateThirdFrame(pos, rot, points, idx0, idx1, d0.data(), n0, d1.data(), n1, third, 1, hdr[5] ? &ba : nullptr);
    } catch (const Error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == MAGE_EDEVICE ? 3 : (e.status == MAGE_EUNSUPPORTED ? 6 : 4);
    } catch (const std::out_of_range& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&init.LastThirdResult(), sizeof(mage_mono_init_third_result), 1, o);
    if (t) {
        const uint32_t na = (uint32_t)t->ObservationPoints.size();
        fwrite(&na, 4, 1, o);
        fwrite(t->Position.data(), 4, 3, o);
        fwrite(t->Rotation.data(), 4, 9, o);
        wr(o, t->KeyPointOf);
        wr(o, t->Verdicts);
        wr(o, t->Distances);
        wr(o, t->Projections);
        wr(o, t->Unassociated);
        wr(o, t->Observations);
        wr(o, t->ObservationPoints);
        wr(o, t->ObservationCameras);
        wr(o, t->ObservationInformation);
    }
    fclose(o);
    return 0;
}
