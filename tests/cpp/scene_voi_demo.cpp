// Drives mage::hot::CalculateVolumeOfInterest (include/mage/mage.hpp) on a pose history read from a
// file: u32 n_kf, device_plus_one; i32 iterations, voxel_count_floor; the ten float settings in the
// reference's order (threshold, the three prominences, the two angles, pitch, roll, yaw, depth
// modifier); per keyframe 12 floats and {near, far}.
// Writes u32 returned, the mage_voi_result, the AxisAlignedVolume (6 floats, prefilled with 7) and the trace.
#include <cstdio>
#include <vector>

#include "mage/mage.hpp"

using namespace mage::hot;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[2];
    int32_t ints[2];
    float fl[10];
    if (fread(hdr, 4, 2, f) != 2 || fread(ints, 4, 2, f) != 2 || fread(fl, 4, 10, f) != 10) return 2;
    std::vector<VOIKeyframe> kf(hdr[0]);
    for (auto& k : kf)
        if (fread(k.WorldFromCamera.data(), 4, 12, f) != 12 || fread(&k.NearDepth, 4, 1, f) != 1 || fread(&k.FarDepth, 4, 1, f) != 1)
            return 2;
    fclose(f);
    VolumeOfInterestSettings s;
    s.Iterations = ints[0];
    s.VoxelCountFloor = ints[1];
    s.Threshold = fl[0];
    s.AwayProminence = fl[1];
    s.TowardProminence = fl[2];
    s.SideProminence = fl[3];
    s.KernelAngleXRads = fl[4];
    s.KernelAngleYRads = fl[5];
    s.KernelPitchRads = fl[6];
    s.KernelRollRads = fl[7];
    s.KernelYawRads = fl[8];
    s.KernelDepthModifier = fl[9];
    AxisAlignedVolume voi;
    voi.Min = {7.f, 7.f, 7.f};
    voi.Max = {7.f, 7.f, 7.f};
    mage_voi_result r{};
    std::vector<mage_voi_level> trace;
    uint32_t ok = 0;
    try {
        ok = CalculateVolumeOfInterest(kf, s, voi, &r, &trace, (int)hdr[1] - 1) ? 1u : 0u;
    } catch (const Error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == MAGE_EDEVICE ? 3 : 4;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&ok, 4, 1, o);
    fwrite(&r.status, 4, 1, o);
    fwrite(&r.levels_done, 4, 1, o);
    fwrite(voi.Min.data(), 4, 3, o);
    fwrite(voi.Max.data(), 4, 3, o);
    if (!trace.empty()) fwrite(trace.data(), sizeof(mage_voi_level), trace.size(), o);
    fclose(o);
    return 0;
}
