// Drives mage::hot::LocallyAssociateNewAssociations (include/mage/mage.hpp) on a problem read from a file:
//   u32 n_points, n_ki, n_kf, device_plus_one, num_levels; f32 search radius, max angle, image border;
//   i32 max Hamming distance, min Hamming difference; the points; Ki's descriptors;
//   per keyframe: pose (16 floats), i32 slot, u32 n_kp, keypoints, descriptors, mask bytes.
// Writes the records and the verdict bytes (points x keyframes), then per keyframe the mask bytes.
// With a third argument "creation" the file goes on with Ki's pose (16 floats), its n_ki keypoints,
// u32 max grid count, u32 has_mask [, n_ki mask bytes] and per keyframe u32 n_matches and the matches; the program
// then drives mage::hot::NewMapPointsCreation instead (the points in the file are not used) and writes
// u32 n_points, per point the 48-byte record, u32 n and n {i32 keyframe, u32 keypoint} pairs, then
// per keyframe the mask bytes.  Exit 3: no usable device.
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

int main(int argc, char** argv)
{
    const bool creation = argc == 4 && std::strcmp(argv[3], "creation") == 0;
    if (argc != 3 && !creation) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[5];
    float fs[3];
    int32_t is[2];
    if (!rd(f, hdr, 5) || !rd(f, fs, 3) || !rd(f, is, 2)) return 2;
    std::vector<NewMapPoint> points(hdr[0]);
    std::vector<Descriptor> ki_desc(hdr[1]);
    if (!rd(f, points.data(), points.size()) || !rd(f, ki_desc.data(), ki_desc.size())) return 2;
    const uint32_t n_kf = hdr[2];
    std::vector<std::vector<KeyPoint>> kp(n_kf);
    std::vector<std::vector<Descriptor>> desc(n_kf);
    std::vector<std::vector<bool>> mask(n_kf);
    std::vector<MappingKeyframeView> kfs(n_kf);
    for (uint32_t k = 0; k < n_kf; k++) {
        KeyframeView& v = kfs[k].View;
        int32_t slot = -1;
        uint32_t n = 0;
        if (!rd(f, v.Position.data(), 3) || !rd(f, v.Rotation.data(), 9) || !rd(f, v.Intrinsics.data(), 4) ||
            !rd(f, &slot, 1) || !rd(f, &n, 1))
            return 2;
        kp[k].resize(n);
        desc[k].resize(n);
        std::vector<uint8_t> bytes(n);
        if (!rd(f, kp[k].data(), n) || !rd(f, desc[k].data(), n) || !rd(f, bytes.data(), n)) return 2;
        mask[k].assign(bytes.begin(), bytes.end());
        v.KeyPoints = &kp[k];
        kfs[k].Descriptors = &desc[k];
        kfs[k].UnassociatedKeypointMask = &mask[k];
        kfs[k].Slot = slot;
    }
    NewMapPointsCreationSettings s;
    s.NumLevels = hdr[4];
    NewPointsAssociationSettings a;
    a.NewMapPointsSearchRadius = fs[0];
    a.MaxKeyframeAngleDegrees = fs[1];
    a.KiImageBorder = fs[2];
    a.MaxHammingDistance = is[0];
    a.MinHammingDifference = is[1];
    if (creation) {
        KeyframeView ki{};
        std::vector<KeyPoint> ki_kp(hdr[1]);
        uint32_t has_mask = 0, grid_cap = 0;
        if (!rd(f, ki.Position.data(), 3) || !rd(f, ki.Rotation.data(), 9) || !rd(f, ki.Intrinsics.data(), 4) ||
            !rd(f, ki_kp.data(), ki_kp.size()) || !rd(f, &grid_cap, 1) || !rd(f, &has_mask, 1))
            return 2;
        ki.KeyPoints = &ki_kp;
        s.NewPointMaxGridCount = grid_cap;
        std::vector<uint8_t> bytes(has_mask ? hdr[1] : 0);
        if (!rd(f, bytes.data(), bytes.size())) return 2;
        std::vector<bool> ki_mask(bytes.begin(), bytes.end());
        std::vector<std::vector<DMatch>> matches(n_kf);
        for (uint32_t k = 0; k < n_kf; k++) {
            uint32_t n = 0;
            if (!rd(f, &n, 1)) return 2;
            matches[k].resize(n);
            if (!rd(f, matches[k].data(), n)) return 2;
        }
        fclose(f);
        std::vector<MapPointKeyframeAssociations> made;
        try {
            made = NewMapPointsCreation(s, a, ki, ki_desc, ki_mask, kfs, matches, (int)hdr[3] - 1);
        } catch (const Error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return e.status == MAGE_EDEVICE ? 3 : 4;
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        const uint32_t n = (uint32_t)made.size();
        fwrite(&n, 4, 1, o);
        for (const MapPointKeyframeAssociations& m : made) {
            const uint32_t na = (uint32_t)m.Keyframes.size();
            fwrite(&m.MapPoint, sizeof(NewMapPoint), 1, o);
            fwrite(&na, 4, 1, o);
            fwrite(m.Keyframes.data(), sizeof(KeyframeAssociation), na, o);
        }
        for (uint32_t k = 0; k < n_kf; k++) {
            std::vector<uint8_t> out(mask[k].begin(), mask[k].end());
            if (!out.empty()) fwrite(out.data(), 1, out.size(), o);
        }
        fclose(o);
        return 0;
    }
    fclose(f);
    std::vector<uint8_t> verdicts;
    std::vector<mage_new_point_assoc> records;
    std::vector<std::vector<KeyframeAssociation>> gained;
    try {
        gained = LocallyAssociateNewAssociations(s, a, ki_desc, kfs, points, &verdicts, &records, (int)hdr[3] - 1);
    } catch (const Error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == MAGE_EDEVICE ? 3 : 4;
    }
    // the gained lists are the associated records, in keyframe order
    for (size_t p = 0; p < points.size(); p++) {
        size_t g = 0;
        for (uint32_t k = 0; k < n_kf; k++)
            if (verdicts[p * n_kf + k] == MAGE_NA_ASSOCIATED) {
                if (g >= gained[p].size() || gained[p][g].Keyframe != (int)k ||
                    (int32_t)gained[p][g].Keypoint != records[p * n_kf + k].keypoint)
                    return 5;
                g++;
            }
        if (g != gained[p].size()) return 5;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (!records.empty()) fwrite(records.data(), sizeof(mage_new_point_assoc), records.size(), o);
    if (!verdicts.empty()) fwrite(verdicts.data(), 1, verdicts.size(), o);
    for (uint32_t k = 0; k < n_kf; k++) {
        std::vector<uint8_t> bytes(mask[k].begin(), mask[k].end());
        if (!bytes.empty()) fwrite(bytes.data(), 1, bytes.size(), o);
    }
    fclose(o);
    return 0;
}
