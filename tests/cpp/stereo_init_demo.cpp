// Drives mage::hot::TriangulateStereoPair (include/mage/mage.hpp) on a stereo pair read from a file:
//   u32 n0, n1, n_matches, device_plus_one, has_descriptors, whole_call; i32 crop[4]; per frame: pose (3 + 9 + 4
//   floats), keypoints, [n x 32 descriptor bytes]; n_matches matches (used when has_descriptors is 0).
// With a sixth header word set the file continues with frame0ToFrame1 (16 floats) and the camera
// {fx, fy, cx, cy, u32 width, height} of both frames, and mage::hot::StereoMapInit::Initialize runs
// instead: writes u32 code, n_points, then frame 1's pose (3 + 9 floats) and the points when OK.
// Otherwise writes u32 n_matches, n_points, the mask bytes, the matches, the verdict bytes, the points and the
// bundle arrays (points, observations, cameras, map points, information).  Exit 3: no usable device.
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
    std::array<int32_t, 4> crop;
    if (!rd(f, hdr, 6) || !rd(f, crop.data(), 4)) return 2;
    KeyframeView frame[2];
    std::vector<KeyPoint> kp[2];
    std::vector<uint8_t> desc[2];
    for (int k = 0; k < 2; k++) {
        kp[k].resize(hdr[k]);
        desc[k].resize(hdr[4] ? 32 * (size_t)hdr[k] : 0);
        if (!rd(f, frame[k].Position.data(), 3) || !rd(f, frame[k].Rotation.data(), 9) ||
            !rd(f, frame[k].Intrinsics.data(), 4) || !rd(f, kp[k].data(), kp[k].size()) ||
            !rd(f, desc[k].data(), desc[k].size()))
            return 2;
        frame[k].KeyPoints = &kp[k];
    }
    std::vector<DMatch> matches(hdr[2]);
    if (!rd(f, matches.data(), matches.size())) return 2;
    if (hdr[5]) {
        std::array<float, 16> m;
        mage_camera_config cam{};
        if (!rd(f, m.data(), 16) || !rd(f, &cam.fx, 4) || !rd(f, &cam.width, 2)) return 2;
        fclose(f);
        StereoMapInit init(StereoMapInitializationSettings{}, (int)hdr[3] - 1);
        std::optional<InitializationData> d;
        try {
            d = init.Initialize({cam, &kp[0], desc[0].data()}, {cam, &kp[1], desc[1].data()}, m);
        } catch (const Error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return e.status == MAGE_EDEVICE ? 3 : 4;
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        const uint32_t n[2] = {(uint32_t)init.LastResult().code, d ? (uint32_t)d->MapPoints.size() : 0u};
        fwrite(n, 4, 2, o);
        if (d) {
            fwrite(d->Frame1Position.data(), 4, 3, o);
            fwrite(d->Frame1Rotation.data(), 4, 9, o);
            wr(o, d->MapPoints);
        }
        fclose(o);
        return 0;
    }
    fclose(f);
    StereoTriangulation r;
    try {
        r = TriangulateStereoPair(StereoMapInitializationSettings{}, frame[0], desc[0].data(), frame[1], desc[1].data(),
                                  crop, hdr[4] ? nullptr : &matches, (int)hdr[3] - 1);
    } catch (const Error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == MAGE_EDEVICE ? 3 : 4;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const uint32_t n[2] = {(uint32_t)r.Matches.size(), (uint32_t)r.Points.size()};
    fwrite(n, 4, 2, o);
    wr(o, std::vector<uint8_t>(r.Frame0Mask.begin(), r.Frame0Mask.end()));
    wr(o, r.Matches);
    wr(o, r.Verdicts);
    wr(o, r.Points);
    wr(o, r.BundlePoints);
    wr(o, r.BundleObservations);
    wr(o, r.BundleCameras);
    wr(o, r.BundleMapPoints);
    wr(o, r.BundleInformation);
    fclose(o);
    return 0;
}
