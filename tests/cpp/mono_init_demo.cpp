// Drives mage::hot::MonoMapInit::InitializeWithFrames (include/mage/mage.hpp) on a frame pair read from a file:
//   u32 n0, n1, n_matches, device_plus_one, has_descriptors, min_feature_matches; float intr[8]; per frame:
//   keypoints, [n x 32 descriptor bytes]; n_matches matches (used when has_descriptors is 0).
// Writes the mage_mono_init_result, u32 n_matches, n_points, the matches the stage ran on, and when the
// verdict is OK frame 1's pose (3 + 9 floats), the points and the bundle arrays (points, observations,
// cameras, map points, information).  Exit 3: no usable device; 5: std::out_of_range; 6: over a limit.
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
    float intr[8];
    if (!rd(f, hdr, 6) || !rd(f, intr, 8)) return 2;
    MonoFrame frame[2];
    std::vector<KeyPoint> kp[2];
    std::vector<uint8_t> desc[2];
    for (int k = 0; k < 2; k++) {
        kp[k].resize(hdr[k]);
        desc[k].resize(hdr[4] ? 32 * (size_t)hdr[k] : 0);
        if (!rd(f, kp[k].data(), kp[k].size()) || !rd(f, desc[k].data(), desc[k].size())) return 2;
        std::copy(intr + 4 * k, intr + 4 * k + 4, frame[k].Intrinsics.begin());
        frame[k].KeyPoints = &kp[k];
        frame[k].Descriptors = hdr[4] ? desc[k].data() : nullptr;
    }
    std::vector<DMatch> matches(hdr[2]);
    if (!rd(f, matches.data(), matches.size())) return 2;
    fclose(f);
    MonoMapInitializationSettings settings;
    settings.MinFeatureMatches = hdr[5];
    MonoMapInit init(settings, (int)hdr[3] - 1);
    std::optional<MonoInitializationData> d;
    try {
        d = init.InitializeWithFrames(hdr[4] ? nullptr : &matches, frame[0], frame[1]);
    } catch (const Error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == MAGE_EDEVICE ? 3 : (e.status == MAGE_EUNSUPPORTED ? 6 : 4);
    } catch (const std::out_of_range& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&init.LastResult(), sizeof(mage_mono_init_result), 1, o);
    const uint32_t n[2] = {(uint32_t)init.LastMatches().size(), d ? (uint32_t)d->MapPoints.size() : 0u};
    fwrite(n, 4, 2, o);
    wr(o, init.LastMatches());
    if (d) {
        fwrite(d->Frame1Position.data(), 4, 3, o);
        fwrite(d->Frame1Rotation.data(), 4, 9, o);
        wr(o, d->MapPoints);
        wr(o, d->BundlePoints);
        wr(o, d->BundleObservations);
        wr(o, d->BundleCameras);
        wr(o, d->BundleMapPoints);
        wr(o, d->BundleInformation);
    }
    fclose(o);
    return 0;
}
