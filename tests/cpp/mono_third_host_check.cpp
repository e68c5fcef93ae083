// mono_third_host_check — mage_mono_init_third_frame_host's code as a stand-alone program
// (tests/test_mono_third_reference.py builds it with -fsanitize=address,undefined): the twin's
// translation unit is compiled in, no library and no GPU.  It feeds the twin its limit cases — a bad
// index into frame 0 and into frame 1, a third frame of 0, 1, 4096 and 4097 keypoints — with every
// buffer exactly as long as its count, so that a write past a count is a sanitizer report, and checks
// the statuses.  Exit 0 and "6 cases" when all is well.
#include <cstdio>
#include <string>
#include <vector>

#include "monoinit_third.cpp"

namespace mage {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace mage

static uint32_t g_state = 12345u;
static uint32_t rnd()
{
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}

// n points in front of a camera pair one unit apart, each with its keypoint (the same descriptor in
// all three frames) among n2 third-frame keypoints; bad0 / bad1: a point whose index names no keypoint.
static int run(uint32_t n, uint32_t n2, int bad0, int bad1, uint32_t want_status, uint32_t want_matched_min)
{
    mage_mono_init_settings s{};
    s.struct_size = sizeof(s);
    s.min_third_frame_match_percentage = 0.5f;
    s.extra_frame_max_outlier_error = 8.f;
    s.extra_frame_bundle_adjustment_steps = 5;
    s.extra_frame_huber_width = 4.f;
    s.extra_frame_search_radius = 40.f;
    s.five_point_max_hamming_distance = s.extra_frame_max_hamming_distance = 30;
    s.five_point_min_hamming_difference = s.extra_frame_min_hamming_difference = 1;
    const float intr[4] = {320.f, 240.f, 500.f, 500.f};
    const float pos3[6] = {0.f, 0.f, 0.f, -1.f, 0.f, 0.f};
    const float r9[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<float> pts(3 * (size_t)n);
    std::vector<int32_t> i0(n), i1(n);
    std::vector<uint8_t> d0(32 * (size_t)n), d1(32 * (size_t)n), d2(32 * (size_t)n2);
    std::vector<mage_keypoint> kp(n2);
    for (auto& b : d2) b = (uint8_t)rnd();
    for (uint32_t t = 0; t < n2; t++) {
        kp[t] = mage_keypoint{};
        kp[t].x = (float)(rnd() % 600) + 20.f;
        kp[t].y = (float)(rnd() % 440) + 20.f;
        kp[t].octave = t % 5 == 4 ? 1 : 0;
    }
    for (uint32_t i = 0; i < n; i++) {
        const float u = 60.f + (float)(rnd() % 520), v = 60.f + (float)(rnd() % 360), z = 4.f + (float)(rnd() % 40) * 0.1f;
        pts[3 * i] = (u - 320.f) / 500.f * z + 0.5f;
        pts[3 * i + 1] = (v - 240.f) / 500.f * z;
        pts[3 * i + 2] = z;
        i0[i] = i1[i] = (int32_t)i;
        for (int b = 0; b < 32; b++) d0[32 * i + b] = d1[32 * i + b] = (uint8_t)rnd();
        if (n2) {  // the point's keypoint: the last of the frame for point 0, so that the end of the arrays is reached
            const uint32_t t = i == 0 ? n2 - 1 : (i * 37u) % n2;
            kp[t].x = u;
            kp[t].y = v;
            kp[t].octave = 0;
            for (int b = 0; b < 32; b++) d2[32 * t + b] = d0[32 * i + b];
        }
    }
    if (bad0 >= 0) i0[bad0] = (int32_t)n;
    if (bad1 >= 0) i1[bad1] = -1;
    mage_mono_init_third_result r;
    std::vector<int32_t> key(n), dist(2 * (size_t)n);
    std::vector<uint8_t> ver(n), mask(n2);
    std::vector<float> proj(2 * (size_t)n), uv(2 * (size_t)n), info(n), bp(3 * (size_t)n), buv(2 * (size_t)n), binfo(n);
    std::vector<uint32_t> opt(n), ocam(n);
    std::vector<uint8_t> outl(n, 0);
    if (n > 2) outl[1] = 1;
    const float opos[3] = {-0.5f, 0.f, 0.f};
    for (int pass = 0; pass < 2; pass++) {
        const mage_status st = mage_mono_init_third_frame_host(
            &s, intr, pos3, r9, pts.data(), n, i0.data(), i1.data(), d0.data(), n, d1.data(), n, kp.data(), d2.data(), n2, 1,
            pass ? outl.data() : nullptr, opos, r9, 0.25f, &r, key.data(), ver.data(), dist.data(), proj.data(), mask.data(),
            uv.data(), opt.data(), ocam.data(), info.data(), bp.data(), buv.data(), binfo.data());
        if (st != MAGE_OK) {
            fprintf(stderr, "status %d: %s\n", (int)st, mage::g_error.c_str());
            return 1;
        }
        if (r.status != want_status || r.n_points != n) {
            fprintf(stderr, "n2 %u: status %u, expected %u\n", n2, r.status, want_status);
            return 1;
        }
        if (want_status == 0 && r.n_matched < want_matched_min) {
            fprintf(stderr, "n2 %u: %u matched, expected at least %u\n", n2, r.n_matched, want_matched_min);
            return 1;
        }
        if (want_status == 0 && n2 > 1 && (key[0] != (int32_t)n2 - 1 || mask[n2 - 1] != 0)) {
            fprintf(stderr, "n2 %u: the last keypoint was not reached\n", n2);
            return 1;
        }
        if (pass && want_status == 0 && r.verdict != MAGE_M3_FEW_MATCHES && n > 2 && r.n_associated + 1 != r.n_matched) {
            fprintf(stderr, "n2 %u: the flagged association was not culled\n", n2);
            return 1;
        }
    }
    return 0;
}

int main()
{
    int bad = 0;
    bad |= run(40, 200, 7, -1, MAGE_M3_STATUS_BAD_INDEX, 0);
    bad |= run(40, 200, -1, 39, MAGE_M3_STATUS_BAD_INDEX, 0);
    bad |= run(40, 0, -1, -1, 0, 0);
    bad |= run(40, 1, -1, -1, 0, 1);
    bad |= run(40, 4096, -1, -1, 0, 30);
    bad |= run(40, 4097, -1, -1, MAGE_M3_STATUS_OVER_LIMIT, 0);
    if (bad) return 1;
    printf("6 cases\n");
    return 0;
}
