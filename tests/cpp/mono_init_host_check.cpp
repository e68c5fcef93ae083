// mono_init_host_check — mage_mono_init_two_view_host's code as a stand-alone program
// (tests/test_mono_init_sanitize.py builds it with -fsanitize=address,undefined): the twin's
// translation unit is compiled in, no library and no GPU.  Usage: mono_init_host_check IN OUT.
// IN: mage_mono_init_settings, intr4[8], n0, n1, n_matches, cap (uint32), kp0, kp1, matches.
// OUT: mage_mono_init_result, the records (n_points), the BA arrays (n_points), the trace.
#include <cstdio>
#include <string>
#include <vector>

#include "monoinit.cpp"

namespace mage {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace mage

template <class T>
static bool take(FILE* f, T* p, size_t n)
{
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}

template <class T>
static void put(FILE* f, const T* p, size_t n)
{
    if (n) fwrite(p, sizeof(T), n, f);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    mage_mono_init_settings s;
    float intr[8];
    uint32_t hdr[4];
    if (!take(in, &s, 1) || !take(in, intr, 8) || !take(in, hdr, 4)) return 2;
    const uint32_t n0 = hdr[0], n1 = hdr[1], nm = hdr[2], cap = hdr[3];
    std::vector<mage_keypoint> kp0(n0), kp1(n1);
    std::vector<mage_dmatch> mm(nm);
    if (!take(in, kp0.data(), n0) || !take(in, kp1.data(), n1) || !take(in, mm.data(), nm)) return 2;
    fclose(in);
    mage_mono_init_result r;
    std::vector<mage_stereo_point> out(cap);
    std::vector<float> bp(3 * (size_t)cap), uv(4 * (size_t)cap), info(2 * (size_t)cap);
    std::vector<uint32_t> cam(2 * (size_t)cap), pt(2 * (size_t)cap);
    std::vector<char> trace(mage_mono_init_trace_bytes(s.ransac_iterations_for_models), (char)0xA5);
    const mage_status st =
        mage_mono_init_two_view_host(&s, intr, kp0.data(), n0, kp1.data(), n1, mm.data(), nm, &r, out.data(), cap,
                                     bp.data(), uv.data(), cam.data(), pt.data(), info.data(), trace.data());
    if (st != MAGE_OK) {
        fprintf(stderr, "status %d: %s\n", (int)st, mage::g_error.c_str());
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const size_t n = r.n_points;
    put(o, &r, 1);
    put(o, out.data(), n);
    put(o, bp.data(), 3 * n);
    put(o, uv.data(), 4 * n);
    put(o, cam.data(), 2 * n);
    put(o, pt.data(), 2 * n);
    put(o, info.data(), 2 * n);
    put(o, trace.data(), trace.size());
    fclose(o);
    return 0;
}
