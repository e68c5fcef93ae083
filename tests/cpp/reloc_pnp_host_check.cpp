// reloc_pnp_host_check — mage_reloc_pnp_host's code as a stand-alone program
// (tests/test_reloc_pnp_sanitize.py builds it with -fsanitize=address,undefined): the twin's
// translation unit is compiled in, no library and no GPU.  Usage: reloc_pnp_host_check IN OUT.
// IN: mage_reloc_settings, intr4[4], n_kf, n_kp, n_matches, cap (uint32), map_xyzi, kp, matches.
// OUT: mage_reloc_pnp_result, the inlier indices (n_kept), the BA arrays (n_kept when OK), the trace.
#include <cstdio>
#include <string>
#include <vector>

#include "reloc_pnp.cpp"

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
    mage_reloc_settings s;
    float intr[4];
    uint32_t hdr[4];
    if (!take(in, &s, 1) || !take(in, intr, 4) || !take(in, hdr, 4)) return 2;
    const uint32_t n_kf = hdr[0], n_kp = hdr[1], nm = hdr[2], cap = hdr[3];
    std::vector<float> map(4 * (size_t)n_kf);
    std::vector<mage_keypoint> kp(n_kp);
    std::vector<mage_dmatch> mm(nm);
    if (!take(in, map.data(), map.size()) || !take(in, kp.data(), n_kp) || !take(in, mm.data(), nm)) return 2;
    fclose(in);
    mage_reloc_pnp_result r;
    std::vector<uint32_t> idx(cap);
    std::vector<float> p3(3 * (size_t)cap), uv(2 * (size_t)cap), info(cap);
    std::vector<char> trace(mage_reloc_pnp_trace_bytes(s.ransac_iterations), (char)0);
    const mage_status st = mage_reloc_pnp_host(&s, intr, map.data(), n_kf, kp.data(), n_kp, mm.data(), nm, &r, idx.data(),
                                               cap, p3.data(), uv.data(), info.data(), trace.data());
    if (st != MAGE_OK) {
        fprintf(stderr, "status %d: %s\n", (int)st, mage::g_error.c_str());
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const size_t n = r.n_kept, nb = r.verdict == MAGE_RP_OK ? n : 0;
    put(o, &r, 1);
    put(o, idx.data(), n);
    put(o, p3.data(), 3 * nb);
    put(o, uv.data(), 2 * nb);
    put(o, info.data(), nb);
    put(o, trace.data(), trace.size());
    fclose(o);
    return 0;
}
