// track_host_check — the tracker's shared host code run without a GPU (tests/test_track_host.py):
// track_math.hpp's arithmetic, track_window.hpp's build_window / apply_window and track_bufs.hpp's
// block table, driven by flat binary files.  Usage: track_host_check math|window|block IN OUT.
#include <cstdio>
#include <string>
#include <vector>

#include "track_window.hpp"

using namespace mage::track;

namespace {

struct In {
    FILE* f;
    template <class T>
    T one()
    {
        T v{};
        if (fread(&v, sizeof(T), 1, f) != 1) throw std::string("short input");
        return v;
    }
    template <class T>
    std::vector<T> many(size_t n)
    {
        std::vector<T> v(n);
        if (n && fread(v.data(), sizeof(T), n, f) != n) throw std::string("short input");
        return v;
    }
};

struct Out {
    FILE* f;
    template <class T>
    void one(const T& v)
    {
        fwrite(&v, sizeof(T), 1, f);
    }
    template <class T>
    void many(const std::vector<T>& v)
    {
        if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
    }
};

TrackConst read_const(In& in)
{
    TrackConst c{};
    c.s = in.one<mage_track_settings>();
    for (int i = 0; i < 4; i++) c.K[i] = in.one<double>();
    c.fx = (float)c.K[0], c.fy = (float)c.K[1], c.cx = (float)c.K[2], c.cy = (float)c.K[3];
    c.plane_z = in.one<double>();
    octave_factors(c.s.scale_factor, c.s.num_levels, c.fmax, c.fmin, &c.log2s);
    return c;
}

void run_math(In& in, Out& out)
{
    const TrackConst c = read_const(in);
    const Pose kf = load_pose(in.many<double>(12).data()), q = load_pose(in.many<double>(12).data());
    const Pose prev = load_pose(in.many<double>(12).data()), prev2 = load_pose(in.many<double>(12).data());
    const uint32_t fid = in.one<uint32_t>(), n = in.one<uint32_t>();
    const std::vector<mage_keypoint> kp = in.many<mage_keypoint>(n);
    const uint32_t m = in.one<uint32_t>();
    const std::vector<float> cpts = in.many<float>(3 * m);
    const std::vector<int32_t> coct = in.many<int32_t>(m);
    const std::vector<float> cmvd = in.many<float>(3 * m), cdmin = in.many<float>(m), cdmax = in.many<float>(m);

    // a keyframe of the keypoints at pose kf (tracking.make_keyframe), then the attributes of the
    // given points under the same pose (tracking.point_attributes)
    float R32[9], t32[3], C[3];
    pose_f32(kf.R, kf.t, R32, t32);
    world_position(R32, t32, C);
    std::vector<float> pts(3 * n), mvd(3 * n), dmin(n), dmax(n), amvd(3 * m), admin(m), admax(m);
    for (uint32_t i = 0; i < n; i++) {
        backproject_to_plane(kp[i].x, kp[i].y, kf, c.K, c.plane_z, fid, i, c.s.map_point_depth_noise, &pts[3 * i]);
        point_attributes(&pts[3 * i], C, kp[i].octave, c.fmin, c.fmax, &mvd[3 * i], dmin[i], dmax[i]);
    }
    for (uint32_t i = 0; i < m; i++)
        point_attributes(&cpts[3 * i], C, coct[i], c.fmin, c.fmax, &amvd[3 * i], admin[i], admax[i]);
    out.many(pts), out.many(mvd), out.many(dmin), out.many(dmax), out.many(amvd), out.many(admin), out.many(admax);

    // the given points under pose q: tracking.project and tracking.local_map_queries
    std::vector<uint8_t> front(m), ok(m);
    std::vector<float> uv(2 * m), pxy(2 * m);
    std::vector<int32_t> oct(m);
    pose_f32(q.R, q.t, R32, t32);
    float Cq[3];
    world_position(R32, t32, Cq);
    for (uint32_t i = 0; i < m; i++) {
        front[i] = project_front(R32, t32, c.fx, c.fy, c.cx, c.cy, &cpts[3 * i], uv[2 * i], uv[2 * i + 1]);
        ok[i] = local_map_candidate(R32, t32, Cq, c.fx, c.fy, c.cx, c.cy, c.s, c.log2s, &cpts[3 * i], &cmvd[3 * i], cdmin[i],
                                    cdmax[i], pxy[2 * i], pxy[2 * i + 1], oct[i]);
    }
    out.many(front), out.many(uv), out.many(ok), out.many(pxy), out.many(oct);

    std::vector<double> pred(12);
    store_pose(pred.data(), predict(prev, prev2));
    out.many(pred);
    for (uint32_t k = 0; k < 6; k++) out.one(refinement_confidence(k));
}

void run_window(In& in, Out& out)
{
    const TrackConst c = read_const(in);
    HostRing R;
    R.nk = in.one<uint32_t>(), R.cap = in.one<uint32_t>(), R.acap = in.one<uint32_t>();
    R.ctl.kf_first = in.one<uint32_t>(), R.ctl.kf_count = in.one<uint32_t>();
    for (uint32_t k = 0; k < R.nk; k++) R.ctl.kf_n[k] = in.one<uint32_t>();
    for (uint32_t k = 0; k < R.nk; k++) R.ctl.kf_id[k] = in.one<uint32_t>();
    for (uint32_t k = 0; k < R.nk; k++) R.ctl.kf_an[k] = in.one<uint32_t>();
    const size_t np = (size_t)R.nk * R.cap, na = (size_t)R.nk * R.acap;
    std::vector<mage_keypoint> kp = in.many<mage_keypoint>(np);
    std::vector<float> pts = in.many<float>(3 * np), mvd = in.many<float>(3 * np), dmin = in.many<float>(np),
                       dmax = in.many<float>(np);
    std::vector<double> pose = in.many<double>(12 * R.nk);
    std::vector<uint32_t> ref = in.many<uint32_t>(np);
    std::vector<uint8_t> own = in.many<uint8_t>(np);
    std::vector<int4> assoc = in.many<int4>(na);
    std::vector<uint8_t> aalive = in.many<uint8_t>(na);
    R.v.kf_kp = kp.data(), R.v.kf_pts = pts.data(), R.v.kf_mvd = mvd.data(), R.v.kf_dmin = dmin.data();
    R.v.kf_dmax = dmax.data(), R.v.kf_pose = pose.data(), R.v.kf_ref = ref.data(), R.v.kf_own = own.data();
    R.v.kf_assoc = assoc.data(), R.v.kf_aalive = aalive.data();
    LocalBA L;
    L.have_theta = in.one<uint32_t>() != 0;
    L.theta = in.one<uint32_t>();

    const BaWindow w = build_window(R, c, L);
    const uint32_t E = (uint32_t)w.kept.size(), P = (uint32_t)w.keys.size();
    out.one<uint32_t>(w.valid), out.one(w.nr), out.one(w.theta), out.one(w.steps), out.one(w.huber), out.one(E), out.one(P);
    if (!w.valid) return;
    out.many(w.cam), out.many(w.pt), out.many(w.uv), out.many(w.info), out.many(w.fixed), out.many(w.keys);
    for (const BaObs& ob : w.kept) out.one(ob.kind), out.one(ob.cam), out.one(ob.src);
    out.many(w.pos3), out.many(w.r9), out.many(w.intr), out.many(w.xyz);

    // the write-back, when the input goes on with a solution
    const uint32_t nout = in.one<uint32_t>();
    if (nout == 0xFFFFFFFFu) return;
    const std::vector<uint32_t> outl = in.many<uint32_t>(nout);
    const std::vector<float> pos_o = in.many<float>(3 * w.nr), r9_o = in.many<float>(9 * w.nr), xyz_o = in.many<float>(3 * P);
    std::vector<uint8_t> changed(R.nk, 0);
    apply_window(R, c, w, outl.data(), nout, pos_o.data(), r9_o.data(), xyz_o.data(), changed);
    out.many(pts), out.many(mvd), out.many(dmin), out.many(dmax), out.many(pose), out.many(ref), out.many(own);
    out.many(aalive), out.many(changed);
}

// Records what the table binds: (offset, bytes, part) per entry.
struct Recorder {
    BlockBinder b;
    std::vector<uint64_t> rows;
    template <class T>
    void operator()(T*& member, size_t count, BlockBinder::Part part = BlockBinder::REST)
    {
        const size_t at = b.bytes;
        b(member, count, part);
        rows.push_back(reinterpret_cast<uintptr_t>(member) - b.base);
        rows.push_back(at);
        rows.push_back(count * sizeof(T));
        rows.push_back(part);
    }
};

void run_block(In& in, Out& out)
{
    TrackConst c{};
    c.cap = in.one<uint32_t>();
    const uint32_t lmk = in.one<uint32_t>(), frames = in.one<uint32_t>();
    const uint64_t lm_bytes = in.one<uint64_t>();
    c.nk = lmk > 1 ? lmk : 1;
    c.qcap = lmk > 0 ? c.nk * c.cap : 0;
    c.acap = c.cap + c.qcap;
    TrackBlock k{};
    Recorder r;
    track_block_visit(k, c, frames, lm_bytes, r);
    out.one<uint64_t>(r.b.bytes), out.one<uint64_t>(r.b.ring_begin), out.one<uint64_t>(r.b.moved_begin);
    out.one<uint64_t>(r.b.ring_end), out.one<uint64_t>(r.b.ring_contiguous), out.one<uint64_t>(r.rows.size() / 4);
    out.many(r.rows);
    // the device views (any base) and the mirror views bound to a host base: relative offsets
    std::vector<uint8_t> mirror(r.b.ring_end - r.b.ring_begin + 1);
    const HostRing R = host_ring(c, frames, lm_bytes, mirror.data(), Ctl{});
    track_block(k, c, frames, lm_bytes, reinterpret_cast<void*>(uintptr_t(1) << 40));
    const void* dev[] = {k.b.kf_kp, k.b.kf_desc, k.b.kf_pts, k.b.kf_mvd, k.b.kf_dmin, k.b.kf_dmax, k.b.kf_pose, k.b.kf_ref,
                         k.b.kf_own, k.b.kf_assoc, k.b.kf_aalive};
    const void* host[] = {R.v.kf_kp, R.v.kf_desc, R.v.kf_pts, R.v.kf_mvd, R.v.kf_dmin, R.v.kf_dmax, R.v.kf_pose, R.v.kf_ref,
                          R.v.kf_own, R.v.kf_assoc, R.v.kf_aalive};
    for (int i = 0; i < 11; i++) {
        out.one<int64_t>((const char*)dev[i] - (const char*)k.b.kf_kp);
        out.one<int64_t>((const uint8_t*)host[i] - mirror.data());
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    In in{fopen(argv[2], "rb")};
    Out out{fopen(argv[3], "wb")};
    if (!in.f || !out.f) return 2;
    const std::string mode = argv[1];
    try {
        if (mode == "math")
            run_math(in, out);
        else if (mode == "window")
            run_window(in, out);
        else if (mode == "block")
            run_block(in, out);
        else
            return 2;
    } catch (const std::string& e) {
        fprintf(stderr, "%s\n", e.c_str());
        return 1;
    }
    fclose(out.f);
    return 0;
}
