"""GPU parity of the matchers' paths that the single-call tests of test_gpu_match.py do not reach:
every body of match_kernel through Match, the batched device entry points beyond pair 0 (different
pitches, empty pairs, a shared B set, truncating capacities, counts above the limits, both status
bits of the radius matcher, its split and fused launches), and signed-zero / negative coordinates in
the band index.  Everything is bit-exact against the CPU oracle on DMatch bytes and counts; the
oracle's Match is pinned by test_match_reference.py.  Output buffers are prefilled with 0xA5 and every
byte past a pair's results must still hold it."""
import functools

import numpy as np
import pytest

from match_cases import CANARY, RADIUS_SETTINGS, SETTINGS, assert_regions, dm_bytes, match_sets, radius_sets
from mageslam_amd import matcher
from mageslam_amd._lib import DM_DTYPE, KP_DTYPE

pytestmark = pytest.mark.gpu

EMPTY = np.zeros(0, DM_DTYPE)


@functools.lru_cache(maxsize=None)
def sets_of(na, nb):
    """match_sets(na, nb) at the shape's own seed, generated once and shared (read-only)."""
    A, B = match_sets(na, nb, na * 7 + nb)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def ref_match(na, nb, md, mdiff):
    """oracle.match of sets_of(na, nb), computed once and shared between the tests (read-only)."""
    from oracle import oracle as O

    A, B = sets_of(na, nb)
    o = O.match(A, B, max_distance=md, min_difference=mdiff)
    o.setflags(write=False)
    return o


# ------------------------- A: every body of match_kernel through Match ---------------------------

KEYS16 = [(33, 97), (64, 2048), (1025, 700)]
KEYS32_RESIDENT = [(100, 2049), (300, 2560)]
STREAMING = [(100, 2561), (513, 3000), (1025, 4096), (4096, 2561)]


@pytest.mark.parametrize("na,nb", KEYS16 + KEYS32_RESIDENT + STREAMING)
def test_match_every_kernel_body(gpu, oracle, na, nb):
    """nb <= 2048: Keys16 (minDiff 0) and the fp4 kernel (minDiff >= 1); 2048 < nb <= 2560: Keys32
    resident; above: Keys32 streaming; maxDist >= 128: PADMASK, resident and streaming.  The
    settings make the packed distance arithmetic decide (matches at distances up to 127 and 256),
    unlike (0, 0), where only exact duplicates match."""
    A, B = sets_of(na, nb)
    for md, mdiff in SETTINGS:
        o = ref_match(na, nb, md, mdiff)
        assert len(o) > 0
        g = matcher.Match(A, B, maxHammingDist=md, minHammingDifference=mdiff)
        assert len(g) == len(o) and np.array_equal(dm_bytes(g), dm_bytes(o)), (na, nb, md, mdiff, len(g), len(o))


# ------------------------- B: match_batch_device beyond pair 0 -----------------------------------


def run_match_batch(As, Bs, counts, a_rows, b_rows, md, mdiff, cap=None):
    """One mage_hamming_match_batch_device call: pair p's A at row p * a_rows, B at row p * b_rows
    (b_rows == 0: every pair reads Bs[0]); the rows of a pair's pitch above the given arrays are
    random bytes.  -> (out bytes (pairs, cap * 16), counts (pairs,))."""
    import torch

    pairs = len(counts)
    cap = a_rows if cap is None else cap
    rng = np.random.default_rng(99)
    A = rng.integers(0, 256, (pairs, a_rows, 32), dtype=np.uint8)
    B = rng.integers(0, 256, (pairs if b_rows else 1, max(b_rows, len(Bs[0])), 32), dtype=np.uint8)
    for p in range(pairs):
        A[p, : len(As[p])] = As[p]
    for p in range(len(B)):
        B[p, : len(Bs[p])] = Bs[p]
    tA, tB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    na = torch.tensor([c[0] for c in counts], dtype=torch.int32, device="cuda")
    nb = torch.tensor([c[1] for c in counts], dtype=torch.int32, device="cuda")
    out = torch.full((pairs, cap * 16), CANARY, dtype=torch.uint8, device="cuda")
    nout = torch.full((pairs,), -1, dtype=torch.int32, device="cuda")
    matcher.match_batch_device(tA, a_rows * 32, na, tB, b_rows * 32, nb, pairs, md, mdiff, out, cap, nout)
    torch.cuda.synchronize()
    return out.cpu().numpy(), nout.cpu().numpy()


B1_COUNTS = [(100, 2561), (64, 2048), (300, 2560), (0, 500), (500, 0), (1025, 4096), (33, 97)]


def test_match_batch_all_bodies_one_launch(gpu, oracle):
    """Seven pairs under pitches of 4096 rows, so every pair goes to match_kernel and picks its body
    from its own counts: all four bodies in one launch at pair > 0, Keys16 with minDiff >= 1 (which
    the host call gives to the fp4 kernel), and pairs with a zero count on either side whose rows
    hold matchable descriptors."""
    A5, B5 = sets_of(500, 500)
    As = [sets_of(*c)[0] if min(c) else A5 for c in B1_COUNTS]
    Bs = [sets_of(*c)[1] if min(c) else B5 for c in B1_COUNTS]
    assert len(ref_match(500, 500, 30, 1)) > 0
    for md, mdiff in SETTINGS:
        exp = [ref_match(na, nb, md, mdiff) if min(na, nb) else EMPTY for na, nb in B1_COUNTS]
        assert all(len(e) > 0 for e, c in zip(exp, B1_COUNTS) if min(c))
        out, n = run_match_batch(As, Bs, B1_COUNTS, 4096, 4096, md, mdiff)
        assert_regions(out, n, 4096, exp, (md, mdiff))


B2_COUNTS = [(4096, 2048), (2049, 100), (1, 1), (0, 0), (700, 2047)]


def test_match_batch_fp4_unequal_pitches(gpu, oracle):
    """A B pitch of 2048 rows sends the batch to the fp4 kernel; a_pitch != b_pitch, the largest
    and the smallest pair, an empty pair in the middle.  At (0, 1) only the (1, 1) pair matches."""
    shapes = [c if min(c) else (500, 500) for c in B2_COUNTS]
    As = [sets_of(*s)[0] for s in shapes]
    Bs = [sets_of(*s)[1] for s in shapes]
    for md, mdiff in ((30, 1), (127, 2), (0, 1)):
        exp = [ref_match(na, nb, md, mdiff) if min(na, nb) else EMPTY for na, nb in B2_COUNTS]
        assert sum(len(e) for e in exp) > 0 and (md == 0 or all(len(e) > 0 for e, c in zip(exp, B2_COUNTS) if min(c)))
        out, n = run_match_batch(As, Bs, B2_COUNTS, 4096, 2048, md, mdiff)
        assert_regions(out, n, 4096, exp, (md, mdiff))


def test_match_batch_shared_b(gpu, oracle):
    """With b_pitch == 0 every pair matches its own A set against the one B set (and the call takes
    match_kernel whatever the settings)."""
    rng = np.random.default_rng(31)
    B = sets_of(600, 900)[1]
    As = []
    for na in (600, 1025, 33):
        flip = rng.integers(0, 256, (na, 32), dtype=np.uint8) & rng.integers(0, 256, (na, 32), dtype=np.uint8) \
            & rng.integers(0, 256, (na, 32), dtype=np.uint8)
        As.append(B[rng.integers(0, 900, na)] ^ flip)
    counts = [(len(a), 900) for a in As]
    for md, mdiff in ((30, 1), (127, 0), (200, 0)):
        exp = [oracle.match(a, B, max_distance=md, min_difference=mdiff) for a in As]
        assert all(len(e) > 0 for e in exp)
        out, n = run_match_batch(As, [B], counts, 1040, 0, md, mdiff)
        assert_regions(out, n, 1040, exp, (md, mdiff))


@pytest.mark.parametrize("rows,md,mdiff", [(2048, 30, 1), (4096, 30, 0), (4096, 200, 0)])  # fp4 kernel, match_kernel
def test_match_batch_capacity_truncates(gpu, oracle, rows, md, mdiff):
    """With cap = half of pair 0's matches, d_n[0] is the full count, pair 0's region holds exactly
    the first cap matches, pair 1 (fewer matches than cap) is complete, nothing else is written."""
    shapes = [(1025, 700), (33, 97)]
    exp = [ref_match(na, nb, md, mdiff) for na, nb in shapes]
    cap = len(exp[0]) // 2
    assert 0 < len(exp[1]) <= cap
    out, n = run_match_batch([sets_of(*s)[0] for s in shapes], [sets_of(*s)[1] for s in shapes], shapes, rows, rows,
                             md, mdiff, cap=cap)
    assert_regions(out, n, cap, exp, (rows, md, mdiff))


def test_match_batch_count_above_limit(gpu, oracle):
    """A pair with n_a = 4097 (one above the kernel's limit) under pitches of 4104 rows reports 0
    and writes nothing; the pairs on both sides of it are exact."""
    shapes = [(100, 2561), (4097, 500), (33, 97)]
    As = [match_sets(*s, 5)[0] if s[0] > 4096 else sets_of(*s)[0] for s in shapes]
    Bs = [match_sets(*s, 5)[1] if s[0] > 4096 else sets_of(*s)[1] for s in shapes]
    for md, mdiff in ((30, 1), (200, 0)):
        exp = [ref_match(100, 2561, md, mdiff), EMPTY, ref_match(33, 97, md, mdiff)]
        out, n = run_match_batch(As, Bs, shapes, 4104, 4104, md, mdiff)
        assert_regions(out, n, 4104, exp, (md, mdiff))


# ------------------------- C: radius_match_batch_device ------------------------------------------

Q_PITCH, T_PITCH = 1100, 4100


class RadiusBatch:
    """Device buffers of one batched RadiusMatch layout: pair p's queries at entry p * q_pitch, its
    targets at p * t_pitch.  sets[p] = (qk, qd, tk, td, qpos); counts[p] = (nq, nt) may be below the
    set sizes (a zero count over matchable data) or above them (the limit cases).  The entries of a
    pitch above a set repeat the set, so a read past a count finds plausible keypoints."""

    def __init__(self, sets, counts, q_pitch=Q_PITCH, t_pitch=T_PITCH):
        import torch

        self.pairs = pairs = len(sets)
        self.q_pitch, self.t_pitch = q_pitch, t_pitch
        qk = np.zeros((pairs, q_pitch), KP_DTYPE)
        tk = np.zeros((pairs, t_pitch), KP_DTYPE)
        qd = np.zeros((pairs, q_pitch, 32), np.uint8)
        td = np.zeros((pairs, t_pitch, 32), np.uint8)
        qp = np.zeros((pairs, q_pitch, 2), np.float32)
        for p, (k, d, t, e, pos) in enumerate(sets):
            qk[p], qd[p], qp[p] = np.resize(k, q_pitch), np.resize(d, (q_pitch, 32)), np.resize(pos, (q_pitch, 2))
            tk[p], td[p] = np.resize(t, t_pitch), np.resize(e, (t_pitch, 32))
        dev = "cuda"
        self.qk = torch.from_numpy(qk.view(np.uint8).reshape(pairs, -1)).to(dev)
        self.tk = torch.from_numpy(tk.view(np.uint8).reshape(pairs, -1)).to(dev)
        self.qd, self.td, self.qp = (torch.from_numpy(x).to(dev) for x in (qd, td, qp))
        self.nq = torch.tensor([c[0] for c in counts], dtype=torch.int32, device=dev)
        self.nt = torch.tensor([c[1] for c in counts], dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(pairs * q_pitch, dtype=torch.int32, device=dev)

    def run(self, setting, with_pos, cap=None, pairs=None):
        """-> (out bytes (pairs, cap * 16), counts, status) of the first `pairs` pairs; cap defaults to
        the query pitch."""
        import torch

        pairs = self.pairs if pairs is None else pairs
        cap = self.q_pitch if cap is None else cap
        r, md, mdiff = setting
        out = torch.full((pairs, cap * 16), CANARY, dtype=torch.uint8, device="cuda")
        nout = torch.full((pairs,), -1, dtype=torch.int32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        matcher.radius_match_batch_device(self.qk, self.qp if with_pos else None, self.qd, self.q_pitch, self.nq,
                                          self.tk, self.td, self.t_pitch, self.nt, pairs, r, md, mdiff, self.scratch, out, cap, nout,
                                          status)
        torch.cuda.synchronize()
        return out.cpu().numpy(), nout.cpu().numpy(), int(status.item())


def ref_radius(oracle, s, count, setting, with_pos):
    """The oracle's RadiusMatch over the first count = (nq, nt) entries of set s."""
    qk, qd, tk, td, qpos = s
    nq, nt = count
    if nq == 0 or nt == 0:
        return EMPTY
    r, md, mdiff = setting
    return oracle.radius_match(qk[:nq], qd[:nq], tk[:nt], td[:nt], r, qpos=qpos[:nq] if with_pos else None,
                               max_distance=md, min_difference=mdiff)


C1_COUNTS = [(70, 300), (0, 300), (300, 2048), (257, 2049), (1000, 4096), (1100, 0)]


def test_radius_batch_pitches_overrides_empty_pairs(gpu, oracle):
    """Six pairs (split launch) with q_pitch != t_pitch, position overrides given and not, staged (nt <= 2048)
    and unstaged target sets at pair > 0, pairs with no queries or no targets over matchable data,
    y shifted negative on every other pair."""
    sets = []
    for p, (nq, nt) in enumerate(C1_COUNTS):
        gen = (max(nq, 70), max(nt, 37))  # the empty sides still hold data: only the count says "empty"
        sets.append(radius_sets(*gen, np.random.default_rng(102 + p), shift_y=-20.0 if p & 1 else 0.0))
    batch = RadiusBatch(sets, C1_COUNTS)
    for setting in RADIUS_SETTINGS:
        exp = {}
        for with_pos in (True, False):
            exp[with_pos] = [ref_radius(oracle, s, c, setting, with_pos) for s, c in zip(sets, C1_COUNTS)]
            assert all(len(e) > 0 for e, c in zip(exp[with_pos], C1_COUNTS) if min(c))
            out, n, status = batch.run(setting, with_pos)
            assert status == 0
            assert_regions(out, n, Q_PITCH, exp[with_pos], (setting, with_pos))
        # the overrides matter: a kernel that ignored them (or read another pair's) would differ
        assert all(len(a) != len(b) or not np.array_equal(dm_bytes(a), dm_bytes(b))
                   for a, b, c in zip(exp[True], exp[False], C1_COUNTS) if min(c))


def test_radius_batch_split_and_fused(gpu, oracle):
    """127 pairs (several workgroups per pair plus the post-pass kernel) and 128 pairs (one fused
    workgroup per pair) over the same buffers: 5 distinct small pairs in rotation, one without
    queries."""
    shapes = [(70, 300), (300, 300), (0, 300), (257, 299), (129, 300)]
    seeds = [202, 210, 220, 230, 240]  # on the oracle alone: every non-empty pair matches at every setting
    distinct = [radius_sets(max(nq, 70), nt, np.random.default_rng(seed), shift_y=-20.0 if i & 1 else 0.0)
                for i, ((nq, nt), seed) in enumerate(zip(shapes, seeds))]
    batch = RadiusBatch([distinct[p % 5] for p in range(128)], [shapes[p % 5] for p in range(128)])
    for setting in RADIUS_SETTINGS:
        for with_pos in (True, False):
            ref = [ref_radius(oracle, s, c, setting, with_pos) for s, c in zip(distinct, shapes)]
            assert all(len(e) > 0 for e, c in zip(ref, shapes) if min(c)), [len(e) for e in ref]
            for pairs in (127, 128):
                out, n, status = batch.run(setting, with_pos, pairs=pairs)
                assert status == 0
                assert_regions(out, n, Q_PITCH, [ref[p % 5] for p in range(pairs)], (setting, with_pos, pairs))


def test_radius_batch_status_bits(gpu, oracle):
    """A pair above a limit sets one status bit, reports 0 and writes nothing, and its neighbours are
    exact, with position overrides and without, at every setting: nt = 4097 (above the 4096 targets
    of the band index) sets bit 0; nq = 1101 above its pitch of 1100 sets bit 1; so does nt = 301
    above a target pitch of 300."""
    sets = [radius_sets(70, 300, np.random.default_rng(202)), radius_sets(1100, 4097, np.random.default_rng(301)),
            radius_sets(257, 2049, np.random.default_rng(302), shift_y=-20.0)]
    small = [sets[0], radius_sets(70, 301, np.random.default_rng(303)),
             radius_sets(129, 300, np.random.default_rng(240), shift_y=-20.0)]
    cases = [(sets, [(70, 300), (300, 4097), (257, 2049)], T_PITCH, 1),
             (sets, [(70, 300), (1101, 300), (257, 2049)], T_PITCH, 2),
             (small, [(70, 300), (70, 301), (129, 300)], 300, 2)]
    for data, counts, t_pitch, bit in cases:
        batch = RadiusBatch(data, counts, t_pitch=t_pitch)
        for setting in RADIUS_SETTINGS:
            for with_pos in (True, False):
                exp = [ref_radius(oracle, data[0], counts[0], setting, with_pos), EMPTY,
                       ref_radius(oracle, data[2], counts[2], setting, with_pos)]
                assert len(exp[0]) > 0 and len(exp[2]) > 0
                out, n, status = batch.run(setting, with_pos)
                assert status == bit, (counts[1], setting, with_pos)
                assert_regions(out, n, Q_PITCH, exp, (counts[1], setting, with_pos))


@pytest.mark.parametrize("pairs", [2, 128])  # the post-pass kernel and the fused post-pass
def test_radius_batch_capacity_truncates(gpu, oracle, pairs):
    """With cap = half of pair 0's matches, d_n[0] is the full count, the first cap matches are
    written, the other pairs (fewer matches than cap) are complete and nothing else is written;
    with position overrides and without, at every setting."""
    shapes = [(1000, 4096), (70, 300)]
    sets = [radius_sets(*shapes[0], np.random.default_rng(400)), radius_sets(*shapes[1], np.random.default_rng(202))]
    which = [0, 1] + [1] * (pairs - 2)
    batch = RadiusBatch([sets[w] for w in which], [shapes[w] for w in which])
    for setting in RADIUS_SETTINGS:
        for with_pos in (True, False):
            ref = [ref_radius(oracle, s, c, setting, with_pos) for s, c in zip(sets, shapes)]
            cap = len(ref[0]) // 2
            assert 0 < len(ref[1]) <= cap
            out, n, status = batch.run(setting, with_pos, cap=cap)
            assert status == 0
            assert_regions(out, n, cap, [ref[w] for w in which], (pairs, setting, with_pos))


# ------------------------- D: signed zero and negative coordinates in the band index -------------


def local_map_both(oracle, qk, qd, tk, td, radius, md, mdiff):
    qp = np.stack([qk["x"], qk["y"]], 1)
    qo = qk["octave"].astype(np.int32)
    mask = np.ones(len(tk), bool)
    g, gm = matcher.LocalMapMatch(qp, qo, qd, tk, td, mask, radius, md, mdiff)
    o, om = oracle.local_map_match(qp, qo, qd, None, tk, td, mask.astype(np.uint8), radius, md, mdiff)
    return g, gm, o, om.astype(bool)


def test_signed_zero_band_edge(gpu, oracle):
    """Targets (5, -0.0) and (5, +0.0), one query at (5, 3) with radius 3: py - r == +0.0 and the f32
    box test -0.0 >= +0.0 holds, so the target at -0.0 (descriptor distance 0) is a candidate and
    wins over the one at +0.0 (distance 8)."""
    tk = np.zeros(2, KP_DTYPE)
    tk["x"] = 5
    tk["y"] = [-0.0, 0.0]
    assert np.signbit(tk["y"][0]) and not np.signbit(tk["y"][1])
    td = np.zeros((2, 32), np.uint8)
    td[1, 0] = 0xFF
    qk = np.zeros(1, KP_DTYPE)
    qk["x"], qk["y"] = 5, 3
    qd = np.zeros((1, 32), np.uint8)
    o = oracle.radius_match(qk, qd, tk, td, 3.0, max_distance=30, min_difference=1)
    assert len(o) == 1 and (o["query_idx"][0], o["train_idx"][0], o["distance"][0]) == (0, 0, 0.0)
    g = matcher.RadiusMatch(qk, qd, tk, td, 3.0, maxHammingDist=30, minHammingDifference=1)
    assert np.array_equal(dm_bytes(g), dm_bytes(o)), (g, o)
    g, gm, o, om = local_map_both(oracle, qk, qd, tk, td, 3.0, 30, 1)
    assert list(o) == [0]
    assert np.array_equal(g, o) and np.array_equal(gm, om), (g, o)


@pytest.mark.parametrize("radius", [0.0, 1.0, 2.0])
def test_signed_zero_band_sets(gpu, oracle, radius):
    """200 targets with y in {-2, -1, -0.0, +0.0, 1, 2} and queries whose band edges py - r and
    py + r land exactly on +0.0 (py = r, py = -r), on -0.0 (py = -0.0, r = 0) and on the other
    values: both zeros belong to every band that reaches 0, whichever sign the edge carries."""
    rng = np.random.default_rng(17)
    ys = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], np.float32)
    nt, nq = 200, 96
    tk = np.zeros(nt, KP_DTYPE)
    tk["x"] = rng.integers(0, 6, nt).astype(np.float32)
    tk["y"] = ys[rng.integers(0, 6, nt)]
    tk["octave"] = rng.integers(0, 2, nt)
    pal = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    td = pal[rng.integers(0, 6, nt)] ^ (rng.random((nt, 32)) < 0.02).astype(np.uint8)
    qk = np.zeros(nq, KP_DTYPE)
    qk["x"] = rng.integers(0, 6, nq).astype(np.float32)
    qy = np.array([radius, -radius, -0.0, 0.0, 1.0, -2.0], np.float32)
    qk["y"] = qy[np.arange(nq) % 6]
    qk["octave"] = rng.integers(0, 2, nq)
    qd = pal[rng.integers(0, 6, nq)]
    assert np.signbit(tk["y"][tk["y"] == 0]).any() and not np.signbit(tk["y"][tk["y"] == 0]).all()
    for md, mdiff in ((256, 0), (30, 1), (8, 2)):
        o = oracle.radius_match(qk, qd, tk, td, radius, max_distance=md, min_difference=mdiff)
        g = matcher.RadiusMatch(qk, qd, tk, td, radius, maxHammingDist=md, minHammingDifference=mdiff)
        assert len(o) > 0 and (tk["y"][o["train_idx"]] == 0).any()  # matches at y = +-0.0 are in the result
        assert len(g) == len(o) and np.array_equal(dm_bytes(g), dm_bytes(o)), (radius, md, mdiff, len(g), len(o))
        g, gm, o, om = local_map_both(oracle, qk, qd, tk, td, radius, md, mdiff)
        assert (tk["y"][o[o >= 0]] == 0).any()
        assert np.array_equal(g, o) and np.array_equal(gm, om), (radius, md, mdiff)
