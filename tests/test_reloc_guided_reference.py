"""CPU: the twin of the guided half of the relocalisation (mage_reloc_guided_host) against
restatements of the reference's code (tests/reloc_guided_ref.py), the oracle's pose bundle adjustment
and RadiusMatch standing between its phases, on every scene of tests/reloc_guided_cases.py; and the
scenes themselves: that each stands where it was built to stand, by the margin it was built with.
"""
import numpy as np
import pytest

from mageslam_amd import reloc
from tests import reloc_guided_cases as gc
from tests import reloc_guided_ref as gr

PROBLEMS = [(n, c) for n in gc.NAMES for c in range(len(gc.scene(n).cands))]
IDS = [f"{n}-{c}" for n, c in PROBLEMS]


@pytest.mark.parametrize("name,c", PROBLEMS, ids=IDS)
def test_phase1_is_the_reference_query_set(name, c):
    s, r = gc.scene(name), gr.run(name, c)
    g = r.g1
    if g.status & (reloc.RG_STATUS_OVER_LIMIT | reloc.RG_STATUS_BAD_ORDER) or g.verdict == reloc.RG_SKIPPED:
        assert g.verdict == reloc.RG_SKIPPED and len(g.query_ref) == 0 and int(g.result["n_assoc"]) == 0
        assert g.result["pos3_first"].tobytes() == gr.IDENT[0].tobytes() and g.result["r9_first"].tobytes() == gr.IDENT[1].tobytes()
        return
    cand = s.cands[c]
    ref, pos = gr.query_set(cand, *r.first, gr.INTR)
    assert np.array_equal(g.query_ref, ref)
    assert g.query_pos.tobytes() == pos.tobytes()
    assert g.query_kp.tobytes() == cand.kp[ref].tobytes() and g.query_desc.tobytes() == cand.desc[ref].tobytes()
    n_assoc = len(cand.order) if cand.order is not None else int((cand.map_xyzi[:, 3] > 0).sum())
    assert (int(g.result["n_assoc"]), int(g.result["n_queries"])) == (n_assoc, len(ref))
    assert g.result["pos3_first"].tobytes() == r.first[0].tobytes() and g.result["r9_first"].tobytes() == r.first[1].tobytes()


@pytest.mark.parametrize("name,c", PROBLEMS, ids=IDS)
def test_phase2_is_the_reference_gates_and_associations(name, c):
    s, r = gc.scene(name), gr.run(name, c)
    if r.g2 is None:
        return
    cand, g = s.cands[c], r.g2
    verdict, map_points = gr.after_radius_match(s.settings, cand, r.g1.query_ref, r.rm, *r.first)
    assert g.verdict == verdict
    assert int(g.result["n_radius_matches"]) == len(r.rm)
    assert g.assoc.tolist() == [list(p) for p in map_points]
    if verdict != reloc.RG_OK:
        assert len(g.ba_points3) == 0
        return
    k, t = g.assoc[:, 0], g.assoc[:, 1]
    assert g.ba_points3.tobytes() == np.ascontiguousarray(cand.map_xyzi[k, :3]).tobytes()
    assert g.ba_info.tobytes() == np.ascontiguousarray(cand.map_xyzi[k, 3]).tobytes()
    assert g.ba_uv.tobytes() == np.stack([s.kp["x"][t], s.kp["y"][t]], 1).tobytes()


@pytest.mark.parametrize("name,c", PROBLEMS, ids=IDS)
def test_phase3_is_the_reference_outlier_gate(name, c):
    s, r = gc.scene(name), gr.run(name, c)
    if r.g3 is None:
        return
    n, out = len(r.g2.assoc), int(r.second[2].sum())
    assert r.g3.verdict == gr.after_second_ba(s.settings, n, out)
    assert (int(r.g3.result["n_in_front"]), int(r.g3.result["n_outliers"])) == (n, out)
    assert r.g3.result["pos3"].tobytes() == r.second[0].tobytes() and r.g3.result["r9"].tobytes() == r.second[1].tobytes()
    # all n associations stay, the outliers included (:428-430)
    assert np.array_equal(r.g3.assoc, r.g2.assoc)


def outcomes(name):
    s = gc.scene(name)
    rows = []
    for c, cand in enumerate(s.cands):
        r = gr.run(name, c)
        rows.append((int(cand.associated_mask.sum()), int(r.pnp["result"]["verdict"]), r.final.verdict))
    return rows


@pytest.mark.parametrize("name", gc.NAMES)
@pytest.mark.parametrize("rounds", [None, 0, 1, 2])
def test_frame_choice_is_the_reference_round_robin(name, rounds):
    """The lowest candidate whose single pass succeeds is what the sequential loop over rounds and
    candidates returns, `worthwhile` flags and all; with 0 rounds nothing is tried."""
    import dataclasses

    s = gc.scene(name)
    st = s.settings if rounds is None else dataclasses.replace(s.settings, round_robin_iterations=rounds)
    results = np.array([gr.run(name, c).final.result for c in range(len(s.cands))])
    frame = reloc.choose_host(st, results)
    rows = outcomes(name)
    if any(r["status"] & (reloc.RG_STATUS_OVER_LIMIT | reloc.RG_STATUS_BAD_ORDER) for r in results):
        assert int(frame["index"]) == -1  # input the reference has no word for
        return
    index, passes = gr.routine(st, len(s.kp), rows)
    assert int(frame["index"]) == index
    if rounds is None:
        assert index == s.expect_index
    if st.round_robin_iterations == 0:
        assert index == -1 and passes == []
    if index >= 0:
        w = results[index]
        assert int(frame["n_assoc"]) == int(w["n_in_front"]) and frame["pos3"].tobytes() == w["pos3"].tobytes()
        assert frame["r9"].tobytes() == w["r9"].tobytes()
        # the reference stops at the winner: no pass behind it, in any round
        assert passes[-1][1] == index and passes[-1][0] == 0
    else:
        assert int(frame["n_assoc"]) == 0 and frame["r9"].tobytes() == gr.IDENT[1].tobytes()


@pytest.mark.parametrize("name", gc.NAMES)
def test_scene_stands_where_it_was_built(name):
    """Verdicts and status bits as built; gates passed or failed by the margin the scene was built
    with, from the oracle's own outcome; the bundle adjustments' outlier margins wide."""
    s = gc.scene(name)
    st = s.settings
    for c in range(len(s.cands)):
        r = gr.run(name, c)
        f = r.final.result
        assert (r.final.verdict, r.final.status) == (s.expect[c], s.expect_status[c]), (name, c, f)
        counts = (int(f["n_radius_matches"]), int(f["n_in_front"]), int(f["n_outliers"]))
        if name in gc.NATURAL and s.expect[c] == reloc.RG_OK:
            n = int(f["n_assoc"])
            # every association is found again; a tenth of them displaced and flagged
            assert counts == (n, n, int(round(0.1 * n)))
            assert counts[0] >= st.min_radius_match_correspondences + 5 and counts[1] >= st.min_map_points + 5
            assert (counts[1] - counts[2]) / counts[1] >= st.bundle_adjust_inliers_pct_required + 0.4
        if name in gc.NATURAL and s.expect[c] == reloc.RG_FEW_RADIUS_MATCHES:
            assert counts[0] == 0
        for which in (1, 2):
            m = gr.margins(name, c, which)
            if m is None:
                continue
            key = f"{name}/{c}/{which}"
            print(f"{key}: fragile={bool(m.fragile[0])} m_rho {m.m_rho[0]:.3g} m_ss {m.m_ss[0]:.3g} m_z {m.m_z[0]:.3g}")
            assert m.m_ss[0] >= 1e-3 and m.m_z[0] >= 1.0, key
            assert bool(m.fragile[0]) == (key in gc.POSE_FRAGILE), key
            if which == 2:
                assert np.array_equal(m.outlier, r.second[2]), key
    exact = {"gates_exact": (15, 10, 6), "short_radius": (14, 0, 0), "short_points": (15, 9, 0), "short_share": (15, 10, 7)}
    if name in exact:
        f = gr.run(name, 0).final.result
        assert (int(f["n_radius_matches"]), int(f["n_in_front"]), int(f["n_outliers"])) == exact[name]
        assert (st.min_radius_match_correspondences, st.min_map_points, st.bundle_adjust_inliers_pct_required) == (15, 10, 0.4)
    if name in gc.CRAFTED and name != "disagree" and gr.run(name, 0).pb1 is not None:
        # the first bundle adjustment stands still: the identity, bit for bit
        first = gr.run(name, 0).first
        assert first[0].tobytes() == gr.IDENT[0].tobytes() and first[1].tobytes() == gr.IDENT[1].tobytes()


def test_depth_zero_points_are_queried_and_then_removed():
    r = gr.run("depth0", 0)
    cand = gc.scene("depth0").cands[0]
    z = cand.map_xyzi[:, 2]
    assoc = cand.associated_mask
    zero, behind = np.flatnonzero(assoc & (z == 0)), np.flatnonzero(assoc & (z < 0))
    assert len(zero) == 4 and len(behind) == 4
    assert set(zero) <= set(r.g1.query_ref) and not set(behind) & set(r.g1.query_ref)
    matched = set(r.g1.query_ref[r.rm["query_idx"]])
    assert set(zero) <= matched and not set(zero) & set(r.g2.assoc[:, 0])
    # a depth of exactly zero divides by 1: the predicted position is fx X + cx
    i = int(np.flatnonzero(r.g1.query_ref == zero[0])[0])
    X = cand.map_xyzi[zero[0]]
    assert r.g1.query_pos[i].tolist() == [X[0] * gc.INTR[2] + gc.INTR[0], X[1] * gc.INTR[3] + gc.INTR[1]]


def test_projection_and_behind_filter_disagree_in_float():
    """Points in front for ProjectUndistorted (a float depth > 0) that RemoveMapPointsThatAreBehind
    removes exist, and the twin treats them as the reference would: queried, matched, removed."""
    pos3, r9, odd = gc.search_disagreement()
    assert len(odd) == 3
    s, r = gc.scene("disagree"), gr.run("disagree", 0)
    assert r.first[0].tobytes() == pos3.tobytes() and r.first[1].tobytes() == r9.tobytes()
    cand = s.cands[0]
    ks = [int(np.flatnonzero((cand.map_xyzi[:, :3] == X).all(1) & cand.associated_mask)[0]) for X in odd]
    matched = set(r.g1.query_ref[r.rm["query_idx"]])
    assert set(ks) <= matched and not set(ks) & set(r.g2.assoc[:, 0])
    assert int(r.g2.result["n_radius_matches"]) - int(r.g2.result["n_in_front"]) == 3


def test_tied_queries_are_both_dropped():
    r = gr.run("tie", 0)
    cand = gc.scene("tie").cands[0]
    # the two associations with one descriptor
    _, inv, cnt = np.unique(cand.desc[cand.associated_mask], axis=0, return_inverse=True, return_counts=True)
    twins = np.flatnonzero(cand.associated_mask)[cnt[inv.reshape(-1)] == 2]
    assert len(twins) == 2 and set(twins) <= set(r.g1.query_ref)
    assert not set(twins) & set(r.g1.query_ref[r.rm["query_idx"]])


def test_guided_search_host_backend_composes_the_phases():
    for name in ("f5_two", "gates_exact", "f3_none"):
        s = gc.scene(name)
        if s.pnp is not None:
            continue
        got = reloc.guided_search(s.settings, gr.INTR, s.cands, s.kp, s.desc, s.matches, backend="host", pose_ba=gr.oracle_ba,
                                  radius_match=gr.oracle_rm)
        for c in range(len(s.cands)):
            r = gr.run(name, c)
            assert got.results[c].tobytes() == r.final.result.tobytes(), (name, c)
            assert np.array_equal(got.assoc[c], r.final.assoc)
        assert got.index == s.expect_index
        assert len(got.associations) == (int(got.results[got.index]["n_in_front"]) if got.index >= 0 else 0)


def test_over_cap_reports_the_bit_and_keeps_the_first_queries():
    s, r = gc.scene("n65"), gr.run("n65", 0)
    g = reloc.guided_host(s.settings, True, gr.INTR, s.cands[0], s.kp, *r.first, cap=50)
    assert g.status == reloc.RG_STATUS_OVER_CAP and int(g.result["n_queries"]) == 50 and int(g.result["n_assoc"]) == 65
    assert np.array_equal(g.query_ref, r.g1.query_ref[:50]) and g.query_pos.tobytes() == r.g1.query_pos[:50].tobytes()
