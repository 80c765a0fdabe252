"""tests/golden/assembly_blocks.npz (written by tests/golden/make_assembly_blocks.py) without a GPU: the inputs the helper rebuilds
are the ones the references were computed for, the case table reaches every row of both dispatch tables of
csrc/block_solver.hip, every census condition holds, the exact cases are exact at 60 digits, no robust edge sits near its
switch, and both CPU evaluations give the recorded figures again."""
import numpy as np
import pytest

from tests import assembly_helpers as H

BLOCK_CASES = [n for n in H.NAMES if H.make_case(n)["kind"] in ("blocks", "single")]
GROUP_ROWS = {(2, 3), (2, 6), (3, 6), (6, 6), (7, 7), (1, 6)}


@pytest.mark.parametrize("name", H.NAMES)
def test_rebuilt_inputs_are_the_fixtures(name):
    k = H.load_case(name)
    assert H.input_hash(k["c"]) == k["input_sha"]
    for o in H.outputs_of(k["c"]):
        assert len(k["ref"][o]) == len(k["scale"][o])
        assert np.all(np.isfinite(k["scale"][o])) and np.all(k["scale"][o] >= 0)
        assert 0 < k["bound"][o] < np.inf, (o, k["bound"][o])                 # no output held by figure has a bound of 0
        for r, s in zip(k["ref"][o], k["scale"][o]):
            if o not in ("w_diag", "w_off"):
                assert np.max(np.abs(r)) <= s * (1 + 1e-15), (o, r, s)        # a value is at most its operand sum


def test_the_case_table_reaches_every_row_of_both_dispatch_tables():
    vert, off, thresholds = H.parse_tables()
    assert len(vert) == len(set(vert)) == 13 and len(off) == len(set(off)) == 14
    assert thresholds == (2.0, 1, 16.0, 4, 8)
    for avg, G in ((0.0, 1), (2.0, 1), (2.0 + 1e-9, 4), (16.0, 4), (16.0 + 1e-9, 8), (1e6, 8)):   # the helper's copy of pick_group
        lo, g1, hi, g4, g8 = thresholds
        assert H.pick_group(avg) == (g1 if avg <= lo else (g4 if avg <= hi else g8)) == G
    V, O = set(), set()
    for name in H.NAMES:
        c = H.make_case(name)
        v, o = H.rows_reached(c, H.structure(c))
        V |= v
        O |= o
    assert V | set(H.UNREACHED_ROWS["vertex"]) == set(vert) and not V & set(H.UNREACHED_ROWS["vertex"])
    assert O | set(H.UNREACHED_ROWS["offdiag"]) == set(off) and not O & set(H.UNREACHED_ROWS["offdiag"])


@pytest.mark.parametrize("G", (1, 4, 8))
def test_census_of_the_lane_group_cases(G):
    rows = set()
    for p in (3, 6, 7):
        c = H.make_case("g%d_p%d" % (G, p))
        st = H.structure(c)
        cen = H.census(c, st)
        assert set(g for g, _, _ in cen["groups"]) == {G}, cen["groups"]
        rows |= set((d, dv) for _, d, dv in cen["groups"])
        for q in st["per"]:
            lens = [len(w) for w in q["vp"]]
            assert lens[:6] == [0, 1, G - 1, G, G + 1, 3 * G + 1] and lens == list(c["want"])
        assert (c["nP"] * G) % H.K_THREADS != 0                  # the last workgroup ends in idle lane groups
        assert cen["tr_pp"] > 0 and cen["n_op"] > 0
    assert rows >= GROUP_ROWS


def test_census_of_destinations_sets_and_parts():
    for name in ("fam_6_3", "fam_3_2", "fam_7_3", "fam_3_3"):
        c = H.make_case(name)
        st = H.structure(c)
        cen = H.census(c, st)
        assert {1, 2, 5} <= cen["dst"] and cen["tr_pp"] > 0 and cen["tr_pl"] > 0 and cen["plain_pl"] > 0, (name, cen)
        assert any(s["n"] == 0 for s in c["sets"]) and sum(s["n"] > 0 for s in c["sets"]) >= 3
        assert any((s["v0"] < 0).any() or (s["v1"] is not None and (s["v1"] < 0).any()) for s in c["sets"])      # fixed vertices
        lists_p = [sum(len(q["vp"][v]) for q in st["per"]) for v in range(c["nP"])]
        lists_l = [sum(len(q["vl"][v]) for q in st["per"]) for v in range(c["nL"])]
        assert lists_p[-1] == 0 and lists_l[-1] == 0             # a vertex with no contributor
        # two and three sets write the same off-diagonal blocks
        assert max(sum(blk in q["ol"] for q in st["per"]) for blk in range(len(st["pl"][1]))) >= 2
    c = H.make_case("fam_6_3")
    st = H.structure(c)
    assert max(sum(blk in q["op"] for q in st["per"]) for blk in range(len(st["pp"][1]))) >= 3
    assert sorted(set(s["d"] for s in c["sets"])) == [1, 2, 3, 6] and sum(s["v1"] is None for s in c["sets"]) == 2
    assert H.census(H.make_case("fam_3_2"), H.structure(H.make_case("fam_3_2")))["n_ol"] > H.K_THREADS
    n = H.make_case("nary_6_3")
    assert [s["parts"] for s in n["sets"]] == [0, H.PART_NO_VERTEX0 | H.PART_NO_VERTEX1 | H.PART_NO_CHI2, H.PART_NO_VERTEX0 | H.PART_NO_CHI2]
    single = H.make_case("robust_single")
    assert H.census(single, H.structure(single))["dst"] == {1} and set(single["sets"][0]["kinds"]) == set(range(6))
    for name in ("robust_set", "robust_edge"):
        c = H.make_case(name)
        kinds = set(int(H._kernel_of(s, k)[0]) for s in c["sets"] for k in range(s["n"]))
        assert kinds >= {1, 2, 3, 4, 5}, (name, kinds)
    assert tuple(sorted(H.CHI2_DIMS)) == (1, 2, 3, 6, 7) and H.CHI2_SIZES == (1, 255, 256, 257, 513)


@pytest.mark.parametrize("name", H.NAMES)
def test_no_robust_edge_near_its_switch(name):
    """e2 at 60 digits: a relative 1e-6 from delta^2 (DCS: from delta) or exactly on it -- 100 % of the edges, none excluded."""
    n_rob, n_on, n_bad = H.threshold_census(H.make_case(name))
    assert n_bad == 0
    assert [n_rob, n_on, n_bad] == list(H.fixture()[name + "/threshold"])
    if name == "robust_edge":
        assert n_on == 9
        c = H.make_case(name)
        for s in c["sets"]:                                      # on the switch: identity information, dyadic errors
            sel = s["on_switch"]
            assert np.array_equal(s["om"][sel], np.tile(np.eye(s["d"]).reshape(-1), (sel.sum(), 1))) and set(s["err"][sel].reshape(-1)) == {0.0, 2.0}


def test_extreme_ratios_reach_the_smooth_kernels():
    import mpmath as mp
    c = H.make_case("robust_set")
    for s in c["sets"]:
        if s["kind"] not in (2, 3, 5):
            continue
        d = s["d"]
        e2 = np.array([float(s["err"][k] @ s["om"][k].reshape(d, d) @ s["err"][k]) for k in range(s["n"])])
        ratio = e2 / (s["delta"] if s["kind"] == 5 else s["delta"] ** 2)
        assert ratio.max() > 0.9e8 and ratio.min() < 1.1e-8, (s["kind"], ratio.min(), ratio.max())
    assert mp.mp.dps >= 15


def test_the_exact_cases_are_exact_at_60_digits():
    import mpmath as mp
    from tests import reference_mp  # noqa: F401
    assert mp.mp.dps == 60
    c = H.make_case("chi2_exact")
    s = c["sets"][0]
    assert s["n"] == H.EXACT_N > H.MAX_PARTIALS * H.K_THREADS and s["kind"] == 0 and s["kinds"] is None and np.all(s["om"] == 1.0)
    K = np.rint(s["err"][:, 0] * 8).astype(np.int64)
    assert np.array_equal(K / 8.0, s["err"][:, 0])
    total = int((K * K).sum())
    assert total < 2 ** 53                                       # every partial sum of the terms k^2 / 64 is an integer / 64 below 2^53
    assert mp.fsum(mp.mpf(float(v)) ** 2 for v in s["err"][::997, 0]) * 64 == int((K[::997] ** 2).sum())
    assert mp.mpf(float(H.fixture()["chi2_exact/exact_chi2"])) * 64 == total
    assert H._grid_sum(s["err"][:, 0] ** 2, 0.0) == total / 64.0
    for size in H.SCALE_SIZES:                                   # computeScale: b exact (dyadic data, identity information)
        c = H.make_case("scale_n%d" % size)
        assert c["nP"] * c["p"] + c["nL"] * c["l"] == size
        ev = H.evaluate(c, H.structure(c), "np")
        b = np.concatenate([ev["bp"].reshape(-1), ev["bl"].reshape(-1)])
        assert np.array_equal(b, c["b_exact"]) and np.array_equal(b * 8, np.rint(b * 8)) and np.abs(b).max() < 2 ** 20
        opposite = (c["lam"] * c["x"] * b < 0).sum()
        assert size // 3 - 4 <= opposite <= size // 3 + 1, (size, opposite)


@pytest.mark.parametrize("name", [n for n in H.NAMES if n != "chi2_exact"])
def test_cpu_figures_are_the_recorded_ones(name):
    from oracle import oracle as O
    k = H.load_case(name)
    c, st = k["c"], k["st"]
    got = {}
    if c["kind"] == "chi2":
        got["chi2"] = ([H.oracle_solver(O, c).chi2()], [H.evaluate(c, st, "np", False)["chi2"]])
    elif c["kind"] == "scale":
        o = H.oracle_solver(O, c)
        o.view("x", o.n)[:] = c["x"]
        got["scale"] = ([o.compute_scale(c["lam"])], [H.scale_numpy(c, c["b_exact"])])
    else:
        e = H.evaluate(c, st, "np")
        ov, nv = H.oracle_evaluation(O, c, st), H.numpy_outputs(c, st, e)
        for o in ("Hpp", "Hpl", "Hll", "b", "chi2"):
            if o in k["ref"]:
                got[o] = (ov[o], nv[o])
        if c["kind"] == "single":
            f = H.fixture()
            wo, wn = (H.weights_from_blocks(c, st, v["Hpp"], f[name + "/single_idx"], f[name + "/single_M"]) for v in (ov, nv))
            got["w_diag"], got["w_off"] = (np.concatenate([wo[0], wo[2]]), np.concatenate([wn[0], wn[2]])), (wo[1], wn[1])
        if name in H.HX_CASES:
            for i, lam in enumerate(c["lams"]):
                ov["_o"].build_system()
                ov["_o"].set_lambda_split(lam[0], lam[1], False)
                got["Hx%d" % i] = (H.split_b(c, ov["_o"].multiply_full(c["x"])), H.split_b(c, H.multiply(c, st, e, c["x"], lam)))
    assert set(got) == set(H.outputs_of(c))
    for o, pair in got.items():
        figs = tuple(float(H.figures(g, k["ref"][o], k["scale"][o]).max()) for g in pair)
        print("ASMBLK_CPU", name, o, figs, k["cpu"][o])
        assert figs == k["cpu"][o], (o, figs, k["cpu"][o])
