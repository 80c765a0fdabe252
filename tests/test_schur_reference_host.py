"""tests/golden/schur_blocks.npz (written by tests/golden/make_schur_blocks.py) without a GPU: the fixture loads, the inputs the
helper rebuilds are the ones the references were computed for, the CPU evaluations stay inside the bounds their recorded figures
give, every census and coverage condition holds, and the per-block measure sees what the global max-norm does not."""
import numpy as np
import pytest

from tests import schur_helpers as H
from tests.helpers import relerr

NAMES = sorted(H.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_rebuilt_inputs_are_the_fixtures(name):
    k = H.load_case(name)
    c, a = k["c"], k["a"]
    assert H.input_hash(c) == k["input_sha"]
    assert H.assembled_hash(a) == k["assembled_sha"]
    outs = H.OUTPUTS + (("xp_solved", "xl_solved") if c["nP"] <= H.FULL_SOLVE_MAX_POSES else ())
    assert set(k["ref"]) == set(outs)
    shapes = dict(Dinv=(c["nL"], c["l"], c["l"]), Hschur=(len(a["hs"][1]), c["p"], c["p"]), bschur=(c["nP"], c["p"]),
                  xl=(c["nL"], c["l"]), xp_solved=(c["nP"], c["p"]), xl_solved=(c["nL"], c["l"]))
    for o in outs:
        assert k["ref"][o].shape == shapes[o] and k["scale"][o].shape == shapes[o][:1]
        assert np.all(np.isfinite(k["ref"][o])) and np.all(k["scale"][o] > 0)
        assert np.all(np.abs(k["ref"][o]).reshape(shapes[o][0], -1).max(axis=1) <= k["scale"][o] * (1 + 1e-15))
        assert 0 < k["bound"][o] <= H.MARGIN * 64.0, (o, k["bound"][o])


@pytest.mark.parametrize("name", NAMES)
def test_cpu_evaluations_stay_inside_their_bounds(name):
    """The oracle and NumPy, evaluated now, against the stored references: at most the bound their recorded figures give (another
    compiler may round the oracle's sums differently; the recorded figure itself is printed)."""
    from oracle import oracle as O
    k = H.load_case(name)
    c, a = k["c"], k["a"]
    cen = H.census_of(c, a)
    with_solve = c["nP"] <= H.FULL_SOLVE_MAX_POSES
    for which, ev in (("oracle", H.oracle_evaluation(O, c, a, with_solve)), ("numpy", H.numpy_evaluation(c, a, cen, with_solve))):
        for o in k["ref"]:
            f = H.figures(ev[o], k["ref"][o], k["scale"][o])
            print("SCHURBLK_CPU", name, which, o, "%.3g (stored %.3g / %.3g, bound %.3g)" % ((f.max(),) + k["cpu"][o] + (k["bound"][o],)))
            assert f.max() <= k["bound"][o], (which, o, int(np.argmax(f)), f.max())
            if which == "numpy":                                 # NumPy's sums are the recorded ones up to the BLAS build: a factor of 2
                assert f.max() <= 2.0 * k["cpu"][o][1] and k["cpu"][o][1] <= 2.0 * f.max(), (o, f.max(), k["cpu"][o][1])
            else:                                                # the oracle's depend on the C compiler's contraction: the same factor
                assert f.max() <= 2.0 * max(k["cpu"][o]) , (o, f.max(), k["cpu"][o])


@pytest.mark.parametrize("name", NAMES)
def test_census_conditions(name):
    k = H.load_case(name)
    cen = H.census_of(k["c"], k["a"])
    H.assert_census(name, k["c"], cen)
    # several partial blocks per destination: the slots rd_ptr / rd_slot hand to the reduction
    assert cen["n_td"] > len(k["a"]["hs"][1])


def test_coverage_counts():
    f = H.fixture()
    g = H.load_case("graded_20")
    seen = H.coverage(g["c"], g["a"])["seen"]
    assert seen[1] >= 40 and seen[2] >= 40 and seen[5] >= 40, seen
    assert float(f["graded_20/cond_landmark"]) > 1e7 > float(f["graded_0/cond_landmark"])
    assert [g["c"]["lam"], H.load_case("graded_10")["c"]["lam"], H.load_case("graded_0")["c"]["lam"]] == [2.0 ** -20, 2.0 ** -10, 1.0]
    x = H.load_case("fixed")
    cov = H.coverage(x["c"], x["a"])
    assert cov["fixed_obs"] >= 30 and cov["unseen_landmarks"] == 1 and cov["bare_poses"] >= 1, cov
    assert int(f["contrast/blocks_below_1e10"]) >= 20
    assert set(H.CASES[n][2] for n in NAMES) == {1, 4, 8}
    assert set(H.CASES[n][:2] for n in NAMES) == {(6, 3), (3, 2), (7, 3), (3, 3)}
    assert sum(H.load_case(n)["c"]["nP"] <= H.FULL_SOLVE_MAX_POSES for n in NAMES) >= 8


def test_the_block_measure_sees_what_the_global_norm_misses():
    """One block of Hschur between two poses of the 2^-20-scaled third, zeroed in a copy of the reference: the global max-norm
    stays below the 1e-12 the suite used to hold Hschur to, the block's own figure is far over its bound."""
    k = H.load_case("contrast")
    ref, s = k["ref"]["Hschur"], k["scale"]["Hschur"]
    scaled = k["c"]["pose_scale"] < 1.0
    ri = k["a"]["hs"][1]
    col = np.repeat(np.arange(k["c"]["nP"]), np.diff(k["a"]["hs"][0]))
    big = np.abs(ref).reshape(len(ref), -1).max(axis=1)
    cand = np.flatnonzero(scaled[ri] & scaled[col] & (big > 0) & (big < 1e-12 * big.max()))
    assert len(cand) > 0
    q = int(cand[np.argmax(big[cand])])
    planted = ref.copy()
    planted[q] = 0.0
    assert 0.0 < relerr(planted, ref) < 1e-12
    f = H.figures(planted, ref, s)
    assert int(np.argmax(f)) == q and f[q] > 1e3 * k["bound"]["Hschur"], (q, f[q], k["bound"]["Hschur"])
    assert np.all(np.delete(f, q) == 0.0)


@pytest.mark.parametrize("name", H.FUSED_CASES)
def test_fused_cases(name):
    """The fused BA cases: the rebuilt estimates are the fixture's, the census gives the lane group the GPU test expects, and both
    CPU evaluations (the oracle's fp64 producers and Schur loop; NumPy in the tiles' order) reproduce their recorded figures
    within a factor of 2 and so stay inside the bounds."""
    from oracle import oracle as O
    k = H.load_fused_case(name)
    c, st = k["c"], k["st"]
    assert H.fused_input_hash(c) == k["input_sha"]
    assert c["nP"] == (38 if name == "ba_chain" else 10) and c["nL"] == (400 if name == "ba_chain" else 40)
    assert (len(c["classes"]) > 1) == (name == "ba_prodc")
    for i, lam in enumerate(H.FUSED_LAMBDAS):
        eo, en, cen = H.fused_cpu_evaluations(O, c, st, lam)
        assert cen["G"] == (8 if name == "ba_chain" else 4)
        for o in H.OUTPUTS:
            key = "%s@%d" % (o, i)
            assert np.all(k["scale"][key] > 0) and np.all(np.isfinite(k["ref"][key]))
            for which, ev, rec in (("oracle", eo, k["cpu"][key][0]), ("numpy", en, k["cpu"][key][1])):
                f = H.figures(ev[o], k["ref"][key], k["scale"][key]).max()
                print("SCHURBLK_CPU", name, which, key, "%.3g (stored %.3g, bound %.3g)" % (f, rec, k["bound"][key]))
                assert f <= k["bound"][key] and f <= 2.0 * max(k["cpu"][key]), (which, key, f, rec)


def test_copied_constants_are_the_librarys():
    """The tile budget of the census and the partial-block limit behind the reach of schur_rhs_kernel are copies: held to the
    definitions in the sources, so a change there fails here instead of leaving the reach assertions describing something else."""
    import os
    import re
    src = os.path.join(H.ROOT, "openslam_g2o_amd", "csrc")
    with open(os.path.join(src, "block_solver.h")) as f:
        m = re.search(r"size_t\s+schur_tile_bytes\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", f.read())
    assert m and int(m.group(1)) * int(m.group(2)) == H.TILE_BYTES
    with open(os.path.join(src, "block_solver.hip")) as f:
        m = re.search(r"constexpr\s+double\s+kFuseReduceMaxPartials\s*=\s*([0-9.]+)\s*;", f.read())
    assert m and float(m.group(1)) == H.FUSE_REDUCE_MAX_PARTIALS
    assert H.plan_module().census.__defaults__[2] == H.TILE_BYTES      # the probe's own budget
