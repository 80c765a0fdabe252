"""SparseCholesky::inverse_blocks block by block against a 60-digit reference (tests/golden/inverse_blocks.npz, written by
tests/golden/make_inverse_blocks.py; inputs and measure in tests/inverse_helpers.py).

Every requested block is held to its own scale: err = max |M - Z| / (u s), s the largest entry of the block of |Z| |A| |Z|.
The bound per case is 8 x what plain fp64 on the CPU attains under the same measure (the larger of NumPy's Cholesky with
triangular solves and the oracle's column solves, both stored in the fixture): another summation order and another elimination
order, not another algorithm.  Each test prints its worst ratio as a line "INVBLK {json}"; the device rows of
profiles/inverse_blocks.jsonl are those JSON objects from a run of this file with pytest -s (the rows with path "cpu" come
from the fixture generator, which keeps the device rows when it rewrites its own).

The cases and the code they reach:
  chain_flat / chain_graded  random-walk covariance (no decay, condition in the thousands), the second scaled D A D over 1e6
  chain_decay                the far corner lies ~1e-33 below the largest entry and comes from the unit-vector sweeps
  hubs                       every front below the root has a boundary of 66 / 66 / 70 rows: a second, almost empty 64-row chunk
                             in spinv_gather_y_kernel / spinv_zjb_kernel (a >= nbr in the last one)
  grid                       nested dissection: several levels, fronts with several children, scattered rel indices
  wide_panel                 pivot panels of 48 / 48 / 42 scalars: the second k0 pass of spinv_zjb_kernel.  Needs the option
                             max_sn_scalars_lds = 48: the 12 blocks of block size 7 count as a band, whose fronts are capped at 24
                             scalars by default (the 32 and 16 blocks of sizes 3 and 6 get 48 without it)
  wide_panel64               the same with both caps at 64 scalars: panels of 63 / 60 / 63 pivot scalars, the widest the planner
                             makes.  The dynamic LDS of spinv_gather_y_kernel is then (63 * 63 + 64 * 64) * 8 = 64 520 bytes and
                             that of spinv_zjj_kernel 2 * 63 * 63 * 8 = 63 504: both below 64 KiB, so with the block sizes the
                             library dispatches no plan needs the raised LDS limit that sparse_inverse asks for, and no test
                             here reaches it
The front shapes are asserted from stats(), so no case passes without the front it is there for.  stats() does not tell how
many requests a call left to the sweeps; that the far pairs of the chains do leave the recursion is shown on the wide seam,
where the far corner and its neighbour come out bit for bit as with marginals_recursion = 0 (the same sweeps) while the blocks
gathered from the sparse inverse do not."""
import json

import numpy as np
import pytest

from tests import inverse_helpers as H

pytestmark = pytest.mark.gpu

PARAMS = [(case, bs) for case in H.CASES for bs in H.BLOCK_SIZES]
WIDE_OPTIONS = {"max_sn_scalars": H.WIDE_CAP, "max_sn_scalars_lds": H.WIDE_CAP}


def _options(case):
    return WIDE_OPTIONS if case == "wide_panel" else None


def _assert_fronts(c, st):
    """The front the case is there for exists in the plan."""
    case, bs, nb = c["case"], c["bs"], c["nb"]
    if case == "hubs":
        assert st["maxFrontDim"] >= (H.HUBS[bs] + 1) * bs and st["numFronts"] > 1, st
    elif case == "grid":
        assert st["numLevels"] > 1 and st["numFronts"] > 2, st
    elif case == "wide_panel":
        # two fronts of at most 48 // bs blocks each over 2 * (48 // bs) dense blocks: both are full, and the first has a boundary
        assert st["numFronts"] == 2 and st["maxFrontDim"] == nb * bs, st
        assert (nb // 2) * bs > 32


def _report(c, path, r):
    print("INVBLK " + json.dumps(dict(case=c["case"], bs=c["bs"], path=path, device=float(r.max()), bound=c["bound"],
                                      cpu_numpy=c["cpu_numpy"], cpu_oracle=c["cpu_oracle"],
                                      device_over_cpu=float(r.max()) / max(c["cpu_numpy"], c["cpu_oracle"]))))


def _check(c, path, M, rows=None, Z=None, s=None):
    rows = c["rows"] if rows is None else rows
    Z = c["Zreq"] if Z is None else Z
    s = c["sreq"] if s is None else s
    assert M is not None and M.shape == (len(rows), c["bs"], c["bs"])
    r = H.ratios(M, Z, s)
    _report(c, path, r)
    worst = int(np.argmax(r))
    assert r.max() <= c["bound"], (path, int(rows[worst]), r.max(), c["bound"])


def _exact_properties(c, M, again, recursion=True):
    """By construction (the same slab entry or the same sweep), so a violation is an indexing bug: the repeated request and a
    permuted request list give identical blocks and, with the recursion, a transposed request of a pair on the matrix's own
    pattern -- which lies inside the pattern of the factor -- is the exact transpose (the sweeps answer the two orientations
    from different columns).  `again(rows, cols)` runs another request list on the same factor."""
    rows, cols, idx, tr = c["rows"], c["cols"], c["idx"], c["tr"]
    assert np.array_equal(M[-1], M[np.flatnonzero((idx == idx[-1]) & ~tr)[0]])                  # one request repeated
    perm = np.random.RandomState(5).permutation(len(rows))
    Mp = again(rows[perm], cols[perm])
    assert Mp is not None and np.array_equal(Mp, M[perm])
    if recursion:
        first = {}
        for i, (k, t) in enumerate(zip(idx, tr)):
            first.setdefault((int(k), bool(t)), i)
        checked = 0
        for k in np.flatnonzero(c["own"]):
            if (int(k), True) in first:
                assert np.array_equal(M[first[(int(k), True)]], M[first[(int(k), False)]].T), c["pairs"][k]
                checked += 1
        assert checked > 0


@pytest.mark.parametrize("case,bs", PARAMS)
def test_narrow_seam_blocks_match_the_reference(case, bs):
    """HipLinearSolver.solvePattern (recursion; pairs outside the pattern of the factor fall to the sweeps in the same call):
    in-pattern and off-pattern pairs interleaved in one list (the off[i] = -1 skip of the gather, the stable sort by column)."""
    from openslam_g2o_amd import capi
    c = H.load_case(case, bs)
    ls, M = H.narrow_seam(capi, c, c["rows"], c["cols"], _options(case))
    _assert_fronts(c, ls.stats())
    _check(c, "narrow", M)
    _exact_properties(c, M, lambda r, k: ls.solvePattern(c["cp"], c["ri"], c["vals"], r, k))


@pytest.mark.parametrize("case,bs", PARAMS)
def test_wide_seam_blocks_match_the_reference(case, bs):
    """HipBlockSolver.computeMarginals on the same matrix, assembled on the device from the case's generic edges (bit for bit
    the fixture's matrix, asserted before any inverse is compared), with marginals_recursion 1 and 0."""
    from openslam_g2o_amd import capi
    c = H.load_case(case, bs)
    s = H.wide_seam(capi, c, _options(case))
    s.setOption("marginals_recursion", 1)
    M1 = s.computeMarginals(c["rows"], c["cols"])
    _assert_fronts(c, s.stats())
    _check(c, "wide_recursion", M1)
    _exact_properties(c, M1, lambda r, k: s.computeMarginals(r, k))
    s.setOption("marginals_recursion", 0)
    M0 = s.computeMarginals(c["rows"], c["cols"])
    _check(c, "wide_sweeps", M0)
    _exact_properties(c, M0, lambda r, k: s.computeMarginals(r, k), recursion=False)
    if case.startswith("chain"):
        # the far corner, its transpose, its neighbour and the repeat left the recursion for the sweeps in the first run: bit for
        # bit what the sweeps alone give, which the blocks gathered from the sparse inverse are not
        nb = c["nb"]
        far = np.flatnonzero(np.abs(c["rows"] - c["cols"]) >= nb - 2)
        assert len(far) == 5 and np.array_equal(M1[far], M0[far])
        assert not np.array_equal(M1[c["rows"] == c["cols"]], M0[c["rows"] == c["cols"]])


@pytest.mark.parametrize("bs", H.BLOCK_SIZES)
def test_wide_panels_of_64_scalars(bs):
    """wide_panel64 on both seams with both supernode caps at their upper limit of 64 scalars: a dense matrix of
    2 * (64 // bs) blocks in exactly two fronts of at most 64 // bs blocks each, so both hold 63 / 60 / 63 pivot scalars and the
    first has a boundary of as many rows (the LDS these panels take is in the head of this file)."""
    from openslam_g2o_amd import capi
    c = H.load_case("wide_panel64", bs)
    opt = {"max_sn_scalars": 64, "max_sn_scalars_lds": 64}
    assert c["nb"] == 2 * (64 // bs)
    ls, M = H.narrow_seam(capi, c, c["rows"], c["cols"], opt)
    st = ls.stats()
    assert st["numFronts"] == 2 and st["maxFrontDim"] == c["nb"] * bs, st
    _check(c, "narrow", M)
    _exact_properties(c, M, lambda r, k: ls.solvePattern(c["cp"], c["ri"], c["vals"], r, k))
    s = H.wide_seam(capi, c, opt)
    M1 = s.computeMarginals(c["rows"], c["cols"])
    st = s.stats()
    assert st["numFronts"] == 2 and st["maxFrontDim"] == c["nb"] * bs, st
    _check(c, "wide_recursion", M1)


def test_not_positive_definite_returns_none_and_the_handle_stays_usable():
    from openslam_g2o_amd import capi
    c = H.load_case("chain_flat", 3)
    bad = c["vals"].copy()
    q = int(c["cp"][6]) - 1                                      # the diagonal block of block 5
    assert c["ri"][q] == 5
    bad[q] = -bad[q]
    ls = capi.HipLinearSolver(3, 0)
    assert ls.solvePattern(c["cp"], c["ri"], bad, c["rows"], c["cols"]) is None
    _check(c, "narrow_after_not_pd", ls.solvePattern(c["cp"], c["ri"], c["vals"], c["rows"], c["cols"]))

    E = dict(c["E"])
    E["UW"] = -64.0 * np.asarray(c["E"]["UW"])                    # the prior turned negative: block 0 loses its diagonal
    s = capi.HipBlockSolver(3, 2, 0)
    H.bind_edges(s, E)
    s.buildSystem()
    assert s.computeMarginals(c["rows"], c["cols"]) is None
    s2 = H.wide_seam(capi, c)
    _check(c, "wide_after_not_pd", s2.computeMarginals(c["rows"], c["cols"]))
    # the handle that reported not-PD: the right prior, the system built again
    bs, nu = 3, len(c["E"]["ui"])
    s.setEdgeData(1, np.array([(a * np.eye(bs)).reshape(-1) for a in c["E"]["ua"]]), None,
                  np.ascontiguousarray(c["E"]["UW"].reshape(nu, -1)), np.zeros((nu, bs)))
    s.buildSystem()
    _check(c, "wide_same_handle_after_not_pd", s.computeMarginals(c["rows"], c["cols"]))
