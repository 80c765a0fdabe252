"""The inverse-block fixture on the CPU (tests/golden/inverse_blocks.npz, tests/inverse_helpers.py): what plain fp64 attains
against the 60-digit reference under the per-block measure, and which wrong results the measure this replaces -- every block to
1e-9 of the largest entry of the whole inverse -- let through."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import inverse_helpers as H

PARAMS = [(case, bs) for case in H.CASES for bs in H.BLOCK_SIZES]


@pytest.mark.parametrize("case,bs", PARAMS)
def test_fixture_matrix_is_the_exact_assembly_of_its_edges(case, bs):
    """The stored matrix is what make_edges / assemble give (the seeds still produce the stored inputs), and the oracle's
    generic assembly of the same edges -- the recipe of the wide seam -- reproduces it bit for bit."""
    c = H.load_case(case, bs)
    E = H.make_edges(case, bs)
    for name in ("vi", "vj", "a0", "J1", "W", "ui", "ua", "UW"):
        assert np.array_equal(E[name], c["E"][name]), name
    cp, ri, vals = H.to_ccs(c["nb"], H.assemble(c["E"]))
    assert np.array_equal(cp, c["cp"]) and np.array_equal(ri, c["ri"]) and np.array_equal(vals, c["vals"])
    assert [tuple(p) for p in H.unique_pairs(case, bs, c["nb"], H.assemble(c["E"]))] == c["pairs"]

    class Shim:                                                  # the generic interface of capi.HipBlockSolver over the oracle
        def __init__(self):
            self.o = O.OracleSolver(bs, H.LANDMARK_DIM[bs], c["nb"], 0, schur=False)

        def addEdgeSet(self, d, v0, v1=None):
            k = self.o.add_edge_set(d, v0, v1)
            self.o.set_dims(k, bs, bs)
            return k

        def buildStructure(self, nP, nL, schur):
            self.o.build_structure()

        def setEdgeData(self, k, J0, J1, om, err):
            self.o.set_edge_data(k, J0, J1, om, err)

    s = Shim()
    H.bind_edges(s, c["E"])
    s.o.build_system()
    ocp, ori = s.o.pattern("pp")
    assert np.array_equal(ocp, c["cp"]) and np.array_equal(ori, c["ri"])
    assert np.array_equal(s.o.values("Hpp").reshape(-1, bs * bs), c["vals"])


@pytest.mark.parametrize("case,bs", PARAMS)
def test_fp64_on_the_cpu_against_the_reference(case, bs):
    """NumPy's Cholesky with triangular solves and the oracle's column solves, every request of the case: both stay within the
    margin the device is held to (8 x the larger of the two figures stored with the fixture; another BLAS sums in another
    order), and the reference's own rounding to fp64 is below one unit of the measure (s >= |Z| entry by entry)."""
    c = H.load_case(case, bs)
    A = H.dense_from_ccs(c["nb"], bs, c["cp"], c["ri"], c["vals"])
    rn = H.ratios(H.blocks_of(H.numpy_inverse(A), bs, c["rows"], c["cols"]), c["Zreq"], c["sreq"])
    cols = np.unique(c["cols"])
    if len(cols) > 12:                                           # the corner's column, and a spread of the others
        cols = np.unique(np.concatenate([cols[::max(1, len(cols) // 10)], [c["nb"] - 1]]))
    sel = np.flatnonzero(np.isin(c["cols"], cols))
    ro = H.ratios(H.oracle_blocks(O, c, c["rows"][sel], c["cols"][sel]), c["Zreq"][sel], c["sreq"][sel])
    print("INVBLK_CPU", case, bs, "numpy %.3g (stored %.3g) oracle %.3g (stored %.3g, all columns)" % (rn.max(), c["cpu_numpy"], ro.max(),
                                                                                                  c["cpu_oracle"]))
    assert rn.max() <= c["bound"] and ro.max() <= c["bound"]
    assert np.all(np.abs(c["Z"]).reshape(len(c["s"]), -1).max(axis=1) <= c["s"] * (1 + 1e-15))


def _old_passes_new_fails(c, M):
    zmax = np.abs(c["Z"]).max()
    assert H.old_measure_passes(M, c["Zreq"], zmax), "the old measure was expected to let this through"
    r = H.ratios(M, c["Zreq"], c["sreq"])
    assert r.max() > c["bound"], (r.max(), c["bound"])
    return r.max()


@pytest.mark.parametrize("bs", H.BLOCK_SIZES)
def test_wrong_off_pattern_blocks_pass_the_old_measure_and_fail_the_new(bs):
    """chain_decay, the blocks the unit-vector sweeps produce (far corner, its transpose, the block that shares its column, the
    repeat): returned as zero, returned transposed, taken from the neighbouring block column."""
    c = H.load_case("chain_decay", bs)
    nb = c["nb"]
    off = np.flatnonzero(np.abs(c["rows"] - c["cols"]) >= nb - 2)
    assert len(off) == 5
    M = c["Zreq"].copy()
    M[off] = 0.0
    _old_passes_new_fails(c, M)
    M = c["Zreq"].copy()
    M[off] = M[off].transpose(0, 2, 1)
    _old_passes_new_fails(c, M)
    # request (nb - 1, 0) answered with block (nb - 1, 1), the neighbouring block column (stored as the transpose of (1, nb - 1))
    M = c["Zreq"].copy()
    i = int(np.flatnonzero((c["rows"] == nb - 1) & (c["cols"] == 0))[0])
    M[i] = c["Z"][c["pairs"].index((1, nb - 1))].T
    _old_passes_new_fails(c, M)


@pytest.mark.parametrize("bs", H.BLOCK_SIZES)
def test_stale_boundary_rows_pass_the_old_measure_and_fail_the_new(bs):
    """hubs: a front whose boundary rows beyond the first 64 kept stale values, emulated by moving the entries of those rows
    and columns of the hub blocks by 1e-10 of the largest entry of the inverse."""
    c = H.load_case("hubs", bs)
    h0 = H.HUB_CHAIN * bs + 64                                   # scalar index of the 65th boundary row
    M = c["Zreq"].copy()
    eps = 1e-10 * np.abs(c["Z"]).max()
    for i, (r, k) in enumerate(zip(c["rows"], c["cols"])):
        for a in range(bs):
            for b in range(bs):
                if r * bs + a >= h0 and k * bs + b >= h0:
                    M[i, a, b] += eps
    assert np.abs(M - c["Zreq"]).max() > 0
    _old_passes_new_fails(c, M)


@pytest.mark.parametrize("bs", H.BLOCK_SIZES)
def test_relative_error_on_the_smallest_block_passes_the_old_measure_and_fails_the_new(bs):
    c = H.load_case("chain_graded", bs)
    size = np.abs(c["Zreq"]).reshape(len(c["rows"]), -1).max(axis=1)
    i = int(np.argmin(size))
    assert size[i] < 1e-12 * size.max()
    M = c["Zreq"].copy()
    M[i] *= 1.0 + 1e-9
    _old_passes_new_fails(c, M)


@pytest.mark.parametrize("bs,figure", [(3, 8.7e-34), (6, 3.3e-35)])
def test_the_corner_of_the_former_tridiagonal_matrix_lies_far_below_its_tolerance(bs, figure):
    """The matrix of test_inverse_blocks_inside_and_outside_the_pattern_on_both_seams (tests/test_gpu_marginals.py): its far
    corner block, the only block that test takes from the sweeps, relative to the largest entry of the inverse.  1e-9 of that
    entry is 24 orders of magnitude above the corner.  (The last block column by a back-substitution on the banded Cholesky
    factor: products along the chain, so the tiny entries keep their relative accuracy.)"""
    nb = 40
    rng = np.random.default_rng(400 + bs)
    n = nb * bs
    A = np.zeros((n, n))
    for c in range(1, nb):
        A[bs * (c - 1):bs * c, bs * c:bs * (c + 1)] = rng.normal(size=(bs, bs))
    A = A + A.T
    A += np.eye(n) * (np.abs(A).sum(axis=1).max() + 1.0)
    L = np.linalg.cholesky(A)
    zmax = np.abs(np.linalg.inv(A)).max()
    corner = 0.0
    for k in range(bs):
        y = np.zeros(n)
        for i in range(n - bs + k, n):                           # L y = e: zero above the unit entry
            y[i] = ((1.0 if i == n - bs + k else 0.0) - L[i, n - bs:i] @ y[n - bs:i]) / L[i, i]
        z = np.zeros(n)
        for i in range(n - 1, -1, -1):
            hi = min(n, i + 2 * bs)
            z[i] = (y[i] - L[i + 1:hi, i] @ z[i + 1:hi]) / L[i, i]
        corner = max(corner, np.abs(z[:bs]).max())
    assert abs(corner / zmax / figure - 1.0) < 0.06, corner / zmax
    assert corner < 1e-20 * 1e-9 * zmax
