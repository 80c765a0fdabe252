"""computeMarginals / solvePattern: blocks of the inverse of the pose system from the device
factorisation against the CPU oracle (unit right-hand sides through the restated CSparse path) and, for BA with the
Schur complement, against the pose block of the dense inverse of the full Hessian."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import inverse_helpers as IH
from tests.helpers import ba_case, hip_ba, manhattan_golden, oracle_ba, relerr

pytestmark = pytest.mark.gpu


def test_pose_graph_marginals_match_oracle_solves():
    from openslam_g2o_amd import capi
    g = manhattan_golden()
    J0, J1, err = O.se2_edges(g["estimates"], g["vi"], g["vj"], g["meas"])
    s = capi.HipBlockSolver(3, 2, 0)
    k = s.addEdgeSet(3, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
    s.buildStructure(g["nP"], 0, False)
    s.setEdgeData(k, J0, J1, g["omega"], err)
    s.buildSystem()
    rows = np.array([0, 5, 5, 3498, 1200, 7], np.int32)
    cols = np.array([0, 5, 7, 3498, 3000, 5], np.int32)
    M = s.computeMarginals(rows, cols)
    assert M is not None and M.shape == (6, 3, 3)
    o = O.OracleSolver(3, 2, g["nP"], 0, schur=False)
    ko = o.add_edge_set(3, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
    o.set_dims(ko, 3, 3)
    o.build_structure()
    o.set_edge_data(ko, J0, J1, g["omega"], err)
    o.build_system()
    cp, row = o.pattern("pp")
    val = o.values("Hpp")
    n = 3 * g["nP"]
    for c in np.unique(cols):
        for kk in range(3):
            e = np.zeros(n)
            e[3 * c + kk] = 1.0
            ok, x, _ = O.linear_solve_blocks(g["nP"], 3, cp, row, val, e)
            assert ok
            for i in np.flatnonzero(cols == c):
                r = rows[i]
                assert np.abs(M[i][:, kk] - x[3 * r:3 * r + 3]).max() <= 1e-9 * np.abs(x).max()
    assert np.abs(M[2] - M[5].T).max() <= 1e-9 * np.abs(M[2]).max()      # (5,7) and (7,5): the inverse is symmetric
    assert np.all(np.linalg.eigvalsh(0.5 * (M[0] + M[0].T)) > 0)         # a covariance block


def test_ba_marginals_default_is_the_inverse_of_hpp_like_the_reference():
    """BlockSolver::computeMarginals hands *_Hpp to solvePattern also under Schur (block_solver.hpp:489-493): the
    default result is the inverse of Hpp alone (dense numpy inverse of the oracle's Hpp)."""
    pr = ba_case(10, 40)
    s = hip_ba(pr)
    s.buildSystem()
    o = oracle_ba(pr)
    o.build_system()
    nP = pr["nP"]
    Hpp = o.dense_full()[:6 * nP, :6 * nP]
    Hinv = np.linalg.inv(Hpp)
    rows = np.array([0, 2, 7, 3], np.int32)
    cols = np.array([0, 5, 7, 1], np.int32)
    M = s.computeMarginals(rows, cols)
    for i in range(len(rows)):
        ref = Hinv[6 * rows[i]:6 * rows[i] + 6, 6 * cols[i]:6 * cols[i] + 6]
        assert np.abs(M[i] - ref).max() <= 1e-9 * np.abs(Hinv).max()
    s.setLambda(1.0, True)      # the reduced system is formed again by the next solve
    assert s.solve()
    xo = None
    o.set_lambda(1.0, True)
    assert o.solve()
    assert relerr(s.x(), o.x()) < 1e-7


def test_ba_pose_marginals_are_the_pose_block_of_the_full_inverse():
    pr = ba_case(10, 40)
    s = hip_ba(pr)
    s.setOption("marginals_reduced", 1)
    s.buildSystem()
    o = oracle_ba(pr)
    o.build_system()
    H = o.dense_full()
    nP = pr["nP"]
    Hinv = np.linalg.inv(H)
    rows = np.array([0, 2, 7, 3], np.int32)
    cols = np.array([0, 5, 7, 1], np.int32)
    M = s.computeMarginals(rows, cols)
    for i in range(len(rows)):
        ref = Hinv[6 * rows[i]:6 * rows[i] + 6, 6 * cols[i]:6 * cols[i] + 6]
        assert np.abs(M[i] - ref).max() <= 1e-7 * np.abs(Hinv[:6 * nP, :6 * nP]).max()
    # the solver still solves afterwards
    s.setLambda(1.0, True)
    assert s.solve()


def test_sparse_inverse_gives_every_block_of_the_pattern():
    """computeMarginals by the sparse-inverse recursion over the frontal matrices (one top-down pass for ALL requested
    blocks): every block of the reduced pattern of a BA system -- diagonal and off-diagonal, both orientations --
    against the dense inverse of Hpp, and against the column-by-column path (option marginals_recursion = 0)."""
    from openslam_g2o_amd import capi
    pr = ba_case(90, 400)
    s = hip_ba(pr)
    s.buildSystem()
    o = oracle_ba(pr)
    o.build_system()
    nP = pr["nP"]
    Hinv = np.linalg.inv(o.dense_full()[:6 * nP, :6 * nP])
    cp, ri = s.pattern(capi.HSCHUR)
    rows, cols = [], []
    for c in range(nP):
        for q in range(cp[c], cp[c + 1]):
            rows += [ri[q], c]
            cols += [c, ri[q]]
    rows, cols = np.array(rows, np.int32), np.array(cols, np.int32)
    M = s.computeMarginals(rows, cols)
    assert M is not None and M.shape == (len(rows), 6, 6)
    scale = np.abs(Hinv).max()
    for i in range(len(rows)):
        ref = Hinv[6 * rows[i]:6 * rows[i] + 6, 6 * cols[i]:6 * cols[i] + 6]
        assert np.abs(M[i] - ref).max() <= 1e-9 * scale, (rows[i], cols[i])
    s.setOption("marginals_recursion", 0)
    sel = np.arange(0, len(rows), 37)
    M0 = s.computeMarginals(rows[sel], cols[sel])
    assert np.abs(M0 - M[sel]).max() <= 1e-9 * scale
    s.setLambda(1.0, True)      # the solver still solves afterwards
    assert s.solve()


def test_sparse_inverse_with_large_fronts_matches_column_solves():
    """Pose graph with fronts of several hundred rows (scratch-slab fronts: their panels come from the whole-GPU passes):
    diagonal blocks spread over the tree and a few coupled pairs, recursion against unit right-hand sides; a pair outside
    the pattern of the factor falls back to the column path inside the same call."""
    from openslam_g2o_amd import capi
    from tests.helpers import sphere_golden
    g = sphere_golden()
    J0, J1, err = O.se3_edges(g["poses"], g["vi"], g["vj"], g["Z"])
    s = capi.HipBlockSolver(6, 3, 0)
    k = s.addEdgeSet(6, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
    s.buildStructure(g["nP"], 0, False)
    s.setEdgeData(k, J0, J1, g["omega"], err)
    s.buildSystem()
    nP = g["nP"]
    lam = 1e-3 * s.maxDiagonal()
    hcp, hri = s.pattern(capi.HPP)
    hv = s.values(capi.HPP).reshape(-1, 6, 6).copy()
    for c in range(nP):                                          # the damped matrix the factorisation sees
        assert hri[hcp[c + 1] - 1] == c
        hv[hcp[c + 1] - 1] += lam * np.eye(6)
    s.setLambda(lam, True)
    diag = np.arange(0, nP, 97, dtype=np.int32)
    hi, hj = g["hidx"][g["vi"]], g["hidx"][g["vj"]]
    keep = (hi >= 0) & (hj >= 0)
    pi, pj = hi[keep][::701].astype(np.int32), hj[keep][::701].astype(np.int32)   # measured pairs: blocks of the pattern
    rows = np.concatenate([diag, pi, [0]]).astype(np.int32)
    cols = np.concatenate([diag, pj, [nP - 1]]).astype(np.int32)
    M = s.computeMarginals(rows, cols)
    s.setOption("marginals_recursion", 0)
    M0 = s.computeMarginals(rows, cols)
    assert M is not None and M0 is not None
    assert np.abs(M - M0).max() <= 1e-9 * np.abs(M0).max()
    # ... and both against the oracle's column solves, block by block and each block to its own scale (tests/inverse_helpers.py),
    # so that the two device paths, which read the same factor, are not only compared with each other.  An oracle solve of
    # this graph takes a good part of a second, so three block columns: 0, 1 and nP - 1.  They hold a diagonal block, the
    # measured pair (0, 1) and the corner (0, nP - 1) outside the pattern, 1e-25 of the largest entry, which the sweeps produce
    # in both runs; every request with its row and column among them is compared, whole.  The oracle factorises the device's
    # own Hpp (read back before the damping, which is added here as setLambda adds it), so no assembly rounding enters.
    # Margin: no 60-digit figure exists for a system of 13 194 unknowns; what stands in for the CPU's figure is the distance
    # between two fp64 CPU inverses of this system, the oracle's column solves and NumPy's dense Cholesky with triangular
    # solves, measured once: 1.23 (0, 0), 0.50 (0, 1), 0.40 (0, nP - 1) u s.  The device gets 8 x the largest, and the
    # oracle reference its own 1 x, as legacy_margin does.
    margin = 9.0 * 1.23
    c = dict(nb=nP, bs=6, cp=hcp, ri=hri, vals=hv.reshape(-1, 36))
    block_cols = (0, 1, nP - 1)
    assert (pi[0], pj[0]) == (0, 1)
    X = IH.oracle_inverse_columns(O, c, block_cols)
    sel = [j for j in range(len(rows)) if rows[j] in block_cols and cols[j] in block_cols]
    assert sorted((int(rows[j]), int(cols[j])) for j in sel) == [(0, 0), (0, 1), (0, nP - 1)]
    for j in sel:
        ref = X[int(cols[j])][6 * rows[j]:6 * rows[j] + 6]
        sc = IH.scale_from_columns(nP, 6, hcp, hri, hv, X, rows[j], cols[j])
        for name, got in (("recursion", M[j]), ("sweeps", M0[j])):
            r = np.abs(got - ref).max() / (IH.U * sc)
            print("sphere block (%d, %d) %s: %.3g u s (margin %.3g), block %.3g, scale %.3g" % (rows[j], cols[j], name, r, margin,
                                                                                          np.abs(ref).max(), sc))
            assert r <= margin, (int(rows[j]), int(cols[j]), name, r)


@pytest.mark.parametrize("bs", [3, 6])
def test_inverse_blocks_inside_and_outside_the_pattern_on_both_seams(bs):
    """SparseCholesky::inverse_blocks behind LinearSolver::solvePattern and BlockSolver::computeMarginals: a block-tridiagonal
    system of 40 blocks.  Every diagonal and sub-diagonal block lies inside the pattern of the factor (gathered from the
    sparse inverse); the far corner (0, nb-1), its transpose and (1, nb-1) -- which shares a column with the corner -- lie
    outside it (an interior separator is eliminated last) and come from the unit-vector sweeps, one pair per distinct
    column; the corner is requested twice (two outputs from one pair of sweeps).  Against the dense inverse, to the tolerance of the tests above."""
    from openslam_g2o_amd import capi
    nb = 40
    rng = np.random.default_rng(400 + bs)
    pairs = [(c, c) for c in range(nb)] + [(c, c - 1) for c in range(1, nb)] + [(0, nb - 1), (nb - 1, 0), (1, nb - 1), (0, nb - 1)]
    rows, cols = np.array([r for r, _ in pairs], np.int32), np.array([c for _, c in pairs], np.int32)

    def check(M, Ainv):
        assert M is not None and M.shape == (len(rows), bs, bs)
        for i in range(len(rows)):
            ref = Ainv[bs * rows[i]:bs * rows[i] + bs, bs * cols[i]:bs * cols[i] + bs]
            assert np.abs(M[i] - ref).max() <= 1e-9 * np.abs(Ainv).max(), (rows[i], cols[i])

    def check_per_block(M, A_):
        """Every block to its own scale (tests/inverse_helpers.py): against NumPy's fp64 inverse through a Cholesky factor, to
        9 x what fp64 on the CPU attains on the narrow seam's matrix against the 60-digit reference (8 for the device, 1 for
        this reference; tests/golden/inverse_blocks.npz, legacy_tridiag).  1e-9 of the largest entry, above, lies 24 orders of
        magnitude over the corner block."""
        Z = IH.numpy_inverse(A_)
        r = IH.ratios(M, IH.blocks_of(Z, bs, rows, cols), IH.scales_fp64(A_, Z, bs, rows, cols))
        print("per-block ratio %.3g, margin %.3g" % (r.max(), IH.legacy_margin(bs)))
        assert r.max() <= IH.legacy_margin(bs), (int(np.argmax(r)), r.max())

    # narrow seam: diagonally dominant block-tridiagonal matrix, upper block CCS with column-major blocks
    n = nb * bs
    A = np.zeros((n, n))
    for c in range(1, nb):
        A[bs * (c - 1):bs * c, bs * c:bs * (c + 1)] = rng.normal(size=(bs, bs))
    A = A + A.T
    A += np.eye(n) * (np.abs(A).sum(axis=1).max() + 1.0)
    cp, ri, vals = [0], [], []
    for c in range(nb):
        for r in ([c - 1, c] if c else [c]):
            ri.append(r)
            vals.append(A[bs * r:bs * (r + 1), bs * c:bs * (c + 1)].T.reshape(-1))
        cp.append(len(ri))
    ls = capi.HipLinearSolver(bs, 0)
    Mn = ls.solvePattern(np.array(cp, np.int32), np.array(ri, np.int32), np.array(vals), rows, cols)
    check(Mn, np.linalg.inv(A))
    check_per_block(Mn, A)

    # wide seam: a chain of binary pose-pose edges plus one unary prior gives Hpp that pattern
    s = capi.HipBlockSolver(bs, 2 if bs == 3 else 3, 0)
    ne = nb - 1
    k = s.addEdgeSet(bs, np.arange(ne), np.arange(1, nb))
    u = s.addEdgeSet(bs, np.array([0]))
    s.buildStructure(nb, 0, False)
    eye = np.eye(bs).reshape(-1)
    s.setEdgeData(k, -eye + 0.1 * rng.normal(size=(ne, bs * bs)), eye + 0.1 * rng.normal(size=(ne, bs * bs)), np.tile(eye, (ne, 1)),
                  rng.normal(size=(ne, bs)))
    s.setEdgeData(u, eye[None], None, eye[None], np.zeros((1, bs)))
    s.buildSystem()
    hcp, hri = s.pattern(capi.HPP)
    assert list(hcp) == cp and list(hri) == ri
    hv = s.values(capi.HPP).reshape(-1, bs, bs)
    H = np.zeros((n, n))
    for c in range(nb):
        for q in range(hcp[c], hcp[c + 1]):
            H[bs * hri[q]:bs * (hri[q] + 1), bs * c:bs * (c + 1)] = hv[q].T
    Hinv = np.linalg.inv(np.triu(H) + np.triu(H, 1).T)
    s.setOption("marginals_recursion", 1)
    M1 = s.computeMarginals(rows, cols)
    s.setOption("marginals_recursion", 0)
    M0 = s.computeMarginals(rows, cols)
    check(M1, Hinv)
    check(M0, Hinv)
    Hs = np.triu(H) + np.triu(H, 1).T
    check_per_block(M1, Hs)
    check_per_block(M0, Hs)
    assert np.abs(M1 - M0).max() <= 1e-9 * np.abs(Hinv).max()
