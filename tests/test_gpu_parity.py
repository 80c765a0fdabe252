"""GPU parity tests (run with -m gpu on the MI355X box): the HIP path, called through the
C ABI, against the CPU oracle on the same seeded inputs and against the committed golden
vectors from the reference's CSparse path.

Tolerances (fp64).  Assembly / Schur intermediates: 1e-12 relative (only summation order
and FMA contraction differ).  dx: the stated bar is 1e-8 relative; the forward
error of ANY backward-stable solve is ~cond*eps, so the bound used is
    max(1e-8, 4 * cond(reduced system) * eps)
with the condition number of the damped reduced system measured per case (dx_tolerance below:
dense eigenvalues of the oracle's Hschur) -- 1e-8 wherever cond <= 1e7, the conditioning-scaled
bound for the LM-damped systems with tiny lambda (cond up to ~1e11).  The conditioning-independent
residual |H x - b|_inf / |b|_inf is held at 1e-11.  chi2: 1e-9 relative (north_star bar: 1e-6).
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import GOLD, ba_case, hip_ba, manhattan_golden, oracle_ba, relerr

pytestmark = pytest.mark.gpu

TOL_MAT = 1e-12
from tests.helpers import TOL_DX, dx_tolerance  # noqa: E402,F401
TOL_RES = 1e-11
TOL_CHI = 1e-9


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _cmp_system(s, o, capi, huber=0.0):
    for which, name in ((capi.HPP, "Hpp"), (capi.HPL, "Hpl"), (capi.HLL, "Hll")):
        assert relerr(s.values(which), o.values(name)) < TOL_MAT, name
    assert relerr(s.b(), o.b()) < TOL_MAT
    assert abs(s.chi2() - o.chi2()) <= TOL_CHI * o.chi2()


@pytest.mark.parametrize("P,L", [(8, 40), (40, 400), (300, 3000)])
def test_ba_build_schur_solve(P, L):
    capi = _capi()
    pr = ba_case(P, L)
    s, o = hip_ba(pr), oracle_ba(pr)
    s.buildSystem()
    o.build_system()
    # structure
    for w, n in ((capi.HPP, "pp"), (capi.HPL, "pl"), (capi.HSCHUR, "hs")):
        cp, ri = s.pattern(w)
        ocp, ori = o.pattern(n)
        assert np.array_equal(cp, ocp) and np.array_equal(ri, ori)
    _cmp_system(s, o, capi)
    lam = 1e-5 * o.max_diagonal()
    assert abs(s.maxDiagonal() - o.max_diagonal()) <= 1e-13 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < TOL_MAT
    assert relerr(s.values(capi.DINV), o.values("Dinv")) < TOL_MAT
    x, xo = s.x(), o.x()
    tol, cond = dx_tolerance(o)
    assert relerr(x, xo) < tol, (relerr(x, xo), tol, cond)
    assert relerr(s.b(), o.b()) < TOL_MAT                      # solve() must not modify b (block_solver.hpp:435-436)
    r = s.multiplyHessian(x) - s.b()                            # damped system: H already contains lambda
    assert np.abs(r).max() <= TOL_RES * np.abs(s.b()).max()
    assert abs(s.computeScale(lam) - o.compute_scale(lam)) <= 1e-6 * abs(o.compute_scale(lam))
    s.restoreDiagonal()
    o.restore_diagonal()
    assert relerr(s.values(capi.HPP), o.values("Hpp")) < TOL_MAT
    assert relerr(s.values(capi.HLL), o.values("Hll")) < TOL_MAT


def test_ba_golden_vectors():
    capi = _capi()
    gold = dict(np.load(os.path.join(GOLD, "ba_small.npz")))
    pr = ba_case(20, 200)
    s = hip_ba(pr)
    s.buildSystem()
    assert abs(s.chi2() - gold["chi2"]) <= TOL_CHI * gold["chi2"]
    assert relerr(s.b(), gold["b"]) < TOL_MAT
    s.setLambda(float(gold["lam"]), True)
    assert s.solve()
    assert relerr(s.values(capi.HSCHUR), gold["Hschur"]) < TOL_MAT
    x = s.x()
    assert relerr(x, gold["x_dense"]) < 1e-9                                   # cond ~1e8 with lambda = 1
    assert relerr(x[:6 * pr["nP"]], gold["xp_ref_csparse"]) < 1e-9            # reference CSparse on Hschur


def test_huber_and_lm_trial_sequence():
    capi = _capi()
    pr = ba_case(60, 500, outlier_frac=0.05)
    s, o = hip_ba(pr, huber=1.0), oracle_ba(pr, huber=1.0)
    s.buildSystem()
    o.build_system()
    _cmp_system(s, o, capi)
    lam = 1e-5 * o.max_diagonal()
    for trial in range(3):                       # setLambda(backup) / solve / restoreDiagonal per LM trial
        s.setLambda(lam, True)
        o.set_lambda(lam, True)
        assert s.solve() and o.solve()
        tol, cond = dx_tolerance(o)
        assert relerr(s.x(), o.x()) < tol, (relerr(s.x(), o.x()), tol, cond)
        s.restoreDiagonal()
        o.restore_diagonal()
        lam *= 4.0
    assert relerr(s.values(capi.HPP), o.values("Hpp")) < TOL_MAT


def test_not_positive_definite_is_reported():
    pr = ba_case(12, 80)
    s, o = hip_ba(pr), oracle_ba(pr)
    s.buildSystem()
    o.build_system()
    lam = -10.0 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert o.solve() is False
    assert s.solve() is False                    # G2OHIP_NOT_PD, like csparse_helper.cpp:136
    s.restoreDiagonal()
    s.setLambda(1.0, True)
    assert s.solve() is True                     # the handle stays usable


def test_manhattan_golden_no_schur():
    """Config 1 input (manhattan3500, BlockSolver_3_2 semantics, no Schur): x of the first GN
    system against the reference CSparse golden vector; duplicate edges accumulate."""
    capi = _capi()
    g = manhattan_golden()
    J0, J1, err = O.se2_edges(g["estimates"], g["vi"], g["vj"], g["meas"])
    s = capi.HipBlockSolver(3, 2, 0)
    k = s.addEdgeSet(3, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
    s.buildStructure(g["nP"], 0, False)
    s.setEdgeData(k, J0, J1, g["omega"], err)
    s.buildSystem()
    assert s.nnzb(capi.HPP) == 8949
    assert relerr(s.b(), g["b0"]) < TOL_MAT
    assert abs(s.chi2() - g["chi2_gn"][0]) <= TOL_CHI * g["chi2_gn"][0]
    assert s.solve()
    assert relerr(s.x(), g["x_gn0"]) < 1e-8
    s.setLambda(float(g["lambda0"]), True)
    assert s.solve()
    assert relerr(s.x(), g["x_lm0"]) < 1e-8
    s.restoreDiagonal()
    # full Gauss-Newton run on the GPU solver reproduces the reference chi2 trajectory
    est = g["estimates"].copy()
    for it in range(5):
        J0, J1, err = O.se2_edges(est, g["vi"], g["vj"], g["meas"])
        s.setEdgeData(k, J0, J1, g["omega"], err)
        s.buildSystem()
        assert abs(s.chi2() - g["chi2_gn"][it]) <= 1e-6 * g["chi2_gn"][it]
        assert s.solve()
        est = O.se2_oplus(est, g["hidx"], s.x())


def test_narrow_seam_linear_solver():
    capi = _capi()
    g = manhattan_golden()
    J0, J1, err = O.se2_edges(g["estimates"], g["vi"], g["vj"], g["meas"])
    o = O.OracleSolver(3, 2, g["nP"], 0, schur=False)
    k = o.add_edge_set(3, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
    o.set_dims(k, 3, 3)
    o.build_structure()
    o.set_edge_data(k, J0, J1, g["omega"], err)
    o.build_system()
    cp, row = o.pattern("pp")
    ls = capi.HipLinearSolver(3, 0)
    ok, x = ls.solve(cp, row, o.values("Hpp"), o.b())
    assert ok and relerr(x, g["x_gn0"]) < 1e-8
    ok, x = ls.solve(cp, row, o.values("Hpp"), 2.0 * o.b())       # values-only refill, same pattern
    assert ok and relerr(x, 2.0 * g["x_gn0"]) < 1e-8
    bad = o.values("Hpp").copy()
    bad *= -1.0
    ok, _ = ls.solve(cp, row, bad, o.b())
    assert not ok
    ls.init()
    for leaf in (4, 64):                                            # ordering knobs do not change the answer
        ls.setOption("nd_leaf", leaf)
        ls.init()
        ok, x = ls.solve(cp, row, o.values("Hpp"), o.b())
        assert ok and relerr(x, g["x_gn0"]) < 1e-8
    st = ls.stats()
    assert st["choleskyNNZ"] > 0 and st["numFronts"] > 0


def test_landmark_seen_by_hundreds_of_poses_is_split_over_tiles():
    """A landmark whose blocks and pair list exceed a tile's LDS budget (here 200+ observations; a tile holds ~64) is cut
    into chunk-pair tiles with two block ranges each (build_structure).  Generic path: Jacobian arrays over the ABI,
    Hpl read from memory.  Hschur, Dinv, x against the oracle; the landmark's inverse is written by every one of its
    tiles (the same bits)."""
    from openslam_g2o_amd import capi, synthetic as S
    pr = S.make_ba_loops(640, 900, laps=4, hubs=2)
    Jp, Jc, err = S.ba_linearize(pr)
    pr.update(Jp=Jp, Jc=Jc, err=err, omega=S.ba_omega(pr))
    assert np.bincount(pr["pt_idx"]).max() > 200
    s = hip_ba(pr, huber=1.0)
    o = oracle_ba(pr, huber=1.0)
    s.buildSystem()
    o.build_system()
    s.setLambda(3.0, True)
    o.set_lambda(3.0, True)
    assert s.solve() and o.solve()
    assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < 1e-11
    assert relerr(s.values(capi.DINV), o.values("Dinv")) < 1e-12
    assert relerr(s.x(), o.x()) < dx_tolerance(o)[0]


@pytest.mark.parametrize("group", [2, 4, 7])
def test_grouped_trailing_updates_of_an_in_place_chain_equal_the_panel_by_panel_ones(group):
    """A large supernode is a chain of 48-column panels factorised in place in one frontal matrix.  Option big_group: a panel inside
    a group updates only the columns of the group's remaining panels, the group's last panel applies the whole group to the rest of
    the trailing matrix (rank-(group x 48) instead of `group` passes over it; csparse_helper.cpp:88-143 computes the same sums column
    by column).  big_group_min_rows lowered so that the hub front of this graph (every third pose sees the hub points: a dense
    supernode of 1 000+ rows) and the sphere's 882-row separators take the grouped path; x against the oracle / the golden vector and
    against big_group = 1 (same matrix, another summation order of the trailing updates: rounding only)."""
    from openslam_g2o_amd import capi, synthetic as S
    from tests.helpers import sphere_golden
    pr = S.make_ba_loops(640, 900, laps=4, hubs=2)
    Jp, Jc, err = S.ba_linearize(pr)
    pr.update(Jp=Jp, Jc=Jc, err=err, omega=S.ba_omega(pr))
    o = oracle_ba(pr, huber=1.0)
    o.build_system()
    o.set_lambda(3.0, True)
    assert o.solve()
    xs = {}
    for g in (1, group):
        s = hip_ba(pr, huber=1.0, options={"big_group": g, "big_group_min_rows": 64})
        s.buildSystem()
        s.setLambda(3.0, True)
        assert s.solve()
        xs[g] = s.x()
        assert s.stats()["maxFrontDim"] > 1000
        assert relerr(xs[g], o.x()) < dx_tolerance(o)[0]
        x2 = s.x()
        assert s.solve() and np.array_equal(s.x(), x2)            # bit-repeatable
    assert relerr(xs[group], xs[1]) < 1e-9 and not np.array_equal(xs[group], xs[1])   # (the grouped path really ran)
    # config 2 (no Schur complement): the sphere's separators
    gs = sphere_golden()
    J0, J1, e = O.se3_edges(gs["poses"], gs["vi"], gs["vj"], gs["Z"])
    s = capi.HipBlockSolver(6, 3, 0)
    s.setOption("big_group", group)
    s.setOption("big_group_min_rows", 64)
    k = s.addEdgeSet(6, gs["hidx"][gs["vi"]], gs["hidx"][gs["vj"]])
    s.buildStructure(gs["nP"], 0, False)
    s.setEdgeData(k, J0, J1, gs["omega"], e)
    s.buildSystem()
    assert s.solve()
    assert relerr(s.x(), gs["x_gn0"]) < 1e-7


def test_edge_cases_mixed_sets_fixed_and_unary():
    """Two edge sets (projection edges + 6-dof pose-pose edges), a unary prior set, fixed
    vertices on both sides, a landmark seen once, a pose without landmarks."""
    capi = _capi()
    rng = np.random.default_rng(3)
    pr = ba_case(16, 60)
    nP, nL = pr["nP"], pr["nL"]
    # drop all but one observation of landmark 0 and every observation of the last pose
    keep = np.ones(pr["E"], bool)
    keep[1:5] = False
    keep[pr["v1"] == nP - 1] = False
    v0, v1 = pr["v0"][keep], pr["v1"][keep]
    Jp, Jc, om, err = pr["Jp"][keep], pr["Jc"][keep], pr["omega"][keep], pr["err"][keep]
    # odometry-like pose-pose edges, some reversed (transposed block), one duplicate, one to a fixed pose
    a = np.arange(-1, nP - 1, dtype=np.int32)
    b = a + 1
    b[5], a[5] = a[5], b[5]
    a = np.append(a, a[7]).astype(np.int32)
    b = np.append(b, b[7]).astype(np.int32)
    n2 = len(a)
    JA, JB = rng.normal(size=(n2, 36)), rng.normal(size=(n2, 36))
    W = rng.normal(size=(n2, 6, 6))
    O2 = (W @ W.transpose(0, 2, 1) + 6 * np.eye(6)).reshape(n2, 36)
    e2 = rng.normal(size=(n2, 6))
    # unary priors on a few poses
    u = np.array([0, 3, nP - 1], np.int32)
    JU = rng.normal(size=(3, 18))
    WU = rng.normal(size=(3, 3, 3))
    OU = (WU @ WU.transpose(0, 2, 1) + 3 * np.eye(3)).reshape(3, 9)
    eU = rng.normal(size=(3, 3))

    s = capi.HipBlockSolver(6, 3, 0)
    k0 = s.addEdgeSet(2, v0, v1)
    k1 = s.addEdgeSet(6, a, b)
    k2 = s.addEdgeSet(3, u, None)
    s.buildStructure(nP, nL, True)
    s.setEdgeData(k0, Jp, Jc, om, err)
    s.setEdgeData(k1, JA, JB, O2, e2)
    s.setEdgeData(k2, JU, None, OU, eU)
    o = O.OracleSolver(6, 3, nP, nL, True)
    q0 = o.add_edge_set(2, v0, v1); o.set_dims(q0, 3, 6)
    q1 = o.add_edge_set(6, a, b); o.set_dims(q1, 6, 6)
    q2 = o.add_edge_set(3, u, None); o.set_dims(q2, 6, 0)
    o.build_structure()
    o.set_edge_data(q0, Jp, Jc, om, err)
    o.set_edge_data(q1, JA, JB, O2, e2)
    o.set_edge_data(q2, JU, None, OU, eU)
    s.buildSystem()
    o.build_system()
    for w, n in ((capi.HPP, "pp"), (capi.HPL, "pl"), (capi.HSCHUR, "hs")):
        assert np.array_equal(s.pattern(w)[1], o.pattern(n)[1])
    _cmp_system(s, o, capi)
    s.setLambda(10.0, True)
    o.set_lambda(10.0, True)
    assert s.solve() and o.solve()
    assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < TOL_MAT
    assert relerr(s.x(), o.x()) < 1e-9
    # rebuilding with new data after init() keeps working (Solver::init contract)
    s.init()
    s.buildSystem()
    s.setLambda(10.0, True)
    assert s.solve() and relerr(s.x(), o.x()) < 1e-9


def test_large_scale_properties():
    """Size-independent properties at a scale the oracle would need minutes for:
    residual of the damped system, linearity in b, symmetry of the Schur pipeline."""
    capi = _capi()
    pr = ba_case(20000, 200000)
    s = hip_ba(pr)
    s.buildSystem()
    lam = 1e-5 * s.maxDiagonal()
    s.setLambda(lam, True)
    assert s.solve()
    x, b = s.x(), s.b()
    r = s.multiplyHessian(x) - b
    assert np.abs(r).max() <= 1e-10 * np.abs(b).max()
    # linearity: doubling the errors doubles b and x (same H)
    s.setEdgeData(0, pr["Jp"], pr["Jc"], pr["omega"], 2.0 * pr["err"])
    s.restoreDiagonal()
    s.buildSystem()
    s.setLambda(lam, True)
    assert s.solve()
    assert relerr(s.x(), 2.0 * x) < 1e-9 and relerr(s.b(), 2.0 * b) < 1e-13
    st = s.stats()
    assert st["hessianPoseDimension"] == 6 * pr["nP"] and st["choleskyNNZ"] > 0


@pytest.mark.parametrize("fused", [True, False])
def test_indefinite_landmark_blocks_take_the_signed_split(fused):
    """block_solver.hpp:563-604 allows negative damping.  With the landmark diagonal damped by a NEGATIVE value between the
    eigenvalues of the landmark blocks, Dinv is indefinite: the Schur tiles' symmetric split Dinv = C Sg C' then carries
    signs (Sg != I, the per-tile flag path).  A large pose damping keeps the reduced system positive definite, so the solve
    succeeds and must equal the oracle's and a dense solve of the full damped system."""
    pr = ba_case(40, 400)
    s = hip_ba(pr) if fused else hip_ba(pr, options={"ba_fused": 0})
    o = oracle_ba(pr)
    s.buildSystem()
    o.build_system()
    Hll = o.values("Hll").reshape(-1, 3, 3)
    ev = np.linalg.eigvalsh(Hll)
    # -lam_l inside the widest gap of the eigenvalue spectrum that still splits the eigenvalues of >= 50 blocks (no block
    # gets close to singular), and a pose damping that dominates B Dinv B'
    allev = np.sort(ev.reshape(-1))
    best = None
    for a, b in zip(allev[:-1], allev[1:]):
        mid = 0.5 * (a + b)
        indef = int(((ev[:, 0] < mid) & (ev[:, 2] > mid)).sum())
        if indef >= 50 and (best is None or (b - a) / mid > best[0]):
            best = ((b - a) / mid, mid, indef)
    assert best is not None
    lam_l = -float(best[1])
    gap = float(np.abs(ev + lam_l).min())
    Hd = o.dense_full()
    lam_p = 100.0 * float(np.abs(Hd).max()) ** 2 / gap
    H = Hd.copy()
    nP6 = 6 * o.nP
    H[np.arange(nP6), np.arange(nP6)] += lam_p
    H[np.arange(nP6, H.shape[0]), np.arange(nP6, H.shape[0])] += lam_l
    xd = np.linalg.solve(H, o.b())
    s.setLambdaSplit(lam_p, lam_l, True)
    o.set_lambda_split(lam_p, lam_l, True)
    assert s.solve() and o.solve()
    s.restoreDiagonal()
    tol = 1e-9 * max(1.0, float(np.abs(Hd).max()) / gap)         # (conditioning of the damped landmark blocks)
    assert relerr(o.x(), xd) < tol
    assert relerr(s.x(), xd) < tol and relerr(s.x(), o.x()) < tol
    # and back to an ordinary solve afterwards (the flag is per solve)
    s.setLambda(5.0, True)
    o.restore_diagonal()
    o.set_lambda(5.0, True)
    assert s.solve() and o.solve()
    assert relerr(s.x(), o.x()) < 1e-9


def test_update_structure_grows_a_pose_graph_online():
    """Solver::updateStructure (block_solver.hpp:297-351): the manhattan graph built for its first 3 000 poses, solved, then
    grown by the remaining poses and edges (g2ohip_update_structure) -- the solution equals the one of a solver built on the
    whole graph and the reference's golden vector; with a Schur complement the call refuses like the reference."""
    capi = _capi()
    g = manhattan_golden()
    J0, J1, err = O.se2_edges(g["estimates"], g["vi"], g["vj"], g["meas"])
    h0, h1 = g["hidx"][g["vi"]], g["hidx"][g["vj"]]
    n0 = 3000
    first = (h0 < n0) & (h1 < n0)
    order = np.concatenate([np.nonzero(first)[0], np.nonzero(~first)[0]])
    nf = int(first.sum())
    s = capi.HipBlockSolver(3, 2, 0)
    k = s.addEdgeSet(3, h0[order[:nf]], h1[order[:nf]])
    s.buildStructure(n0, 0, False)
    s.setEdgeData(k, J0[order[:nf]], J1[order[:nf]], g["omega"][order[:nf]], err[order[:nf]])
    s.buildSystem()
    s.setLambda(float(g["lambda0"]), True)
    assert s.solve() and len(s.x()) == 3 * n0
    s.restoreDiagonal()
    assert s.updateStructure(g["nP"] - n0, k, h0[order[nf:]], h1[order[nf:]])
    assert len(s.b()) == 3 * g["nP"]
    s.setEdgeData(k, J0[order], J1[order], g["omega"][order], err[order])
    s.buildSystem()
    assert s.nnzb(capi.HPP) == 8949
    assert relerr(s.b(), g["b0"]) < TOL_MAT
    s.setLambda(float(g["lambda0"]), True)
    assert s.solve()
    assert relerr(s.x(), g["x_lm0"]) < 1e-8
    s.restoreDiagonal()
    # vertices only (no edges yet): structure grows, the new diagonal blocks are empty
    assert s.updateStructure(0)
    # a system with marginalised vertices: refused (the reference aborts)
    pr = ba_case(20, 200)
    sb = hip_ba(pr)
    assert sb.updateStructure(1) is False


@pytest.mark.parametrize("graph", ["manhattan", "sphere"])
def test_front_kernel_variants_agree_on_the_pose_graphs(graph):
    """The LDS-front kernel on the two golden pose graphs with all LDS levels in dependency-driven launches (dep_levels 64
    against 16 and against one launch per level: the schedule the stall fallback drops to).  Same solution to rounding, and the
    reference's.  (Round 6: the A/B options of the kernel's earlier forms -- fuse_fwd_any, lds_mfma -- left the library.)"""
    capi = _capi()
    from tests.helpers import sphere_golden
    if graph == "manhattan":
        g = manhattan_golden(); p, l, d = 3, 2, 3
        J0, J1, err = O.se2_edges(g["estimates"], g["vi"], g["vj"], g["meas"])
    else:
        g = sphere_golden(); p, l, d = 6, 3, 6
        J0, J1, err = O.se3_edges(g["poses"], g["vi"], g["vj"], g["Z"])
    xs, stats = [], []
    variants = ({}, {"dep_levels": 16}, {"dep_levels": 0})
    for opts in variants:
        s = capi.HipBlockSolver(p, l, 0)
        for k_, v_ in opts.items():
            s.setOption(k_, v_)
        k = s.addEdgeSet(d, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
        s.buildStructure(g["nP"], 0, False)
        s.setEdgeData(k, J0, J1, g["omega"], err)
        s.buildSystem()
        s.setLambda(float(g["lambda0"]), True)
        two = []
        for _ in range(2):
            assert s.solve(), opts
            two.append(s.x())
        assert np.array_equal(two[0], two[1])             # repeatable bit for bit
        s.restoreDiagonal()
        xs.append(two[0])
        stats.append(s.stats())
    assert relerr(xs[0], g["x_lm0"]) < 1e-8
    for x in xs[1:]:
        assert relerr(x, xs[0]) < 1e-11
    assert all(st["dependencyFallbacks"] == 0 for st in stats)


def test_sphere_golden_no_schur():
    """Config 2 input (sphere, 2 200 VertexSE3 / 8 647 EdgeSE3, BlockSolver_6_3 semantics, fp64,
    1 GPU): first-iteration x against the reference CSparse golden vectors, then three damped
    iterations reproduce the reference chi2 trajectory.  The nested-dissection fronts of this graph
    exceed the LDS budget, so the HBM-scratch front path is exercised too."""
    capi = _capi()
    from tests.helpers import sphere_golden
    g = sphere_golden()
    s = capi.HipBlockSolver(6, 3, 0)
    k = s.addEdgeSet(6, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
    s.buildStructure(g["nP"], 0, False)
    assert s.nnzb(capi.HPP) == 10843
    poses = g["poses"].copy()
    lam = float(g["lambda0"])
    for it in range(3):
        J0, J1, err = O.se3_edges(poses, g["vi"], g["vj"], g["Z"])
        s.setEdgeData(k, J0, J1, g["omega"], err)
        s.buildSystem()
        assert abs(s.chi2() - g["chi2_lm"][it]) <= 1e-6 * g["chi2_lm"][it]
        if it == 0:
            assert relerr(s.b(), g["b0"]) < TOL_MAT
            assert abs(s.maxDiagonal() * 1e-5 - lam) <= 1e-12 * lam
            assert s.solve()
            assert relerr(s.x(), g["x_gn0"]) < 1e-7
        s.setLambda(lam, True)
        assert s.solve()
        x = s.x()
        if it == 0:
            assert relerr(x, g["x_lm0"]) < 1e-8
        r = s.multiplyHessian(x) - s.b()
        assert np.abs(r).max() <= TOL_RES * np.abs(s.b()).max()
        s.restoreDiagonal()
        poses = O.se3_oplus(poses, g["hidx"], x)
    st = s.stats()
    assert st["maxFrontDim"] > 90          # large separators: scratch-slab fronts were used


def test_sharded_path_single_rank_rccl():
    """The N>1 code path on real hardware with world_size 1: RCCL process group, zero-copy torch views
    of the resident Hschur / bschur arrays (__cuda_array_interface__), the solver running on torch's
    stream, all-reduce, split solve -- must reproduce the plain solve."""
    import torch
    import torch.distributed as dist
    from openslam_g2o_amd import distributed as D
    capi = _capi()
    pr = ba_case(64, 700)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        sh = D.ShardedBlockSolver(6, 3, rank=0, world=1, force_exchange=True)   # union pattern + all-reduce on 1 rank
        info = sh.setup_ba(pr, torch_device=dev)
        assert info["L_local"] == pr["nL"]
        sh.buildSystem()
        sh.setLambda(25.0, True)
        ok = sh.solve()                   # all_reduce over a 1-rank group is the identity
        sh.restoreDiagonal()
        ts = sh._reduced_tensors()
        assert ts[0].is_cuda and ts[0].dtype == torch.float64 and ts[0].numel() == sh.local.nnzb(capi.HSCHUR) * 36
        x = sh.local.x()
        ref = hip_ba(pr)
        ref.buildSystem()
        ref.setLambda(25.0, True)
        assert ok and ref.solve()
        assert relerr(x, ref.x()) < 1e-12
        assert torch.allclose(ts[0].cpu(), torch.from_numpy(ref.values(capi.HSCHUR)), rtol=0, atol=1e-9)
    finally:
        dist.destroy_process_group()


def _dimension_family(p, l, d, pose_d=(), prior_d=0, schur=True):
    """One case of test_block_solver_dimension_families: 40 poses, 150 landmarks.  Edge sets: landmark observations of error
    dimension d (Schur only), a chain of pose-pose edges of full dimension, further pose-pose sets of the error dimensions
    pose_d (pose k -- pose k + 2, k + 3, ...) and, for prior_d > 0, unary edges of that error dimension on every landmark."""
    capi = _capi()
    rng = np.random.default_rng(100 * p + 10 * l + d)
    nP, nL, K = 40, 150 if schur else 0, 4 if d > 1 else 6

    def spd(n, m):
        W = rng.normal(size=(n, m, m))
        return (W @ W.transpose(0, 2, 1) + m * np.eye(m)).reshape(n, m * m)

    sets = []   # (error dim, v0, v1, dim0, dim1, J0, J1, omega, err, huber delta)
    if schur:
        pt = np.repeat(np.arange(nL), K)
        cam = (rng.integers(0, nP - K, size=nL)[:, None] + np.arange(K)[None, :]).reshape(-1)
        cam[rng.random(len(cam)) < 0.03] = -1                         # a few observations from fixed poses
        v0, v1 = (nP + pt).astype(np.int32), cam.astype(np.int32)
        E = len(v0)
        J0, J1 = rng.normal(size=(E, d * l)), rng.normal(size=(E, d * p))
        om = spd(E, d)
        sets.append((d, v0, v1, l, p, J0, J1, om, rng.normal(size=(E, d)), 1.5))
    # pose-pose edges of full dimension keep the pose system connected (EdgeSim3 / EdgeSE2 / EdgeSE3)
    for step, dd in enumerate((p,) + tuple(pose_d), 1):
        a, b = np.arange(0, nP - step, dtype=np.int32), np.arange(step, nP, dtype=np.int32)
        n = len(a)
        JA, JB = rng.normal(size=(n, dd * p)), rng.normal(size=(n, dd * p))
        O2 = spd(n, dd)
        sets.append((dd, a, b, p, p, JA, JB, O2, rng.normal(size=(n, dd)), 0.0))
    if prior_d:
        u = (nP + np.arange(nL)).astype(np.int32)
        sets.append((prior_d, u, None, l, 0, rng.normal(size=(nL, prior_d * l)), None, spd(nL, prior_d), rng.normal(size=(nL, prior_d)), 0.0))
    s = capi.HipBlockSolver(p, l, 0)
    ks = [s.addEdgeSet(dd, v0, v1) for dd, v0, v1, *_ in sets]
    s.buildStructure(nP, nL, schur)
    o = O.OracleSolver(p, l, nP, nL, schur)
    qs = []
    for dd, v0, v1, dim0, dim1, *_ in sets:
        qs.append(o.add_edge_set(dd, v0, v1))
        o.set_dims(qs[-1], dim0, dim1)
    o.build_structure()
    for k, q, (dd, v0, v1, dim0, dim1, J0, J1, om, err, delta) in zip(ks, qs, sets):
        s.setEdgeData(k, J0, J1, om, err)
        if delta:
            s.setRobustKernel(k, capi.KERNEL_HUBER, delta)
            o.set_edge_data(q, J0, J1, om, err, delta)
        else:
            o.set_edge_data(q, J0, J1, om, err)
    s.buildSystem()
    o.build_system()
    if schur:
        _cmp_system(s, o, capi)
    else:
        assert relerr(s.values(capi.HPP), o.values("Hpp")) < TOL_MAT
        assert relerr(s.b(), o.b()) < TOL_MAT
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-3 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    if schur:
        assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < TOL_MAT
    assert relerr(s.x(), o.x()) < 1e-9
    r = s.multiplyHessian(s.x()) - s.b()
    assert np.abs(r).max() <= TOL_RES * np.abs(s.b()).max()


@pytest.mark.parametrize("p,l,d", [(7, 3, 2), (7, 3, 3), (3, 2, 2), (3, 2, 1), (6, 3, 3), (6, 3, 1), (6, 3, 2), (3, 3, 2)])
def test_block_solver_dimension_families(p, l, d):
    """The fixed-size solver families of the reference (BlockSolver_7_3 / _3_2 / _6_3, block_solver.h:163-175) with the
    edge shapes its type libraries produce for them: sim3 projections (d=2/3 on 7-dof poses, types_seven_dof_expmap.h),
    SE2 landmark observations (d=2) and bearings (d=1, types_slam2d), 3D point observations (d=3) and depth-only (d=1),
    projections onto 6-dof poses (d=2) and the (3, 3) family.
    Random Jacobians / information through the generic edge-data path, Schur on, against the oracle."""
    _dimension_family(p, l, d)


@pytest.mark.parametrize("p,l,d,pose_d,prior_d,schur", [(6, 3, 2, (2, 3), 0, False), (3, 2, 2, (2,), 0, False), (3, 2, 2, (), 3, True)],
                         ids=["6-pose_d23-noschur", "3-pose_d2-noschur", "3-2-2-prior3"])
def test_block_solver_dimension_families_table_rows(p, l, d, pose_d, prior_d, schur):
    """The rows of the assembly tables the families above do not reach: pose-pose edges of an error dimension below the pose
    dimension (off-diagonal shapes (2,6,6), (3,6,6), (2,3,3): no Schur complement, poses only) and unary edges of error
    dimension 3 on 2D landmarks (vertex row (3,2)).  With the cases above, every row of dispatch_vertex and dispatch_offdiag,
    every chi2 dimension and the Schur pairs (6,3), (3,2), (7,3), (3,3) are launched at least once.  Not reachable through the
    edge-set interface: the Schur pair (6,2) -- no off-diagonal row (d,6,2) exists, so no pose-landmark set of it can be assembled."""
    _dimension_family(p, l, d, pose_d, prior_d, schur)


def test_unsupported_shapes_are_argument_errors():
    """A shape outside the assembly tables comes back as G2OHIP_ERR_ARG (-1) with the table's message, and the handle stays usable.
    (The block-size messages of the Cholesky / PCG launches cannot be reached through the C ABI: g2ohip_create and g2ohip_ls_create
    refuse a dimension other than 3, 6, 7.)"""
    capi = _capi()
    rng = np.random.default_rng(11)
    nP = 6
    a, b = np.arange(0, nP - 1, dtype=np.int32), np.arange(1, nP, dtype=np.int32)

    def pose_solver(p, d):
        s = capi.HipBlockSolver(p, 2 if p == 3 else 3, 0)
        k = s.addEdgeSet(d, a, b)
        s.buildStructure(nP, 0, False)
        s.setEdgeData(k, rng.normal(size=(nP - 1, d * p)), rng.normal(size=(nP - 1, d * p)), np.tile(np.eye(d).reshape(-1), (nP - 1, 1)),
                      rng.normal(size=(nP - 1, d)))
        return s

    def message(call):
        with pytest.raises(capi.G2oHipError) as e:
            call()
        assert "(-1)" in str(e.value)
        return str(e.value)

    s = pose_solver(6, 4)
    assert "chi2: unsupported error dimension" in message(s.chi2)
    assert "unsupported (error_dim, vertex_dim) = (4,6)" in message(s.buildSystem)
    s = pose_solver(3, 1)   # the vertex row (1,3) exists, the pose-pose off-diagonal shape (1,3,3) does not
    assert "unsupported off-diagonal block shape (d,rows,cols) = (1,3,3)" in message(s.buildSystem)
    s = pose_solver(3, 3)
    s.buildSystem()
    s.setLambda(1.0, True)
    assert s.solve()


def test_dependency_driven_launches_and_stall_fallback():
    """Levels of the elimination tree sharing one launch (parents wait on device-scope counters their children bump)
    give bit-identical results to one launch per level; a waiting workgroup that gives up (spin limit 0 forces it)
    flags the factorisation, the solver drops to per-level launches and repeats the solve."""
    pr = ba_case(600, 6000)
    xs = []
    cases = ({"dep_levels": 0}, {"dep_levels": 16, "dep_backward": 0}, {"dep_levels": 16, "dep_spin_limit": 0},
             {"dep_levels": 16}, {"dep_levels": 3, "use_graph": 1})
    for opts in cases:
        s = hip_ba(pr, options=opts)
        assert s.stats()["numLevels"] >= 4
        mine = []
        for it in range(3):
            s.buildSystem()
            s.setLambda(10.0, True)
            assert s.solve(), opts
            s.restoreDiagonal()
            mine.append(s.x())
        assert np.array_equal(mine[0], mine[1]) and np.array_equal(mine[0], mine[2])   # repeatable
        xs.append(mine[0])
    # the factorisation is bit-identical whatever the grouping; a grouped backward sweep runs every level with the
    # group's workgroup size, which changes the partition (not the terms) of its dot products
    assert np.array_equal(xs[1], xs[0]) and np.array_equal(xs[2], xs[0])
    assert relerr(xs[3], xs[0]) < 1e-13 and relerr(xs[4], xs[0]) < 1e-13
    o = oracle_ba(pr)
    o.build_system()
    o.set_lambda(10.0, True)
    assert o.solve() and relerr(xs[0], o.x()) < 1e-8


def test_schur_reduction_folded_into_factorisation():
    """solve() on one GPU skips the reduction pass of the Schur complement: the factorisation assembles its fronts
    from Hpp and the tiles' partial blocks (same operations, same order).  Bit-identical to the materialised path;
    Hschur is written on demand; the split API (solveSchur / solveReduced) keeps materialising."""
    capi = _capi()
    pr = ba_case(300, 3000)
    a, b = hip_ba(pr, options={"fuse_schur_reduce": 1}), hip_ba(pr, options={"fuse_schur_reduce": 0})
    for s in (a, b):
        s.buildSystem()
        s.setLambda(7.0, True)
        assert s.solve()
    assert np.array_equal(a.x(), b.x())
    assert np.array_equal(a.values(capi.HSCHUR), b.values(capi.HSCHUR))
    xa = a.x()
    a.solveSchur()
    assert a.solveReduced()
    a.solveBackSubstitute()
    assert np.array_equal(a.x(), xa)
    assert a.solve() and np.array_equal(a.x(), xa)          # and back to the folded path
    o = oracle_ba(pr)
    o.build_system()
    o.set_lambda(7.0, True)
    assert o.solve() and relerr(xa, o.x()) < 1e-8
    assert relerr(a.values(capi.HSCHUR), o.values("Hschur")) < TOL_MAT


@pytest.mark.parametrize("fold", [1, 0])
def test_ba_with_large_fronts(fold):
    """BA whose reduced system is nearly dense (every landmark seen by 60 of 100 cameras): the fronts exceed the
    LDS budget, so the scratch-slab path (whole-GPU passes, MFMA trailing update) runs on a Schur complement --
    with the reduction folded into the large fronts' assembly (fold=1) and from a materialised Hschur (fold=0)."""
    capi = _capi()
    pr = ba_case(100, 240, obs_per_landmark=60)
    s = hip_ba(pr, options={"fuse_schur_reduce": fold})
    assert s.stats()["maxFrontDim"] >= 240
    o = oracle_ba(pr)
    s.buildSystem()
    o.build_system()
    lam = 1e-4 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < TOL_MAT
    assert relerr(s.x(), o.x()) < 1e-7
    r = s.multiplyHessian(s.x()) - s.b()
    assert np.abs(r).max() <= 1e-9 * np.abs(s.b()).max()


def _random_block_spd(bs, nb, dens, seed):
    """Random block-sparse SPD matrix (dense array) and its upper block-CCS arrays (column-major blocks)."""
    rng = np.random.default_rng(seed)
    mask = np.triu(rng.random((nb, nb)) < dens, 1)
    mask |= np.eye(nb, k=1, dtype=bool)                      # connected
    n = nb * bs
    A = np.zeros((n, n))
    for j in range(nb):
        for i in np.nonzero(mask[:, j])[0]:
            A[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs] = rng.normal(size=(bs, bs))
    A = A + A.T
    A += np.eye(n) * (np.abs(A).sum(axis=1).max() + 1.0)     # strictly diagonally dominant: SPD
    cp, row, vals = [0], [], []
    for j in range(nb):
        for i in range(j + 1):
            if i == j or mask[i, j]:
                row.append(i)
                vals.append(A[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs].T.reshape(-1))
        cp.append(len(row))
    return A, np.array(cp, np.int32), np.array(row, np.int32), np.array(vals), rng


@pytest.mark.parametrize("bs", [3, 6, 7])
def test_scratch_slab_sweep_variants(bs):
    """The scratch-slab fronts (several workgroups per front with ticketed partial sums, forward step inside the panel kernel,
    zero fill + original blocks per phase) against a dense LAPACK solve, in the default schedule, with one launch per level (what
    the stall fallback uses) and with one workgroup per front (big_front_passes = 0).  (Round 6: the options that selected the
    earlier forms of these kernels one by one left the library with the forms.)"""
    capi = _capi()
    A, cp, row, vals, rng = _random_block_spd(bs, 200 if bs > 3 else 380, 0.2, 70 + bs)
    b = rng.normal(size=A.shape[0])
    xr = np.linalg.solve(A, b)
    variants = {
        "default": {},
        "one launch per level": {"dep_levels": 0},
        "one workgroup per scratch-slab front": {"big_front_passes": 0},
    }
    xs = {}
    for name, opts in variants.items():
        ls = capi.HipLinearSolver(bs, 0)
        for k, v in opts.items():
            ls.setOption(k, v)
        ok, x = ls.solve(cp, row, vals, b)
        assert ok, name
        assert ls.stats()["maxFrontDim"] >= 512, "the case must reach the multi-workgroup sweeps"
        assert relerr(x, xr) < 1e-10, name
        for _ in range(10 if name == "default" else 1):   # (the default form hands results between workgroups inside launches)
            ok, x2 = ls.solve(cp, row, vals, b)
            assert ok and np.array_equal(x, x2), name + ": not repeatable"
        xs[name] = x
        if name == "default":
            # (fronts of 1 000 rows and more: panels of 64 scalars, pivot block + panel rows in one launch with the rows on the matrix cores --
            # big_panel_solve_kernel --, the level's extend-add in one launch) a matrix that is not positive definite is reported from
            # there too, and the handle solves the good one again afterwards, to the same bits
            assert ls.stats()["maxFrontDim"] >= 1024
            bad, _ = ls.solve(cp, row, -vals, b)
            assert not bad
            ok, x3 = ls.solve(cp, row, vals, b)
            assert ok and np.array_equal(x, x3)
    assert relerr(xs["one launch per level"], xs["default"]) < 1e-12


def test_merged_backward_launch_stall_fallback():
    """A chunk of a merged backward launch that gives up waiting for its parent front (spin limit 0 forces it) flags the
    solve; the LinearSolver seam repeats it with one launch per level (NOT "not positive definite") and stays there."""
    capi = _capi()
    A, cp, row, vals, rng = _random_block_spd(6, 200, 0.2, 91)
    b = rng.normal(size=A.shape[0])
    xr = np.linalg.solve(A, b)
    ls = capi.HipLinearSolver(6, 0)
    ls.setOption("dep_spin_limit", 0)
    for _ in range(3):
        ok, x = ls.solve(cp, row, vals, b)
        assert ok and relerr(x, xr) < 1e-10
    ls2 = capi.HipLinearSolver(6, 0)
    ls2.setOption("dep_levels", 0)
    ok, x2 = ls2.solve(cp, row, vals, b)
    assert ok and relerr(x, x2) < 1e-13      # (the fallback also ungroups the sweeps of the LDS fronts: same terms, other partitions)


@pytest.mark.parametrize("bs", [3, 6, 7])
@pytest.mark.parametrize("passes", [1, 0])
def test_linear_solver_large_fronts_all_block_sizes(bs, passes):
    """LinearSolver seam on random block-sparse SPD systems dense enough for fronts of several hundred rows: the
    scratch-slab path for every block size (whole-GPU passes with the MFMA update, and one workgroup per front),
    against a dense LAPACK solve."""
    capi = _capi()
    rng = np.random.default_rng(50 + bs)
    nb = 160 if bs > 3 else 260
    dens = 0.18
    mask = np.triu(rng.random((nb, nb)) < dens, 1)
    mask |= np.eye(nb, k=1, dtype=bool)                      # connected
    n = nb * bs
    A = np.zeros((n, n))
    for j in range(nb):
        for i in np.nonzero(mask[:, j])[0]:
            A[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs] = rng.normal(size=(bs, bs))
    A = A + A.T
    A += np.eye(n) * (np.abs(A).sum(axis=1).max() + 1.0)     # strictly diagonally dominant: SPD
    cp, row, vals = [0], [], []
    for j in range(nb):
        for i in range(j + 1):
            if i == j or mask[i, j]:
                row.append(i)
                vals.append(A[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs].T.reshape(-1))   # column-major block
        cp.append(len(row))
    cp, row, vals = np.array(cp, np.int32), np.array(row, np.int32), np.array(vals)
    b = rng.normal(size=n)
    ls = capi.HipLinearSolver(bs, 0)
    ls.setOption("big_front_passes", passes)
    ok, x = ls.solve(cp, row, vals, b)
    assert ok
    assert ls.stats()["maxFrontDim"] >= 240
    xr = np.linalg.solve(A, b)
    assert relerr(x, xr) < 1e-10
    # LinearSolver::solvePattern: blocks of the inverse -- diagonal ones, pairs of the pattern, and a pair that may lie outside it
    Ainv = np.linalg.inv(A)
    pr_ = [(j, j) for j in range(0, nb, 17)] + [(int(row[q]), j) for j in range(0, nb, 23) for q in range(cp[j], cp[j + 1])][:40] + [(nb - 1, 0), (0, nb - 1)]
    rr, cc = np.array([a for a, _ in pr_], np.int32), np.array([c for _, c in pr_], np.int32)
    M = ls.solvePattern(cp, row, vals, rr, cc)
    assert M is not None and M.shape == (len(rr), bs, bs)
    for i in range(len(rr)):
        ref = Ainv[rr[i] * bs:(rr[i] + 1) * bs, cc[i] * bs:(cc[i] + 1) * bs]
        assert np.abs(M[i] - ref).max() <= 1e-10 * np.abs(Ainv).max(), (rr[i], cc[i])
    ok, _ = ls.solve(cp, row, -vals, b)
    assert not ok
    assert ls.solvePattern(cp, row, -vals, rr[:2], cc[:2]) is None
    if passes == 1:
        # a supernode cap beyond 64 scalars is capped by the analysis (wider pivot panels have no whole-GPU pass and used to fall back
        # to one workgroup per front): the same fronts as with 60, the same solution
        a, c = capi.HipLinearSolver(bs, 0), capi.HipLinearSolver(bs, 0)
        a.setOption("max_sn_scalars", 144)
        c.setOption("max_sn_scalars", 64)
        oka, xa = a.solve(cp, row, vals, b)
        okc, xc = c.solve(cp, row, vals, b)
        assert oka and okc and a.stats()["numFronts"] == c.stats()["numFronts"] and np.array_equal(xa, xc)
        assert relerr(xa, xr) < 1e-10


def test_dependency_driven_launches_soak():
    """Random problem sizes / leaf sizes through the dependency-driven launches (tools/probe/soak_dep.py, short form):
    bit-identical factorisation against one launch per level, repeatable across solves."""
    import subprocess
    import sys
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probe", "soak_dep.py")
    out = subprocess.run([sys.executable, tool, "3", "24"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "problems 24 bad 0" in out.stdout, out.stdout[-2000:]


@pytest.mark.parametrize("kind", [2, 3, 4, 5])
def test_robust_kernels_other_than_huber(kind):
    """PseudoHuber, Cauchy, Saturated and DCS (robust_kernel_impl.cpp:80-126) through assembly, chi2 and a damped solve,
    generic edge-data path and fused BA path, against the oracle."""
    capi = _capi()
    pr = ba_case(40, 400, outlier_frac=0.1)
    delta = 1.2
    o = oracle_ba(pr, huber=delta)
    o.set_robust_kernel(0, kind)
    o.build_system()
    s = hip_ba(pr)
    s.setRobustKernel(0, kind, delta)
    s.buildSystem()
    _cmp_system(s, o, capi)
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-3 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    assert relerr(s.x(), o.x()) < 1e-8
    from openslam_g2o_amd import lm
    sf, g = lm.setup_device_ba(pr)
    sf.setRobustKernel(0, kind, delta)
    g.linearize()
    sf.buildSystem()
    assert relerr(sf.b(), o.b()) < 1e-11 and abs(sf.chi2() - o.chi2()) <= 1e-11 * o.chi2()
    with pytest.raises(Exception):
        s.setRobustKernel(0, 9, 1.0)


def test_env_options_are_applied_by_the_library(monkeypatch):
    """G2OHIP_OPTIONS is parsed inside g2ohip_create / g2ohip_ls_create (round-3 advisor finding: C and C++ consumers such as
    the g2o plugin ignored it when only the Python wrapper read it): a valid list changes the kernels used (same solution),
    a malformed or unknown entry fails the creation with G2OHIP_ERR_ARG and a message."""
    capi = _capi()
    pr = ba_case(30, 300)
    ref = hip_ba(pr)
    ref.buildSystem()
    assert ref.solve()
    monkeypatch.setenv("G2OHIP_OPTIONS", " band_kernel=0, dep_levels = 0 ")
    s = hip_ba(pr)
    s.buildSystem()
    assert s.solve()
    assert relerr(s.x(), ref.x()) < 1e-9
    monkeypatch.setenv("G2OHIP_OPTIONS", "band_kernel=0,ba_fused=1")   # the narrow seam skips block-solver-only names
    capi.HipLinearSolver(3)
    monkeypatch.setenv("G2OHIP_OPTIONS", "band_kernel")
    with pytest.raises(capi.G2oHipError, match="malformed"):
        capi.HipBlockSolver(6, 3, 0)
    monkeypatch.setenv("G2OHIP_OPTIONS", "no_such_option=1")
    with pytest.raises(capi.G2oHipError, match="unknown option"):
        capi.HipBlockSolver(6, 3, 0)
