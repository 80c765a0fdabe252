"""GPU: landmark SLAM on the device -- odometry edges (EdgeSE2 / EdgeSE3) plus observations of point landmarks
(EdgeSE2PointXY / EdgeSE3PointXYZ with a sensor offset) bound to ONE handle of the pose-graph front end
(g2ohip_pg_set_landmark_edges / _estimates), landmarks marginalised (BlockSolver_3_2 / BlockSolver_6_3): producers against
the NumPy restatement of tests/landmark_helpers.py, the assembled and reduced system and its solution against the CPU
oracle fed the NumPy Jacobians, vertex updates and the estimate stack, whole Levenberg-Marquardt runs, error paths."""
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm, synthetic as S
from oracle import oracle as O
from tests import landmark_helpers as LH
from tests.helpers import dx_tolerance, relerr

pytestmark = pytest.mark.gpu

TOL_J = 1e-12      # producers: same formulas in fp64 (TOL_J of tests/test_gpu_posegraph.py)
TOL_B = 1e-11      # right-hand side (the parity tests' bound for b)
TOL_HS = 1e-12     # reduced system (TOL_MAT of the parity tests)
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE

# Relative chi2 gap per LM iteration between two equally valid oracle runs of test_lm_run_matches_oracle's graphs (the
# oracle's Schur path against the same loop solving the full system [Hpp Hpl; Hpl' Hll] without elimination), measured on
# the CPU (tools/landmark_slam_time.py --drift, profiles/landmark_slam.jsonl): the two differ by rounding only.
ORACLE_DRIFT = {
    "se2": [3.266e-15, 1.511e-14, 4.720e-14, 3.459e-15, 1.515e-15, 8.661e-16, 6.496e-16, 1.516e-15, 4.114e-15, 8.661e-16],
    "se3": [1.573e-15, 8.597e-15, 3.668e-14, 1.268e-14, 2.149e-15, 7.171e-16, 1.578e-15, 1.434e-16, 5.737e-16, 2.868e-16],
}

CASES = {"se2": ("se2", 400, 150), "se3": ("se3", 200, 300)}


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _graph(kind, **kw):
    k, n, L = CASES[kind]
    return S.make_landmark_slam(k, n, L, **kw)


def _feed_oracle(g, o, huber=0.0, poses=None, points=None):
    A0, A1, e0 = LH.pose_edges(g, poses=poses)
    B0, B1, e1 = LH.landmark_edges(g, poses=poses, points=points)
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    o.set_edge_data(1, B0, B1, g["omega_l"], e1, huber)
    return (A0, A1, e0), (B0, B1, e1)


@pytest.mark.parametrize("kind,fixed_landmarks", [("se2", 0), ("se3", 3)])
def test_producers_system_and_solution_against_oracle(kind, fixed_landmarks):
    """edgeData of both sets against the NumPy restatement; buildSystem + solve with the landmarks marginalised against
    OracleSolver fed the NumPy Jacobians.  One pose is fixed (gauge); the 3-D case also fixes three landmarks."""
    capi = _capi()
    g = _graph(kind, fixed_landmarks=fixed_landmarks)
    dp, dl = LH.dims(g)
    s, graph = lm.setup_device_landmark_slam(g)
    k0, k1 = s.landmark_sets
    graph.linearize()
    o = LH.oracle_landmark(g, True)
    (A0, A1, e0), (B0, B1, e1) = _feed_oracle(g, o)
    dA0, dA1, de0 = s.edgeData(k0, g["E"], dp, dp, dp)
    dB0, dB1, de1 = s.edgeData(k1, g["M"], dl, dp, dl)
    figs = dict(J0_pose=relerr(dA0, A0), J1_pose=relerr(dA1, A1), err_pose=relerr(de0, e0), J0_lm=relerr(dB0, B0),
                J1_lm=relerr(dB1, B1), err_lm=relerr(de1, e1))
    print(kind, "producers", figs)
    assert max(figs.values()) < TOL_J, figs
    s.buildSystem()
    o.build_system()
    print(kind, "b", relerr(s.b(), o.b()), "chi2", s.chi2(), o.chi2())
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    tol, cond = dx_tolerance(o)
    fig = dict(Hschur=relerr(s.values(capi.HSCHUR), o.values("Hschur")), dx=relerr(s.x(), o.x()), tol=tol, cond=cond)
    print(kind, "solve", fig)
    assert np.array_equal(s.pattern(capi.HSCHUR)[1], o.pattern("hs")[1])
    assert fig["Hschur"] < TOL_HS
    assert fig["dx"] < tol
    s.restoreDiagonal()
    # error-only evaluation leaves the Jacobians and gives the same errors
    s.pgLinearize(False)
    assert relerr(s.edgeData(k1, g["M"], dl, dp, dl)[2], e1) < TOL_J
    # both store forms of the landmark kernels write the same numbers
    s.setOption("pg_landmark_staged", 0)
    s.pgLinearize(True)
    xB0, xB1, xe1 = s.edgeData(k1, g["M"], dl, dp, dl)
    assert np.array_equal(xB0, dB0) and np.array_equal(xB1, dB1) and np.array_equal(xe1, de1)


@pytest.mark.parametrize("kind", ["se2", "se3"])
@pytest.mark.parametrize("per_edge", [False, True])
def test_robust_kernel_on_the_observation_set(kind, per_edge):
    """Huber on the observations, outliers in the data: chi2, b, the reduced system and dx against the oracle with the same
    kernel -- once as the set's kernel, once as a per-edge kernel array."""
    capi = _capi()
    g = _graph(kind, outlier_frac=0.05)
    delta = 1.0
    s, graph = lm.setup_device_landmark_slam(g, huber_delta=0.0 if per_edge else delta)
    k0, k1 = s.landmark_sets
    if per_edge:
        s.setRobustKernelPerEdge(k1, np.full(g["M"], capi.KERNEL_HUBER, np.int32), np.full(g["M"], delta))
    graph.linearize()
    s.buildSystem()
    o = LH.oracle_landmark(g, True)
    (_, _, e0), (_, _, e1) = _feed_oracle(g, o, huber=delta)
    o.build_system()
    w = np.einsum("ni,nij,nj->n", e1, g["omega_l"].reshape(g["M"], e1.shape[1], e1.shape[1]), e1)
    assert (w > delta * delta).sum() > 0.02 * g["M"]                    # the kernel is active on the outliers
    print(kind, per_edge, "chi2", s.chi2(), o.chi2(), "b", relerr(s.b(), o.b()))
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    assert relerr(s.b(), o.b()) < TOL_B
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    tol, _ = dx_tolerance(o)
    assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < TOL_HS
    assert relerr(s.x(), o.x()) < tol


@pytest.mark.parametrize("kind", ["se2", "se3"])
def test_update_and_estimate_stack(kind):
    g = _graph(kind, fixed_landmarks=2)
    dp, dl = LH.dims(g)
    s, graph = lm.setup_device_landmark_slam(g)
    graph.linearize()
    s.buildSystem()
    s.setLambda(1e-3 * s.maxDiagonal(), True)
    assert s.solve()
    s.restoreDiagonal()
    x = s.x()
    assert np.abs(x[dp * g["nP"]:]).max() > 0
    assert np.array_equal(s.pgGetEstimates(), g["poses"]) and np.array_equal(s.pgGetLandmarkEstimates(), g["points"])
    s.pgPush()
    with pytest.raises(capi_error()):
        s.pgPush()                                                   # one level
    s.pgUpdate()
    oplus = O.se2_oplus if kind == "se2" else O.se3_oplus
    poses1 = oplus(g["poses"], g["hidx"], x)
    points1 = LH.points_oplus(g["points"], g["pt_hidx"], x, dp * g["nP"], g["nP"])
    dpose, dpts = s.pgGetEstimates(), s.pgGetLandmarkEstimates()
    print(kind, "update", np.abs(dpose - poses1).max(), np.abs(dpts - points1).max())
    assert np.abs(dpose - poses1).max() < 1e-12 * np.abs(poses1).max()
    assert np.abs(dpts - points1).max() < 1e-12 * np.abs(points1).max()
    assert np.array_equal(dpose[0], g["poses"][0]) and np.array_equal(dpts[:2], g["points"][:2])   # fixed vertices stay
    assert not np.array_equal(dpts[2:], g["points"][2:])
    s.pgPop()
    assert np.array_equal(s.pgGetEstimates(), g["poses"]) and np.array_equal(s.pgGetLandmarkEstimates(), g["points"])
    s.pgPush()
    s.pgUpdate()
    s.pgDiscardTop()
    assert np.array_equal(s.pgGetLandmarkEstimates(), dpts)
    with pytest.raises(capi_error()):
        s.pgPop()


def capi_error():
    return _capi().G2oHipError


def _drift_bound(kind):
    return [max(1e-12, 10.0 * d) for d in ORACLE_DRIFT[kind]]


@pytest.mark.parametrize("kind", ["se2", "se3"])
def test_lm_run_matches_oracle(kind):
    """Ten Levenberg-Marquardt iterations (lm.optimize) with everything on the device against the same loop over
    OracleSolver + the NumPy producers: chi2 of iteration 0 to 1e-12 relative, the same accepted / rejected pattern of LM
    trials, and chi2 of every later iteration within ten times the gap that two equally valid CPU runs show at that
    iteration (floor 1e-12): ORACLE_DRIFT above, the oracle's Schur path against the full system solved without elimination.
    Measured gaps (relative, iterations 0..9): 2-D 3.3e-15 1.5e-14 4.7e-14 3.5e-15 1.5e-15 8.7e-16 6.5e-16 1.5e-15 4.1e-15
    8.7e-16; 3-D 1.6e-15 8.6e-15 3.7e-14 1.3e-14 2.1e-15 7.2e-16 1.6e-15 1.4e-16 5.7e-16 2.9e-16; both CPU runs take one
    trial in every iteration.  Ten times the largest of them is 4.7e-13, so the floor of 1e-12 is the bound everywhere.
    The device run with use_graph = 1 gives the same trajectory as with 0."""
    g = LH.lm_test_graph(kind)
    s, graph = lm.setup_device_landmark_slam(g)
    n_gpu, chi_gpu, lam_gpu, tr_gpu = lm.optimize(graph, s, 10, "lm")
    n_cpu, chi_cpu, lam_cpu, tr_cpu, og = LH.oracle_lm_run(g, 10)
    gaps = [abs(a - b) / b for a, b in zip(chi_gpu, chi_cpu)]
    print(kind, "lm chi2 gpu", chi_gpu)
    print(kind, "lm chi2 cpu", chi_cpu)
    print(kind, "lm gaps", gaps, "bound", _drift_bound(kind), "trials", tr_gpu, tr_cpu)
    assert n_gpu == n_cpu == 10 and tr_gpu == tr_cpu
    assert gaps[0] < 1e-12 or n_gpu == 0
    for it, (gap, bound) in enumerate(zip(gaps, _drift_bound(kind))):
        assert gap <= bound, (it, gap, bound)
    assert chi_gpu[-1] < 0.01 * chi_gpu[0]
    s2, graph2 = lm.setup_device_landmark_slam(g, options={"use_graph": 1})
    n2, chi2, lam2, tr2 = lm.optimize(graph2, s2, 10, "lm")
    assert n2 == n_gpu and tr2 == tr_gpu
    assert np.array_equal(chi2, chi_gpu) and np.array_equal(lam2, lam_gpu)
    assert np.array_equal(s2.pgGetEstimates(), s.pgGetEstimates())
    assert np.array_equal(s2.pgGetLandmarkEstimates(), s.pgGetLandmarkEstimates())
    # the optimum is near the ground truth (gauge: pose 0)
    e0 = np.abs(g["points"] - g["points_true"]).max()
    e1 = np.abs(s.pgGetLandmarkEstimates() - g["points_true"]).max()
    assert e1 < 0.5 * e0, (e0, e1)


def test_without_schur_the_pose_block_alone_is_solved():
    """do_schur = 0 with landmarks in the structure: the front end adds nothing of its own -- the system is assembled in full,
    solve() factorises Hpp alone (x_p = Hpp^-1 b_p) and leaves the landmark part of x at zero, exactly what
    OracleSolver(schur=False) does; pgUpdate then moves the poses and leaves the landmarks."""
    capi = _capi()
    g = _graph("se2")
    s, graph = lm.setup_device_landmark_slam(g, schur=False)
    graph.linearize()
    s.buildSystem()
    o = LH.oracle_landmark(g, False)
    _feed_oracle(g, o)
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B
    for w, n in ((capi.HPP, "Hpp"), (capi.HPL, "Hpl"), (capi.HLL, "Hll")):
        assert relerr(s.values(w), o.values(n)) < TOL_HS
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    x, xo = s.x(), o.x()
    nps = 3 * g["nP"]
    assert relerr(x[:nps], xo[:nps]) < 1e-8
    assert not x[nps:].any() and not xo[nps:].any()
    s.pgUpdate()
    assert np.array_equal(s.pgGetLandmarkEstimates(), g["points"]) and not np.array_equal(s.pgGetEstimates(), g["poses"])


def _rc(fn, *a):
    return fn(*a)


def test_error_paths():
    capi = _capi()
    L = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = _graph("se2")
    h, hl = g["hidx"], g["pt_hidx"]
    vi, vj, vp, vl = (_i32(g[k]) for k in ("vi", "vj", "vp", "vl"))
    Z, om, zl, oml, pts = (_f64(g[k]) for k in ("Z", "omega", "zl", "omega_l", "points"))

    def fresh(p=3, l=2):
        s = capi.HipBlockSolver(p, l, 0)
        k0 = s.addEdgeSet(p, h[vi], h[vj])
        k1 = s.addEdgeSet(l, h[vp], hl[vl])
        s.buildStructure(g["nP"], g["nL"], True)
        return s, k0, k1

    def set_lm(s, k, typ, a=vp, b=vl, off=None):
        return L.g2ohip_pg_set_landmark_edges(s.h, k, typ, _ip(a), _ip(b), _dp(zl), _dp(oml), None if off is None else _dp(off))

    # landmark edges / estimates before pgSetEdges
    s, k0, k1 = fresh()
    assert set_lm(s, k1, 3) == STATE
    assert L.g2ohip_pg_set_landmark_estimates(s.h, g["L"], _dp(pts), _ip(_i32(hl))) == STATE
    s.pgSetEdges(k0, 1, vi, vj, Z, om)
    s.pgSetEstimates(g["poses"], h)
    # wrong pairing, wrong set, offset on a 2-D set
    assert set_lm(s, k1, 4) == ARG                                   # EdgeSE3PointXYZ beside an EdgeSE2 pose set
    assert set_lm(s, k1, 5) == ARG
    assert set_lm(s, k0, 3) == ARG                                   # the pose-pose set as landmark set
    assert set_lm(s, k1, 3, off=_f64(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]))) == ARG
    # an index whose hessian index disagrees with the edge set, an index out of range
    bad = vp.copy()
    bad[7] = bad[7] + 1 if bad[7] + 1 < g["n"] else bad[7] - 1
    assert set_lm(s, k1, 3, a=bad) == ARG
    bad = vl.copy()
    bad[5] = g["L"] + 3
    assert set_lm(s, k1, 3) == 0
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE                    # landmark edges bound, no landmark estimates
    assert set_lm(s, k1, 3, b=bad) == 0                              # (the landmark table is not known yet ...)
    assert L.g2ohip_pg_set_landmark_estimates(s.h, g["L"], _dp(pts), _ip(_i32(hl))) == ARG   # ... now it is: out of range
    assert set_lm(s, k1, 3) == 0
    wrong = _i32(hl).copy()
    wrong[4], wrong[5] = wrong[5], wrong[4]
    assert L.g2ohip_pg_set_landmark_estimates(s.h, g["L"], _dp(pts), _ip(wrong)) == ARG
    wrong = _i32(hl).copy()
    wrong[4] = g["nP"] - 1                                           # a pose's index
    assert L.g2ohip_pg_set_landmark_estimates(s.h, g["L"], _dp(pts), _ip(wrong)) == ARG
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE
    s.pgSetLandmarkEstimates(pts, hl)
    s.pgLinearize(True)
    s.buildSystem()
    assert s.chi2() > 0
    # the binding goes with g2ohip_clear_edge_sets
    s.clearEdgeSets()
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE
    k0 = s.addEdgeSet(3, h[vi], h[vj])
    k1 = s.addEdgeSet(2, h[vp], hl[vl])
    s.buildStructure(g["nP"], g["nL"], True)
    assert set_lm(s, k1, 3) == STATE                                 # pgSetEdges first, again
    s.pgSetEdges(k0, 1, vi, vj, Z, om)
    s.pgSetEstimates(g["poses"], h)
    assert L.g2ohip_pg_linearize(s.h, 1) == 0                        # pose half alone: as before
    assert set_lm(s, k1, 3) == 0
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE
    s.pgSetLandmarkEstimates(pts, hl)
    assert L.g2ohip_pg_linearize(s.h, 1) == 0
    # a rejected call commits nothing: the previous table / binding stands
    s.buildSystem()
    chi0, est0 = s.chi2(), s.pgGetEstimates()
    wrong = _i32(h).copy()
    wrong[3], wrong[4] = wrong[4], wrong[3]
    assert wrong[3] != wrong[4]
    assert L.g2ohip_pg_set_estimates(s.h, len(wrong), _dp(_f64(g["poses"] + 0.25)), _ip(wrong)) == ARG
    assert np.array_equal(s.pgGetEstimates(), est0)
    assert L.g2ohip_pg_linearize(s.h, 1) == 0
    s.buildSystem()
    assert s.chi2() == chi0
    bad = vi.copy()                                                  # one vi whose hessian index disagrees with the edge set
    bad[7] = (bad[7] + 1) % len(h)
    assert h[bad[7]] != h[vi[7]]
    assert L.g2ohip_pg_set_edges(s.h, k0, 1, _ip(bad), _ip(vj), _dp(_f64(Z + 0.25)), _dp(om)) == ARG
    assert L.g2ohip_pg_linearize(s.h, 1) == 0
    s.buildSystem()
    assert s.chi2() == chi0
    assert np.array_equal(s.pgGetEstimates(), est0)
    # type 3 beside an SE3 pose set
    g3 = _graph("se3")
    h3, hl3 = g3["hidx"], g3["pt_hidx"]
    s3 = capi.HipBlockSolver(6, 3, 0)
    q0 = s3.addEdgeSet(6, h3[g3["vi"]], h3[g3["vj"]])
    q1 = s3.addEdgeSet(3, h3[g3["vp"]], hl3[g3["vl"]])
    s3.buildStructure(g3["nP"], g3["nL"], True)
    s3.pgSetEdges(q0, 2, g3["vi"], g3["vj"], g3["Z"], g3["omega"])
    rc = L.g2ohip_pg_set_landmark_edges(s3.h, q1, 3, _ip(_i32(g3["vp"])), _ip(_i32(g3["vl"])), _dp(_f64(g3["zl"])),
                                        _dp(_f64(g3["omega_l"])), None)
    assert rc == ARG
    s3.pgSetLandmarkEdges(q1, 4, g3["vp"], g3["vl"], g3["zl"], g3["omega_l"], g3["offset"])


def test_profile_of_the_oracle_drift_is_recorded():
    """ORACLE_DRIFT is what profiles/landmark_slam.jsonl records (tools/landmark_slam_time.py --drift)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "landmark_slam.jsonl")
    rec = {}
    for line in open(path):
        d = json.loads(line)
        if d.get("what") == "oracle_drift":
            rec[d["kind"]] = d["relative_chi2_gap"]
    for kind in ("se2", "se3"):
        assert np.allclose(rec[kind], ORACLE_DRIFT[kind], rtol=1e-3, atol=1e-18), kind
