"""GPU: RGB-D / stereo landmark SLAM on the device -- EdgeSE3 odometry plus EdgeSE3PointXYZDepth / EdgeSE3PointXYZDisparity
observations of one camera (ParameterCamera: offset + Kcam) bound through g2ohip_pg_set_landmark_camera_edges, landmarks
marginalised (BlockSolver_6_3): producers against the NumPy restatement of tests/landmark_camera_helpers.py, the assembled and
reduced system and its solution against the CPU oracle fed the NumPy Jacobians, the tail shapes of both store forms, robust
kernels, vertex updates and the estimate stack, whole Levenberg-Marquardt runs, error paths.  Bounds as in
tests/test_gpu_landmark_slam.py."""
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm
from oracle import oracle as O
from tests import landmark_camera_helpers as CH
from tests import landmark_helpers as LH
from tests.helpers import dx_tolerance, relerr

pytestmark = pytest.mark.gpu

TOL_J = 1e-12      # producers: same formulas in fp64
TOL_B = 1e-11      # right-hand side
TOL_HS = 1e-12     # reduced system
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE
KINDS = ["depth", "disparity"]

# Relative chi2 gap per LM iteration between two equally valid oracle runs of test_lm_run_matches_oracle's graphs (the
# oracle's Schur path against the full system solved without elimination), measured on the CPU
# (tools/landmark_slam_time.py --drift --kinds depth,disparity, profiles/landmark_camera.jsonl).
ORACLE_DRIFT = {
    "depth": [7.893e-15, 9.926e-14, 1.984e-13, 4.439e-13, 2.152e-13, 3.281e-15, 2.940e-15, 5.191e-16, 1.367e-14, 1.731e-15],
    "disparity": [2.392e-15, 2.225e-15, 2.414e-15, 2.257e-13, 6.563e-15, 0.0, 1.205e-15, 1.895e-15, 8.445e-15, 1.724e-14],
}


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _feed_oracle(g, o, huber=0.0):
    A0, A1, e0 = LH.pose_edges(g)
    B0, B1, e1 = CH.landmark_edges(g)
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    o.set_edge_data(1, B0, B1, g["omega_l"], e1, huber)
    return (A0, A1, e0), (B0, B1, e1)


@pytest.mark.parametrize("obs,fixed_landmarks", [("depth", 3), ("disparity", 0), ("disparity", 3)])
def test_producers_system_and_solution_against_oracle(obs, fixed_landmarks):
    capi = _capi()
    g = CH.graph(obs, fixed_landmarks=fixed_landmarks)
    s, graph = lm.setup_device_landmark_slam(g)
    k0, k1 = s.landmark_sets
    graph.linearize()
    o = LH.oracle_landmark(g, True)
    (A0, A1, e0), (B0, B1, e1) = _feed_oracle(g, o)
    dA0, dA1, de0 = s.edgeData(k0, g["E"], 6, 6, 6)
    dB0, dB1, de1 = s.edgeData(k1, g["M"], 3, 6, 3)
    figs = dict(J0_pose=relerr(dA0, A0), J1_pose=relerr(dA1, A1), err_pose=relerr(de0, e0), J0_lm=relerr(dB0, B0),
                J1_lm=relerr(dB1, B1), err_lm=relerr(de1, e1))
    print(obs, "producers", figs)
    assert max(figs.values()) < TOL_J, figs
    s.buildSystem()
    o.build_system()
    print(obs, "b", relerr(s.b(), o.b()), "chi2", s.chi2(), o.chi2())
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    tol, cond = dx_tolerance(o)
    fig = dict(Hschur=relerr(s.values(capi.HSCHUR), o.values("Hschur")), dx=relerr(s.x(), o.x()), tol=tol, cond=cond)
    print(obs, "solve", fig)
    assert np.array_equal(s.pattern(capi.HSCHUR)[1], o.pattern("hs")[1])
    assert fig["Hschur"] < TOL_HS
    assert fig["dx"] < tol
    s.restoreDiagonal()
    # error-only evaluation leaves the Jacobians and gives the same errors
    s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])            # (same tables: only invalidates the evaluation)
    s.pgLinearize(False)
    xB0, xB1, xe1 = s.edgeData(k1, g["M"], 3, 6, 3)
    assert np.array_equal(xB0, dB0) and np.array_equal(xB1, dB1) and relerr(xe1, e1) < TOL_J
    # both store forms write the same numbers
    s.setOption("pg_landmark_staged", 0)
    s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
    s.pgLinearize(True)
    xB0, xB1, xe1 = s.edgeData(k1, g["M"], 3, 6, 3)
    assert np.array_equal(xB0, dB0) and np.array_equal(xB1, dB1) and np.array_equal(xe1, de1)
    s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
    s.pgLinearize(False)
    assert np.array_equal(s.edgeData(k1, g["M"], 3, 6, 3)[2], de1)


def _truncated(g, M):
    """The first M observations of g; landmarks that lose all their observations are fixed and leave the structure."""
    t = dict(g)
    t["vp"], t["vl"], t["zl"], t["omega_l"], t["M"] = g["vp"][:M], g["vl"][:M], g["zl"][:M], g["omega_l"][:M], M
    seen = np.bincount(t["vl"], minlength=g["L"]) > 0
    t["nL"] = int(seen.sum())
    t["pt_hidx"] = np.where(seen, g["nP"] + np.cumsum(seen) - 1, -1).astype(np.int32)
    return t


@pytest.mark.parametrize("obs", KINDS)
@pytest.mark.parametrize("M", [100, 256, 513, 1025])
def test_tail_shapes_of_the_store_forms(obs, M):
    """Observation counts below one block, exactly one block and 256 k + 1: the last block of the staged form holds 100,
    256 or 1 edges.  Producers only, against NumPy, both store forms."""
    g = _truncated(CH.graph(obs), M)
    B0, B1, e1 = CH.landmark_edges(g)
    for staged in (1, 0):
        s, graph = lm.setup_device_landmark_slam(g, options={"pg_landmark_staged": staged})
        graph.linearize()
        dB0, dB1, de1 = s.edgeData(s.landmark_sets[1], M, 3, 6, 3)
        figs = (relerr(dB0, B0), relerr(dB1, B1), relerr(de1, e1))
        print(obs, M, staged, figs)
        assert dB0.shape[0] == M and max(figs) < TOL_J
        if staged:
            first = (dB0, dB1, de1)
        else:
            assert all(np.array_equal(a, b) for a, b in zip(first, (dB0, dB1, de1)))


@pytest.mark.parametrize("obs", KINDS)
@pytest.mark.parametrize("per_edge", [False, True])
def test_robust_kernel_on_the_observation_set(obs, per_edge):
    capi = _capi()
    g = CH.graph(obs, outlier_frac=0.05)
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
    w = np.einsum("ni,nij,nj->n", e1, g["omega_l"].reshape(g["M"], 3, 3), e1)
    assert (w > delta * delta).sum() > 0.02 * g["M"]
    print(obs, per_edge, "chi2", s.chi2(), o.chi2(), "b", relerr(s.b(), o.b()))
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    assert relerr(s.b(), o.b()) < TOL_B
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    tol, _ = dx_tolerance(o)
    assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < TOL_HS
    assert relerr(s.x(), o.x()) < tol


@pytest.mark.parametrize("obs", KINDS)
def test_update_and_estimate_stack(obs):
    err = _capi().G2oHipError
    g = CH.graph(obs, fixed_landmarks=2)
    s, graph = lm.setup_device_landmark_slam(g)
    graph.linearize()
    s.buildSystem()
    s.setLambda(1e-3 * s.maxDiagonal(), True)
    assert s.solve()
    s.restoreDiagonal()
    x = s.x()
    assert np.abs(x[6 * g["nP"]:]).max() > 0
    assert np.array_equal(s.pgGetEstimates(), g["poses"]) and np.array_equal(s.pgGetLandmarkEstimates(), g["points"])
    s.pgPush()
    with pytest.raises(err):
        s.pgPush()                                                   # one level
    s.pgUpdate()
    poses1 = O.se3_oplus(g["poses"], g["hidx"], x)
    points1 = LH.points_oplus(g["points"], g["pt_hidx"], x, 6 * g["nP"], g["nP"])
    dpose, dpts = s.pgGetEstimates(), s.pgGetLandmarkEstimates()
    print(obs, "update", np.abs(dpose - poses1).max(), np.abs(dpts - points1).max())
    assert np.abs(dpose - poses1).max() < 1e-12 * np.abs(poses1).max()
    assert np.abs(dpts - points1).max() < 1e-12 * np.abs(points1).max()
    assert np.array_equal(dpose[0], g["poses"][0]) and np.array_equal(dpts[:2], g["points"][:2])   # fixed vertices stay
    assert not np.array_equal(dpts[2:], g["points"][2:])
    # the evaluation follows the moved estimates
    s.pgLinearize(False)
    e1 = CH.landmark_edges(g, poses=poses1, points=points1, jac=False)
    assert relerr(s.edgeData(s.landmark_sets[1], g["M"], 3, 6, 3)[2], e1) < 1e-11
    s.pgPop()
    assert np.array_equal(s.pgGetEstimates(), g["poses"]) and np.array_equal(s.pgGetLandmarkEstimates(), g["points"])
    s.pgPush()
    s.pgUpdate()
    s.pgDiscardTop()
    assert np.array_equal(s.pgGetLandmarkEstimates(), dpts)
    with pytest.raises(err):
        s.pgPop()


def _drift_bound(obs):
    return [max(1e-12, 10.0 * d) for d in ORACLE_DRIFT[obs]]


@pytest.mark.parametrize("obs", KINDS)
def test_lm_run_matches_oracle(obs):
    """Ten Levenberg-Marquardt iterations with everything on the device against the same loop over OracleSolver + the NumPy
    producers: the same accepted / rejected pattern of LM trials, chi2 of iteration 0 to 1e-12 relative and of every later
    iteration within max(1e-12, ten times the gap two equally valid CPU runs show at that iteration) (ORACLE_DRIFT above;
    the largest is 4.4e-13, so the bound is 1e-12 except 2.0e-12, 4.4e-12 and 2.2e-12 at iterations 2-4 of the depth run
    and 2.3e-12 at iteration 3 of the disparity run).  use_graph = 1 gives the identical trajectory."""
    g = CH.lm_test_graph(obs)
    s, graph = lm.setup_device_landmark_slam(g)
    n_gpu, chi_gpu, lam_gpu, tr_gpu = lm.optimize(graph, s, 10, "lm")
    n_cpu, chi_cpu, lam_cpu, tr_cpu, og = CH.oracle_lm_run(g, 10)
    gaps = [abs(a - b) / b for a, b in zip(chi_gpu, chi_cpu)]
    print(obs, "lm chi2 gpu", chi_gpu)
    print(obs, "lm chi2 cpu", chi_cpu)
    print(obs, "lm gaps", gaps, "bound", _drift_bound(obs), "trials", tr_gpu, tr_cpu)
    assert n_gpu == n_cpu == 10 and tr_gpu == tr_cpu
    assert gaps[0] < 1e-12
    for it, (gap, bound) in enumerate(zip(gaps, _drift_bound(obs))):
        assert gap <= bound, (it, gap, bound)
    assert chi_gpu[-1] < 0.01 * chi_gpu[0]
    s2, graph2 = lm.setup_device_landmark_slam(g, options={"use_graph": 1})
    n2, chi2, lam2, tr2 = lm.optimize(graph2, s2, 10, "lm")
    assert n2 == n_gpu and tr2 == tr_gpu
    assert np.array_equal(chi2, chi_gpu) and np.array_equal(lam2, lam_gpu)
    assert np.array_equal(s2.pgGetEstimates(), s.pgGetEstimates())
    assert np.array_equal(s2.pgGetLandmarkEstimates(), s.pgGetLandmarkEstimates())
    # the landmarks end nearer the ground truth than they started (gauge: pose 0)
    e0 = np.abs(g["points"] - g["points_true"]).max()
    e1 = np.abs(s.pgGetLandmarkEstimates() - g["points_true"]).max()
    print(obs, "landmark error", e0, "->", e1)
    assert e1 < e0, (e0, e1)


@pytest.mark.parametrize("obs", KINDS)
def test_error_paths(obs):
    capi = _capi()
    L = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    typ = 5 if obs == "depth" else 6
    g = CH.graph(obs)
    h, hl = g["hidx"], g["pt_hidx"]
    vi, vj, vp, vl = (_i32(g[k]) for k in ("vi", "vj", "vp", "vl"))
    Z, om, zl, oml, pts, off, kc = (_f64(g[k]) for k in ("Z", "omega", "zl", "omega_l", "points", "offset", "kcam"))

    def fresh():
        s = capi.HipBlockSolver(6, 3, 0)
        k0 = s.addEdgeSet(6, h[vi], h[vj])
        k1 = s.addEdgeSet(3, h[vp], hl[vl])
        s.buildStructure(g["nP"], g["nL"], True)
        return s, k0, k1

    def set_cam(s, k, t, a=vp, b=vl, kcam=kc, offset=off):
        return L.g2ohip_pg_set_landmark_camera_edges(s.h, k, t, _ip(a), _ip(b), _dp(zl), _dp(oml), None if offset is None else _dp(offset),
                                                     None if kcam is None else _dp(kcam))

    def set_lm(s, k, t):
        return L.g2ohip_pg_set_landmark_edges(s.h, k, t, _ip(vp), _ip(vl), _dp(zl), _dp(oml), _dp(off))

    s, k0, k1 = fresh()
    assert set_cam(s, k1, typ) == STATE                              # before pgSetEdges
    s.pgSetEdges(k0, 2, vi, vj, Z, om)
    s.pgSetEstimates(g["poses"], h)
    for t in (3, 4, 7):
        assert set_cam(s, k1, t) == ARG                              # the Cartesian types and an unknown one
    for t in (5, 6):
        assert set_lm(s, k1, t) == ARG                               # the camera types through the Cartesian entry
    assert set_cam(s, k0, typ) == ARG                                # the pose-pose set as observation set
    assert set_cam(s, k1, typ, kcam=None) == ARG
    for bad_k in ([0.0, 500, 1, 1], [500, 0.0, 1, 1], [np.inf, 500, 1, 1], [500, 500, np.nan, 1]):
        assert set_cam(s, k1, typ, kcam=_f64(np.array(bad_k, np.float64))) == ARG
    assert L.g2ohip_pg_set_landmark_camera_edges(s.h, k1, typ, _ip(vp), None, _dp(zl), _dp(oml), None, _dp(kc)) == ARG
    bad = vp.copy()
    bad[7] = bad[7] + 1 if bad[7] + 1 < g["n"] else bad[7] - 1       # a pose whose hessian index disagrees with the set
    assert set_cam(s, k1, typ, a=bad) == ARG
    bad = vp.copy()
    bad[5] = g["n"] + 3                                              # out of range
    assert set_cam(s, k1, typ, a=bad) == ARG
    assert L.g2ohip_pg_linearize(s.h, 1) == 0                        # nothing of the failed calls is left: pose half alone
    assert set_cam(s, k1, typ) == 0
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE                    # observations bound, no landmark estimates
    bad = vl.copy()
    bad[5] = g["L"] + 3
    assert set_cam(s, k1, typ, b=bad) == 0                           # (the landmark table is not known yet ...)
    assert L.g2ohip_pg_set_landmark_estimates(s.h, g["L"], _dp(pts), _ip(_i32(hl))) == ARG   # ... now it is
    assert set_cam(s, k1, typ, offset=None) == 0                     # NULL offset: identity
    s.pgSetLandmarkEstimates(pts, hl)
    assert set_cam(s, k1, typ, b=bad) == ARG                         # rejected: the good binding stays
    s.pgLinearize(True)
    e_id = CH.landmark_edges(dict(g, offset=None), jac=False)
    assert relerr(s.edgeData(k1, g["M"], 3, 6, 3)[2], e_id) < TOL_J
    # beside a type-1 pose set
    g2 = LH.lm_test_graph("se2")
    s2 = capi.HipBlockSolver(3, 2, 0)
    q0 = s2.addEdgeSet(3, g2["hidx"][g2["vi"]], g2["hidx"][g2["vj"]])
    q1 = s2.addEdgeSet(2, g2["hidx"][g2["vp"]], g2["pt_hidx"][g2["vl"]])
    s2.buildStructure(g2["nP"], g2["nL"], True)
    s2.pgSetEdges(q0, 1, g2["vi"], g2["vj"], g2["Z"], g2["omega"])
    rc = L.g2ohip_pg_set_landmark_camera_edges(s2.h, q1, typ, _ip(_i32(g2["vp"])), _ip(_i32(g2["vl"])), _dp(_f64(g2["zl"])),
                                               _dp(_f64(g2["omega_l"])), None, _dp(kc))
    assert rc == ARG
    # the binding goes with g2ohip_clear_edge_sets; rebinding afterwards
    s.clearEdgeSets()
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE
    k0 = s.addEdgeSet(6, h[vi], h[vj])
    k1 = s.addEdgeSet(3, h[vp], hl[vl])
    s.buildStructure(g["nP"], g["nL"], True)
    assert set_cam(s, k1, typ) == STATE                              # pgSetEdges first, again
    s.pgSetEdges(k0, 2, vi, vj, Z, om)
    s.pgSetEstimates(g["poses"], h)
    assert set_cam(s, k1, typ) == 0
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE
    s.pgSetLandmarkEstimates(pts, hl)
    assert L.g2ohip_pg_linearize(s.h, 1) == 0
    assert relerr(s.edgeData(k1, g["M"], 3, 6, 3)[2], CH.landmark_edges(g, jac=False)) < TOL_J
    # the Cartesian entry replaces the binding of the one slot, and the camera entry takes it back
    assert set_lm(s, k1, 4) == 0
    s.pgLinearize(True)
    assert relerr(s.edgeData(k1, g["M"], 3, 6, 3)[2], LH.se3_pointxyz_edges(g["poses"], g["points"], vp, vl, zl, off, jac=False)) < TOL_J
    assert set_cam(s, k1, typ) == 0
    s.pgLinearize(True)
    assert relerr(s.edgeData(k1, g["M"], 3, 6, 3)[2], CH.landmark_edges(g, jac=False)) < TOL_J


def test_profile_of_the_oracle_drift_is_recorded():
    """ORACLE_DRIFT is what profiles/landmark_camera.jsonl records (tools/landmark_slam_time.py --drift)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "landmark_camera.jsonl")
    rec = {}
    for line in open(path):
        d = json.loads(line)
        if d.get("what") == "oracle_drift":
            rec[d["kind"]] = d["relative_chi2_gap"]
    for obs in KINDS:
        assert np.allclose(rec[obs], ORACLE_DRIFT[obs], rtol=1e-3, atol=1e-18), obs
