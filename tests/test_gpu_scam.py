"""GPU: stereo bundle adjustment over VertexSE3 on the device -- Edge_XYZ_VSC observations of VertexSBAPointXYZ points from
VertexSCam cameras (type 23 in the landmark slot beside a type-2 pose set that may hold zero edges, g2ohip_pg_set_scam_edges):
the producer against the fp64 restatement of openslam_g2o_amd/scam.py within 8 x that restatement's recorded drift against 60
digits (tests/golden/scam_edges.npz), tails, both store forms, the error-only evaluation, the assembled and reduced system and its
solution against the CPU oracle fed scam.py's arrays, robust kernels, vertex updates and the estimate stack, whole
Levenberg-Marquardt runs, the joint graph with a GICP set (type 15) on the same handle, a gauge held by a type-9 prior, an offset
set (type 19) beside it, error paths.  Tolerances of the system tests as in tests/test_gpu_landmark_camera.py."""
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm, synthetic as S
from oracle import oracle as O
from tests import landmark_helpers as LH
from tests import scam_helpers as H
from tests.helpers import dx_tolerance, relerr

pytestmark = pytest.mark.gpu

Z = np.load(H.GOLDEN)
TOL_J = 1e-12      # producers of the generated graphs: same formulas in fp64
TOL_B = 1e-11      # right-hand side
TOL_HS = 1e-12     # reduced system
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE

# Relative chi2 gap per LM iteration between two equally valid oracle runs of the graphs of the whole-run tests (the oracle's
# Schur path against the full system solved without elimination), measured on the CPU (tools/scam_ba_time.py --drift,
# profiles/scam_edges.jsonl).
ORACLE_DRIFT = {
    "scam_ba_6_120": [9.447e-16, 2.545e-15, 0.0, 1.859e-16, 1.118e-15, 7.494e-16, 1.901e-16, 9.802e-16, 4.055e-15, 2.674e-15],
    "scam_ba_6_120_gicp": [2.457e-15, 1.002e-14, 1.447e-15, 9.294e-16, 3.725e-16],
}


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _data(s, g):
    return s.edgeData(s.landmark_sets[1], g["M"], 3, 6, 3)


def _chi2_ref(g, poses, err):
    e0 = H.pose_edges(g, poses, jac=False)
    return H.SC.chi2(err, g["omega_l"]) + float(np.einsum("ni,nij,nj->n", e0, np.asarray(g["omega"]).reshape(-1, 6, 6), e0).sum())


def _within(tag, dev, ref, drift):
    """device against the restatement: 8 x the recorded drift of (err, J) -- the restatement's own figure against 60 digits."""
    fig = (np.abs(dev[2] - ref[2]).max(), max(np.abs(dev[0] - ref[0]).max(), np.abs(dev[1] - ref[1]).max()))
    print(tag, "device vs restatement (err, J)", fig, "bound", H.DRIFT_FACTOR * np.asarray(drift))
    for f, b in zip(fig, drift):
        assert f <= H.DRIFT_FACTOR * b, (tag, fig, drift)


@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_producer_tails(n):
    """1, 63, 64, 65, 255, 256, 257, 300 observations (either side of a wave and of a 256-thread block, a partial last block), both
    store forms, against the fp64 restatement; the error-only evaluation at the moved state leaves J0 / J1 bit-identical."""
    row = H.EDGE_COUNTS.index(n)
    g = H.load_graph(Z, n)
    s, graph = H.device_setup(g, schur=False)
    graph.linearize()
    ref = H.producers(H.FP64, g)
    dev = _data(s, g)
    assert dev[0].shape == (n, 18) and dev[1].shape == (n, 9) and dev[2].shape == (n, 3)
    _within("scam %d" % n, dev, ref, Z["drift"][row])
    s.buildSystem()
    c_ref = _chi2_ref(g, g["poses"], ref[2])
    print(n, "chi2", s.chi2(), c_ref)
    assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref
    # the other store form: the same bits
    s.setOption("pg_landmark_staged", 0)
    s.pgSetEstimates(g["poses"], g["hidx"])
    s.pgLinearize(True)
    direct = _data(s, g)
    for a, b in zip(dev, direct):
        assert np.array_equal(a, b)
    # an error-only evaluation after an update of cameras and points leaves J and gives the errors of the moved estimates, in
    # both store forms
    moved_err = []
    for staged in (0, 1):
        s.setOption("pg_landmark_staged", staged)
        s.pgSetEstimates(g["poses"], g["hidx"])
        s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
        s.pgLinearize(True)
        s.buildSystem()
        s.setX(Z["moved_x"])
        s.pgUpdate()
        s.pgLinearize(False)
        mp, mq = s.pgGetEstimates(), s.pgGetLandmarkEstimates()
        assert np.abs(mp - Z["moved_poses"]).max() < 1e-14 and np.abs(mq - Z["moved_points"]).max() < 1e-14
        e_ref = H.producers(H.FP64, g, mp, mq, jac=False)
        after = _data(s, g)
        assert np.array_equal(after[0], dev[0]) and np.array_equal(after[1], dev[1])
        fig = np.abs(after[2] - e_ref).max()
        print(n, "moved: device vs restatement", fig, "bound", H.DRIFT_FACTOR * Z["moved_drift"][row])
        assert fig <= H.DRIFT_FACTOR * Z["moved_drift"][row]
        assert np.abs(after[2] - dev[2]).max() > 1.0
        c_ref = _chi2_ref(g, mp, e_ref)
        assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref
        moved_err.append(after[2])
    assert np.array_equal(moved_err[0], moved_err[1])


@pytest.mark.parametrize("schur", [True, False])
@pytest.mark.parametrize("fixed_points", [0, 3])
def test_system_and_solution_against_oracle(fixed_points, schur):
    """b, chi2, Hschur (do_schur = 1) or Hpp (do_schur = 0: the pose block alone) and dx against OracleSolver fed scam.py's arrays,
    with and without fixed points, on sba_demo's graph: no pose-pose edge, two fixed cameras."""
    capi = _capi()
    g = S.make_scam_ba(6, 120, fixed_points=fixed_points)
    s, graph = H.device_setup(g, schur=schur)
    graph.linearize()
    o, _, _ = H.oracle_scam(g, schur)
    J0, J1, err = H.feed_oracle(g, o, None, None)
    dev = _data(s, g)
    figs = dict(J0=relerr(dev[0], J0), J1=relerr(dev[1], J1), err=relerr(dev[2], err))
    print("producers", figs)
    assert max(figs.values()) < TOL_J, figs
    s.buildSystem()
    o.build_system()
    print("b", relerr(s.b(), o.b()), "chi2", s.chi2(), o.chi2())
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    tol, cond = H.dx_tolerance(o, schur)
    which, name, pat =(capi.HSCHUR, "Hschur", "hs") if schur else (capi.HPP, "Hpp", None)
    fig = {name: relerr(s.values(which), o.values(name)), "dx": relerr(s.x(), o.x()), "tol": tol, "cond": cond}
    print("fixed_points", fixed_points, "schur", schur, fig)
    if schur:
        assert np.array_equal(s.pattern(capi.HSCHUR)[1], o.pattern(pat)[1])
        assert np.abs(s.x()[6 * g["nP"]:]).min() > 0              # (every free point moves)
    else:
        assert np.abs(s.x()[6 * g["nP"]:]).max() == 0             # (the pose block alone: the landmark increment stays zero)
    assert fig[name] < TOL_HS
    assert fig["dx"] < tol


@pytest.mark.parametrize("per_edge", [False, True])
def test_robust_kernel_on_the_observation_set(per_edge):
    """sba_demo's ROBUST_KERNEL: Huber on every observation, set-level and per-edge, on a graph with 5 % gross outliers."""
    capi = _capi()
    g = S.make_scam_ba(6, 120, outlier_frac=0.05, point_noise=0.02)   # (points near the truth: the inliers lie on either side of delta)
    delta = 2.0
    s, graph = H.device_setup(g, huber=0.0 if per_edge else delta)
    k1 = s.landmark_sets[1]
    if per_edge:
        s.setRobustKernelPerEdge(k1, np.full(g["M"], capi.KERNEL_HUBER, np.int32), np.full(g["M"], delta))
    graph.linearize()
    s.buildSystem()
    o, _, _ = H.oracle_scam(g, True)
    _, _, e1 = H.feed_oracle(g, o, None, None, huber=delta)
    o.build_system()
    w = np.einsum("ni,nij,nj->n", e1, g["omega_l"].reshape(g["M"], 3, 3), e1)
    assert (w > delta * delta).sum() > 0.02 * g["M"] and (w < delta * delta).sum() > 0.5 * g["M"]
    print(per_edge, "chi2", s.chi2(), o.chi2(), "b", relerr(s.b(), o.b()))
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    assert relerr(s.b(), o.b()) < TOL_B
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    tol, _ = dx_tolerance(o)
    assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < TOL_HS
    assert relerr(s.x(), o.x()) < tol


def test_update_and_estimate_stack():
    err = _capi().G2oHipError
    g = S.make_scam_ba(6, 120, fixed_points=2)
    s, graph = H.device_setup(g)
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
    poses1, points1 = H.oplus(g, g["poses"], g["points"], x)
    dpose, dpts = s.pgGetEstimates(), s.pgGetLandmarkEstimates()
    print("update", np.abs(dpose - poses1).max(), np.abs(dpts - points1).max())
    assert np.abs(dpose - poses1).max() < 1e-12 * np.abs(poses1).max()
    assert np.abs(dpts - points1).max() < 1e-12 * np.abs(points1).max()
    assert np.array_equal(dpose[:2], g["poses"][:2]) and np.array_equal(dpts[:2], g["points"][:2])   # fixed vertices stay
    assert not np.array_equal(dpose[2:], g["poses"][2:]) and not np.array_equal(dpts[2:], g["points"][2:])
    # the evaluation follows the moved estimates
    s.pgLinearize(False)
    e1 = H.producers(H.FP64, g, dpose, dpts, jac=False)
    assert relerr(_data(s, g)[2], e1) < 1e-11
    s.pgPop()
    assert np.array_equal(s.pgGetEstimates(), g["poses"]) and np.array_equal(s.pgGetLandmarkEstimates(), g["points"])
    s.pgLinearize(False)                                             # (after a pop the device evaluates at the restored estimate)
    assert relerr(_data(s, g)[2], H.producers(H.FP64, g, jac=False)) < TOL_J
    s.pgPush()
    s.pgUpdate()
    s.pgDiscardTop()
    assert np.array_equal(s.pgGetLandmarkEstimates(), dpts) and np.array_equal(s.pgGetEstimates(), dpose)
    with pytest.raises(err):
        s.pgPop()


def _drift_bound(name):
    return [max(1e-12, 10.0 * d) for d in ORACLE_DRIFT[name]]


def _lm_against_oracle(name, g, iterations):
    s, graph = H.device_setup(g)
    n_gpu, chi_gpu, lam_gpu, tr_gpu = lm.optimize(graph, s, iterations, "lm")
    r = H.oracle_lm_run(g, iterations)
    gaps = [abs(a - b) / b for a, b in zip(chi_gpu, r["chis"])]
    print(name, "lm chi2 gpu", chi_gpu)
    print(name, "lm chi2 cpu", r["chis"].tolist())
    print(name, "lm gaps", gaps, "bound", _drift_bound(name), "trials", tr_gpu, r["trials"])
    assert n_gpu == r["done"] == iterations and [int(t) for t in tr_gpu] == r["trials"]
    assert gaps[0] < 1e-12
    for it, (gap, bound) in enumerate(zip(gaps, _drift_bound(name))):
        assert gap <= bound, (it, gap, bound)
    assert chi_gpu[-1] < 0.01 * chi_gpu[0]
    return s, n_gpu, chi_gpu, lam_gpu, tr_gpu


def test_lm_run_matches_oracle():
    """Ten Levenberg-Marquardt iterations on make_scam_ba(6, 120) -- sba_demo's graph -- with everything on the device against the
    same loop over OracleSolver + scam.py: the same accepted / rejected pattern of LM trials, chi2 of iteration 0 to 1e-12 relative
    and of every later iteration within max(1e-12, ten times the gap two equally valid CPU runs show at that iteration)
    (ORACLE_DRIFT above: the largest is 4.1e-15, so the bound is 1e-12 throughout).  use_graph = 1 gives the identical trajectory."""
    g = H.lm_graph(False)
    s, n_gpu, chi_gpu, lam_gpu, tr_gpu = _lm_against_oracle("scam_ba_6_120", g, H.LM_ITERATIONS)
    s2, graph2 = H.device_setup(g, options={"use_graph": 1})
    n2, chi2, lam2, tr2 = lm.optimize(graph2, s2, H.LM_ITERATIONS, "lm")
    assert n2 == n_gpu and tr2 == tr_gpu
    assert np.array_equal(chi2, chi_gpu) and np.array_equal(lam2, lam_gpu)
    assert np.array_equal(s2.pgGetEstimates(), s.pgGetEstimates())
    assert np.array_equal(s2.pgGetLandmarkEstimates(), s.pgGetLandmarkEstimates())
    # the points end nearer the ground truth than they started (gauge: two fixed cameras); laterally -- the depth of a point 10
    # units ahead of a 0.2-unit row of cameras stays poorly determined
    e0 = np.abs(g["points"] - g["points_true"])[:, :2].max()
    e1 = np.abs(s.pgGetLandmarkEstimates() - g["points_true"])[:, :2].max()
    print("lateral point error", e0, "->", e1)
    assert e1 < 0.5 * e0, (e0, e1)


def test_joint_graph_with_gicp():
    """gicp_sba_demo's graph: the type-15 and the type-23 set on one handle.  Producers of both against their restatements, one
    solve against the oracle, five LM iterations against the oracle loop."""
    capi = _capi()
    g = H.lm_graph(True)
    s, graph = H.device_setup(g)
    assert s.gicp_set is not None and s.gicp_set != s.landmark_sets[1]
    graph.linearize()
    o, kg, _ = H.oracle_scam(g, True)
    J0, J1, err = H.feed_oracle(g, o, kg, None)
    G0, G1, eg = H.gicp_edges(g)[:3]
    dev = _data(s, g)
    dg = s.edgeData(s.gicp_set, len(g["gi"]), 3, 6, 6)
    figs = dict(J0=relerr(dev[0], J0), J1=relerr(dev[1], J1), err=relerr(dev[2], err), G0=relerr(dg[0], G0), G1=relerr(dg[1], G1),
                eg=relerr(dg[2], eg))
    print("joint producers", figs)
    assert max(figs.values()) < TOL_J, figs
    s.buildSystem()
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    tol, cond = dx_tolerance(o)
    fig = dict(Hschur=relerr(s.values(capi.HSCHUR), o.values("Hschur")), dx=relerr(s.x(), o.x()), tol=tol, cond=cond)
    print("joint solve", fig)
    assert fig["Hschur"] < TOL_HS and fig["dx"] < tol
    s.restoreDiagonal()
    _lm_against_oracle("scam_ba_6_120_gicp", g, H.JOINT_ITERATIONS)


def _prior_graph():
    """A small graph whose gauge is held by a type-9 prior on every camera: no fixed camera, no pose-pose edge."""
    g = S.make_scam_ba(4, 40, fixed=1)
    n = g["n"]
    g.update(hidx=np.arange(n, dtype=np.int32), nP=n, pt_hidx=(g["pt_hidx"] + 1).astype(np.int32), prior="pose",
             vq=np.arange(n, dtype=np.int32), zq=g["poses_true"].copy(), omega_q=np.tile((100.0 * np.eye(6)).reshape(1, 36), (n, 1)),
             prior_offset=None)
    return g


def test_gauge_held_by_a_prior_and_an_offset_set_beside():
    capi = _capi()
    g = _prior_graph()
    assert (g["hidx"] >= 0).all() and len(g["vi"]) == 0
    s, graph = H.device_setup(g)
    assert s.prior_set is not None
    graph.linearize()
    o, _, kq = H.oracle_scam(g, True)
    H.feed_oracle(g, o, None, kq)
    s.buildSystem()
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B and abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    tol, _ = dx_tolerance(o)
    assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < TOL_HS and relerr(s.x(), o.x()) < tol
    # a type-19 offset set beside the stereo set: bound and evaluated, the stereo producer unchanged
    from openslam_g2o_amd import offset_edges as OE
    g2 = S.make_scam_ba(4, 40)
    ident = np.array([[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]])
    oi, oj = np.array([0, 1, 2], np.int32), np.array([1, 2, 3], np.int32)
    omeas = np.stack([OE.se3_compose(OE.se3_invert(g2["poses_true"][a]), g2["poses_true"][b]) for a, b in zip(oi, oj)])
    g2["offset_edges"] = (19, oi, oj, np.zeros(3, np.int32), np.zeros(3, np.int32), omeas, np.tile(np.eye(6).reshape(1, 36), (3, 1)), ident)
    s2, graph2 = H.device_setup(g2)
    assert s2.offset_set is not None
    graph2.linearize()
    ref = H.producers(H.FP64, g2)
    assert max(relerr(a, b) for a, b in zip(_data(s2, g2), ref)) < TOL_J
    eo = s2.edgeData(s2.offset_set, 3, 6, 6, 6)[2]
    assert np.abs(eo).max() < 1e-12                                  # (exact relative poses, identity offsets)
    s2.buildSystem()
    c = H.SC.chi2(ref[2], g2["omega_l"])
    assert abs(s2.chi2() - c) <= 1e-12 * c


def test_error_paths():
    capi = _capi()
    L = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = S.make_scam_ba(6, 120)
    h, hl = g["hidx"], g["pt_hidx"]
    vi, vj, vp, vl = (_i32(g[k]) for k in ("vi", "vj", "vp", "vl"))
    Zp, om, zl, oml, pts, kc = (_f64(g[k]) for k in ("Z", "omega", "zl", "omega_l", "points", "kcam"))
    Zp, om = Zp.reshape(-1, 12), om.reshape(-1, 36)
    ref_err = H.producers(H.FP64, g, jac=False)

    def fresh():
        s = capi.HipBlockSolver(6, 3, 0)
        k0 = s.addEdgeSet(6, h[vi], h[vj])
        k1 = s.addEdgeSet(3, h[vp], hl[vl])
        s.buildStructure(g["nP"], g["nL"], True)
        return s, k0, k1

    def bind(s, k, a=vp, b=vl, z=zl, w=oml, kcam=kc):
        p = lambda v, f: None if v is None else f(v)
        return L.g2ohip_pg_set_scam_edges(s.h, k, p(a, _ip), p(b, _ip), p(z, _dp), p(w, _dp), p(kcam, _dp))

    def still_evaluates(s, k1):
        """the previously bound set still evaluates"""
        s.pgSetLandmarkEstimates(pts, hl)            # (same tables: only invalidates the evaluation)
        assert L.g2ohip_pg_linearize(s.h, 1) == 0
        assert relerr(s.edgeData(k1, g["M"], 3, 6, 3)[2], ref_err) < TOL_J

    s, k0, k1 = fresh()
    assert bind(s, k1) == STATE                                      # before pgSetEdges
    s.pgSetEdges(k0, 2, vi, vj, Zp, om)                              # a type-2 set of zero edges
    s.pgSetEstimates(g["poses"], h)
    assert bind(s, k0) == ARG                                        # wrong set dimensions: the pose-pose set
    assert L.g2ohip_pg_linearize(s.h, 1) == 0                        # nothing of the failed call is left: the empty pose half alone
    assert bind(s, k1) == 0
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE                    # observations bound, no landmark estimates
    s.pgSetLandmarkEstimates(pts, hl)
    still_evaluates(s, k1)
    cases = []
    for missing in ("a", "b", "z", "w", "kcam"):                     # null arrays
        cases.append({missing: None})
    for col, val in ((0, np.nan), (1, np.inf), (2, np.nan), (3, -np.inf), (4, np.nan), (0, 0.0), (1, 0.0)):   # intrinsics
        bad = kc.copy()
        bad[col] = val
        cases.append(dict(kcam=bad))
    bad = zl.copy()
    bad[17, 2] = np.nan
    cases.append(dict(z=bad))                                        # non-finite measurement
    bad = oml.copy()
    bad[5, 4] = np.inf
    cases.append(dict(w=bad))                                        # non-finite information
    for arr, key, val in ((vp, "a", -1), (vp, "a", g["n"] + 3), (vl, "b", -2), (vl, "b", g["L"] + 3)):   # negative / out of table
        bad = arr.copy()
        bad[5] = val
        cases.append({key: bad})
    bad = vp.copy()
    bad[7] = bad[7] + 1 if bad[7] + 1 < g["n"] else bad[7] - 1       # a camera whose hessian index disagrees with the set
    cases.append(dict(a=bad))
    for kw in cases:
        assert bind(s, k1, **kw) == ARG, list(kw)
        still_evaluates(s, k1)
    assert bind(s, k1, kcam=_f64([500.0, 500.0, 320.0, 240.0, 0.0])) == 0     # a zero baseline is legal (third row = first)
    s.pgSetLandmarkEstimates(pts, hl)
    s.pgLinearize(True)
    e = s.edgeData(k1, g["M"], 3, 6, 3)[2]
    assert np.array_equal(e[:, 2] + zl[:, 2], e[:, 0] + zl[:, 0])
    assert bind(s, k1) == 0
    # the other landmark entries share the slot: the Cartesian entry replaces the binding, the stereo entry takes it back
    off = _f64([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    assert L.g2ohip_pg_set_landmark_edges(s.h, k1, 4, _ip(vp), _ip(vl), _dp(zl), _dp(oml), _dp(off)) == 0
    s.pgLinearize(True)
    assert relerr(s.edgeData(k1, g["M"], 3, 6, 3)[2], LH.se3_pointxyz_edges(g["poses"], g["points"], vp, vl, zl, off, jac=False)) < TOL_J
    assert L.g2ohip_pg_set_landmark_camera_edges(s.h, k1, 23, _ip(vp), _ip(vl), _dp(zl), _dp(oml), None, _dp(kc)) == ARG
    assert L.g2ohip_pg_set_landmark_edges(s.h, k1, 23, _ip(vp), _ip(vl), _dp(zl), _dp(oml), None) == ARG
    assert bind(s, k1) == 0
    still_evaluates(s, k1)
    # a pose type other than 2
    g2 = LH.lm_test_graph("se2")
    s2 = capi.HipBlockSolver(3, 2, 0)
    q0 = s2.addEdgeSet(3, g2["hidx"][g2["vi"]], g2["hidx"][g2["vj"]])
    q1 = s2.addEdgeSet(2, g2["hidx"][g2["vp"]], g2["pt_hidx"][g2["vl"]])
    s2.buildStructure(g2["nP"], g2["nL"], True)
    s2.pgSetEdges(q0, 1, g2["vi"], g2["vj"], g2["Z"], g2["omega"])
    assert L.g2ohip_pg_set_scam_edges(s2.h, q1, _ip(_i32(g2["vp"])), _ip(_i32(g2["vl"])), _dp(_f64(g2["zl"])), _dp(_f64(g2["omega_l"])),
                                      _dp(kc)) == ARG
    assert b"EdgeSE3 pose set" in L.g2ohip_last_error()
    # while the stereo set is bound the pose-pose entry refuses other pose types
    assert L.g2ohip_pg_set_edges(s.h, k0, 12, None, None, None, None) == ARG
    still_evaluates(s, k1)
    # the binding goes with g2ohip_clear_edge_sets; rebinding afterwards
    s.clearEdgeSets()
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE
    k0 = s.addEdgeSet(6, h[vi], h[vj])
    k1 = s.addEdgeSet(3, h[vp], hl[vl])
    s.buildStructure(g["nP"], g["nL"], True)
    assert bind(s, k1) == STATE                                      # pgSetEdges first, again
    s.pgSetEdges(k0, 2, vi, vj, Zp, om)
    s.pgSetEstimates(g["poses"], h)
    assert bind(s, k1) == 0
    assert L.g2ohip_pg_linearize(s.h, 1) == STATE
    still_evaluates(s, k1)


def test_growth_of_the_structure_is_refused_and_the_binding_stays():
    """A set grown by g2ohip_update_structure would make g2ohip_pg_linearize return G2OHIP_ERR_STATE until it is bound again (the
    guard of every slot, by edge count).  Through a stereo set that state cannot be reached: like the reference, whose
    updateStructure refuses the Schur complement, g2ohip_update_structure refuses every structure that holds landmarks, with or
    without do_schur, and a type-23 set always has some.  So: the refusal, for the observation set and for the pose-pose set, and
    the binding still evaluates afterwards."""
    capi = _capi()
    L = capi.load()
    g = S.make_scam_ba(6, 120)
    m = g["M"] - 40
    part = H.take_edges(g, slice(0, m))
    h, hl = g["hidx"], g["pt_hidx"]
    for schur in (False, True):
        s, graph = H.device_setup(part, schur=schur)
        k0, k1 = s.landmark_sets
        graph.linearize()
        assert s.updateStructure(0, k1, h[g["vp"][m:]], hl[g["vl"][m:]]) is False
        assert s.updateStructure(0, k0, h[[2, 3]], h[[3, 4]]) is False
        s.pgSetLandmarkEstimates(part["points"], hl)               # (same tables: only invalidates the evaluation)
        assert L.g2ohip_pg_linearize(s.h, 1) == 0
        assert max(relerr(a, b) for a, b in zip(s.edgeData(k1, m, 3, 6, 3), H.producers(H.FP64, part))) < TOL_J


def test_profile_of_the_oracle_drift_is_recorded():
    """ORACLE_DRIFT is what profiles/scam_edges.jsonl records (tools/scam_ba_time.py --drift)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scam_edges.jsonl")
    rec = {}
    for line in open(path):
        d = json.loads(line)
        if d.get("what") == "oracle_drift":
            rec[d["graph"]] = d["relative_chi2_gap"]
    for name in ORACLE_DRIFT:
        assert np.allclose(rec[name], ORACLE_DRIFT[name], rtol=1e-3, atol=1e-18), name
