"""GPU: stereo bundle adjustment on the device -- EdgeProjectXYZ2UVU observations bound through g2ohip_ba_set_stereo_edges into
the BA front end's slot (BlockSolver_6_3, points marginalised): the producer against the NumPy restatement of
tests/stereo_helpers.py, the assembled and reduced system and its solution against the CPU oracle fed the NumPy Jacobians,
the tail shapes of both store forms, the evaluation state, robust kernels, vertex updates and the estimate stack, a whole
Levenberg-Marquardt run, error paths.  Bounds as in tests/test_gpu_landmark_camera.py."""
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm, synthetic as S
from tests import stereo_helpers as SH
from tests.helpers import dx_tolerance, relerr

pytestmark = pytest.mark.gpu

TOL_J = 1e-12      # producers: same formulas in fp64
TOL_B = 1e-11      # right-hand side
TOL_HS = 1e-12     # reduced system
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE

# Relative chi2 gap per LM iteration between two equally valid oracle runs of test_lm_run_matches_oracle's graph (the oracle's
# Schur path against the full system solved without elimination), measured on the CPU (tools/ba_stereo_time.py --drift,
# profiles/stereo_ba.jsonl).
ORACLE_DRIFT = [7.059e-15, 6.881e-14, 9.511e-15, 5.068e-15, 1.237e-14, 9.533e-15, 5.071e-15, 0.0, 1.278e-14, 4.869e-15]


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _device(g, options=None):
    """Solver with the stereo set (id 0) bound by hand: fixed points (pt_hidx) and information matrices (omega) of the problem."""
    capi = _capi()
    s = capi.HipBlockSolver(6, 3, 0)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    k = s.addEdgeSet(3, g["v0"], g["v1"])
    s.buildStructure(g["nP"], g["nL"], True)
    s.baSetStereoEdges(k, g["cam_idx"], g["pt_idx"], g["meas"], g.get("omega"), g["f"], g["cx"], g["cy"], g["baseline"])
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], SH.pt_hidx(g))
    return s


def _edge_data(s, g):
    return s.edgeData(0, g["E"], 3, 3, 6)


CASES = {
    "plain": lambda: SH.graph(),
    "fixed_points": lambda: SH.with_fixed_points(SH.graph(), 3),
    "duplicate": lambda: SH.with_duplicate(SH.graph(), 517),
    "full_information": lambda: dict(SH.graph(), omega=SH.full_information(1025)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_producers_system_and_solution_against_oracle(case):
    capi = _capi()
    g = CASES[case]()
    if case == "plain":
        s, _ = lm.setup_device_ba(g)                                 # the host layer's own set-up
    else:
        s = _device(g)
    s.baLinearize(True)
    J0, J1, err = SH.linearize(g)
    d0, d1, de = _edge_data(s, g)
    figs = dict(J0=relerr(d0, J0), J1=relerr(d1, J1), err=relerr(de, err))
    print(case, "producers", figs)
    assert max(figs.values()) < TOL_J, figs
    o = SH.oracle_stereo(g, True)
    o.set_edge_data(0, J0, J1, SH.omega(g), err)
    s.buildSystem()
    o.build_system()
    print(case, "b", relerr(s.b(), o.b()), "chi2", s.chi2(), o.chi2())
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    tol, cond = dx_tolerance(o)
    fig = dict(Hschur=relerr(s.values(capi.HSCHUR), o.values("Hschur")), dx=relerr(s.x(), o.x()), tol=tol, cond=cond)
    print(case, "solve", fig)
    assert np.array_equal(s.pattern(capi.HSCHUR)[0], o.pattern("hs")[0]) and np.array_equal(s.pattern(capi.HSCHUR)[1], o.pattern("hs")[1])
    assert fig["Hschur"] < TOL_HS
    assert fig["dx"] < tol
    s.restoreDiagonal()


@pytest.mark.parametrize("E", [100, 256, 513, 1025])
def test_tail_shapes_of_the_store_forms(E):
    """Observation counts below one block, exactly one block and 256 k + 1: the last block of the staged form holds 100, 256 or
    1 edges.  Producers and the chi2 that rides along, against NumPy, both store forms, which are bit-identical."""
    g = SH.truncated(SH.graph(), E)
    J0, J1, err = SH.linearize(g)
    chi = float((err * err).sum())
    for staged in (1, 0):
        s = _device(g, options={"ba_stereo_staged": staged})
        s.baLinearize(True)
        d0, d1, de = _edge_data(s, g)
        figs = (relerr(d0, J0), relerr(d1, J1), relerr(de, err))
        c = s.chi2()
        print(E, staged, figs, "chi2", c, chi)
        assert d0.shape[0] == E and max(figs) < TOL_J
        assert abs(c - chi) <= 1e-12 * chi
        if staged:
            first = (d0, d1, de, c)
        else:
            assert all(np.array_equal(a, b) for a, b in zip(first, (d0, d1, de, c)))
    # the option switches the form on a bound handle too
    s.setOption("ba_stereo_staged", 1)
    s.baLinearize(True)
    assert all(np.array_equal(a, b) for a, b in zip(first, _edge_data(s, g)))


def test_evaluation_state():
    """Error-only evaluation leaves the Jacobians; an evaluation without moved estimates launches nothing (the stage timers of
    g2ohip_get_stats keep what the last launch left) and the data stay."""
    g = SH.graph()
    s, _ = lm.setup_device_ba(g)
    s.setProfiling(1)
    s.baLinearize(True)
    d0, d1, de = _edge_data(s, g)
    st = s.stats()
    assert st["timeLinearize"] > 0 and st["timeResiduals"] == 0.0
    s.baLinearize(False)                                             # nothing moved: neither kind of evaluation is launched
    s.baLinearize(True)
    st2 = s.stats()
    assert st2["timeResiduals"] == 0.0 and st2["timeLinearize"] == st["timeLinearize"]
    assert all(np.array_equal(a, b) for a, b in zip((d0, d1, de), _edge_data(s, g)))
    # moved estimates, errors only: new errors, the Jacobians of before
    g2 = dict(g, pts=g["pts"] + 0.01)
    s.baSetEstimates(g2["cams"], g2["cam_hidx"], g2["pts"], SH.pt_hidx(g2))
    s.baLinearize(False)
    assert s.stats()["timeResiduals"] > 0
    with pytest.raises(_capi().G2oHipError):                          # (the Jacobians no longer belong to the estimates)
        _edge_data(s, g)
    e2 = SH.linearize(g2, jac=False)
    assert abs(s.chi2() - float((e2 * e2).sum())) <= 1e-12 * float((e2 * e2).sum())
    assert relerr(_edge_data_err(s, g), e2) < TOL_J
    s.buildSystem()                                                  # what an LM trial leaves: the old Jacobians, the new errors
    o = SH.oracle_stereo(g, True)
    J0, J1, _ = SH.linearize(g)
    o.set_edge_data(0, J0, J1, SH.omega(g), e2)
    o.build_system()
    print("b from old Jacobians and new errors", relerr(s.b(), o.b()))
    assert relerr(s.b(), o.b()) < TOL_B
    s.baLinearize(True)
    x0, x1, xe = _edge_data(s, g)
    J0, J1, _ = SH.linearize(g2)
    assert relerr(xe, e2) < TOL_J and relerr(x0, J0) < TOL_J and relerr(x1, J1) < TOL_J
    assert not np.array_equal(x0, d0)


@pytest.mark.parametrize("per_edge", [False, True])
def test_robust_kernel(per_edge):
    capi = _capi()
    g = SH.graph(outlier_frac=0.05)
    delta = 30.0                                                     # (pixels: a third of the errors at the initial estimates lie above it)
    s, graph = lm.setup_device_ba(g, huber_delta=0.0 if per_edge else delta)
    if per_edge:
        s.setRobustKernelPerEdge(0, np.full(g["E"], capi.KERNEL_HUBER, np.int32), np.full(g["E"], delta))
    graph.linearize()
    s.buildSystem()
    J0, J1, err = SH.linearize(g)
    w = (err * err).sum(axis=1)
    assert 0.02 * g["E"] < (w > delta * delta).sum() < 0.98 * g["E"]   # the kernel is active on some edges and not on others
    o = SH.oracle_stereo(g, True)
    o.set_edge_data(0, J0, J1, SH.omega(g), err, delta)
    o.build_system()
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
    s.restoreDiagonal()
    # the chi2 that rides along with an error-only evaluation is the robustified one
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], SH.pt_hidx(g))
    graph.compute_active_errors()
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    rho = np.where(w <= delta * delta, w, 2 * np.sqrt(w) * delta - delta * delta).sum()
    assert abs(s.chi2() - rho) <= 1e-12 * rho


def test_update_and_estimate_stack():
    err = _capi().G2oHipError
    g = SH.graph()
    s, graph = lm.setup_device_ba(g)
    graph.linearize()
    s.buildSystem()
    s.setLambda(1e-3 * s.maxDiagonal(), True)
    assert s.solve()
    s.restoreDiagonal()
    x = s.x()
    cams0, pts0 = s.baGetEstimates()
    assert np.array_equal(cams0, g["cams"]) and np.array_equal(pts0, g["pts"])
    s.baPush()
    with pytest.raises(err):
        s.baPush()                                                   # one level
    s.baUpdate()
    g1 = S.ba_oplus(g, x)
    cams1, pts1 = s.baGetEstimates()
    print("update", np.abs(cams1 - g1["cams"]).max(), np.abs(pts1 - g1["pts"]).max())
    assert np.abs(cams1 - g1["cams"]).max() < 1e-12 * np.abs(g1["cams"]).max()
    assert np.abs(pts1 - g1["pts"]).max() < 1e-12 * np.abs(g1["pts"]).max()
    assert np.array_equal(cams1[:2], g["cams"][:2]) and not np.array_equal(cams1[2:], g["cams"][2:])   # fixed cameras stay
    # the evaluation follows the moved estimates
    s.baLinearize(False)
    assert relerr(_edge_data_err(s, g), SH.linearize(g1, jac=False)) < 1e-11
    s.baPop()
    cams2, pts2 = s.baGetEstimates()
    assert np.array_equal(cams2, g["cams"]) and np.array_equal(pts2, g["pts"])
    s.baPush()
    s.baUpdate()
    s.baDiscardTop()
    cams3, pts3 = s.baGetEstimates()
    assert np.array_equal(cams3, cams1) and np.array_equal(pts3, pts1)
    with pytest.raises(err):
        s.baPop()
    assert np.array_equal(s.baGetEstimatesOf([3], [7])[1][0], pts1[7])


def _edge_data_err(s, g):
    """The errors alone (after an error-only evaluation copy_edge_data refuses the Jacobians)."""
    capi = _capi()
    e = np.empty((g["E"], 3))
    rc = s.L.g2ohip_copy_edge_data(s.h, 0, None, None, capi._dp(e))
    assert rc == 0, rc
    return e


def _drift_bound():
    return [max(1e-12, 10.0 * d) for d in ORACLE_DRIFT]


def test_lm_run_matches_oracle():
    """Ten Levenberg-Marquardt iterations with everything on the device against the same loop over OracleSolver + the NumPy
    producers: the same accepted / rejected pattern of LM trials, chi2 of iteration 0 to 1e-12 relative and of every later
    iteration within max(1e-12, ten times the gap two equally valid CPU runs show at that iteration) (ORACLE_DRIFT above; the
    largest is 6.9e-14, so the bound is 1e-12 throughout).  use_graph = 1 gives the identical trajectory."""
    g = SH.lm_test_graph()
    s, graph = lm.setup_device_ba(g)
    n_gpu, chi_gpu, lam_gpu, tr_gpu = lm.optimize(graph, s, 10, "lm")
    n_cpu, chi_cpu, lam_cpu, tr_cpu, og = SH.oracle_lm_run(g, 10)
    gaps = [abs(a - b) / b for a, b in zip(chi_gpu, chi_cpu)]
    print("lm chi2 gpu", chi_gpu)
    print("lm chi2 cpu", chi_cpu)
    print("lm gaps", gaps, "bound", _drift_bound(), "trials", tr_gpu, tr_cpu)
    assert n_gpu == n_cpu == 10 and tr_gpu == tr_cpu
    assert gaps[0] < 1e-12
    for it, (gap, bound) in enumerate(zip(gaps, _drift_bound())):
        assert gap <= bound, (it, gap, bound)
    e = SH.linearize(g, jac=False)
    assert chi_gpu[-1] < 0.01 * float((e * e).sum())
    s2, graph2 = lm.setup_device_ba(g, options={"use_graph": 1})
    n2, chi2, lam2, tr2 = lm.optimize(graph2, s2, 10, "lm")
    assert n2 == n_gpu and tr2 == tr_gpu
    assert np.array_equal(chi2, chi_gpu) and np.array_equal(lam2, lam_gpu)
    a, b = s.baGetEstimates(), s2.baGetEstimates()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.abs(a[1] - g["pts"]).max() > 0.05                      # the points have moved


def test_error_paths():
    capi = _capi()
    L = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = SH.graph()
    E = g["E"]
    cv, pv, z = _i32(g["cam_idx"]), _i32(g["pt_idx"]), _f64(g["meas"])
    z2 = _f64(g["meas"][:, :2])
    f, cx, cy, b = g["f"], g["cx"], g["cy"], g["baseline"]
    ref = SH.linearize(g)

    def stereo(s, k, a=cv, q=pv, m=z, ff=f, bb=b):
        return L.g2ohip_ba_set_stereo_edges(s.h, k, None if a is None else _ip(a), _ip(q), None if m is None else _dp(m), None, ff, cx, cy, bb)

    def still_works(s):
        s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], SH.pt_hidx(g))      # (same tables: only invalidates the evaluation)
        s.baLinearize(True)
        assert all(relerr(a, r) < TOL_J for a, r in zip(_edge_data(s, g), ref))

    s = capi.HipBlockSolver(6, 3, 0)
    k = s.addEdgeSet(3, g["v0"], g["v1"])
    assert stereo(s, k) == STATE                                     # before buildStructure
    s.buildStructure(g["nP"], g["nL"], True)
    assert L.g2ohip_ba_linearize(s.h, 1) == STATE                    # nothing bound
    assert stereo(s, k) == 0
    assert L.g2ohip_ba_linearize(s.h, 1) == STATE                    # bound, no estimates
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], SH.pt_hidx(g))
    still_works(s)
    assert L.g2ohip_ba_set_edges(s.h, k, _ip(cv), _ip(pv), _dp(z2), None, f, cx, cy) == ARG      # a d = 3 set handed to the mono entry
    assert L.g2ohip_ba_set_edges_classes(s.h, k, _ip(cv), _ip(pv), _dp(z2), None, 1, _dp(_f64(np.array([f, cx, cy, 0.0, 1.0]))), None) == ARG
    assert stereo(s, k + 1) == ARG and stereo(s, -1) == ARG          # no such set
    assert stereo(s, k, a=None) == ARG and stereo(s, k, m=None) == ARG
    for bad_b in (np.inf, -np.inf, np.nan):
        assert stereo(s, k, bb=bad_b) == ARG
    assert stereo(s, k, ff=0.0) == ARG and stereo(s, k, ff=np.nan) == ARG
    bad = cv.copy()
    bad[5] = g["P"] + 3                                              # out of range
    assert stereo(s, k, a=bad) == ARG
    bad = pv.copy()
    bad[E - 1] = -1
    assert stereo(s, k, q=bad) == ARG
    bad = cv.copy()
    bad[7] = bad[7] + 1                                              # a camera whose hessian index disagrees with the set
    assert stereo(s, k, a=bad) == ARG
    bad = pv.copy()
    bad[300] = bad[300] + 1 if bad[300] + 1 < g["L"] else bad[300] - 1
    assert stereo(s, k, q=bad) == ARG
    still_works(s)                                                   # every rejected call left the binding as it was
    # new tables validate the bound stereo set again
    h = g["cam_hidx"].copy()
    h[2], h[3] = h[3], h[2]
    assert L.g2ohip_ba_set_estimates(s.h, g["P"], _dp(_f64(g["cams"])), _ip(_i32(h)), g["L"], _dp(_f64(g["pts"])), _ip(SH.pt_hidx(g))) == ARG
    still_works(s)
    # per-edge kernels: refused at the binding (the mono rule), taken by the bound set
    s.setRobustKernelPerEdge(k, np.zeros(E, np.int32), np.ones(E))
    still_works(s)
    assert stereo(s, k) == STATE
    s.setRobustKernelPerEdge(k, None, None)
    assert stereo(s, k) == 0
    still_works(s)
    # a d = 2 set handed to the stereo entry
    m, _ = lm.setup_device_ba(S.make_ba_problem(*SH.GRAPH))
    assert stereo(m, 0) == ARG
    m.baLinearize(True)                                              # the mono binding is untouched
    assert abs(m.chi2() - float((S.ba_linearize(S.make_ba_problem(*SH.GRAPH), jac=False) ** 2).sum())) <= 1e-12 * m.chi2()
    # the binding goes with clearEdgeSets and comes back
    s.clearEdgeSets()
    assert L.g2ohip_ba_linearize(s.h, 1) == STATE
    k = s.addEdgeSet(3, g["v0"], g["v1"])
    s.buildStructure(g["nP"], g["nL"], True)
    assert stereo(s, k) == 0
    still_works(s)
    # growth by update_structure is refused with marginalised points, as for every Schur structure
    assert L.g2ohip_update_structure(s.h, 0, k, 0, None, None) == capi.ERR_UNSUPPORTED


def test_rebinding_the_slot_mono_stereo_mono():
    """One handle with a d = 2 and a d = 3 set over the same vertices (the set that is not bound is fed zeros through
    setEdgeData: it contributes nothing): mono -> stereo -> mono, each result equal to a fresh handle's."""
    capi = _capi()
    gs = SH.graph()
    gm = dict(gs, meas=gs["meas"][:, :2])
    E = gs["E"]

    def handle():
        s = capi.HipBlockSolver(6, 3, 0)
        ka = s.addEdgeSet(2, gs["v0"], gs["v1"])
        kb = s.addEdgeSet(3, gs["v0"], gs["v1"])
        s.buildStructure(gs["nP"], gs["nL"], True)
        s.baSetEstimates(gs["cams"], gs["cam_hidx"], gs["pts"], SH.pt_hidx(gs))
        return s, ka, kb

    def idle(s, k, d):
        s.setEdgeData(k, np.zeros((E, d * 3)), np.zeros((E, d * 6)), np.tile(np.eye(d).reshape(-1), (E, 1)), np.zeros((E, d)))

    def mono(s, ka, kb):
        s.baSetEdges(ka, gm["cam_idx"], gm["pt_idx"], gm["meas"], None, gm["f"], gm["cx"], gm["cy"])
        idle(s, kb, 3)
        return run(s)

    def stereo(s, ka, kb):
        s.baSetStereoEdges(kb, gs["cam_idx"], gs["pt_idx"], gs["meas"], None, gs["f"], gs["cx"], gs["cy"], gs["baseline"])
        idle(s, ka, 2)
        return run(s)

    def run(s):
        s.baLinearize(True)
        c = s.chi2()
        s.buildSystem()
        bb = s.b()
        s.setLambda(10.0, True)
        assert s.solve()
        s.restoreDiagonal()
        return c, bb, s.x()

    s, ka, kb = handle()
    r1, r2, r3 = mono(s, ka, kb), stereo(s, ka, kb), mono(s, ka, kb)
    f1, f2 = mono(*handle()), stereo(*handle())
    for got, want, name in ((r1, f1, "mono"), (r2, f2, "stereo after mono"), (r3, f1, "mono after stereo")):
        for a, b in zip(got, want):
            assert np.array_equal(a, b), name
    assert not np.array_equal(r1[2], r2[2])
    # and the stereo result is the one of the handle that has the stereo set alone
    s1 = _device(gs)
    s1.baLinearize(True)
    assert abs(s1.chi2() - r2[0]) <= 1e-12 * r2[0]


def test_profile_of_the_oracle_drift_is_recorded():
    """ORACLE_DRIFT is what profiles/stereo_ba.jsonl records (tools/ba_stereo_time.py --drift)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stereo_ba.jsonl")
    rec = None
    for line in open(path):
        d = json.loads(line)
        if d.get("what") == "oracle_drift":
            rec = d["relative_chi2_gap"]
    assert rec is not None and np.allclose(rec, ORACLE_DRIFT, rtol=1e-3, atol=1e-18)
