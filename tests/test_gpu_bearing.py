"""GPU: bearing-only observations of 2-D point landmarks on the device (EdgeSE2PointXYBearing = type 20 beside an EdgeSE2 set, with
or without an EdgeSE2PointXY set over the same landmark table, g2ohip_pg_set_bearing_edges): the producer against the fp64
restatement of openslam_g2o_amd/bearing.py within 8 x that restatement's recorded drift against 60 digits
(tests/golden/bearing_edges.npz), tails, both store forms, the error-only evaluation, the assembled system and its solution against
the CPU oracle with the landmarks marginalised (error dimension 1 on the landmark side of the Schur path) and without, robust
kernels, a Levenberg-Marquardt run against the host-fed one, the binding rules, the prior and offset slots beside it, a graph
from a file."""
import os

import numpy as np
import pytest

from openslam_g2o_amd import bearing as BE, g2o_io, lm, synthetic as S
from oracle import oracle as O
from tests import bearing_helpers as H
from tests import landmark_helpers as LH
from tests import offset_helpers as OH
from tests import prior_helpers as PH
from tests import producer_metric as PM
from tests.helpers import relerr

pytestmark = pytest.mark.gpu

Z = np.load(H.GOLDEN)
TOL_B = 1e-11       # right-hand side, as tests/test_gpu_offset_edges.py
TOL_H = 1e-12       # assembled blocks
TOL_X = 1e-8        # solution
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _data(s, g, n=None):
    return s.edgeData(s.bearing_set, len(g["bp"]) if n is None else n, 1, 3, 2)


def _chi2_ref(g, poses, points, err, huber=0.0):
    e0 = H.pose_edges(g, poses, jac=False)
    c = BE.chi2(err, g["omega_b"], huber) + float(np.einsum("ni,nij,nj->n", e0, np.asarray(g["omega"]).reshape(-1, 3, 3), e0).sum())
    if len(g["vp"]):
        e1 = H.xy_edges(g, poses, points, jac=False)
        c += float(np.einsum("ni,nij,nj->n", e1, np.asarray(g["omega_l"]).reshape(-1, 2, 2), e1).sum())
    return c


def _within(tag, dev, ref, drift):
    """device against the restatement: 8 x the recorded drift of (err, J), itself below the per-row ceiling of producer_metric."""
    fig = (np.abs(dev[2] - ref[2]).max(), max(np.abs(dev[0] - ref[0]).max(), np.abs(dev[1] - ref[1]).max()))
    ones = np.ones((len(ref[2]), 1))
    rows = (PM.worst_row(dev[2], ref[2], ones, 1)[0], max(PM.worst_row(dev[0], ref[0], ones, 1)[0], PM.worst_row(dev[1], ref[1], ones, 1)[0]))
    print(tag, "device vs restatement (err, J)", fig, "bound", H.DRIFT_FACTOR * np.asarray(drift), "per-row figure", rows)
    for f, b, r in zip(fig, drift, rows):
        assert H.DRIFT_FACTOR * b <= PM.CEILING
        assert f <= H.DRIFT_FACTOR * b, (tag, fig, drift)
        assert r <= PM.CEILING


@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_producer_tails(n):
    row = H.EDGE_COUNTS.index(n)
    g = H.load_graph(Z, n)
    s, graph = H.device_setup(g, schur=False)
    graph.linearize()
    ref = H.producers(H.FP64, g)
    dev = _data(s, g)
    _within("bearing %d" % n, dev, ref, Z["drift"][row])
    s.buildSystem()
    c_ref = _chi2_ref(g, g["poses"], g["points"], ref[2])
    print(n, "chi2", s.chi2(), c_ref)
    assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref
    # the other store form: the same bits
    s.setOption("pg_landmark_staged", 0)
    s.pgSetEstimates(g["poses"], g["hidx"])
    s.pgLinearize(True)
    direct = _data(s, g)
    for a, b in zip(dev, direct):
        assert np.array_equal(a, b)
    # an error-only evaluation after an update of poses and landmarks leaves J and gives the errors of the moved estimates, in
    # both store forms
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
        assert np.abs(after[2] - dev[2]).max() > 1e-3
        c_ref = _chi2_ref(g, mp, mq, e_ref)
        assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref


@pytest.mark.parametrize("schur", [True, False])
@pytest.mark.parametrize("mode", H.MODES)
@pytest.mark.parametrize("huber", [0.0, 1.0])
def test_assembled_system_against_oracle(huber, mode, schur):
    """b, Hschur (landmarks marginalised: rank-1 terms of error dimension 1 in the 2x2 landmark blocks) or Hpp, chi2 and dx against
    OracleSolver fed the fp64 producers of all sets, with and without Huber, bearing-only and beside an EdgeSE2PointXY set."""
    capi = _capi()
    g = H.load_graph(Z, 257, mode)
    s, graph = H.device_setup(g, huber=huber, schur=schur)
    assert (s.landmark_sets[1] is None) == (mode == "bearing-only") and s.bearing_set is not None
    graph.linearize()
    o, kx, kb = H.oracle_bearing(g, schur)
    J0, J1, err = H.feed_oracle(g, o, kx, kb, huber=huber)
    if huber > 0:
        w = g["omega_b"] * err[:, 0] ** 2
        assert (w > 4 * huber * huber).sum() > 20 and (w < huber * huber).sum() > 20
    s.buildSystem()
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    which, name = (capi.HSCHUR, "Hschur") if schur else (capi.HPP, "Hpp")
    fig = {name: relerr(s.values(which), o.values(name)), "Hll": relerr(s.values(capi.HLL), o.values("Hll")),
           "Hpl": relerr(s.values(capi.HPL), o.values("Hpl")), "dx": relerr(s.x(), o.x())}
    print("huber %g %s schur %s" % (huber, mode, schur), fig)
    assert fig[name] < TOL_H and fig["Hll"] < TOL_H and fig["Hpl"] < TOL_H and fig["dx"] < TOL_X
    if schur:
        assert np.abs(s.x()[3 * g["nP"]:]).min() > 0          # (every free landmark moves)


class HostFedBearingGraph:
    """The graph protocol of openslam_g2o_amd.lm over ONE library handle whose bearing set is an ordinary edge set fed from the
    host: every evaluation reads poses and landmarks back, evaluates bearing.py in fp64 and uploads J0 / J1 / err through
    g2ohip_set_edge_data.  The estimates, the odometry set, the EdgeSE2PointXY set and the update stay with the device front end."""

    def __init__(self, s, g, set_id):
        self.s, self.g, self.k, self.J = s, g, set_id, None

    def _feed(self, jac):
        self.s.pgLinearize(jac)
        poses, points = self.s.pgGetEstimates(), self.s.pgGetLandmarkEstimates()
        if jac:
            J0, J1, err = H.producers(H.FP64, self.g, poses, points)
            self.J = (J0, J1)
        else:
            err = H.producers(H.FP64, self.g, poses, points, jac=False)
        self.s.setEdgeData(self.k, self.J[0], self.J[1], self.g["omega_b"], err)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


def _host_fed(g):
    capi = _capi()
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    sh = capi.HipBlockSolver(3, 2, 0)
    q0 = sh.addEdgeSet(3, h[g["vi"]], h[g["vj"]])
    qx = sh.addEdgeSet(2, h[g["vp"]], hl[g["vl"]]) if len(g["vp"]) else None
    qb = sh.addEdgeSet(1, h[g["bp"]], hl[g["bl"]])
    sh.buildStructure(g["nP"], g["nL"], True)
    sh.pgSetEdges(q0, 1, g["vi"], g["vj"], g["Z"], g["omega"])
    sh.pgSetEstimates(g["poses"], h)
    if qx is not None:
        sh.pgSetLandmarkEdges(qx, 3, g["vp"], g["vl"], g["zl"], g["omega_l"], None)
    sh.pgSetLandmarkEstimates(g["points"], hl)
    return sh, HostFedBearingGraph(sh, g, qb)


@pytest.mark.parametrize("mode", H.MODES)
def test_lm_run_device_resident_against_host_fed(mode):
    """LM twice through the same library over a 12-pose make_bearing_slam graph: device-resident, and with the bearing set
    host-fed from bearing.py.  Equal trial counts (the CPU runs' as well: one iteration rejects steps); the chi2 gap of every
    iteration within 8 x the gap between two equally valid CPU runs (the oracle's solver and a dense solve, recorded by
    tests/golden/make_bearing_edges.py); the poses end as close to the truth as the CPU run's."""
    key = "bearing" if mode == "bearing-only" else "mixed"
    g = H.lm_graph(mode)
    lam0 = H.LM_LAMBDA[mode]
    s, graph = H.device_setup(g)
    n_dev, chi_dev, _, tr_dev = lm.optimize(graph, s, H.LM_ITERATIONS, "lm", user_lambda_init=lam0)
    sh, host = _host_fed(g)
    n_host, chi_host, _, tr_host = lm.optimize(host, sh, H.LM_ITERATIONS, "lm", user_lambda_init=lam0)
    gaps = [abs(a - b) / b for a, b in zip(chi_dev, chi_host)]
    bound = H.DRIFT_FACTOR * Z["lm_%s_gap" % key]
    print(mode, "lm chi2 device", chi_dev)
    print(mode, "lm chi2 host-fed", chi_host)
    print(mode, "lm gaps", gaps, "bound", bound.tolist(), "trials", tr_dev, tr_host, Z["lm_%s_trials" % key].tolist())
    assert n_dev == n_host == H.LM_ITERATIONS
    assert [int(t) for t in tr_dev] == [int(t) for t in tr_host] and max(tr_dev) > 1
    for it, (gap, b) in enumerate(zip(gaps, bound)):
        assert gap <= b, (it, gap, b)
    e0, e1 = Z["lm_%s_pose_error" % key]
    final = H.pose_error(g, s.pgGetEstimates())
    print(mode, "pose error: initial", e0, "CPU run", e1, "device", final, "device vs CPU poses",
          np.abs(s.pgGetEstimates() - Z["lm_%s_poses" % key]).max(), "CPU vs CPU",
          np.abs(Z["lm_%s_poses" % key] - Z["lm_%s_poses_dense" % key]).max())
    assert e1 < e0 and final <= e1 * (1.0 + 1e-6)


def test_binding_rules():
    capi = _capi()
    Lb = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = H.load_graph(Z, 65)
    h, hl = _i32(g["hidx"]), _i32(g["pt_hidx"])
    vi, vj, vp, vl, bp, bl = (_i32(g[k]) for k in ("vi", "vj", "vp", "vl", "bp", "bl"))
    Zm, om, zl, wl, zb, wb = (_f64(g[k]) for k in ("Z", "omega", "zl", "omega_l", "zb", "omega_b"))

    def bind(s, k, a=bp, b=bl, m=zb, w=wb):
        p = lambda x, fn: None if x is None else fn(x)
        return Lb.g2ohip_pg_set_bearing_edges(s.h, k, p(a, _ip), p(b, _ip), p(m, _dp), p(w, _dp))

    # a handle whose landmark table is referenced by the bearing slot alone
    u = capi.HipBlockSolver(3, 2, 0)
    u0, u1 = u.addEdgeSet(3, h[vi], h[vj]), u.addEdgeSet(1, h[bp], hl[bl])
    assert bind(u, u1) == STATE                                        # before g2ohip_build_structure
    u.buildStructure(g["nP"], g["nL"], True)
    assert bind(u, u1) == STATE                                        # before a pose set is bound
    u.pgSetEdges(u0, 1, vi, vj, Zm, om)
    u.pgSetEstimates(g["poses"], h)
    assert bind(u, u1) == 0
    u.bearing_set = u1                                                 # (what pgSetBearingEdges records; the raw entry is used here)
    assert Lb.g2ohip_pg_linearize(u.h, 1) == STATE                     # bearing edges are bound but no landmark estimates
    wrong = hl.copy()
    wrong[0], wrong[1] = wrong[1], wrong[0]
    assert Lb.g2ohip_pg_set_landmark_estimates(u.h, 6, _dp(_f64(g["points"])), _ip(wrong)) == ARG
    assert Lb.g2ohip_pg_set_landmark_estimates(u.h, 5, _dp(_f64(g["points"][:5])), _ip(hl[:5])) == ARG   # a table too short for bl
    u.pgSetLandmarkEstimates(g["points"], hl)
    u.pgLinearize(True)
    alone = _data(u, g)
    assert np.array_equal(alone[2], H.producers(H.FP64, g, jac=False)) or np.abs(alone[2] - H.producers(H.FP64, g, jac=False)).max() < 1e-14
    assert Lb.g2ohip_pg_set_landmark_estimates(u.h, 6, _dp(_f64(g["points"])), _ip(wrong)) == ARG
    assert Lb.g2ohip_pg_linearize(u.h, 1) == 0
    assert np.array_equal(_data(u, g)[2], alone[2])
    # ... and the estimate stack moves that table
    u.buildSystem()
    u.setX(Z["moved_x"])
    u.pgPush()
    u.pgUpdate()
    assert np.abs(u.pgGetLandmarkEstimates() - Z["moved_points"]).max() < 1e-14
    u.pgPop()
    assert np.array_equal(u.pgGetLandmarkEstimates(), g["points"]) and np.array_equal(u.pgGetEstimates(), g["poses"])
    u.pgPush()
    u.pgUpdate()
    u.pgDiscardTop()
    assert np.abs(u.pgGetLandmarkEstimates() - Z["moved_points"]).max() < 1e-14

    # the bearing slot beside an EdgeSE2PointXY set and a prior set
    s = capi.HipBlockSolver(3, 2, 0)
    k0, kx, k1 = s.addEdgeSet(3, h[vi], h[vj]), s.addEdgeSet(2, h[vp], hl[vl]), s.addEdgeSet(1, h[bp], hl[bl])
    kz = s.addEdgeSet(1, _i32([]), _i32([]))                           # a set of zero edges
    kq = s.addEdgeSet(3, h[_i32([1, 2])], None)                        # a unary set (EdgeSE2Prior)
    s.buildStructure(g["nP"], g["nL"], False)
    s.pgSetEdges(k0, 1, vi, vj, Zm, om)
    s.pgSetEstimates(g["poses"], h)
    s.pgSetLandmarkEdges(kx, 3, vp, vl, zl, wl, None)
    s.pgSetLandmarkEstimates(g["points"], hl)
    s.pgSetPriorEdges(kq, 7, _i32([1, 2]), g["poses"][[1, 2]] + 0.01, np.tile(np.eye(3).reshape(1, -1), (2, 1)), None)
    assert bind(s, k1) == 0
    s.bearing_set = k1
    s.pgLinearize(True)
    s.buildSystem()
    chi0, ref = s.chi2(), _data(s, g)
    for x, y in zip(ref, alone):
        assert np.array_equal(x, y)

    def unchanged():
        assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
        s.buildSystem()
        assert s.chi2() == chi0
        for a, b in zip(_data(s, g), ref):
            assert np.array_equal(a, b)

    other = _f64(zb + 0.25)
    t = capi.HipBlockSolver(6, 3, 0)                                   # an EdgeSE3 pose set: the pose type must be 1
    T = np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), (4, 1))
    q0, q1 = t.addEdgeSet(6, h[vi], h[vj]), t.addEdgeSet(1, h[bp], hl[bl])
    t.buildStructure(g["nP"], g["nL"], False)
    t.pgSetEdges(q0, 2, vi, vj, T[:3], np.tile(np.eye(6).reshape(1, -1), (3, 1)))
    assert bind(t, q1) == ARG
    w = capi.HipBlockSolver(3, 2, 0)                                   # a unary set, a set of other dimensions (2, 3, 2), a pose-pose one (1, 3, 3)
    w0, wu, w2, wp = w.addEdgeSet(3, h[vi], h[vj]), w.addEdgeSet(1, h[bp], None), w.addEdgeSet(2, h[bp], hl[bl]), w.addEdgeSet(1, h[bp], h[(bp + 1) % 4])
    w.buildStructure(g["nP"], g["nL"], False)
    w.pgSetEdges(w0, 1, vi, vj, Zm, om)
    assert bind(w, wu) == ARG and bind(w, w2) == ARG and bind(w, wp) == ARG
    assert bind(s, kx, a=vp, b=vl, m=zb[:24], w=wb[:24]) == ARG         # bound as the landmark set
    assert bind(s, k0, a=vi, b=vj, m=zb[:3], w=wb[:3]) == ARG           # bound as the pose-pose set
    assert bind(s, kq, a=bp[:2], b=bl[:2], m=zb[:2], w=wb[:2]) == ARG   # bound as the prior set
    assert bind(s, 99) == ARG and bind(s, -1) == ARG
    for null in ("a", "b", "m", "w"):
        assert bind(s, k1, **{null: None}) == ARG
    for src, name, top in ((bp, "a", 4), (bl, "b", 6)):
        bad = src.copy()
        bad[7] = top
        assert bind(s, k1, m=other, **{name: bad}) == ARG              # outside the pose / landmark table
        bad[7] = -1
        assert bind(s, k1, m=other, **{name: bad}) == ARG
        bad[7] = (src[7] + 1) % top
        assert bind(s, k1, m=other, **{name: bad}) == ARG              # another vertex: its hessian index is not the set's
    for arr, name in ((zb, "m"), (wb, "w")):
        for v in (np.nan, np.inf):
            x = arr.copy()
            x[2] = v
            assert bind(s, k1, **{name: x}) == ARG
    unchanged()
    # refusals of the other entries while the set is bound
    zeros = lambda c: _dp(_f64(np.zeros((65, c))))
    assert Lb.g2ohip_pg_set_prior_edges(s.h, k1, 7, _ip(bp), zeros(3), zeros(9), None) == ARG
    assert Lb.g2ohip_pg_set_landmark_edges(s.h, k1, 3, _ip(bp), _ip(bl), zeros(2), zeros(4), None) == ARG
    assert Lb.g2ohip_pg_set_edges(s.h, k1, 1, _ip(bp), _ip(bl), zeros(3), zeros(9)) == ARG
    assert Lb.g2ohip_pg_set_offset_edges(s.h, k1, 18, _ip(bp), _ip(bl), _ip(bp), _ip(bp), zeros(3), zeros(9), 1, zeros(3)) == ARG
    assert Lb.g2ohip_pg_set_gicp_edges(s.h, k1, _ip(bp), _ip(bl), zeros(6), zeros(9), None) == ARG
    assert Lb.g2ohip_pg_set_cam_edges(s.h, k1, 17, _ip(bp), _ip(bl), zeros(1), zeros(1)) == ARG
    for typ in (2, 10, 12):                                            # pose types that do not fit the bound bearing set
        assert Lb.g2ohip_pg_set_edges(s.h, k0, typ, _ip(vi), _ip(vj), _dp(Zm), _dp(om)) == ARG
    unchanged()
    with pytest.raises(ValueError):
        s.pgSetBearingEdges(k1, bp[:-1], bl[:-1], zb[:-1], wb[:-1])
    with pytest.raises(ValueError):
        s.pgSetBearingEdges(k1, bp, bl, zb, wb[:-1])
    # n = 0 is legal (null arrays), and replaces the binding; binding the full set again restores it
    assert bind(s, kz, a=None, b=None, m=None, w=None) == 0
    assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
    assert bind(s, k1) == 0
    unchanged()
    # changed estimate tables are validated against the bearing set too
    wrong = h.copy()
    wrong[1], wrong[2] = wrong[2], wrong[1]
    assert Lb.g2ohip_pg_set_estimates(s.h, 4, _dp(_f64(g["poses"])), _ip(wrong)) == ARG
    wrong = hl.copy()
    wrong[0], wrong[1] = wrong[1], wrong[0]
    assert Lb.g2ohip_pg_set_landmark_estimates(s.h, 6, _dp(_f64(g["points"])), _ip(wrong)) == ARG
    assert Lb.g2ohip_pg_set_landmark_estimates(s.h, 5, _dp(_f64(g["points"][:5])), _ip(hl[:5])) == ARG   # a table too short for bl
    unchanged()
    # g2ohip_update_structure: a bearing set needs landmarks in the structure, and with landmarks in the structure the library
    # refuses growth as the reference does (block_solver.hpp:313-316) -- nothing changes, the binding stands
    assert s.updateStructure(0, k1, h[_i32([1])], hl[_i32([2])]) is False
    unchanged()
    s.clearEdgeSets()
    assert s.bearing_set is None
    assert Lb.g2ohip_pg_linearize(s.h, 1) == STATE


def test_beside_priors_and_offset_edges():
    """The bearing slot beside a prior set (type 7) and a sensor-offset set (type 18) on one handle, landmarks marginalised: the
    reduced system and dx against the oracle fed the fp64 producers of all four sets."""
    capi = _capi()
    g = S.make_bearing_slam(12, 10, seed=2, priors="pose", prior_stride=4)
    r = S.make_offset_rig("se2", 12, 2, 3, seed=2)
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    go = dict(kind="se2", offset_type=18, poses=g["poses"], oi=r["oi"], oj=r["oj"], opf=r["opf"], opt=r["opt"], omeas=r["omeas"],
              oinfo=r["oinfo"], offsets=r["offsets"])
    s = capi.HipBlockSolver(3, 2, 0)
    k0, kb = s.addEdgeSet(3, h[g["vi"]], h[g["vj"]]), s.addEdgeSet(1, h[g["bp"]], hl[g["bl"]])
    kq, ko = s.addEdgeSet(3, h[g["vq"]], None), s.addEdgeSet(3, h[go["oi"]], h[go["oj"]])
    s.buildStructure(g["nP"], g["nL"], True)
    s.pgSetEdges(k0, 1, g["vi"], g["vj"], g["Z"], g["omega"])
    s.pgSetEstimates(g["poses"], h)
    s.pgSetBearingEdges(kb, g["bp"], g["bl"], g["zb"], g["omega_b"])
    s.pgSetLandmarkEstimates(g["points"], hl)
    s.pgSetPriorEdges(kq, 7, g["vq"], g["zq"], g["omega_q"], None)
    s.pgSetOffsetEdges(ko, 18, go["oi"], go["oj"], go["opf"], go["opt"], go["omeas"], go["oinfo"], go["offsets"])
    s.pgLinearize(True)
    o = O.OracleSolver(3, 2, g["nP"], g["nL"], True)
    o.set_dims(o.add_edge_set(3, h[g["vi"]], h[g["vj"]]), 3, 3)
    o.set_dims(o.add_edge_set(1, h[g["bp"]], hl[g["bl"]]), 3, 2)
    o.set_dims(o.add_edge_set(3, h[g["vq"]]), 3, 0)
    o.set_dims(o.add_edge_set(3, h[go["oi"]], h[go["oj"]]), 3, 3)
    o.build_structure()
    A0, A1, e0 = LH.pose_edges(g)
    B0, B1, e1 = H.producers(H.FP64, g)
    Q0, eq = PH.prior_edges(g)
    J0, J1, err = OH.producers(OH.FP64, go)
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    o.set_edge_data(1, B0, B1, g["omega_b"], e1)
    o.set_edge_data(2, Q0, None, g["omega_q"], eq)
    o.set_edge_data(3, J0, J1, go["oinfo"], err)
    dev = _data(s, g)
    assert max(relerr(dev[0], B0), relerr(dev[1], B1), relerr(dev[2], e1)) < 1e-12
    s.buildSystem()
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B and abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    fig = dict(Hschur=relerr(s.values(capi.HSCHUR), o.values("Hschur")), dx=relerr(s.x(), o.x()))
    print("beside priors and offset edges", fig)
    assert fig["Hschur"] < TOL_H and fig["dx"] < TOL_X


@pytest.mark.parametrize("mode", H.MODES)
def test_from_a_file(mode, tmp_path):
    """written with g2o_io.write_g2o_bearing, read back, set up, one LM iteration: device-resident against host-fed."""
    g = S.make_bearing_slam(10, 8, with_xy=(mode != "bearing-only"), seed=9)
    path = os.path.join(str(tmp_path), "bearing.g2o")
    g2o_io.write_g2o_bearing(path, g)
    p = g2o_io.bearing_problem(g2o_io.read_g2o(path))
    s, graph = H.device_setup(p)
    graph.linearize()
    chi0 = graph.chi2()
    done, chis, _, tr = lm.optimize(graph, s, 1, "lm")
    sh, host = _host_fed(p)
    done_h, chis_h, _, tr_h = lm.optimize(host, sh, 1, "lm")
    print(mode, "from a file: chi2", chi0, "->", chis, "host-fed", chis_h, "trials", tr, tr_h)
    assert done == done_h == 1 and [int(t) for t in tr] == [int(t) for t in tr_h]
    assert chis[-1] < chi0 and abs(chis[-1] - chis_h[-1]) <= 1e-9 * chis_h[-1]
    assert np.abs(s.pgGetEstimates() - sh.pgGetEstimates()).max() < 1e-9
    assert np.abs(s.pgGetLandmarkEstimates() - sh.pgGetLandmarkEstimates()).max() < 1e-9
