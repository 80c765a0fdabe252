"""GPU: landmark self-calibration on the device (EdgeSE2PointXYCalib = type 24 beside an EdgeSE2 set,
g2ohip_pg_set_pointxy_calib_edges): the producer against the fp64 restatement of openslam_g2o_amd/pointxy_calib.py within 8 x that
restatement's recorded drift against 60 digits (tests/golden/pointxy_calib_edges.npz), tails, both store forms, the error-only
evaluation, vertex indexing over both tables, the assembled system and its solution against the CPU oracle's three-vertex edges, a
dense calibration row with a long list on one (calib, landmark) pair, a Levenberg-Marquardt run against the host-fed one, the
binding rules, the other slots beside it, a graph from a file."""
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io, lm, offset_edges as OE, synthetic as S
from tests import pointxy_calib_helpers as H
from tests import producer_metric as PM
from tests.helpers import relerr

pytestmark = pytest.mark.gpu

Z = np.load(H.GOLDEN)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_B = 1e-11       # right-hand side, as tests/test_gpu_sensor_calib.py
TOL_H = 1e-12       # assembled blocks
TOL_X = 1e-8        # solution
TOL_X_DENSE = 1e-7  # the dense tolerance of tests/test_gpu_sensor_calib.py
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE
PCG = {"linear_solver": 1, "pcg_tolerance": 1e-22, "pcg_absolute_tolerance": 0, "pcg_max_iterations": 2000}   # (to the rounding level)
KEYS = ("Jp", "Jl", "Jc")


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _data(s, n):
    """(Jp, Jl, Jc, err) as the next buildSystem reads them; the three sets must show the SAME shared arrays."""
    kpl, kpc, klc = s.pointxy_calib_sets
    Jp, Jl, err = s.edgeData(kpl, n, 2, 3, 2)
    Jp2, Jc, err2 = s.edgeData(kpc, n, 2, 3, 3)
    Jl3, Jc3, err3 = s.edgeData(klc, n, 2, 2, 3)
    assert np.array_equal(Jp, Jp2) and np.array_equal(Jl, Jl3) and np.array_equal(Jc, Jc3)
    assert np.array_equal(err, err2) and np.array_equal(err, err3)
    return Jp, Jl, Jc, err


def _chi2_ref(g, poses, err, huber=0.0):
    e0 = H.pose_edges(g, poses, jac=False)
    return OE.chi2(err, g["omega_q"], huber) + float(np.einsum("ni,nij,nj->n", e0, np.asarray(g["omega"]).reshape(-1, 3, 3), e0).sum())


def _record(line):
    """one line per (kind, graph) in profiles/pointxy_calib.jsonl: a later run replaces its earlier figure"""
    path = os.path.join(ROOT, "profiles", "pointxy_calib.jsonl")
    same = lambda d: d.get("kind") == line["kind"] and d.get("graph") == line.get("graph")
    keep = [l for l in open(path).read().splitlines() if l.strip() and not same(json.loads(l))] if os.path.exists(path) else []
    with open(path, "w") as f:
        for l in keep + [json.dumps(line)]:
            f.write(l + "\n")


def _within(tag, dev, ref, drift):
    """device against the restatement: 8 x the recorded drift of (err, J), itself below the per-row ceiling of producer_metric."""
    n = len(ref[3])
    fig = (np.abs(dev[3] - ref[3]).max(), max(np.abs(dev[k] - ref[k]).max() for k in range(3)))
    ones = np.ones((n, 2))
    rows = (PM.worst_row(dev[3], ref[3], ones, 2)[0], max(PM.worst_row(dev[k], ref[k], ones, 2)[0] for k in range(3)))
    print(tag, "device vs restatement (err, J)", fig, "bound", H.DRIFT_FACTOR * np.asarray(drift), "per-row figure", rows)
    _record(dict(kind="device_vs_restatement", graph=tag, edges=n, err=float(fig[0]), J=float(fig[1]), bound_err=float(H.DRIFT_FACTOR * drift[0]),
                 bound_J=float(H.DRIFT_FACTOR * drift[1])))
    for f, b, r in zip(fig, drift, rows):
        assert H.DRIFT_FACTOR * b <= PM.CEILING
        assert f <= H.DRIFT_FACTOR * b, (tag, fig, drift)
        assert r <= PM.CEILING


@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_producer_tails(n):
    row = H.EDGE_COUNTS.index(n)
    g = H.load_graph(Z, n)
    s, graph = H.device_setup(g)
    assert s.landmark_sets[1] is None and len(s.pointxy_calib_sets) == 3
    graph.linearize()
    ref = H.producers(H.FP64, g)
    dev = _data(s, n)
    _within("pointxy_calib_%d" % n, dev, ref, Z["drift"][row])
    if n >= H.N_SPECIAL:
        # the golden edges proper against the 60-digit values: the device's 8 x drift from the restatement plus the restatement's own
        m, (be, bJ) = H.N_SPECIAL, Z["drift"][1]
        fig = (np.abs(dev[3][:m] - Z["err"][:m]).max(), max(np.abs(dev[k][:m] - Z[key][:m]).max() for k, key in enumerate(KEYS)))
        print("golden edges: device vs 60 digits (err, J)", fig, "bound", (H.DRIFT_FACTOR + 1) * be, (H.DRIFT_FACTOR + 1) * bJ)
        assert fig[0] <= (H.DRIFT_FACTOR + 1) * be and fig[1] <= (H.DRIFT_FACTOR + 1) * bJ
    fp, fl = g["qp"] == 0, g["ql"] == 0
    assert not dev[0][fp].any() and not dev[1][fl].any()                  # the blocks of the fixed pose and the fixed landmark: zeros
    assert dev[0][~fp].any(axis=1).all() and dev[1][~fl].any(axis=1).all() and dev[2].any(axis=1).all()
    s.buildSystem()
    c_ref = _chi2_ref(g, None, ref[3])
    assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref
    # the other store form: the same bits
    s.setOption("pg_landmark_staged", 0)
    s.pgSetEstimates(g["poses"], g["hidx"])
    s.pgLinearize(True)
    direct = _data(s, n)
    for a, b in zip(dev, direct):
        assert np.array_equal(a, b)
    # an error-only evaluation after an update leaves J and gives the errors of the moved tables, in both store forms
    for staged in (0, 1):
        s.setOption("pg_landmark_staged", staged)
        s.pgSetEstimates(g["poses"], g["hidx"])
        s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
        s.pgLinearize(True)
        s.buildSystem()
        s.setX(Z["moved_x"])
        s.pgUpdate()
        s.pgLinearize(False)
        mp_, mq_ = s.pgGetEstimates(), s.pgGetLandmarkEstimates()
        assert np.abs(mp_ - Z["moved_poses"]).max() < 1e-14 and np.abs(mq_ - Z["moved_points"]).max() < 1e-14
        e_ref = H.producers(H.FP64, g, mp_, mq_, jac=False)
        after = _data(s, n)
        assert all(np.array_equal(after[k], dev[k]) for k in range(3))
        fig = np.abs(after[3] - e_ref).max()
        print(n, "moved: device vs restatement", fig, "bound", H.DRIFT_FACTOR * Z["moved_drift"][row])
        assert fig <= H.DRIFT_FACTOR * Z["moved_drift"][row]
        assert np.abs(after[3] - dev[3]).max() > 1e-3
        c_ref = _chi2_ref(g, mp_, e_ref)
        assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref


def test_index_permutation():
    """The 9 pose rows scattered over a table of 40 rows and the 12 landmarks over a table of 30 whose other rows hold other values
    (fixed, unused); the calibration vertices are not the last rows.  A kernel that reads row k instead of row v[k], or the wrong
    table, cannot give the same bits."""
    n = 25
    g = H.load_graph(Z, n)
    s, graph = H.device_setup(g)
    graph.linearize()
    ref = _data(s, n)
    rng = np.random.default_rng(11)
    where = rng.permutation(39)[:9].astype(np.int32)             # new row of old pose row r: row 39 is never one of them
    wl = rng.permutation(30)[:12].astype(np.int32)
    assert (where != np.arange(9)).sum() >= 7 and where.max() >= 9 and where[[6, 7, 8]].max() < 39 and (wl != np.arange(12)).sum() >= 10
    poses = rng.normal(size=(40, 3)) * 5.0
    poses[where] = g["poses"]
    hidx = np.full(40, -1, np.int32)
    hidx[where] = g["hidx"]
    points = rng.normal(size=(30, 2)) * 5.0
    points[wl] = g["points"]
    pt_hidx = np.full(30, -1, np.int32)
    pt_hidx[wl] = g["pt_hidx"]
    gp = H.finish(dict(g, poses=poses, hidx=hidx, points=points, pt_hidx=pt_hidx, vi=where[g["vi"]], vj=where[g["vj"]], qp=where[g["qp"]],
                       ql=wl[g["ql"]], qc=where[g["qc"]]))
    sp, graph_p = H.device_setup(gp)
    graph_p.linearize()
    for a, b in zip(_data(sp, n), ref):
        assert np.array_equal(a, b)
    s.buildSystem()
    sp.buildSystem()
    assert sp.chi2() == s.chi2() and np.array_equal(sp.b(), s.b())
    # the pose and the calibration vertex of every edge swapped: another graph
    gs = dict(g, qp=g["qc"], qc=g["qp"])
    ss, graph_s = H.device_setup(gs)
    graph_s.linearize()
    assert (np.abs(_data(ss, n)[3] - ref[3]).max(axis=1) > 1e-6).all()


def _dense_device(s):
    """the device's [Hpp Hpl; Hpl' Hll] as a dense symmetric matrix"""
    capi = _capi()
    p, l, nP, nL = 3, 2, s.nP, s.nL
    Hm = np.zeros((p * nP + l * nL, p * nP + l * nL))
    cp, row = s.pattern(capi.HPP)
    v = s.values(capi.HPP).reshape(-1, p, p)
    for c in range(nP):
        for q in range(cp[c], cp[c + 1]):
            r, B = row[q], v[q].T
            Hm[p * r:p * r + p, p * c:p * c + p] = B
            Hm[p * c:p * c + p, p * r:p * r + p] = B.T
    cp, row = s.pattern(capi.HPL)
    v = s.values(capi.HPL).reshape(-1, l, p)
    o = p * nP
    for c in range(nL):
        for q in range(cp[c], cp[c + 1]):
            r, B = row[q], v[q].T
            Hm[p * r:p * r + p, o + l * c:o + l * c + l] = B
            Hm[o + l * c:o + l * c + l, p * r:p * r + p] = B.T
    v = s.values(capi.HLL).reshape(-1, l, l)
    for c in range(nL):
        Hm[o + l * c:o + l * c + l, o + l * c:o + l * c + l] = v[c].T
    return Hm


def _check_system(s, g, huber, schur, tag):
    o, kx, m = H.oracle_calib(g, schur)
    _, _, _, err = H.feed_oracle(g, o, kx, m, huber)
    s.buildSystem()
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    Hd, Ho = _dense_device(s), o.dense_full()
    P = 3 * g["nP"]
    fig = dict(Hpp=relerr(Hd[:P, :P], Ho[:P, :P]), Hpl=relerr(Hd[:P, P:], Ho[:P, P:]), Hll=relerr(Hd[P:, P:], Ho[P:, P:]), dx=relerr(s.x(), o.x()))
    print(tag, fig)
    assert fig["Hpp"] < TOL_H and fig["Hpl"] < TOL_H and fig["Hll"] < TOL_H and fig["dx"] < TOL_X
    x = s.x()
    if schur:
        assert np.abs(x[P:]).min() > 0                                    # (every free landmark moves)
    else:                                                                 # the documented behaviour: Hpp alone is solved
        assert not x[P:].any()
        xp = np.linalg.solve(Ho[:P, :P], o.b()[:P])
        assert relerr(x[:P], xp) < TOL_X
    s.restoreDiagonal()
    o.restore_diagonal()
    return err


def _refix(g, pose_rows=(0,), point_rows=()):
    hidx, pt_hidx, nP, nL = g2o_io.landmark_hessian_index(g["n"], g["L"], list(pose_rows), list(point_rows))
    poses = g["poses"].copy()
    if g["calib_row"] in pose_rows:
        poses[g["calib_row"]] = g["offset_true"]
    return dict(g, hidx=hidx, pt_hidx=pt_hidx, nP=nP, nL=nL, poses=poses)


@pytest.mark.parametrize("case,solver", [(c, v) for c in ("calib_free", "calib_fixed", "landmark_fixed") for v in ("direct", "pcg")] +
                         [("no_schur", "direct")])
@pytest.mark.parametrize("huber", [0.0, 8.0])
def test_assembled_system_against_oracle(huber, case, solver):
    """Hpp, Hpl, Hll, b, chi2 and the solved x against OracleSolver fed the fp64 restatement through add_multi_edge_set: 20 poses, 12
    landmarks, 200 observations, every tenth a gross outlier; with and without Huber on the three sets (width 8: at the initial
    estimates, the offset at the identity, the inliers' e' Omega e spread over 8 .. 135); the calibration vertex free and fixed; a
    fixed landmark; the direct solver and PCG; do_schur 1, and do_schur 0 with the direct solver (Hpp alone is solved, the
    landmarks stay)."""
    g = S.make_pointxy_calib_slam(20, 12, seed=2)
    g["zq"][::10] += 2.0
    if case == "calib_fixed":
        g = _refix(g, [0, g["calib_row"]])
    elif case == "landmark_fixed":
        g = _refix(g, [0], [3])
        assert (g["ql"] == 3).any()
    schur = case != "no_schur"
    s, graph = H.device_setup(g, huber=huber, schur=schur, options=PCG if solver == "pcg" else None)
    graph.linearize()
    err = _check_system(s, g, huber, schur, "huber %g %s %s" % (huber, case, solver))
    if huber > 0:
        w = np.einsum("ni,nij,nj->n", err, g["omega_q"].reshape(-1, 2, 2), err)
        assert (w > 4 * huber * huber).sum() >= 6 and (w < huber * huber).sum() >= 6
    dev = _data(s, g["Q"])
    fp, fl = np.asarray(g["hidx"]) < 0, np.asarray(g["pt_hidx"]) < 0
    assert not dev[0][fp[g["qp"]]].any() and not dev[1][fl[g["ql"]]].any() and not dev[2][fp[g["qc"]]].any()


def test_dense_row_and_column():
    """Every edge names the one calibration vertex; landmark 0 is observed 300 times (from 60 poses, five times each), so one
    (calib, landmark) block of Hpl sums 300 terms.  x against a dense fp64 solve of the oracle's damped matrix."""
    capi = _capi()
    rng = np.random.default_rng(4)
    g = S.make_pointxy_calib_slam(60, 8, seed=1)
    extra = 300
    qp = np.concatenate([g["qp"], np.tile(np.arange(60), 5)]).astype(np.int32)
    ql = np.concatenate([g["ql"], np.zeros(extra)]).astype(np.int32)
    qc = np.full(len(qp), g["calib_row"], np.int32)
    from openslam_g2o_amd import pointxy_calib as PC
    z_new = np.stack([PC.predict(g["poses_true"][p], g["points_true"][0], g["offset_true"]) for p in qp[-extra:]]) + rng.normal(size=(extra, 2)) * 0.05
    g = dict(g, qp=qp, ql=ql, qc=qc, zq=np.concatenate([g["zq"], z_new]), omega_q=np.tile(g["omega_q"][:1], (len(qp), 1)), Q=len(qp))
    s, graph = H.device_setup(g)
    graph.linearize()
    o, kx, m = H.oracle_calib(g)
    H.feed_oracle(g, o, kx, m)
    s.buildSystem()
    o.build_system()
    cp, row = s.pattern(capi.HPL)
    c0 = int(g["pt_hidx"][0] - g["nP"])
    assert (row[cp[c0]:cp[c0 + 1]] == g["hidx"][g["calib_row"]]).any() and (ql == 0).sum() >= 300
    lam = 1e-4 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve()
    x_ref = np.linalg.solve(o.dense_full(), o.b())
    fig = dict(dx=relerr(s.x(), x_ref), H=relerr(_dense_device(s), o.dense_full()), b=relerr(s.b(), o.b()))
    print("dense row and column", fig)
    assert fig["b"] < TOL_B and fig["H"] < TOL_H and fig["dx"] < TOL_X_DENSE
    x = s.x()
    assert s.solve() and np.array_equal(s.x(), x)                        # bit-repeatable


class HostFedGraph:
    """The graph protocol of openslam_g2o_amd.lm over ONE library handle whose three calibration sets are ordinary edge sets fed from
    the host: every evaluation reads both tables back, evaluates pointxy_calib.py in fp64 and uploads the arrays through
    g2ohip_set_edge_data.  The estimates, the odometry set, the EdgeSE2PointXY set and the update stay with the device front end."""

    def __init__(self, s, g, ids):
        self.s, self.g, self.ids, self.J = s, g, ids, None

    def _feed(self, jac):
        self.s.pgLinearize(jac)
        poses, points = self.s.pgGetEstimates(), self.s.pgGetLandmarkEstimates()
        if jac:
            Jp, Jl, Jc, err = H.producers(H.FP64, self.g, poses, points)
            self.J = (Jp, Jl, Jc)
        else:
            err = H.producers(H.FP64, self.g, poses, points, jac=False)
        Jp, Jl, Jc = self.J
        for k, (A, B) in zip(self.ids, ((Jp, Jl), (Jp, Jc), (Jl, Jc))):
            self.s.setEdgeData(k, A, B, self.g["omega_q"], err)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


def _three_sets(s, g):
    capi = _capi()
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
    ids = []
    for (a, b), pt in zip(((h[g["qp"]], hl[g["ql"]]), (h[g["qp"]], h[g["qc"]]), (hl[g["ql"]], h[g["qc"]])), parts):
        ids.append(s.addEdgeSet(2, a, b))
        s.setEdgeSetParts(ids[-1], pt)
    return ids


def _host_fed(g):
    capi = _capi()
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    sh = capi.HipBlockSolver(3, 2, 0)
    q0 = sh.addEdgeSet(3, h[g["vi"]], h[g["vj"]])
    qx = sh.addEdgeSet(2, h[g["vp"]], hl[g["vl"]]) if len(g["vp"]) else None
    ids = _three_sets(sh, g)
    sh.buildStructure(g["nP"], g["nL"], True)
    sh.pgSetEdges(q0, 1, g["vi"], g["vj"], g["Z"], g["omega"])
    sh.pgSetEstimates(g["poses"], h)
    if qx is not None:
        sh.pgSetLandmarkEdges(qx, 3, g["vp"], g["vl"], g["zl"], g["omega_l"], None)
    sh.pgSetLandmarkEstimates(g["points"], hl)
    return sh, HostFedGraph(sh, g, ids)


def test_lm_run_device_resident_against_host_fed():
    """LM twice through the same library over make_pointxy_calib_slam at 40 poses and 30 landmarks: device-resident, and with the
    three sets host-fed from pointxy_calib.py.  Equal trial counts (the CPU runs' as well); the chi2 gap of every iteration within
    the largest gap between two equally valid CPU runs (the oracle's Schur solver and a dense solve, recorded by
    tests/golden/make_pointxy_calib_edges.py, never taken from the device); the offset moves from the identity to within the
    generator's noise of the truth."""
    g = H.lm_graph()
    s, graph = H.device_setup(g)
    n_dev, chi_dev, _, tr_dev = lm.optimize(graph, s, H.LM_ITERATIONS, "lm")
    sh, host = _host_fed(g)
    n_host, chi_host, _, tr_host = lm.optimize(host, sh, H.LM_ITERATIONS, "lm")
    gaps = [abs(a - b) / b for a, b in zip(chi_dev, chi_host)]
    bound = float(Z["lm_gap"].max())
    print("lm chi2 device", chi_dev)
    print("lm chi2 host-fed", chi_host)
    print("lm gaps", gaps, "bound", bound, "trials", tr_dev, tr_host, Z["lm_trials"].tolist())
    _record(dict(kind="lm_device_vs_host_fed", gaps=[float(x) for x in gaps], bound=bound, trials=[int(t) for t in tr_dev]))
    assert n_dev == n_host == H.LM_ITERATIONS
    assert [int(t) for t in tr_dev] == [int(t) for t in tr_host] == Z["lm_trials"].tolist()
    for it, gap in enumerate(gaps):
        assert gap <= bound, (it, gap, bound)
    e0, e1 = H.offset_error(g, g["poses"]), H.offset_error(g, s.pgGetEstimates())
    print("offset error: initial", e0, "device", e1, "CPU run", Z["lm_offset_error"][1].tolist())
    assert e0[0] > 0.3 and e1[0] <= H.LM_ARGS["noise"] and e1[1] <= H.LM_ARGS["noise"]


def test_binding_rules():
    capi = _capi()
    Lb = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = S.make_pointxy_calib_slam(12, 6, seed=4, with_xy=True)
    # one more pose row behind the calibration vertex: the parameter vertex of a type-22 group (an additive row while bound)
    g = dict(g, n=g["n"] + 1, nP=g["nP"] + 1, poses=np.vstack([g["poses"], [1.0, 1.1, 0.5]]), hidx=np.append(g["hidx"], g["nP"]).astype(np.int32),
             pt_hidx=np.where(g["pt_hidx"] >= 0, g["pt_hidx"] + 1, -1).astype(np.int32))
    prow = g["n"] - 1
    n = g["Q"]
    h, hl = _i32(g["hidx"]), _i32(g["pt_hidx"])
    vi, vj, qp, ql, qc, vp, vl = (_i32(g[k]) for k in ("vi", "vj", "qp", "ql", "qc", "vp", "vl"))
    Zm, om, zm, zw = (_f64(g[k]) for k in ("Z", "omega", "zq", "omega_q"))

    def bind(s, ids, a=qp, b=ql, c=qc, m=zm, w=zw):
        p = lambda x, fn: None if x is None else fn(x)
        return Lb.g2ohip_pg_set_pointxy_calib_edges(s.h, ids[0], ids[1], ids[2], p(a, _ip), p(b, _ip), p(c, _ip), p(m, _dp), p(w, _dp))

    def odom_sets(s):
        e = np.arange(3)
        out = []
        for (a, b), pt in zip(((h[vi[e]], h[vj[e]]), (h[vi[e]], h[np.full(3, prow)]), (h[vj[e]], h[np.full(3, prow)])), (0, 7, 5)):
            out.append(s.addEdgeSet(3, a, b))
            s.setEdgeSetParts(out[-1], pt)
        return out

    def bind_odom(s, ko, vp_rows=None):
        rows = _i32(np.full(3, prow) if vp_rows is None else vp_rows)
        return Lb.g2ohip_pg_set_odom_calib_edges(s.h, ko[0], ko[1], ko[2], _ip(_i32(vi[:3])), _ip(_i32(vj[:3])), _ip(rows),
                                                 _dp(_f64(np.tile([0.5, 0.6, 1.0], (3, 1)))), None)

    s = capi.HipBlockSolver(3, 2, 0)
    k0 = s.addEdgeSet(3, h[vi], h[vj])
    kxy = s.addEdgeSet(2, h[vp], hl[vl])
    ids = _three_sets(s, g)
    kb = s.addEdgeSet(1, h[qp], hl[ql])                                   # bound in the bearing slot below
    kpr = s.addEdgeSet(3, h[qp], None)                                    # ... the prior slot
    koff = s.addEdgeSet(3, h[vi], h[vj])                                  # ... the offset slot
    ko = odom_sets(s)
    kc21 = []
    for (a, b), pt in zip(((h[vi], h[vj]), (h[vi], h[qc[:len(vi)]]), (h[vj], h[qc[:len(vi)]])), (0, 7, 5)):
        kc21.append(s.addEdgeSet(3, a, b))
        s.setEdgeSetParts(kc21[-1], pt)
    assert bind(s, ids) == STATE                                          # before g2ohip_build_structure
    s.buildStructure(g["nP"], g["nL"], True)
    assert bind(s, ids) == STATE                                          # no type-1 set bound
    s.pgSetEdges(k0, 1, vi, vj, Zm, om)
    s.pgSetEstimates(g["poses"], h)
    s.pgSetLandmarkEdges(kxy, 3, vp, vl, g["zl"], g["omega_l"], None)
    s.pgSetLandmarkEstimates(g["points"], hl)
    s.pgSetBearingEdges(kb, qp, ql, np.zeros(n), np.ones(n))
    s.pgSetPriorEdges(kpr, 7, qp, g["poses"][qp], np.tile(np.eye(3).reshape(1, 9), (n, 1)), None)
    ne = len(vi)
    s.pgSetOffsetEdges(koff, 18, vi, vj, np.zeros(ne, np.int32), np.zeros(ne, np.int32), Zm, om, np.zeros((1, 3)))
    s.pgSetSensorCalibEdges(*kc21, vi, vj, qc[:ne], Zm, om)
    assert bind_odom(s, ko) == 0                                          # a type-22 group on a row of its own: an additive row
    s.setRobustKernelPerEdge(ids[1], np.full(n, capi.KERNEL_HUBER, np.int32), np.ones(n))
    assert bind(s, ids) == STATE                                          # per-edge robust kernels at binding
    s.setRobustKernelPerEdge(ids[1], None, None)
    assert bind(s, ids) == 0
    s.pointxy_calib_sets = tuple(ids)                                     # (what pgSetPointXYCalibEdges records; the raw entry is used here)
    s.pgLinearize(True)
    s.buildSystem()
    chi0, b0, ref = s.chi2(), s.b(), _data(s, n)
    assert np.abs(ref[3] - H.producers(H.FP64, g, jac=False)).max() < 1e-12

    def unchanged():
        assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
        s.buildSystem()
        assert s.chi2() == chi0 and np.array_equal(s.b(), b0)
        for a, b in zip(_data(s, n), ref):
            assert np.array_equal(a, b)

    other = _f64(zm.copy())
    other[:, -1] += 0.25                                                  # (a rejected call must not leave these measurements behind)
    kpl, kpc, klc = ids
    for bad_ids in ((99, kpc, klc), (kpl, -1, klc), (kpl, kpc, 99),       # a foreign set id
                    (kpl, kpl, klc), (kpl, kpc, kpc), (klc, kpc, klc),    # a repeated set id
                    (kpl, klc, kpc), (kpc, kpl, klc),                     # wrong parts / dimensions: the sets exchanged
                    (k0, kpc, klc), (kxy, kpc, klc), (kb, kpc, klc), (kpr, kpc, klc), (koff, kpc, klc),   # bound in another slot
                    (kpl, kc21[1], klc), (kpl, ko[1], klc)):              # ... the type-21 group's, a type-22 group's (dimensions too)
        assert bind(s, bad_ids, m=other) == ARG, bad_ids
    for null in ("a", "b", "c", "m"):
        assert bind(s, ids, **{null: None}) == ARG
    for arr, name in ((zm, "m"), (zw, "w")):
        for v in (np.nan, np.inf):
            x = arr.copy()
            x[2, 1] = v
            assert bind(s, ids, **{name: x}) == ARG                       # non-finite values
    for name, src, size in (("a", qp, len(h)), ("b", ql, len(hl)), ("c", qc, len(h))):
        for v in (size, -1):
            bad = src.copy()
            bad[3] = v
            assert bind(s, ids, m=other, **{name: bad}) == ARG            # outside its table
        bad = src.copy()
        bad[3] = next(v for v in range(1, 6) if v != src[3] and (name != "b" or hl[v] != hl[src[3]]))
        assert bind(s, ids, m=other, **{name: bad}) == ARG                # another vertex: its hessian index is not the sets'
    bad = qp.copy()
    bad[3] = qc[3]
    assert bind(s, ids, m=other, a=bad) == ARG                            # pose_vertex[k] == calib_vertex[k]
    unchanged()
    # ownership in the other direction: every other entry refuses the group's set ids
    zeros = lambda c: _dp(_f64(np.zeros((n, c))))
    for k in ids:
        assert Lb.g2ohip_pg_set_prior_edges(s.h, k, 7, _ip(qp), zeros(3), zeros(9), None) == ARG
        assert Lb.g2ohip_pg_set_landmark_edges(s.h, k, 3, _ip(qp), _ip(ql), zeros(2), zeros(4), None) == ARG
        assert Lb.g2ohip_pg_set_edges(s.h, k, 1, _ip(qp), _ip(qc), zeros(3), zeros(9)) == ARG
        assert Lb.g2ohip_pg_set_offset_edges(s.h, k, 18, _ip(qp), _ip(qc), _ip(qp), _ip(qp), zeros(3), zeros(9), 1, zeros(3)) == ARG
        assert Lb.g2ohip_pg_set_bearing_edges(s.h, k, _ip(qp), _ip(ql), zeros(1), zeros(1)) == ARG
        assert Lb.g2ohip_pg_set_sensor_calib_edges(s.h, k, kc21[1], kc21[2], _ip(qp), _ip(qc), _ip(qc), zeros(3), None) == ARG
        assert Lb.g2ohip_pg_set_odom_calib_edges(s.h, k, ko[1], ko[2], _ip(qp), _ip(qc), _ip(qc), zeros(3), None) == ARG
    for typ in (2, 10, 12):                                               # pose types that do not fit the bound group
        assert Lb.g2ohip_pg_set_edges(s.h, k0, typ, _ip(vi), _ip(vj), _dp(Zm), _dp(om)) == ARG
    unchanged()
    with pytest.raises(ValueError):
        s.pgSetPointXYCalibEdges(*ids, qp[:-1], ql[:-1], qc[:-1], zm[:-1], zw[:-1])
    # the additive-row rule, in both call orders: a type-22 group whose parameter row is this group's calibration row is refused ...
    # (on a handle of its own: the type-22 sets over the calibration row never get data)
    u = capi.HipBlockSolver(3, 2, 0)
    u0 = u.addEdgeSet(3, h[vi], h[vj])
    uid = _three_sets(u, g)
    e3, crow = np.arange(3), np.full(3, qc[0])
    uo = []
    for (a, b), pt in zip(((h[vi[e3]], h[vj[e3]]), (h[vi[e3]], h[crow]), (h[vj[e3]], h[crow])), (0, 7, 5)):
        uo.append(u.addEdgeSet(3, a, b))
        u.setEdgeSetParts(uo[-1], pt)
    u.buildStructure(g["nP"], g["nL"], True)
    u.pgSetEdges(u0, 1, vi, vj, Zm, om)
    u.pgSetEstimates(g["poses"], h)
    u.pgSetLandmarkEstimates(g["points"], hl)
    assert bind(u, uid) == 0
    u.pointxy_calib_sets = tuple(uid)
    assert bind_odom(u, uo, crow) == ARG
    assert "additive row" in Lb.g2ohip_last_error().decode()
    assert Lb.g2ohip_pg_linearize(u.h, 1) == 0
    for a, b in zip(_data(u, n), ref):
        assert np.array_equal(a, b)
    # ... and while a type-22 group is bound on its own row, this entry refuses that row as a pose or as a calibration vertex
    for name, src in (("a", qp), ("c", qc)):
        bad = src.copy()
        bad[3] = prow
        assert bind(s, ids, m=other, **{name: bad}) == ARG
    unchanged()
    # info = NULL is the identity
    assert bind(s, ids, w=None) == 0
    assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
    ident = _data(s, n)
    assert all(np.array_equal(a, b) for a, b in zip(ident, ref))
    assert bind(s, ids) == 0
    # g2ohip_pg_set_estimates / g2ohip_pg_set_landmark_estimates with changed tables validate the group too
    wrong = h.copy()
    wrong[qc[0]], wrong[1] = wrong[1], wrong[qc[0]]
    assert Lb.g2ohip_pg_set_estimates(s.h, len(h), _dp(_f64(g["poses"])), _ip(wrong)) == ARG
    wrong_l = hl.copy()
    wrong_l[2], wrong_l[3] = wrong_l[3], wrong_l[2]
    assert Lb.g2ohip_pg_set_landmark_estimates(s.h, len(hl), _dp(_f64(g["points"])), _ip(wrong_l)) == ARG
    assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
    for a, b in zip(_data(s, n), ref):
        assert np.array_equal(a, b)
    # the wrapper binds the same group
    s.pgSetPointXYCalibEdges(*ids, qp, ql, qc, zm, zw)
    assert s.pointxy_calib_sets == tuple(ids)
    # update_structure refuses structures with landmarks: the group cannot grow, and the binding still evaluates
    assert not s.updateStructure(0, kpl, h[_i32([1])], hl[_i32([2])])
    assert s.pointxy_calib_sets == tuple(ids)
    assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
    for a, b in zip(_data(s, n), ref):
        assert np.array_equal(a, b)
    # no landmark table: pg_linearize refuses a bound group
    t = capi.HipBlockSolver(3, 2, 0)
    q0 = t.addEdgeSet(3, h[vi], h[vj])
    tid = _three_sets(t, g)
    t.buildStructure(g["nP"], g["nL"], True)
    t.pgSetEdges(q0, 1, vi, vj, Zm, om)
    t.pgSetEstimates(g["poses"], h)
    assert bind(t, tid) == 0
    assert Lb.g2ohip_pg_linearize(t.h, 1) == STATE
    s.clearEdgeSets()
    assert s.pointxy_calib_sets is None
    assert Lb.g2ohip_pg_linearize(s.h, 1) == STATE


def test_wrong_dimensions_unary_and_edge_counts():
    capi = _capi()
    Lb = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = S.make_pointxy_calib_slam(12, 6, seed=4)
    h, hl = _i32(g["hidx"]), _i32(g["pt_hidx"])
    qp, ql, qc = (_i32(g[k]) for k in ("qp", "ql", "qc"))
    t = capi.HipBlockSolver(3, 2, 0)
    q0 = t.addEdgeSet(3, h[g["vi"]], h[g["vj"]])
    tpl, tpc, tlc = _three_sets(t, g)
    k3 = t.addEdgeSet(3, h[qp], hl[ql])                                   # error dimension 3
    ku = t.addEdgeSet(2, h[qp], None)                                     # a unary set
    kcl = t.addEdgeSet(2, h[qc], hl[ql])                                  # (calib, landmark): the other vertex order, parts of set_lc
    t.setEdgeSetParts(kcl, 5)
    kshort = t.addEdgeSet(2, hl[ql[:-1]], h[qc[:-1]])                     # one edge short, the parts of set_lc
    t.setEdgeSetParts(kshort, 5)
    t.buildStructure(g["nP"], g["nL"], True)
    t.pgSetEdges(q0, 1, g["vi"], g["vj"], g["Z"], g["omega"])
    bind = lambda ids: Lb.g2ohip_pg_set_pointxy_calib_edges(t.h, ids[0], ids[1], ids[2], _ip(qp), _ip(ql), _ip(qc), _dp(_f64(g["zq"])), None)
    for bad_ids in ((k3, tpc, tlc), (ku, tpc, tlc), (tpl, tpc, kcl), (tpl, tpc, kshort)):
        assert bind(bad_ids) == ARG, bad_ids
    assert bind((tpl, tpc, tlc)) == 0
    # a pose type other than 1: the same three sets on a (6, 3) handle whose pose set is an EdgeSE3 set
    u = capi.HipBlockSolver(6, 3, 0)
    u0 = u.addEdgeSet(6, h[g["vi"]], h[g["vj"]])
    uid = _three_sets(u, g)
    u.buildStructure(g["nP"], g["nL"], True)
    ne = len(g["vi"])
    u.pgSetEdges(u0, 2, g["vi"], g["vj"], np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), (ne, 1)), np.tile(np.eye(6).reshape(1, -1), (ne, 1)))
    assert Lb.g2ohip_pg_set_pointxy_calib_edges(u.h, uid[0], uid[1], uid[2], _ip(qp), _ip(ql), _ip(qc), _dp(_f64(g["zq"])), None) == ARG
    assert "goes with an EdgeSE2 pose set" in Lb.g2ohip_last_error().decode()


def test_beside_the_others():
    """A type-3 set, a bearing set and a type-21 group bound on the same handle: the group evaluates to the bits it gives alone,
    and so do the others (the system of all four against the system without the group differs; each set's arrays do not)."""
    capi = _capi()
    g = S.make_pointxy_calib_slam(14, 8, seed=3, with_xy=True)
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    n, ne = g["Q"], len(g["vi"])
    zb, wb = np.linspace(-1, 1, n), np.full(n, 4.0)
    crow = np.full(ne, g["calib_row"], np.int32)

    def build(with_group, with_others):
        s = capi.HipBlockSolver(3, 2, 0)
        k0 = s.addEdgeSet(3, h[g["vi"]], h[g["vj"]])
        kxy = s.addEdgeSet(2, h[g["vp"]], hl[g["vl"]]) if with_others else None
        kb = s.addEdgeSet(1, h[g["qp"]], hl[g["ql"]]) if with_others else None
        k21 = []
        if with_others:
            for (a, b), pt in zip(((h[g["vi"]], h[g["vj"]]), (h[g["vi"]], h[crow]), (h[g["vj"]], h[crow])), (0, 7, 5)):
                k21.append(s.addEdgeSet(3, a, b))
                s.setEdgeSetParts(k21[-1], pt)
        ids = _three_sets(s, g) if with_group else None
        s.buildStructure(g["nP"], g["nL"], True)
        s.pgSetEdges(k0, 1, g["vi"], g["vj"], g["Z"], g["omega"])
        s.pgSetEstimates(g["poses"], h)
        if with_others:
            s.pgSetLandmarkEdges(kxy, 3, g["vp"], g["vl"], g["zl"], g["omega_l"], None)
            s.pgSetBearingEdges(kb, g["qp"], g["ql"], zb, wb)
            s.pgSetSensorCalibEdges(*k21, g["vi"], g["vj"], crow, g["Z"], g["omega"])
        if with_group:
            s.pgSetPointXYCalibEdges(*ids, g["qp"], g["ql"], g["qc"], g["zq"], g["omega_q"])
        s.pgSetLandmarkEstimates(g["points"], hl)
        s.pgLinearize(True)
        out = dict(pose=s.edgeData(k0, ne, 3, 3, 3))
        if with_others:
            out.update(xy=s.edgeData(kxy, len(g["vp"]), 2, 3, 2), bearing=s.edgeData(kb, n, 1, 3, 2), c21=s.edgeData(k21[0], ne, 3, 3, 3),
                       c21l=s.edgeData(k21[2], ne, 3, 3, 3))
        if with_group:
            out.update(group=_data(s, n))
        s.buildSystem()
        return out, s.chi2()
    all_, chi_all = build(True, True)
    alone, chi_alone = build(True, False)
    others, chi_others = build(False, True)
    for k in ("pose", "group"):
        assert all(np.array_equal(a, b) for a, b in zip(all_[k], alone[k])), k
    for k in ("pose", "xy", "bearing", "c21", "c21l"):
        assert all(np.array_equal(a, b) for a, b in zip(all_[k], others[k])), k
    e0 = H.pose_edges(g, jac=False)
    chi_pose = float(np.einsum("ni,nij,nj->n", e0, np.asarray(g["omega"]).reshape(-1, 3, 3), e0).sum())
    assert abs(chi_all - (chi_alone + chi_others - chi_pose)) <= 1e-12 * chi_all


def test_from_a_file(tmp_path):
    """written with g2o_io.write_g2o_pointxy_calib, read back, set up: the same device system."""
    g = S.make_pointxy_calib_slam(10, 6, seed=9, with_xy=True)
    path = os.path.join(str(tmp_path), "calib.g2o")
    g2o_io.write_g2o_pointxy_calib(path, g)
    p = g2o_io.pointxy_calib_problem(g2o_io.read_g2o(path))
    out = []
    for q in (g, p):
        s, graph = H.device_setup(q)
        graph.linearize()
        s.buildSystem()
        out.append((s.chi2(), s.b(), s.values(_capi().HPL), _data(s, g["Q"])))
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert all(np.array_equal(a, b) for a, b in zip(out[0][3], out[1][3]))
