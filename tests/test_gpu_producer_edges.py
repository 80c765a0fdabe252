"""GPU: the device producers (pg_se2 / pg_se3 / landmark / BA linearisation), the vertex updates and the robust kernels on
the branch-covering inputs of tests/golden/producer_edges.npz, against the extended-precision reference stored there
(tests/golden/make_producer_edges.py; nothing here evaluates a reference).

Metric (tests/producer_metric.py): per edge and output block, max |got - ref| / max(1, max |ref block|, ops[edge]) with
ops[edge] the fixture's per-edge operand magnitude (translations, positions, angles, measurement, offset; for H / b blocks
the largest sum of the magnitudes of the terms added into an entry).  Bound per output: 8 x the oracle's own worst per-edge
error against the same reference, never above 1e-12; a stated rounding floor only for the four outputs on which the oracle
is exact (producer_metric.bound).  The worst edge of
every comparison is printed with its index (and quaternion case for EdgeSE3) as a PRODUCER_FIGURE line."""
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm
from tests import producer_metric as PM

pytestmark = pytest.mark.gpu

FX = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "producer_edges.npz")))
TAILS = (1, 255, 256, 257, 513)


def _capi():
    from openslam_g2o_amd import capi
    return capi


def check(key, got, ref=None, ops=None, what="", tag=None):
    ref = FX[key] if ref is None else ref
    fig, k = PM.worst(got, ref, ops)
    b = PM.bound(FX, key)
    rec = dict(output=key, who="device", case=what, worst_per_edge=fig, edge=k, bound=b)
    if tag is not None:
        rec["branch"] = tag(k)
    print("PRODUCER_FIGURE", json.dumps(rec))
    assert fig <= b, rec
    return fig


def _eye(n, d):
    return np.tile(np.eye(d).reshape(1, d * d), (n, 1))


def _error_only_leaves_jacobians(s, k, shape, J0, J1, err, x, moved=None):
    """pgLinearize(False) at CHANGED estimates (push, update by x): the Jacobian arrays keep the values written before, the
    errors change; back at the old estimates (pop) the error-only evaluation gives the first errors bit for bit."""
    before = s.pgGetEstimates()
    s.setX(x)
    s.pgPush()
    s.pgUpdate()
    assert not np.array_equal(s.pgGetEstimates(), before)
    if moved is not None:
        moved()
    s.pgLinearize(False)
    xJ0, xJ1, xerr = s.edgeData(k, *shape)
    assert np.array_equal(xJ0, J0) and np.array_equal(xJ1, J1) and not np.array_equal(xerr, err)
    s.pgPop()
    assert np.array_equal(s.pgGetEstimates(), before)
    s.pgLinearize(False)
    xJ0, xJ1, xerr = s.edgeData(k, *shape)
    assert np.array_equal(xJ0, J0) and np.array_equal(xJ1, J1) and np.array_equal(xerr, err)


def _pose_graph(pre, etype, d):
    capi = _capi()
    hidx, vi, vj = FX[pre + "_hidx"], FX[pre + "_vi"], FX[pre + "_vj"]
    s = capi.HipBlockSolver(d, 2 if d == 3 else 3, 0)
    k = s.addEdgeSet(d, hidx[vi], hidx[vj])
    s.buildStructure(int(hidx.max()) + 1, 0, False)
    s.pgSetEdges(k, etype, vi, vj, FX[pre + "_Z"], _eye(len(vi), d))
    s.pgSetEstimates(FX[pre + "_poses"], hidx)
    return s, k, len(vi)


@pytest.mark.parametrize("pre,etype,d", [("se3", 2, 6), ("se2", 1, 3)])
def test_pose_pose_producers_on_every_branch(pre, etype, d):
    s, k, n = _pose_graph(pre, etype, d)
    s.pgLinearize(True)
    J0, J1, err = s.edgeData(k, n, d, d, d)
    tag = (lambda e: "case%d/qw%s" % (FX["se3_case"][e], "+" if FX["se3_sign"][e] > 0 else "-")) if pre == "se3" else None
    ops = FX[pre + "_ops"]
    check(pre + "_err", err, ops=ops, tag=tag)
    check(pre + "_J0", J0, ops=ops, tag=tag)
    check(pre + "_J1", J1, ops=ops, tag=tag)
    if pre == "se3":      # ... and every (case, sign) group on its own, so that the printed worst edges cover all seven
        for c in range(4):
            for sg in (1, -1):
                sel = np.nonzero((FX["se3_case"] == c) & (FX["se3_sign"] == sg))[0]
                assert len(sel) >= 12 or (c == 0 and sg == -1 and len(sel) == 0)
                if len(sel):
                    what = "case%d/qw%s" % (c, "+" if sg > 0 else "-")
                    check("se3_J0", J0[sel], FX["se3_J0"][sel], ops[sel], what)
                    check("se3_J1", J1[sel], FX["se3_J1"][sel], ops[sel], what)
    _error_only_leaves_jacobians(s, k, (n, d, d, d), J0, J1, err, 0.01 * np.random.RandomState(7).normal(size=s.vectorSize()))


@pytest.mark.parametrize("pre", ["lm2", "lm3"])
@pytest.mark.parametrize("staged", [1, 0])
@pytest.mark.parametrize("n", TAILS)
def test_landmark_producers_tails_and_store_forms(pre, staged, n):
    capi = _capi()
    se2 = pre == "lm2"
    p, l = (3, 2) if se2 else (6, 3)
    hidx, pt_hidx = FX[pre + "_hidx"], FX[pre + "_pt_hidx"]
    vi, vj, vp, vl = FX[pre + "_vi"], FX[pre + "_vj"], FX[pre + "_vp"][:n], FX[pre + "_vl"][:n]
    nP, nL = int(hidx.max()) + 1, int(pt_hidx.max()) + 1 - (int(hidx.max()) + 1)
    s = capi.HipBlockSolver(p, l, 0)
    k0 = s.addEdgeSet(p, hidx[vi], hidx[vj])
    k1 = s.addEdgeSet(l, hidx[vp], pt_hidx[vl])
    s.buildStructure(nP, nL, True)
    s.pgSetEdges(k0, 1 if se2 else 2, vi, vj, FX[pre + "_Z"], _eye(len(vi), p))
    s.pgSetEstimates(FX[pre + "_poses"], hidx)
    s.pgSetLandmarkEdges(k1, 3 if se2 else 4, vp, vl, FX[pre + "_zl"][:n], _eye(n, l), None if se2 else FX["lm3_offset"])
    s.pgSetLandmarkEstimates(FX[pre + "_points"], pt_hidx)
    s.setOption("pg_landmark_staged", staged)
    s.pgLinearize(True)
    J0, J1, err = s.edgeData(k1, n, l, p, l)
    ops, what = FX[pre + "_ops"][:n], "staged=%d n=%d" % (staged, n)
    check(pre + "_err", err, FX[pre + "_err"][:n], ops, what)
    check(pre + "_J0", J0, FX[pre + "_J0"][:n], ops, what)
    check(pre + "_J1", J1, FX[pre + "_J1"][:n], ops, what)
    # the vertex update of the landmark graph (points: pg_points_update_kernel) inside the error-only check
    pts = FX[pre + "_points"]

    def moved():
        got = s.pgGetLandmarkEstimates()
        check("upd_%s_pts" % pre, got, ops=FX["upd_%s_pts_ops" % pre], what=what)
        fixed = np.nonzero(pt_hidx < 0)[0]
        assert len(fixed) == 3 and np.array_equal(got[fixed], pts[fixed])
        assert np.array_equal(s.pgGetEstimates()[0], FX[pre + "_poses"][0])          # the fixed pose
    _error_only_leaves_jacobians(s, k1, (n, l, p, l), J0, J1, err, FX["upd_%s_x" % pre], moved)
    assert np.array_equal(s.pgGetLandmarkEstimates(), pts)


def _ba_problem(pre):
    cam_idx, pt_idx, cam_hidx = FX["ba_cam_idx"], FX["ba_pt_idx"], FX["ba_cam_hidx"]
    nP, L = int(cam_hidx.max()) + 1, len(FX["ba_pts"])
    f, cx, cy = FX["ba_classes"][0, :3]
    return dict(P=len(cam_hidx), L=L, E=len(cam_idx), nP=nP, nL=L, f=float(f), cx=float(cx), cy=float(cy), cams=FX["ba_cams"],
                pts=FX["ba_pts"], meas=FX[pre + "_meas"], cam_idx=cam_idx, pt_idx=pt_idx, cam_hidx=cam_hidx,
                v0=(nP + pt_idx).astype(np.int32), v1=cam_hidx[cam_idx].astype(np.int32))


def _check_ba_system(pre, s, pr, what):
    capi = _capi()
    nP, L, E = pr["nP"], pr["L"], pr["E"]
    edge_of = {(int(pr["v1"][e]), int(pr["pt_idx"][e])): e for e in range(E) if pr["v1"][e] >= 0}
    assert len(edge_of) == int((pr["v1"] >= 0).sum())              # one edge per (camera, point) pair
    cp, ri = s.pattern(capi.HPL)
    V = s.values(capi.HPL).reshape(-1, 18)
    assert len(V) == len(edge_of)
    got = np.zeros((E, 18))
    for c in range(L):
        for q in range(cp[c], cp[c + 1]):
            got[edge_of[(int(ri[q]), c)]] = V[q]
    check(pre + "_Hpl", got, ops=FX[pre + "_Hpl_ops"], what=what)
    check(pre + "_Hll", s.values(capi.HLL).reshape(L, 9), ops=FX[pre + "_Hll_ops"], what=what)
    cp, ri = s.pattern(capi.HPP)
    V = s.values(capi.HPP).reshape(-1, 36)
    diag = np.array([V[[q for q in range(cp[c], cp[c + 1]) if ri[q] == c][0]] for c in range(nP)])
    check(pre + "_Hpp", diag, ops=FX[pre + "_Hpp_ops"], what=what)
    check(pre + "_b", s.b().reshape(-1, 1), FX[pre + "_b"].reshape(-1, 1), FX[pre + "_b_ops"], what)
    check(pre + "_chi2", np.array([[s.chi2()]]), np.array([[float(FX[pre + "_chi2"])]]), np.array([float(FX[pre + "_chi2_ops"])]), what)


@pytest.mark.parametrize("fuse_landmarks", [1, 0])
def test_ba_fused_path_with_edge_classes(fuse_landmarks):
    """Edge classes exist on the fused path only (build_system refuses a class table with ba_fused = 0), so the class set
    has no materialised Jacobians to compare; ba_linearize_edge is held by the one-class set below."""
    capi = _capi()
    pr = _ba_problem("ba")
    s = capi.HipBlockSolver(6, 3, 0)
    s.setOption("ba_fused", 1)
    s.setOption("ba_fuse_landmarks", fuse_landmarks)
    k = s.addEdgeSet(2, pr["v0"], pr["v1"])
    s.buildStructure(pr["nP"], pr["nL"], True)
    s.baSetEdgesClasses(k, pr["cam_idx"], pr["pt_idx"], pr["meas"], FX["ba_classes"], FX["ba_edge_class"])
    s.baSetEstimates(pr["cams"], pr["cam_hidx"], pr["pts"], np.arange(pr["L"], dtype=np.int32))
    lm.DeviceBAGraph(s).linearize()
    s.buildSystem()
    _check_ba_system("ba", s, pr, "classes fuse_landmarks=%d" % fuse_landmarks)


@pytest.mark.parametrize("fused,fuse_landmarks", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_ba_one_class_fused_and_materialised(fused, fuse_landmarks):
    pr = _ba_problem("ba1")
    s, graph = lm.setup_device_ba(pr, huber_delta=float(FX["ba1_huber"]), options={"ba_fused": fused, "ba_fuse_landmarks": fuse_landmarks})
    graph.linearize()
    what = "fused=%d fuse_landmarks=%d" % (fused, fuse_landmarks)
    if not fused:                                                   # the materialised Jacobians of ba_linearize_edge
        J0, J1, err = s.edgeData(0, pr["E"], 2, 3, 6)
        check("ba1_err", err, ops=FX["ba1_ops"], what=what)
        check("ba1_J0", J0, ops=FX["ba1_ops"], what=what)
        check("ba1_J1", J1, ops=FX["ba1_ops"], what=what)
    s.buildSystem()
    _check_ba_system("ba1", s, pr, what)


def test_vertex_updates_on_every_branch():
    capi = _capi()
    for pre, etype, d in (("upd_se3", 2, 6), ("upd_se2", 1, 3)):
        poses, hidx, x = FX[pre + "_poses"], FX[pre + "_hidx"], FX[pre + "_x"]
        free = np.nonzero(hidx >= 0)[0].astype(np.int32)
        s = capi.HipBlockSolver(d, 2 if d == 3 else 3, 0)
        k = s.addEdgeSet(d, hidx[free[:1]], hidx[free[1:2]])
        s.buildStructure(len(free), 0, False)
        s.pgSetEdges(k, etype, free[:1], free[1:2], poses[:1, :(3 if d == 3 else 12)], _eye(1, d))
        s.pgSetEstimates(poses, hidx)
        s.setX(x)
        s.pgPush()
        s.pgUpdate()
        got = s.pgGetEstimates()
        check(pre, got, ops=FX[pre + "_ops"])
        fixed = np.nonzero(hidx < 0)[0]
        assert len(fixed) and np.array_equal(got[fixed], poses[fixed])
        s.pgPop()
        assert np.array_equal(s.pgGetEstimates(), poses)
    cams, hc, pts, hp = FX["upd_cam_cams"], FX["upd_cam_hidx"], FX["upd_pts_pts"], FX["upd_pts_hidx"]
    nc, npt = len(hc), len(hp)
    cam_idx = np.arange(nc, dtype=np.int32)
    pt_idx = (cam_idx % npt).astype(np.int32)
    nP, nL = nc - 1, npt - 1
    s = capi.HipBlockSolver(6, 3, 0)
    k = s.addEdgeSet(2, np.where(hp[pt_idx] >= 0, nP + hp[pt_idx], -1).astype(np.int32), hc[cam_idx])
    s.buildStructure(nP, nL, True)
    s.baSetEdges(k, cam_idx, pt_idx, np.zeros((nc, 2)), None)
    s.baSetEstimates(cams, hc, pts, hp)
    s.setX(np.concatenate([FX["upd_cam_x"], FX["upd_pts_x"]]))
    s.baPush()
    s.baUpdate()
    gc, gp = s.baGetEstimates()
    check("upd_cam", gc, ops=FX["upd_cam_ops"])
    check("upd_pts", gp, ops=FX["upd_pts_ops"])
    assert np.array_equal(gc[0], cams[0]) and np.array_equal(gp[0], pts[0])
    s.baPop()
    bc, bp = s.baGetEstimates()
    assert np.array_equal(bc, cams) and np.array_equal(bp, pts)


@pytest.mark.parametrize("run", ["edge", "set1", "set2", "set3", "set4", "set5"])
def test_robust_kernels_on_both_sides_of_and_exactly_at_the_threshold(run):
    capi = _capi()
    J0, J1, err = FX["rob_J0"], FX["rob_J1"], FX["rob_err"]
    n = len(err)
    v0, v1 = np.arange(0, 2 * n, 2, dtype=np.int32), np.arange(1, 2 * n, 2, dtype=np.int32)
    s = capi.HipBlockSolver(3, 2, 0)
    k = s.addEdgeSet(3, v0, v1)
    s.buildStructure(2 * n, 0, False)
    s.setEdgeData(k, J0, J1, _eye(n, 3), err)
    if run == "edge":
        s.setRobustKernelPerEdge(k, FX["rob_kinds"], FX["rob_deltas"])
    else:
        s.setRobustKernel(k, int(run[3:]), float(FX["rob_set_delta"]))
    s.buildSystem()
    cp, ri = s.pattern(capi.HPP)
    V = s.values(capi.HPP).reshape(-1, 9)
    diag = np.array([V[[q for q in range(cp[c], cp[c + 1]) if ri[q] == c][0]] for c in range(2 * n)])
    pre = "rob_%s_" % run
    z = np.zeros(2 * n)
    for key, got, ref in (("rob_Hpp", diag, FX[pre + "Hpp"]), ("rob_b", s.b().reshape(2 * n, 3), FX[pre + "b"].reshape(2 * n, 3)),
                          ("rob_chi2", np.array([[s.chi2()]]), np.array([[float(FX[pre + "chi2"])]]))):
        check(key, got, ref, z[:len(ref)], run)
