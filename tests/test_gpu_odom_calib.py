"""GPU: odometry self-calibration on the device (EdgeSE2OdomDifferentialCalib = type 22 beside an EdgeSE2 set that may be empty,
g2ohip_pg_set_odom_calib_edges): the producer against the fp64 restatement of openslam_g2o_amd/odom_calib.py within 8 x that
restatement's recorded drift against 60 digits (tests/golden/odom_calib_edges.npz), tails, both store forms, the error-only
evaluation, fixed vertices, vertex indexing; the additive rows of the pose table in g2ohip_pg_update; the assembled system and its
solution against the CPU oracle's three-vertex edges, alone, beside a type-21 group and with two parameter vertices; a
Levenberg-Marquardt run against the host-fed one; the binding rules; a graph from a file."""
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io, lm, odom_calib as OC, synthetic as S
from tests import calib_helpers as CH
from tests import odom_calib_helpers as H
from tests.helpers import relerr
from tests.test_gpu_sensor_calib import PCG, TOL_B, TOL_H, TOL_X, _dense_pp

pytestmark = pytest.mark.gpu

Z = np.load(H.GOLDEN)
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _data(s, n):
    """(Ji, Jj, Jp, err) as the next buildSystem reads them; the three sets must show the SAME shared arrays."""
    kij, kip, kjp = s.odom_calib_sets
    Ji, Jj, err = s.edgeData(kij, n, 3, 3, 3)
    Ji2, Jp, err2 = s.edgeData(kip, n, 3, 3, 3)
    Jj3, Jp3, err3 = s.edgeData(kjp, n, 3, 3, 3)
    assert np.array_equal(Ji, Ji2) and np.array_equal(Jj, Jj3) and np.array_equal(Jp, Jp3)
    assert np.array_equal(err, err2) and np.array_equal(err, err3)
    return Ji, Jj, Jp, err


def _within(tag, dev, ref, drift):
    """device against the restatement, per array (err, Ji, Jj, Jp): 8 x the recorded drift of that array."""
    fig = [np.abs(dev[k] - ref[k]).max() for k in (3, 0, 1, 2)]
    print(tag, "device vs restatement (err, Ji, Jj, Jp)", fig, "bound", H.DRIFT_FACTOR * np.asarray(drift))
    for f, b in zip(fig, drift):
        assert f <= H.DRIFT_FACTOR * b, (tag, fig, drift)


@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_producer_tails(n):
    row = H.EDGE_COUNTS.index(n)
    g = H.load_graph(Z, n)
    s, graph = H.device_setup(g)
    graph.linearize()
    ref = H.producers(H.FP64, g)
    dev = _data(s, n)
    _within("odom calib %d" % n, dev, ref, Z["drift"][row])
    fixed_i, fixed_j = g["oi"] == 0, g["oj"] == 0
    assert not dev[0][fixed_i].any() and not dev[1][fixed_j].any()                 # the blocks of the fixed pose: zeros
    s.buildSystem()
    c_ref = OC.chi2(ref[3], g["oinfo"])
    assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref
    # the other store form: the same bits
    s.setOption("pg_landmark_staged", 0)
    s.pgSetEstimates(g["poses"], g["hidx"])
    s.pgLinearize(True)
    for a, b in zip(dev, _data(s, n)):
        assert np.array_equal(a, b)
    # an error-only evaluation after an update leaves J and gives the errors of the moved table, in both store forms
    for staged in (0, 1):
        s.setOption("pg_landmark_staged", staged)
        s.pgSetEstimates(g["poses"], g["hidx"])
        s.pgLinearize(True)
        s.buildSystem()
        s.setX(Z["moved_x"])
        s.pgUpdate()
        s.pgLinearize(False)
        moved = s.pgGetEstimates()
        assert np.abs(moved - Z["moved_poses"]).max() < 1e-14
        e_ref = H.producers(H.FP64, g, poses=moved, jac=False)
        after = _data(s, n)
        assert all(np.array_equal(after[k], dev[k]) for k in range(3))
        fig = np.abs(after[3] - e_ref).max()
        print(n, "moved: device vs restatement", fig, "bound", H.DRIFT_FACTOR * Z["moved_drift"][row])
        assert fig <= H.DRIFT_FACTOR * Z["moved_drift"][row]
        assert np.abs(after[3] - dev[3]).max() > 1e-3


@pytest.mark.parametrize("fixed", ["i", "j", "p"])
def test_fixed_vertex_blocks_are_zero(fixed):
    """One vertex kind fixed at a time: pose 2 (vertex 0 of some edges), pose 3 (vertex 1 of some), the first parameter vertex."""
    g = H.load_graph(Z, 65)
    row = dict(i=2, j=3, p=H.PARAM_ROW)[fixed]
    hidx, nP = g2o_io.hessian_index(g["n"], [0, row])
    g = dict(g, hidx=hidx, nP=nP)
    s, graph = H.device_setup(g)
    graph.linearize()
    dev, ref = _data(s, 65), H.producers(H.FP64, g)
    _within("fixed " + fixed, dev, ref, Z["drift"][H.EDGE_COUNTS.index(65)])
    col = dict(i="oi", j="oj", p="op")[fixed]
    k = "ijp".index(fixed)
    hit = g[col] == row
    assert hit.any() and not dev[k][hit].any() and dev[k][~hit & (g[col] != 0)].any(axis=1).all()
    others = [a for a in range(3) if a != k]
    assert all(dev[a][hit & (g["oi"] != 0) & (g["oj"] != 0)].any(axis=1).all() for a in others)


def test_index_permutation():
    """Shuffled edge order gives shuffled output, and the rows of the graph scattered over a larger table give the same bits."""
    n = 65
    g = H.load_graph(Z, n)
    s, graph = H.device_setup(g)
    graph.linearize()
    ref = _data(s, n)
    rng = np.random.default_rng(11)
    perm = rng.permutation(n)
    sp, graph_p = H.device_setup(H.take_edges(g, perm))
    graph_p.linearize()
    for a, b in zip(_data(sp, n), ref):
        assert np.array_equal(a, b[perm])
    where = rng.permutation(40)[:8].astype(np.int32)           # new row of old row r
    poses = rng.normal(size=(40, 3)) * 5.0
    poses[where] = g["poses"]
    hidx = np.full(40, -1, np.int32)
    hidx[where] = g["hidx"]
    gw = dict(g, poses=poses, hidx=hidx, n=40, oi=where[g["oi"]], oj=where[g["oj"]], op=where[g["op"]], param_rows=where[g["param_rows"]])
    sw, graph_w = H.device_setup(gw)
    graph_w.linearize()
    for a, b in zip(_data(sw, n), ref):
        assert np.array_equal(a, b)


def _update_graph():
    """4 rows: pose 0 fixed, poses 1 and 2, the parameter vertex (k_l, k_r, b = 4.0 > pi) in row 3; two edges."""
    poses = np.array([[0.0, 0.0, 0.1], [1.0, 0.2, 3.0], [2.0, -0.3, -1.0], [1.1, 0.9, 4.0]])
    return dict(kind="se2", n=4, nP=3, poses=poses, hidx=np.array([-1, 0, 1, 2], np.int32), vi=np.zeros(0, np.int32), vj=np.zeros(0, np.int32),
                Z=np.zeros((0, 3)), omega=np.zeros((0, 9)), oi=np.array([0, 1], np.int32), oj=np.array([1, 2], np.int32),
                op=np.array([3, 3], np.int32), omeas=np.array([[0.5, 0.7, 1.0], [0.6, 0.6, 0.8]]), oinfo=np.tile(np.eye(3).reshape(1, 9), (2, 1)),
                param_rows=np.array([3], np.int32))


def test_update_adds_on_parameter_rows_and_wraps_on_pose_rows():
    """One g2ohip_pg_update: the parameter row (b = 4.0, beyond pi) takes its whole step, component 2 included; the pose row whose
    angle crosses pi ends wrapped.  A kernel that ignores the mask wraps 4.0 + u to 4.0 + u - 2 pi.  Push, update, pop restores both
    bit for bit; after the group is released the same table wraps the row again."""
    g = _update_graph()
    s, graph = H.device_setup(g)
    graph.linearize()
    s.buildSystem()
    x = np.array([0.1, -0.2, 0.25, 0.0, 0.0, 0.0, 0.01, -0.02, 0.125])        # pose 1: 3.0 + 0.25 > pi; the parameter row: 4.0 + 0.125
    before = s.pgGetEstimates()
    s.pgPush()
    s.setX(x)
    s.pgUpdate()
    after = s.pgGetEstimates()
    print("parameter row", after[3], "pose row", after[1])
    assert after[3, 2] == 4.0 + 0.125 and after[3, 0] == 1.1 + 0.01 and after[3, 1] == 0.9 + -0.02
    assert after[1, 2] == OC.normalize_theta(OC.FP64, 3.0 + 0.25) and after[1, 2] < 0
    assert np.array_equal(after, H.oplus(g, before, x)) and np.array_equal(after[[0, 2]], before[[0, 2]])
    s.pgPop()
    assert np.array_equal(s.pgGetEstimates(), before)
    # released: the same handle, the same table, no group -- row 3 is a VertexSE2 again
    s.clearEdgeSets()
    h = g["hidx"]
    k0 = s.addEdgeSet(3, h[np.array([1, 2])], h[np.array([2, 3])])      # (row 3 as the VertexSE2 of an EdgeSE2)
    s.buildStructure(3, 0, False)
    s.pgSetEdges(k0, 1, [1, 2], [2, 3], [[1.0, 0.0, 0.0], [0.5, 0.0, 0.1]], np.tile(np.eye(3).reshape(1, 9), (2, 1)))
    s.pgSetEstimates(g["poses"], h)
    s.pgLinearize(True)
    s.buildSystem()
    s.setX(x)
    s.pgUpdate()
    wrapped = s.pgGetEstimates()
    assert wrapped[3, 2] == OC.normalize_theta(OC.FP64, 4.0 + 0.125) and wrapped[3, 2] < 0
    assert np.array_equal(wrapped[:3], after[:3])


def _check_system(s, g, huber, tag):
    o, m, mc = H.oracle_graph(g)
    H.feed_oracle(g, o, m, mc, huber)
    s.buildSystem()
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    fig = dict(Hpp=relerr(_dense_pp(s), o.dense_full()), dx=relerr(s.x(), o.x()))
    print(tag, fig)
    assert fig["Hpp"] < TOL_H and fig["dx"] < TOL_X


def _system_graph(case):
    if case == "alone":                      # the group alone beside a zero-edge pose set
        g = S.make_calib_rig(40, loops=0, seed=2, odom_calib=True)
        return {k: v for k, v in H.without_odometry(g).items() if k not in ("ci", "cj", "cl", "cmeas", "cinfo")} | dict(
            hidx=np.concatenate([g["hidx"][:40], [-1], [39]]).astype(np.int32), nP=40)
    if case in ("both", "both_offset_fixed"):   # the example's graph: both groups, no EdgeSE2
        g = H.without_odometry(S.make_calib_rig(40, loops=21, seed=2, wrap_every=10, odom_calib=True))
        if case == "both_offset_fixed":
            hidx, nP = g2o_io.hessian_index(g["n"], [0, g["offset_row"]])
            poses = g["poses"].copy()
            poses[g["offset_row"]] = g["offset_true"]
            g = dict(g, hidx=hidx, nP=nP, poses=poses)
        return g
    return H.without_odometry(S.make_calib_rig(40, loops=21, seed=2, odom_calib=True, n_params=2))   # two robots


@pytest.mark.parametrize("solver", ["direct", "pcg"])
@pytest.mark.parametrize("case", ["alone", "both", "both_offset_fixed", "two_params"])
@pytest.mark.parametrize("huber", [0.0, 12.0])
def test_assembled_system_against_oracle(huber, case, solver):
    """H, b, chi2 and the solved x against OracleSolver(schur=False) fed the fp64 restatements through add_multi_edge_set (one
    multi-edge set per group), at the tolerances of tests/test_gpu_sensor_calib.py; no EdgeSE2 in any of the graphs."""
    g = _system_graph(case)
    assert len(g["vi"]) == 0 and len(g["oi"]) == 39
    s, graph = H.device_setup(g, huber=huber, options=PCG if solver == "pcg" else None)
    assert len(s.odom_calib_sets) == 3 and (s.calib_sets is None) == (case == "alone")
    graph.linearize()
    _check_system(s, g, huber, "huber %g %s %s" % (huber, case, solver))
    dev = _data(s, 39)
    fixed = np.asarray(g["hidx"]) < 0
    assert not dev[0][fixed[g["oi"]]].any() and not dev[1][fixed[g["oj"]]].any() and dev[2].any(axis=1).all()


class HostFedGraph:
    """The graph protocol of openslam_g2o_amd.lm over ONE library handle whose odometry-calibration sets are ordinary edge sets fed
    from the host through g2ohip_set_edge_data: every evaluation reads the table back and evaluates odom_calib.py in fp64.  The
    table, the type-21 group and the update (additive on the parameter rows: the group is NOT bound here, so the host applies the
    step) stay as they are."""

    def __init__(self, s, g, ids):
        self.s, self.g, self.ids, self.J, self.stack = s, g, ids, None, []

    def _feed(self, jac):
        self.s.pgLinearize(jac)
        poses = self.s.pgGetEstimates()
        if jac:
            Ji, Jj, Jp, err = H.producers(H.FP64, self.g, poses)
            self.J = (Ji, Jj, Jp)
        else:
            err = H.producers(H.FP64, self.g, poses, jac=False)
        Ji, Jj, Jp = self.J
        for k, (A, B) in zip(self.ids, ((Ji, Jj), (Ji, Jp), (Jj, Jp))):
            self.s.setEdgeData(k, A, B, self.g["oinfo"], err)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()

    def update(self):
        self.s.pgSetEstimates(H.oplus(self.g, self.s.pgGetEstimates(), self.s.x()), self.g["hidx"])

    def push(self):
        self.stack.append(self.s.pgGetEstimates())

    def pop(self):
        self.s.pgSetEstimates(self.stack.pop(), self.g["hidx"])

    def discard_top(self):
        self.stack.pop()


def _host_fed(g):
    """the type-21 group device-resident, the new group's three sets host-fed"""
    capi = _capi()
    h = np.asarray(g["hidx"], np.int32)
    sh = capi.HipBlockSolver(3, 2, 0)
    q0 = sh.addEdgeSet(3, h[g["vi"]], h[g["vj"]])
    parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
    kc, ko = [], []
    for ids, cols in ((kc, ("ci", "cj", "cl")), (ko, ("oi", "oj", "op"))):
        a, b, c = (g[k] for k in cols)
        for (u, v), pt in zip(((a, b), (a, c), (b, c)), parts):
            ids.append(sh.addEdgeSet(3, h[u], h[v]))
            sh.setEdgeSetParts(ids[-1], pt)
    sh.buildStructure(g["nP"], 0, False)
    sh.pgSetEdges(q0, 1, g["vi"], g["vj"], g["Z"], g["omega"])
    sh.pgSetEstimates(g["poses"], h)
    sh.pgSetSensorCalibEdges(*kc, g["ci"], g["cj"], g["cl"], g["cmeas"], g["cinfo"])
    return sh, HostFedGraph(sh, g, ko)


def test_lm_run_device_resident_against_host_fed():
    """LM twice through the same library over the example's graph (60 poses, 89 scan matches, 59 odometry-calibration edges, no
    EdgeSE2), ten iterations from a damping of LM_LAMBDA_INIT (odom_calib_helpers: every one of the ten then descends): device-resident, and with the new group's three sets host-fed from odom_calib.py and the additive
    update applied on the host.  Equal trial counts; the chi2 gap of every iteration within the type-21 LM test's bound (8 x the
    largest gap between two equally valid CPU runs recorded in tests/golden/sensor_calib_edges.npz).  The recovered (k_l, k_r, b)
    moves from (1, 1, 1) to within 5 sigma of the generator's truth, sigma from the parameter vertex's covariance block (its
    block of the inverse of the undamped Hpp at the result, from g2ohip_compute_marginals)."""
    g = H.without_odometry(H.lm_graph())
    s, graph = H.device_setup(g)
    n_dev, chi_dev, _, tr_dev = lm.optimize(graph, s, H.LM_ITERATIONS, "lm", user_lambda_init=H.LM_LAMBDA_INIT)
    sh, host = _host_fed(g)
    n_host, chi_host, _, tr_host = lm.optimize(host, sh, H.LM_ITERATIONS, "lm", user_lambda_init=H.LM_LAMBDA_INIT)
    gaps = [abs(a - b) / b for a, b in zip(chi_dev, chi_host)]
    bound = H.DRIFT_FACTOR * float(np.load(CH.GOLDEN)["lm_gap"].max())
    print("lm chi2 device", chi_dev)
    print("lm chi2 host-fed", chi_host)
    print("lm gaps", gaps, "bound", bound, "trials", tr_dev, tr_host)
    assert n_dev == n_host == H.LM_ITERATIONS
    assert [int(t) for t in tr_dev] == [int(t) for t in tr_host]
    for it, gap in enumerate(gaps):
        assert gap <= bound, (it, gap, bound)
    assert (np.diff(chi_dev) < 0).all() and [int(t) for t in tr_dev] == [1] * H.LM_ITERATIONS   # (every iteration descends: helpers)
    est = s.pgGetEstimates()
    row = int(g["param_rows"][0])
    hp = int(g["hidx"][row])
    graph.linearize()
    s.buildSystem()
    cov = s.computeMarginals([hp], [hp])                                  # g2ohip_compute_marginals: the block of the inverse of Hpp
    assert cov is not None
    cov = cov[0]
    dense = np.linalg.inv(_dense_pp(s))[3 * hp:3 * hp + 3, 3 * hp:3 * hp + 3]
    assert np.abs(cov - dense).max() <= 1e-9 * np.abs(dense).max()       # (the bound of tests/test_gpu_marginals.py)
    sigma = np.sqrt(np.diag(cov))
    d1, d0 = np.abs(est[row] - g["params_true"][0]), np.abs(1.0 - g["params_true"][0])
    print("parameters", est[row], "truth", g["params_true"][0], "sigma", sigma, "error / sigma", d1 / sigma)
    assert (d1 <= 5.0 * sigma).all() and (d1 < d0).all()


def test_use_graph_replays_match():
    g = _system_graph("both")
    out = []
    for use_graph in (0, 1):
        s, graph = H.device_setup(g, options={"use_graph": use_graph})
        done, chis, _, tr = lm.optimize(graph, s, 3, "lm")
        out.append((chis, [int(t) for t in tr], s.pgGetEstimates()))
    assert out[0][1] == out[1][1] and np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2])


def test_binding_rules():
    capi = _capi()
    Lb = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = S.make_calib_rig(12, loops=5, seed=4, odom_calib=True)
    n, nc = len(g["oi"]), len(g["ci"])
    h = _i32(g["hidx"])
    P = int(g["param_rows"][0])
    vi, vj, oi, oj, op, ci, cj, cl = (_i32(g[k]) for k in ("vi", "vj", "oi", "oj", "op", "ci", "cj", "cl"))
    Zm, om, zm, zw, cm, cw = (_f64(g[k]) for k in ("Z", "omega", "omeas", "oinfo", "cmeas", "cinfo"))
    parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)

    def three(s, a, b, c):
        ids = []
        for (u, v), pt in zip(((a, b), (a, c), (b, c)), parts):
            ids.append(s.addEdgeSet(3, h[u], h[v]))
            s.setEdgeSetParts(ids[-1], pt)
        return ids

    def bind(s, ids, a=oi, b=oj, c=op, m=zm, w=zw):
        p = lambda x, fn: None if x is None else fn(x)
        return Lb.g2ohip_pg_set_odom_calib_edges(s.h, ids[0], ids[1], ids[2], p(a, _ip), p(b, _ip), p(c, _ip), p(m, _dp), p(w, _dp))

    def bind21(s, ids, a=ci, b=cj, c=cl):
        return Lb.g2ohip_pg_set_sensor_calib_edges(s.h, ids[0], ids[1], ids[2], _ip(a), _ip(b), _ip(c), _dp(cm), _dp(cw))

    s = capi.HipBlockSolver(3, 2, 0)
    k0 = s.addEdgeSet(3, h[vi], h[vj])
    ids = three(s, oi, oj, op)
    cids = three(s, ci, cj, cl)
    kpr = s.addEdgeSet(3, h[_i32([P])], None)                              # a prior on the parameter row
    kpr2 = s.addEdgeSet(3, h[_i32([2])], None)                             # a prior on pose 2
    assert bind(s, ids) == STATE                                          # before g2ohip_build_structure
    s.buildStructure(g["nP"], 0, False)
    assert bind(s, ids) == STATE                                          # no type-1 set bound
    s.pgSetEdges(k0, 1, vi, vj, Zm, om)
    s.pgSetEstimates(g["poses"], h)
    s.setRobustKernelPerEdge(ids[1], np.full(n, capi.KERNEL_HUBER, np.int32), np.ones(n))
    assert bind(s, ids) == STATE                                          # per-edge robust kernels at binding
    s.setRobustKernelPerEdge(ids[1], None, None)
    one = lambda c: _dp(_f64(np.zeros((1, c))))
    eye = _dp(_f64(np.eye(3).reshape(1, 9)))
    # row kinds, first order: a prior bound on a pose row does not refuse the group, one on the parameter row does (the prior
    # slot holds one set: the second call replaces the first)
    assert Lb.g2ohip_pg_set_prior_edges(s.h, kpr2, 7, _ip(_i32([2])), one(3), eye, None) == 0
    assert bind(s, ids) == 0
    s.clearEdgeSets()
    k0 = s.addEdgeSet(3, h[vi], h[vj])
    ids = three(s, oi, oj, op)
    kpr = s.addEdgeSet(3, h[_i32([P])], None)
    s.buildStructure(g["nP"], 0, False)
    s.pgSetEdges(k0, 1, vi, vj, Zm, om)
    s.pgSetEstimates(g["poses"], h)
    assert Lb.g2ohip_pg_set_prior_edges(s.h, kpr, 7, _ip(_i32([P])), one(3), eye, None) == 0
    assert bind(s, ids) == ARG
    s.clearEdgeSets()
    k0 = s.addEdgeSet(3, h[vi], h[vj])
    ids = three(s, oi, oj, op)
    cids = three(s, ci, cj, cl)
    s.buildStructure(g["nP"], 0, False)
    s.pgSetEdges(k0, 1, vi, vj, Zm, om)
    s.pgSetEstimates(g["poses"], h)
    assert bind21(s, cids) == 0
    assert bind(s, cids) == ARG                                           # the type-21 group's ids
    assert bind(s, ids) == 0
    assert bind21(s, ids) == ARG                                          # ... and the other way round
    s.odom_calib_sets, s.calib_sets = tuple(ids), tuple(cids)
    s.pgLinearize(True)
    s.buildSystem()
    chi0, ref = s.chi2(), _data(s, n)
    assert np.abs(ref[3] - H.producers(H.FP64, g, jac=False)).max() < 1e-12

    def unchanged():
        assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
        s.buildSystem()
        assert s.chi2() == chi0
        for a, b in zip(_data(s, n), ref):
            assert np.array_equal(a, b)

    other = _f64(zm.copy())
    other[:, 0] += 0.25                                                   # (a rejected call must not leave these measurements behind)
    kij, kip, kjp = ids
    for bad_ids in ((99, kip, kjp), (kij, -1, kjp), (kij, kip, 99), (kij, kij, kjp), (kij, kip, kip), (kjp, kip, kjp),
                    (kij, kjp, kip), (k0, kip, kjp), (cids[0], kip, kjp)):  # bad, repeated, wrong parts, bound in another slot
        assert bind(s, bad_ids, m=other) == ARG, bad_ids
    t = capi.HipBlockSolver(3, 2, 0)                                      # (sets that never get data: a handle of their own)
    q0 = t.addEdgeSet(3, h[vi], h[vj])
    tij, tip, tjp = three(t, oi, oj, op)
    k2 = t.addEdgeSet(2, h[oi], h[oj])                                    # error dimension 2
    ku = t.addEdgeSet(3, h[oi], None)                                     # a unary set
    kshort = t.addEdgeSet(3, h[oj[:-1]], h[op[:-1]])                      # one edge short, the parts of set_jp
    t.setEdgeSetParts(kshort, 5)
    t.buildStructure(g["nP"], 0, False)
    t.pgSetEdges(q0, 1, vi, vj, Zm, om)
    for bad_ids in ((k2, tip, tjp), (ku, tip, tjp), (tij, tip, kshort)):
        assert bind(t, bad_ids) == ARG, bad_ids
    assert bind(t, (tij, tip, tjp)) == 0
    for null in ("a", "b", "c", "m"):
        assert bind(s, ids, **{null: None}) == ARG
    for arr, name in ((zm, "m"), (zw, "w")):
        for v in (np.nan, np.inf):
            x = arr.copy()
            x[2, 1] = v
            assert bind(s, ids, **{name: x}) == ARG                       # non-finite values
    for name, src in (("a", oi), ("b", oj), ("c", op)):
        for v in (len(h), -1):
            bad = src.copy()
            bad[3] = v
            assert bind(s, ids, m=other, **{name: bad}) == ARG            # outside the table
        bad = src.copy()
        bad[3] = next(v for v in range(1, 12) if v not in (oi[3], oj[3]))
        assert bind(s, ids, m=other, **{name: bad}) == ARG                # another row: its hessian index is not the sets'
    for name, src in (("c", oi), ("c", oj), ("a", oj), ("b", op)):
        bad = dict(a=oi, b=oj, c=op)[name].copy()
        bad[3] = src[3]
        assert bind(s, ids, m=other, **{name: bad}) == ARG                # a vertex named twice
    unchanged()
    # row kinds, second order: while the group is bound the other entries refuse an index that names the additive row (a handle
    # of its own: its prior sets never get data)
    u = capi.HipBlockSolver(3, 2, 0)
    u0 = u.addEdgeSet(3, h[vi], h[vj])
    uids = three(u, oi, oj, op)
    kpr = u.addEdgeSet(3, h[_i32([P])], None)
    kpr2 = u.addEdgeSet(3, h[_i32([2])], None)
    lm0 = _i32([g["nP"]])                                                  # (the one landmark's hessian index)
    koffP, koff2 = u.addEdgeSet(3, h[_i32([P])], h[_i32([2])]), u.addEdgeSet(3, h[_i32([1])], h[_i32([2])])
    klmP, klm2 = u.addEdgeSet(2, h[_i32([P])], lm0), u.addEdgeSet(2, h[_i32([2])], lm0)
    kbrP, kbr2 = u.addEdgeSet(1, h[_i32([P])], lm0), u.addEdgeSet(1, h[_i32([2])], lm0)
    u.buildStructure(g["nP"], 1, False)
    u.pgSetEdges(u0, 1, vi, vj, Zm, om)
    u.pgSetEstimates(g["poses"], h)
    assert bind(u, uids) == 0
    assert Lb.g2ohip_pg_set_prior_edges(u.h, kpr, 7, _ip(_i32([P])), one(3), eye, None) == ARG
    assert Lb.g2ohip_pg_set_prior_edges(u.h, kpr2, 7, _ip(_i32([2])), one(3), eye, None) == 0   # (a pose row is fine)
    z1 = _ip(_i32([0]))
    for k, row, want in ((koffP, P, ARG), (koff2, 1, 0)):                 # the offset binder: vi names the additive row / a pose row
        assert Lb.g2ohip_pg_set_offset_edges(u.h, k, 18, _ip(_i32([row])), _ip(_i32([2])), z1, z1, one(3), eye, 1, one(3)) == want, (k, row)
    for k, row, want in ((klmP, P, ARG), (klm2, 2, 0)):                   # the landmark binder's pose side
        assert Lb.g2ohip_pg_set_landmark_edges(u.h, k, 3, _ip(_i32([row])), z1, one(2), _dp(_f64(np.eye(2).reshape(1, 4))), None) == want, (k, row)
    for k, row, want in ((kbrP, P, ARG), (kbr2, 2, 0)):                   # the bearing binder's pose side
        assert Lb.g2ohip_pg_set_bearing_edges(u.h, k, _ip(_i32([row])), z1, one(1), _dp(_f64(np.ones((1, 1))))) == want, (k, row)
    # growth of the POSE set releases the group with the rest of the front end (handle t: update_structure needs a structure
    # without landmarks)
    t.odom_calib_sets = (tij, tip, tjp)
    assert t.updateStructure(0, q0, h[_i32([1])], h[_i32([2])])
    assert t.odom_calib_sets is None
    assert bind(t, (tij, tip, tjp)) == STATE                              # (no pose set is bound any more: pg_set_edges again)
    bad = vi.copy()
    bad[0] = P
    assert Lb.g2ohip_pg_set_edges(s.h, k0, 1, _ip(bad), _ip(vj), _dp(Zm), _dp(om)) == ARG
    bad = cl.copy()
    bad[:] = P
    assert bind21(s, cids, c=bad) == ARG
    for k in ids:                                                         # ... and the group's set ids
        assert Lb.g2ohip_pg_set_prior_edges(s.h, k, 7, _ip(oi), one(3), eye, None) == ARG
        assert Lb.g2ohip_pg_set_edges(s.h, k, 1, _ip(oi), _ip(oj), _dp(zm), _dp(zw)) == ARG
    for typ in (2, 10, 12):
        assert Lb.g2ohip_pg_set_edges(s.h, k0, typ, _ip(vi), _ip(vj), _dp(Zm), _dp(om)) == ARG
    # a type-21 group whose laser offset is the row this group wants as its parameter vertex
    bad = op.copy()
    bad[:] = g["offset_row"]
    assert bind(s, ids, c=bad) == ARG
    with pytest.raises(ValueError):
        s.pgSetOdomCalibEdges(*ids, oi[:-1], oj[:-1], op[:-1], zm[:-1], zw[:-1])
    # g2ohip_pg_set_estimates with changed tables validates the group too
    wrong = h.copy()
    wrong[3], wrong[4] = wrong[4], wrong[3]
    assert Lb.g2ohip_pg_set_estimates(s.h, len(h), _dp(_f64(g["poses"])), _ip(wrong)) == ARG
    s.pgSetOdomCalibEdges(*ids, oi, oj, op, zm, zw)
    assert s.odom_calib_sets == tuple(ids)
    # info = NULL is the identity
    assert bind(s, ids, w=None) == 0
    assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
    e = _data(s, n)[3]
    assert np.abs(e - ref[3]).max() == 0
    assert bind(s, ids) == 0
    # growth of one of the three sets drops the group; clear_edge_sets drops everything
    assert s.updateStructure(0, kij, h[_i32([1])], h[_i32([2])])
    assert s.odom_calib_sets is None and s.calib_sets == tuple(cids)
    assert bind(s, ids) == ARG                                            # (the edge counts differ now)
    s.clearEdgeSets()
    assert s.odom_calib_sets is None and s.calib_sets is None
    assert Lb.g2ohip_pg_linearize(s.h, 1) == STATE


def test_from_a_file(tmp_path):
    """written with g2o_io.write_g2o_odom_calib, read back, set up, one LM iteration equals the in-memory problem."""
    g = H.without_odometry(S.make_calib_rig(10, loops=4, seed=9, odom_calib=True))
    path = os.path.join(str(tmp_path), "rig.g2o")
    g2o_io.write_g2o_odom_calib(path, g)
    p = g2o_io.odom_calib_problem(g2o_io.read_g2o(path))
    out = []
    for q in (p, g):
        s, graph = H.device_setup(q)
        graph.linearize()
        chi0 = graph.chi2()
        done, chis, _, tr = lm.optimize(graph, s, 1, "lm")
        out.append((chi0, chis[-1], [int(t) for t in tr], s.pgGetEstimates()))
    print("from a file: chi2", out[0][:3], "in memory", out[1][:3])
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and out[0][2] == out[1][2] and np.array_equal(out[0][3], out[1][3])
    assert out[0][1] < out[0][0]
