"""GPU: laser self-calibration on the device (EdgeSE2SensorCalib = type 21 beside an EdgeSE2 set,
g2ohip_pg_set_sensor_calib_edges): the producer against the fp64 restatement of openslam_g2o_amd/sensor_calib.py within 8 x that
restatement's recorded drift against 60 digits (tests/golden/sensor_calib_edges.npz), tails, both store forms, the error-only
evaluation, vertex indexing, the assembled system and its solution against the CPU oracle's three-vertex edges, the dense block row
of the shared offset vertex under the direct solver, a Levenberg-Marquardt run against the host-fed one, the binding rules, the other
slots beside it, a graph from a file."""
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io, lm, offset_edges as OE, synthetic as S
from oracle import oracle as O
from tests import calib_helpers as H
from tests import producer_metric as PM
from tests.helpers import relerr

pytestmark = pytest.mark.gpu

Z = np.load(H.GOLDEN)
TOL_B = 1e-11       # right-hand side, as tests/test_gpu_offset_edges.py
TOL_H = 1e-12       # assembled blocks
TOL_X = 1e-8        # solution
TOL_X_DENSE = 1e-7  # the relative error of the loop-closure parity tests (tests/test_gpu_lm.py)
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE
PCG = {"linear_solver": 1, "pcg_tolerance": 1e-22, "pcg_absolute_tolerance": 0, "pcg_max_iterations": 2000}   # (to the rounding level)


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _data(s, n):
    """(Ji, Jj, Jl, err) as the next buildSystem reads them; the three sets must show the SAME shared arrays."""
    kij, kil, kjl = s.calib_sets
    Ji, Jj, err = s.edgeData(kij, n, 3, 3, 3)
    Ji2, Jl, err2 = s.edgeData(kil, n, 3, 3, 3)
    Jj3, Jl3, err3 = s.edgeData(kjl, n, 3, 3, 3)
    assert np.array_equal(Ji, Ji2) and np.array_equal(Jj, Jj3) and np.array_equal(Jl, Jl3)
    assert np.array_equal(err, err2) and np.array_equal(err, err3)
    return Ji, Jj, Jl, err


def _chi2_ref(g, poses, err, huber=0.0):
    e0 = H.pose_edges(g, poses, jac=False)
    return OE.chi2(err, g["cinfo"], huber) + float(np.einsum("ni,nij,nj->n", e0, np.asarray(g["omega"]).reshape(-1, 3, 3), e0).sum())


def _within(tag, dev, ref, drift):
    """device against the restatement: 8 x the recorded drift of (err, J), itself below the per-row ceiling of producer_metric."""
    n = len(ref[3])
    fig = (np.abs(dev[3] - ref[3]).max(), max(np.abs(dev[k] - ref[k]).max() for k in range(3)))
    ones = np.ones((n, 3))
    rows = (PM.worst_row(dev[3], ref[3], ones, 3)[0], max(PM.worst_row(dev[k], ref[k], ones, 3)[0] for k in range(3)))
    print(tag, "device vs restatement (err, J)", fig, "bound", H.DRIFT_FACTOR * np.asarray(drift), "per-row figure", rows)
    for f, b, r in zip(fig, drift, rows):
        assert H.DRIFT_FACTOR * b <= PM.CEILING
        assert f <= H.DRIFT_FACTOR * b, (tag, fig, drift)
        assert r <= PM.CEILING


@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_producer_tails(n):
    row = H.EDGE_COUNTS.index(n)
    g = H.load_graph(Z, n)
    s, graph = H.device_setup(g)
    graph.linearize()
    ref = H.producers(H.FP64, g)
    dev = _data(s, n)
    _within("calib %d" % n, dev, ref, Z["drift"][row])
    if n >= H.N_SPECIAL:
        # the golden edges proper against the 60-digit values: the device's 8 x drift from the restatement plus the restatement's own
        m, (be, bJ) = H.N_SPECIAL, Z["drift"][1]
        fig = (np.abs(dev[3][:m] - Z["err"][:m]).max(), max(np.abs(dev[k][:m] - Z[key][:m]).max() for k, key in enumerate(("Ji", "Jj", "Jl"))))
        print("golden edges: device vs 60 digits (err, J)", fig, "bound", (H.DRIFT_FACTOR + 1) * be, (H.DRIFT_FACTOR + 1) * bJ)
        assert fig[0] <= (H.DRIFT_FACTOR + 1) * be and fig[1] <= (H.DRIFT_FACTOR + 1) * bJ
        same = g["poses"][g["ci"][:m], 2] == g["poses"][g["cj"][:m], 2]
        assert same.any() and not dev[2][:m][same][:, [0, 1, 3, 4]].any()          # th1 == th2: d e_t / d tl is exactly zero
    fixed_i, fixed_j = g["ci"] == 0, g["cj"] == 0
    assert not dev[0][fixed_i].any() and not dev[1][fixed_j].any()                 # the blocks of the fixed pose: zeros
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
    # an error-only evaluation after a pose update leaves J and gives the errors of the moved poses, in both store forms
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
        c_ref = _chi2_ref(g, moved, e_ref)
        assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref


def test_index_permutation():
    """vi, vj, vl shuffled over a pose table larger than the edge list: the 8 rows of the graph scattered over a table of 40 rows
    whose other rows hold other values (fixed, unused).  A kernel that reads row k instead of row v[k] cannot give the same bits."""
    n = 25                                           # (fewer edges than rows)
    g = H.load_graph(Z, n)
    s, graph = H.device_setup(g)
    graph.linearize()
    ref = _data(s, n)
    rng = np.random.default_rng(11)
    where = rng.permutation(40)[:8].astype(np.int32)           # new row of old row r
    assert (where != np.arange(8)).sum() >= 6 and where.max() >= 8
    poses = rng.normal(size=(40, 3)) * 5.0
    poses[where] = g["poses"]
    hidx = np.full(40, -1, np.int32)
    hidx[where] = g["hidx"]
    gp = dict(g, poses=poses, hidx=hidx, n=40, vi=where[g["vi"]], vj=where[g["vj"]], ci=where[g["ci"]], cj=where[g["cj"]], cl=where[g["cl"]])
    sp, graph_p = H.device_setup(gp)
    graph_p.linearize()
    for a, b in zip(_data(sp, n), ref):
        assert np.array_equal(a, b)
    s.buildSystem()
    sp.buildSystem()
    assert sp.chi2() == s.chi2() and np.array_equal(sp.b(), s.b())
    # the two poses of every edge swapped: another graph
    gs = dict(g, ci=g["cj"], cj=g["ci"])
    ss, graph_s = H.device_setup(gs)
    graph_s.linearize()
    assert (np.abs(_data(ss, n)[3] - ref[3]).max(axis=1) > 1e-6).all()


def _dense_pp(s):
    """the device's Hpp as a dense symmetric matrix"""
    capi = _capi()
    cp, row = s.pattern(capi.HPP)
    v = s.values(capi.HPP).reshape(-1, 3, 3)
    n = 3 * s.nP
    Hm = np.zeros((n, n))
    for c in range(s.nP):
        for q in range(cp[c], cp[c + 1]):
            r = row[q]
            B = v[q].T   # stored column-major
            Hm[3 * r:3 * r + 3, 3 * c:3 * c + 3] = B
            Hm[3 * c:3 * c + 3, 3 * r:3 * r + 3] = B.T
    return Hm


def _check_system(s, g, huber, tag):
    o, m = H.oracle_calib(g)
    _, _, err = H.feed_oracle(g, o, m, huber)
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
    s.restoreDiagonal()
    o.restore_diagonal()
    return err


def _refix(g, fixed_rows):
    hidx, nP = g2o_io.hessian_index(g["n"], fixed_rows)
    poses = g["poses"].copy()
    if g["offset_row"] in fixed_rows:
        poses[g["offset_row"]] = g["offset_true"]
    return dict(g, hidx=hidx, nP=nP, poses=poses)


@pytest.mark.parametrize("solver", ["direct", "pcg"])
@pytest.mark.parametrize("case", ["offset_free", "offset_fixed", "pose_fixed"])
@pytest.mark.parametrize("huber", [0.0, 12.0])
def test_assembled_system_against_oracle(huber, case, solver):
    """H, b, chi2 and the solved x against OracleSolver(schur=False) fed the fp64 restatement through add_multi_edge_set: 40 poses, 60
    calibration edges (every tenth a gross outlier on either side of +-pi) plus 39 odometry edges; with and without Huber on the
    three sets; the offset free, the offset fixed, a fixed pose inside the graph (pose 17: vertex 0 of some edges, vertex 1 of
    others); the direct solver and PCG."""
    g = S.make_calib_rig(40, loops=21, seed=2, wrap_every=10)
    assert len(g["ci"]) == 60
    if case == "offset_fixed":
        g = _refix(g, [0, g["offset_row"]])
    elif case == "pose_fixed":
        g = _refix(g, [0, 17])
        assert (g["ci"] == 17).any() and (g["cj"] == 17).any()
    s, graph = H.device_setup(g, huber=huber, options=PCG if solver == "pcg" else None)
    graph.linearize()
    err = _check_system(s, g, huber, "huber %g %s %s" % (huber, case, solver))
    if huber > 0:
        w = np.einsum("ni,nij,nj->n", err, g["cinfo"].reshape(-1, 3, 3), err)
        assert (w > 4 * huber * huber).sum() >= 6 and (w < huber * huber).sum() >= 6
    dev = _data(s, 60)
    fixed = np.asarray(g["hidx"]) < 0
    assert not dev[0][fixed[g["ci"]]].any() and not dev[1][fixed[g["cj"]]].any() and not dev[2][fixed[g["cl"]]].any()


def test_dense_row_solve():
    """300 poses, every calibration edge touching L, the direct solver: L's block column holds a block for every free vertex, every
    front of the multifrontal factorisation carries its three rows.  x against a dense NumPy solve of the oracle's damped matrix."""
    capi = _capi()
    g = S.make_calib_rig(300, loops=40, seed=1)
    s, graph = H.device_setup(g)
    graph.linearize()
    o, m = H.oracle_calib(g)
    H.feed_oracle(g, o, m)
    s.buildSystem()
    o.build_system()
    cp, row = s.pattern(capi.HPP)
    assert s.nP == 300 and np.diff(cp).max() == 300                      # (L's block column is full)
    lam = 1e-4 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve()
    x_ref = np.linalg.solve(o.dense_full(), o.b())
    fig = dict(dx=relerr(s.x(), x_ref), Hpp=relerr(_dense_pp(s), o.dense_full()), b=relerr(s.b(), o.b()))
    print("dense row", fig, s.stats())
    assert fig["b"] < TOL_B and fig["Hpp"] < TOL_H and fig["dx"] < TOL_X_DENSE
    x = s.x()
    assert s.solve() and np.array_equal(s.x(), x)                        # bit-repeatable


class HostFedCalibGraph:
    """The graph protocol of openslam_g2o_amd.lm over ONE library handle whose three calibration sets are ordinary edge sets fed
    from the host: every evaluation reads the poses back, evaluates sensor_calib.py in fp64 and uploads the arrays through
    g2ohip_set_edge_data.  The poses, the odometry set and the update stay with the device front end."""

    def __init__(self, s, g, ids):
        self.s, self.g, self.ids, self.J = s, g, ids, None

    def _feed(self, jac):
        self.s.pgLinearize(jac)
        poses = self.s.pgGetEstimates()
        if jac:
            Ji, Jj, Jl, err = H.producers(H.FP64, self.g, poses)
            self.J = (Ji, Jj, Jl)
        else:
            err = H.producers(H.FP64, self.g, poses, jac=False)
        Ji, Jj, Jl = self.J
        for k, (A, B) in zip(self.ids, ((Ji, Jj), (Ji, Jl), (Jj, Jl))):
            self.s.setEdgeData(k, A, B, self.g["cinfo"], err)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


def _three_sets(s, g):
    capi = _capi()
    h = np.asarray(g["hidx"], np.int32)
    parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
    ids = []
    for (a, b), pt in zip(((g["ci"], g["cj"]), (g["ci"], g["cl"]), (g["cj"], g["cl"])), parts):
        ids.append(s.addEdgeSet(3, h[a], h[b]))
        s.setEdgeSetParts(ids[-1], pt)
    return ids


def _host_fed(g):
    capi = _capi()
    h = np.asarray(g["hidx"], np.int32)
    sh = capi.HipBlockSolver(3, 2, 0)
    q0 = sh.addEdgeSet(3, h[g["vi"]], h[g["vj"]])
    ids = _three_sets(sh, g)
    sh.buildStructure(g["nP"], 0, False)
    sh.pgSetEdges(q0, 1, g["vi"], g["vj"], g["Z"], g["omega"])
    sh.pgSetEstimates(g["poses"], h)
    return sh, HostFedCalibGraph(sh, g, ids)


def test_lm_run_device_resident_against_host_fed():
    """LM twice through the same library over the rig of 60 poses and 89 calibration edges, 8 iterations: device-resident, and with
    the three sets host-fed from sensor_calib.py.  Equal trial counts (the CPU runs' as well); the chi2 gap of every iteration
    within 8 x the largest gap between two equally valid CPU runs (the oracle's solver and a dense solve, recorded by
    tests/golden/make_sensor_calib_edges.py; single iterations of those two agree to the last bit, so the run's largest gap is
    the scale); the offset moves from the identity to within the measurement noise of the truth."""
    g = H.lm_graph()
    s, graph = H.device_setup(g)
    n_dev, chi_dev, _, tr_dev = lm.optimize(graph, s, H.LM_ITERATIONS, "lm")
    sh, host = _host_fed(g)
    n_host, chi_host, _, tr_host = lm.optimize(host, sh, H.LM_ITERATIONS, "lm")
    gaps = [abs(a - b) / b for a, b in zip(chi_dev, chi_host)]
    bound = H.DRIFT_FACTOR * float(Z["lm_gap"].max())
    print("lm chi2 device", chi_dev)
    print("lm chi2 host-fed", chi_host)
    print("lm gaps", gaps, "bound", bound, "trials", tr_dev, tr_host, Z["lm_trials"].tolist())
    assert n_dev == n_host == H.LM_ITERATIONS
    assert [int(t) for t in tr_dev] == [int(t) for t in tr_host] == Z["lm_trials"].tolist()
    for it, gap in enumerate(gaps):
        assert gap <= bound, (it, gap, bound)
    assert abs(chi_dev[-1] - Z["lm_chis"][-1]) <= 1e-9 * Z["lm_chis"][-1]
    e0, e1 = H.offset_error(g, g["poses"]), H.offset_error(g, s.pgGetEstimates())
    print("offset error: initial", e0, "device", e1, "CPU run", Z["lm_offset_error"][1].tolist())
    assert e0[0] > 0.3 and e1[0] <= H.LM_ARGS["noise"][0] and e1[1] <= H.LM_ARGS["noise"][1]


def test_binding_rules():
    capi = _capi()
    Lb = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = S.make_calib_rig(12, loops=5, seed=4)
    n = len(g["ci"])
    h = _i32(g["hidx"])
    vi, vj, ci, cj, cl = (_i32(g[k]) for k in ("vi", "vj", "ci", "cj", "cl"))
    Zm, om, zm, zw = (_f64(g[k]) for k in ("Z", "omega", "cmeas", "cinfo"))

    def bind(s, ids, a=ci, b=cj, c=cl, m=zm, w=zw):
        p = lambda x, fn: None if x is None else fn(x)
        return Lb.g2ohip_pg_set_sensor_calib_edges(s.h, ids[0], ids[1], ids[2], p(a, _ip), p(b, _ip), p(c, _ip), p(m, _dp), p(w, _dp))

    s = capi.HipBlockSolver(3, 2, 0)
    k0 = s.addEdgeSet(3, h[vi], h[vj])
    ids = _three_sets(s, g)
    koff = s.addEdgeSet(3, h[ci], h[cj])                                  # bound in the offset slot below
    assert bind(s, ids) == STATE                                          # before g2ohip_build_structure
    s.buildStructure(g["nP"], 0, False)
    assert bind(s, ids) == STATE                                          # no type-1 set bound
    s.pgSetEdges(k0, 1, vi, vj, Zm, om)
    s.pgSetEstimates(g["poses"], h)
    s.pgSetOffsetEdges(koff, 18, ci, cj, np.zeros(n, np.int32), np.zeros(n, np.int32), zm, zw, np.zeros((1, 3)))
    s.setRobustKernelPerEdge(ids[1], np.full(n, capi.KERNEL_HUBER, np.int32), np.ones(n))
    assert bind(s, ids) == STATE                                          # per-edge robust kernels at binding
    s.setRobustKernelPerEdge(ids[1], None, None)
    assert bind(s, ids) == 0
    s.calib_sets = tuple(ids)                                             # (what pgSetSensorCalibEdges records; the raw entry is used here)
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
    other[:, -1] += 0.25                                                  # (a rejected call must not leave these measurements behind)
    kij, kil, kjl = ids
    for bad_ids in ((99, kil, kjl), (kij, -1, kjl), (kij, kil, 99),       # a bad set id
                    (kij, kij, kjl), (kij, kil, kil), (kjl, kil, kjl),    # a repeated set id
                    (kij, kjl, kil),                                      # wrong parts: (i, l) and (j, l) exchanged
                    (k0, kil, kjl), (koff, kil, kjl)):                    # bound in another slot: the pose set, the offset set
        assert bind(s, bad_ids, m=other) == ARG, bad_ids
    t = capi.HipBlockSolver(3, 2, 0)                                      # (sets that never get data: a handle of their own)
    q0 = t.addEdgeSet(3, h[vi], h[vj])
    tij, til, tjl = _three_sets(t, g)
    k2 = t.addEdgeSet(2, h[ci], h[cj])                                    # error dimension 2
    ku = t.addEdgeSet(3, h[ci], None)                                     # a unary set
    kshort = t.addEdgeSet(3, h[cj[:-1]], h[cl[:-1]])                      # one edge short, the parts of set_jl
    t.setEdgeSetParts(kshort, 5)
    t.buildStructure(g["nP"], 0, False)
    t.pgSetEdges(q0, 1, vi, vj, Zm, om)
    for bad_ids in ((k2, til, tjl), (ku, til, tjl), (tij, til, kshort)):  # wrong dimensions, a unary set, wrong edge count
        assert bind(t, bad_ids) == ARG, bad_ids
    assert bind(t, (tij, til, tjl)) == 0
    for null in ("a", "b", "c", "m"):
        assert bind(s, ids, **{null: None}) == ARG
    for arr, name in ((zm, "m"), (zw, "w")):
        for v in (np.nan, np.inf):
            x = arr.copy()
            x[2, 1] = v
            assert bind(s, ids, **{name: x}) == ARG                       # non-finite values
    for name, src in (("a", ci), ("b", cj), ("c", cl)):
        for v in (len(h), -1):
            bad = src.copy()
            bad[3] = v
            assert bind(s, ids, m=other, **{name: bad}) == ARG            # outside the pose table
        bad = src.copy()
        bad[3] = next(v for v in range(1, 12) if v not in (ci[3], cj[3]))
        assert bind(s, ids, m=other, **{name: bad}) == ARG                # another pose: its hessian index is not the sets'
    for name, src in (("c", ci), ("c", cj), ("a", cj), ("b", cl)):
        bad = dict(a=ci, b=cj, c=cl)[name].copy()
        bad[3] = src[3]
        assert bind(s, ids, m=other, **{name: bad}) == ARG                # vl == vi, vl == vj, vi == vj, vj == vl
    unchanged()
    # refusals of the other entries while the group is bound
    zeros = lambda c: _dp(_f64(np.zeros((n, c))))
    for k in ids:
        assert Lb.g2ohip_pg_set_prior_edges(s.h, k, 7, _ip(ci), zeros(3), zeros(9), None) == ARG
        assert Lb.g2ohip_pg_set_landmark_edges(s.h, k, 3, _ip(ci), _ip(cj), zeros(2), zeros(4), None) == ARG
        assert Lb.g2ohip_pg_set_edges(s.h, k, 1, _ip(ci), _ip(cj), _dp(zm), _dp(zw)) == ARG
        assert Lb.g2ohip_pg_set_offset_edges(s.h, k, 18, _ip(ci), _ip(cj), _ip(ci), _ip(ci), _dp(zm), _dp(zw), 1, zeros(3)) == ARG
        assert Lb.g2ohip_pg_set_bearing_edges(s.h, k, _ip(ci), _ip(cj), zeros(1), zeros(1)) == ARG
    for typ in (2, 10, 12):                                               # pose types that do not fit the bound group
        assert Lb.g2ohip_pg_set_edges(s.h, k0, typ, _ip(vi), _ip(vj), _dp(Zm), _dp(om)) == ARG
    unchanged()
    with pytest.raises(ValueError):
        s.pgSetSensorCalibEdges(*ids, ci[:-1], cj[:-1], cl[:-1], zm[:-1], zw[:-1])
    # info = NULL is the identity
    assert bind(s, ids, w=None) == 0
    assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
    s.buildSystem()
    e0 = H.pose_edges(g, jac=False)
    e_off = OE.offset_edges(H.FP64, 18, g["poses"], ci, cj, np.zeros(n, np.int32), np.zeros(n, np.int32), zm, np.zeros((1, 3)), jac=False)
    c_id = float((ref[3] * ref[3]).sum()) + float(np.einsum("ni,nij,nj->n", e0, om.reshape(-1, 3, 3), e0).sum()) + OE.chi2(e_off, zw)
    assert abs(s.chi2() - c_id) <= 1e-12 * c_id
    assert bind(s, ids) == 0
    unchanged()
    # g2ohip_pg_set_estimates with changed tables validates the group too
    wrong = h.copy()
    wrong[3], wrong[4] = wrong[4], wrong[3]
    assert Lb.g2ohip_pg_set_estimates(s.h, len(h), _dp(_f64(g["poses"])), _ip(wrong)) == ARG
    unchanged()
    # the wrapper binds the same group
    s.pgSetSensorCalibEdges(*ids, ci, cj, cl, zm, zw)
    assert s.calib_sets == tuple(ids)
    unchanged()
    # growth of one of the three sets drops the group
    assert s.updateStructure(0, kij, h[_i32([1])], h[_i32([2])])
    assert s.calib_sets is None
    assert bind(s, ids) == ARG                                            # (the edge counts differ now)
    s.clearEdgeSets()
    assert s.calib_sets is None
    assert Lb.g2ohip_pg_linearize(s.h, 1) == STATE


def test_beside_a_prior_set_and_an_offset_set():
    """The calibration slot beside a prior set (type 7) and an EdgeSE2Offset set (type 18) on one handle: the system and dx against
    the oracle fed the fp64 producers of all four."""
    from tests import offset_helpers as OH
    capi = _capi()
    g = S.make_calib_rig(14, loops=6, seed=3)
    r = S.make_offset_rig("se2", 14, 2, 2, seed=2)
    h = np.asarray(g["hidx"], np.int32)
    vq = np.array([3, 9], np.int32)
    zq = g["poses_true"][vq] + 0.01
    omq = np.tile((np.eye(3) * 50.0).reshape(1, 9), (2, 1))
    go = dict(kind="se2", offset_type=18, poses=g["poses"], oi=r["oi"], oj=r["oj"], opf=r["opf"], opt=r["opt"], omeas=r["omeas"], oinfo=r["oinfo"],
              offsets=r["offsets"])
    s, graph = lm.setup_device_pose_graph(1, g["poses"], h, g["nP"], g["vi"], g["vj"], g["Z"], g["omega"], priors=(7, vq, zq, omq, None),
                                          offset_edges=(18, go["oi"], go["oj"], go["opf"], go["opt"], go["omeas"], go["oinfo"], go["offsets"]),
                                          calib_edges=H.calib_dict(g))
    assert s.prior_set is not None and s.offset_set is not None and len(s.calib_sets) == 3
    graph.linearize()
    o = O.OracleSolver(3, 2, g["nP"], 0, False)
    o.set_dims(o.add_edge_set(3, h[g["vi"]], h[g["vj"]]), 3, 3)
    o.set_dims(o.add_edge_set(3, h[vq]), 3, 0)
    o.set_dims(o.add_edge_set(3, h[go["oi"]], h[go["oj"]]), 3, 3)
    m = o.add_multi_edge_set(3, np.stack([h[g["ci"]], h[g["cj"]], h[g["cl"]]], axis=1))
    o.build_structure()
    A0, A1, e0 = H.pose_edges(g)
    from tests import prior_helpers as PH
    Q0, eq = PH.prior_edges_of(7, g["poses"], vq, zq)
    J0, J1, eo = OH.producers(OH.FP64, go)
    Ji, Jj, Jl, err = H.producers(H.FP64, g)
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    o.set_edge_data(1, Q0, None, omq, eq)
    o.set_edge_data(2, J0, J1, go["oinfo"], eo)
    o.set_multi_edge_data(m, [Ji, Jj, Jl], g["cinfo"], err, 0.0, 1)
    dev = _data(s, len(g["ci"]))
    assert max(relerr(dev[0], Ji), relerr(dev[1], Jj), relerr(dev[2], Jl), relerr(dev[3], err)) < 1e-12
    s.buildSystem()
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B and abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    fig = dict(Hpp=relerr(_dense_pp(s), o.dense_full()), dx=relerr(s.x(), o.x()))
    print("beside priors and offset edges", fig)
    assert fig["Hpp"] < TOL_H and fig["dx"] < TOL_X


def test_from_a_file(tmp_path):
    """written with g2o_io.write_g2o_calib, read back, set up, one LM iteration: device-resident against host-fed."""
    g = S.make_calib_rig(10, loops=4, seed=9)
    path = os.path.join(str(tmp_path), "rig.g2o")
    g2o_io.write_g2o_calib(path, g)
    p = g2o_io.calib_problem(g2o_io.read_g2o(path))
    s, graph = H.device_setup(p)
    graph.linearize()
    chi0 = graph.chi2()
    done, chis, _, tr = lm.optimize(graph, s, 1, "lm")
    sh, host = _host_fed(p)
    done_h, chis_h, _, tr_h = lm.optimize(host, sh, 1, "lm")
    print("from a file: chi2", chi0, "->", chis, "host-fed", chis_h, "trials", tr, tr_h)
    assert done == done_h == 1 and [int(t) for t in tr] == [int(t) for t in tr_h]
    assert chis[-1] < chi0 and abs(chis[-1] - chis_h[-1]) <= 1e-9 * chis_h[-1]
    assert np.abs(s.pgGetEstimates() - sh.pgGetEstimates()).max() < 1e-9
