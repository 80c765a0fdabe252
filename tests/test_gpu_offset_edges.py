"""GPU: the sensor-offset pose-pose edges on the device (EdgeSE2Offset = type 18 beside an EdgeSE2 set, EdgeSE3Offset = type 19
beside an EdgeSE3 set, g2ohip_pg_set_offset_edges): the producers against the fp64 restatement of openslam_g2o_amd/offset_edges.py
within 8 x that restatement's recorded drift against 60 digits (tests/golden/offset_edges.npz), tails, both store forms, the
error-only evaluation, parameter indexing, the assembled system and its solution against the CPU oracle, robust kernels, a
Levenberg-Marquardt run against the host-fed one, the binding rules, the other slots beside it, a graph from a file."""
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io, lm, offset_edges as OE, synthetic as S
from oracle import oracle as O
from tests import landmark_helpers as LH
from tests import offset_helpers as H
from tests import prior_helpers as PH
from tests import producer_metric as PM
from tests.helpers import relerr

pytestmark = pytest.mark.gpu

Z = np.load(H.GOLDEN)
TOL_B = 1e-11       # right-hand side, as tests/test_gpu_gicp.py
TOL_H = 1e-12       # assembled blocks
TOL_X = 1e-8        # solution
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _data(s, g, n=None):
    d = H.DIM[g["kind"]]
    return s.edgeData(s.offset_set, len(g["oi"]) if n is None else n, d, d, d)


def _chi2_ref(g, poses, err, huber=0.0):
    e0 = H.pose_edges(g, poses, jac=False)
    d = H.DIM[g["kind"]]
    return OE.chi2(err, g["oinfo"], huber) + float(np.einsum("ni,nij,nj->n", e0, np.asarray(g["omega"]).reshape(-1, d, d), e0).sum())


def _within(tag, dev, ref, drift, d):
    """device against the restatement: 8 x the recorded drift of (err, J), itself below the per-row ceiling of producer_metric."""
    fig = (np.abs(dev[2] - ref[2]).max(), max(np.abs(dev[0] - ref[0]).max(), np.abs(dev[1] - ref[1]).max()))
    rows = (PM.worst_row(dev[2], ref[2], np.ones((len(ref[2]), d)), d)[0],
            max(PM.worst_row(dev[0], ref[0], np.ones((len(ref[2]), d)), d)[0], PM.worst_row(dev[1], ref[1], np.ones((len(ref[2]), d)), d)[0]))
    print(tag, "device vs restatement (err, J)", fig, "bound", H.DRIFT_FACTOR * np.asarray(drift), "per-row figure", rows)
    for f, b, r in zip(fig, drift, rows):
        assert H.DRIFT_FACTOR * b <= PM.CEILING
        assert f <= H.DRIFT_FACTOR * b, (tag, fig, drift)
        assert r <= PM.CEILING


@pytest.mark.parametrize("kind,etype", H.KINDS)
@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_producer_tails(kind, etype, n):
    d = H.DIM[kind]
    row = H.EDGE_COUNTS.index(n)
    g = H.load_graph(Z, kind, n)
    s, graph = H.device_setup(g)
    graph.linearize()
    ref = H.producers(H.FP64, g)
    dev = _data(s, g)
    _within("%s %d" % (kind, n), dev, ref, Z[kind + "_drift"][row], d)
    s.buildSystem()
    c_ref = _chi2_ref(g, None, ref[2])
    assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref
    # the other store form: the same bits
    s.setOption("pg_landmark_staged", 0)
    s.pgSetEstimates(g["poses"], g["hidx"])
    s.pgLinearize(True)
    direct = _data(s, g)
    for a, b in zip(dev, direct):
        assert np.array_equal(a, b)
    # an error-only evaluation after a pose update leaves J and gives the errors of the moved poses, in both store forms
    for staged in (0, 1):
        s.setOption("pg_landmark_staged", staged)
        s.pgSetEstimates(g["poses"], g["hidx"])
        s.pgLinearize(True)
        s.buildSystem()
        s.setX(Z[kind + "_moved_x"])
        s.pgUpdate()
        s.pgLinearize(False)
        moved = s.pgGetEstimates()
        assert np.abs(moved - Z[kind + "_moved_poses"]).max() < 1e-14
        e_ref = H.producers(H.FP64, g, poses=moved, jac=False)
        after = _data(s, g)
        assert np.array_equal(after[0], dev[0]) and np.array_equal(after[1], dev[1])
        fig = np.abs(after[2] - e_ref).max()
        print(kind, n, "moved: device vs restatement", fig, "bound", H.DRIFT_FACTOR * Z[kind + "_moved_drift"][row])
        assert fig <= H.DRIFT_FACTOR * Z[kind + "_moved_drift"][row]
        assert np.abs(after[2] - dev[2]).max() > 1e-3
        c_ref = _chi2_ref(g, moved, e_ref)
        assert abs(s.chi2() - c_ref) <= 1e-12 * c_ref


@pytest.mark.parametrize("kind,etype", H.KINDS)
def test_parameter_indexing(kind, etype):
    """The table rows permuted with param_from / param_to permuted accordingly: identical bits.  The two parameter columns swapped
    with the rows left alone: another graph."""
    g = H.load_graph(Z, kind, 257)
    s, graph = H.device_setup(g)
    graph.linearize()
    ref = _data(s, g)
    perm = np.array([2, 0, 1])                       # new row r holds old row perm[r]
    new_of_old = np.argsort(perm).astype(np.int32)
    gp = dict(g, offsets=g["offsets"][perm], opf=new_of_old[g["opf"]], opt=new_of_old[g["opt"]])
    sp, graph_p = H.device_setup(gp)
    graph_p.linearize()
    for a, b in zip(_data(sp, gp), ref):
        assert np.array_equal(a, b)
    gs = dict(g, opf=g["opt"], opt=g["opf"])
    ss, graph_s = H.device_setup(gs)
    graph_s.linearize()
    swapped = _data(ss, gs)
    differs = g["opf"] != g["opt"]
    assert differs.any() and (~differs).any()
    assert (np.abs(swapped[2] - ref[2]).max(axis=1)[differs] > 1e-6).all()
    assert np.array_equal(swapped[2][~differs], ref[2][~differs])


def _check_system(s, o, tag):
    capi = _capi()
    s.buildSystem()
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    fig = dict(Hpp=relerr(s.values(capi.HPP), o.values("Hpp")), dx=relerr(s.x(), o.x()))
    print(tag, fig)
    assert fig["Hpp"] < TOL_H and fig["dx"] < TOL_X
    s.restoreDiagonal()
    o.restore_diagonal()


@pytest.mark.parametrize("kind,etype", H.KINDS)
@pytest.mark.parametrize("huber", [0.0, 1.0])
@pytest.mark.parametrize("gauge", ["fixed", "free"])
def test_assembled_system_against_oracle(kind, etype, huber, gauge):
    """b, Hpp, chi2 and x against OracleSolver(schur=False) fed the fp64 restatement of both sets, with and without Huber on the
    offset set; with pose 0 fixed (the gauge held by one fixed pose, no prior) and with every pose free."""
    g = H.load_graph(Z, kind, 257)
    if gauge == "free":
        g = dict(g, hidx=np.arange(4, dtype=np.int32), nP=4)
    s, graph = H.device_setup(g, huber=huber)
    graph.linearize()
    o = H.oracle_offset(g)
    J0, J1, err = H.feed_oracle(g, o, huber=huber)
    if huber > 0:
        d = H.DIM[kind]
        w = np.einsum("ni,nij,nj->n", err, g["oinfo"].reshape(-1, d, d), err)
        assert (w > 4 * huber * huber).sum() > 20 and (w < huber * huber).sum() > 20
    _check_system(s, o, "%s huber %g gauge %s" % (kind, huber, gauge))


class HostFedOffsetGraph:
    """The graph protocol of openslam_g2o_amd.lm over ONE library handle whose offset set is an ordinary edge set fed from the
    host: every evaluation reads the poses back, evaluates offset_edges.py in fp64 and uploads J0 / J1 / err through
    g2ohip_set_edge_data.  The poses, the odometry set and the update stay with the device front end."""

    def __init__(self, s, g, set_id):
        self.s, self.g, self.k, self.J = s, g, set_id, None

    def _feed(self, jac):
        self.s.pgLinearize(jac)
        poses = self.s.pgGetEstimates()
        if jac:
            J0, J1, err = H.producers(H.FP64, self.g, poses)
            self.J = (J0, J1)
        else:
            err = H.producers(H.FP64, self.g, poses, jac=False)
        self.s.setEdgeData(self.k, self.J[0], self.J[1], self.g["oinfo"], err)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


def _host_fed(g):
    capi = _capi()
    d = H.DIM[g["kind"]]
    h = np.asarray(g["hidx"], np.int32)
    sh = capi.HipBlockSolver(d, 2 if d == 3 else 3, 0)
    q0 = sh.addEdgeSet(d, h[g["vi"]], h[g["vj"]])
    q1 = sh.addEdgeSet(d, h[g["oi"]], h[g["oj"]])
    sh.buildStructure(g["nP"], 0, False)
    sh.pgSetEdges(q0, 1 if d == 3 else 2, g["vi"], g["vj"], g["Z"], g["omega"])
    sh.pgSetEstimates(g["poses"], h)
    return sh, HostFedOffsetGraph(sh, g, q1)


@pytest.mark.parametrize("kind,etype", H.KINDS)
def test_lm_run_device_resident_against_host_fed(kind, etype):
    """LM twice through the same library over a rig of 12 poses, 2 sensors and 36 offset edges: device-resident, and with the
    offset set host-fed from offset_edges.py.  Equal trial counts (the CPU runs' as well: one iteration rejects steps); the chi2
    gap of every iteration within 8 x the gap between two equally valid CPU runs (the oracle's solver and a dense solve, recorded
    by tests/golden/make_offset_edges.py); the poses end as close to the truth as the CPU run's."""
    g = H.lm_graph(kind)
    lam0 = H.LM_LAMBDA[kind]
    s, graph = H.device_setup(g)
    n_dev, chi_dev, _, tr_dev = lm.optimize(graph, s, H.LM_ITERATIONS, "lm", user_lambda_init=lam0)
    sh, host = _host_fed(g)
    n_host, chi_host, _, tr_host = lm.optimize(host, sh, H.LM_ITERATIONS, "lm", user_lambda_init=lam0)
    gaps = [abs(a - b) / b for a, b in zip(chi_dev, chi_host)]
    bound = H.DRIFT_FACTOR * Z["lm_%s_gap" % kind]
    print(kind, "lm chi2 device", chi_dev)
    print(kind, "lm chi2 host-fed", chi_host)
    print(kind, "lm gaps", gaps, "bound", bound.tolist(), "trials", tr_dev, tr_host, Z["lm_%s_trials" % kind].tolist())
    assert n_dev == n_host == H.LM_ITERATIONS
    assert [int(t) for t in tr_dev] == [int(t) for t in tr_host] and max(tr_dev) > 1
    for it, (gap, b) in enumerate(zip(gaps, bound)):
        assert gap <= b, (it, gap, b)
    e0, e1 = Z["lm_%s_pose_error" % kind]
    final = H.pose_error(g, s.pgGetEstimates())
    poses_gap = np.abs(Z["lm_%s_poses" % kind] - Z["lm_%s_poses_dense" % kind]).max()
    print(kind, "pose error: initial", e0, "CPU run", e1, "device", final, "device vs CPU poses",
          np.abs(s.pgGetEstimates() - Z["lm_%s_poses" % kind]).max(), "CPU vs CPU", poses_gap)
    assert e1 < e0 and final <= e1 * (1.0 + 1e-6)


@pytest.mark.parametrize("kind,etype", H.KINDS)
def test_binding_rules(kind, etype):
    capi = _capi()
    Lb = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    d, ms, ptype = H.DIM[kind], H.STRIDE[kind], 1 if kind == "se2" else 2
    l = 2 if kind == "se2" else 3
    g = H.load_graph(Z, kind, 65)
    h = _i32(g["hidx"])
    vi, vj, oi, oj, pf, pt = (_i32(g[k]) for k in ("vi", "vj", "oi", "oj", "opf", "opt"))
    Zm, om, zm, zw, tab = (_f64(g[k]) for k in ("Z", "omega", "omeas", "oinfo", "offsets"))

    def bind(s, k, typ=etype, a=oi, b=oj, f=pf, t=pt, m=zm, w=zw, n_params=3, table=tab):
        p = lambda x, fn: None if x is None else fn(x)
        return Lb.g2ohip_pg_set_offset_edges(s.h, k, typ, p(a, _ip), p(b, _ip), p(f, _ip), p(t, _ip), p(m, _dp), p(w, _dp), n_params, p(table, _dp))

    s = capi.HipBlockSolver(d, l, 0)
    k0, k1 = s.addEdgeSet(d, h[vi], h[vj]), s.addEdgeSet(d, h[oi], h[oj])
    kz = s.addEdgeSet(d, _i32([]), _i32([]))                           # a set of zero edges
    assert bind(s, k1) == STATE                                        # before g2ohip_build_structure
    s.buildStructure(g["nP"], 0, False)
    assert bind(s, k1) == STATE                                        # before a pose set is bound
    s.pgSetEdges(k0, ptype, vi, vj, Zm, om)
    s.pgSetEstimates(g["poses"], h)
    assert bind(s, k1) == 0
    s.offset_set = k1                                                  # (what pgSetOffsetEdges records; the raw entry is used here)
    s.pgLinearize(True)
    s.buildSystem()
    chi0, ref = s.chi2(), _data(s, g)

    def unchanged():
        assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
        s.buildSystem()
        assert s.chi2() == chi0
        for a, b in zip(_data(s, g), ref):
            assert np.array_equal(a, b)

    other = _f64(zm.copy())
    other[:, -1] += 0.25
    assert bind(s, k1, typ=37 - etype, m=other) == ARG                 # the other kind's type beside this pose set
    assert bind(s, k1, typ=15, m=other) == ARG
    t = capi.HipBlockSolver(d, l, 0)
    to_point = _i32(np.full(65, g["nP"]))                              # (the hessian index of the one landmark)
    q0, ku, kw = t.addEdgeSet(d, h[vi], h[vj]), t.addEdgeSet(d, h[oi], None), t.addEdgeSet(l, h[oi], to_point)
    t.buildStructure(g["nP"], 1, False)
    t.pgSetEdges(q0, ptype, vi, vj, Zm, om)
    assert bind(t, ku) == ARG and bind(t, kw) == ARG                   # a unary set, a set of other dimensions (l, d, l)
    assert bind(s, k0, a=vi, b=vj, f=pf[:3], t=pt[:3], m=zm[:3], w=zw[:3]) == ARG   # bound as the pose-pose set
    for null in ("a", "b", "f", "t", "m", "w", "table"):
        assert bind(s, k1, **{null: None}) == ARG
    assert bind(s, k1, n_params=0, m=other) == ARG
    for name, src in (("f", pf), ("t", pt)):
        for v in (3, -1):
            bad = src.copy()
            bad[7] = v
            assert bind(s, k1, m=other, **{name: bad}) == ARG          # a parameter index outside [0, n_params)
    assert bind(s, k1, n_params=2, m=other) == ARG                     # ... of a shorter table
    bad = oi.copy()
    bad[7] = 4
    assert bind(s, k1, a=bad, m=other) == ARG                          # outside the pose table
    bad[7] = -1
    assert bind(s, k1, a=bad, m=other) == ARG
    bad[7] = next(v for v in range(4) if v not in (oi[7], oj[7]))
    assert bind(s, k1, a=bad, m=other) == ARG                          # another pose: its hessian index is not the set's
    for arr, name in ((zm, "m"), (zw, "w"), (tab, "table")):
        for v in (np.nan, np.inf):
            x = arr.copy()
            x[2, 1] = v                                                # (SE3: inside a column of the rotation part)
            assert bind(s, k1, **{name: x}) == ARG
    unchanged()
    # refusals of the other entries while the set is bound
    zeros = lambda c: _dp(_f64(np.zeros((65, c))))
    assert Lb.g2ohip_pg_set_prior_edges(s.h, k1, 7 if kind == "se2" else 9, _ip(oi), zeros(ms), zeros(d * d), None) == ARG
    assert Lb.g2ohip_pg_set_landmark_edges(s.h, k1, ptype + 2, _ip(oi), _ip(oj), zeros(l), zeros(l * l), None) == ARG
    assert Lb.g2ohip_pg_set_edges(s.h, k1, ptype, _ip(oi), _ip(oj), _dp(zm), _dp(zw)) == ARG
    if kind == "se3":
        assert Lb.g2ohip_pg_set_gicp_edges(s.h, k1, _ip(oi), _ip(oj), zeros(6), zeros(9), None) == ARG
        assert Lb.g2ohip_pg_set_cam_edges(s.h, k1, 16, _ip(oi), _ip(oj), zeros(7), zeros(36)) == ARG
    for typ in (3 - ptype, 10, 12):                                    # pose types that do not fit the bound offset set
        assert Lb.g2ohip_pg_set_edges(s.h, k0, typ, _ip(vi), _ip(vj), _dp(Zm), _dp(om)) == ARG
    unchanged()
    with pytest.raises(ValueError):
        s.pgSetOffsetEdges(k1, etype, oi[:-1], oj[:-1], pf[:-1], pt[:-1], zm[:-1], zw[:-1], tab)
    with pytest.raises(ValueError):
        s.pgSetOffsetEdges(k1, etype, oi, oj, pf, pt, zm, zw, tab[:, :-1])
    # n = 0 is legal (null edge arrays), and replaces the binding; binding the full set again restores it
    assert bind(s, kz, a=None, b=None, f=None, t=None, m=None, w=None) == 0
    assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
    assert bind(s, k1) == 0
    unchanged()
    # g2ohip_pg_set_estimates with changed tables validates the set too
    wrong = h.copy()
    wrong[1], wrong[2] = wrong[2], wrong[1]
    assert Lb.g2ohip_pg_set_estimates(s.h, 4, _dp(_f64(g["poses"])), _ip(wrong)) == ARG
    unchanged()
    # growth by g2ohip_update_structure: refused until bound again
    assert s.updateStructure(0, k1, h[_i32([1])], h[_i32([2])])
    assert Lb.g2ohip_pg_linearize(s.h, 1) == STATE
    s.pgSetOffsetEdges(k1, etype, np.append(oi, 1), np.append(oj, 2), np.append(pf, 0), np.append(pt, 1), np.vstack([zm, zm[:1]]),
                       np.vstack([zw, zw[:1]]), tab)
    s.pgLinearize(True)
    assert np.array_equal(_data(s, g, 66)[2][:65], ref[2])
    s.clearEdgeSets()
    assert s.offset_set is None
    assert Lb.g2ohip_pg_linearize(s.h, 1) == STATE


@pytest.mark.parametrize("kind,etype", H.KINDS)
def test_beside_a_landmark_set_and_a_prior_set(kind, etype):
    """The offset slot beside a landmark set (type 3 / 4, landmarks marginalised) and a prior set (type 7 / 9): the reduced system
    and dx against the oracle fed the fp64 producers of all four sets."""
    capi = _capi()
    g = S.make_landmark_slam(kind, 12, 10, priors="pose", prior_stride=4)
    r = S.make_offset_rig(kind, 12, 2, 3, seed=2)
    d, l, ptype = H.DIM[kind], (2 if kind == "se2" else 3), (1 if kind == "se2" else 2)
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    go = dict(kind=kind, offset_type=etype, poses=g["poses"], oi=r["oi"], oj=r["oj"], opf=r["opf"], opt=r["opt"], omeas=r["omeas"],
              oinfo=r["oinfo"], offsets=r["offsets"])
    prior = PH.prior_type(g)
    s = capi.HipBlockSolver(d, l, 0)
    k0, k1 = s.addEdgeSet(d, h[g["vi"]], h[g["vj"]]), s.addEdgeSet(l, h[g["vp"]], hl[g["vl"]])
    kq, k2 = s.addEdgeSet(PH.PRIOR_DIM[prior], h[g["vq"]], None), s.addEdgeSet(d, h[go["oi"]], h[go["oj"]])
    s.buildStructure(g["nP"], g["nL"], True)
    s.pgSetEdges(k0, ptype, g["vi"], g["vj"], g["Z"], g["omega"])
    s.pgSetEstimates(g["poses"], h)
    s.pgSetLandmarkEdges(k1, ptype + 2, g["vp"], g["vl"], g["zl"], g["omega_l"], g.get("offset"))
    s.pgSetLandmarkEstimates(g["points"], hl)
    s.pgSetPriorEdges(kq, prior, g["vq"], g["zq"], g["omega_q"], g.get("prior_offset"))
    s.pgSetOffsetEdges(k2, etype, go["oi"], go["oj"], go["opf"], go["opt"], go["omeas"], go["oinfo"], go["offsets"])
    s.pgLinearize(True)
    o = O.OracleSolver(d, l, g["nP"], g["nL"], True)
    o.set_dims(o.add_edge_set(d, h[g["vi"]], h[g["vj"]]), d, d)
    o.set_dims(o.add_edge_set(l, h[g["vp"]], hl[g["vl"]]), d, l)
    o.set_dims(o.add_edge_set(PH.PRIOR_DIM[prior], h[g["vq"]]), d, 0)
    o.set_dims(o.add_edge_set(d, h[go["oi"]], h[go["oj"]]), d, d)
    o.build_structure()
    A0, A1, e0 = LH.pose_edges(g)
    B0, B1, e1 = LH.landmark_edges(g)
    Q0, eq = PH.prior_edges(g)
    J0, J1, err = H.producers(H.FP64, go)
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    o.set_edge_data(1, B0, B1, g["omega_l"], e1)
    o.set_edge_data(2, Q0, None, g["omega_q"], eq)
    o.set_edge_data(3, J0, J1, go["oinfo"], err)
    dev = _data(s, go)
    assert max(relerr(dev[0], J0), relerr(dev[1], J1), relerr(dev[2], err)) < 1e-12
    s.buildSystem()
    o.build_system()
    assert relerr(s.b(), o.b()) < TOL_B and abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    fig = dict(Hschur=relerr(s.values(capi.HSCHUR), o.values("Hschur")), dx=relerr(s.x(), o.x()))
    print(kind, "beside landmarks and priors", fig)
    assert fig["Hschur"] < TOL_H and fig["dx"] < TOL_X


@pytest.mark.parametrize("kind,etype", H.KINDS)
def test_from_a_file(kind, etype, tmp_path):
    """written with g2o_io.write_g2o_offset, read back, set up, one LM iteration: device-resident against host-fed."""
    g = S.make_offset_rig(kind, 10, 3, 2, seed=9)
    path = os.path.join(str(tmp_path), "rig.g2o")
    g2o_io.write_g2o_offset(path, g, param_ids=[4, 1, 8])
    p = g2o_io.offset_problem(g2o_io.read_g2o(path))
    s, graph = H.device_setup(p)
    graph.linearize()
    chi0 = graph.chi2()
    done, chis, _, tr = lm.optimize(graph, s, 1, "lm")
    sh, host = _host_fed(p)
    done_h, chis_h, _, tr_h = lm.optimize(host, sh, 1, "lm")
    print(kind, "from a file: chi2", chi0, "->", chis, "host-fed", chis_h, "trials", tr, tr_h)
    assert done == done_h == 1 and [int(t) for t in tr] == [int(t) for t in tr_h]
    assert chis[-1] < chi0 and abs(chis[-1] - chis_h[-1]) <= 1e-9 * chis_h[-1]
    assert np.abs(s.pgGetEstimates() - sh.pgGetEstimates()).max() < 1e-9
