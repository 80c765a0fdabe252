"""GPU: the SBA group's pose-pose constraints on the device -- EdgeSBACam (type 16) and EdgeSBAScale (type 17), bound by
g2ohip_pg_set_cam_edges, each as a set of its own beside a type-12 pose set.

Every producer bound is 8 x (tests/producer_metric.MARGIN) a figure of tests/golden/sbacam_pose_edges.npz (generator:
tests/golden/make_sbacam_pose_edges.py, lines "oracle_drift" of profiles/sba_cam_edges.jsonl): the distance of the fp64
restatement (openslam_g2o_amd/sbacam.py) from the same formulas in mpmath at 60 digits, for the same graph and output -- the
oracle's own error, never the device's.  The Jacobians are the reference's numeric ones (central difference, delta = 1e-9), so
that drift is ~1e-6 on entries of order 1 (3e-4 on the branch graph, whose last edge has translations of 1e3).  Where the
recorded drift of an output is exactly 0 the device must equal the 60-digit values rounded to fp64; so must the columns and
blocks that are zero by construction and the error of the e = 0 edge.

Lane mapping: the EdgeSBACam Jacobian runs one lane per (edge, side, column), 12 lanes per edge, 256 threads per block: 21 edges
fill one block, the 22nd straddles it.  The error kernels and the EdgeSBAScale kernel run one lane per edge: 257 is one past a
block, 300 leaves partial last blocks in both.

The whole-run comparison: the device-resident run against the same library with the two sets fed from the host (sbacam.py in
fp64 through setEdgeData, the cameras read back for every evaluation); chi2 per iteration within 8 x the relative fp64-vs-mpmath
chi2 gap the generator recorded for that iteration over the CPU oracle solver, the accept / reject sequences identical."""
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm
from tests import sbacam_pose_helpers as H
from tests.helpers import TOL_DX, relerr
from tests.producer_metric import MARGIN

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE
TOL_MAT = 1e-12          # assembled blocks and right-hand side in the existing assembly tests (tests/test_gpu_se3expmap.py)
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "sbacam_pose_edges.npz"))
KEYS = H.CAM_KEYS + ("J0", "J1", "err", "drift")
# (EdgeSBACam graph, EdgeSBAScale graph): each slot alone and, where the two share a camera table, both bound
CASES = [("branch", None), (None, "coincident")]
for _n in H.EDGE_COUNTS:
    CASES += [("c%d" % _n, None), (None, "s%d" % _n), ("c%d" % _n, "s%d" % _n)]


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _gold(name):
    g = {k: GOLD["%s_%s" % (name, k)] for k in KEYS}
    g["nP"] = int(g["hidx"].max()) + 1
    return g


def _edges(g):
    return dict(vi=g["vi"], vj=g["vj"], meas=g["meas"], info=g["info"])


def _setup(cam=None, scale=None, **kw):
    """A pure VertexCam pose graph on a (6, 3) handle: no points, no projection set."""
    base = cam or scale
    prob = dict(est=base["est"], hidx=base["hidx"], nP=base["nP"])
    if cam is not None:
        prob["cam_edges"] = _edges(cam)
    if scale is not None:
        assert np.array_equal(scale["est"], base["est"])
        prob["scale_edges"] = _edges(scale)
    return lm.setup_device_sbacam_ba(prob, **kw)


def _data(s, g, scale):
    return s.edgeData(s.scale_set if scale else s.cam_set, len(g["vi"]), 1 if scale else 6, 6, 6)


def _zinv(s):
    import torch
    from openslam_g2o_amd.distributed import tensor_from_device_ptr
    ptr, n = s.deviceArray(_capi().ARR_CAM_ZINV)
    s.sync()
    return tensor_from_device_ptr(ptr, n, torch.device("cuda:0")).cpu().numpy().copy().reshape(-1, 7)


def _within(got, ref, drift, what):
    """8 x the recorded drift; a drift of exactly 0 requires equality."""
    fig = float(np.abs(got - ref).max())
    print("   ", what, "device vs mpmath", fig, "fp64 restatement vs mpmath", drift)
    if drift == 0:
        assert np.array_equal(got, ref), what
    else:
        assert fig <= MARGIN * drift, (what, fig, drift)


def _check_set(s, g, scale, name, err_only):
    J0, J1, err = _data(s, g, scale)
    assert np.array_equal(err, err_only), name                       # the error-only form gave the same bits
    _within(err, g["err"], g["drift"][0], name + " err")
    _within(J0, g["J0"], g["drift"][1], name + " J0")
    _within(J1, g["J1"], g["drift"][2], name + " J1")
    fixed0, fixed1 = g["hidx"][g["vi"]] < 0, g["hidx"][g["vj"]] < 0
    assert not J0[fixed0].any() and not J1[fixed1].any()             # blocks of fixed vertices: zeros
    if scale:
        assert not J0[:, 3:].any() and not J1[:, 3:].any()           # rotation columns: exactly zero
    f0, f1, fe = H.producers(H.FP64, g, scale)
    print("    %s bit-equal to the fp64 restatement: err %s J0 %s J1 %s" % (name, np.array_equal(err, fe), np.array_equal(J0, f0), np.array_equal(J1, f1)))
    return J0, J1, err


def _err_only(s, g, scale):
    """err of a set that has no Jacobians yet (g2ohip_copy_edge_data with NULL Jacobian pointers)."""
    from openslam_g2o_amd.capi import _dp
    err = np.empty((len(g["vi"]), 1 if scale else 6))
    assert s.L.g2ohip_copy_edge_data(s.h, s.scale_set if scale else s.cam_set, None, None, _dp(err)) == 0
    return err


@pytest.mark.parametrize("cname,sname", CASES)
def test_producers_against_mpmath(cname, sname):
    """err, J0, J1 of every fixture graph against the 60-digit values, with each slot alone and with both bound.  The error-only
    form runs first on the fresh handle (its errors are held to the same bound) and the full form must reproduce its bits; a second
    error-only evaluation after the full one leaves the Jacobians in place."""
    cam = _gold(cname) if cname else None
    scale = _gold(sname) if sname else None
    s, graph = _setup(cam, scale)
    graph.compute_active_errors()                                      # error-only, before any Jacobian exists
    only = {sc: _err_only(s, g, sc) for sc, g in ((False, cam), (True, scale)) if g is not None}
    for sc, g in ((False, cam), (True, scale)):
        if g is not None:
            _within(only[sc], g["err"], g["drift"][0], "error-only err")
    graph.linearize()
    full = {}
    for sc, g, name in ((False, cam, cname), (True, scale, sname)):
        if g is not None:
            full[sc] = _check_set(s, g, sc, name, only[sc])
    base = cam or scale
    s.pgSetEstimates(base["est"], base["hidx"])                        # (same values: the next evaluation is a fresh one)
    graph.compute_active_errors()
    for sc, g in ((False, cam), (True, scale)):
        if g is not None:
            again = _data(s, g, sc)
            assert all(np.array_equal(a, b) for a, b in zip(again, full[sc]))
    if cam is not None:
        _within(_zinv(s), GOLD[cname + "_zinv"], cam["drift"][3], cname + " inverse measurements")
    if cname == "branch":
        assert not full[False][2][8].any()                             # the e = 0 edge
    if sname == "coincident":
        J0, J1, err = full[True]
        assert np.isfinite(err).all() and err[0, 0] == scale["meas"][0] and not J0.any() and not J1.any()


def _dense(nP, sets):
    N = 6 * nP
    Hm, b, chi = np.zeros((N, N)), np.zeros(N), 0.0
    for v0, v1, d, J0, J1, om, err in sets:
        for k in range(len(v0)):
            A, B = J0[k].reshape(6, d).T, J1[k].reshape(6, d).T
            W, e = om[k].reshape(d, d), err[k]
            chi += e @ W @ e
            for va, Ja in ((v0[k], A), (v1[k], B)):
                if va < 0:
                    continue
                b[6 * va:6 * va + 6] -= Ja.T @ W @ e
                for vb, Jb in ((v0[k], A), (v1[k], B)):
                    if vb >= 0:
                        Hm[6 * va:6 * va + 6, 6 * vb:6 * vb + 6] += Ja.T @ W @ Jb
    return Hm, b, chi


def test_assembled_system_against_dense_numpy():
    """H and b through the C ABI against a dense sum of J' Omega J, -J' Omega e built from the device's own J / err of the
    22-edge EdgeSBACam set and the 22-edge EdgeSBAScale set: the (1, 6, 6) off-diagonal row and the (1, 6) vertex row of the
    generic assembly.  Bound: TOL_DX of tests/helpers.py through its relerr; the assembled blocks also meet the 1e-12 that the
    existing assembly tests state."""
    capi = _capi()
    cam, scale = _gold("c22"), _gold("s22")
    s, graph = _setup(cam, scale)
    graph.linearize()
    h = cam["hidx"]
    c0, c1, ce = _data(s, cam, False)
    s0, s1, se = _data(s, scale, True)
    Hm, b, chi = _dense(cam["nP"], [(h[cam["vi"]], h[cam["vj"]], 6, c0, c1, cam["info"], ce),
                                    (h[scale["vi"]], h[scale["vj"]], 1, s0, s1, scale["info"], se)])
    s.buildSystem()
    colptr, rowidx = s.pattern(capi.HPP)
    want = np.concatenate([Hm[6 * rowidx[q]:6 * rowidx[q] + 6, 6 * c:6 * c + 6].T.reshape(-1)
                           for c in range(len(colptr) - 1) for q in range(colptr[c], colptr[c + 1])])
    offdiag = sum(int(rowidx[q] != c) for c in range(len(colptr) - 1) for q in range(colptr[c], colptr[c + 1]))
    figs = relerr(s.values(capi.HPP), want), relerr(s.b(), b)
    print("Hpp", figs[0], "b", figs[1], "chi2", s.chi2(), chi, "off-diagonal blocks", offdiag)
    assert offdiag > 0 and (s1[:, :3] != 0).any()
    assert figs[0] < TOL_DX and figs[1] < TOL_DX
    assert figs[0] < TOL_MAT and figs[1] < TOL_MAT
    assert abs(s.chi2() - chi) <= 1e-9 * chi


class HostFedPoseSets:
    """The graph protocol of openslam_g2o_amd.lm over ONE library handle whose EdgeSBACam / EdgeSBAScale sets are ordinary edge
    sets fed from the host: every evaluation reads the cameras back, evaluates sbacam.py in fp64 and uploads J0 / J1 / err through
    g2ohip_set_edge_data.  The cameras, the projection set (when there is one) and the update stay with the device front end."""

    def __init__(self, s, g, sets):
        self.s, self.g, self.sets, self.J = s, g, sets, {}

    def _feed(self, jac):
        self.s.pgLinearize(jac)
        cams = self.s.pgGetEstimates()
        for k, key, scale in self.sets:
            e = self.g[key]
            r = H.pose_edges(H.FP64, cams, e["vi"], e["vj"], e["meas"], self.g["hidx"], scale=scale, jac=jac)
            if jac:
                self.J[k] = (r[0], r[1])
            self.s.setEdgeData(k, self.J[k][0], self.J[k][1], e["info"], r[2] if jac else r)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


def _fed_setup(g, huber):
    capi = _capi()
    s = capi.HipBlockSolver(6, 3, 0)
    hidx = np.asarray(g["hidx"], np.int32)
    none = np.zeros(0, np.int32)
    points = len(g["vp"]) > 0
    k0 = s.addEdgeSet(6, none, none)
    if points:
        k1 = s.addEdgeSet(g["zl"].shape[1], hidx[g["vp"]], g["pt_hidx"][g["vl"]])
    kc = s.addEdgeSet(6, hidx[g["cam_edges"]["vi"]], hidx[g["cam_edges"]["vj"]])
    ks = s.addEdgeSet(1, hidx[g["scale_edges"]["vi"]], hidx[g["scale_edges"]["vj"]])
    s.buildStructure(g["nP"], g["nL"] if points else 0, points)
    s.pgSetEdges(k0, 12, none, none, np.zeros((0, 7)), np.zeros((0, 36)))
    s.pgSetEstimates(g["est"], hidx)
    if points:
        s.pgSetCamProjectEdges(k1, 11 + g["zl"].shape[1], g["vp"], g["vl"], g["zl"], g["omega_l"], g["intrinsics"])
        s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
    if huber:
        s.setRobustKernel(kc, capi.KERNEL_HUBER, huber)
    return s, HostFedPoseSets(s, g, [(kc, "cam_edges", False), (ks, "scale_edges", True)])


@pytest.mark.parametrize("tag,points,huber", [("ba", True, 0.0), ("pose", False, 0.0), ("huber", True, H.HUBER)])
def test_lm_run(tag, points, huber):
    """make_sbacam_ba(12 cameras, 60 points, cam_edges=4, scale_edges=2), ten LM iterations from LM_LAMBDA: with the projection
    set, without it (a pure pose graph), and with Huber on the EdgeSBACam set."""
    g = H.lm_problem(points)
    s, graph = lm.setup_device_sbacam_ba(g, cam_huber_delta=huber)
    assert s.cam_set is not None and s.scale_set is not None and (s.landmark_sets[1] is not None) == points
    graph.compute_active_errors()
    chi0 = graph.chi2()
    done, chis, _, trials = lm.optimize(graph, s, H.ITERATIONS, "lm", user_lambda_init=H.LM_LAMBDA)
    f, fgraph = _fed_setup(g, huber)
    fdone, fchis, _, ftrials = lm.optimize(fgraph, f, H.ITERATIONS, "lm", user_lambda_init=H.LM_LAMBDA)
    chis, fchis, rec = np.array(chis), np.array(fchis), GOLD["lm_%s_rel" % tag]
    rel = np.abs(chis - fchis) / np.abs(fchis)
    print(tag, "chi2", chi0, "->", chis, "trials", trials, "fed", ftrials, "recorded", list(GOLD["lm_%s_trials" % tag]),
          "\n rel chi2 device vs fed", rel, "\n recorded fp64 vs mpmath", rec,
          "\n cameras device vs fed", H.transform_gap(s.pgGetEstimates(), f.pgGetEstimates()), "recorded", GOLD["lm_%s_est_drift" % tag][0])
    assert done == fdone == H.ITERATIONS
    assert list(trials) == list(ftrials)
    assert abs(chi0 - GOLD["lm_%s_chi0" % tag][0]) <= 1e-9 * chi0
    for it in range(H.ITERATIONS):
        bound = MARGIN * rec[it] if rec[it] > 0 else 4 * np.finfo(float).eps
        assert rel[it] <= bound, (it, rel[it], bound)
    assert chis[-1] < 0.01 * chi0
    assert np.array_equal(s.pgGetEstimates()[0], g["est"][0])        # the fixed camera


def test_stack():
    """push -> update -> pop restores the cameras and the next linearize reproduces J / err bit for bit; discard keeps the step."""
    cam, scale = _gold("c22"), _gold("s22")
    s, graph = _setup(cam, scale)
    graph.linearize()
    ref = _data(s, cam, False) + _data(s, scale, True)
    rng = np.random.default_rng(4)
    s.setX((rng.normal(size=(cam["nP"], 6)) * np.array([0.1] * 3 + [0.03] * 3)).ravel())
    graph.push()
    graph.update()
    moved = s.pgGetEstimates()
    assert np.array_equal(moved[0], cam["est"][0]) and (moved[1:] != cam["est"][1:]).any(axis=1).all()
    graph.linearize()
    new = _data(s, cam, False) + _data(s, scale, True)
    assert not np.array_equal(new[2], ref[2]) and not np.array_equal(new[5], ref[5])
    graph.pop()
    assert np.array_equal(s.pgGetEstimates(), cam["est"])
    graph.linearize()
    assert all(np.array_equal(a, b) for a, b in zip(_data(s, cam, False) + _data(s, scale, True), ref))
    graph.push()
    graph.update()
    graph.discard_top()
    assert np.array_equal(s.pgGetEstimates(), moved)
    graph.linearize()
    assert all(np.array_equal(a, b) for a, b in zip(_data(s, cam, False) + _data(s, scale, True), new))
    with pytest.raises(_capi().G2oHipError):
        graph.pop()


def test_binding_rules():
    """Every refused call returns G2OHIP_ERR_ARG (G2OHIP_ERR_STATE before a type-12 set exists) and the bound graph still
    linearizes to the same bits."""
    capi = _capi()
    Lb = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    cam, scale = _gold("c22"), _gold("s22")
    h = _i32(cam["hidx"])
    nv, n = len(h), 22
    vi, vj, z, w = _i32(cam["vi"]), _i32(cam["vj"]), _f64(cam["meas"]), _f64(cam["info"])
    si, sj, sz, sw = _i32(scale["vi"]), _i32(scale["vj"]), _f64(scale["meas"]), _f64(scale["info"])
    none_i, none_d = _i32(np.zeros(0)), _f64(np.zeros(0))

    def bind(s, k, typ, a=vi, b=vj, zz=z, ww=w):
        p = lambda x, f: None if x is None else f(x)
        return Lb.g2ohip_pg_set_cam_edges(s.h, k, typ, p(a, _ip), p(b, _ip), p(zz, _dp), p(ww, _dp))

    def bind_scale(s, k, a=si, b=sj, zz=sz, ww=sw):
        return bind(s, k, 17, a, b, zz, ww)

    s = capi.HipBlockSolver(6, 3, 0)
    k0 = s.addEdgeSet(6, none_i, none_i)
    kc = s.addEdgeSet(6, h[vi], h[vj])
    ks = s.addEdgeSet(1, h[si], h[sj])
    kc2 = s.addEdgeSet(6, h[vi], h[vj])                                # the same edges again: for the rebinding
    k3 = s.addEdgeSet(3, h[vi], h[vj])                                # a binary pose-pose set of error_dim 3
    kq = s.addEdgeSet(6, h[vi], None)                                  # a unary set
    ke = s.addEdgeSet(6, none_i, none_i)                               # an empty set
    s.buildStructure(cam["nP"], 0, False)
    assert bind(s, kc, 16) == STATE                                    # no type-12 set yet
    assert Lb.g2ohip_pg_set_edges(s.h, k0, 12, None, None, None, None) == 0
    s._pg = (12, 7)
    s.pgSetEstimates(cam["est"], h)
    assert bind(s, kc, 16) == 0 and bind_scale(s, ks) == 0
    s.cam_set, s.scale_set = kc, ks
    s.pgLinearize(True)
    ref = _data(s, cam, False) + _data(s, scale, True)

    def still_bound():
        s.pgSetEstimates(cam["est"], h)                                # (same table: forces a fresh evaluation)
        s.pgLinearize(True)
        return all(np.array_equal(a, b) for a, b in zip(_data(s, cam, False) + _data(s, scale, True), ref))

    assert still_bound()
    for typ in (15, 18, 12):
        assert bind(s, kc, typ) == ARG and still_bound()               # not a type of this entry
    assert bind(s, ks, 16) == ARG and bind(s, k3, 16) == ARG and still_bound()      # type 16 with error_dim 1 / 3
    assert bind_scale(s, kc2) == ARG and bind_scale(s, k3) == ARG and still_bound()  # type 17 with error_dim 6 / 3
    assert bind(s, kq, 16) == ARG and still_bound()                    # a unary set
    assert bind(s, k0, 16, none_i, none_i, none_d, none_d) == ARG and still_bound()  # bound as the pose-pose set
    assert bind_scale(s, kc) == ARG and bind(s, ks, 16) == ARG and still_bound()    # bound in the other slot
    for hole in range(4):                                              # a null array with n > 0
        args = [vi, vj, z, w]
        args[hole] = None
        assert bind(s, kc, 16, *args) == ARG and still_bound()
        args = [si, sj, sz, sw]
        args[hole] = None
        assert bind_scale(s, ks, *args) == ARG and still_bound()
    for v in (np.nan, np.inf):
        bad = z.copy()
        bad[n - 1, 1] = v
        assert bind(s, kc, 16, zz=bad) == ARG and still_bound()        # non-finite measurement
        bad = w.copy()
        bad[3, 7] = v
        assert bind(s, kc, 16, ww=bad) == ARG and still_bound()        # non-finite information
        bad = sz.copy()
        bad[5] = v
        assert bind_scale(s, ks, zz=bad) == ARG and still_bound()
        bad = sw.copy()
        bad[0] = v
        assert bind_scale(s, ks, ww=bad) == ARG and still_bound()
    bad = z.copy()
    bad[4, 3:] = 0.0
    assert bind(s, kc, 16, zz=bad) == ARG and still_bound()            # a measurement quaternion of norm 0
    for a, b in ((vi, si), (vj, sj)):
        for v in (nv, -1):                                             # a vertex index outside the pose table
            bad, sbad = a.copy(), b.copy()
            bad[n - 1] = sbad[0] = v
            assert (bind(s, kc, 16, bad, vj) if a is vi else bind(s, kc, 16, vi, bad)) == ARG and still_bound()
            assert (bind_scale(s, ks, sbad, sj) if a is vi else bind_scale(s, ks, si, sbad)) == ARG and still_bound()
    bad = vi.copy()
    bad[6] = (vi[6] + 1) % nv                                          # a hessian index that differs from the set's
    assert h[bad[6]] != h[vi[6]]
    assert bind(s, kc, 16, bad, vj) == ARG and still_bound()
    # pg_set_edges: types 1 / 2 / 10 while a slot is bound; a type-12 set with n > 0 still names EdgeSBACam
    for typ in (1, 2, 10):
        assert Lb.g2ohip_pg_set_edges(s.h, k0, typ, _ip(none_i), _ip(none_i), _dp(none_d), _dp(none_d)) == ARG and still_bound()
    assert Lb.g2ohip_pg_set_edges(s.h, kc2, 12, _ip(vi), _ip(vj), _dp(z), _dp(w)) == ARG
    assert b"EdgeSBACam" in Lb.g2ohip_last_error() and still_bound()
    # the other pg_set_* entries refuse the ids of the two slots
    ident = _f64(np.tile([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], (n, 1)))
    kc5 = _f64(np.tile([500.0, 500.0, 320.0, 240.0, 0.1], (nv, 1)))
    for k in (kc, ks):
        assert Lb.g2ohip_pg_set_edges(s.h, k, 12, _ip(vi), _ip(vj), _dp(z), _dp(w)) == ARG and still_bound()
        assert Lb.g2ohip_pg_set_prior_edges(s.h, k, 9, _ip(vi), _dp(ident), _dp(w), None) == ARG and still_bound()
        assert Lb.g2ohip_pg_set_cam_project_edges(s.h, k, 13, _ip(vi), _ip(vj), _dp(z), _dp(w), nv, _dp(kc5)) == ARG and still_bound()
        assert Lb.g2ohip_pg_set_gicp_edges(s.h, k, _ip(vi), _ip(vj), _dp(z), _dp(w), None) == ARG and still_bound()
    # a later pg_set_estimates with a table the sets do not fit
    assert Lb.g2ohip_pg_set_estimates(s.h, nv - 1, _dp(_f64(cam["est"][:-1])), _ip(h[:-1])) == ARG and still_bound()
    # n = 0 is accepted (NULL arrays), then the full set again
    assert bind(s, ke, 16, None, None, None, None) == 0
    s.pgSetEstimates(cam["est"], h)
    s.pgLinearize(True)
    assert Lb.g2ohip_build_system(s.h) == STATE                        # kc left the slot: its device-written data is cleared
    assert bind(s, kc, 16) == 0 and still_bound()
    # rebinding replaces the set: kc2 takes the slot and evaluates to the same bits, kc keeps no data
    assert bind(s, kc2, 16) == 0
    s.cam_set = kc2
    assert still_bound()
    assert Lb.g2ohip_build_system(s.h) == STATE
    assert bind(s, kc, 16) == 0
    s.cam_set = kc
    assert still_bound()
    # binding the same arrays again in either order keeps the pair
    assert bind_scale(s, ks) == 0 and bind(s, kc, 16) == 0 and still_bound()

    # the new entry beside pose types 1, 2 and 10
    for p, l, typ, stride in ((3, 2, 1, 3), (6, 3, 2, 12), (7, 3, 10, 8)):
        t = capi.HipBlockSolver(p, l, 0)
        ka = t.addEdgeSet(p, h[vi], h[vj])
        kb = t.addEdgeSet(6 if p == 6 else p, h[vi], h[vj])
        kd = t.addEdgeSet(1, h[si], h[sj])
        t.buildStructure(cam["nP"], 0, False)
        assert bind(t, kb, 16) == STATE
        meas = np.zeros((n, stride))
        if typ == 10:
            meas[:, 3] = meas[:, 7] = 1.0
        if typ == 2:
            meas[:] = [1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
        assert Lb.g2ohip_pg_set_edges(t.h, ka, typ, _ip(vi), _ip(vj), _dp(_f64(meas)), _dp(_f64(np.tile(np.eye(p).ravel(), (n, 1))))) == 0
        assert bind(t, kb, 16) == ARG and bind_scale(t, kd) == ARG
    # the Python wrapper forgets the bindings where the library drops them
    s.clearEdgeSets()
    assert s.cam_set is None and s.scale_set is None
