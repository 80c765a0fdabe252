"""GPU: anchored inverse-depth bundle adjustment on the device -- three-vertex EdgeProjectPSI2UV observations bound through
g2ohip_ba_set_inverse_depth_edges into the BA front end's projection slot as three binary sets: the producer against the fp64
restatement within 8 x its recorded drift from 60 digits (tests/golden/psi2uv_edges.npz), the assembled system against a dense
NumPy n-ary assembly, whole Levenberg-Marquardt runs device-resident against host-fed, the estimate stack, an EdgeSE3Expmap set
beside it, the binding rules."""
import numpy as np
import pytest

from openslam_g2o_amd import lm, psi2uv as X, se3expmap, synthetic as S
from tests import psi2uv_helpers as H
from tests.helpers import relerr

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE
TOL_MAT = 1e-12          # assembled blocks and right-hand side, TOL_CHI for chi2: tests/test_gpu_parity.py (_cmp_system) and
TOL_CHI = 1e-9           # tests/test_gpu_multi_edge.py
KPP, KPA, KCA = 0, 1, 2  # ids of the three sets behind lm.setup_device_ba: (point, pose), (point, anchor), (pose, anchor)


def _capi():
    from openslam_g2o_amd import capi
    return capi


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN)


def _bound(drift, *arrays):
    """8 x the recorded drift; a drift of exactly 0 is floored at 4 ulp of the largest magnitude (tests/test_gpu_se3expmap.py)."""
    return H.DRIFT_FACTOR * drift if drift > 0 else 4 * np.spacing(max(np.abs(a).max() for a in arrays))


def _data(s, n):
    """(J_point, J_pose, J_anchor, err) of the binding, every array through BOTH sets that hold it (they share the buffers)."""
    jp, jc, e = s.edgeData(KPP, n, 2, 3, 6)
    jp2, ja, e2 = s.edgeData(KPA, n, 2, 3, 6)
    jc2, ja2, e3 = s.edgeData(KCA, n, 2, 6, 6)
    assert np.array_equal(jp, jp2) and np.array_equal(jc, jc2) and np.array_equal(ja, ja2) and np.array_equal(e, e2) and np.array_equal(e, e3)
    return jp, jc, ja, e


def _err(s, n, k=KPP):
    e = np.empty((n, 2))
    assert s.L.g2ohip_copy_edge_data(s.h, k, None, None, _capi()._dp(e)) == 0
    return e


def _set_estimates(s, g, cams=None, pts=None):
    s.baSetEstimates(g["cams"] if cams is None else cams, g["cam_hidx"], g["pts"] if pts is None else pts, g["pt_hidx"])


@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_producers_against_mpmath(golden, n):
    z = golden
    g = H.load_graph(z, n)
    s, _ = lm.setup_device_ba(g)
    s.baLinearize(True)
    dev = _data(s, n)
    F = H.producers(g)
    drift = z["drift_%d" % n]
    be = _bound(drift[0], z["ref_err"][:n])
    bj = _bound(drift[1], z["ref_Jp"][:n], z["ref_Jc"][:n], z["ref_Ja"][:n])
    figs = dict(err=np.abs(dev[3] - F[3]).max(), J=max(np.abs(dev[i] - F[i]).max() for i in range(3)), bound_err=be, bound_J=bj)
    print(n, figs, "against 60 digits", np.abs(dev[3] - z["ref_err"][:n]).max())
    assert figs["err"] <= be and figs["J"] <= bj, figs
    assert all(np.all(np.abs(dev[i]).max(axis=1) > 0) for i in range(3))        # blocks of fixed vertices are written like the others
    # the same estimates again, errors only: bit-identical errors, the Jacobians stay
    _set_estimates(s, g)
    s.baLinearize(False)
    for k in (KPP, KPA, KCA):
        assert np.array_equal(_err(s, n, k), dev[3])
    again = _data(s, n)
    assert all(np.array_equal(a, b) for a, b in zip(again, dev))
    # moved estimates, errors only: the Jacobians still stay
    _set_estimates(s, g, z["step_cams"], z["step_pts"])
    s.baLinearize(False)
    e2 = _err(s, n)
    f2 = H.producers(g, z["step_cams"], z["step_pts"], jac=False)
    sd = z["step_drift_%d" % n]
    b2 = _bound(sd[0], z["step_ref_err"][:n])
    print(n, "moved, errors", np.abs(e2 - f2).max(), b2)
    assert np.abs(e2 - f2).max() <= b2 and not np.array_equal(e2, dev[3])
    kept = _data(s, n)
    assert all(np.array_equal(a, b) for a, b in zip(kept[:3], dev[:3]))
    # ... and with Jacobians
    s.baLinearize(True)
    dev2 = _data(s, n)
    F2 = H.producers(g, z["step_cams"], z["step_pts"])
    bj2 = _bound(sd[1], z["step_ref_Jp"][:n], z["step_ref_Jc"][:n], z["step_ref_Ja"][:n])
    fj = max(np.abs(dev2[i] - F2[i]).max() for i in range(3))
    print(n, "moved, Jacobians", fj, bj2)
    assert fj <= bj2 and np.array_equal(dev2[3], e2)


def _dense(g, J, omega, err, delta=0.0):
    """Dense H, b, chi2 of the three-vertex edges (tests/test_gpu_multi_edge._dense) over 6 nP + 3 nL unknowns."""
    from tests.test_gpu_multi_edge import _dense as dense
    nP, nL = g["nP"], g["nL"]
    dims = np.array([6] * nP + [3] * nL)
    offs = np.concatenate([[0], np.cumsum(dims)[:-1]])
    verts = np.stack([g["pairs"][0][0], g["pairs"][0][1], g["pairs"][1][1]], axis=1)
    Jm = [J[0].reshape(-1, 3, 2).transpose(0, 2, 1), J[1].reshape(-1, 6, 2).transpose(0, 2, 1), J[2].reshape(-1, 6, 2).transpose(0, 2, 1)]
    return dense(int(dims.sum()), dims, offs, verts, Jm, omega.reshape(-1, 2, 2).transpose(0, 2, 1), err, delta)


def _block_values(Hm, pattern, rows0, cols0, dr, dc):
    colptr, rowidx = pattern
    out = []
    for c in range(len(colptr) - 1):
        for q in range(colptr[c], colptr[c + 1]):
            r = rowidx[q]
            out.append(Hm[rows0 + dr * r:rows0 + dr * r + dr, cols0 + dc * c:cols0 + dc * c + dc].T.reshape(-1))   # column-major
    return np.concatenate(out)


@pytest.mark.parametrize("huber", [0.0, H.LM_HUBER])
def test_assembled_system_against_dense_numpy(golden, huber):
    """Hpp, Hpl, Hll, b, chi2 of the generic assembly of the three sets against a dense NumPy n-ary assembly of the device's own
    err / J / information (the 300-edge graph: fixed anchor, fixed observing camera, fixed point, a doubled (point, pose) pair,
    edges observed by their own anchor)."""
    capi = _capi()
    n = 300
    g = H.load_graph(golden, n)
    s, _ = lm.setup_device_ba(g, huber_delta=huber)
    s.baLinearize(True)
    jp, jc, ja, e = _data(s, n)
    Hm, b, chi = _dense(g, (jp, jc, ja), g["info"], e, huber)
    s.buildSystem()
    nP = g["nP"]
    for which, rows0, cols0, dr, dc, name in ((capi.HPP, 0, 0, 6, 6, "Hpp"), (capi.HPL, 0, 6 * nP, 6, 3, "Hpl"), (capi.HLL, 6 * nP, 6 * nP, 3, 3, "Hll")):
        if which == capi.HLL:
            want = np.concatenate([Hm[6 * nP + 3 * j:6 * nP + 3 * j + 3, 6 * nP + 3 * j:6 * nP + 3 * j + 3].T.reshape(-1) for j in range(g["nL"])])
        else:
            want = _block_values(Hm, s.pattern(which), rows0, cols0, dr, dc)
        fig = relerr(s.values(which), want)
        print(huber, name, fig)
        assert fig < TOL_MAT, name
    print(huber, "b", relerr(s.b(), b), "chi2", s.chi2(), chi)
    assert relerr(s.b(), b) < TOL_MAT
    assert abs(s.chi2() - chi) <= TOL_CHI * chi


class _HostFedGraph:
    """lm.py's graph protocol over the DEVICE solver with the three sets fed from the host: the estimates stay in the front end's
    tables (update / push / pop on the device), are read back for every evaluation, and the sets go through setEdgeData from
    psi2uv.py."""

    device_resident = False

    def __init__(self, s, g, ids):
        self.s, self.g, self.ids = s, g, ids
        self.J = None

    def _feed(self, jac):
        cams, pts = self.s.baGetEstimates()
        out = X.problem_edges(self.g, cams, pts, jac)
        if jac:
            self.J = out[:3]
        jp, jc, ja = self.J
        err = out[3] if jac else out
        om = H.omega_of(self.g)
        for k, (a, b) in zip(self.ids, ((jp, jc), (jp, ja), (jc, ja))):
            self.s.setEdgeData(k, a, b, om, err)

    def linearize(self):
        self._feed(True)

    def compute_active_errors(self):
        self._feed(False)

    def chi2(self):
        return self.s.chi2()

    def update(self):
        self.s.baUpdate()

    def push(self):
        self.s.baPush()

    def pop(self):
        self.s.baPop()

    def discard_top(self):
        self.s.baDiscardTop()


def _host_fed_solver(g, huber=0.0, options=None):
    capi = _capi()
    h = capi.HipBlockSolver(6, 3, 0)
    for name, value in (options or {}).items():
        h.setOption(name, value)
    parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
    ids = []
    for (v0, v1), pt in zip(g["pairs"], parts):
        ids.append(h.addEdgeSet(2, v0, v1))
        h.setEdgeSetParts(ids[-1], pt)
    h.buildStructure(g["nP"], g["nL"], True)
    h.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], np.arange(g["L"], dtype=np.int32))
    if huber > 0:
        for k in ids:
            h.setRobustKernel(k, capi.KERNEL_HUBER, huber)
    return h, _HostFedGraph(h, g, ids)


@pytest.mark.parametrize("kernel", ["plain", "huber"])
def test_whole_run_device_resident_against_host_fed(golden, kernel):
    """lm.optimize with the three sets produced on the device against the same loop fed from the NumPy restatement, over the same
    device solver: the chi2 trajectory and the final estimates differ by at most 8 x what the fp64-fed and the mpmath-fed runs
    over the CPU oracle differ by (recorded in the fixture; a recorded 0 is floored at 4 ulp).  Equal trial counts, decreasing
    chi2; use_graph = 1 gives the identical trajectory."""
    z = golden
    g = H.lm_graph()
    huber = H.LM_HUBER if kernel == "huber" else 0.0
    s, graph = lm.setup_device_ba(g, huber_delta=huber)
    n1, chi1, lam1, tr1 = lm.optimize(graph, s, H.LM_ITERATIONS, "lm")
    h, hgraph = _host_fed_solver(g, huber)
    n2, chi2, lam2, tr2 = lm.optimize(hgraph, h, H.LM_ITERATIONS, "lm")
    gaps = np.abs(np.array(chi1) - np.array(chi2)) / np.abs(np.array(chi2))
    rec = z["lm_%s_gap" % kernel]
    bound = [_bound(r, np.ones(1)) for r in rec]
    print(kernel, "chi2 device", chi1)
    print(kernel, "chi2 host-fed", chi2)
    print(kernel, "gaps", gaps, "bound", bound, "trials", tr1, tr2)
    assert n1 == n2 == H.LM_ITERATIONS and list(tr1) == list(tr2) == list(z["lm_%s_trials" % kernel])
    assert np.all(gaps <= bound), (gaps, bound)
    assert np.all(np.diff(chi1) < 0)
    a, b = s.baGetEstimates(), h.baGetEstimates()
    est = max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())
    eb = _bound(z["lm_%s_estimates" % kernel][0], a[0], a[1])
    print(kernel, "estimates", est, eb)
    assert est <= eb
    # and against the CPU oracle's trajectory: the same problem, another solver
    assert np.abs(np.array(chi1) - z["lm_%s_chis" % kernel]).max() <= 1e-9 * z["lm_%s_chis" % kernel][0]
    s3, graph3 = lm.setup_device_ba(g, huber_delta=huber, options={"use_graph": 1})
    n3, chi3, lam3, tr3 = lm.optimize(graph3, s3, H.LM_ITERATIONS, "lm")
    assert n3 == n1 and list(tr3) == list(tr1) and np.array_equal(chi3, chi1) and np.array_equal(lam3, lam1)
    c = s3.baGetEstimates()
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_estimate_stack(golden):
    n = 300
    g = H.load_graph(golden, n)
    s, graph = lm.setup_device_ba(g)
    graph.linearize()
    e0 = _err(s, n)
    s.buildSystem()
    s.setLambda(1e-3 * s.maxDiagonal(), True)
    assert s.solve()
    s.restoreDiagonal()
    cams0, pts0 = s.baGetEstimates()
    s.baPush()
    s.baUpdate()
    cams1, pts1 = s.baGetEstimates()
    free_c, free_p = g["cam_hidx"] >= 0, g["pt_hidx"] >= 0
    assert not np.array_equal(cams1[free_c], cams0[free_c]) and np.array_equal(cams1[~free_c], cams0[~free_c])
    assert not np.array_equal(pts1[free_p], pts0[free_p]) and np.array_equal(pts1[~free_p], pts0[~free_p])
    # the device's oplus: exp(u) T for the cameras, plain addition for psi
    x = s.x()
    upd = np.zeros((g["P"], 6))
    upd[free_c] = x[:6 * g["nP"]].reshape(-1, 6)[g["cam_hidx"][free_c]]
    assert np.abs(se3expmap.oplus(cams0, upd) - cams1).max() < 1e-12
    xl = x[6 * g["nP"]:].reshape(-1, 3)
    assert np.abs(pts0[free_p] + xl[g["pt_hidx"][free_p]] - pts1[free_p]).max() < 1e-14
    s.baLinearize(False)
    e1 = _err(s, n)
    assert not np.array_equal(e1, e0)
    assert np.abs(e1 - H.producers(g, cams1, pts1, jac=False)).max() < 1e-9
    s.baPop()
    cams2, pts2 = s.baGetEstimates()
    assert np.array_equal(cams2, cams0) and np.array_equal(pts2, pts0)
    s.baLinearize(False)
    assert np.array_equal(_err(s, n), e0)


def _with_pose_edges(g):
    """EdgeSE3Expmap odometry between the cameras of an inverse-depth problem (make_ba_odometry over the same scene)."""
    o = S.make_ba_odometry(g["P"], g["L"], loop_every=4)
    g = dict(g)
    g["pose_edges"] = o["pose_edges"]
    return g


def test_with_an_se3expmap_set_bound_beside_it():
    """The EdgeSE3Expmap slot keeps working beside the inverse-depth binding: its producer output, the assembled system against
    dense NumPy (n-ary edges + the binary pose set), and an LM run that descends."""
    capi = _capi()
    g = _with_pose_edges(S.make_ba_inverse_depth(12, 60))
    g["pt_hidx"] = np.arange(g["L"], dtype=np.int32)
    pe = g["pose_edges"]
    s, graph = lm.setup_device_ba(g)
    kp = 3
    graph.linearize()
    n = g["E"]
    jp, jc, ja, e = _data(s, n)
    F = H.producers(g)
    assert all(np.abs(a - b).max() < 1e-9 for a, b in zip((jp, jc, ja, e), F))
    d0, d1, de = s.edgeData(kp, pe["n"], 6, 6, 6)
    P0, P1, pe_err = se3expmap.pose_edges(g["cams"], pe["vi"], pe["vj"], pe["meas"])
    assert relerr(d0, P0) < 1e-13 and relerr(d1, P1) < 1e-13 and np.abs(de - pe_err).max() < 1e-13
    Hm, b, chi = _dense(g, (jp, jc, ja), S.ba_omega(g), e)
    from tests.test_gpu_se3expmap import _dense as dense_binary
    H2, b2, chi2 = dense_binary(g, [(pe["v0"], pe["v1"], 6, 6, 6, d0, d1, pe["info"], de)])
    Hm, b, chi = Hm + H2, b + b2, chi + chi2
    s.buildSystem()
    nP = g["nP"]
    for which, rows0, cols0, dr, dc, name in ((capi.HPP, 0, 0, 6, 6, "Hpp"), (capi.HPL, 0, 6 * nP, 6, 3, "Hpl")):
        fig = relerr(s.values(which), _block_values(Hm, s.pattern(which), rows0, cols0, dr, dc))
        print(name, fig)
        assert fig < TOL_MAT, name
    assert relerr(s.b(), b) < TOL_MAT and abs(s.chi2() - chi) <= TOL_CHI * chi
    done, chis, lams, trials = lm.optimize(graph, s, 4, "lm")
    print("with pose edges", chis, trials)
    assert done == 4 and np.all(np.diff(chis) < 0)
    # rebinding the projection slot keeps the pose binding
    s.baSetInverseDepthEdges(*s.psi_sets, g["cam_idx"], g["anchor_idx"], g["pt_idx"], g["meas"], None, g["f"], g["cx"], g["cy"])
    s.baLinearize(True)
    cams, _ = s.baGetEstimates()
    assert np.abs(s.edgeData(kp, pe["n"], 6, 6, 6)[2] - se3expmap.pose_edges(cams, pe["vi"], pe["vj"], pe["meas"], jac=False)).max() < 1e-12


def test_binding_rules(golden):
    capi = _capi()
    L = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    n = 65
    g = H.load_graph(golden, n)
    cv, av, pv, m, info = _i32(g["cam_idx"]), _i32(g["anchor_idx"]), _i32(g["pt_idx"]), _f64(g["meas"]), _f64(g["info"])
    ref = H.producers(g)
    f, cx, cy = g["f"], g["cx"], g["cy"]
    P_ALL, P_OFF = capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2
    (vp, vc), (_, va), _ = g["pairs"]

    s = capi.HipBlockSolver(6, 3, 0)
    ids = []
    for (v0, v1), pt in zip(g["pairs"], (0, P_ALL, P_OFF)):
        ids.append(s.addEdgeSet(2, v0, v1))
        s.setEdgeSetParts(ids[-1], pt)
    kpp, kpa, kca = ids
    k_parts = s.addEdgeSet(2, vp, va)                                    # (point, anchor) with the parts left at 0
    k_short = s.addEdgeSet(2, vc[:n - 1], va[:n - 1])                    # (pose, anchor), one edge short
    s.setEdgeSetParts(k_short, P_OFF)
    k_d3 = s.addEdgeSet(3, vp, vc)                                       # (point, pose) of another error dimension
    # a mono binding to alternate with: EdgeProjectXYZ2UV over the edges that are not observed by their own anchor
    own = g["cam_idx"] == g["anchor_idx"]
    k_mono = s.addEdgeSet(2, vp[~own], vc[~own])
    n_mono = int((~own).sum())

    def psi(k0=kpp, k1=kpa, k2=kca, c=cv, a=av, p=pv, mm=m, ii=info, ff=f):
        return L.g2ohip_ba_set_inverse_depth_edges(s.h, k0, k1, k2, None if c is None else _ip(c), None if a is None else _ip(a),
                                                   None if p is None else _ip(p), None if mm is None else _dp(mm),
                                                   None if ii is None else _dp(ii), ff, cx, cy)

    def feed_others():
        for k, nn, d, d0, d1 in ((k_parts, n, 2, 3, 6), (k_short, n - 1, 2, 6, 6), (k_d3, n, 3, 3, 6), (k_mono, n_mono, 2, 3, 6)):
            s.setEdgeData(k, np.zeros((nn, d * d0)), np.zeros((nn, d * d1)), np.tile(np.eye(d).reshape(-1), (nn, 1)), np.zeros((nn, d)))

    def still_works(want=ref):
        _set_estimates(s, g)                                             # (same tables: only invalidates the evaluation)
        s.baLinearize(True)
        got = _data(s, n)
        assert all(np.abs(a - r).max() < 1e-9 for a, r in zip(got, want))

    def rejected(rc, code=ARG):
        """The call was refused with `code`, and the binding it found is untouched: a linearize of it gives the same data."""
        assert rc == code, (rc, code)
        still_works()

    assert psi() == STATE                                                # before buildStructure
    s.buildStructure(g["nP"], g["nL"], True)
    assert psi() == 0                                                    # before the estimates: validated by baSetEstimates
    feed_others()
    _set_estimates(s, g)
    still_works()
    # every refusal is followed by a linearize of the binding it found, before anything binds again
    rejected(psi(k0=99))                                                 # no such set
    rejected(psi(k1=-1))
    rejected(psi(k1=kpp))                                                # the same set twice
    rejected(psi(k2=kpa))
    rejected(psi(k0=k_d3))                                               # error_dim 3
    rejected(psi(k0=kpa, k1=kpp))                                        # parts on the wrong sets
    rejected(psi(k1=k_parts))                                            # parts 0 on the (point, anchor) set
    rejected(psi(k2=k_short))                                            # unequal n
    rejected(psi(k2=kpa, k1=kca))                                        # dimensions
    rejected(psi(c=None))
    rejected(psi(a=None))
    rejected(psi(p=None))
    rejected(psi(mm=None))
    bad = m.copy()
    bad[7, 1] = np.nan
    rejected(psi(mm=bad))
    bad = info.copy()
    bad[n - 1, 3] = np.inf
    rejected(psi(ii=bad))
    rejected(psi(ff=0.0))
    rejected(psi(ff=np.nan))
    bad = cv.copy()
    bad[9] = g["P"]
    rejected(psi(c=bad))                                                 # outside the camera table
    bad = av.copy()
    bad[11] = g["P"] + 3
    rejected(psi(a=bad))                                                 # ... an anchor
    bad = pv.copy()
    bad[0] = -1
    rejected(psi(p=bad))
    bad = pv.copy()
    bad[12] = g["L"]
    rejected(psi(p=bad))
    free = np.nonzero(g["cam_hidx"] >= 0)[0]
    k_free = int(np.nonzero(~own & (g["cam_hidx"][g["cam_idx"]] >= 0))[0][0])
    bad = cv.copy()
    bad[k_free] = next(int(c) for c in free if c != cv[k_free] and c != av[k_free])
    rejected(psi(c=bad))                                                 # a camera whose hessian index disagrees with the sets
    k_anc = int(np.nonzero(~own & (g["cam_hidx"][g["anchor_idx"]] >= 0))[0][0])
    bad = av.copy()
    bad[k_anc] = next(int(c) for c in free if c != cv[k_anc] and c != av[k_anc])
    rejected(psi(a=bad))                                                 # ... an anchor
    # the anchor's own observation: such an edge carries -1 on every camera side -- an observing pose moved ONTO its anchor is
    # refused (its sets hold the camera's index), and so is an own observation moved off its anchor (its sets hold -1)
    bad = cv.copy()
    bad[k_free] = av[k_free]
    rejected(psi(c=bad))
    k_own = int(np.nonzero(own)[0][0])
    bad = cv.copy()
    bad[k_own] = next(int(c) for c in free if c != av[k_own])
    rejected(psi(c=bad))
    # new tables validate the binding again, anchors included
    hx = g["cam_hidx"].copy()
    a_free = int(av[k_anc])
    other = next(int(c) for c in free if c != a_free)
    hx[a_free], hx[other] = hx[other], hx[a_free]
    rejected(L.g2ohip_ba_set_estimates(s.h, g["P"], _dp(_f64(g["cams"])), _ip(_i32(hx)), g["L"], _dp(_f64(g["pts"])), _ip(_i32(g["pt_hidx"]))))
    rejected(L.g2ohip_ba_set_estimates(s.h, int(av.max()), _dp(_f64(g["cams"])), _ip(_i32(g["cam_hidx"])), g["L"], _dp(_f64(g["pts"])),
                                       _ip(_i32(g["pt_hidx"]))))     # a table that ends before the last anchor
    # per-edge kernels: refused at the binding (on any of the three), taken by the bound sets
    for k in ids:
        s.setRobustKernelPerEdge(k, np.zeros(n, np.int32), np.ones(n))
        still_works()
        rejected(psi(), STATE)
        s.setRobustKernelPerEdge(k, None, None)
    # replacing the binding: other measurements, identity information written on the device
    m2 = m + 0.5
    assert psi(mm=m2, ii=None) == 0
    want2 = X.edges(g["cams"], g["pts"], cv, av, pv, m2, f, cx, cy)
    still_works(want2)
    assert not np.array_equal(want2[3], ref[3])
    s.buildSystem()
    chi = float((want2[3] ** 2).sum())
    assert abs(s.chi2() - chi) <= 1e-12 * chi                            # (identity information; the other sets hold zero errors)
    # a mono binding takes the slot: the three sets lose their device-written data ...
    s.baSetEdges(k_mono, cv[~own], pv[~own], m[~own], None, f, cx, cy)
    _set_estimates(s, g)
    s.baLinearize(True)
    assert L.g2ohip_build_system(s.h) == STATE
    e = np.empty((n, 2))
    for k in ids:
        assert L.g2ohip_copy_edge_data(s.h, k, None, None, _dp(e)) == STATE
    e_mono = np.empty((n_mono, 2))
    assert L.g2ohip_copy_edge_data(s.h, k_mono, None, None, _dp(e_mono)) == 0
    assert np.isfinite(e_mono).all()
    # ... and back: the inverse-depth binding replaces the mono one, which leaves without data
    assert psi() == 0
    still_works()
    assert L.g2ohip_build_system(s.h) == STATE                           # k_mono has to be fed by the host again
    feed_others()
    still_works()
    s.buildSystem()
    Hm, b, chi = _dense(g, ref[:3], g["info"], ref[3])
    assert abs(s.chi2() - chi) <= TOL_CHI * chi and relerr(s.b(), b) < 1e-9
    # host arrays handed to one of the bound sets are replaced by the next device evaluation, shared buffers included
    s.setEdgeData(kpa, np.zeros((n, 6)), np.zeros((n, 12)), np.tile(np.eye(2).reshape(-1), (n, 1)), np.zeros((n, 2)))
    still_works()
    # growth by update_structure is refused with marginalised points, as for every Schur structure: the binding stays
    assert L.g2ohip_update_structure(s.h, 0, kpp, 0, None, None) == capi.ERR_UNSUPPORTED
    still_works()
    # the binding goes with clearEdgeSets and comes back
    s.clearEdgeSets()
    assert L.g2ohip_ba_linearize(s.h, 1) == STATE
    ids = []
    for (v0, v1), pt in zip(g["pairs"], (0, P_ALL, P_OFF)):
        ids.append(s.addEdgeSet(2, v0, v1))
        s.setEdgeSetParts(ids[-1], pt)
    s.buildStructure(g["nP"], g["nL"], True)
    assert L.g2ohip_ba_linearize(s.h, 1) == STATE
    assert psi(*ids) == 0
    _set_estimates(s, g)
    s.baLinearize(True)
    got = _data(s, n)
    assert all(np.abs(a - r).max() < 1e-9 for a, r in zip(got, ref))


def test_the_bound_pose_edge_set_is_refused():
    """One of the three sets being the set bound in the EdgeSE3Expmap slot: G2OHIP_ERR_ARG, both bindings intact.  (A (6, 6) set
    of error dimension 6 fails the shape check as well; the test pins that the call is refused and nothing is lost.)"""
    capi = _capi()
    L = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = _with_pose_edges(S.make_ba_inverse_depth(12, 60))
    g["pt_hidx"] = np.arange(g["L"], dtype=np.int32)
    pe = g["pose_edges"]
    s, graph = lm.setup_device_ba(g)
    kp = 3
    rc = L.g2ohip_ba_set_inverse_depth_edges(s.h, 0, 1, kp, _ip(_i32(g["cam_idx"])), _ip(_i32(g["anchor_idx"])), _ip(_i32(g["pt_idx"])),
                                             _dp(_f64(g["meas"])), None, g["f"], g["cx"], g["cy"])
    assert rc == ARG
    s.baLinearize(True)
    F = H.producers(g)
    got = _data(s, g["E"])
    assert all(np.abs(a - b).max() < 1e-9 for a, b in zip(got, F))
    assert np.abs(s.edgeData(kp, pe["n"], 6, 6, 6)[2] - se3expmap.pose_edges(g["cams"], pe["vi"], pe["vj"], pe["meas"], jac=False)).max() < 1e-12
