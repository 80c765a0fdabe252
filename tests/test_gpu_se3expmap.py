"""GPU: pose-pose constraints in device-resident bundle adjustment -- EdgeSE3Expmap edges bound through
g2ohip_ba_set_pose_edges into the BA front end's second slot, beside a mono (fused or generic) or stereo projection set: the
producer against the fp64 restatement within 8 x its recorded drift from 60 digits (tests/golden/se3expmap_edges.npz), the
Jacobians on the fused path, the assembled system against dense NumPy, whole Levenberg-Marquardt runs device-resident against
host-fed, the estimate stack, the binding rules."""
import numpy as np
import pytest

from openslam_g2o_amd import lm, se3expmap as X, synthetic as S
from tests import se3expmap_helpers as H
from tests.helpers import relerr

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE
TOL_MAT = 1e-12          # assembled blocks and right-hand side, TOL_CHI for chi2: tests/test_gpu_parity.py (_cmp_system, which
TOL_CHI = 1e-9           # test_edge_cases_mixed_sets_fixed_and_unary holds its mixed sets to)
TOL_FUSED = 2e-12        # fused against generic: tests/test_gpu_lm.py holds each of the two to the oracle within 1e-12
KP = 1                   # id of the pose set behind lm.setup_device_ba


def _capi():
    from openslam_g2o_amd import capi
    return capi


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN)


def _bound(drift, *arrays):
    """8 x the recorded drift; a drift of exactly 0 is floored at 4 ulp of the largest magnitude (tests/test_gpu_sbacam.py)."""
    return H.DRIFT_FACTOR * drift if drift > 0 else 4 * np.spacing(max(np.abs(a).max() for a in arrays))


def _pose_data(s, n):
    return s.edgeData(KP, n, 6, 6, 6)


def _pose_err(s, n):
    e = np.empty((n, 6))
    assert s.L.g2ohip_copy_edge_data(s.h, KP, None, None, _capi()._dp(e)) == 0
    return e


@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_producers_against_mpmath(golden, n):
    z = golden
    g = H.load_graph(z, n)
    s, _ = lm.setup_device_ba(g)
    s.baLinearize(True)
    d0, d1, de = _pose_data(s, n)
    F0, F1, fe = H.producers(g)
    drift = z["drift_%d" % n]
    be = _bound(drift[0], z["ref_err"][:n])
    bj = _bound(drift[1], z["ref_J0"][:n], z["ref_J1"][:n])
    figs = dict(err=np.abs(de - fe).max(), J=max(np.abs(d0 - F0).max(), np.abs(d1 - F1).max()), bound_err=be, bound_J=bj)
    print(n, figs, "against 60 digits", np.abs(de - z["ref_err"][:n]).max())
    assert figs["err"] <= be and figs["J"] <= bj, figs
    assert np.all(np.abs(d0).max(axis=1) > 0) and np.all(np.abs(d1).max(axis=1) > 0)
    if n > 5:
        assert not np.any(de[5])                                         # identical poses, identity measurement
    # the same estimates again, errors only: bit-identical errors, the Jacobians stay
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], np.arange(g["L"], dtype=np.int32))
    s.baLinearize(False)
    assert np.array_equal(_pose_err(s, n), de)
    x0, x1, _ = _pose_data(s, n)
    assert np.array_equal(x0, d0) and np.array_equal(x1, d1)
    # moved cameras, errors only
    s.baSetEstimates(z["step_cams"], g["cam_hidx"], g["pts"], np.arange(g["L"], dtype=np.int32))
    s.baLinearize(False)
    e2 = _pose_err(s, n)
    f2 = H.producers(g, cams=z["step_cams"], jac=False)
    b2 = _bound(z["step_drift_%d" % n][0], z["step_ref_err"][:n])
    print(n, "moved", np.abs(e2 - f2).max(), b2)
    assert np.abs(e2 - f2).max() <= b2
    x0, x1, _ = _pose_data(s, n)
    assert np.array_equal(x0, d0) and np.array_equal(x1, d1)


def _solve(s, lam=10.0):
    s.buildSystem()
    b, chi = s.b(), s.chi2()
    Hpp = s.values(_capi().HPP)
    s.setLambda(lam, True)
    assert s.solve()
    s.restoreDiagonal()
    return Hpp, b, chi, s.x()


@pytest.mark.parametrize("stereo", [False, True])
def test_fused_path_writes_the_pose_jacobians(stereo):
    """ba_fused on: ba_linearize(True) produces no projection Jacobians (build_system re-evaluates them) but must produce the pose
    set's; the system equals the one of ba_fused = 0.  With a stereo projection set both runs take the generic path."""
    g = S.make_ba_odometry(12, 60, loop_every=4, **({"stereo_baseline": 0.2} if stereo else {}))
    n = g["pose_edges"]["n"]
    out = []
    for fused in (1, 0):
        s, _ = lm.setup_device_ba(g, options={"ba_fused": fused})
        s.baLinearize(False)                                             # (an error-only evaluation first: the early return must not swallow the Jacobians)
        s.baLinearize(True)
        d0, d1, de = _pose_data(s, n)
        F0, F1, fe = H.producers(g)
        assert np.abs(d0).max() > 0.5 and relerr(d0, F0) < 1e-13 and relerr(d1, F1) < 1e-13 and np.abs(de - fe).max() < 1e-13
        out.append(_solve(s))
    for a, b, name in zip(out[0], out[1], ("Hpp", "b", "chi2", "dx")):
        fig = relerr(np.atleast_1d(a), np.atleast_1d(b))
        print(stereo, name, fig)
        assert fig < (1e-9 if name == "dx" else TOL_FUSED), name


def _dense(g, sets):
    """H and b of the whole system from per-set (v0, v1, d0, d1, J0, J1, omega, err); sizes (6 nP + 3 nL)."""
    nP, nL = g["nP"], g["nL"]
    N = 6 * nP + 3 * nL
    Hm, b, chi = np.zeros((N, N)), np.zeros(N), 0.0

    def rng_of(v):
        return slice(6 * v, 6 * v + 6) if v < nP else slice(6 * nP + 3 * (v - nP), 6 * nP + 3 * (v - nP) + 3)
    for v0, v1, d, d0, d1, J0, J1, om, err in sets:
        for k in range(len(v0)):
            A, B = J0[k].reshape(d0, d).T, J1[k].reshape(d1, d).T
            W, e = om[k].reshape(d, d), err[k]
            chi += e @ W @ e
            for va, Ja in ((v0[k], A), (v1[k], B)):
                if va < 0:
                    continue
                b[rng_of(va)] -= Ja.T @ W @ e
                for vb, Jb in ((v0[k], A), (v1[k], B)):
                    if vb >= 0:
                        Hm[rng_of(va), rng_of(vb)] += Ja.T @ W @ Jb
    return Hm, b, chi


def _block_values(Hm, pattern, rows0, cols0, dr, dc):
    colptr, rowidx = pattern
    out = []
    for c in range(len(colptr) - 1):
        for q in range(colptr[c], colptr[c + 1]):
            r = rowidx[q]
            out.append(Hm[rows0 + dr * r:rows0 + dr * r + dr, cols0 + dc * c:cols0 + dc * c + dc].T.reshape(-1))   # column-major
    return np.concatenate(out)


def test_assembled_system_against_dense_numpy(golden):
    """Hpp, Hpl, Hll, b, chi2 of the generic assembly against a dense NumPy assembly of the device's own err / J / information
    of both sets (the 65-edge graph: edges to the fixed camera on either side, a doubled pair, a pair in both orders)."""
    capi = _capi()
    n = 65
    g = H.load_graph(golden, n)
    pe = g["pose_edges"]
    s, _ = lm.setup_device_ba(g, options={"ba_fused": 0})
    s.baLinearize(True)
    Jp, Jc, e = s.edgeData(0, g["E"], 2, 3, 6)
    d0, d1, de = _pose_data(s, n)
    Hm, b, chi = _dense(g, [(g["v0"], g["v1"], 2, 3, 6, Jp, Jc, S.ba_omega(g), e), (pe["v0"], pe["v1"], 6, 6, 6, d0, d1, pe["info"], de)])
    s.buildSystem()
    nP = g["nP"]
    for which, rows0, cols0, dr, dc, name in ((capi.HPP, 0, 0, 6, 6, "Hpp"), (capi.HPL, 0, 6 * nP, 6, 3, "Hpl"), (capi.HLL, 6 * nP, 6 * nP, 3, 3, "Hll")):
        if which == capi.HLL:
            want = np.concatenate([Hm[6 * nP + 3 * j:6 * nP + 3 * j + 3, 6 * nP + 3 * j:6 * nP + 3 * j + 3].T.reshape(-1) for j in range(g["nL"])])
        else:
            want = _block_values(Hm, s.pattern(which), rows0, cols0, dr, dc)
        fig = relerr(s.values(which), want)
        print(name, fig)
        assert fig < TOL_MAT, name
    print("b", relerr(s.b(), b), "chi2", s.chi2(), chi)
    assert relerr(s.b(), b) < TOL_MAT
    assert abs(s.chi2() - chi) <= TOL_CHI * chi


class _HostFedGraph:
    """lm.py's graph protocol over the DEVICE solver with the pose set fed from the host: the projection set stays in the front
    end, the cameras are read back for every evaluation and the pose set goes through setEdgeData from se3expmap.py."""

    device_resident = False

    def __init__(self, s, prob):
        self.s, self.pe = s, prob["pose_edges"]
        self.J = None

    def _feed(self, jac):
        cams, _ = self.s.baGetEstimates()
        out = X.pose_edges(cams, self.pe["vi"], self.pe["vj"], self.pe["meas"], jac)
        if jac:
            self.J = out[:2]
        self.s.setEdgeData(KP, self.J[0], self.J[1], self.pe["info"], out[2] if jac else out)

    def linearize(self):
        self._feed(True)
        self.s.baLinearize(True)

    def compute_active_errors(self):
        self._feed(False)
        self.s.baLinearize(False)

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


@pytest.mark.parametrize("kernel", ["plain", "huber"])
def test_whole_run_device_resident_against_host_fed(golden, kernel):
    """lm.optimize with both sets on the device against the same loop with the pose set fed from the NumPy restatement, over the
    same device solver: the chi2 trajectory and the final estimates differ by at most 8 x what the fp64-fed and the
    mpmath-fed runs over the CPU oracle differ by (recorded in the fixture; a recorded 0 is floored at 4 ulp).  The chi2
    decreases; use_graph = 1 gives the identical trajectory (as tests/test_gpu_stereo_ba.py holds it)."""
    capi = _capi()
    z = golden
    g = H.lm_graph()
    huber = H.LM_HUBER if kernel == "huber" else 0.0
    s, graph = lm.setup_device_ba(g, huber_delta_pose=huber)
    n1, chi1, lam1, tr1 = lm.optimize(graph, s, H.LM_ITERATIONS, "lm")
    h = capi.HipBlockSolver(6, 3, 0)                                     # the projection set in the front end, the pose set beside it, not bound
    k = h.addEdgeSet(2, g["v0"], g["v1"])
    kp = h.addEdgeSet(6, g["pose_edges"]["v0"], g["pose_edges"]["v1"])
    assert (k, kp) == (0, KP)
    h.buildStructure(g["nP"], g["nL"], True)
    h.baSetEdges(k, g["cam_idx"], g["pt_idx"], g["meas"], None, g["f"], g["cx"], g["cy"])
    h.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], np.arange(g["L"], dtype=np.int32))
    if huber > 0:
        h.setRobustKernel(kp, capi.KERNEL_HUBER, huber)
    n2, chi2, lam2, tr2 = lm.optimize(_HostFedGraph(h, g), h, H.LM_ITERATIONS, "lm")
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
    s3, graph3 = lm.setup_device_ba(g, huber_delta_pose=huber, options={"use_graph": 1})
    n3, chi3, lam3, tr3 = lm.optimize(graph3, s3, H.LM_ITERATIONS, "lm")
    assert n3 == n1 and list(tr3) == list(tr1) and np.array_equal(chi3, chi1) and np.array_equal(lam3, lam1)
    c = s3.baGetEstimates()
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_estimate_stack_with_both_sets_bound(golden):
    g = H.load_graph(golden, 65)
    s, graph = lm.setup_device_ba(g)
    graph.linearize()
    e0 = _pose_err(s, 65)
    s.buildSystem()
    s.setLambda(1e-3 * s.maxDiagonal(), True)
    assert s.solve()
    s.restoreDiagonal()
    cams0, pts0 = s.baGetEstimates()
    s.baPush()
    s.baUpdate()
    cams1, _ = s.baGetEstimates()
    assert not np.array_equal(cams1[2:], cams0[2:]) and np.array_equal(cams1[:2], cams0[:2])
    s.baLinearize(False)
    e1 = _pose_err(s, 65)
    assert not np.array_equal(e1, e0)
    assert np.abs(e1 - H.producers(g, cams=cams1, jac=False)).max() < 1e-12
    s.baPop()
    cams2, pts2 = s.baGetEstimates()
    assert np.array_equal(cams2, cams0) and np.array_equal(pts2, pts0)
    s.baLinearize(False)
    assert np.array_equal(_pose_err(s, 65), e0)


def test_binding_rules(golden):
    capi = _capi()
    L = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    n = 65
    g = H.load_graph(golden, n)
    pe = g["pose_edges"]
    vi, vj, m, info = _i32(pe["vi"]), _i32(pe["vj"]), _f64(pe["meas"]), _f64(pe["info"])
    ref = H.producers(g)
    pts_h = np.arange(g["L"], dtype=np.int32)

    def pose(s, k, a=vi, b=vj, mm=m, ii=info):
        return L.g2ohip_ba_set_pose_edges(s.h, k, None if a is None else _ip(a), None if b is None else _ip(b), None if mm is None else _dp(mm),
                                          None if ii is None else _dp(ii))

    def mono(s, k):
        s.baSetEdges(k, g["cam_idx"], g["pt_idx"], g["meas"], None, g["f"], g["cx"], g["cy"])

    def still_works(s, want=ref, count=n):
        s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], pts_h)      # (same tables: only invalidates the evaluation)
        s.baLinearize(True)
        got = _pose_data(s, count)
        assert all(np.abs(a - r).max() < 1e-12 for a, r in zip(got, want))

    def rejected(s, rc, code=ARG):
        """The call was refused with `code`, and the binding it found is untouched: a linearize of it gives the same data."""
        assert rc == code, (rc, code)
        still_works(s)

    s = capi.HipBlockSolver(6, 3, 0)
    k = s.addEdgeSet(2, g["v0"], g["v1"])
    kp = s.addEdgeSet(6, pe["v0"], pe["v1"])
    k3 = s.addEdgeSet(3, pe["v0"], pe["v1"])                             # a pose-pose set of another error dimension
    k0 = s.addEdgeSet(6, np.zeros(0, np.int32), np.zeros(0, np.int32))   # a pose-pose set without edges
    ku = s.addEdgeSet(6, np.array([0, 1], np.int32), None)               # a unary set with error dimension 6
    assert pose(s, kp) == STATE                                          # before buildStructure
    s.buildStructure(g["nP"], g["nL"], True)
    assert pose(s, kp) == STATE                                          # no projection binding yet
    mono(s, k)
    assert pose(s, kp) == 0                                              # before the estimates: validated by baSetEstimates
    s.setEdgeData(k3, np.zeros((n, 18)), np.zeros((n, 18)), np.tile(np.eye(3).reshape(-1), (n, 1)), np.zeros((n, 3)))
    s.setEdgeData(ku, np.zeros((2, 36)), None, np.tile(np.eye(6).reshape(-1), (2, 1)), np.zeros((2, 6)))
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], pts_h)
    still_works(s)
    # every refusal is followed by a linearize of the binding it found, before anything binds again
    rejected(s, pose(s, 9))                                              # no such set
    rejected(s, pose(s, -1))
    rejected(s, pose(s, k))                                              # the projection set itself
    rejected(s, pose(s, k3))                                             # error_dim 3
    rejected(s, pose(s, ku))                                             # unary
    rejected(s, pose(s, kp, a=None))
    rejected(s, pose(s, kp, b=None))
    rejected(s, pose(s, kp, mm=None))
    bad = m.copy()
    bad[7, 3] = np.nan
    rejected(s, pose(s, kp, mm=bad))
    bad = info.copy()
    bad[n - 1, 35] = np.inf
    rejected(s, pose(s, kp, ii=bad))
    bad = vi.copy()
    bad[9] = g["P"]
    rejected(s, pose(s, kp, a=bad))                                      # outside the camera table
    bad = vj.copy()
    bad[0] = -1
    rejected(s, pose(s, kp, b=bad))
    bad = vi.copy()
    bad[20] = 3 if bad[20] != 3 else 4
    rejected(s, pose(s, kp, a=bad))                                      # a camera whose hessian index disagrees with the set
    # (only now a call that binds: another FIXED camera on edge 1, hidx -1 either way -- legal; then the first binding again)
    bad = vj.copy()
    bad[1] = 1
    assert g["cam_hidx"][1] == -1 and pose(s, kp, b=bad) == 0
    assert pose(s, kp) == 0
    still_works(s)
    # a binary set with six rows whose vertex 0 is a 3-dof point (a handle of its own: the generic assembly has no (6, 3) kernels,
    # so such a set is never assembled): refused by its shape, the projection binding evaluates as before
    t = capi.HipBlockSolver(6, 3, 0)
    tk = t.addEdgeSet(2, g["v0"], g["v1"])
    tl = t.addEdgeSet(6, np.array([g["nP"], g["nP"] + 1], np.int32), np.array([0, 1], np.int32))
    t.buildStructure(g["nP"], g["nL"], True)
    mono(t, tk)
    t.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], pts_h)
    two = np.array([2, 3], np.int32)
    assert L.g2ohip_ba_set_pose_edges(t.h, tl, _ip(two), _ip(two), _dp(m[:2].copy()), None) == ARG
    t.baLinearize(True)
    pe2 = S.ba_linearize(g, jac=False)
    e_t = np.empty((g["E"], 2))
    assert L.g2ohip_copy_edge_data(t.h, tk, None, None, _dp(e_t)) == 0 and np.abs(e_t - pe2).max() < 1e-9
    # new tables validate the bound pose set again
    hx = g["cam_hidx"].copy()
    hx[2], hx[3] = hx[3], hx[2]
    rejected(s, L.g2ohip_ba_set_estimates(s.h, g["P"], _dp(_f64(g["cams"])), _ip(_i32(hx)), g["L"], _dp(_f64(g["pts"])), _ip(pts_h)))
    # per-edge kernels: refused at the binding, taken by the bound set
    s.setRobustKernelPerEdge(kp, np.zeros(n, np.int32), np.ones(n))
    still_works(s)
    rejected(s, pose(s, kp), STATE)
    s.setRobustKernelPerEdge(kp, None, None)
    # replacing the binding: other measurements, identity information written on the device
    m2 = m.copy()
    m2[:, 9:12] += 0.25
    assert pose(s, kp, mm=m2, ii=None) == 0
    want2 = X.pose_edges(g["cams"], vi, vj, m2)
    still_works(s, want2)
    assert not np.array_equal(want2[2], ref[2])
    s.buildSystem()
    e = want2[2]
    proj = S.ba_linearize(g, jac=False)
    chi = float((e * e).sum() + (proj * proj).sum())
    assert abs(s.chi2() - chi) <= 1e-12 * chi                            # (identity information)
    # rebinding the projection slot keeps the pose binding
    mono(s, k)
    still_works(s, want2)
    # n = 0: accepted, launches nothing, the system is the projection set's
    assert pose(s, k0, a=np.zeros(1, np.int32), b=np.zeros(1, np.int32), mm=np.zeros(12), ii=None) == 0
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], pts_h)
    s.baLinearize(True)
    assert L.g2ohip_build_system(s.h) == STATE                           # the set that left the slot took its device-written data with it
    s.setEdgeData(kp, np.zeros((n, 36)), np.zeros((n, 36)), np.tile(np.eye(6).reshape(-1), (n, 1)), np.zeros((n, 6)))
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], pts_h)
    s.baLinearize(True)
    s.buildSystem()
    assert abs(s.chi2() - float((proj * proj).sum())) <= 1e-12 * s.chi2()
    assert pose(s, kp) == 0
    still_works(s)
    # growth by update_structure is refused with marginalised points, as for every Schur structure: the binding stays
    assert L.g2ohip_update_structure(s.h, 0, kp, 0, None, None) == capi.ERR_UNSUPPORTED
    still_works(s)
    # the binding goes with clearEdgeSets and comes back
    s.clearEdgeSets()
    assert L.g2ohip_ba_linearize(s.h, 1) == STATE
    k = s.addEdgeSet(2, g["v0"], g["v1"])
    kp = s.addEdgeSet(6, pe["v0"], pe["v1"])
    s.buildStructure(g["nP"], g["nL"], True)
    assert pose(s, kp) == STATE                                          # dropped with the projection binding
    mono(s, k)
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], pts_h)
    s.baLinearize(True)                                                  # the projection set alone: the pose set is not bound ...
    with pytest.raises(capi.G2oHipError):
        _pose_data(s, n)                                                 # ... and has no data
    assert pose(s, kp) == 0
    still_works(s)


def test_fused_path_stays_with_the_pose_set_bound():
    """The pose set touches no landmark, so the fused assembly and back-substitution of the mono projection set stay in use
    with it bound: between linearize and the end of solve neither the stand-alone landmark assembly nor the Hpl assembly is
    launched (kernel slots of g2ohip_kernel_time), exactly as without the pose set, while the pose set's own off-diagonal
    blocks are assembled; with ba_fused = 0 both are launched."""
    g = S.make_ba_odometry(12, 60, loop_every=4)
    plain = {k: v for k, v in g.items() if k != "pose_edges"}
    LM, PL, PP = "assemble_vertex(landmark)", "assemble_offdiag(Hpl)", "assemble_offdiag(Hpp)"

    def slots(prob, fused):
        s, graph = lm.setup_device_ba(prob, options={"ba_fused": fused})
        s.setProfiling(1)
        graph.linearize()
        s.sync()
        s.kernelTimes(reset=True)
        s.buildSystem()
        s.setLambda(10.0, True)
        assert s.solve()
        s.restoreDiagonal()
        s.sync()
        return s.kernelTimes(reset=True)
    with_set, without, generic = slots(g, 1), slots(plain, 1), slots(g, 0)
    print("fused, pose set", sorted(with_set))
    print("fused, no pose set", sorted(without))
    print("generic, pose set", sorted(generic))
    assert LM not in without and PL not in without                       # (what "fused" means here)
    assert LM not in with_set and PL not in with_set
    assert PP in with_set and PP not in without                          # the pose set's blocks between two cameras
    assert LM in generic and PL in generic
    assert "back_substitute" in with_set


def test_empty_pose_set_with_use_graph():
    """n = 0 bound on a handle that replays captured launch sequences: nothing is launched for the set, the run is the one of
    the graph without it, bit for bit."""
    capi = _capi()
    g = H.lm_graph()
    none = np.zeros(0, np.int32)
    s = capi.HipBlockSolver(6, 3, 0)
    s.setOption("use_graph", 1)
    k = s.addEdgeSet(2, g["v0"], g["v1"])
    k0 = s.addEdgeSet(6, none, none)
    s.buildStructure(g["nP"], g["nL"], True)
    s.baSetEdges(k, g["cam_idx"], g["pt_idx"], g["meas"], None, g["f"], g["cx"], g["cy"])
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], np.arange(g["L"], dtype=np.int32))
    one = np.zeros(1, np.int32)                                          # (non-null arrays; none of their entries is read)
    assert s.L.g2ohip_ba_set_pose_edges(s.h, k0, capi._ip(one), capi._ip(one), capi._dp(np.zeros(12)), None) == 0
    a = lm.optimize(lm.DeviceBAGraph(s), s, 4, "lm")
    plain = {kk: v for kk, v in g.items() if kk != "pose_edges"}
    s2, graph2 = lm.setup_device_ba(plain, options={"use_graph": 1})
    b = lm.optimize(graph2, s2, 4, "lm")
    assert a[0] == b[0] == 4 and list(a[3]) == list(b[3]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    ea, eb = s.baGetEstimates(), s2.baGetEstimates()
    assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])


def test_growth_of_a_bound_pose_set_cannot_be_reached():
    """g2ohip_update_structure grows sets of structures WITHOUT landmarks only.  In such a structure no edge set has a 3-dof
    vertex 0 (build_structure takes the vertex dimensions from the vertices' classes; a projection set whose points are all
    fixed has none), so both projection entries refuse it, no projection binding exists and the pose entry returns
    G2OHIP_ERR_STATE: the refusal of a grown pose set in g2ohip_ba_linearize is a guard that no sequence of calls reaches."""
    capi = _capi()
    L = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = S.make_ba_odometry(12, 60, loop_every=4)
    pe = g["pose_edges"]
    s = capi.HipBlockSolver(6, 3, 0)
    k = s.addEdgeSet(2, np.full(g["E"], -1, np.int32), g["v1"])          # motion-only: every point fixed
    ks = s.addEdgeSet(3, np.full(g["E"], -1, np.int32), g["v1"])
    kp = s.addEdgeSet(6, pe["v0"], pe["v1"])
    s.buildStructure(g["nP"], 0, False)
    cv, pv, z = _i32(g["cam_idx"]), _i32(g["pt_idx"]), _f64(g["meas"])
    z3 = _f64(np.concatenate([g["meas"], g["meas"][:, :1]], axis=1))
    assert L.g2ohip_ba_set_edges(s.h, k, _ip(cv), _ip(pv), _dp(z), None, g["f"], g["cx"], g["cy"]) == ARG
    assert L.g2ohip_ba_set_stereo_edges(s.h, ks, _ip(cv), _ip(pv), _dp(z3), None, g["f"], g["cx"], g["cy"], 0.2) == ARG
    assert L.g2ohip_ba_set_pose_edges(s.h, kp, _ip(_i32(pe["vi"])), _ip(_i32(pe["vj"])), _dp(_f64(pe["meas"])), None) == STATE
    # the growth itself is what such a structure allows: the set grows, and no front end is there to refuse it
    assert L.g2ohip_update_structure(s.h, 0, kp, 1, _ip(_i32(pe["v0"][:1])), _ip(_i32(pe["v1"][:1]))) == 0
    assert L.g2ohip_ba_linearize(s.h, 1) == STATE                        # nothing bound
