"""GPU: device-resident Sim3 bundle adjustment -- EdgeSim3ProjectXYZ over VertexSim3Expmap / VertexSBAPointXYZ bound as landmark
type 11 (g2ohip_pg_set_sim3_project_edges) beside a type-10 pose set.

Every bound is 8 x a figure of tests/golden/sim3_project_edges.npz (generator: tests/golden/make_sim3_project_edges.py, lines
"oracle_drift" of profiles/sim3_project.jsonl): the distance of the fp64 restatement (openslam_g2o_amd/sim3.py) from the same
formulas in mpmath at 60 digits, for the same graph -- the oracle's own error, never the device's.  The Jacobian of this edge is
DEFINED as a central difference with delta = 1e-9 (the reference has no analytic one), so 1 / (2 delta) = 5e8 multiplies every
rounding of the error.

Lane mapping: the error kernel runs one lane per edge, the Jacobian kernel 10 lanes per edge (edge, column), 256 threads per
block.  Edge counts: 1; 7 (the seventh edge's lanes 60-69 straddle a wave boundary); 25 (250 lanes: inside one block); 26 (the
block boundary falls inside an edge); 257 (one past a block of the error kernel); 300 (partial last blocks of both kernels).

The whole-run comparison: an mpmath-fed run is too slow for a GPU test, so the fp64-fed and the mpmath-fed run are recorded by the
generator over the CPU oracle solver (same lm.optimize loop, same producers, solver of the same system); the GPU test runs the
device-resident graph and the fp64-fed graph over the device solver and bounds their difference by 8 x the recorded one."""
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm, synthetic as S
from tests import sim3_project_helpers as H

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "sim3_project_edges.npz"))
GRAPH_KEYS = ("est", "points", "hidx", "pt_hidx", "vp", "vl", "zl", "omega_l", "intrinsics", "J0", "J1", "err", "drift")


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _gold_graph(n):
    g = {k: GOLD["n%d_%s" % (n, k)] for k in GRAPH_KEYS}
    g["nP"] = int(g["hidx"].max()) + 1
    g["nL"] = int((g["pt_hidx"] >= 0).sum())
    g.update(vi=np.zeros(0, np.int32), vj=np.zeros(0, np.int32), meas=np.zeros((0, 8)), info=np.zeros((0, 49)))
    return g


def _data(s, g):
    return s.edgeData(s.landmark_sets[1], len(g["vp"]), 2, 7, 3)


def _figs(J0, J1, err, g):
    return dict(err=np.abs(err - g["err"]).max(), J=max(np.abs(J0 - g["J0"]).max(), np.abs(J1 - g["J1"]).max()))


@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_producers_against_mpmath(n):
    """err, J0, J1 of g2ohip_copy_edge_data against mpmath: 8 x the fp64 restatement's drift on the same graph.  Few poses and
    points shared by many edges; pose 0 and point 0 are fixed (their blocks are exactly zero), edges 2 and 3 observe the same
    pair, every camera has intrinsics of its own.  The EdgeSim3 set beside the observations is empty."""
    g = _gold_graph(n)
    s, graph = lm.setup_device_sim3_ba(g)
    graph.linearize()
    J0, J1, err = _data(s, g)
    s.pgSetEstimates(g["est"], g["hidx"])                           # (same values: the next evaluation is a fresh one)
    graph.compute_active_errors()                                   # error-only: same errors, the Jacobians stay
    xJ0, xJ1, err_only = _data(s, g)
    figs = _figs(J0, J1, err, g)
    print(n, "device vs mpmath", figs, "fp64 restatement vs mpmath", g["drift"])
    assert np.array_equal(xJ0, J0) and np.array_equal(xJ1, J1)
    assert np.array_equal(err_only, err)
    assert figs["err"] <= 8 * g["drift"][0], figs
    assert figs["J"] <= 8 * g["drift"][1], figs
    fixed0, fixed1 = g["hidx"][g["vp"]] < 0, g["pt_hidx"][g["vl"]] < 0
    if n > 1:
        assert fixed0.any() and fixed1.any() and (g["vp"][2], g["vl"][2]) == (g["vp"][3], g["vl"][3])
        assert len(np.unique(g["intrinsics"], axis=0)) == len(g["intrinsics"])
    assert not J0[fixed0].any() and not J1[fixed1].any()
    assert (np.abs(J0[~fixed0]).max(axis=1) > 0).all() and (np.abs(J1[~fixed1]).max(axis=1) > 0).all()


def test_fix_scale():
    """_fix_scale: column 6 of every J0 block exactly 0.0 and pg_update leaves every s bit-identical; switched off, column 6 is
    non-zero and within bound and s moves.  (A step in sigma scales S.map(X) as a whole and the projection does not see it: the
    non-zero column is the rounding of the two errors times 1 / (2 delta), in mpmath ~1e-50 -- the bound holds it to the fp64
    restatement's own noise.)"""
    g = _gold_graph(25)
    free = g["hidx"][g["vp"]] >= 0
    x = GOLD["update_x"]
    s, graph = lm.setup_device_sim3_ba(dict(g, fix_scale=True))
    graph.linearize()
    J0, J1, _ = _data(s, g)
    assert not J0[:, 12:].any()
    assert (np.abs(J0[free, :12]).max(axis=1) > 0).all()
    assert np.abs(J0[:, :12] - g["J0"][:, :12]).max() <= 8 * g["drift"][1]      # (columns 0-5 do not see the flag)
    s.setX(x)
    s.pgUpdate()
    moved = s.pgGetEstimates()
    assert np.array_equal(moved[:, 7], g["est"][:, 7])
    assert not np.array_equal(moved[1:, :7], g["est"][1:, :7])
    s.pgSetEstimates(g["est"], g["hidx"])
    s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
    s.pgSetSim3FixScale(False)
    graph.linearize()                                               # (the flag alone invalidates the landmark Jacobians)
    J0, J1, err = _data(s, g)
    assert np.abs(J0[free, 12:]).max() > 0
    figs = _figs(J0, J1, err, g)
    assert figs["J"] <= 8 * g["drift"][1], figs
    s.setX(x)
    s.pgUpdate()
    assert (s.pgGetEstimates()[1:, 7] != g["est"][1:, 7]).all()


def test_fix_scale_flag_alone_invalidates_jacobians():
    """pg_set_sim3_fix_scale between two linearizations, nothing else touched: the second one re-evaluates J0."""
    g = _gold_graph(26)
    s, graph = lm.setup_device_sim3_ba(g)
    graph.linearize()
    a = _data(s, g)[0]
    s.pgSetSim3FixScale(True)
    graph.linearize()
    b = _data(s, g)[0]
    assert np.abs(a[:, 12:]).max() > 0 and not b[:, 12:].any() and np.array_equal(a[:, :12], b[:, :12])


def test_update_and_stack():
    """pg_update with a recorded step: poses against mpmath oplus as transformations (R, t, s), points exactly points + their
    slices of x; push / update / pop restores both tables bit for bit, discard_top keeps the update, fixed vertices untouched."""
    g = _gold_graph(25)
    s, graph = lm.setup_device_sim3_ba(g)
    s.setX(GOLD["update_x"])
    graph.push()
    graph.update()
    up, upl = s.pgGetEstimates(), s.pgGetLandmarkEstimates()
    d = 0.0
    for a, b in zip(up, GOLD["update_est"]):
        (Ra, ta, sa), (Rb, tb, sb) = H.transform(a), H.transform(b)
        d = max(d, np.abs(Ra - Rb).max(), np.abs(ta - tb).max(), abs(sa - sb))
    print("update: device vs mpmath", d, "fp64 restatement vs mpmath", GOLD["update_drift"][0])
    assert d <= 8 * GOLD["update_drift"][0]
    assert np.array_equal(upl, GOLD["update_points"])
    assert np.array_equal(up[0], g["est"][0]) and (up[1:] != g["est"][1:]).any(axis=1).all()
    assert np.array_equal(upl[0], g["points"][0]) and (upl[1:] != g["points"][1:]).all()
    graph.pop()
    assert np.array_equal(s.pgGetEstimates(), g["est"]) and np.array_equal(s.pgGetLandmarkEstimates(), g["points"])
    graph.push()
    graph.update()
    graph.discard_top()
    assert np.array_equal(s.pgGetEstimates(), up) and np.array_equal(s.pgGetLandmarkEstimates(), upl)
    with pytest.raises(_capi().G2oHipError):
        graph.pop()


def _fed_run(g, huber):
    """lm.optimize over the device solver with the estimates on the host and the fp64 restatement feeding set_edge_data."""
    capi = _capi()
    s = capi.HipBlockSolver(7, 3, 0)
    ks = [None, None]
    if len(g["vi"]):
        ks[0] = s.addEdgeSet(7, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
    ks[1] = s.addEdgeSet(2, g["hidx"][g["vp"]], g["pt_hidx"][g["vl"]])
    s.buildStructure(g["nP"], g["nL"], True)
    if huber:
        s.setRobustKernel(ks[1], capi.KERNEL_HUBER, huber)
    feed = lambda w, J0, J1, err: s.setEdgeData(ks[w], J0, J1, g["omega_l"] if w else g["info"], err)
    graph = H.HostSim3BAGraph(H.FP64, g, feed, s.x, s.chi2)
    done, chis, _, trials = lm.optimize(graph, s, H.ITERATIONS, "lm")
    return done, np.array(chis), trials, graph.est, graph.points


@pytest.mark.parametrize("tag,sim3_edges,huber", H.RUNS)
def test_lm_run(tag, sim3_edges, huber):
    """make_sim3_ba(12 cameras, 60 points, 4 observations per point), five LM iterations with Schur on, device-resident against
    the same library fed by the fp64 restatement every trial: final poses and points within 8 x the recorded fp64-fed /
    mpmath-fed difference; chi2 decreases and ends below its recorded start."""
    g = S.make_sim3_ba(sim3_edges=sim3_edges, **H.BA_ARGS)
    s, graph = lm.setup_device_sim3_ba(g, huber_delta=huber)
    graph.compute_active_errors()
    chi0 = graph.chi2()
    done, chis, _, trials = lm.optimize(graph, s, H.ITERATIONS, "lm")
    est, pts = s.pgGetEstimates(), s.pgGetLandmarkEstimates()
    fdone, fchis, ftrials, fest, fpts = _fed_run(g, huber)
    dest, dpts = np.abs(est - fest).max(), np.abs(pts - fpts).max()
    rec = (GOLD["lm_%s_est_drift" % tag][0], GOLD["lm_%s_points_drift" % tag][0])
    print(tag, "chi2", chi0, "->", chis, "trials", trials, "fed", ftrials, "recorded", list(GOLD["lm_%s_trials" % tag]),
          "\n rel chi2 device vs fed", np.abs(np.array(chis) - fchis) / np.abs(fchis), "recorded fp64 vs mpmath", GOLD["lm_%s_rel" % tag],
          "\n poses", dest, "recorded", rec[0], "points", dpts, "recorded", rec[1])
    assert done == fdone == H.ITERATIONS
    assert dest <= 8 * rec[0], (dest, rec[0])
    assert dpts <= 8 * rec[1], (dpts, rec[1])
    assert abs(chi0 - GOLD["lm_%s_chi0" % tag][0]) <= 1e-9 * chi0
    assert (np.diff([chi0] + list(chis)) <= 0).all() and chis[-1] < GOLD["lm_%s_chi0" % tag][0]
    assert np.array_equal(est[:2], g["est"][:2])                    # the two fixed cameras


def test_refusals():
    """Every refused call returns G2OHIP_ERR_ARG and the bound graph still linearizes to the same bits; pg_linearize before the
    landmark estimates is G2OHIP_ERR_STATE."""
    capi = _capi()
    Lb = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = _gold_graph(26)
    h, ph = _i32(g["hidx"]), _i32(g["pt_hidx"])
    vp, vl, z, w, kc = _i32(g["vp"]), _i32(g["vl"]), _f64(g["zl"]), _f64(g["omega_l"]), _f64(g["intrinsics"])
    n, nv = len(vp), len(h)
    none_i, none_d = _i32(np.zeros(0)), _f64(np.zeros(0))

    def bind(s, k, pv=vp, lv=vl, cams=kc):
        return Lb.g2ohip_pg_set_sim3_project_edges(s.h, k, _ip(pv), _ip(lv), _dp(z), _dp(w), len(cams), _dp(cams))

    s = capi.HipBlockSolver(7, 3, 0)
    k0 = s.addEdgeSet(7, none_i, none_i)
    k1 = s.addEdgeSet(2, h[vp], ph[vl])
    k3 = s.addEdgeSet(3, h[vp], ph[vl])                              # error_dim 3: not an EdgeSim3ProjectXYZ set
    kq = s.addEdgeSet(7, h[vp], None)
    s.buildStructure(g["nP"], g["nL"], True)
    s.landmark_sets = (k0, k1)
    assert Lb.g2ohip_pg_set_sim3_project_edges(s.h, k1, _ip(vp), _ip(vl), _dp(z), _dp(w), nv, _dp(kc)) == STATE    # no pose set yet
    assert Lb.g2ohip_pg_set_edges(s.h, k0, 10, None, None, None, None) == 0                                       # zero edges
    s._pg = (10, 8)
    s.pgSetEstimates(g["est"], h)
    assert bind(s, k1) == 0
    assert Lb.g2ohip_pg_linearize(s.h, 1) == STATE                  # no landmark estimates yet
    s.pgSetLandmarkEstimates(g["points"], ph)
    s.pgLinearize(True)
    ref = _data(s, g)

    def still_bound():
        s.pgSetEstimates(g["est"], h)                               # (same table: forces a fresh evaluation)
        s.pgLinearize(True)
        return all(np.array_equal(a, b) for a, b in zip(_data(s, g), ref))

    assert still_bound()
    z3, w3 = _f64(np.zeros((n, 3))), _f64(np.tile(np.eye(3).ravel(), (n, 1)))
    w2 = _f64(np.tile(np.eye(2).ravel(), (n, 1)))
    ident = _f64(np.tile([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], (n, 1)))
    w7 = _f64(np.tile(np.eye(7).ravel(), (n, 1)))
    kcam = _f64([500.0, 500.0, 320.0, 240.0])
    # types 3-6 and priors beside type 10
    assert Lb.g2ohip_pg_set_landmark_edges(s.h, k1, 3, _ip(vp), _ip(vl), _dp(z), _dp(w2), None) == ARG and still_bound()
    assert Lb.g2ohip_pg_set_landmark_edges(s.h, k3, 4, _ip(vp), _ip(vl), _dp(z3), _dp(w3), None) == ARG and still_bound()
    for typ in (5, 6):
        assert Lb.g2ohip_pg_set_landmark_camera_edges(s.h, k3, typ, _ip(vp), _ip(vl), _dp(z3), _dp(w3), None, _dp(kcam)) == ARG
        assert still_bound()
    assert Lb.g2ohip_pg_set_landmark_edges(s.h, k1, 11, _ip(vp), _ip(vl), _dp(z), _dp(w2), None) == ARG and still_bound()
    for typ in (7, 8, 9):
        assert Lb.g2ohip_pg_set_prior_edges(s.h, kq, typ, _ip(vp), _dp(ident), _dp(w7), None) == ARG and still_bound()
    # the pose set cannot turn into types 1 / 2 under a type-11 set
    for typ in (1, 2):
        assert Lb.g2ohip_pg_set_edges(s.h, k0, typ, _ip(none_i), _ip(none_i), _dp(none_d), _dp(none_d)) == ARG and still_bound()
    assert bind(s, k3) == ARG and still_bound()                     # wrong set dimensions
    assert bind(s, k0) == ARG and still_bound()                     # the set already bound as the pose-pose set
    assert bind(s, k1, cams=kc[:-1]) == ARG and still_bound()       # n_cams differs from the pose table
    assert bind(s, k1, cams=_f64(np.vstack([kc, kc[:1]]))) == ARG and still_bound()
    bad = kc.copy()
    bad[3, 0] = 0.0
    assert bind(s, k1, cams=bad) == ARG and still_bound()           # fx = 0
    bad = kc.copy()
    bad[2, 1] = 0.0
    assert bind(s, k1, cams=bad) == ARG and still_bound()           # fy = 0
    for v in (np.nan, np.inf):
        bad = kc.copy()
        bad[nv - 1, 3] = v
        assert bind(s, k1, cams=bad) == ARG and still_bound()       # non-finite intrinsics
    bad = vp.copy()
    bad[n - 1] = nv
    assert bind(s, k1, pv=bad) == ARG and still_bound()             # pose index out of range
    bad = vl.copy()
    bad[5] = len(ph)
    assert bind(s, k1, lv=bad) == ARG and still_bound()             # point index out of range
    bad = vp.copy()
    bad[0] = -1
    assert bind(s, k1, pv=bad) == ARG and still_bound()
    bad = vp.copy()
    bad[4] = (vp[4] + 1) % nv                                       # a hessian index that differs from the set's
    assert h[bad[4]] != h[vp[4]]
    assert bind(s, k1, pv=bad) == ARG and still_bound()
    bad = vl.copy()
    bad[4] = (vl[4] + 1) % len(ph)
    assert bind(s, k1, lv=bad) == ARG and still_bound()
    assert Lb.g2ohip_pg_set_estimates(s.h, nv - 1, _dp(_f64(g["est"][:-1])), _ip(h[:-1])) == ARG and still_bound()   # table != n_cams
    # re-binding in either order keeps the pair
    assert Lb.g2ohip_pg_set_edges(s.h, k0, 10, None, None, None, None) == 0 and still_bound()
    assert bind(s, k1) == 0 and still_bound()

    for p, typ, stride in ((3, 1, 3), (6, 2, 12)):                  # type 11 beside a type-1 / type-2 pose set, handles not (7, 3)
        s2 = capi.HipBlockSolver(p, 3 if p == 6 else 2, 0)
        ka = s2.addEdgeSet(p, h[vp], (h[vp] + 1) % g["nP"])
        kb = s2.addEdgeSet(2, h[vp], ph[vl])
        s2.buildStructure(g["nP"], g["nL"], True)
        vj = _i32((vp + 1) % nv)
        assert Lb.g2ohip_pg_set_edges(s2.h, ka, typ, _ip(vp), _ip(vj), _dp(_f64(np.zeros((n, stride)))),
                                      _dp(_f64(np.tile(np.eye(p).ravel(), (n, 1))))) == 0
        assert bind(s2, kb) == ARG
    s73 = capi.HipBlockSolver(7, 2, 0)                              # a handle that is not (7, 3)
    ka = s73.addEdgeSet(7, none_i, none_i)
    kb = s73.addEdgeSet(2, h[vp], ph[vl])
    s73.buildStructure(g["nP"], g["nL"], True)
    assert Lb.g2ohip_pg_set_edges(s73.h, ka, 10, None, None, None, None) == 0
    assert bind(s73, kb) == ARG
