"""GPU: unary pose priors on the device -- EdgeSE2Prior / EdgeSE2XYPrior / EdgeSE3Prior (with a ParameterSE3Offset) bound as
ONE unary edge set beside the pose-pose set of the pose-graph front end (g2ohip_pg_set_prior_edges), with and without a
landmark set: the producer against the NumPy restatement of tests/prior_helpers.py, the assembled and reduced system and its
solution against the CPU oracle fed the NumPy Jacobians, tails, a free gauge held by priors alone, a prior on a fixed pose,
robust kernels, a whole Levenberg-Marquardt run, error paths."""
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm, synthetic as S
from oracle import oracle as O
from tests import landmark_helpers as LH
from tests import prior_helpers as PH
from tests.helpers import dx_tolerance, relerr

pytestmark = pytest.mark.gpu

TOL_J = 1e-12      # producers: same formulas in fp64 (the bounds of tests/test_gpu_landmark_slam.py)
TOL_B = 1e-11      # right-hand side
TOL_HS = 1e-12     # reduced system
ARG, STATE = -1, -3      # G2OHIP_ERR_ARG, G2OHIP_ERR_STATE
N, L = PH.LM_SIZE        # 70 poses, 40 landmarks; prior_stride = 10: 8 priors, two of them on pose 10

# Relative chi2 gap per LM iteration between two equally valid CPU runs of test_lm_run_matches_oracle's graphs
# (prior_helpers.lm_prior_graph: 70 poses, 40 landmarks, priors="pose", prior_stride=10, perturb=(4.0, 1.0, 5.0), seed=43):
# the oracle's Schur path against the same loop solving the full system without elimination (OracleLandmarkSolver(dense=True)).
# Measured on the CPU, never on the device; recorded in profiles/prior_edges.jsonl.  Both CPU runs take the trials
# 2-D [1 1 1 1 1 1 1 1 1 1], 3-D [1 2 1 1 1 1 1 3 1 1].  (With the generator's default seed 42 and the perturbation (0.5, 0.2,
# 0.5) the runs converge to the last bit within seven iterations and the two CPU runs then disagree on accept / reject, so
# seed 43 and the larger perturbation are used: both runs are still descending at iteration 9.)
#   iteration    0        1        2        3        4        5        6        7        8        9
#   2-D      9.4e-15  1.4e-14  1.7e-14  3.1e-15  1.8e-16  3.6e-16  7.3e-16  3.7e-16  3.7e-16  5.6e-16
#   3-D      4.6e-16  4.6e-15  9.7e-15  1.9e-15  4.1e-14  1.0e-13  2.6e-13  1.2e-12  1.3e-12  2.2e-12
ORACLE_DRIFT = {
    "se2": [9.436e-15, 1.414e-14, 1.672e-14, 3.051e-15, 1.799e-16, 3.649e-16, 7.349e-16, 3.693e-16, 3.706e-16, 5.574e-16],
    "se3": [4.638e-16, 4.626e-15, 9.686e-15, 1.876e-15, 4.066e-14, 9.998e-14, 2.623e-13, 1.211e-12, 1.296e-12, 2.195e-12],
}
ORACLE_TRIALS = {"se2": [1] * 10, "se3": [1, 2, 1, 1, 1, 1, 1, 3, 1, 1]}

CASES = [("se2", "pose"), ("se2", "xy"), ("se3", "pose")]


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _graph(kind, priors, **kw):
    return S.make_landmark_slam(kind, N, L, priors=priors, prior_stride=10, **kw)


def _prior_data(s, g):
    d, dp = PH.PRIOR_DIM[PH.prior_type(g)], LH.dims(g)[0]
    J0, _, err = s.edgeData(s.prior_set, len(g["vq"]), d, dp, 0)
    return J0, err


def _check_system(s, o, tag, schur=True):
    capi = _capi()
    s.buildSystem()
    o.build_system()
    print(tag, "b", relerr(s.b(), o.b()), "chi2", s.chi2(), o.chi2())
    assert relerr(s.b(), o.b()) < TOL_B
    assert abs(s.chi2() - o.chi2()) <= 1e-12 * o.chi2()
    lam = 1e-5 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    assert s.solve() and o.solve()
    if schur:
        tol, cond = dx_tolerance(o)
        fig = dict(Hschur=relerr(s.values(capi.HSCHUR), o.values("Hschur")), dx=relerr(s.x(), o.x()), tol=tol, cond=cond)
        print(tag, "solve", fig)
        assert np.array_equal(s.pattern(capi.HSCHUR)[1], o.pattern("hs")[1])
        assert fig["Hschur"] < TOL_HS
    else:
        fig = dict(Hpp=relerr(s.values(capi.HPP), o.values("Hpp")), dx=relerr(s.x(), o.x()), tol=1e-8)
        print(tag, "solve", fig)
        assert fig["Hpp"] < TOL_HS
        tol = 1e-8
    assert fig["dx"] < tol
    s.restoreDiagonal()
    o.restore_diagonal()


@pytest.mark.parametrize("kind,priors", CASES)
def test_producers_system_and_solution_against_oracle(kind, priors):
    """edgeData of the prior set against the restatement; buildSystem + solve (landmarks marginalised, pose 0 fixed) against
    OracleSolver fed the NumPy Jacobians of all three sets; error-only evaluation; both store forms bit-identical."""
    g = _graph(kind, priors)
    assert len(g["vq"]) == 8 and (g["vq"] == 10).sum() == 2
    s, graph = lm.setup_device_landmark_slam(g)
    graph.linearize()
    o = PH.oracle_prior(g, True)
    _, _, (Q0, eq) = PH.feed_oracle(g, o)
    dQ0, deq = _prior_data(s, g)
    figs = dict(J0=relerr(dQ0, Q0), err=relerr(deq, eq))
    print(kind, priors, "producer", figs)
    assert max(figs.values()) < TOL_J, figs
    k0, k1 = s.landmark_sets
    dp, dl = LH.dims(g)
    assert relerr(s.edgeData(k1, g["M"], dl, dp, dl)[2], LH.landmark_edges(g, jac=False)) < TOL_J    # the other sets as before
    _check_system(s, o, "%s %s" % (kind, priors))
    s.pgLinearize(False)                                             # error-only: leaves J, gives the same errors
    xQ0, xeq = _prior_data(s, g)
    assert np.array_equal(xQ0, dQ0) and relerr(xeq, eq) < TOL_J
    s.setOption("pg_landmark_staged", 0)
    s.pgLinearize(True)
    xQ0, xeq = _prior_data(s, g)
    assert np.array_equal(xQ0, dQ0) and np.array_equal(xeq, deq)


def _pose_only_priors(kind, ptype, count):
    """The odometry of the landmark graph alone plus `count` priors, cycling over the poses (the fixed one included)."""
    g = S.make_landmark_slam(kind, N, L)
    rng = np.random.default_rng(count)
    vq = (np.arange(count) % N).astype(np.int32)
    if kind == "se2":
        zq = g["poses_true"][vq] + rng.normal(size=(count, 3)) * (0.3, 0.3, 0.05)
        zq[:, 2] = S._wrap(zq[:, 2])
        zq = zq if ptype == 7 else zq[:, :2].copy()
        offset = None
    else:
        offset = S._iso_pack(S._exp_so3(np.array([[-0.2, 0.15, 0.1]]))[0], np.array([[-0.3, 0.2, 0.1]]))[0]
        Rx, tx = PH._iso(g["poses_true"][vq])
        Rp, tp = PH._iso(offset)
        zq = S._iso_pack(Rx @ Rp[0] @ S._exp_so3(rng.normal(size=(count, 3)) * 0.05)[0],
                         np.einsum("nij,j->ni", Rx, tp[0]) + tx + 0.3 * rng.normal(size=(count, 3)))
    d = PH.PRIOR_DIM[ptype]
    W = rng.normal(size=(count, d, d))
    omega_q = (W @ W.transpose(0, 2, 1) + d * np.eye(d)).reshape(count, d * d)      # full SPD information matrices
    return g, vq, zq, omega_q, offset


@pytest.mark.parametrize("kind,ptype", [("se2", 7), ("se2", 8), ("se3", 9)])
@pytest.mark.parametrize("count", [1, 257])
def test_tails_on_a_pose_only_graph(kind, ptype, count):
    """No landmarks, no Schur (setup_device_pose_graph(priors=...)): one prior, and 257 = one full workgroup and one lane."""
    g, vq, zq, omega_q, offset = _pose_only_priors(kind, ptype, count)
    p = 3 if kind == "se2" else 6
    s, graph = lm.setup_device_pose_graph(1 if kind == "se2" else 2, g["poses"], g["hidx"], g["nP"], g["vi"], g["vj"], g["Z"],
                                          g["omega"], priors=(ptype, vq, zq, omega_q, offset))
    graph.linearize()
    Q0, eq = PH.prior_edges_of(ptype, g["poses"], vq, zq, offset)
    d = PH.PRIOR_DIM[ptype]
    dQ0, _, deq = s.edgeData(s.prior_set, count, d, p, 0)
    figs = dict(J0=relerr(dQ0, Q0), err=relerr(deq, eq))
    print(kind, ptype, count, "producer", figs)
    assert max(figs.values()) < TOL_J, figs
    o = O.OracleSolver(p, 2 if kind == "se2" else 3, g["nP"], 0, False)
    h = np.asarray(g["hidx"], np.int32)
    q0 = o.add_edge_set(p, h[g["vi"]], h[g["vj"]])
    o.set_dims(q0, p, p)
    q1 = o.add_edge_set(d, h[vq])
    o.set_dims(q1, p, 0)
    o.build_structure()
    A0, A1, e0 = LH.pose_edges(g)
    o.set_edge_data(q0, A0, A1, g["omega"], e0)
    o.set_edge_data(q1, Q0, None, omega_q, eq)
    _check_system(s, o, "%s type %d x %d" % (kind, ptype, count), schur=False)
    s.setOption("pg_landmark_staged", 0)
    s.pgLinearize(True)
    xQ0, _, xeq = s.edgeData(s.prior_set, count, d, p, 0)
    assert np.array_equal(xQ0, dQ0) and np.array_equal(xeq, deq)


@pytest.mark.parametrize("kind", ["se2", "se3"])
def test_free_gauge_held_by_the_priors(kind):
    """gauge="free": no fixed pose, the priors alone make the system definite.  Without them it is not: checked on the
    oracle's dense matrix (the deficient system is never handed to the device)."""
    g = _graph(kind, "pose", gauge="free")
    assert (g["hidx"] >= 0).all() and g["nP"] == N
    s, graph = lm.setup_device_landmark_slam(g)
    graph.linearize()
    o = PH.oracle_prior(g, True)
    _, _, (Q0, eq) = PH.feed_oracle(g, o)
    dQ0, deq = _prior_data(s, g)
    assert max(relerr(dQ0, Q0), relerr(deq, eq)) < TOL_J
    _check_system(s, o, "%s free gauge" % kind)
    dp = LH.dims(g)[0]
    ev = np.linalg.eigvalsh(o.dense_full())
    assert ev[0] > 1e-9 * ev[-1]
    bare = PH.oracle_prior(g, True, with_priors=False)
    A0, A1, e0 = LH.pose_edges(g)
    B0, B1, e1 = LH.landmark_edges(g)
    bare.set_edge_data(0, A0, A1, g["omega"], e0)
    bare.set_edge_data(1, B0, B1, g["omega_l"], e1)
    bare.build_system()
    ev0 = np.linalg.eigvalsh(bare.dense_full())
    print(kind, "smallest / largest eigenvalue with priors", ev[0] / ev[-1], "without", ev0[:dp] / ev0[-1])
    assert (np.abs(ev0[:dp]) < 1e-10 * ev0[-1]).all()                 # the gauge freedom: dim(pose) null directions


@pytest.mark.parametrize("kind", ["se2", "se3"])
def test_prior_on_the_fixed_pose(kind):
    """Prior 0 sits on pose 0, which is fixed (hessian index -1): it adds its own e' Omega e to chi2 and leaves H and b alone."""
    capi = _capi()
    g = _graph(kind, "pose")
    assert g["vq"][0] == 0 and g["hidx"][0] == -1
    g2 = dict(g, vq=g["vq"][1:], zq=g["zq"][1:], omega_q=g["omega_q"][1:])
    out = []
    for pr in (g, g2):
        s, graph = lm.setup_device_landmark_slam(pr)
        graph.linearize()
        s.buildSystem()
        chi = s.chi2()
        s.setLambda(0.0, True)
        assert s.solve()
        out.append((chi, s.b(), s.values(capi.HSCHUR), s.x()))
    o = PH.oracle_prior(g, True)
    _, _, (Q0, eq) = PH.feed_oracle(g, o)
    o.build_system()
    own = float(eq[0] @ g["omega_q"][0].reshape(len(eq[0]), -1) @ eq[0])
    print(kind, "chi2 with / without the prior on the fixed pose", out[0][0], out[1][0], "its own", own)
    assert own > 0 and abs(out[0][0] - o.chi2()) <= 1e-12 * o.chi2()
    assert abs((out[0][0] - out[1][0]) - own) <= 1e-12 * o.chi2()
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


@pytest.mark.parametrize("kind", ["se2", "se3"])
@pytest.mark.parametrize("per_edge", [False, True])
def test_huber_on_the_prior_set(kind, per_edge):
    """Two of the eight priors carry a gross error (a GPS fix gone wrong); Huber on the set, once as the set's kernel and once
    per edge: chi2, b, the reduced system and dx against the oracle with the same kernel."""
    capi = _capi()
    g = _graph(kind, "pose")
    zq = g["zq"].copy()
    col = (0, 1) if kind == "se2" else (9, 10)
    zq[2, col[0]] += 8.0
    zq[5, col[1]] -= 6.0
    g = dict(g, zq=zq)
    delta = 1.0
    s, graph = lm.setup_device_landmark_slam(g)
    if per_edge:
        s.setRobustKernelPerEdge(s.prior_set, np.full(8, capi.KERNEL_HUBER, np.int32), np.full(8, delta))
    else:
        s.setRobustKernel(s.prior_set, capi.KERNEL_HUBER, delta)
    graph.linearize()
    o = PH.oracle_prior(g, True)
    _, _, (Q0, eq) = PH.feed_oracle(g, o, huber=delta)
    d = eq.shape[1]
    w = np.einsum("ni,nij,nj->n", eq, g["omega_q"].reshape(8, d, d), eq)
    assert (w[[2, 5]] > 100 * delta * delta).all()                   # the kernel is active on the gross errors
    _check_system(s, o, "%s huber per_edge=%s" % (kind, per_edge))


def _drift_bound(kind):
    return [max(1e-12, 10.0 * d) for d in ORACLE_DRIFT[kind]]


@pytest.mark.parametrize("kind", ["se2", "se3"])
def test_lm_run_matches_oracle(kind):
    """Ten Levenberg-Marquardt iterations with everything on the device against the same loop over OracleSolver + the NumPy
    producers (prior set included): chi2 of iteration 0 to 1e-12 relative, the same accepted / rejected pattern of trials,
    chi2 of every later iteration within ten times the gap two equally valid CPU runs show at that iteration (floor 1e-12):
    ORACLE_DRIFT above.  The device run with use_graph = 1 gives the bit-identical trajectory."""
    g = PH.lm_prior_graph(kind)
    s, graph = lm.setup_device_landmark_slam(g)
    n_gpu, chi_gpu, lam_gpu, tr_gpu = lm.optimize(graph, s, 10, "lm")
    n_cpu, chi_cpu, lam_cpu, tr_cpu, og = PH.oracle_lm_run(g, 10)
    gaps = [abs(a - b) / b for a, b in zip(chi_gpu, chi_cpu)]
    print(kind, "lm chi2 gpu", chi_gpu)
    print(kind, "lm chi2 cpu", chi_cpu)
    print(kind, "lm gaps", gaps, "bound", _drift_bound(kind), "trials", tr_gpu, tr_cpu)
    assert tr_cpu == ORACLE_TRIALS[kind]
    assert n_gpu == n_cpu == 10 and tr_gpu == tr_cpu
    assert gaps[0] < 1e-12
    for it, (gap, bound) in enumerate(zip(gaps, _drift_bound(kind))):
        assert gap <= bound, (it, gap, bound)
    assert chi_gpu[-1] < 0.5 * chi_gpu[0]
    s2, graph2 = lm.setup_device_landmark_slam(g, options={"use_graph": 1})
    n2, chi2, lam2, tr2 = lm.optimize(graph2, s2, 10, "lm")
    assert n2 == n_gpu and tr2 == tr_gpu
    assert np.array_equal(chi2, chi_gpu) and np.array_equal(lam2, lam_gpu)
    assert np.array_equal(s2.pgGetEstimates(), s.pgGetEstimates())
    assert np.array_equal(s2.pgGetLandmarkEstimates(), s.pgGetLandmarkEstimates())


def test_profile_of_the_oracle_drift_is_recorded():
    """ORACLE_DRIFT / ORACLE_TRIALS are what profiles/prior_edges.jsonl records, for the graph prior_helpers builds."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prior_edges.jsonl")
    rec = {}
    for line in open(path):
        d = json.loads(line)
        if d.get("what") == "oracle_drift":
            rec[d["kind"]] = d
    for kind in ("se2", "se3"):
        r = rec[kind]
        assert np.allclose(r["relative_chi2_gap"], ORACLE_DRIFT[kind], rtol=1e-3, atol=1e-18), kind
        assert r["trials"] == r["trials_dense"] == ORACLE_TRIALS[kind]
        assert (r["n"], r["L"]) == PH.LM_SIZE and tuple(r["perturb"]) == PH.LM_PERTURB and r["seed"] == PH.LM_SEED


def test_error_paths():
    capi = _capi()
    Lb = capi.load()
    from openslam_g2o_amd.capi import _dp, _f64, _i32, _ip
    g = _graph("se2", "pose")
    h, hl = _i32(g["hidx"]), _i32(g["pt_hidx"])
    vi, vj, vp, vl, vq = (_i32(g[k]) for k in ("vi", "vj", "vp", "vl", "vq"))
    Z, om, zl, oml, zq, omq = (_f64(g[k]) for k in ("Z", "omega", "zl", "omega_l", "zq", "omega_q"))
    ident = _f64(PH.IDENTITY)

    def sets(s, p=3, l=2, d=3):
        return s.addEdgeSet(p, h[vi], h[vj]), s.addEdgeSet(l, h[vp], hl[vl]), s.addEdgeSet(d, h[vq], None)

    def set_pr(s, k, typ, a=vq, z=zq, w=omq, off=None):
        return Lb.g2ohip_pg_set_prior_edges(s.h, k, typ, None if a is None else _ip(a), None if z is None else _dp(z),
                                            None if w is None else _dp(w), None if off is None else _dp(off))

    s = capi.HipBlockSolver(3, 2, 0)
    k0, k1, k2 = sets(s)
    assert set_pr(s, k2, 7) == STATE                                 # before g2ohip_build_structure
    s.buildStructure(g["nP"], g["nL"], True)
    assert set_pr(s, k2, 7) == STATE                                 # before g2ohip_pg_set_edges
    s.pgSetEdges(k0, 1, vi, vj, Z, om)
    assert set_pr(s, k2, 7) == 0                                     # (the pose table is not known yet: indices checked later)
    s.pgSetEstimates(g["poses"], h)
    s.pgSetLandmarkEdges(k1, 3, vp, vl, zl, oml)
    s.pgSetLandmarkEstimates(g["points"], hl)
    for typ in (9, 6, 10, 0):
        assert set_pr(s, k2, typ) == ARG                             # EdgeSE3Prior beside EdgeSE2, not a prior type
    assert set_pr(s, k0, 7) == ARG and set_pr(s, k1, 7) == ARG       # bound as the pose-pose / landmark set (and not unary)
    assert set_pr(s, k2, 8, z=_f64(zq[:, :2]), w=_f64(np.tile(np.eye(2).ravel(), (8, 1)))) == ARG   # error dimension 3, not 2
    assert set_pr(s, k2, 7, off=ident) == ARG                        # an offset belongs to type 9
    assert set_pr(s, k2, 7, a=None) == ARG and set_pr(s, k2, 7, z=None) == ARG and set_pr(s, k2, 7, w=None) == ARG
    bad = vq.copy()
    bad[3] = g["n"] + 2
    assert set_pr(s, k2, 7, a=bad) == ARG
    bad[3] = -1
    assert set_pr(s, k2, 7, a=bad) == ARG
    bad[3] = vq[3] + 1                                               # another pose: its hessian index is not the set's
    assert set_pr(s, k2, 7, a=bad) == ARG
    with pytest.raises(ValueError):
        s.pgSetPriorEdges(k2, 7, vq[:-1], zq[:-1], omq[:-1])
    with pytest.raises(ValueError):
        s.pgSetPriorEdges(k2, 7, vq, zq, omq, offset=np.zeros(7))
    assert set_pr(s, k2, 7) == 0
    s.pgLinearize(True)
    s.buildSystem()
    chi0 = s.chi2()
    J0, _, e0 = s.edgeData(k2, 8, 3, 3, 0)
    assert relerr(e0, PH.prior_edges(g, jac=False)) < TOL_J
    # a rejected rebinding commits nothing: the previous binding linearizes to the same numbers
    assert set_pr(s, k2, 7, a=bad, z=_f64(zq + 0.25)) == ARG
    assert set_pr(s, k2, 9, z=_f64(zq + 0.25)) == ARG
    assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
    s.buildSystem()
    J1, _, e1 = s.edgeData(k2, 8, 3, 3, 0)
    assert s.chi2() == chi0 and np.array_equal(J0, J1) and np.array_equal(e0, e1)
    # g2ohip_pg_set_estimates with changed tables validates the prior set too and commits nothing when it fails
    wrong = h.copy()
    wrong[10], wrong[11] = wrong[11], wrong[10]
    assert Lb.g2ohip_pg_set_estimates(s.h, len(wrong), _dp(_f64(g["poses"] + 0.25)), _ip(wrong)) == ARG
    assert Lb.g2ohip_pg_linearize(s.h, 1) == 0
    s.buildSystem()
    assert s.chi2() == chi0
    # a later call replaces the binding
    assert set_pr(s, k2, 7, z=_f64(zq + 0.25)) == 0
    s.pgLinearize(True)
    assert relerr(s.edgeData(k2, 8, 3, 3, 0)[2], PH.se2_prior_edges(g["poses"], vq, zq + 0.25, jac=False)) < TOL_J
    # g2ohip_clear_edge_sets drops the binding
    s.clearEdgeSets()
    assert Lb.g2ohip_pg_linearize(s.h, 1) == STATE
    k0, k1, k2 = sets(s)
    s.buildStructure(g["nP"], g["nL"], True)
    assert set_pr(s, k2, 7) == STATE
    # type 7 beside an SE3 pose set, a non-finite offset
    g3 = _graph("se3", "pose")
    h3, hl3 = _i32(g3["hidx"]), _i32(g3["pt_hidx"])
    s3 = capi.HipBlockSolver(6, 3, 0)
    q0 = s3.addEdgeSet(6, h3[g3["vi"]], h3[g3["vj"]])
    q1 = s3.addEdgeSet(3, h3[g3["vp"]], hl3[g3["vl"]])
    q2 = s3.addEdgeSet(6, h3[g3["vq"]], None)
    s3.buildStructure(g3["nP"], g3["nL"], True)
    s3.pgSetEdges(q0, 2, g3["vi"], g3["vj"], g3["Z"], g3["omega"])
    s3.pgSetEstimates(g3["poses"], h3)
    z3, w3 = _f64(g3["zq"]), _f64(g3["omega_q"])
    assert set_pr(s3, q2, 7, a=_i32(g3["vq"]), z=z3, w=w3) == ARG
    nan = _f64(g3["prior_offset"]).copy()
    nan[10] = np.nan
    assert set_pr(s3, q2, 9, a=_i32(g3["vq"]), z=z3, w=w3, off=nan) == ARG
    assert set_pr(s3, q2, 9, a=_i32(g3["vq"]), z=z3, w=w3, off=_f64(g3["prior_offset"])) == 0
    s3.pgLinearize(True)                                             # the prior slot does not need the landmark slot
    assert relerr(s3.edgeData(q2, 8, 6, 6, 0)[2], PH.prior_edges(g3, jac=False)) < TOL_J
    # growth of the prior set (g2ohip_update_structure, no Schur): refused until it is bound again
    gp, vq1, zq1, omq1, _ = _pose_only_priors("se2", 7, 1)
    sp, graph = lm.setup_device_pose_graph(1, gp["poses"], gp["hidx"], gp["nP"], gp["vi"], gp["vj"], gp["Z"], gp["omega"],
                                           priors=(7, vq1, zq1, omq1, None))
    sp.pgLinearize(True)
    assert sp.updateStructure(0, sp.prior_set, _i32(gp["hidx"])[[5]], None)
    assert Lb.g2ohip_pg_linearize(sp.h, 1) == STATE
    vq2, zq2 = np.array([vq1[0], 5], np.int32), np.concatenate([zq1, gp["poses_true"][[5]]])
    sp.pgSetPriorEdges(sp.prior_set, 7, vq2, zq2, np.concatenate([omq1, omq1]))
    sp.pgLinearize(True)
    assert relerr(sp.edgeData(sp.prior_set, 2, 3, 3, 0)[2], PH.se2_prior_edges(gp["poses"], vq2, zq2, jac=False)) < TOL_J
