"""CPU: the Sim3 restatement (openslam_g2o_amd/sim3.py through tests/sim3_helpers.py) in fp64 against the same formulas in
mpmath at 60 digits -- exp(log(S)) = S, S S^-1 = identity, the error of EdgeSim3 and its central-difference Jacobian -- over
inputs that take each of the four exp branches and each of the four log branches (the edge with e = 0 exactly included), with
the assertion that both arithmetics took the same branch in EVERY evaluation, perturbed ones included; the file round trip of
VERTEX_SIM3:EXPMAP / EDGE_SIM3:EXPMAP; make_sim3_graph; and the recorded oracle-drift figures of tests/golden/sim3_edges.npz
(generator beside it: tests/golden/make_sim3_edges.py, which also writes them to profiles/sim3_edges.jsonl).

Bounds: an exp . log or mul . inverse chain is a few dozen fp64 operations on values of magnitude <= ~10, so 1e-13 absolute is
two orders above its rounding; the error likewise.  The Jacobian multiplies the rounding of two errors (each a few 1e-16 ..
1e-15) by 1 / (2 delta) = 5e8: 1e-5 is the same two orders above."""
import json
import os

import numpy as np

from openslam_g2o_amd import g2o_io, synthetic as S
from tests import sim3_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_J = 1e-13, 1e-5


def _mpdiff(a, b):
    return max(abs(float(x - y)) for x, y in zip(a, b))


def test_thresholds_are_avoided():
    for v in (H.SMALL_SIGMA, H.BIG_SIGMA):
        assert not 1e-6 <= v <= 1e-4
    for v in (0.8 * H.SMALL_THETA, 1.2 * H.SMALL_THETA, 0.8 * H.BIG_THETA, 1.2 * H.BIG_THETA):
        assert not 1e-3 <= v <= 2e-2


def test_exp_log_inverse_every_branch():
    """exp(log(S)) = S and S S^-1 = identity in both arithmetics, fp64 against mpmath, same branches."""
    rng = np.random.default_rng(3)
    seen_exp, seen_log = set(), set()
    for b in range(4):
        for _ in range(6):
            v = H.branch_vector(b, rng)
            t64, tmp = [], []
            S64, Smp = H.sim3_exp(H.FP64, v, t64), H.sim3_exp(H.MP, v, tmp)
            l64, lmp = H.sim3_log(H.FP64, S64, t64), H.sim3_log(H.MP, Smp, tmp)
            back64, backmp = H.sim3_exp(H.FP64, l64, t64), H.sim3_exp(H.MP, lmp, tmp)
            assert t64 == tmp
            seen_exp.add(dict(t64[:1])["exp"])
            seen_log.add([x for x in t64 if x[0] == "log"][0][1])
            assert _mpdiff(Smp, [H.MP.num(x) for x in S64]) < TOL
            assert _mpdiff(lmp, [H.MP.num(x) for x in l64]) < TOL
            assert _mpdiff(lmp, [H.MP.num(x) for x in v]) < 1e-40                 # log(exp(v)) = v in mpmath itself
            assert max(abs(x - y) for x, y in zip(back64, S64)) < TOL             # exp(log(S)) = S
            assert _mpdiff(backmp, Smp) < 1e-40
            # S S^-1 = identity up to |q|^2 - 1: the reference's small-angle branch takes R = I + Omega + Omega^2, which is a
            # rotation only to O(theta^2) (theta <= 4.8e-7 here: 2.3e-13), and nothing normalises the quaternion made from it
            u64 = H.sim3_mul(H.FP64, S64, H.sim3_inverse(H.FP64, S64))
            ump = H.sim3_mul(H.MP, Smp, H.sim3_inverse(H.MP, Smp))
            assert max(abs(x - y) for x, y in zip(u64, H.IDENTITY)) < 1e-12
            assert _mpdiff(ump, [H.MP.num(x) for x in H.IDENTITY]) < 1e-12
            assert _mpdiff(ump, [H.MP.num(x) for x in u64]) < TOL
    assert seen_exp == seen_log == {0, 1, 2, 3}


def test_error_and_jacobian_every_branch_class():
    """The branch-class graph: every log branch of the error with a fixed vertex on either side, e = 0 exactly; fp64 against
    mpmath with identical traces (exp / log branches, quaternion cases, LU pivots of all 29 evaluations per edge)."""
    g = H.branch_class_graph()
    t64, tmp = [], []
    J0, J1, e = H.edges(H.FP64, g["est"], g["vi"], g["vj"], g["meas"], g["hidx"], trace=t64)
    M0, M1, me = H.edges(H.MP, g["est"], g["vi"], g["vj"], g["meas"], g["hidx"], trace=tmp)
    assert t64 == tmp and len(t64) > 0
    assert {x[1] for x in t64 if x[0] == "log"} == {0, 1, 2, 3}
    assert not e[-1].any() and not me[-1].any()                                  # the measurement equals the relative pose
    figs = dict(err=np.abs(e - me).max(), J=max(np.abs(J0 - M0).max(), np.abs(J1 - M1).max()))
    print(figs)
    assert figs["err"] < TOL and figs["J"] < TOL_J
    assert not J0[0].any() and not J1[1].any() and J1[0].any() and J0[1].any()   # blocks of the fixed vertex
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sim3_edges.npz"))
    assert np.array_equal(gold["branch_err"], me) and np.array_equal(gold["branch_J0"], M0) and np.array_equal(gold["branch_J1"], M1)
    assert np.array_equal(gold["branch_meas"], g["meas"]) and np.array_equal(gold["branch_est"], g["est"])
    # the recorded drift is this run's figure up to the platform's libm (sin, cos, exp, log, acos are not correctly rounded
    # everywhere): the same order of magnitude, not the same bits
    assert 0.25 * gold["branch_drift"][1] <= figs["J"] <= 4 * gold["branch_drift"][1]
    Jf0, Jf1 = H.edges(H.FP64, g["est"], g["vi"], g["vj"], g["meas"], g["hidx"], fix_scale=True)[:2]
    assert not Jf0[:, 42:].any() and not Jf1[:, 42:].any()                       # _fix_scale: column 6 exactly zero
    assert np.array_equal(Jf0[:, :42], J0[:, :42])


def test_recorded_figures():
    """profiles/sim3_edges.jsonl carries the drift of every golden graph, and the figures in the .npz are the same ones."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sim3_edges.npz"))
    lines = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "sim3_edges.jsonl")) if l.strip()]
    drift = {l["graph"].split()[0]: l for l in lines if l.get("kind") == "oracle_drift" and "J" in l}
    for name in ("branch", "n1", "n18", "n19", "n257", "n300"):
        assert drift[name]["err"] == gold[name + "_drift"][0] and drift[name]["J"] == gold[name + "_drift"][1]
        assert 0 < gold[name + "_drift"][0] < TOL and 0 < gold[name + "_drift"][1] < TOL_J
    runs = {l["graph"]: l for l in lines if l.get("kind") == "oracle_drift" and "chi2_mp" in l}
    for tag in ("plain", "huber"):
        r = runs["lm " + tag]
        assert np.array_equal(r["chi2_rel_fp64_vs_mp"], gold["lm_%s_rel" % tag])
        assert r["chi2_mp"][-1] < r["chi2_initial"] and r["dx_first_solve_rel"] == gold["lm_%s_dx_drift" % tag][0]


def test_file_round_trip(tmp_path):
    """write -> read reproduces estimates, measurements (as transformations: both directions invert and pass through log /
    exp), information (exactly) and the four vertex extras (exactly)."""
    g = S.make_sim3_graph(12, 4, 0.02, 5)
    extras = np.arange(48, dtype=np.float64).reshape(12, 4) + 0.5
    path = str(tmp_path / "sim3.g2o")
    g2o_io.write_g2o_sim3(path, g["est"], g["vi"], g["vj"], g["meas"], g["info"], extras=extras, fixed=[0])
    rd = g2o_io.read_g2o(path)
    assert rd["kind"] == "sim3" and rd["fixed"] == [0]
    assert np.array_equal(rd["vi"], g["vi"]) and np.array_equal(rd["vj"], g["vj"])
    assert np.array_equal(rd["info"].reshape(-1, 49), g["info"]) and np.array_equal(rd["sim3_extras"], extras)
    for a, b in list(zip(rd["estimates"], g["est"])) + list(zip(rd["meas"], g["meas"])):
        (Ra, ta, sa), (Rb, tb, sb) = H.transform(a), H.transform(b)
        assert np.abs(Ra - Rb).max() < 1e-12 and np.abs(ta - tb).max() < 1e-12 * max(1.0, np.abs(tb).max()) and abs(sa - sb) < 1e-12
    hidx, num_free = g2o_io.hessian_index(len(rd["ids"]), rd["fixed"])
    assert num_free == 11 and np.array_equal(hidx, g["hidx"])


def test_make_sim3_graph():
    """Deterministic from the seed; s = 1 in the ground truth; chi2 = 0 there without noise; the initial estimate carries the
    scale drift (none with fix_scale); vertex 0 fixed."""
    a, b = S.make_sim3_graph(40, 10, 0.01, 7), S.make_sim3_graph(40, 10, 0.01, 7)
    for k in a:
        assert np.array_equal(a[k], b[k])
    c = S.make_sim3_graph(40, 10, 0.01, 8)
    assert not np.array_equal(a["meas"], c["meas"])
    assert (a["est_true"][:, 7] == 1.0).all() and a["hidx"][0] == -1 and (a["hidx"][1:] == np.arange(39)).all()
    assert len(a["vi"]) == 39 + 1 + 2 and a["est"][:, 7].max() > 1.4
    g0 = S.make_sim3_graph(40, 10, 0.01, 7, noise=0.0)
    e = H.edges(H.FP64, g0["est_true"], g0["vi"], g0["vj"], g0["meas"], jac=False)
    assert H.chi2(e, g0["info"]) < 1e-22                  # 42 edges x 7 entries of ~1e-15, squared, times information <= 1e4
    e = H.edges(H.FP64, a["est"], a["vi"], a["vj"], a["meas"], jac=False)
    assert H.chi2(e, a["info"]) > 1e3
    f = S.make_sim3_graph(40, 10, 0.01, 7, fix_scale=True)
    assert f["fix_scale"] and np.abs(f["est"][:, 7] - 1).max() < 0.2 and not a["fix_scale"]
