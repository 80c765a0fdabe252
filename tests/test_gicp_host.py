"""CPU: the host side of the GICP front end (Edge_V_V_GICP, type 15) -- the fp64 restatement of openslam_g2o_amd/gicp.py
against its 60-digit evaluation (tests/golden/gicp_edges.npz), the analytic Jacobians against central differences through
VertexSE3::oplusImpl, the information builders against their closed forms, the .g2o round trip, the generator's determinism."""
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io, gicp as G, synthetic as S
from oracle import oracle as O
from tests import gicp_helpers as H

Z = np.load(H.GOLDEN)
NAMES = [H.graph_name(n, plpl) for _, plpl in H.MODES for n in H.EDGE_COUNTS]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_60_digits(name):
    """fp64 against mpmath: exactly the recorded drift (the fixture is what the generator gives), which is rounding-sized: a few
    ulp of the largest entry for err and J, cond(M) ~ 1 / epsilon = 100 times that for the plane-to-plane information."""
    g = H.load_graph(Z, name)
    J0, J1, err, om = H.producers(H.FP64, g)
    d = Z[name + "_drift"]
    fig = (np.abs(err - Z[name + "_ref_err"]).max(), max(np.abs(J0 - Z[name + "_ref_J0"]).max(), np.abs(J1 - Z[name + "_ref_J1"]).max()),
           np.abs(om - Z[name + "_ref_omega"]).max())
    print(name, fig, d)
    assert fig[0] <= d[0] and fig[1] <= d[1] and fig[2] <= d[2]
    assert d[0] <= 16 * np.finfo(float).eps * max(1.0, np.abs(Z[name + "_ref_err"]).max())
    assert d[1] <= 16 * np.finfo(float).eps * np.abs(Z[name + "_ref_J0"]).max()
    assert d[2] <= 1e4 * np.finfo(float).eps * np.abs(Z[name + "_ref_omega"]).max()
    if g["gcov"] is None:
        assert d[2] == 0.0 and np.array_equal(om, g["ginfo"])
    else:
        assert np.array_equal(om.reshape(-1, 3, 3), om.reshape(-1, 3, 3).transpose(0, 2, 1))      # symmetric to the bit


def test_fixture_is_what_the_generator_builds():
    for name in ("pp65", "pl300"):
        g, f = H.base_graph(int(name[2:]), name.startswith("pl")), H.load_graph(Z, name)
        for k in H.GRAPH_KEYS:
            assert (g[k] is None and f[k] is None) or np.array_equal(g[k], f[k]), (name, k)
    g = H.base_graph(300, True)
    assert set(zip(g["gi"].tolist(), g["gj"].tolist())) == set(H.PAIRS) and g["hidx"].tolist() == [-1, 0, 1]
    assert len(g["vi"]) == 2


@pytest.mark.parametrize("mode", ["pp", "pl"])
def test_analytic_jacobians_against_central_differences(mode):
    """d e / d u of both vertices through X <- X fromVectorMQT(u) (the oracle's se3_oplus), h = 1e-6: truncation h^2 |e'''| / 6
    ~ 1e-11, rounding eps |e| / h ~ 1e-10."""
    g = H.load_graph(Z, mode + "65")
    J0, J1, err, _ = H.producers(H.FP64, g)
    free = np.arange(len(g["hidx"]), dtype=np.int32)                  # (every pose moves here, the fixed one too)
    h = 1e-6
    worst = 0.0
    for side, J in ((0, J0), (1, J1)):
        v = g["gi"] if side == 0 else g["gj"]
        for c in range(6):
            x = np.zeros(6 * len(free))
            out = []
            for sgn in (1.0, -1.0):
                x[:] = 0.0
                x[c::6] = sgn * h
                moved = O.se3_oplus(g["poses"], free, x)
                e = np.zeros_like(err)
                for k in range(len(v)):
                    X0 = moved[g["gi"][k]] if side == 0 else g["poses"][g["gi"][k]]
                    X1 = moved[g["gj"][k]] if side == 1 else g["poses"][g["gj"][k]]
                    e[k] = G.error(G.FP64, X0, X1, g["gmeas"][k, :3], g["gmeas"][k, 3:])
                out.append(e)
            num = (out[0] - out[1]) / (2 * h)
            same = g["gi"] == g["gj"]
            assert not same.any()
            worst = max(worst, np.abs(num - J[:, 3 * c:3 * c + 3]).max())
    print(mode, "analytic vs central differences", worst)
    assert worst < 5e-9


def test_information_builders_against_closed_forms():
    """prec = e I + (1 - e) n n', cov = I - (1 - e) n n' for a unit normal (R is orthogonal with third row n); make_rot's rows;
    plane_omega against numpy's inverse."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        if abs(n[1]) > 0.95:
            continue
        R = G.make_rot(n)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and np.array_equal(R[2], n)
        assert np.allclose(R[0], np.cross(n, R[1]), atol=1e-15) and abs(R[1] @ n) < 1e-15
        assert np.allclose(G.prec(n, 0.01), 0.01 * np.eye(3) + 0.99 * np.outer(n, n), atol=1e-14)
        assert np.allclose(G.cov(n, 0.001), np.eye(3) - 0.999 * np.outer(n, n), atol=1e-14)
        assert np.array_equal(G.read_information(n), G.prec(n, 0.01))
    g = H.load_graph(Z, "pl65")
    om = H.producers(H.FP64, g, jac=False)[1].reshape(-1, 3, 3)
    for k in range(len(om)):
        A, B = g["poses"][g["gi"][k]][:9].reshape(3, 3).T, g["poses"][g["gj"][k]][:9].reshape(3, 3).T
        R = A.T @ B
        c0, c1 = g["gcov"][k][:9].reshape(3, 3).T, g["gcov"][k][9:].reshape(3, 3).T
        assert np.allclose(om[k], np.linalg.inv(c0 + R @ c1 @ R.T), rtol=0, atol=1e-10)


def test_g2o_round_trip(tmp_path):
    g = S.make_gicp(4, 25, pairs=[(0, 1), (1, 2), (2, 3), (0, 3), (3, 1)], seed=9)
    path = os.path.join(str(tmp_path), "gicp.g2o")
    g2o_io.write_g2o_gicp(path, g)
    rd = g2o_io.read_g2o(path)
    assert rd["kind"] == "se3" and rd["fixed"] == [0]
    p = g2o_io.gicp_problem(rd)
    for k in ("gi", "gj", "gmeas", "normal0", "normal1", "vi", "vj", "hidx"):
        assert np.array_equal(p[k], g[k]), k
    assert p["nP"] == g["nP"] and p["gcov"] is None
    assert np.abs(p["poses"] - g["poses"]).max() < 1e-14 and np.abs(p["Z"] - g["Z"]).max() < 1e-14
    assert np.array_equal(p["omega"], g["omega"])
    assert np.array_equal(p["ginfo"], g["ginfo"])                     # make_gicp's epsilon is Edge_V_V_GICP::read's .01
    q = g2o_io.gicp_problem(rd, plane_to_plane=True)
    assert np.array_equal(q["gcov"], S.make_gicp(4, 25, pairs=[(0, 1), (1, 2), (2, 3), (0, 3), (3, 1)], seed=9, plane_to_plane=True)["gcov"])
    with pytest.raises(ValueError):
        g2o_io.gicp_problem(dict(kind="se2"))


def test_generator_is_deterministic_and_sane():
    a, b = S.make_gicp(3, 30, plane_to_plane=True, seed=4), S.make_gicp(3, 30, plane_to_plane=True, seed=4)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, b[k]), k
    c = S.make_gicp(3, 30, plane_to_plane=True, seed=5)
    assert not np.array_equal(a["gmeas"], c["gmeas"])
    assert a["hidx"].tolist() == [-1, 0, 1] and np.array_equal(a["poses"][0], a["poses_true"][0])
    assert np.allclose(np.linalg.norm(a["normal0"], axis=1), 1.0) and np.abs(a["normal0"][:, 1]).max() < 0.95
    e_true = G.gicp_edges(G.FP64, a["poses_true"], a["gi"], a["gj"], a["gmeas"], jac=False)[0]
    e_init = G.gicp_edges(G.FP64, a["poses"], a["gi"], a["gj"], a["gmeas"], jac=False)[0]
    assert np.abs(e_true).max() < 0.1 < np.abs(e_init).max()           # noise of 0.01 per coordinate against a visible perturbation
    for k in range(len(a["gcov"])):
        for c in (a["gcov"][k][:9], a["gcov"][k][9:]):
            assert np.linalg.eigvalsh(c.reshape(3, 3)).min() > 0.005
    n = S.make_gicp(3, 5, odometry=False)
    assert len(n["vi"]) == 0 and n["Z"].shape == (0, 12) and n["omega"].shape == (0, 36)


def test_lm_fixture_conditions():
    """What the LM comparison of tests/test_gpu_gicp.py rests on, recorded by the generator from two CPU runs (the oracle's
    solver and a dense solve): ten iterations, still descending at the last one, closer to the truth than the initial guess."""
    for mode, _ in H.MODES:
        chis, err = Z["lm_%s_chis" % mode], Z["lm_%s_pose_error" % mode]
        assert len(chis) == H.LM_ITERATIONS == len(Z["lm_%s_trials" % mode]) and (np.diff(chis) < 0).all()
        assert chis[-1] < 0.999 * chis[-2] and err[1] < err[0] and Z["lm_%s_trials" % mode].max() > 1
        assert Z["lm_%s_gap" % mode].max() < 1e-12
