"""CPU: the host side of the BA front end's pose-pose slot (EdgeSE3Expmap) -- openslam_g2o_amd/se3expmap.py against the
60-digit reference of tests/se3expmap_helpers.py and against central differences, the fixture, the `.g2o` reader / writer,
synthetic.make_ba_odometry, the interface."""
import os

import numpy as np

from openslam_g2o_amd import g2o_io, se3expmap as X, synthetic as S
from tests import se3expmap_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_against_mpmath_and_the_fixture():
    """fp64 against 60 digits on the first 65 edges (every special edge is among them): a few ulp of the largest entry; and the
    fixture holds what the generator computes today."""
    z = np.load(H.GOLDEN)
    g = H.base_graph(65)
    pe = g["pose_edges"]
    assert np.array_equal(z["cams"], g["cams"]) and np.array_equal(z["meas"][:65], pe["meas"]) and np.array_equal(z["vi"][:65], pe["vi"])
    M0, M1, me, d = H.mp_pose_edges(g["cams"], pe["vi"], pe["vj"], pe["meas"])
    assert np.array_equal(M0, z["ref_J0"][:65]) and np.array_equal(M1, z["ref_J1"][:65]) and np.array_equal(me, z["ref_err"][:65])
    F0, F1, fe = H.producers(g)
    fig = np.array([np.abs(fe - me).max(), max(np.abs(F0 - M0).max(), np.abs(F1 - M1).max())])
    print("drift", fig, "recorded", z["drift_65"])
    assert np.array_equal(fig, z["drift_65"])
    assert fig[0] < 32 * np.finfo(float).eps * np.abs(me).max() and fig[1] < 32 * np.finfo(float).eps * max(np.abs(M0).max(), np.abs(M1).max())
    assert np.all(np.abs(d - 0.99999) > 1e-9) and (d > 0.99999).sum() >= 2 and not np.any(fe[5])
    assert np.all(np.abs(F0).max(axis=1) > 0) and np.all(np.abs(F1).max(axis=1) > 0)
    # the error-only evaluation is the same arithmetic
    assert np.array_equal(H.producers(g, jac=False), fe)
    # the recorded step: oplus against 60 digits
    h = g["cam_hidx"]
    upd = np.zeros((g["P"], 6))
    upd[h >= 0] = z["step_x"].reshape(-1, 6)[h[h >= 0]]
    moved = X.oplus(g["cams"], upd)
    assert np.abs(moved - z["step_cams"]).max() == z["step_oplus_drift"][0] < 1e-14
    assert np.abs(moved - S._apply_cam_update(g["cams"], upd)).max() < 1e-14      # (and the update the project's generator uses)


def test_jacobians_are_the_derivative_at_zero_error():
    """On edges with zero error J0 / J1 equal central differences of the error through exp(delta) T (h = 1e-5: truncation about
    1e-10, rounding about 1e-11 on entries of order <= 10; bound 1e-7).  Pins the vertex order and the sign of J1."""
    rng = np.random.default_rng(5)
    n = 6
    Ti = X.exp(np.concatenate([rng.normal(size=(n, 3)) * 0.7, rng.normal(size=(n, 3)) * 2.0], axis=1))
    Tj = X.exp(np.concatenate([rng.normal(size=(n, 3)) * 0.7, rng.normal(size=(n, 3)) * 2.0], axis=1))
    C = X.relative_measurement(Ti, Tj)
    assert np.abs(X.error(Ti, Tj, C)).max() < 1e-14
    J0, J1 = X.jacobians(Ti, Tj, C)
    h = 1e-5
    for side, J in ((0, J0), (1, J1)):
        for c in range(6):
            u = np.zeros((n, 6))
            u[:, c] = h
            if side == 0:
                ep, em = X.error(X.oplus(Ti, u), Tj, C), X.error(X.oplus(Ti, -u), Tj, C)
            else:
                ep, em = X.error(Ti, X.oplus(Tj, u), C), X.error(Ti, X.oplus(Tj, -u), C)
            num = (ep - em) / (2 * h)
            got = J.reshape(n, 6, 6)[:, c, :]            # column c of the column-major blocks
            assert np.abs(got).max() <= 10.0
            assert np.abs(num - got).max() < 1e-7, (side, c, np.abs(num - got).max())
    assert np.abs(J0 + J1).max() > 0.1                   # (the two are not each other's negative: swapping them would show)


def test_g2o_round_trip(tmp_path):
    """A problem with pose edges keeps its measurement, information and linearised system through the file; a file without the
    tag reads exactly as before."""
    for kw in ({}, {"stereo_baseline": 0.2}):
        g = S.make_ba_odometry(10, 40, loop_every=3, **kw)
        pe = g["pose_edges"]
        pe["info"] = H._spd6(np.random.default_rng(1), pe["n"])
        path = str(tmp_path / "pose.g2o")
        g2o_io.write_g2o_ba(path, g)
        r = g2o_io.read_g2o_ba(path)
        rp = r["pose_edges"]
        assert np.array_equal(rp["vi"], pe["vi"]) and np.array_equal(rp["vj"], pe["vj"])
        assert np.array_equal(rp["v0"], pe["v0"]) and np.array_equal(rp["v1"], pe["v1"])
        assert np.abs(rp["meas"] - pe["meas"]).max() < 1e-14 * max(1.0, np.abs(pe["meas"]).max())
        assert np.array_equal(rp["info"], pe["info"])
        a, b = H.producers(g), H.producers(r)
        for u, v in zip(a, b):
            assert np.abs(u - v).max() < 1e-12 * max(1.0, np.abs(u).max())
        assert ("observation" in r) == bool(kw)
        # without the tag: the same dict as the problem without pose edges gives
        plain = {k: v for k, v in g.items() if k != "pose_edges"}
        p2 = str(tmp_path / "plain.g2o")
        g2o_io.write_g2o_ba(p2, plain)
        assert "EDGE_SE3:EXPMAP" not in open(p2).read()
        q, full = g2o_io.read_g2o_ba(p2), dict(r)
        full.pop("pose_edges")
        assert "pose_edges" not in q and sorted(q) == sorted(full)
        for k in q:
            assert np.array_equal(q[k], full[k]), k


def test_make_ba_odometry():
    a, b = S.make_ba_odometry(20, 100, loop_every=5, seed=3), S.make_ba_odometry(20, 100, loop_every=5, seed=3)
    c = S.make_ba_odometry(20, 100, loop_every=5, seed=4)
    pa, pb = a["pose_edges"], b["pose_edges"]
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    assert not np.array_equal(pa["meas"], c["pose_edges"]["meas"])
    base = S.make_ba_problem(20, 100, seed=3)
    for k in base:
        assert np.array_equal(a[k], base[k]), k                       # the projection problem is make_ba_problem's
    n_odo = 18                                                        # (0, 1) joins two fixed cameras and is left out
    assert pa["n"] == n_odo + 3 and np.array_equal(pa["vj"][:n_odo] - pa["vi"][:n_odo], np.ones(n_odo))
    assert np.array_equal(pa["vj"][n_odo:] - pa["vi"][n_odo:], np.full(3, 5))
    assert np.array_equal(pa["v0"], a["cam_hidx"][pa["vi"]]) and np.array_equal(pa["v1"], a["cam_hidx"][pa["vj"]])
    truth = np.zeros((20, 12))
    truth[:, 0] = truth[:, 4] = truth[:, 8] = 1.0
    truth[:, 9] = -np.arange(20) * 0.5
    e = X.pose_edges(truth, pa["vi"], pa["vj"], pa["meas"], jac=False)      # the noise alone
    assert 0 < np.abs(e[:, :3]).max() < 5 * 0.002 and 0 < np.abs(e[:, 3:]).max() < 5 * 0.01
    s = S.make_ba_odometry(20, 100, loop_every=5, seed=3, stereo_baseline=0.2)
    assert s["observation"] == "stereo" and np.array_equal(s["pose_edges"]["meas"], pa["meas"])


def test_interface_is_declared_everywhere():
    name = "g2ohip_ba_set_pose_edges"
    hdr = open(os.path.join(ROOT, "include", "g2ohip.h")).read()
    assert name in hdr and "types_six_dof_expmap.cpp:271-286" in hdr and "se3quat.h:178-215" in hdr
    from openslam_g2o_amd import capi
    assert callable(getattr(capi.HipBlockSolver, "baSetPoseEdges"))
    hpp = open(os.path.join(ROOT, "openslam_g2o_amd", "cpp", "hip_block_solver.hpp")).read()
    assert "baSetPoseEdges" in hpp and name in hpp
    inc = open(os.path.join(ROOT, "openslam_g2o_amd", "csrc", "ba_pose_edge.inc")).read()
    assert "scratch 0" in inc and "VGPRs" in inc
