"""Host side of the SBA-format front end (no GPU): the fp64 restatement openslam_g2o_amd/sbacam.py of VertexCam /
EdgeProjectP2MC / EdgeProjectP2SC, the `.g2o` reader and writer, the problem builders and the golden file."""
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io as IO, sbacam as SB, synthetic as S
from tests import sbacam_helpers as H

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "sbacam_edges.npz"))
F = SB.FP64


def _err(cam, X, kc, z, stereo):
    return np.array(SB.project_error(F, cam, X, kc, z, stereo))


@pytest.mark.parametrize("stereo", [False, True])
def test_analytic_jacobian_against_central_differences(stereo):
    """The reference's analytic Jacobian (types_sba.cpp:249-403) against central differences of the restated error through the
    restated oplus (camera) and plain addition (point).  The bound is derived here, per column: a central difference of step h
    is off by h^2 / 6 * |f'''| (truncation) and by eps * |e| / h (rounding of the two errors); f''' along the column is itself
    measured by a fourth-order stencil of second differences at a ten times larger step, with a factor 2 for that estimate's
    own error; h = 1e-4 balances the two terms near 1e-9 relative.  For the quaternion columns the analytic entry is the
    derivative of the reference's update at 0, which the central difference through oplus is as well (qr.w = sqrt(1 - |v|^2)
    is even in v)."""
    g = H.random_graph(65, 5, stereo)
    h = 1e-4
    eps = np.finfo(np.float64).eps
    worst = 0.0
    for k in range(0, 65, 7):
        a, b = int(g["vp"][k]), int(g["vl"][k])
        cam, X, kc, z = g["est"][a], g["points"][b], g["intrinsics"][a], g["zl"][k]
        Jc, Jx = SB.project_jacobians(F, cam, X, kc, stereo)
        Jc, Jx = np.array(Jc), np.array(Jx)

        def along(c, s):
            if c < 6:
                x = np.zeros(6)
                x[c] = s
                return _err(SB.oplus(F, cam, x), X, kc, z, stereo)
            dX = np.zeros(3)
            dX[c - 6] = s
            return _err(cam, X + dX, kc, z, stereo)

        for c in range(9):
            num = (along(c, h) - along(c, -h)) / (2 * h)
            H3 = 10 * h
            f3 = np.abs(along(c, 2 * H3) - 2 * along(c, H3) + 2 * along(c, -H3) - along(c, -2 * H3)) / (2 * H3 ** 3)
            scale = np.abs(along(c, 0.0)) + np.abs(z)             # (the projection's magnitude: what the subtraction rounds)
            bound = 2 * f3 * h * h / 6 + 4 * eps * scale / h
            ana = Jc[:, c] if c < 6 else Jx[:, c - 6]
            assert (np.abs(num - ana) <= bound).all(), (k, c, num, ana, bound)
            worst = max(worst, float((np.abs(num - ana) / bound).max()))
    print("worst |numeric - analytic| / bound", worst)


def test_oplus_composition_and_normalisation():
    """SBACam::update: t moves by x[0:3] exactly; the new quaternion has norm 1 to rounding also from an unnormalised start; the
    rotation is R(q) R(qr) (post-multiplication); a zero step leaves a unit camera's rotation and translation; no sign flip."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        cam = np.concatenate([rng.normal(size=3), q])
        x = np.concatenate([rng.normal(size=3), rng.normal(size=3) * 0.1])
        out = np.array(SB.oplus(F, cam, x))
        assert np.array_equal(out[:3], cam[:3] + x[:3])
        assert abs(np.linalg.norm(out[3:]) - 1.0) <= 4 * np.finfo(float).eps
        qr = np.concatenate([x[3:], [np.sqrt(1 - x[3:] @ x[3:])]])
        R, Rr = SB.transform(cam)[0], SB.transform(np.concatenate([np.zeros(3), qr]))[0]
        assert np.abs(SB.transform(out)[0] - R @ Rr).max() <= 64 * np.finfo(float).eps
        scaled = np.concatenate([cam[:3], 3.0 * q])
        assert abs(np.linalg.norm(SB.oplus(F, scaled, x)[3:]) - 1.0) <= 4 * np.finfo(float).eps
        same = np.array(SB.oplus(F, cam, np.zeros(6)))
        assert np.abs(same - cam).max() <= 4 * np.finfo(float).eps
        neg = np.array(SB.oplus(F, np.concatenate([cam[:3], -q]), np.zeros(6)))
        assert np.abs(neg[3:] + q).max() <= 4 * np.finfo(float).eps      # -q stays -q: no normalizeRotation
    two = SB.update(F, np.stack([cam, cam]), np.array([-1, 0]), x)
    assert np.array_equal(two[0], cam) and not np.array_equal(two[1], cam)


@pytest.mark.parametrize("stereo", [False, True])
def test_g2o_round_trip(tmp_path, stereo):
    """A written file read back: every double bit for bit (translations, points, measurements, intrinsics and baselines), the
    quaternion normalised on read as VertexCam::read does, FIX lines -> hessian indices, the information the identity."""
    g = S.make_sbacam_ba(12, 30, 4, stereo=stereo, seed=3)
    g["pt_hidx"] = g["pt_hidx"].copy()
    g["pt_hidx"][2] = -1
    g["pt_hidx"][3:] -= 1
    g["nL"] -= 1
    g["est"] = g["est"].copy()
    g["est"][4, 3:] *= 2.5                                          # an unnormalised quaternion in the file
    path = str(tmp_path / "cams.g2o")
    IO.write_g2o_sbacam(path, g)
    rd = IO.read_g2o(path)
    assert rd["kind"] == "sbacam" and rd["cam_stereo"] == stereo and len(rd["vi"]) == 0
    q = IO.sbacam_ba_problem(rd)
    for k in ("points", "hidx", "pt_hidx", "vp", "vl", "zl", "omega_l", "intrinsics"):
        assert np.array_equal(q[k], g[k]), k
    assert (q["nP"], q["nL"], q["stereo"]) == (g["nP"], g["nL"], stereo)
    assert np.array_equal(q["est"][:, :3], g["est"][:, :3])
    e = g["est"][:, 3:]
    norm = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2] + e[:, 3] * e[:, 3])
    assert np.array_equal(q["est"][:, 3:], e / norm[:, None])
    assert np.abs(np.linalg.norm(q["est"][:, 3:], axis=1) - 1.0).max() <= 2 * np.finfo(float).eps
    assert len(np.unique(q["intrinsics"], axis=0)) == 12
    q2 = IO.sbacam_ba_problem(rd, fixed_cams=[0, 5], fixed_points=[])
    assert q2["nP"] == 10 and q2["nL"] == 30 and q2["hidx"][5] == -1 and q2["hidx"][6] == 4 and q2["pt_hidx"][0] == 10


def test_sbacam_ba_problem_hessian_indices(tmp_path):
    """Free cameras by vertex id, then free points by vertex id (sparse_optimizer.cpp:174-187), whatever the order of the
    lines; a VERTEX_CAM line without intrinsics gets the reference's defaults."""
    path = str(tmp_path / "shuffled.g2o")
    with open(path, "w") as f:
        f.write("VERTEX_XYZ 12 0.5 0.25 4\nVERTEX_CAM 7 0 0 0 0 0 0 2 500 510 320 240 0.1\nVERTEX_XYZ 10 -0.5 0 5\n"
                "VERTEX_CAM 3 1 0 0 0 0 0 1\nVERTEX_CAM 5 2 0 0 0 0 0 1 400 410 300 200 0.2\nFIX 3 12\n"
                "EDGE_PROJECT_P2MC 10 7 1.5 2.5\nEDGE_PROJECT_P2MC 12 3 3 4\nEDGE_PROJECT_P2MC 10 5 5 6\n")
    rd = IO.read_g2o(path)
    q = IO.sbacam_ba_problem(rd)
    assert list(rd["ids"]) == [3, 5, 7] and list(rd["cam_point_ids"]) == [10, 12]
    assert list(q["hidx"]) == [-1, 0, 1] and list(q["pt_hidx"]) == [2, -1] and (q["nP"], q["nL"]) == (2, 1)
    assert list(q["vp"]) == [2, 0, 1] and list(q["vl"]) == [0, 1, 0]
    assert np.array_equal(q["zl"], [[1.5, 2.5], [3, 4], [5, 6]]) and np.array_equal(q["omega_l"], np.tile([1.0, 0, 0, 1], (3, 1)))
    assert np.array_equal(q["intrinsics"], [[300, 300, 320, 320, 0.1], [400, 410, 300, 200, 0.2], [500, 510, 320, 240, 0.1]])
    assert np.array_equal(q["est"][2], [0, 0, 0, 0, 0, 0, 1])       # (0, 0, 0, 2) normalised


def test_vertex_xyz_keeps_its_meaning_for_the_other_readers(tmp_path):
    """VERTEX_XYZ is one tag: the same three doubles reach the sim3 keys of read_g2o, read_g2o_ba and the cam keys."""
    g = S.make_sbacam_ba(12, 8, 3, seed=1)
    pa, pb, pc = (str(tmp_path / n) for n in ("cam.g2o", "sim3.g2o", "ba.g2o"))
    IO.write_g2o_sbacam(pa, g)
    s3 = S.make_sim3_ba(12, 8, 3, seed=1)
    s3["points"] = g["points"]
    IO.write_g2o_sim3(pb, s3["est"], s3["vi"], s3["vj"], s3["meas"], s3["info"], extras=s3["intrinsics"], points=s3["points"],
                      vp=s3["vp"], vl=s3["vl"], zl=s3["zl"], omega_l=s3["omega_l"])
    with open(pc, "w") as f:
        f.write("PARAMS_CAMERAPARAMETERS 0 500 320 240 0\nVERTEX_SE3:EXPMAP 0 0 0 0 0 0 0 1\n")
        for j, X in enumerate(g["points"]):
            f.write("VERTEX_XYZ %d %s\n" % (1 + j, " ".join("%.17g" % v for v in X)))
    ra, rb, rc = IO.read_g2o(pa), IO.read_g2o(pb), IO.read_g2o_ba(pc)
    assert np.array_equal(ra["cam_points"], g["points"]) and np.array_equal(rb["sim3_points"], g["points"])
    assert np.array_equal(rc["pts"], g["points"])
    assert "sim3_points" not in ra and "cam_points" not in rb and rb["kind"] == "sim3"


def test_error_paths(tmp_path):
    with pytest.raises(ValueError):
        S.make_sbacam_ba(12, 10, 13)
    with pytest.raises(ValueError):
        IO.sbacam_ba_problem(dict(kind="sim3"))
    g = S.make_sbacam_ba(12, 10, 3, seed=2)
    bad = dict(g, omega_l=2.0 * g["omega_l"])
    with pytest.raises(ValueError):
        IO.write_g2o_sbacam(str(tmp_path / "x.g2o"), bad)           # the format has no place for an information matrix
    path = str(tmp_path / "mixed.g2o")
    with open(path, "w") as f:
        f.write("VERTEX_CAM 0 0 0 0 0 0 0 1 1 1 0 0 0\nVERTEX_XYZ 1 0 0 1\nEDGE_PROJECT_P2MC 1 0 0 0\nEDGE_PROJECT_P2SC 1 0 0 0 0\n")
    with pytest.raises(ValueError):
        IO.read_g2o(path)
    path = str(tmp_path / "nopoints.g2o")
    with open(path, "w") as f:
        f.write("VERTEX_CAM 0 0 0 0 0 0 0 1 1 1 0 0 0\n")
    with pytest.raises(ValueError):
        IO.sbacam_ba_problem(IO.read_g2o(path))


def test_python_layer_argument_checks():
    """capi.HipBlockSolver.pgSetCamProjectEdges refuses wrong shapes before the library is called (no GPU, no library)."""
    from openslam_g2o_amd import capi
    s = capi.HipBlockSolver.__new__(capi.HipBlockSolver)
    s._set_sizes = {1: 3}
    vp = vl = np.zeros(3, np.int32)
    k5 = np.ones((2, 5))
    with pytest.raises(ValueError):
        s.pgSetCamProjectEdges(1, 12, vp, vl, np.zeros((3, 2)), np.zeros((3, 4)), k5)       # not 13 / 14
    with pytest.raises(ValueError):
        s.pgSetCamProjectEdges(1, 14, vp, vl, np.zeros((3, 2)), np.zeros((3, 4)), k5)       # stereo needs [n][3], [n][9]
    with pytest.raises(ValueError):
        s.pgSetCamProjectEdges(1, 13, vp[:2], vl, np.zeros((3, 2)), np.zeros((3, 4)), k5)
    with pytest.raises(ValueError):
        s.pgSetCamProjectEdges(1, 13, vp, vl, np.zeros((3, 2)), np.zeros((3, 4)), np.ones((2, 4)))   # (fx, fy, cx, cy) only
    assert capi.HipBlockSolver.PG_POSE_STRIDE[12] == 7 and capi.HipBlockSolver.PG_POSE_DIM[12] == 6
    assert "g2ohip_pg_set_cam_project_edges" in capi.EXPORTS


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("n", H.EDGE_COUNTS)
def test_golden_file_agrees_with_a_fresh_evaluation(n, stereo):
    """The stored inputs are the generator's graph, and the recorded drift is exactly the distance of a fresh fp64 evaluation
    from the stored mpmath figures; every pz is of order 1 or more; the graph has the shared, fixed and repeated vertices the
    GPU tests rely on."""
    name = H.graph_name(n, stereo)
    g = H.random_graph(n, 100 + n + (1000 if stereo else 0), stereo)
    for k in ("est", "points", "hidx", "pt_hidx", "vp", "vl", "zl", "omega_l", "intrinsics"):
        assert np.array_equal(GOLD["%s_%s" % (name, k)], g[k]), k
    J0, J1, err = H.producers(F, g)
    drift = GOLD[name + "_drift"]
    assert np.abs(err - GOLD[name + "_err"]).max() == drift[0]
    assert max(np.abs(J0 - GOLD[name + "_J0"]).max(), np.abs(J1 - GOLD[name + "_J1"]).max()) == drift[1]
    assert drift[0] < 1e-11 and drift[1] < 1e-10                   # (an analytic Jacobian: nothing like the 1e-4 of a numeric one)
    depth = [SB.camera_point(F, g["est"][a], g["points"][b])[2] for a, b in zip(g["vp"], g["vl"])]
    assert min(depth) > 1.5
    if n > 1:
        assert g["hidx"][0] < 0 and g["pt_hidx"][0] < 0 and (g["vp"][2], g["vl"][2]) == (g["vp"][3], g["vl"][3])
        assert len(np.unique(g["intrinsics"], axis=0)) == len(g["intrinsics"]) and len(g["est"]) <= 5 and len(g["points"]) <= 6


def test_golden_update_and_lm_records():
    g = H.random_graph(65, 165, False)
    x = H.update_step(g, 21)
    assert np.array_equal(GOLD["update_x"], x)
    assert H.transform_gap(H.update(F, g["est"], g["hidx"], x), GOLD["update_est"]) == GOLD["update_drift"][0]
    assert np.array_equal(GOLD["update_points"], H.moved_points(g["points"], g["pt_hidx"], g["nP"], x))
    assert np.linalg.norm(x[:6 * g["nP"]].reshape(-1, 6)[:, 3:], axis=1).max() < 0.2
    for tag, stereo, huber in H.RUNS:
        chis, chi0 = GOLD["lm_%s_chis" % tag], GOLD["lm_%s_chi0" % tag][0]
        assert len(chis) == H.ITERATIONS and chis[-1] < 0.01 * chi0
        assert GOLD["lm_%s_est_drift" % tag][0] < 1e-9 and GOLD["lm_%s_points_drift" % tag][0] < 1e-9
