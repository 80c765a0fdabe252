"""CPU side of the landmark SLAM front end (EdgeSE2PointXY / EdgeSE3PointXYZ beside the pose-graph front end): the C ABI
declares and exports the three entries, the NumPy restatement of the two edge types passes the reference's own Jacobian
check, the generator and the `.g2o` reader / writer behave."""
import ctypes
import os
import re

import numpy as np
import pytest

from openslam_g2o_amd import capi, g2o_io, synthetic as S
from oracle import oracle as O
from tests import landmark_helpers as LH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("g2ohip_pg_set_landmark_edges", "g2ohip_pg_set_landmark_estimates", "g2ohip_pg_get_landmark_estimates")


def test_header_declares_and_library_exports_the_landmark_entries():
    hdr = open(os.path.join(ROOT, "include", "g2ohip.h")).read()
    declared = set(re.findall(r"\b(g2ohip_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared, "include/g2ohip.h does not declare %s" % name
        assert hasattr(lib, name), "libg2ohip.so does not export %s" % name
        assert name in capi.EXPORTS
    m = re.search(r"int g2ohip_pg_set_landmark_edges\(([^;]*)\);", hdr)
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["g2ohip_solver* s", "int set", "int type", "const int32_t* pose_vertex", "const int32_t* point_vertex",
                    "const double* meas", "const double* info", "const double* offset"]
    for meth in ("pgSetLandmarkEdges", "pgSetLandmarkEstimates", "pgGetLandmarkEstimates"):
        assert callable(getattr(capi.HipBlockSolver, meth))


@pytest.mark.parametrize("kind", ["se2", "se3"])
def test_numpy_jacobians_against_central_differences(kind):
    """The reference's own check (g2o/types/slam3d/test_slam3d_jacobian.cpp: analytic linearizeOplus against numeric
    differentiation through oplus), as tests/test_oracle.py::test_se3_jacobian_against_central_differences does it for EdgeSE3:
    central differences of the restatement's error through the oracle's pose oplus and plain addition on the landmark, step
    1e-6, bound 1e-6.  The SE3 graph carries a non-identity sensor offset."""
    g = S.make_landmark_slam(kind, 60, 90)
    if kind == "se3":
        assert np.abs(g["offset"] - np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])).max() > 0.05
    dp, dl = LH.dims(g)
    J0, J1, err = LH.landmark_edges(g)
    M = g["M"]
    assert J0.shape == (M, dl * dp) and J1.shape == (M, dl * dl) and err.shape == (M, dl)
    h = 1e-6
    oplus = O.se2_oplus if kind == "se2" else O.se3_oplus
    every = np.arange(g["n"], dtype=np.int32)          # every pose moves by the same increment: one sweep per column
    worst = 0.0
    for c in range(dp):
        x = np.zeros((g["n"], dp))
        x[:, c] = h
        ep = LH.landmark_edges(g, poses=oplus(g["poses"], every, x.ravel()), jac=False)
        em = LH.landmark_edges(g, poses=oplus(g["poses"], every, -x.ravel()), jac=False)
        num = (ep - em) / (2 * h)
        worst = max(worst, np.abs(num - J0.reshape(M, dp, dl)[:, c, :]).max())
    for c in range(dl):
        d = np.zeros((g["L"], dl))
        d[:, c] = h
        ep = LH.landmark_edges(g, points=g["points"] + d, jac=False)
        em = LH.landmark_edges(g, points=g["points"] - d, jac=False)
        num = (ep - em) / (2 * h)
        worst = max(worst, np.abs(num - J1.reshape(M, dl, dl)[:, c, :]).max())
    print("%s: largest |analytic - central difference| = %.3e" % (kind, worst))
    assert worst < 1e-6
    # points_oplus: plain addition of the landmark's slice, fixed ones stay
    gf = S.make_landmark_slam(kind, 60, 90, fixed_landmarks=3)
    x = np.arange(dp * gf["nP"] + dl * gf["nL"], dtype=np.float64)
    moved = LH.points_oplus(gf["points"], gf["pt_hidx"], x, dp * gf["nP"], gf["nP"])
    assert np.array_equal(moved[:3], gf["points"][:3])
    assert np.array_equal(moved[3:], gf["points"][3:] + x[dp * gf["nP"]:].reshape(-1, dl))


@pytest.mark.parametrize("kind,n,L", [("se2", 400, 150), ("se3", 200, 300)])
def test_generator_is_deterministic_and_shaped(kind, n, L):
    a = S.make_landmark_slam(kind, n, L, outlier_frac=0.05, fixed_landmarks=2)
    b = S.make_landmark_slam(kind, n, L, outlier_frac=0.05, fixed_landmarks=2)
    for k in ("poses", "points", "Z", "zl", "vi", "vj", "vp", "vl", "omega", "omega_l", "hidx", "pt_hidx"):
        assert np.array_equal(a[k], b[k]), k
    c = S.make_landmark_slam(kind, n, L, outlier_frac=0.05, fixed_landmarks=2, seed=43)
    assert not np.array_equal(a["zl"], c["zl"])
    dp, dl = LH.dims(a)
    E, M = a["E"], a["M"]
    assert a["n"] == n and a["L"] == L and a["nP"] == n - 1 and a["nL"] == L - 2
    assert a["poses"].shape == (n, 3 if kind == "se2" else 12) and a["points"].shape == (L, dl)
    assert a["poses_true"].shape == a["poses"].shape and a["points_true"].shape == a["points"].shape
    assert a["Z"].shape == (E, 3 if kind == "se2" else 12) and a["omega"].shape == (E, dp * dp)
    assert a["zl"].shape == (M, dl) and a["omega_l"].shape == (M, dl * dl)
    for k, hi in (("vi", n), ("vj", n), ("vp", n), ("vl", L)):
        assert a[k].dtype == np.int32 and a[k].min() >= 0 and a[k].max() < hi
    assert E >= n - 1 and (a["vj"][:n - 1] - a["vi"][:n - 1] == 1).all()
    assert E > n - 1 and (a["vj"][n - 1:] - a["vi"][n - 1:] > 1).all()            # loop closures: places are revisited
    seen = np.bincount(a["vl"], minlength=L)
    assert seen.min() >= 1                                                          # every landmark observed
    assert np.median(seen) >= 3                                                     # ... most of them from several poses
    assert len(np.unique(a["vp"].astype(np.int64) * L + a["vl"])) == M              # no observation twice
    assert a["hidx"][0] == -1 and np.array_equal(a["hidx"][1:], np.arange(n - 1))
    assert (a["pt_hidx"][:2] == -1).all() and np.array_equal(a["pt_hidx"][2:], a["nP"] + np.arange(L - 2))
    assert np.array_equal(a["points"][:2], a["points_true"][:2]) and np.array_equal(a["poses"][0], a["poses_true"][0])
    # at the ground truth the observation errors are the measurement noise (sigma 0.05) except for the outliers
    e = LH.landmark_edges(a, poses=a["poses_true"], points=a["points_true"], jac=False)
    r = np.linalg.norm(e, axis=1)
    assert np.median(r) < 0.15 and 0.01 * M < (r > 0.5).sum() < 0.1 * M
    if kind == "se3":
        R = a["poses"][:, :9].reshape(-1, 3, 3)
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12


@pytest.mark.parametrize("kind", ["se2", "se3"])
def test_reader_writer_round_trip(kind, tmp_path):
    g = S.make_landmark_slam(kind, 40, 30, fixed_landmarks=1)
    path = str(tmp_path / "lm.g2o")
    g2o_io.write_g2o_landmarks(path, g)
    text = open(path).read().split("\n")
    tags = ("VERTEX_SE2", "VERTEX_XY", "EDGE_SE2", "EDGE_SE2_XY") if kind == "se2" else \
        ("VERTEX_SE3:QUAT", "VERTEX_TRACKXYZ", "EDGE_SE3:QUAT", "EDGE_SE3_TRACKXYZ")
    counts = [sum(l.split(" ", 1)[0] == t for l in text) for t in tags]
    assert counts == [40, 30, g["E"], g["M"]]
    assert ("FIX 0 40" in text) and (kind == "se2" or text[0].startswith("PARAMS_SE3OFFSET 0 "))
    rd = g2o_io.read_g2o(path)
    assert rd["kind"] == kind and np.array_equal(rd["point_ids"], 40 + np.arange(30))
    assert rd["fixed"] == [0] and rd["fixed_points"] == [0]
    back = g2o_io.landmark_problem(rd)
    for k in ("n", "L", "nP", "nL", "E", "M"):
        assert back[k] == g[k], k
    for k in ("vi", "vj", "vp", "vl", "hidx", "pt_hidx"):
        assert np.array_equal(back[k], g[k]), k
    tol = 0.0 if kind == "se2" else 1e-14            # (3-D poses pass through quaternions)
    for k in ("poses", "Z"):
        assert np.abs(back[k] - g[k]).max() <= tol * max(1.0, np.abs(g[k]).max()), k
    for k in ("points", "zl", "omega", "omega_l"):
        assert np.array_equal(back[k], g[k]), k
    if kind == "se3":
        assert np.abs(back["offset"] - g["offset"]).max() < 1e-14
    # the same linearised graph
    e0, e1 = LH.landmark_edges(g, jac=False), LH.landmark_edges(back, jac=False)
    assert np.abs(e0 - e1).max() <= 1e-12 * np.abs(e0).max()
    # index mapping: free poses by id, then the free landmarks by id (sparse_optimizer.cpp:174-187)
    h, hl, nP, nL = g2o_io.landmark_hessian_index(5, 4, [1], [0, 2])
    assert list(h) == [0, -1, 1, 2, 3] and list(hl) == [-1, 4, -1, 5] and (nP, nL) == (4, 2)


def test_pose_only_file_reads_as_before(tmp_path):
    """A file without landmark tags: the keys and values read_g2o has always returned, nothing else."""
    path = str(tmp_path / "pg.g2o")
    with open(path, "w") as f:
        f.write("VERTEX_SE2 3 1 2 0.5\nVERTEX_SE2 1 0 0 0\nVERTEX_SE2 2 0.5 1 0.25\nFIX 1\n")
        f.write("EDGE_SE2 1 2 0.5 1 0.25 10 1 2 20 3 30\nEDGE_SE2 2 3 0.5 1 0.25 10 0 0 20 0 30\n")
    rd = g2o_io.read_g2o(path)
    assert sorted(rd.keys()) == sorted(["kind", "ids", "estimates", "vi", "vj", "meas", "info", "fixed"])
    assert rd["kind"] == "se2" and list(rd["ids"]) == [1, 2, 3] and rd["fixed"] == [0]
    assert np.array_equal(rd["estimates"], [[0, 0, 0], [0.5, 1, 0.25], [1, 2, 0.5]])
    assert list(rd["vi"]) == [0, 1] and list(rd["vj"]) == [1, 2]
    assert np.array_equal(rd["info"][0], [[10, 1, 2], [1, 20, 3], [2, 3, 30]])
    with pytest.raises(ValueError):
        g2o_io.landmark_problem(rd)
