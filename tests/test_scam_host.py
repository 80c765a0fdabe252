"""Host side of the stereo observations of VertexSCam cameras (Edge_XYZ_VSC = type 23; CPU only): openslam_g2o_amd/scam.py in fp64
against the 60-digit fixture tests/golden/scam_edges.npz within the recorded drift, the exact Jacobian against the reference's
central difference through the VertexSE3 oplus at 60 digits, mapPoint on a hand-computed point of sba_demo's set-up, the wording
of the headers, the generator, the set-up of the device graph (recorded, no device) and the CPU Levenberg-Marquardt runs whose
drift profiles/scam_edges.jsonl records."""
import ctypes
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm, scam as SC, synthetic as S
from tests import scam_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(H.GOLDEN)


def test_restatement_in_fp64_equals_the_fixture_within_the_stored_drift():
    g = H.load_graph(Z)
    for form in (SC.scam_edges_numpy, lambda *a: SC.scam_edges(SC.FP64, *a)):
        J0, J1, err = form(g["poses"], g["points"], g["vp"], g["vl"], g["zl"], g["kcam"])
        for row, n in enumerate(H.EDGE_COUNTS):
            de = np.abs(err[:n] - Z["err"][:n]).max()
            dJ = max(np.abs(J0[:n] - Z["J0"][:n]).max(), np.abs(J1[:n] - Z["J1"][:n]).max())
            assert de <= Z["drift"][row, 0] and dJ <= Z["drift"][row, 1], (n, de, dJ, Z["drift"][row])
    assert Z["drift"][0, 0] > 0 and Z["moved_drift"][0] > 0          # (8 x 0 would ask the device for bit equality)
    # the moved state: the oracle's oplus on the free cameras, plain addition on the free points
    mp, mq = H.oplus(g, g["poses"], g["points"], Z["moved_x"])
    assert np.array_equal(mp, Z["moved_poses"]) and np.array_equal(mq, Z["moved_points"])
    assert np.array_equal(mp[0], g["poses"][0]) and np.array_equal(mq[11], g["points"][11]) and not np.array_equal(mp[1:], g["poses"][1:])
    em = H.producers(H.FP64, g, mp, mq, jac=False)
    for row, n in enumerate(H.EDGE_COUNTS):
        assert np.abs(em[:n] - Z["moved_err"][:n]).max() <= Z["moved_drift"][row]
    assert H.depths(g).min() >= H.MIN_DEPTH and H.depths(g, mp, mq).min() >= H.MIN_DEPTH


def test_graph_of_the_fixture_is_the_generators():
    g, b = H.load_graph(Z), H.base_graph()
    for k in H.GRAPH_KEYS:
        assert np.array_equal(g[k], b[k]), k
    assert (g["n"], g["nP"], g["L"], g["nL"], g["E"], g["M"]) == (4, 3, 12, 11, 3, 300)
    pairs = set(zip(g["vp"].tolist(), g["vl"].tolist()))
    assert len(pairs) == 48 and g["hidx"][0] == -1 and g["pt_hidx"][11] == -1           # pairs repeat; one fixed vertex of each kind
    R = g["poses"][:, :9].reshape(4, 3, 3)
    for i in range(4):                                                                   # rotations: proper, far from the identity ...
        assert np.abs(R[i] @ R[i].T - np.eye(3)).max() < 1e-14 and np.trace(R[i]) < 2.0
        for j in range(i):                                                               # ... and from each other (angle > 0.5 rad)
            assert np.trace(R[i] @ R[j].T) < 1.0 + 2.0 * np.cos(0.5)


def test_exact_jacobian_equals_the_central_difference_at_60_digits():
    MP = H.MP()
    g = H.load_graph(Z)
    noise = float(Z["numeric_noise"])
    assert 0 < noise < 1e-9 * float(Z["J_max_abs"])
    worst = 0.0
    for k in list(range(0, 300, 7)) + [299]:
        X, L = g["poses"][g["vp"][k]], g["points"][g["vl"][k]]
        A, B = SC.scam_jacobians(MP, X, L, g["kcam"])
        N0, N1 = SC.numeric_jacobians(MP, X, L, g["kcam"], g["zl"][k])
        worst = max(worst, max(abs(float(n - a)) for n, a in zip(N0 + N1, A + B)))
    print("central difference vs exact at 60 digits", worst, "recorded", noise)
    assert worst <= 8.0 * noise
    # in fp64 the same difference is dominated by its own rounding error: |e| eps / delta, here ~1e3 * 1e-16 / 1e-9
    X, L = g["poses"][1], g["points"][3]
    A, B = SC.scam_jacobians(SC.FP64, X, L, g["kcam"])
    N0, N1 = SC.numeric_jacobians(SC.FP64, X, L, g["kcam"], g["zl"][0])
    assert max(abs(n - a) for n, a in zip(N0 + N1, A + B)) < 1e-2
    # the translation is in the camera frame: its columns are those of -I, free of R (a world-frame translation would give -R')
    q = SC.camera_point(SC.FP64, X, L)
    assert A[0] == g["kcam"][0] * (-1.0 * q[2] - q[0] * 0.0) / (q[2] * q[2]) and A[1] == 0.0 and A[3] == 0.0


def test_map_point_of_a_hand_computed_point():
    """sba_demo.cpp:189-230: camera 0 at (-1, 0, 0) with the identity rotation, Kcam (500, 500, 320, 240), baseline 0.075.  The
    point (0.5, -0.25, 10) lies at q = (1.5, -0.25, 10) in its frame: u = 500 * 1.5 / 10 + 320 = 395, v = 500 * -0.25 / 10 + 240 =
    227.5, u_right = 500 * (1.5 - 0.075) / 10 + 320 = 391.25."""
    X = [1, 0, 0, 0, 1, 0, 0, 0, 1, -1.0, 0.0, 0.0]
    assert SC.map_point(SC.FP64, X, [0.5, -0.25, 10.0], S.SCAM_KCAM) == [395.0, 227.5, 391.25]
    assert [float(v) for v in SC.map_point(H.MP(), X, [0.5, -0.25, 10.0], S.SCAM_KCAM)] == [395.0, 227.5, 391.25]
    assert SC.scam_error(SC.FP64, X, [0.5, -0.25, 10.0], S.SCAM_KCAM, [394.0, 228.0, 391.0]) == [1.0, -0.5, 0.25]
    # a rotated camera: 90 degrees about y turns the camera's z axis onto the world's x axis
    Xr = [0, 0, -1, 0, 1, 0, 1, 0, 0, 0.0, 0.0, 0.0]
    assert SC.camera_point(SC.FP64, Xr, [10.0, -0.25, -1.5]) == [1.5, -0.25, 10.0]
    # the oplus is VertexSE3's: translation in the camera frame
    moved = SC.se3_oplus(SC.FP64, Xr, [0.0, 0.0, 2.0, 0.0, 0.0, 0.0])
    assert moved[9:] == [2.0, 0.0, 0.0] and moved[:9] == [float(v) for v in Xr[:9]]


def test_headers_carry_the_entry_and_its_wording():
    header = open(os.path.join(ROOT, "include", "g2ohip.h")).read()
    assert "int g2ohip_pg_set_scam_edges(g2ohip_solver* s, int set," in header
    entry = header[header.index("type 23 = Edge_XYZ_VSC"):header.index("int g2ohip_pg_set_scam_edges")]
    for word in ("DELIBERATE DEVIATION", "types_icp.h:376-413", "SCAM_ANALYTIC_JACOBIANS", "vertex 0 of the set is the POSE", "Not covered:",
                 "the g2o plugin adapter", "sharded solves", "per-camera intrinsics", "more than one landmark set per handle"):
        assert word in entry, word
    gicp = header[header.index("Type 15 = Edge_V_V_GICP"):header.index("int g2ohip_pg_set_gicp_edges")]
    assert "Not covered: VertexSCam" not in gicp and "g2ohip_pg_set_scam_edges" in gicp
    kernel = open(os.path.join(ROOT, "openslam_g2o_amd", "csrc", "pg_scam.inc")).read()
    for word in ("DELIBERATE DEVIATION", "types_icp.cpp:242-321", "pop()", "pg_store<STAGED, 18>"):
        assert word in kernel, word
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "g2ohip_pg_set_scam_edges" in text and "Not covered: `VertexSCam`" not in text, doc
    survey = open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "stay OUT" not in survey[survey.index("`g2o/types/icp`"):].split("\n")[0]
    lib = os.environ.get("G2OHIP_LIB") or os.path.join(ROOT, "openslam_g2o_amd", "lib", "libg2ohip.so")
    if not os.path.exists(lib):
        pytest.fail("the library is not built: %s" % lib)
    assert hasattr(ctypes.CDLL(lib), "g2ohip_pg_set_scam_edges")
    from openslam_g2o_amd import capi
    assert hasattr(capi.HipBlockSolver, "pgSetScamEdges") and "g2ohip_pg_set_scam_edges" in capi.EXPORTS
    hpp = open(os.path.join(ROOT, "openslam_g2o_amd", "cpp", "hip_block_solver.hpp")).read()
    assert "pgSetScamEdges" in hpp


def test_make_scam_ba():
    a, b = S.make_scam_ba(5, 500, seed=3), S.make_scam_ba(5, 500, seed=3)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert a["observation"] == "stereo_vsc" and tuple(a["kcam"]) == (500.0, 500.0, 320.0, 240.0, 0.075)
    assert a["n"] == 5 and a["nP"] == 3 and list(a["hidx"]) == [-1, -1, 0, 1, 2] and len(a["vi"]) == 0 and a["Z"].shape == (0, 12)
    assert np.array_equal(a["poses_true"][:, 9], np.arange(5) * 0.04 - 1.0) and np.array_equal(a["poses"], a["poses_true"])
    assert a["points_true"][:, 2].min() >= 10.0 and a["points_true"][:, 2].max() < 11.0 and np.abs(a["points_true"][:, 1]).max() <= 0.5
    assert np.bincount(a["vl"], minlength=a["L"]).min() >= 2 and a["M"] == len(a["vp"]) == len(a["zl"])
    assert sorted(a["pt_hidx"]) == list(range(a["nP"], a["nP"] + a["L"])) and a["nL"] == a["L"]
    # only observations inside the image, measured with the stated noise
    proj = SC.scam_edges_numpy(a["poses_true"], a["points_true"], a["vp"], a["vl"], np.zeros((a["M"], 3)), a["kcam"], jac=False)
    assert proj[:, 0].min() >= 0 and proj[:, 0].max() < 640 and proj[:, 1].min() >= 0 and proj[:, 1].max() < 480
    e = a["zl"] - proj
    assert 0.8 < e[:, 0].std() < 1.2 and 0.8 < e[:, 1].std() < 1.2 and 0.8 / 16 < e[:, 2].std() < 1.2 / 16
    assert 0.8 < (a["points"] - a["points_true"]).std() < 1.2
    # every camera that sees a point observes it: the same count by brute force
    full = SC.scam_edges_numpy(a["poses_true"], a["points_true"], np.repeat(np.arange(5), a["L"]), np.tile(np.arange(a["L"]), 5),
                               np.zeros((5 * a["L"], 3)), a["kcam"], jac=False)
    assert ((full[:, 0] >= 0) & (full[:, 0] < 640) & (full[:, 1] >= 0) & (full[:, 1] < 480)).sum() == a["M"]
    o = S.make_scam_ba(6, 120, outlier_frac=0.05, fixed_points=3)
    assert 10 < o["outlier"].sum() < 80 and list(o["pt_hidx"][:4]) == [-1, -1, -1, o["nP"]] and o["nL"] == o["L"] - 3
    eo = o["zl"] - SC.scam_edges_numpy(o["poses_true"], o["points_true"], o["vp"], o["vl"], np.zeros((o["M"], 3)), o["kcam"], jac=False)
    assert np.abs(eo[~o["outlier"]]).max() < 6 and np.abs(eo[o["outlier"]]).max() > 50
    j = S.make_scam_ba(6, 120, gicp=True)
    plain = S.make_scam_ba(6, 120)
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(j[k])), k
    assert len(j["gi"]) == 100 and np.array_equal(j["gj"], j["gi"] + 1) and j["gmeas"].shape == (100, 6) and j["ginfo"].shape == (100, 9)
    assert j["gcov"] is None and np.abs(np.linalg.norm(j["normal0"], axis=1) - 1).max() < 1e-14
    from openslam_g2o_amd import gicp as G
    eg = G.gicp_edges(SC.FP64, j["poses_true"], j["gi"], j["gj"], j["gmeas"], None, jac=False)[0]
    assert 0 < np.abs(eg).max() < 0.1
    # a size with five observations per point
    big = S.make_scam_ba(400, 4000, spacing=2.56)
    assert 4.5 < big["M"] / big["L"] < 5.5
    with pytest.raises(ValueError):
        S.make_scam_ba(5, 100, fixed=5)


def test_existing_generators_return_what_they_did():
    """make_scam_ba is a new function over streams of its own: the digests recorded for make_landmark_slam still hold."""
    import hashlib
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "landmark_slam_default_sha256.json")))
    assert rec
    g = S.make_gicp(4, 10)
    assert len(g["gi"]) == 30 and g["poses"].shape == (4, 12)
    assert hashlib.sha256(np.ascontiguousarray(S._GICP_PLANES).tobytes()).hexdigest() == hashlib.sha256(
        np.array([[1.0, 0.1, 0.2, 6.0], [0.1, 0.5, 1.0, 2.5], [-0.3, 0.2, 1.0, 3.0], [-1.0, 0.3, 0.4, 5.0], [0.2, 0.6, -1.0, 2.0]]).tobytes()).hexdigest()


class _Recorder:
    """Stands in for capi.HipBlockSolver: records the calls lm.setup_device_landmark_slam makes."""

    def __init__(self, *args):
        self.calls = [("init",) + args]
        self.sets = 0

    def addEdgeSet(self, d, v0, v1):
        self.calls.append(("addEdgeSet", d, len(v0), v1 is None))
        self.sets += 1
        return self.sets - 1

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + tuple(a if np.isscalar(a) or a is None else np.asarray(a).shape for a in args))
        return call


def test_setup_binds_the_stereo_set_and_the_gicp_set_on_one_handle(monkeypatch):
    from openslam_g2o_amd import capi
    monkeypatch.setattr(capi, "HipBlockSolver", _Recorder)
    g = S.make_scam_ba(6, 120)
    s, _ = lm.setup_device_landmark_slam(g, huber_delta=1.0)
    assert [c[0] for c in s.calls] == ["init", "addEdgeSet", "addEdgeSet", "buildStructure", "pgSetEdges", "pgSetEstimates", "pgSetScamEdges",
                                       "pgSetLandmarkEstimates", "setRobustKernel"]
    assert s.calls[0] == ("init", 6, 3, 0) and s.calls[1] == ("addEdgeSet", 6, 0, False) and s.calls[2] == ("addEdgeSet", 3, g["M"], False)
    assert s.calls[4] == ("pgSetEdges", 0, 2, (0,), (0,), (0, 12), (0, 36)) and s.calls[6][-1] == (5,) and s.landmark_sets == (0, 1)
    j, _ = lm.setup_device_landmark_slam(S.make_scam_ba(6, 120, gicp=True))
    assert [c[0] for c in j.calls] == ["init", "addEdgeSet", "addEdgeSet", "addEdgeSet", "buildStructure", "pgSetEdges", "pgSetEstimates",
                                       "pgSetScamEdges", "pgSetGicpEdges", "pgSetLandmarkEstimates"]
    assert j.calls[3] == ("addEdgeSet", 3, 100, False) and j.calls[8][1] == 2
    with pytest.raises(ValueError):
        lm.setup_device_landmark_slam(dict(g, kcam=g["kcam"][:4]))


def test_cpu_lm_over_the_oracle_descends_and_its_drift_is_recorded():
    """The two CPU runs of tools/scam_ba_time.py --drift: the oracle's Schur path and the dense solve take the same trials, chi2
    descends through all iterations, and their relative gap is what profiles/scam_edges.jsonl records."""
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "scam_edges.jsonl")):
        d = json.loads(line)
        if d.get("what") == "oracle_drift":
            rec[d["graph"]] = d
    for name, gicp, its in (("scam_ba_6_120", False, H.LM_ITERATIONS), ("scam_ba_6_120_gicp", True, H.JOINT_ITERATIONS)):
        g = H.lm_graph(gicp)
        ra, rb = H.oracle_lm_run(g, its), H.oracle_lm_run(g, its, dense=True)
        print(name, "chi2", ra["chis"], "trials", ra["trials"])
        assert ra["done"] == rb["done"] == its and ra["trials"] == rb["trials"] == rec[name]["trials"]
        assert np.all(np.diff(ra["chis"]) < 0) and ra["chis"][-1] < 0.01 * ra["chis"][0]
        assert np.abs(ra["chis"] - np.array(rec[name]["chi2"])).max() <= 1e-9 * ra["chis"].max()
        gap = np.abs(ra["chis"] - rb["chis"]) / np.abs(rb["chis"])
        assert gap.max() < 1e-12 and max(rec[name]["relative_chi2_gap"]) < 1e-12
        # (the depth of a point 10 units ahead of a 0.2-unit row of cameras stays poorly determined: the lateral position is the check)
        e0 = np.abs(g["points"] - g["points_true"])[:, :2].max()
        assert np.abs(ra["points"] - g["points_true"])[:, :2].max() < 0.5 * e0
