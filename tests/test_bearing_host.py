"""CPU: the bearing-only observations (EdgeSE2PointXYBearing = type 20) on the host side -- the fixture's branch coverage, the
restatement of openslam_g2o_amd/bearing.py in fp64 against its 60-digit evaluation (tests/golden/bearing_edges.npz), the exact
Jacobian against the reference's central difference, the g2o_io round trip, the generator's parallax and distance conditions, LM
over the CPU oracle, the C header and the built library, lm.setup_device_landmark_slam without bearing keys."""
import ctypes
import os

import numpy as np
import pytest

from openslam_g2o_amd import bearing as BE, g2o_io, lm, synthetic as S
from tests import bearing_helpers as H
from tests.producer_metric import wrap_branch

Z = np.load(H.GOLDEN)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _raw(g, poses, points):
    X, L = poses[g["bp"]], points[g["bl"]]
    c, s = np.cos(X[:, 2]), np.sin(X[:, 2])
    dx, dy = L[:, 0] - X[:, 0], L[:, 1] - X[:, 1]
    return g["zb"] - np.arctan2(-s * dx + c * dy, c * dx + s * dy), np.hypot(dx, dy)


def test_fixture_branches_and_distance_floor():
    g = H.load_graph(Z)
    assert len(g["bp"]) == 300 and len(g["poses"]) == 4 and list(g["hidx"]) == [-1, 0, 1, 2] and len(g["vi"]) == 3
    assert len(g["points"]) == 6 and (g["pt_hidx"] < 0).sum() == 1 and len(g["vp"]) == 24
    assert len({(bool(np.cos(t) > 0), bool(np.sin(t) > 0)) for t in g["poses"][:, 2]}) == 4          # the four quadrants
    assert len(set(zip(g["bp"].tolist(), g["bl"].tolist()))) == 24
    for poses, points in ((g["poses"], g["points"]), (Z["moved_poses"], Z["moved_points"])):
        raw, dist = _raw(g, poses, points)
        assert dist.min() >= H.MIN_DISTANCE
        branches = [wrap_branch(r) for r in raw]
        counts = {b: branches.count(b) for b in ("in", "floor", "floor+hi")}
        print("wrap branches", counts, "min distance", dist.min())
        assert min(counts.values()) >= 10 and sum(counts.values()) == 300
        e = H.producers(H.FP64, g, poses, points, jac=False)
        assert (np.pi - np.abs(e)).min() >= 1e-6                                                       # no edge next to the wrap
    near = np.abs(_raw(g, g["poses"], g["points"])[0][0::2])
    assert np.minimum(near, 2 * np.pi - near).max() <= 0.05 + 1e-12                                    # half within 0.05 rad
    moved = H.oplus(g, g["poses"], g["points"], Z["moved_x"])
    assert np.array_equal(moved[0], Z["moved_poses"]) and np.array_equal(moved[1], Z["moved_points"])


def test_restatement_fp64_within_recorded_drift():
    g = H.load_graph(Z)
    J0, J1, err = H.producers(H.FP64, g)
    de = np.abs(err - Z["err"]).max(axis=1)
    dJ = np.maximum(np.abs(J0 - Z["J0"]).max(axis=1), np.abs(J1 - Z["J1"]).max(axis=1))
    em = np.abs(H.producers(H.FP64, g, Z["moved_poses"], Z["moved_points"], jac=False) - Z["moved_err"]).max(axis=1)
    for n, (be, bJ), bm in zip(H.EDGE_COUNTS, Z["drift"], Z["moved_drift"]):
        print(n, "fp64 vs 60 digits (err, J, moved err)", de[:n].max(), dJ[:n].max(), em[:n].max(), "recorded", be, bJ, bm)
        assert de[:n].max() <= be and dJ[:n].max() <= bJ and em[:n].max() <= bm
    assert Z["drift"].max() < 1e-13 and Z["drift"][0, 0] > 0 and Z["moved_drift"][0] > 0


def test_exact_jacobian_against_central_difference():
    """The kernel's deliberate deviation: the exact derivative against BaseBinaryEdge's central difference (delta = 1e-9).  The
    difference is evaluated at 60 digits, where only its truncation error remains; that error is recorded in the fixture, and the
    fp64 analytic Jacobian may differ from it by that plus its own recorded drift (triangle inequality).  No edge is excluded:
    the fixture keeps every error 1e-6 away from the wrap, 500 times further than a step of delta moves it."""
    g = H.load_graph(Z)
    J0, J1, _ = H.producers(H.FP64, g)
    N0, N1 = BE.numeric_edges(H.MP, g["poses"], g["points"], g["bp"], g["bl"], g["zb"])
    N0, N1 = (np.array([[float(v) for v in row] for row in N]) for N in (N0, N1))
    fig = max(np.abs(J0 - N0).max(), np.abs(J1 - N1).max())
    bound = float(Z["numeric_noise"]) + float(Z["drift"][-1, 1])
    print("analytic vs central difference", fig, "truncation", float(Z["numeric_noise"]), "bound", bound)
    assert float(Z["numeric_noise"]) < 1e-12       # (O(delta^2) on entries of order 1)
    assert fig <= bound
    # in fp64 the same difference carries rounding noise of eps pi / delta: only its order is checked
    F0, F1 = BE.numeric_edges(H.FP64, g["poses"], g["points"], g["bp"][:40], g["bl"][:40], g["zb"][:40])
    assert max(np.abs(J0[:40] - np.array(F0)).max(), np.abs(J1[:40] - np.array(F1)).max()) < 1e-5


def test_central_difference_across_the_wrap_is_wrong_by_pi_over_delta():
    """What the deviation avoids: an error within delta of +-pi makes the reference's difference jump by 2 pi / (2 delta)."""
    X, L = np.array([0.2, -0.1, 0.4]), np.array([3.0, 2.0])
    pred = float(BE.bearing_error(H.FP64, X, L, 0.0))                   # e(z = 0) = -angle
    z = -pred + np.pi - 1e-10                                          # e = pi - 1e-10
    N0, _ = BE.numeric_jacobians(H.FP64, X, L, z)
    A, _ = BE.bearing_jacobians(H.FP64, X, L)
    assert abs(A[2] - 1.0) == 0 and abs(abs(N0[2] - A[2]) - np.pi / 1e-9) < 1e-3 * np.pi / 1e-9


@pytest.mark.parametrize("with_xy", [False, True])
def test_g2o_round_trip(with_xy, tmp_path):
    g = S.make_bearing_slam(12, 10, with_xy=with_xy, seed=3)
    path = os.path.join(str(tmp_path), "bearing.g2o")
    g2o_io.write_g2o_bearing(path, g)
    text = open(path).read()
    assert text.count("EDGE_BEARING_SE2_XY") == g["B"] and (text.count("EDGE_SE2_XY") > 0) == with_xy
    rd = g2o_io.read_g2o(path)
    assert len(rd["br_vp"]) == g["B"] and len(rd["lm_vp"]) == g["M"]
    p = g2o_io.bearing_problem(rd)
    for k in ("bp", "bl", "zb", "omega_b", "vp", "vl", "zl", "omega_l", "poses", "points", "hidx", "pt_hidx", "Z", "omega", "vi", "vj"):
        assert np.array_equal(np.asarray(p[k]), np.asarray(g[k])), k
    assert (p["nP"], p["nL"], p["M"], p["B"]) == (g["nP"], g["nL"], g["M"], g["B"])
    e0 = BE.bearing_edges(H.FP64, g["poses"], g["points"], g["bp"], g["bl"], g["zb"], jac=False)
    e1 = BE.bearing_edges(H.FP64, p["poses"], p["points"], p["bp"], p["bl"], p["zb"], jac=False)
    assert np.array_equal(e0, e1)


def test_files_without_the_tag_parse_as_before(tmp_path):
    g = S.make_landmark_slam("se2", 12, 10)
    path = os.path.join(str(tmp_path), "xy.g2o")
    g2o_io.write_g2o_landmarks(path, g)
    rd = g2o_io.read_g2o(path)
    assert not any(k.startswith("br_") for k in rd)
    assert sorted(rd) == sorted(["kind", "ids", "estimates", "vi", "vj", "meas", "info", "fixed", "point_ids", "points", "lm_vp", "lm_vl",
                                 "lm_meas", "lm_info", "lm_param", "offsets", "fixed_points"])
    with pytest.raises(ValueError):
        g2o_io.bearing_problem(rd)


@pytest.mark.parametrize("with_xy", [False, True])
def test_make_bearing_slam(with_xy):
    base = S.make_landmark_slam("se2", 40, 30, seed=4)
    a, b = S.make_bearing_slam(40, 30, with_xy=with_xy, seed=4), S.make_bearing_slam(40, 30, with_xy=with_xy, seed=4)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert len(a["bp"]) == len(a["bl"]) == len(a["zb"]) == len(a["omega_b"]) == a["B"] > 0
    for poses, points in ((a["poses_true"], a["points_true"]), (a["poses"], a["points"])):
        d = points[a["bl"]] - poses[a["bp"], :2]
        assert np.hypot(d[:, 0], d[:, 1]).min() >= 0.5
    # the measurements are the truth's bearings up to the stated noise
    e = BE.bearing_edges(H.FP64, a["poses_true"], a["points_true"], a["bp"], a["bl"], a["zb"], jac=False)
    assert 0 < np.abs(e).max() < 0.1
    if with_xy:
        for k in ("vp", "vl", "zl", "omega_l", "points", "pt_hidx", "poses", "Z"):
            assert np.array_equal(a[k], base[k]), k
        return
    assert a["M"] == 0 and len(a["vp"]) == 0 and a["L"] <= base["L"] and a["nL"] == (a["pt_hidx"] >= 0).sum()
    assert sorted(a["pt_hidx"][a["pt_hidx"] >= 0]) == list(range(a["nP"], a["nP"] + a["nL"]))
    for j in range(a["L"]):
        idx = np.nonzero(a["bl"] == j)[0]
        assert len(idx) >= 2
        for poses, points in ((a["poses_true"], a["points_true"]), (a["poses"], a["points"])):
            d = points[j] - poses[a["bp"][idx], :2]
            w = np.arctan2(d[:, 1], d[:, 0]) % np.pi
            diff = np.abs(w[:, None] - w[None, :])
            assert np.minimum(diff, np.pi - diff).max() >= 0.2
    # a parallax floor that some landmarks cannot meet: they are dropped with their observations, the table is renumbered
    c = S.make_bearing_slam(40, 30, seed=4, min_parallax=1.2)
    assert 0 < c["L"] < a["L"] and c["bl"].max() == c["L"] - 1 and c["points"].shape == (c["L"], 2) and c["B"] < a["B"]
    assert sorted(c["pt_hidx"]) == list(range(c["nP"], c["nP"] + c["L"]))


@pytest.mark.parametrize("mode", H.MODES)
def test_cpu_lm_over_the_oracle_descends(mode):
    g = H.lm_graph(mode)
    r = H.oracle_lm_run(g, lambda_init=H.LM_LAMBDA[mode])
    key = "bearing" if mode == "bearing-only" else "mixed"
    print(mode, "chi2", r["chis"], "trials", r["trials"])
    assert r["done"] == H.LM_ITERATIONS and r["trials"] == Z["lm_%s_trials" % key].tolist() and max(r["trials"]) > 1
    assert np.all(np.diff(r["chis"]) < 0)
    assert np.abs(r["chis"] - Z["lm_%s_chis" % key]).max() <= 1e-9 * Z["lm_%s_chis" % key].max()
    assert H.pose_error(g, r["poses"]) < H.pose_error(g, g["poses"])


def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(ROOT, "include", "g2ohip.h")).read()
    assert "int g2ohip_pg_set_bearing_edges(g2ohip_solver* s, int set," in header
    for word in ("DELIBERATE DEVIATION", "EdgeSE2PointXYOffset", "EdgeSE2PointXYCalib", "more than one bearing set per handle"):
        assert word in header
    lib = os.environ.get("G2OHIP_LIB") or os.path.join(ROOT, "openslam_g2o_amd", "lib", "libg2ohip.so")
    if not os.path.exists(lib):
        pytest.fail("the library is not built: %s" % lib)
    assert hasattr(ctypes.CDLL(lib), "g2ohip_pg_set_bearing_edges")
    from openslam_g2o_amd import capi
    assert hasattr(capi.HipBlockSolver, "pgSetBearingEdges") and capi.HipBlockSolver.bearing_set is None
    hpp = open(os.path.join(ROOT, "openslam_g2o_amd", "cpp", "hip_block_solver.hpp")).read()
    assert "pgSetBearingEdges" in hpp


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


def _recorded(monkeypatch, prob, **kw):
    from openslam_g2o_amd import capi
    monkeypatch.setattr(capi, "HipBlockSolver", _Recorder)
    s, _ = lm.setup_device_landmark_slam(prob, **kw)
    return s


def test_setup_without_bearing_keys_is_unchanged(monkeypatch):
    """As far as it can be asserted without a device: for a prob without bearing keys the calls made on the solver are the ones made
    before the bearing slot existed -- two edge sets, no pgSetBearingEdges, one robust kernel, landmark_sets = (0, 1)."""
    from openslam_g2o_amd import capi
    s = _recorded(monkeypatch, S.make_landmark_slam("se2", 12, 10), huber_delta=1.5)
    names = [c[0] for c in s.calls]
    assert names == ["init", "addEdgeSet", "addEdgeSet", "buildStructure", "pgSetEdges", "pgSetEstimates", "pgSetLandmarkEdges",
                     "pgSetLandmarkEstimates", "setRobustKernel"]
    assert s.calls[-1] == ("setRobustKernel", 1, capi.KERNEL_HUBER, 1.5) and s.landmark_sets == (0, 1)
    assert "bearing_set" not in s.__dict__
    # with the keys: the bearing set is bound, beside the type-3 set or alone, and carries the kernel too
    m = _recorded(monkeypatch, S.make_bearing_slam(12, 10, with_xy=True), huber_delta=1.5)
    assert [c[0] for c in m.calls] == ["init", "addEdgeSet", "addEdgeSet", "addEdgeSet", "buildStructure", "pgSetEdges", "pgSetEstimates",
                                       "pgSetLandmarkEdges", "pgSetBearingEdges", "pgSetLandmarkEstimates", "setRobustKernel", "setRobustKernel"]
    assert m.calls[3][1] == 1 and m.landmark_sets == (0, 1)
    b = _recorded(monkeypatch, S.make_bearing_slam(12, 10), huber_delta=1.5)
    assert [c[0] for c in b.calls] == ["init", "addEdgeSet", "addEdgeSet", "buildStructure", "pgSetEdges", "pgSetEstimates",
                                       "pgSetBearingEdges", "pgSetLandmarkEstimates", "setRobustKernel"]
    assert b.calls[2][1] == 1 and b.landmark_sets == (0, None) and b.calls[-1][1] == 1
