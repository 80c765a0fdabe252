"""CPU: the sensor-offset pose-pose edges (EdgeSE2Offset = type 18, EdgeSE3Offset = type 19) on the host side -- the restatement of
openslam_g2o_amd/offset_edges.py in fp64 against its 60-digit evaluation (tests/golden/offset_edges.npz), the type-18 analytic
Jacobian against the reference's central difference, type 19 with identity offsets against the oracle's EdgeSE3, the g2o_io round
trip, the C header and the built library, the rig generator."""
import ctypes
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io, offset_edges as OE, synthetic as S
from tests import offset_helpers as H

Z = np.load(H.GOLDEN)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


@pytest.mark.parametrize("kind,etype", H.KINDS)
def test_restatement_fp64_within_recorded_drift(kind, etype):
    g = H.load_graph(Z, kind)
    J0, J1, err = H.producers(H.FP64, g)
    de = np.abs(err - Z[kind + "_err"])
    dJ = np.maximum(np.abs(J0 - Z[kind + "_J0"]).max(axis=1), np.abs(J1 - Z[kind + "_J1"]).max(axis=1))
    for n, (be, bJ) in zip(H.EDGE_COUNTS, Z[kind + "_drift"]):
        print(kind, n, "fp64 vs 60 digits (err, J)", de[:n].max(), dJ[:n].max(), "recorded", be, bJ)
        assert de[:n].max() <= be and dJ[:n].max() <= bJ
    assert Z[kind + "_drift"].max() < 1e-13
    moved = H.oplus(g, g["poses"], Z[kind + "_moved_x"])
    assert np.array_equal(moved, Z[kind + "_moved_poses"])


def test_fixture_shape():
    for kind, _ in H.KINDS:
        g = H.load_graph(Z, kind)
        assert len(g["oi"]) == 300 and len(g["poses"]) == 4 and list(g["hidx"]) == [-1, 0, 1, 2] and len(g["vi"]) == 3 and len(g["offsets"]) == 3
        pairs = set(zip(g["oi"].tolist(), g["oj"].tolist()))
        assert (1, 2) in pairs and (2, 1) in pairs and any(0 in p for p in pairs)
        assert (g["opf"] != g["opt"]).any() and (g["opf"] == g["opt"]).any()
        assert set(g["opf"].tolist()) == set(g["opt"].tolist()) == {0, 1, 2}
    P = Z["se3_offsets"]
    assert np.array_equal(P[0], IDENTITY) and P[1][:9].reshape(3, 3).trace() < 1.0       # identity; rotation angle above 90 degrees
    assert np.array_equal(Z["se2_offsets"][0], np.zeros(3)) and abs(Z["se2_offsets"][1][2]) > np.pi / 2


def test_se2_analytic_jacobian_against_central_difference():
    """The kernel's deliberate deviation: the exact derivative against BaseBinaryEdge's central difference (delta = 1e-9).  The
    difference is evaluated at 60 digits, where only its truncation error remains; that error is recorded in the fixture, and
    the fp64 analytic Jacobian may differ from it by that plus its own recorded drift (triangle inequality)."""
    g = H.load_graph(Z, "se2")
    J0, J1, _ = H.producers(H.FP64, g)
    N0, N1 = OE.numeric_edges(H.MP, g["poses"], g["oi"], g["oj"], g["opf"], g["opt"], g["omeas"], g["offsets"])
    N0, N1 = (np.array([[float(v) for v in row] for row in N]) for N in (N0, N1))
    fig = max(np.abs(J0 - N0).max(), np.abs(J1 - N1).max())
    bound = float(Z["se2_numeric_noise"]) + float(Z["se2_drift"][-1, 1])
    print("analytic vs central difference", fig, "truncation", float(Z["se2_numeric_noise"]), "bound", bound)
    assert float(Z["se2_numeric_noise"]) < 1e-12       # (O(delta^2) on entries of order 1 ... 10)
    assert fig <= bound
    # in fp64 the same difference carries rounding noise of eps |e| / delta: only its order is checked
    F0, F1 = OE.numeric_edges(H.FP64, g["poses"], g["oi"][:20], g["oj"][:20], g["opf"][:20], g["opt"][:20], g["omeas"][:20], g["offsets"])
    assert max(np.abs(J0[:20] - np.array(F0)).max(), np.abs(J1[:20] - np.array(F1)).max()) < 1e-5


def test_se3_identity_offsets_equal_the_oracles_edge_se3():
    from oracle import oracle as O
    g = H.load_graph(Z, "se3")
    ident = np.tile(IDENTITY, (3, 1))
    J0, J1, err = OE.offset_edges(H.FP64, 19, g["poses"], g["oi"], g["oj"], g["opf"], g["opt"], g["omeas"], ident)
    A0, A1, e0 = O.se3_edges(g["poses"], g["oi"], g["oj"], g["omeas"])
    be, bJ = Z["se3_drift"][-1]
    fig = (np.abs(err - e0).max(), max(np.abs(J0 - A0).max(), np.abs(J1 - A1).max()))
    print("identity offsets vs oracle EdgeSE3 (err, J)", fig, "drift", be, bJ)
    # two fp64 evaluations of one function, each within the drift of the 60-digit value
    assert fig[0] <= 2 * be and fig[1] <= 2 * bJ


@pytest.mark.parametrize("kind,etype", H.KINDS)
def test_g2o_round_trip(kind, etype, tmp_path):
    g = S.make_offset_rig(kind, 9, 3, 2, seed=3)
    path = os.path.join(str(tmp_path), "rig.g2o")
    ids, param_ids = np.arange(9) * 2 + 10, np.array([7, 2, 9])
    g2o_io.write_g2o_offset(path, g, ids=ids, param_ids=param_ids)
    rd = g2o_io.read_g2o(path)
    assert rd["off_kind"] == kind and list(rd["off_from"]) == [int(param_ids[a]) for a in g["opf"]]
    p = g2o_io.offset_problem(rd)
    row_of = {0: 1, 1: 0, 2: 2}                                   # ids 7, 2, 9 -> rows by ascending id: 2, 7, 9
    assert list(p["param_ids"]) == [2, 7, 9]
    assert np.array_equal(p["opf"], [row_of[a] for a in g["opf"]]) and np.array_equal(p["opt"], [row_of[a] for a in g["opt"]])
    tol = 0.0 if kind == "se2" else 2e-15                         # (SE3: the rotation goes through a quaternion and back)
    for k in ("poses", "Z", "omega", "omeas", "oinfo"):
        assert np.abs(np.asarray(p[k]).reshape(-1) - np.asarray(g[k]).reshape(-1)).max() <= tol, k
    assert np.abs(p["offsets"] - g["offsets"][[1, 0, 2]]).max() <= tol
    for k in ("oi", "oj", "vi", "vj", "hidx"):
        assert np.array_equal(p[k], g[k])
    assert p["offset_type"] == etype and p["nP"] == 8
    # the same errors from the file as from the generator
    e0 = OE.offset_edges(H.FP64, etype, g["poses"], g["oi"], g["oj"], g["opf"], g["opt"], g["omeas"], g["offsets"], jac=False)
    e1 = OE.offset_edges(H.FP64, etype, p["poses"], p["oi"], p["oj"], p["opf"], p["opt"], p["omeas"], p["offsets"], jac=False)
    assert np.abs(e0 - e1).max() < 1e-13
    text = open(path).read()
    if kind == "se3":                                             # the measurement quaternion is normalised on read
        lines = text.splitlines()
        k = next(i for i, l in enumerate(lines) if l.startswith("EDGE_SE3_OFFSET"))
        t = lines[k].split()
        t[8:12] = ["%.17g" % (3.0 * float(v)) for v in t[8:12]]
        lines[k] = " ".join(t)
        scaled = os.path.join(str(tmp_path), "scaled.g2o")
        open(scaled, "w").write("\n".join(lines) + "\n")
        rs = g2o_io.read_g2o(scaled)
        assert abs(np.linalg.norm(rs["off_meas"][0, 3:]) - 1.0) < 1e-15 and np.abs(rs["off_meas"] - rd["off_meas"]).max() < 1e-15
    # an edge that names a parameter id the file does not define
    tag = "PARAMS_SE3OFFSET 9 " if kind == "se3" else "PARAMS_SE2OFFSET 9 "
    broken = os.path.join(str(tmp_path), "broken.g2o")
    open(broken, "w").write("\n".join(l for l in text.splitlines() if not l.startswith(tag)) + "\n")
    with pytest.raises(ValueError):
        g2o_io.read_g2o(broken)


def test_files_without_the_new_tags_parse_as_before(tmp_path):
    g = S.make_gicp(3, 5, seed=1)
    path = os.path.join(str(tmp_path), "scans.g2o")
    g2o_io.write_g2o_gicp(path, g)
    rd = g2o_io.read_g2o(path)
    assert not any(k.startswith("off_") or k == "offsets2" for k in rd)
    with pytest.raises(ValueError):
        g2o_io.offset_problem(rd)


def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(ROOT, "include", "g2ohip.h")).read()
    assert "int g2ohip_pg_set_offset_edges(g2ohip_solver* s, int set, int type," in header
    for word in ("DELIBERATE DEVIATION", "EdgeSE2PointXYOffset", "more than one offset set per handle"):
        assert word in header
    lib = os.environ.get("G2OHIP_LIB") or os.path.join(ROOT, "openslam_g2o_amd", "lib", "libg2ohip.so")
    if not os.path.exists(lib):
        pytest.fail("the library is not built: %s" % lib)
    assert hasattr(ctypes.CDLL(lib), "g2ohip_pg_set_offset_edges")
    from openslam_g2o_amd import capi
    assert hasattr(capi.HipBlockSolver, "pgSetOffsetEdges")
    hpp = open(os.path.join(ROOT, "openslam_g2o_amd", "cpp", "hip_block_solver.hpp")).read()
    assert "pgSetOffsetEdges" in hpp


@pytest.mark.parametrize("kind,etype", H.KINDS)
def test_make_offset_rig(kind, etype):
    a, b, c = S.make_offset_rig(kind, 12, 3, 3, seed=5), S.make_offset_rig(kind, 12, 3, 3, seed=5), S.make_offset_rig(kind, 12, 3, 3, seed=6)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert not np.array_equal(a["omeas"], c["omeas"])
    assert a["offset_type"] == etype and len(a["oi"]) == 36 and len(a["vi"]) == 11 and a["offsets"].shape == (3, H.STRIDE[kind])
    assert len({tuple(np.round(r, 12)) for r in a["offsets"]}) == 3                     # distinct mounted frames
    trivial = np.zeros(3) if kind == "se2" else IDENTITY
    assert all(np.abs(r - trivial).max() > 0.05 for r in a["offsets"])                  # ... none of them the body frame
    assert (a["opf"] != a["opt"]).any()
    pairs = list(zip(a["oi"].tolist(), a["oj"].tolist()))
    assert any((j, i) in pairs for i, j in pairs)                                       # a pair in both orders
    assert a["hidx"][0] == -1 and any(j == 0 for _, j in pairs) and any(i == 0 for i, _ in pairs)   # edges to and from the fixed pose
    assert (a["oj"] - a["oi"]).max() > 1                                                # poses k and k + m, m > 1
    # the measurements are the truth's relative sensor poses up to the stated noise
    e = OE.offset_edges(H.FP64, etype, a["poses_true"], a["oi"], a["oj"], a["opf"], a["opt"], a["omeas"], a["offsets"], jac=False)
    assert 0 < np.abs(e).max() < 0.1
