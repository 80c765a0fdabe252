"""CPU: the laser self-calibration edge (EdgeSE2SensorCalib = type 21) on the host side -- the restatement of
openslam_g2o_amd/sensor_calib.py in fp64 against its 60-digit evaluation (tests/golden/sensor_calib_edges.npz), the exact Jacobian
against a 60-digit central difference and against the reference's delta = 1e-9 difference, the g2o_io round trip, the rig
generator and its observability, a CPU LM run over the oracle's three-vertex edges, the C header and the built library, and the
unchanged setup without calibration edges."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io, lm, sensor_calib as SC, synthetic as S
from tests import calib_helpers as H

Z = np.load(H.GOLDEN)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_fp64_within_recorded_drift():
    g = H.load_graph(Z)
    Ji, Jj, Jl, err = H.producers(H.FP64, g)
    de = np.abs(err - Z["err"]).max(axis=1)
    dJ = np.maximum.reduce([np.abs(a - Z[k]).max(axis=1) for a, k in ((Ji, "Ji"), (Jj, "Jj"), (Jl, "Jl"))])
    for n, (be, bJ) in zip(H.EDGE_COUNTS, Z["drift"]):
        print(n, "fp64 vs 60 digits (err, J)", de[:n].max(), dJ[:n].max(), "recorded", be, bJ)
        assert de[:n].max() <= be and dJ[:n].max() <= bJ
    assert Z["drift"].max() < 1e-13 and Z["drift"].min() > 0
    moved = H.oplus(g, g["poses"], Z["moved_x"])
    assert np.array_equal(moved, Z["moved_poses"])


def test_fixture_shape():
    g = H.load_graph(Z)
    assert len(g["ci"]) == 700 and len(g["poses"]) == 8 and list(g["hidx"]) == [-1, 0, 1, 2, 3, 4, 5, 6] and len(g["vi"]) == 5
    e = Z["err"][:8, 2]
    assert (np.pi - np.abs(e) < 1e-3).all() and (e > 0).sum() == 4 and (e < 0).sum() == 4       # within 1e-3 of +pi and of -pi
    sp = H.take_edges(g, slice(0, H.N_SPECIAL))
    same = g["poses"][sp["ci"], 2] == g["poses"][sp["cj"], 2]
    assert same.sum() >= 4 and np.abs(Z["Jl"][:H.N_SPECIAL][same][:, [0, 1, 3, 4]]).max() == 0.0   # th1 == th2: d e_t / d tl vanishes
    assert np.abs(Z["Jl"][:H.N_SPECIAL][~same][:, [0, 1, 3, 4]]).max(axis=1).min() > 1e-3
    assert (sp["cl"] == H.LEVER_ROW).sum() >= 8 and np.hypot(*g["poses"][H.LEVER_ROW][:2]) > 40    # a large lever arm
    fixed = g["ci"] == 0
    assert fixed.any() and (g["cj"] == 0).any()
    assert not Z["Ji"][fixed].any() and not Z["Jj"][g["cj"] == 0].any() and Z["Ji"][~fixed].any(axis=1).all()   # fixed blocks: zeros
    assert (Z["Jl"][:, 8] == 0).all() and (Z["Jl"][:, 2] == 0).all()                                # d e_th / d (tl, thl) = 0


def _special():
    g = H.take_edges(H.load_graph(Z), slice(0, H.N_SPECIAL))
    return g, H.producers(H.FP64, g, fixed_zero=False)


def test_exact_jacobian_against_60_digit_central_difference():
    """The issue's own table is judged here: the exact derivative in fp64 against the central difference of the 60-digit error with
    step 1e-25 (truncation ~1e-50, far below fp64 rounding).  The fixture records what rounding that difference to fp64 leaves
    against the exact Jacobian at 60 digits; the fp64 Jacobian may differ from it by that plus its own recorded drift (triangle
    inequality, the margin of tests/test_offset_edges_host.py).  The difference is also recomputed."""
    g, (Ji, Jj, Jl, _) = _special()
    cd = SC.numeric_edges(H.MP, g["poses"], g["ci"][:6], g["cj"][:6], g["cl"][:6], g["cmeas"][:6], delta=H.MP.num(10) ** -25)
    for N, key in zip(cd, ("cd60_Ji", "cd60_Jj", "cd60_Jl")):
        assert np.array_equal(np.array([[float(v) for v in row] for row in N]), Z[key][:6])
    fig = max(np.abs(J - Z[k]).max() for J, k in ((Ji, "cd60_Ji"), (Jj, "cd60_Jj"), (Jl, "cd60_Jl")))
    bound = float(Z["cd60_gap"]) + float(Z["drift"][-1, 1])
    print("exact vs 60-digit central difference", fig, "rounding of the difference", float(Z["cd60_gap"]), "bound", bound)
    assert float(Z["cd60_gap"]) < 1e-13
    assert fig <= bound


def test_exact_jacobian_against_the_references_difference():
    """The kernel's deliberate deviation: the exact derivative against BaseMultiEdge's central difference (delta = 1e-9).  The
    difference is evaluated at 60 digits, where only its truncation error remains; that error is recorded in the fixture, and the
    fp64 exact Jacobian may differ from it by that plus its own recorded drift."""
    g, (Ji, Jj, Jl, _) = _special()
    N = SC.numeric_edges(H.MP, g["poses"], g["ci"], g["cj"], g["cl"], g["cmeas"])
    N = [np.array([[float(v) for v in row] for row in A]) for A in N]
    fig = max(np.abs(J - A).max() for J, A in zip((Ji, Jj, Jl), N))
    bound = float(Z["numeric_noise"]) + float(Z["drift"][-1, 1])
    print("exact vs the reference's central difference", fig, "truncation", float(Z["numeric_noise"]), "bound", bound)
    assert float(Z["numeric_noise"]) < 1e-12       # (O(delta^2) on entries of order 1 ... 100)
    assert fig <= bound
    # in fp64 the same difference carries rounding noise of eps |e| / delta: only its order is checked
    F = SC.numeric_edges(H.FP64, g["poses"], g["ci"][:20], g["cj"][:20], g["cl"][:20], g["cmeas"][:20])
    assert max(np.abs(J[:20] - np.array(A)).max() for J, A in zip((Ji, Jj, Jl), F)) < 1e-4


def test_g2o_round_trip(tmp_path):
    g = S.make_calib_rig(9, loops=4, seed=3)
    path = os.path.join(str(tmp_path), "rig.g2o")
    ids = np.arange(10) * 2 + 10
    g2o_io.write_g2o_calib(path, g, ids=ids)
    text = open(path).read()
    assert text.count("EDGE_SE2_CALIB ") == 12 and text.count("VERTEX_SE2 ") == 10 and "FIX 10\n" in text
    rd = g2o_io.read_g2o(path)
    p = g2o_io.calib_problem(rd)
    for k in ("poses", "Z", "omega", "cmeas", "cinfo"):
        assert np.array_equal(np.asarray(p[k]).reshape(-1), np.asarray(g[k]).reshape(-1)), k
    for k in ("ci", "cj", "cl", "vi", "vj", "hidx"):
        assert np.array_equal(p[k], g[k]), k
    assert p["nP"] == g["nP"] == 9 and (p["cl"] == 9).all()
    pf = g2o_io.calib_problem(rd, fixed=[0, 9])
    assert pf["nP"] == 8 and pf["hidx"][9] == -1


def test_files_without_the_tag_parse_as_before(tmp_path):
    g = S.make_offset_rig("se2", 9, 3, 2, seed=3)
    path = os.path.join(str(tmp_path), "rig.g2o")
    g2o_io.write_g2o_offset(path, g)
    rd = g2o_io.read_g2o(path)
    assert not any(k.startswith("cal_") for k in rd)
    assert sorted(rd) == sorted(["kind", "ids", "estimates", "vi", "vj", "meas", "info", "fixed", "offsets2", "off_vi", "off_vj", "off_from",
                                 "off_to", "off_meas", "off_info", "off_kind", "offsets"])
    with pytest.raises(ValueError):
        g2o_io.calib_problem(rd)


def _dense_gauss_newton(g):
    o, m = H.oracle_calib(g)
    H.feed_oracle(g, o, m)
    o.build_system()
    return o, o.dense_full()


def test_make_calib_rig_shape_and_observability():
    a, b, c = S.make_calib_rig(40, seed=5), S.make_calib_rig(40, seed=5), S.make_calib_rig(40, seed=6)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert not np.array_equal(a["cmeas"], c["cmeas"])
    assert a["n"] == 41 and a["nP"] == 40 and a["offset_row"] == 40 and len(a["vi"]) == 39 and len(a["ci"]) == 60
    assert (a["cl"] == 40).all() and a["hidx"][0] == -1 and a["hidx"][40] == 39 and (a["hidx"][1:40] == np.arange(39)).all()
    assert (a["cj"] - a["ci"]).max() > 1 and ((a["cj"] - a["ci"]) == 1).sum() == 39           # consecutive poses and loop closures
    assert np.array_equal(a["poses"][40], np.zeros(3)) and np.array_equal(a["poses_true"][40], [0.3, 0.1, 0.2])
    th = a["poses_true"][:40, 2]
    turn = np.abs((np.diff(th) + np.pi) % (2 * np.pi) - np.pi)
    assert turn.min() > 0.05 and turn.sum() > 2 * np.pi                                       # the trajectory keeps turning
    e = SC.calib_edges(H.FP64, a["poses_true"], a["ci"], a["cj"], a["cl"], a["cmeas"], jac=False)
    assert 0 < np.abs(e).max() < 0.1                                                          # the truth's scan matches up to the noise
    # observability: the dense Gauss-Newton matrix of the free graph, pose 0 fixed, is positive definite -- the offset included
    _, Hm = _dense_gauss_newton(a)
    w = np.linalg.eigvalsh(Hm)
    print("Gauss-Newton eigenvalues", w.min(), w.max())
    assert Hm.shape == (120, 120) and w.min() > 1e-6 * w.max()
    # the offset couples to every pose: a dense block row
    assert all(np.abs(Hm[117:120, 3 * k:3 * k + 3]).max() > 0 for k in range(39))
    f = S.make_calib_rig(40, seed=5, fix_offset=True)
    assert f["nP"] == 39 and f["hidx"][40] == -1 and np.array_equal(f["poses"][40], f["offset_true"])
    wr = S.make_calib_rig(40, seed=5, wrap_every=6)
    ew = SC.calib_edges(H.FP64, wr["poses_true"], wr["ci"], wr["cj"], wr["cl"], wr["cmeas"], jac=False)[::6, 2]
    assert (np.pi - np.abs(ew) < 0.05).all() and (ew > 0).any() and (ew < 0).any()            # both sides of +-pi


def test_cpu_lm_run_descends_and_recovers_the_offset():
    g = H.lm_graph()
    r = H.oracle_lm_run(g)
    e0, e1 = H.offset_error(g, g["poses"]), H.offset_error(g, r["poses"])
    print("chi2", r["chis"], "offset error", e0, "->", e1)
    assert r["done"] == H.LM_ITERATIONS and (np.diff(r["chis"]) <= 0).all() and r["chis"][-1] < 0.8 * r["chis"][0]
    assert np.array_equal(r["chis"], Z["lm_chis"]) and r["trials"] == Z["lm_trials"].tolist()
    assert e1[0] <= H.LM_ARGS["noise"][0] and e1[1] <= H.LM_ARGS["noise"][1] and e0[0] > 0.3


def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(ROOT, "include", "g2ohip.h")).read()
    assert "int g2ohip_pg_set_sensor_calib_edges(g2ohip_solver* s, int set_ij, int set_il, int set_jl," in header
    for word in ("DELIBERATE DEVIATION", "EdgeSE2OdomDifferentialCalib", "VertexOdomDifferentialParams", "more than one calibration",
                 "sharded solves", "the g2o plugin adapter", "base_multi_edge.hpp:63-116", "edge_se2_sensor_calib.h"):
        assert word in header, word
    lib = os.environ.get("G2OHIP_LIB") or os.path.join(ROOT, "openslam_g2o_amd", "lib", "libg2ohip.so")
    if not os.path.exists(lib):
        pytest.fail("the library is not built: %s" % lib)
    assert hasattr(ctypes.CDLL(lib), "g2ohip_pg_set_sensor_calib_edges")
    from openslam_g2o_amd import capi
    assert hasattr(capi.HipBlockSolver, "pgSetSensorCalibEdges") and "g2ohip_pg_set_sensor_calib_edges" in capi.EXPORTS
    hpp = open(os.path.join(ROOT, "openslam_g2o_amd", "cpp", "hip_block_solver.hpp")).read()
    assert "pgSetSensorCalibEdges" in hpp
    src = os.path.join(ROOT, "openslam_g2o_amd", "csrc")
    assert '#include "pg_calib.inc"' in open(os.path.join(src, "block_solver.hip")).read()
    inc = open(os.path.join(src, "pg_calib.inc")).read()
    assert "pg_offset_se2_mul" in inc and "pg_offset_se2_inverse" in inc and "scratch 0 bytes" in inc


def test_setup_without_calib_edges_is_unchanged():
    """calib_edges and huber_delta are keyword arguments behind the existing ones, default None / 0: an existing call binds what it
    bound before, and the new branches are not entered."""
    sig = inspect.signature(lm.setup_device_pose_graph)
    names = list(sig.parameters)
    assert names[:14] == ["edge_type", "estimates", "hidx", "num_free", "vi", "vj", "meas", "info", "landmark_dim", "device", "priors",
                          "fix_scale", "options", "offset_edges"]
    assert names[14:] == ["calib_edges", "huber_delta"]
    assert sig.parameters["calib_edges"].default is None and sig.parameters["huber_delta"].default == 0.0
    from openslam_g2o_amd import capi
    assert capi.HipBlockSolver.calib_sets is None
