"""CPU: the odometry self-calibration edge (EdgeSE2OdomDifferentialCalib = type 22) on the host side -- the restatement of
openslam_g2o_amd/odom_calib.py in fp64 against its 60-digit evaluation (tests/golden/odom_calib_edges.npz), the exact Jacobian of
both branches against the reference's delta = 1e-9 central difference at 60 digits, OdomConvert's two conversions, the g2o_io round
trip, the rig generator (its defaults pinned to the arrays of the commit before this edge), the C header and the built library."""
import ctypes
import hashlib
import inspect
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io, lm, odom_calib as OC, synthetic as S
from tests import odom_calib_helpers as H

Z = np.load(H.GOLDEN)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JKEYS = ("err", "Ji", "Jj", "Jp")


def test_restatement_fp64_within_recorded_drift():
    g = H.load_graph(Z)
    for k in H.GRAPH_KEYS:
        assert np.array_equal(H.base_graph()[k], Z[k]), k                # (the fixture is the generator's graph)
    Ji, Jj, Jp, err = H.producers(H.FP64, g)
    d = [np.abs(a - Z[k]).max(axis=1) for a, k in zip((err, Ji, Jj, Jp), JKEYS)]
    for n, row in zip(H.EDGE_COUNTS, Z["drift"]):
        fig = [a[:n].max() for a in d]
        print(n, "fp64 vs 60 digits (err, Ji, Jj, Jp)", fig, "recorded", row)
        assert all(f <= b for f, b in zip(fig, row))
    assert Z["drift"].min() > 0                                          # (the generator's rule: no array is exact by accident)
    assert Z["drift"][:, :3].max() < 1e-13 and Z["drift"][:, 3].max() < 1e-15 * np.abs(Z["Jp"]).max() * 4   # rounding level of entries <= 152
    assert np.array_equal(H.oplus(g, g["poses"], Z["moved_x"]), Z["moved_poses"])


def test_fixture_shape():
    g = H.load_graph(Z)
    assert len(g["oi"]) == 700 and len(g["poses"]) == 8 and list(g["hidx"]) == [-1, 0, 1, 2, 3, 4, 5, 6] and len(g["vi"]) == 0
    p = g["poses"][[H.PARAM_ROW, H.PARAM_ROW_2]]
    assert (np.abs(p - 1.0) > 0.05).all() and (p[:, 0] != p[:, 1]).all()                       # away from (1, 1, 1), k_l != k_r
    D, margin = OC.branch_margin(g["poses"], g["op"], g["omeas"])
    assert np.array_equal(D, Z["absD"]) and (margin > 1e-8).all()                              # no edge near the branch point: none left out
    straight = ~Z["turning"]
    assert 120 <= straight.sum() <= 160 and D[straight].max() < 1e-8 and D[~straight].min() >= 1e-2 * (1 - 1e-12)
    e = Z["err"][:8, 2]
    assert (np.pi - np.abs(e) < 1e-3).all() and (e > 0).sum() == 4 and (e < 0).sum() == 4      # within 1e-3 of +pi and of -pi
    # every tenth edge a gross outlier.  The six poses lie on no common arc, so the translational error of EVERY edge is of the
    # size of the graph; what tells the kinds apart is the angle: an ordinary edge turns by th2 - th1 plus N(0, 0.05), so its angle
    # error stays below 5 sigma = 0.25, an outlier turns by an arbitrary angle of (-3, 3) (the chance of landing within 0.25: 8 %)
    k = np.arange(700)
    ordinary = (k % 10 != 9) & (k % 5 != 2) & (k >= 8)
    eth = np.abs(Z["err"][:, 2])
    print("angle error: ordinary max", eth[ordinary].max(), "outliers beyond 0.25:", int((eth[9::10] > 0.25).sum()), "of 70")
    assert eth[ordinary].max() < 0.25 and (eth[9::10] > 0.25).sum() >= 63 and np.median(eth[9::10]) > 1.0
    fixed_i, fixed_j = g["oi"] == 0, g["oj"] == 0
    assert fixed_i.any() and fixed_j.any() and not Z["Ji"][fixed_i].any() and not Z["Jj"][fixed_j].any()
    assert Z["Ji"][~fixed_i].any(axis=1).all() and Z["Jp"].any(axis=1).all()
    # the straight branch does not read b: its column of Jp is zero, and so is every entry but d e_x / d k_l, d e_x / d k_r ... R(-0)
    assert not Z["Jp"][straight][:, 6:9].any() and not Z["Jp"][straight][:, [2, 5]].any()
    assert np.abs(Z["Jp"][~straight][:, 6:9]).max(axis=1).min() > 0
    assert (g["op"] == H.PARAM_ROW_2).sum() == 100


def _special():
    g = H.take_edges(H.load_graph(Z), slice(0, H.N_SPECIAL))
    return g, H.producers(H.FP64, g, fixed_zero=False)


def test_exact_jacobian_against_the_references_difference():
    """The issue's own table is judged here, all nine columns, both branches: the exact derivative against BaseMultiEdge's central
    difference (delta = 1e-9, additive on the parameter vertex).  The difference is evaluated at 60 digits, where only its
    truncation error remains; that error is recorded in the fixture (the expression of tests/test_sensor_calib_host.py), and the
    fp64 exact Jacobian may differ from it by that plus its own recorded drift.  The recorded truncation comes from the same two
    formulas, so a wrong exact Jacobian would widen its own bound: the independent guard is the ABSOLUTE cap on it, asserted first --
    delta^2 / 6 times a third derivative of entries that reach about 150 is below 1e-12, a wrong column is wrong by its own size."""
    assert Z["numeric_noise"].max() < 1e-12       # (O(delta^2) on entries of order 1 ... 100)
    g, (Ji, Jj, Jp, _) = _special()
    turning = Z["turning"][:H.N_SPECIAL]
    assert turning.sum() >= 8 and (~turning).sum() >= 6
    N = OC.numeric_edges(H.MP, g["poses"], g["oi"], g["oj"], g["op"], g["omeas"])
    N = [np.array([[float(v) for v in row] for row in A]) for A in N]
    row = Z["drift"][-1]
    for name, J, A, noise, dr in (("Ji", Ji, N[0], Z["numeric_noise"][0], row[1]), ("Jj", Jj, N[1], Z["numeric_noise"][0], row[2]),
                                  ("Jp", Jp, N[2], Z["numeric_noise"][1], row[3])):
        for tag, sel in (("turning", turning), ("straight", ~turning)):
            fig = np.abs(J[sel] - A[sel]).max()
            print(name, tag, "exact vs the reference's central difference", fig, "truncation", float(noise), "bound", float(noise + dr))
            assert fig <= noise + dr
    # every column is exercised: none of the nine is zero on all turning edges but d e_t / d th2
    cols = [np.abs(np.concatenate([Ji, Jj, Jp], axis=1)[turning][:, 3 * c:3 * c + 3]).max() for c in range(9)]
    assert all(c > 0 for c in cols), cols
    # in fp64 the same difference carries rounding noise of eps |e| / delta: only its order is checked
    F = OC.numeric_edges(H.FP64, g["poses"], g["oi"][:20], g["oj"][:20], g["op"][:20], g["omeas"][:20])
    assert max(np.abs(J[:20] - np.array(A)).max() for J, A in zip((Ji, Jj, Jp), F)) < 1e-3


def test_convert_round_trip():
    """convert_to_velocity(convert_to_motion(v, 1)) == v on turning and straight motions: exactly so at 60 digits (to 1e-50), and in
    fp64 up to the rounding of R = y2 (x3 y4 - y3 x4) / (y2 (x3 - x4)), whose numerator and denominator cancel by |th| for small
    turns: 64 eps / |th| relative."""
    eps = np.finfo(np.float64).eps
    for v in ([0.4, 0.7, 1.3], [0.9, 0.2, 0.6], [-0.3, 0.5, 1.0], [0.5, 0.5, 0.9], [1.25, 1.25, 2.0], [0.5, 0.52, 1.0]):
        m = OC.convert_to_motion(H.FP64, v, 1.0)
        back = OC.convert_to_velocity(H.FP64, m, v[2])
        th = abs(m[2])
        tol = 64 * eps / th if th > 0 else 4 * eps
        assert np.abs(np.array(back) - v).max() <= tol * np.abs(v).max(), (v, back)
        if v[0] == v[1]:
            assert m[1] == 0.0 and m[2] == 0.0 and back[0] == back[1]
        mm = OC.convert_to_motion(H.MP, v, 1.0)
        bb = OC.convert_to_velocity(H.MP, mm, v[2])
        assert max(abs(float(a - H.MP.num(b))) for a, b in zip(bb, v)) < 1e-50


def test_g2o_round_trip(tmp_path):
    g = S.make_calib_rig(9, loops=4, seed=3, odom_calib=True, n_params=2)
    path = os.path.join(str(tmp_path), "rig.g2o")
    ids = np.arange(12) * 2 + 10
    g2o_io.write_g2o_odom_calib(path, g, ids=ids)
    text = open(path).read()
    assert text.count("EDGE_SE2_ODOM_DIFFERENTIAL_CALIB ") == 8 and text.count("EDGE_SE2_CALIB ") == 12
    assert text.count("VERTEX_SE2 ") == 10 and text.count("VERTEX_ODOM_DIFFERENTIAL ") == 2 and "FIX 10\n" in text
    assert "VERTEX_ODOM_DIFFERENTIAL 30 1 1 1\n" in text                                        # id k_l k_r b
    rd = g2o_io.read_g2o(path)
    p = g2o_io.odom_calib_problem(rd)
    for k in ("poses", "Z", "omega", "cmeas", "cinfo", "omeas", "oinfo"):
        assert np.array_equal(np.asarray(p[k]).reshape(-1), np.asarray(g[k]).reshape(-1)), k
    for k in ("ci", "cj", "cl", "vi", "vj", "hidx", "oi", "oj", "op", "param_rows"):
        assert np.array_equal(p[k], g[k]), k
    assert p["nP"] == g["nP"] == 11
    # the group alone: no EdgeSE2, no EDGE_SE2_CALIB
    alone = {k: v for k, v in H.without_odometry(g).items() if k not in ("ci", "cj", "cl", "cmeas", "cinfo")}
    g2o_io.write_g2o_odom_calib(path, alone)
    q = g2o_io.odom_calib_problem(g2o_io.read_g2o(path))
    assert "ci" not in q and len(q["vi"]) == 0 and q["Z"].shape == (0, 3) and np.array_equal(q["omeas"], g["omeas"])
    # a file without the tags parses as before
    g2o_io.write_g2o_calib(path, S.make_calib_rig(9, loops=4, seed=3))
    rd = g2o_io.read_g2o(path)
    assert not any(k.startswith("odo") for k in rd)
    with pytest.raises(ValueError):
        g2o_io.odom_calib_problem(rd)


def _rig_hash(g):
    h = hashlib.sha256()
    for k in sorted(g):
        a = np.ascontiguousarray(np.asarray(g[k]))
        for part in (k.encode(), str(a.dtype).encode(), str(a.shape).encode(), a.tobytes()):
            h.update(part)
    return h.hexdigest()


def test_make_calib_rig_defaults_unchanged_and_the_new_half():
    """The hashes are those of make_calib_rig at the commit before the odom_calib argument existed (keys, dtypes, shapes, bytes)."""
    assert _rig_hash(S.make_calib_rig()) == "eda59745545301051b946abece332de95c1d520ebf6e0643f8e213629905d0b0"
    assert _rig_hash(S.make_calib_rig(9, loops=4, seed=3, wrap_every=3, fix_offset=True)) == "0af17df3c025c7709faa0549bc28bdbc0be382b1285837e9b69fa89e1ce085a6"
    a, b = S.make_calib_rig(40, seed=5, odom_calib=True), S.make_calib_rig(40, seed=5, odom_calib=True)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert a["n"] == 42 and a["nP"] == 41 and list(a["param_rows"]) == [41] and (a["op"] == 41).all() and len(a["oi"]) == 39
    assert np.array_equal(a["poses"][41], [1.0, 1.0, 1.0]) and (np.abs(a["params_true"][0] - 1.0) > 0.05).all()   # setToOriginImpl
    turn = np.abs((np.diff(a["poses_true"][:40, 2]) + np.pi) % (2 * np.pi) - np.pi)
    assert (turn == 0).sum() == 7 and (turn > 0.05).sum() == 32                                 # straight and turning segments
    D, _ = OC.branch_margin(a["poses_true"], a["op"], a["omeas"])
    assert (D < 1e-7).sum() == 7                                                                # the straight branch at the truth
    e = OC.odom_calib_edges(H.FP64, a["poses_true"], a["oi"], a["oj"], a["op"], a["omeas"], jac=False)
    assert 0 < np.abs(e).max() < 0.1                                                            # the truth's odometry up to the noise
    e1 = OC.odom_calib_edges(H.FP64, np.concatenate([a["poses_true"][:41], np.ones((1, 3))]), a["oi"], a["oj"], a["op"], a["omeas"], jac=False)
    assert np.abs(e1).max() > 2 * np.abs(e).max()                                               # (1, 1, 1) is not the truth
    two = S.make_calib_rig(40, seed=5, odom_calib=True, n_params=2)
    assert two["n"] == 43 and two["nP"] == 42 and set(two["op"]) == {41, 42} and not np.array_equal(two["params_true"][0], two["params_true"][1])
    # observability: the Gauss-Newton matrix of the whole graph (both groups, no EdgeSE2, pose 0 fixed) is positive definite
    g = H.without_odometry(two)
    o, m, mc = H.oracle_graph(g)
    H.feed_oracle(g, o, m, mc)
    o.build_system()
    w = np.linalg.eigvalsh(o.dense_full())
    print("Gauss-Newton eigenvalues", w.min(), w.max())
    assert w.min() > 1e-9 * w.max()


def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(ROOT, "include", "g2ohip.h")).read()
    assert "int g2ohip_pg_set_odom_calib_edges(g2ohip_solver* s, int set_ij, int set_ip, int set_jp," in header
    for word in ("edge_se2_odom_differential_calib.h:45-63", "odometry_measurement.cpp:95-117", "vertex_odom_differential_params.h:43-46",
                 "additive row", "OF THE BRANCH TAKEN"):
        assert word in header, word
    lib = os.environ.get("G2OHIP_LIB") or os.path.join(ROOT, "openslam_g2o_amd", "lib", "libg2ohip.so")
    if not os.path.exists(lib):
        pytest.fail("the library is not built: %s" % lib)
    assert hasattr(ctypes.CDLL(lib), "g2ohip_pg_set_odom_calib_edges")
    from openslam_g2o_amd import capi
    assert hasattr(capi.HipBlockSolver, "pgSetOdomCalibEdges") and "g2ohip_pg_set_odom_calib_edges" in capi.EXPORTS
    assert capi.HipBlockSolver.odom_calib_sets is None
    assert "pgSetOdomCalibEdges" in open(os.path.join(ROOT, "openslam_g2o_amd", "cpp", "hip_block_solver.hpp")).read()
    src = os.path.join(ROOT, "openslam_g2o_amd", "csrc")
    bs = open(os.path.join(src, "block_solver.hip")).read()
    assert bs.index('#include "pg_calib.inc"') < bs.index('#include "pg_odom_calib.inc"')
    inc = open(os.path.join(src, "pg_odom_calib.inc")).read()
    assert "pg_offset_se2_mul" in inc and "pg_offset_se2_inverse" in inc and "scratch 0 bytes" in inc and "fp contract(off)" in inc
    names = list(inspect.signature(lm.setup_device_odom_calib_graph).parameters)
    assert names[:4] == ["estimates", "hidx", "num_free", "odom_calib_edges"] and "calib_edges" in names and "huber_delta" in names
