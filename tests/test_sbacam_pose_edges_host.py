"""CPU: the fp64 restatement of EdgeSBACam / EdgeSBAScale (openslam_g2o_amd/sbacam.py) against the 60-digit values of
tests/golden/sbacam_pose_edges.npz (generator: tests/golden/make_sbacam_pose_edges.py), the EDGE_CAM / EDGE_SCALE reader and
writer, and the generator's defaults."""
import hashlib
import os

import numpy as np
import pytest

from openslam_g2o_amd import g2o_io as IO, sbacam as SB, synthetic as S
from tests import sbacam_helpers as HB
from tests import sbacam_pose_helpers as H

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "sbacam_pose_edges.npz"))
CAM_NAMES = ["branch"] + ["c%d" % n for n in H.EDGE_COUNTS]
SCALE_NAMES = ["coincident"] + ["s%d" % n for n in H.EDGE_COUNTS]


def gold_graph(name):
    g = {k: GOLD["%s_%s" % (name, k)] for k in H.CAM_KEYS + ("J0", "J1", "err", "drift")}
    g["nP"] = int(g["hidx"].max()) + 1
    return g


@pytest.mark.parametrize("name", CAM_NAMES + SCALE_NAMES)
def test_fp64_restatement_within_recorded_drift(name):
    """The fixture's inputs are the helper's graphs, and the fp64 formulas reproduce the recorded drift (the same operations on
    the same machine arithmetic: equal, not merely within)."""
    scale = name in SCALE_NAMES
    g = gold_graph(name)
    fresh = (H.scale_graphs() if scale else H.cam_graphs())[name]
    for k in H.CAM_KEYS:
        assert np.array_equal(fresh[k], g[k]), k
    J0, J1, err = H.producers(H.FP64, g, scale)
    assert np.abs(err - g["err"]).max() <= g["drift"][0]
    assert np.abs(J0 - g["J0"]).max() <= g["drift"][1] and np.abs(J1 - g["J1"]).max() <= g["drift"][2]
    assert np.isfinite(J0).all() and np.isfinite(J1).all() and np.isfinite(err).all()
    fixed0, fixed1 = g["hidx"][g["vi"]] < 0, g["hidx"][g["vj"]] < 0
    assert not J0[fixed0].any() and not J1[fixed1].any()
    if not scale:
        zi = H.inverse_measurements(H.FP64, g["meas"])
        assert np.abs(zi - GOLD[name + "_zinv"]).max() <= g["drift"][3]
        assert np.abs(np.linalg.norm(zi[:, 3:], axis=1) - 1.0).max() <= 4 * np.finfo(float).eps and (zi[:, 6] >= 0).all()


def test_branch_graph_takes_every_branch():
    g = gold_graph("branch")
    tr = GOLD["branch_trace"]
    assert [tuple(map(bool, tr[k])) for k in (5, 6, 7, 0)] == [H.BRANCH_TRACE[k] for k in (5, 6, 7, 0)]
    assert g["meas"][7, 6] < 0 and abs(np.linalg.norm(g["meas"][7, 3:]) - 2.5) < 1e-12
    assert g["hidx"][g["vi"][0]] < 0 and g["hidx"][g["vj"][1]] < 0 and (g["hidx"][[1, 2]] >= 0).all()
    assert (g["vi"][2], g["vj"][2]) == (g["vi"][3], g["vj"][3]) == (g["vj"][4], g["vi"][4])
    assert not g["err"][8].any()                                   # e = 0 exactly, at 60 digits ...
    assert not H.producers(H.FP64, g, False, jac=False)[8].any()   # ... and in fp64
    assert np.abs(g["est"][[9, 10], :3]).min() > 900


def test_scale_rotation_columns_are_exactly_zero():
    """Every column is evaluated by the restatement (nothing is skipped there): the rotation columns come out exactly zero; the
    coincident pair has a finite error and a zero Jacobian."""
    for name in SCALE_NAMES:
        g = gold_graph(name)
        J0, J1, err = H.producers(H.FP64, g, True)
        for J in (J0, J1, g["J0"], g["J1"]):
            assert not J[:, 3:].any()
    g = gold_graph("coincident")
    J0, J1, err = H.producers(H.FP64, g, True)
    assert err[0, 0] == g["meas"][0] and not J0.any() and not J1.any()


@pytest.mark.parametrize("points", [True, False])
def test_io_round_trip(tmp_path, points):
    g = H.lm_problem(points)
    rng = np.random.default_rng(1)
    A = rng.integers(-3, 4, size=(len(g["cam_edges"]["vi"]), 6, 6)).astype(np.float64)
    g["cam_edges"]["info"] = (A @ A.transpose(0, 2, 1) + 6 * np.eye(6)).reshape(-1, 36)      # a full upper triangle, not a diagonal
    path = str(tmp_path / "a.g2o")
    IO.write_g2o_sbacam(path, g)
    rd = IO.read_g2o(path)
    q = IO.sbacam_ba_problem(rd)
    for key in ("cam_edges", "scale_edges"):
        for k in ("vi", "vj", "meas", "info"):
            assert np.array_equal(np.asarray(q[key][k]).reshape(-1), np.asarray(g[key][k]).reshape(-1)), (key, k)
    assert np.array_equal(rd["cam_edge_info"].reshape(-1, 6, 6), rd["cam_edge_info"].reshape(-1, 6, 6).transpose(0, 2, 1))
    for k in ("hidx", "vp", "vl", "zl", "intrinsics"):
        assert np.array_equal(q[k], g[k]), k
    assert q["nP"] == g["nP"] and q["nL"] == (g["nL"] if points else 0)
    lines = open(path).read().splitlines()
    assert sum(l.startswith("EDGE_CAM ") for l in lines) == 14 and sum(l.startswith("EDGE_SCALE ") for l in lines) == 2
    assert all(len(l.split()) == 3 + 7 + 21 for l in lines if l.startswith("EDGE_CAM "))


def test_file_without_the_tags_is_unchanged(tmp_path):
    g = S.make_sbacam_ba(stereo=True, **HB.BA_ARGS)
    a, b = str(tmp_path / "a.g2o"), str(tmp_path / "b.g2o")
    IO.write_g2o_sbacam(a, g)
    rd = IO.read_g2o(a)
    assert not [k for k in rd if k.startswith("cam_edge_") or k.startswith("cam_scale_")]
    q = IO.sbacam_ba_problem(rd)
    assert "cam_edges" not in q and "scale_edges" not in q
    IO.write_g2o_sbacam(b, q)
    assert open(a).read() == open(b).read()
    assert "EDGE_CAM" not in open(a).read() and "EDGE_SCALE" not in open(a).read()


def test_generator_defaults_are_unchanged():
    h = hashlib.sha256()
    for stereo in (False, True):
        g = S.make_sbacam_ba(stereo=stereo, **HB.BA_ARGS)
        assert "cam_edges" not in g and "scale_edges" not in g
        for k in sorted(g):
            h.update(k.encode())
            h.update(np.ascontiguousarray(np.asarray(g[k])).tobytes())
    assert h.hexdigest() == str(GOLD["default_hash"])


def test_generated_constraints():
    g = H.lm_problem()
    ce, se = g["cam_edges"], g["scale_edges"]
    assert list(zip(ce["vi"][:11], ce["vj"][:11])) == [(i, i + 1) for i in range(11)]
    assert list(zip(ce["vi"][11:], ce["vj"][11:])) == [(0, 4), (4, 8), (8, 0)]
    err = SB.pose_edges(SB.FP64, g["est_true"], ce["vi"], ce["vj"], ce["meas"], jac=False)
    assert 0 < np.abs(err[:, :3]).max() < 0.05 and 0 < np.abs(err[:, 3:]).max() < 0.01      # the noise, at the true cameras
    es = SB.pose_edges(SB.FP64, g["est_true"], se["vi"], se["vj"], se["meas"], scale=True, jac=False)
    assert 0 < np.abs(es).max() < 0.05
    p = H.lm_problem(points=False)
    assert len(p["vp"]) == 0 and np.array_equal(p["est"], g["est"]) and np.array_equal(p["cam_edges"]["meas"], ce["meas"])
