"""CPU: the fixture tests/golden/producer_edges.npz against its own source and against the oracle.

  * one edge in eight of every group, and every edge of the boundary subgroups, is evaluated again with the
    extended-precision reference (tests/reference_mp.py) and must give the stored value to one ulp;
  * the oracle's C producers / oplus (oracle/g2o_oracle_types.c), its robust kernels and tests/landmark_helpers.py against the
    fixture with the per-edge metric of tests/producer_metric.py: each output reproduces the figure the generator stored
    (oracle_<output>) and that figure stays a factor 8 below 1e-12;
  * the generator's branch coverage, recounted from the fp64 predicates."""
import json
import os

import numpy as np

from oracle import oracle as O
from tests import landmark_helpers as LH
from tests import producer_metric as PM
from tests import reference_mp as M

FX = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "producer_edges.npz")))
SHARE = 8


def _ulp_equal(got, stored):
    got, stored = np.asarray(got, np.float64).reshape(-1), np.asarray(stored, np.float64).reshape(-1)
    assert np.all(np.abs(got - stored) <= np.spacing(np.abs(stored))), (got, stored)


def _share(n, boundary=None):
    pick = np.arange(n) % SHARE == 3
    if boundary is not None:
        pick |= boundary
    return np.nonzero(pick)[0]


def test_stored_values_are_the_reference_again():
    for k in _share(len(FX["se3_vi"]), FX["se3_boundary"]):
        r = M.se3_edge(FX["se3_poses"][FX["se3_vi"][k]], FX["se3_poses"][FX["se3_vj"][k]], FX["se3_Z"][k])
        for got, key in zip(r, ("se3_J0", "se3_J1", "se3_err")):
            _ulp_equal(M.f64(got), FX[key][k])
    for k in _share(len(FX["se2_vi"]), FX["se2_boundary"]):
        r = M.se2_edge(FX["se2_poses"][FX["se2_vi"][k]], FX["se2_poses"][FX["se2_vj"][k]], FX["se2_Z"][k])
        for got, key in zip(r, ("se2_J0", "se2_J1", "se2_err")):
            _ulp_equal(M.f64(got), FX[key][k])
    for k in _share(len(FX["lm2_vp"])):
        r = M.se2_point_edge(FX["lm2_poses"][FX["lm2_vp"][k]], FX["lm2_points"][FX["lm2_vl"][k]], FX["lm2_zl"][k])
        for got, key in zip(r, ("lm2_J0", "lm2_J1", "lm2_err")):
            _ulp_equal(M.f64(got), FX[key][k])
        r = M.se3_point_edge(FX["lm3_poses"][FX["lm3_vp"][k]], FX["lm3_points"][FX["lm3_vl"][k]], FX["lm3_zl"][k], FX["lm3_offset"])
        for got, key in zip(r, ("lm3_J0", "lm3_J1", "lm3_err")):
            _ulp_equal(M.f64(got), FX[key][k])
    for k in _share(len(FX["ba_cam_idx"])):
        T, X = FX["ba_cams"][FX["ba_cam_idx"][k]], FX["ba_pts"][FX["ba_pt_idx"][k]]
        f, cx, cy, kind, delta = FX["ba_classes"][FX["ba_edge_class"][k]]
        a, b, e = M.project_edge(T, X, FX["ba_meas"][k], f, cx, cy)
        for got, key in zip((a, b, e), ("ba_J0", "ba_J1", "ba_err")):
            _ulp_equal(M.f64(got), FX[key][k])
        _ulp_equal([float(M.robust(int(kind), delta, e[0] * e[0] + e[1] * e[1])[1])], FX["ba_w"][k])
    # every update (the groups are small and all of it is boundary)
    h = FX["upd_se3_hidx"]
    for v in range(len(h)):
        ref = FX["upd_se3_poses"][v] if h[v] < 0 else M.f64(M.iso_pack(M.se3_oplus(M.iso(FX["upd_se3_poses"][v]), M.V(FX["upd_se3_x"][6 * h[v]:6 * h[v] + 6]))))
        _ulp_equal(ref, FX["upd_se3"][v])
    h = FX["upd_se2_hidx"]
    for v in range(len(h)):
        ref = FX["upd_se2_poses"][v] if h[v] < 0 else M.f64(M.se2_oplus(M.V(FX["upd_se2_poses"][v]), M.V(FX["upd_se2_x"][3 * h[v]:3 * h[v] + 3])))
        _ulp_equal(ref, FX["upd_se2"][v])
    h = FX["upd_cam_hidx"]
    for v in range(len(h)):
        ref = FX["upd_cam_cams"][v] if h[v] < 0 else M.f64(M.iso_pack(M.expmap_oplus(M.iso(FX["upd_cam_cams"][v]), M.V(FX["upd_cam_x"][6 * h[v]:6 * h[v] + 6]))))
        _ulp_equal(ref, FX["upd_cam"][v])
    # robust kernels: chi2 of the per-edge run
    chi = sum(M.robust(int(k), d, sum(M.mp.mpf(float(x)) ** 2 for x in e))[0] for k, d, e in zip(FX["rob_kinds"], FX["rob_deltas"], FX["rob_err"]))
    _ulp_equal([float(chi)], FX["rob_edge_chi2"])


def _oracle_figure(key, got, ops_key=None):
    ops = FX[ops_key or key.rsplit("_", 1)[0] + "_ops"]
    fig, k = PM.worst(got, FX[key], ops)
    print("oracle", key, fig, "edge", k, "stored", float(FX["oracle_" + key]))
    assert fig <= max(float(FX["oracle_" + key]), 0.0) * (1 + 1e-9) + 1e-300, (key, fig, k)
    assert PM.MARGIN * fig <= PM.CEILING
    PM.bound(FX, key)


def test_oracle_producers_and_oplus_against_the_fixture():
    J0, J1, e = O.se3_edges(FX["se3_poses"], FX["se3_vi"], FX["se3_vj"], FX["se3_Z"])
    for key, got in (("se3_J0", J0), ("se3_J1", J1), ("se3_err", e)):
        _oracle_figure(key, got)
    J0, J1, e = O.se2_edges(FX["se2_poses"], FX["se2_vi"], FX["se2_vj"], FX["se2_Z"])
    for key, got in (("se2_J0", J0), ("se2_J1", J1), ("se2_err", e)):
        _oracle_figure(key, got)
    J0, J1, e = LH.se2_pointxy_edges(FX["lm2_poses"], FX["lm2_points"], FX["lm2_vp"], FX["lm2_vl"], FX["lm2_zl"])
    for key, got in (("lm2_J0", J0), ("lm2_J1", J1), ("lm2_err", e)):
        _oracle_figure(key, got)
    J0, J1, e = LH.se3_pointxyz_edges(FX["lm3_poses"], FX["lm3_points"], FX["lm3_vp"], FX["lm3_vl"], FX["lm3_zl"], FX["lm3_offset"])
    for key, got in (("lm3_J0", J0), ("lm3_J1", J1), ("lm3_err", e)):
        _oracle_figure(key, got)
    E = len(FX["ba_cam_idx"])
    for pre, klass in (("ba", FX["ba_edge_class"]), ("ba1", np.zeros(E, np.int32))):
        J0, J1, e = np.zeros((E, 6)), np.zeros((E, 12)), np.zeros((E, 2))
        for c in range(len(FX["ba_classes"])):
            sel = np.nonzero(klass == c)[0]
            if len(sel):
                f, cx, cy = FX["ba_classes"][c, :3]
                J0[sel], J1[sel], e[sel] = O.ba_edges(FX["ba_cams"], FX["ba_pts"], FX["ba_cam_idx"][sel], FX["ba_pt_idx"][sel],
                                                      FX[pre + "_meas"][sel], f, cx, cy)
        for key, got in ((pre + "_J0", J0), (pre + "_J1", J1), (pre + "_err", e)):
            _oracle_figure(key, got, pre + "_ops")
        par = FX["ba_classes"][klass].copy()
        if pre == "ba1":
            par[:, 3], par[:, 4] = 1, float(FX["ba1_huber"])
        nP = int(FX["ba_cam_hidx"].max()) + 1
        prod = PM.ba_products_fp64(O.robustify, pre, J0, J1, e, par, FX["ba_cam_hidx"][FX["ba_cam_idx"]], FX["ba_pt_idx"], nP, len(FX["ba_pts"]))
        for key in ("_Hpl", "_Hpp", "_Hll"):
            _oracle_figure(pre + key, prod[pre + key], pre + key + "_ops")
        fig = PM.worst(prod[pre + "_b"].reshape(-1, 1), FX[pre + "_b"].reshape(-1, 1), FX[pre + "_b_ops"])[0]
        assert fig <= float(FX["oracle_" + pre + "_b"]) * (1 + 1e-9) and PM.MARGIN * fig <= PM.CEILING
        fig = abs(prod[pre + "_chi2"][0] - float(FX[pre + "_chi2"])) / max(1.0, float(FX[pre + "_chi2_ops"]), abs(float(FX[pre + "_chi2"])))
        assert fig <= float(FX["oracle_" + pre + "_chi2"]) * (1 + 1e-9) and PM.MARGIN * fig <= PM.CEILING
    _oracle_figure("upd_se3", O.se3_oplus(FX["upd_se3_poses"], FX["upd_se3_hidx"], FX["upd_se3_x"]), "upd_se3_ops")
    _oracle_figure("upd_se2", O.se2_oplus(FX["upd_se2_poses"], FX["upd_se2_hidx"], FX["upd_se2_x"]), "upd_se2_ops")
    c, p = O.ba_oplus(FX["upd_cam_cams"], FX["upd_pts_pts"], FX["upd_cam_hidx"], FX["upd_pts_hidx"],
                      np.concatenate([FX["upd_cam_x"], FX["upd_pts_x"]]), len(FX["upd_cam_x"]))
    _oracle_figure("upd_cam", c, "upd_cam_ops")
    _oracle_figure("upd_pts", p, "upd_pts_ops")
    for pre, pts in (("lm2", FX["lm2_points"]), ("lm3", FX["lm3_points"])):
        dp, nf = (3, 39) if pre == "lm2" else (6, 39)
        assert nf == int(FX[pre + "_hidx"].max()) + 1
        _oracle_figure("upd_%s_pts" % pre, LH.points_oplus(pts, FX[pre + "_pt_hidx"], FX["upd_%s_x" % pre], dp * nf, nf), "upd_%s_pts_ops" % pre)
    # the robust blocks of every run from the oracle's kernels in fp64, against the stored figures
    figs = dict(rob_Hpp=0.0, rob_b=0.0, rob_chi2=0.0)
    n = len(FX["rob_err"])
    for run in ("edge", "set1", "set2", "set3", "set4", "set5"):
        kk = FX["rob_kinds"] if run == "edge" else np.full(n, int(run[3:]))
        dd = FX["rob_deltas"] if run == "edge" else np.full(n, float(FX["rob_set_delta"]))
        H, b, chi = np.zeros((2 * n, 9)), np.zeros((2 * n, 3)), 0.0
        for k in range(n):
            e2 = float(FX["rob_err"][k] @ FX["rob_err"][k])
            r = O.robustify(int(kk[k]), dd[k], e2) if kk[k] > 0 else (e2, 1.0, 0.0)
            chi += r[0]
            for v, J in ((2 * k, FX["rob_J0"][k]), (2 * k + 1, FX["rob_J1"][k])):
                Jm = J.reshape(3, 3).T
                H[v], b[v] = r[1] * (Jm.T @ Jm).T.reshape(9), -r[1] * (Jm.T @ FX["rob_err"][k])
        z = np.zeros(2 * n)
        figs["rob_Hpp"] = max(figs["rob_Hpp"], PM.worst(H, FX["rob_%s_Hpp" % run], z)[0])
        figs["rob_b"] = max(figs["rob_b"], PM.worst(b, FX["rob_%s_b" % run].reshape(2 * n, 3), z)[0])
        figs["rob_chi2"] = max(figs["rob_chi2"], abs(chi - float(FX["rob_%s_chi2" % run])) / max(1.0, abs(float(FX["rob_%s_chi2" % run]))))
    for key, fig in figs.items():
        assert fig <= float(FX["oracle_" + key]) * (1 + 1e-9) and PM.MARGIN * fig <= PM.CEILING, (key, fig)
    # the oracle's robust kernels at every stored (kind, delta, e2): rho and rho' to the floor of rob_chi2 / rob_Hpp
    for k, d, e in zip(FX["rob_kinds"], FX["rob_deltas"], FX["rob_err"]):
        if k == 0:
            continue
        e2 = float(e @ e)
        got = O.robustify(int(k), d, e2)
        ref = M.robust(int(k), d, M.mp.mpf(e2))
        for g, r, key in ((got[0], ref[0], "rob_chi2"), (got[1], ref[1], "rob_Hpp")):
            assert abs(g - float(r)) <= PM.bound(FX, key) * max(1.0, abs(float(r))), (k, d, e2, g, float(r))


def test_branch_coverage_of_the_fixture():
    cov = json.loads(str(FX["coverage_json"]))
    counts = {}
    for k in range(len(FX["se3_vi"])):
        c, s, tr, gap = PM.se3_branch(FX["se3_poses"][FX["se3_vi"][k]], FX["se3_poses"][FX["se3_vj"][k]], FX["se3_Z"][k])
        assert (c, s) == (FX["se3_case"][k], FX["se3_sign"][k])
        name = "case%d/qw%s" % (c, "+" if s > 0 else "-")
        counts[name] = counts.get(name, 0) + 1
    assert counts == cov["se3"] and len(counts) == 7 and min(counts.values()) >= 12, counts
    assert int(FX["se3_boundary"].sum()) >= 48
    for name in ("inv:floor", "inv:floor+hi", "mul:floor", "mul:floor+hi"):
        assert cov["se2"][name] >= 10
    assert cov["se2"]["exactly+-pi"] >= 6
    assert all(cov["landmarks"]["tail%d" % t] == t for t in (1, 255, 256, 257, 513)) and len(FX["lm3_vp"]) == 513
    assert cov["landmarks"]["fixed_pose_edges"] > 0 and cov["landmarks"]["fixed_landmark_edges"] > 0
    assert min(cov["landmarks"][s] for s in ("front", "beside", "behind")) >= 50
    for pre in ("ba", "ba1"):
        sides = {k: v for k, v in cov["ba"][pre].items() if k.startswith("k")}
        assert min(sides.values()) >= 5 and cov["ba"][pre]["min_depth"] < 0.05 and cov["ba"][pre]["world_max"] > 1e4
        assert cov["ba"][pre]["max_uv"] > 5
    assert len(set(FX["ba_edge_class"].tolist())) >= 3
    up = cov["updates"]
    assert up["se3_update"]["w_neg"] >= 4 and up["se3_update"]["w_zero"] >= 6 and up["se3_update"]["w_pos"] >= 12
    assert min(up["se2_update"].get(s, 0) for s in ("in", "floor", "floor+hi")) >= 2
    assert up["camera_update"]["small"] >= 9 and up["camera_update"]["large"] >= 9
    u = FX["upd_cam_x"].reshape(-1, 6)
    th = np.sqrt((u[:, :3] ** 2).sum(axis=1))
    assert ((th > 0) & (th < 0.00001) & (th > 0.9e-5)).sum() >= 3 and ((th >= 0.00001) & (th < 1.1e-5)).sum() >= 3
    for k in range(1, 6):
        for s in ("<", "==", ">"):
            assert cov["robust"]["edge:k%d:%s" % (k, s)] >= 3 and cov["robust"]["set%d:k%d:%s" % (k, k, s)] >= 1
    assert all(h.min() < 0 for h in (FX["se3_hidx"], FX["se2_hidx"], FX["lm2_hidx"], FX["lm2_pt_hidx"], FX["ba_cam_hidx"],
                                     FX["upd_se3_hidx"], FX["upd_se2_hidx"], FX["upd_cam_hidx"], FX["upd_pts_hidx"]))
