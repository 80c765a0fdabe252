"""CPU side of stereo bundle adjustment on the device (EdgeProjectXYZ2UVU in the BA front end's slot): the NumPy restatement of
the edge against central differences, the generator and the `.g2o` reader / writer with and without the new argument, the
declaration of the entry through every host layer, and the oracle's LM run over the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

from openslam_g2o_amd import capi, g2o_io, synthetic as S
from tests import stereo_helpers as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _central_differences(lin, g, h=1e-6):
    """d err / d (pose update) [E][d][6] and d err / d point [E][d][3] by central differences with step h: the pose through
    synthetic._apply_cam_update (every camera moved, the fixed ones too), the point by plain addition."""
    P, L = g["P"], g["L"]
    cols_c, cols_p = [], []
    for c in range(6):
        upd = np.zeros((P, 6))
        upd[:, c] = h
        ep = lin(dict(g, cams=S._apply_cam_update(g["cams"], upd)))
        em = lin(dict(g, cams=S._apply_cam_update(g["cams"], -upd)))
        cols_c.append((ep - em) / (2 * h))
    for c in range(3):
        d = np.zeros((L, 3))
        d[:, c] = h
        ep = lin(dict(g, pts=g["pts"] + d))
        em = lin(dict(g, pts=g["pts"] - d))
        cols_p.append((ep - em) / (2 * h))
    return np.stack(cols_c, axis=2), np.stack(cols_p, axis=2)


def _rel(fd, an):
    return float(np.abs(fd - an).max() / np.abs(an).max())


def test_restatement_against_central_differences():
    """The stereo restatement's Jacobians against central differences (step 1e-6).  Bound: ten times what the identical
    check gives for the existing synthetic.ba_linearize (rows 0-1 of the same edges) on the same graph, the noise floor of
    the method.  Row 2 is also looked at on its own: it is the only new formula."""
    g = SH.graph()
    assert g["E"] == 1025 and g["meas"].shape == (1025, 3) and g["baseline"] == SH.BASELINE
    E = g["E"]
    mono = dict(g, meas=g["meas"][:, :2])
    Jp, Jc, _ = S.ba_linearize(mono)
    fc, fp = _central_differences(lambda q: S.ba_linearize(q, jac=False), mono)
    floor_c, floor_p = _rel(fc, Jc.reshape(E, 6, 2).transpose(0, 2, 1)), _rel(fp, Jp.reshape(E, 3, 2).transpose(0, 2, 1))
    J0, J1, err = SH.linearize(g)
    assert J0.shape == (E, 9) and J1.shape == (E, 18) and err.shape == (E, 3)
    sc, sp = _central_differences(lambda q: SH.linearize(q, jac=False), g)
    A, B = J0.reshape(E, 3, 3).transpose(0, 2, 1), J1.reshape(E, 6, 3).transpose(0, 2, 1)
    got_c, got_p = _rel(sc, B), _rel(sp, A)
    row2_c, row2_p = _rel(sc[:, 2], B[:, 2]), _rel(sp[:, 2], A[:, 2])
    print("central differences, relative: mono pose %.3e point %.3e | stereo pose %.3e point %.3e | row 2 pose %.3e point %.3e"
          % (floor_c, floor_p, got_c, got_p, row2_c, row2_p))
    assert got_c <= 10 * floor_c and got_p <= 10 * floor_p
    assert row2_c <= 10 * floor_c and row2_p <= 10 * floor_p
    # rows 0-1 are the mono edge's, the errors too: the same products associated differently (f x / z against x / z f), so equal
    # to a few roundings of the largest entry -- 1e-14 is some 45 eps
    assert _rel(A[:, :2], Jp.reshape(E, 3, 2).transpose(0, 2, 1)) < 1e-14 and _rel(B[:, :2], Jc.reshape(E, 6, 2).transpose(0, 2, 1)) < 1e-14
    assert np.abs(err[:, :2] - S.ba_linearize(mono, jac=False)).max() < 1e-14 * np.abs(g["meas"]).max()
    # and the baseline is what tells row 2 from row 0
    assert np.abs(err[:, 2] - err[:, 0]).max() > 1.0


@pytest.mark.parametrize("kw", [{}, {"outlier_frac": 0.05}, {"seed": 43, "obs_per_landmark": 3}])
def test_default_generator_output_is_unchanged(kw):
    a = S.make_ba_problem(40, 205, **kw)
    b = S.make_ba_problem(40, 205, stereo_baseline=None, **kw)
    s = S.make_ba_problem(40, 205, stereo_baseline=0.2, **kw)
    assert sorted(a) == sorted(b) and "observation" not in a and "baseline" not in a
    assert sorted(s) == sorted(list(a) + ["observation", "baseline"])
    for k in a:
        assert np.array_equal(a[k], b[k]) and type(a[k]) is type(b[k]), k
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        if k != "meas":
            assert np.array_equal(a[k], s[k]), k
    assert a["meas"].shape == (a["E"], 2) and s["meas"].shape == (a["E"], 3)
    assert np.array_equal(s["meas"][:, :2], a["meas"])
    assert s["observation"] == "stereo" and s["baseline"] == 0.2
    # the third column: u_right of the true scene plus unit noise, outliers anywhere in the image width
    d = s["meas"][:, 0] - s["meas"][:, 2]                 # disparity = f b / z, z in [3, 4] up to the noise
    inl = np.abs(d - 1000.0 * 0.2 / 3.5) < 1000.0 * 0.2 * (1 / 3.0 - 1 / 4.0) / 2 + 8.0
    if kw.get("outlier_frac", 0) > 0:
        assert 0.01 * a["E"] < (~inl).sum() < 0.1 * a["E"]
        assert s["meas"][~inl, 2].min() >= 0.0 and s["meas"][~inl, 2].max() <= 640.0
    else:
        assert inl.all()


def test_g2o_round_trip_of_a_stereo_problem(tmp_path):
    g = SH.graph()
    g["omega"] = SH.full_information(g["E"])
    path = str(tmp_path / "stereo.g2o")
    g2o_io.write_g2o_ba(path, g)
    lines = open(path).read().split("\n")
    assert lines[0].split() == ["PARAMS_CAMERAPARAMETERS", "0", "1000", "320", "240", "0.20000000000000001"]
    edges = [l for l in lines if l.startswith("EDGE_PROJECT_")]
    assert len(edges) == g["E"] and all(l.split()[0] == "EDGE_PROJECT_XYZ2UVU:EXPMAP" and len(l.split()) == 12 for l in edges)
    back = g2o_io.read_g2o_ba(path)
    assert back["observation"] == "stereo" and back["baseline"] == g["baseline"]
    for k in ("P", "L", "E", "nP", "nL"):
        assert back[k] == g[k], k
    for k in ("cam_idx", "pt_idx", "cam_hidx", "v0", "v1"):
        assert np.array_equal(back[k], g[k]) and back[k].dtype == g[k].dtype, k
    for k in ("f", "cx", "cy", "pts", "meas", "omega", "cams"):
        gap = np.abs(np.asarray(back[k]) - np.asarray(g[k])).max() / np.abs(np.asarray(g[k])).max()
        assert gap <= 1e-15, (k, gap)
    # identity information when the problem carries none
    g2 = SH.graph()
    g2o_io.write_g2o_ba(path, g2)
    assert np.array_equal(g2o_io.read_g2o_ba(path)["omega"], SH.omega(g2))
    # a file that mixes the two edge tags is refused, either way round
    mono = str(tmp_path / "mono.g2o")
    g2o_io.write_g2o_ba(mono, S.make_ba_problem(40, 205))
    mono_edge = [l for l in open(mono).read().split("\n") if l.startswith("EDGE_PROJECT_")][0]
    body = [l for l in lines if l]
    for mixed in (body + [mono_edge], body[:-g["E"]] + [mono_edge] + body[-g["E"]:]):
        bad = str(tmp_path / "mixed.g2o")
        open(bad, "w").write("\n".join(mixed) + "\n")
        with pytest.raises(ValueError):
            g2o_io.read_g2o_ba(bad)


def test_a_mono_problem_is_written_and_read_as_before(tmp_path):
    g = S.make_ba_problem(40, 205)
    path = str(tmp_path / "mono.g2o")
    g2o_io.write_g2o_ba(path, g)
    text = open(path).read()
    lines = text.split("\n")
    assert lines[0] == "PARAMS_CAMERAPARAMETERS 0 1000 320 240 0"
    assert "XYZ2UVU" not in text
    e0 = [l for l in lines if l.startswith("EDGE_")][0].split()
    assert e0[0] == "EDGE_PROJECT_XYZ2UV:EXPMAP" and len(e0) == 9 and e0[3] == "0" and e0[6:] == ["1", "0", "1"]
    assert e0[1] == str(g["P"] + g["pt_idx"][0]) and e0[2] == str(g["cam_idx"][0])
    assert e0[4] == "%.17g" % g["meas"][0][0] and e0[5] == "%.17g" % g["meas"][0][1]
    back = g2o_io.read_g2o_ba(path)
    assert sorted(back) == sorted(list(g) + ["omega"])
    assert back["meas"].shape == (g["E"], 2) and back["omega"].shape == (g["E"], 4)
    assert np.array_equal(back["meas"], g["meas"])


def test_every_host_layer_declares_the_stereo_entry():
    name = "g2ohip_ba_set_stereo_edges"
    hdr = open(os.path.join(ROOT, "include", "g2ohip.h")).read()
    assert name in set(re.findall(r"\b(g2ohip_\w+)\s*\(", hdr)), "include/g2ohip.h does not declare %s" % name
    m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["g2ohip_solver* s", "int set", "const int32_t* cam_vertex", "const int32_t* point_vertex", "const double* meas",
                    "const double* info", "double focal_length", "double cx", "double cy", "double baseline"]
    assert "ba_stereo_staged" in hdr and "types_six_dof_expmap.h:181-200" in hdr
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), name), "libg2ohip.so does not export %s" % name
    assert name in capi.EXPORTS
    assert callable(getattr(capi.HipBlockSolver, "baSetStereoEdges"))
    hpp = open(os.path.join(ROOT, "openslam_g2o_amd", "cpp", "hip_block_solver.hpp")).read()
    assert "baSetStereoEdges" in hpp and name in hpp


def test_oracle_lm_run_converges():
    """Ten LM iterations of the oracle over the restatement on lm_test_graph(): chi2 falls below 1 % of the start, Schur and
    full system alike, with the same accept / reject pattern."""
    g = SH.lm_test_graph()
    z = np.einsum("nij,nj->ni", g["cams"][g["cam_idx"], 0:9].reshape(-1, 3, 3).transpose(0, 2, 1), g["pts"][g["pt_idx"]])[:, 2] \
        + g["cams"][g["cam_idx"], 11]
    assert z.min() > 1.0                                   # every point in front of its cameras at the start
    n, chis, lams, trials, og = SH.oracle_lm_run(g, 10)
    n2, chis2, _, trials2, _ = SH.oracle_lm_run(g, 10, dense=True)
    print("oracle lm chi2", chis, "trials", trials)
    assert n == n2 == 10 and trials == trials2
    e = SH.linearize(g, jac=False)
    start = float((e * e).sum())                           # (information = identity; chis[0] is the chi2 AFTER the first iteration)
    print("start", start)
    assert chis[0] < start and chis[-1] < 0.01 * start
    assert max(abs(a - b) / a for a, b in zip(chis, chis2)) < 1e-9
    assert np.abs(og.pr["pts"] - g["pts"]).max() > 0.05
