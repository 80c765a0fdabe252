"""CPU: the host side of the inverse-depth binding (EdgeProjectPSI2UV) -- the fp64 restatement openslam_g2o_amd/psi2uv.py against
central differences of its own error, the cancellation of the two camera Jacobians on an edge observed by its own anchor, the
generator synthetic.make_ba_inverse_depth, the fixture's bookkeeping and the declaration of the interface in every layer."""
import os

import numpy as np

from openslam_g2o_amd import psi2uv as X
from openslam_g2o_amd import se3expmap
from openslam_g2o_amd import synthetic as S
from tests import psi2uv_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err(g, cams, pts):
    return X.problem_edges(g, cams, pts, jac=False)


def test_jacobians_against_central_differences_of_the_error():
    """Column c of a Jacobian against (e(x + h u_c) - e(x - h u_c)) / 2h through se3expmap.oplus (poses) and plain addition
    (points).  Tolerance, derived: the truncation error of the central difference is h^2 / 6 |e'''|, its rounding error
    eps |e| / h with |e| the size of the two values subtracted -- the projections, up to ~4e3 pixels here, not the residual.
    With D the largest Jacobian entry (the scale of every derivative: the arguments are O(1)), h = 1e-5 gives
    1e-10 / 6 * D * 10 (a factor 10 for the growth of the third derivative over the first: 1 / y2, 1 / psi2 enter up to the
    third power with y2 >= 3, psi2 >= 0.25) + 2.2e-16 * 4e3 / 1e-5 = 1.7e-10 D + 8.8e-8; asserted with a factor 4 on top."""
    g = H.graph_of(H.edge_list(), 300)
    Jp, Jc, Ja, e = X.problem_edges(g)
    n, h = g["E"], 1e-5
    D = max(np.abs(Jp).max(), np.abs(Jc).max(), np.abs(Ja).max())
    tol = 4 * (1.7e-10 * D + 8.8e-8)
    worst = 0.0
    for c in range(3):                                                # the points: every point moves, an edge reads its own
        d = np.zeros((g["L"], 3))
        d[:, c] = h
        num = (_err(g, g["cams"], g["pts"] + d) - _err(g, g["cams"], g["pts"] - d)) / (2 * h)
        worst = max(worst, np.abs(num - Jp[:, 2 * c:2 * c + 2]).max())
    own = g["cam_idx"] == g["anchor_idx"]
    for which, J, idx in (("pose", Jc, g["cam_idx"]), ("anchor", Ja, g["anchor_idx"])):
        for c in range(6):
            num = np.zeros((n, 2))
            for v in range(g["P"]):                                   # one camera at a time: pose and anchor of an edge move apart
                u = np.zeros((g["P"], 6))
                u[v, c] = h
                sel = (idx == v) & ~own
                if not sel.any():
                    continue
                ep = _err(g, se3expmap.oplus(g["cams"], u), g["pts"])
                em = _err(g, se3expmap.oplus(g["cams"], -u), g["pts"])
                num[sel] = ((ep - em) / (2 * h))[sel]
            worst = max(worst, np.abs(num - J[:, 2 * c:2 * c + 2])[~own].max())
    print("central differences: worst", worst, "tolerance", tol, "largest entry", D)
    assert worst <= tol
    # an edge observed by its own anchor does not move with its camera at all: the sum of the two blocks is its derivative
    for c in range(6):
        u = np.zeros((g["P"], 6))
        u[:, c] = h
        num = (_err(g, se3expmap.oplus(g["cams"], u), g["pts"]) - _err(g, se3expmap.oplus(g["cams"], -u), g["pts"])) / (2 * h)
        assert np.abs(num[own]).max() <= tol


def test_camera_jacobians_cancel_on_an_edge_observed_by_its_anchor():
    """cam == anchor: R_ca = R R' is the identity up to rounding and y = x_a, so J_pose + J_anchor = 0 up to the rounding of the
    products: a few ulp of the largest entry (R R' - I is ~2 ulp, and enters every entry once)."""
    g = H.graph_of(H.edge_list(), 300)
    Jp, Jc, Ja, e = X.problem_edges(g)
    own = g["cam_idx"] == g["anchor_idx"]
    assert own.sum() >= 2
    s = np.abs(Jc[own] + Ja[own]).max()
    bound = 16 * np.spacing(max(np.abs(Jc[own]).max(), np.abs(Ja[own]).max()))
    print("cancellation", s, bound)
    assert s <= bound
    assert np.abs(Jc[~own] + Ja[~own]).max() > 1.0                    # ... and only there


def test_make_ba_inverse_depth_round_trip():
    a = S.make_ba_inverse_depth(20, 100, seed=3)
    base = S.make_ba_problem(20, 100, seed=3)
    for k in base:
        if k not in ("pts", "v0", "v1"):
            assert np.array_equal(a[k], base[k]), k
    assert a["observation"] == "inverse_depth"
    K = base["E"] // base["L"]
    assert np.array_equal(a["pt_anchor"], base["cam_idx"].reshape(-1, K)[:, 0])      # the first observing camera
    assert np.array_equal(a["anchor_idx"], a["pt_anchor"][a["pt_idx"]])
    world = X.to_world(a["pts"], a["cams"][a["pt_anchor"]])
    assert np.abs(world - base["pts"]).max() <= 64 * np.spacing(np.abs(base["pts"]).max())
    assert np.abs(X.invert_depth(X.invert_depth(base["pts"])) - base["pts"]).max() <= 4 * np.spacing(np.abs(base["pts"]).max())
    # the errors are those of the XYZ scene: the same projection through another parametrisation
    e_xyz = S.ba_linearize(base, jac=False)
    e_psi = X.problem_edges(a, jac=False)
    assert np.abs(e_xyz - e_psi).max() < 1e-9
    # the three pairs and the rule of the anchor's own observation
    own = a["cam_idx"] == a["anchor_idx"]
    assert own.sum() == base["L"]                                       # every point is observed by its anchor once
    (p0, c0), (p1, a1), (c2, a2) = a["pairs"]
    h = a["cam_hidx"]
    assert np.array_equal(p0, base["v0"]) and np.array_equal(p0, p1) and np.array_equal(c0, c2) and np.array_equal(a1, a2)
    assert np.all(c0[own] == -1) and np.all(a1[own] == -1)
    assert np.array_equal(c0[~own], h[a["cam_idx"]][~own]) and np.array_equal(a1[~own], h[a["anchor_idx"]][~own])
    assert np.array_equal(a["v0"], p0) and np.array_equal(a["v1"], c0)
    assert (a1[~own] == -1).any() and (a1[~own] >= 0).any()             # fixed and free anchors


def test_fixture_matches_its_generator():
    z = np.load(H.GOLDEN)
    lst = H.edge_list()
    for k in lst:
        assert np.array_equal(z[k], lst[k]), k
    for n in H.EDGE_COUNTS:
        g = H.load_graph(z, n)
        F = H.producers(g)
        d = np.array([np.abs(F[3] - z["ref_err"][:n]).max(), max(np.abs(F[i] - z[r][:n]).max() for i, r in enumerate(("ref_Jp", "ref_Jc", "ref_Ja")))])
        assert np.array_equal(d, z["drift_%d" % n]), n
        assert g["nP"] == len(np.setdiff1d(np.union1d(g["cam_idx"], g["anchor_idx"]), [0, 1]))
    assert z["y2"].min() >= 0.5 and np.abs(z["pts"][:, 2]).min() >= 0.05
    # a handful of edges at 60 digits again
    g = H.load_graph(z, 300)
    for k in (0, 2, 5, 6, 299):
        Jp, Jc, Ja, e, _ = H.mp_edge(g["cams"][g["cam_idx"][k]], g["cams"][g["anchor_idx"][k]], g["pts"][g["pt_idx"][k]], g["meas"][k],
                                     g["f"], g["cx"], g["cy"])
        from tests import reference_mp as R
        assert np.array_equal(R.f64(e), z["ref_err"][k]) and np.array_equal(R.f64(Jc), z["ref_Jc"][k])


def test_oracle_multi_edge_system_equals_dense_numpy():
    """The CPU oracle's BaseMultiEdge restatement over the 65-edge graph against the dense n-ary quadratic form: what the recorded
    LM trajectories were computed with."""
    from tests.test_gpu_multi_edge import _dense
    g = H.graph_of(H.edge_list(), 65)
    Jp, Jc, Ja, e = X.problem_edges(g)
    o, m = H.oracle_multi(g)
    o.set_multi_edge_data(m, [Jp, Jc, Ja], g["info"], e, 0.0, 1)
    o.build_system()
    nP, nL = g["nP"], g["nL"]
    dims = np.array([6] * nP + [3] * nL)
    offs = np.concatenate([[0], np.cumsum(dims)[:-1]])
    verts = np.stack([g["pairs"][0][0], g["pairs"][0][1], g["pairs"][1][1]], axis=1)
    J = [Jp.reshape(-1, 3, 2).transpose(0, 2, 1), Jc.reshape(-1, 6, 2).transpose(0, 2, 1), Ja.reshape(-1, 6, 2).transpose(0, 2, 1)]
    Hm, b, chi = _dense(int(dims.sum()), dims, offs, verts, J, g["info"].reshape(-1, 2, 2).transpose(0, 2, 1), e, 0.0)
    assert abs(o.chi2() - chi) <= 1e-12 * chi
    assert np.abs(o.b() - b).max() <= 1e-12 * np.abs(b).max()
    Hd = o.dense_full()
    assert np.abs(Hd - Hm).max() <= 1e-12 * np.abs(Hm).max()


def test_interface_is_declared_everywhere():
    name = "g2ohip_ba_set_inverse_depth_edges"
    hdr = open(os.path.join(ROOT, "include", "g2ohip.h")).read()
    assert name in hdr and "types_six_dof_expmap.cpp:173-233" in hdr and "base_multi_edge.hpp:190-208" in hdr
    from openslam_g2o_amd import capi
    assert name in capi.EXPORTS and callable(getattr(capi.HipBlockSolver, "baSetInverseDepthEdges"))
    hpp = open(os.path.join(ROOT, "openslam_g2o_amd", "cpp", "hip_block_solver.hpp")).read()
    assert "baSetInverseDepthEdges" in hpp and name in hpp
    inc = open(os.path.join(ROOT, "openslam_g2o_amd", "csrc", "ba_psi.inc")).read()
    assert "scratch 0" in inc and "VGPRs" in inc
    for doc in ("README.md", "INTEGRATION.md"):
        assert name in open(os.path.join(ROOT, doc)).read(), doc


def test_symbol_is_exported_by_the_built_library():
    import ctypes
    from openslam_g2o_amd import capi
    name = "g2ohip_ba_set_inverse_depth_edges"
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), name), "libg2ohip.so does not export %s" % name
