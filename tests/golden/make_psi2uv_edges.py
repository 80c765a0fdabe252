"""Generator of tests/golden/psi2uv_edges.npz (CPU only; run from the repository root: python
tests/golden/make_psi2uv_edges.py).  Needs the built CPU oracle (make -C oracle).

The graphs of the device tests of the BA front end's inverse-depth binding (EdgeProjectPSI2UV, g2ohip_ba_set_inverse_depth_edges):
psi2uv_helpers.graph_of(edge_list(), n) for n = 1, 65, 256, 257, 300 -- prefixes of ONE list of 300 three-vertex edges over 8
cameras and 40 points, stored once.  For the list: err and the three Jacobians of the formulas of the reference evaluated with
mpmath at 60 digits (psi2uv_helpers.mp_edge over tests/reference_mp.py), rounded to fp64; per prefix the drift of
openslam_g2o_amd/psi2uv.py (the fp64 restatement) against them: max abs over err, over J_point | J_pose | J_anchor.  The GPU tests
bound the device against the restatement by 8 x the drift recorded here for the same graph -- the restatement's own figure, never
the device's.

  step     one update over every camera but 0 and 1 and every point but the fixed one: VertexSE3Expmap::oplusImpl at 60 digits
           (reference_mp.expmap_oplus) and plain addition; the same reference arrays and drift figures at the moved estimates, and
           the drift of se3expmap.oplus against the moved cameras
  lm       psi2uv_helpers.lm_graph(): LM_ITERATIONS iterations of lm.optimize over the CPU oracle's BaseMultiEdge restatement
           (add_multi_edge_set) fed by the fp64 restatement and by the 60-digit reference (rounded to fp64), plain and with a Huber
           kernel: the trials of both (asserted equal), chi2 per iteration, the relative gap per iteration and the max abs
           difference of the final cameras and points.  The GPU test bounds device-resident against host-fed by 8 x these.

Asserted here, so that the reference alone stays inside them: y2 >= 0.5 and |psi2| >= 0.05 for every edge (before and after the
step), at least two edges observed by their own anchor, a fixed anchor, a fixed observing camera and a fixed point each on some
edge, two edges on the same (point, pose) pair."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import se3expmap  # noqa: E402
from tests import psi2uv_helpers as H  # noqa: E402


def _drift(F, M, n):
    return np.array([np.abs(F[3][:n] - M[3][:n]).max(), max(np.abs(F[i][:n] - M[i][:n]).max() for i in range(3))])


def main():
    lst = H.edge_list()
    out = dict(lst)
    g = H.graph_of(lst, 300)
    M = H.mp_edges(g)
    F = H.producers(g)
    assert M[4].min() >= 0.5 and np.abs(g["pts"][g["pt_idx"], 2]).min() >= 0.05, (M[4].min(), np.abs(g["pts"][:, 2]).min())
    own = g["cam_idx"] == g["anchor_idx"]
    assert own[5] and own[6] and own.sum() >= 2 and not own[:5].any()
    for k in np.nonzero(own)[0]:
        assert g["pairs"][0][1][k] == g["pairs"][1][1][k] == g["pairs"][2][0][k] == -1
    h = g["cam_hidx"]
    assert h[g["anchor_idx"][0]] < 0 and h[g["cam_idx"][0]] >= 0                       # a fixed anchor
    assert h[g["cam_idx"][1]] < 0 and h[g["anchor_idx"][1]] >= 0                       # a fixed observing camera
    assert g["pt_hidx"][g["pt_idx"][2]] < 0 and g["pairs"][0][0][2] == -1               # a fixed point
    assert (g["pt_idx"][3], g["cam_idx"][3]) == (g["pt_idx"][4], g["cam_idx"][4]) and not own[3]
    out.update(ref_Jp=M[0], ref_Jc=M[1], ref_Ja=M[2], ref_err=M[3], y2=M[4])
    for n in H.EDGE_COUNTS:
        out["drift_%d" % n] = _drift(F, M, n)
        print("drift", n, out["drift_%d" % n], flush=True)
    # one recorded step and the evaluation at the moved estimates
    rng = np.random.default_rng(22)
    upd_c = rng.normal(size=(g["P"], 6)) * np.array([0.02] * 3 + [0.05] * 3)
    upd_c[:2] = 0.0
    upd_p = rng.normal(size=(g["L"], 3)) * np.array([0.01, 0.01, 0.005])
    upd_p[H.FIXED_POINT] = 0.0
    cams2 = H.mp_oplus(g["cams"], upd_c)
    pts2 = g["pts"] + upd_p
    cams64 = se3expmap.oplus(g["cams"], upd_c)
    cams64[:2] = g["cams"][:2]
    M2 = H.mp_edges(g, cams2, pts2)
    F2 = H.producers(g, cams2, pts2)
    assert M2[4].min() >= 0.5 and np.abs(pts2[g["pt_idx"], 2]).min() >= 0.05
    out.update(step_upd_cams=upd_c, step_upd_pts=upd_p, step_cams=cams2, step_pts=pts2,
               step_oplus_drift=np.array([np.abs(cams64 - cams2).max()]), step_ref_Jp=M2[0], step_ref_Jc=M2[1], step_ref_Ja=M2[2],
               step_ref_err=M2[3])
    for n in H.EDGE_COUNTS:
        out["step_drift_%d" % n] = _drift(F2, M2, n)
        print("step drift", n, out["step_drift_%d" % n], flush=True)
    print("oplus drift", out["step_oplus_drift"], flush=True)
    # LM trajectories over the CPU oracle: fp64-fed against mpmath-fed
    lg = H.lm_graph()
    for name, huber in (("plain", 0.0), ("huber", H.LM_HUBER)):
        a = H.oracle_lm_run(lg, H.fp64_fn(lg), huber=huber)
        b = H.oracle_lm_run(lg, H.mp_fn(lg), huber=huber)
        assert a["trials"] == b["trials"] and a["done"] == b["done"] == H.LM_ITERATIONS, (a["trials"], b["trials"])
        assert np.all(np.diff(a["chis"]) < 0), a["chis"]
        gap = np.abs(a["chis"] - b["chis"]) / np.abs(b["chis"])
        est = max(np.abs(a["cams"] - b["cams"]).max(), np.abs(a["pts"] - b["pts"]).max())
        out.update({"lm_%s_chis" % name: a["chis"], "lm_%s_gap" % name: gap, "lm_%s_trials" % name: np.array(a["trials"]),
                    "lm_%s_estimates" % name: np.array([est])})
        print("lm", name, a["chis"], gap, a["trials"], est, flush=True)
    np.savez_compressed(H.GOLDEN, **out)


if __name__ == "__main__":
    main()
