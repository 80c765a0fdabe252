"""Generator of tests/golden/pointxy_calib_edges.npz and of the oracle-drift lines of profiles/pointxy_calib.jsonl (CPU only; run
from the repository root: python tests/golden/make_pointxy_calib_edges.py).  Needs the built CPU oracle (make -C oracle).

ONE graph of 700 EdgeSE2PointXYCalib edges (pointxy_calib_helpers.base_graph: 6 robot poses, pose 0 fixed, 12 landmarks, landmark 0
fixed, 5 odometry edges, the calibration vertex in row 6, one with a large lever arm |tc| = 40 in row 7 and one with thc == 0 in row
8); the graphs of the edge counts 1, 255, 256, 257, 700 are its first n edges (one lane per edge, 256 threads per workgroup: one
edge, either side of a workgroup, and a partial last workgroup of 188), so one set of arrays serves them all:

  err, Jp, Jl, Jc            pointxy_calib.py evaluated with mpmath at 60 digits, rounded to fp64 (the Jacobian blocks of fixed
                             vertices are zero, as the device writes them)
  drift [5][2]               per edge count: max abs of the SAME formulas evaluated in fp64 against them, over err and over Jp | Jl |
                             Jc.  The GPU tests bound the device against the fp64 restatement by 8 x this figure -- the
                             restatement's own, never the device's
  moved_x, moved_poses, moved_points, moved_err, moved_drift   a step over the free vertices (the oracle's oplus), the moved
                             estimates, the 60-digit errors there and the drift of the fp64 errors (the error-only evaluation of
                             the GPU tests)
  The first N_SPECIAL = 48 edges are the golden edges proper.  For them:
  cd60_Jp, _Jl, _Jc          the central difference of the 60-digit error with step 1e-25 (truncation ~1e-50, far below fp64
                             rounding), rounded to fp64, blocks of fixed vertices included
  cd60_gap                   max abs of cd60 against the exact Jacobian at 60 digits: what rounding cd60 to fp64 leaves
  numeric_noise              max abs of the reference's central difference (delta = 1e-9) evaluated at 60 digits against the exact
                             Jacobian at 60 digits -- only the truncation error of the difference remains
  lm_*                       synthetic.make_pointxy_calib_slam(**LM_ARGS): LM_ITERATIONS iterations of lm.optimize over the CPU
                             oracle (add_multi_edge_set) fed by pointxy_calib.py, once with the oracle's Schur solver and once
                             solving densely: the trials of both (asserted equal), chi2 per iteration, their relative gap, the
                             error of the offset at the initial guess and at the result

Asserted here, on the inputs and in fp64 as the kernel writes the comparisons:
  * th1 + thc falls inside [-pi, pi), at or above pi and below -pi (the wrap in both directions);
  * the argument of every normalize_theta of the chain stays 1e-6 away from the boundary (a device sin / cos one ulp off must not
    change the branch);
  * the drift of edge 0 is at least one eps of its largest entry (the graph of one edge is bounded by 8 x that drift alone);
  * the special edges hold the lever-arm vertex and an edge with thc == 0."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import pointxy_calib as PC  # noqa: E402
from tests import pointxy_calib_helpers as H  # noqa: E402


def _margin(theta):
    """distance of theta from the wrap boundary pi + 2 pi k"""
    return abs((theta % (2 * np.pi)) - np.pi)


def assert_branches(g):
    seen = set()
    nt = lambda t: PC.normalize_theta(PC.FP64, t)
    for k in range(len(g["qp"])):
        raw = g["poses"][g["qp"][k]][2] + g["poses"][g["qc"][k]][2]     # a = x1 c
        seen.add("above" if raw >= np.pi else "below" if raw < -np.pi else "in")
        for a in (raw, -nt(raw)):                                       # ... and w = a^-1
            assert _margin(a) >= 1e-6, (k, a)
    assert seen == {"in", "above", "below"}, seen
    return sorted(seen)


def drift(g, poses=None, points=None):
    a, b = H.producers(H.FP64, g, poses, points), H.producers(H.MP, g, poses, points)
    dJ = np.maximum.reduce([np.abs(a[s] - b[s]).max(axis=1) for s in range(3)])
    return b, (np.abs(a[3] - b[3]).max(axis=1), dJ)


def main():
    out, lines = {}, []
    g = H.base_graph()
    print("branches", assert_branches(g), flush=True)
    for k in H.GRAPH_KEYS:
        out[k] = np.asarray(g[k])
    (Mp, Ml, Mc, me), (de, dJ) = drift(g)
    eps = float(np.finfo(np.float64).eps)   # (the n = 1 graph is edge 0 alone: its drift must show the rounding level of the formulas)
    assert de[0] >= eps * np.abs(me[0]).max() and dJ[0] >= eps * max(np.abs(M[0]).max() for M in (Mp, Ml, Mc)), (de[0], dJ[0])
    sp = H.take_edges(g, slice(0, H.N_SPECIAL))
    assert (sp["qc"] == H.LEVER_ROW).any() and abs(np.hypot(*g["poses"][H.LEVER_ROW][:2]) - 40.0) < 1e-9
    assert (sp["qc"] == H.ZERO_ROW).any() and g["poses"][H.ZERO_ROW][2] == 0.0
    assert (sp["qp"] == 0).any() and (sp["ql"] == 0).any()                 # the fixed pose and the fixed landmark
    out.update(err=me, Jp=Mp, Jl=Ml, Jc=Mc)
    x = H.update_step(g, 21)
    mp_, mq_ = H.oplus(g, g["poses"], g["points"], x)
    e64, emp = H.producers(H.FP64, g, mp_, mq_, jac=False), H.producers(H.MP, g, mp_, mq_, jac=False)
    dm = np.abs(e64 - emp).max(axis=1)
    out.update(moved_x=x, moved_poses=mp_, moved_points=mq_, moved_err=emp,
               drift=np.array([[de[:n].max(), dJ[:n].max()] for n in H.EDGE_COUNTS]), moved_drift=np.array([dm[:n].max() for n in H.EDGE_COUNTS]))
    for n, row, mv in zip(H.EDGE_COUNTS, out["drift"], out["moved_drift"]):
        lines.append(dict(kind="oracle_drift", graph="pointxy_calib_%d" % n, edges=int(n), err=float(row[0]), J=float(row[1]), moved_err=float(mv),
                          err_max_abs=float(np.abs(me[:n]).max()), J_max_abs=float(max(np.abs(M[:n]).max() for M in (Mp, Ml, Mc)))))
        print(lines[-1], flush=True)
    # the golden edges proper: the exact Jacobian at 60 digits against two central differences of the 60-digit error
    args = (sp["poses"], sp["points"], sp["qp"], sp["ql"], sp["qc"], sp["zq"])
    cd = PC.numeric_edges(H.MP, *args, delta=H.MP.num(10) ** -25)
    nd = PC.numeric_edges(H.MP, *args)
    cd64 = [np.array([[float(v) for v in row] for row in N]) for N in cd]
    gap = noise = 0.0
    for k in range(H.N_SPECIAL):
        Js = PC.pointxy_calib_jacobians(H.MP, sp["poses"][sp["qp"][k]], sp["points"][sp["ql"][k]], sp["poses"][sp["qc"][k]], sp["zq"][k])
        for side, dim in enumerate((3, 2, 3)):
            for r in range(2):
                for c in range(dim):
                    gap = max(gap, abs(float(H.MP.num(cd64[side][k][r + 2 * c]) - Js[side][r][c])))
                    noise = max(noise, abs(float(nd[side][k][r + 2 * c] - Js[side][r][c])))
    out.update(cd60_Jp=cd64[0], cd60_Jl=cd64[1], cd60_Jc=cd64[2], cd60_gap=np.array(gap), numeric_noise=np.array(noise))
    lines.append(dict(kind="numeric_jacobian_truncation", delta=1e-9, max_abs=noise, cd60_gap=gap))
    print(lines[-1], flush=True)
    lg = H.lm_graph()
    a = H.oracle_lm_run(lg)
    b = H.oracle_lm_run(lg, dense=True)
    assert a["trials"] == b["trials"] and a["done"] == b["done"] == H.LM_ITERATIONS, (a["trials"], b["trials"])
    gapc = np.abs(a["chis"] - b["chis"]) / np.abs(b["chis"])
    e0, e1 = H.offset_error(lg, lg["poses"]), H.offset_error(lg, a["poses"])
    assert e1[0] <= H.LM_ARGS["noise"] and e1[0] < e0[0] and e1[1] < e0[1] and a["chis"][-1] < a["chis"][0] and gapc.max() > 0, \
        (a["chis"], a["trials"], e0, e1, gapc)
    out.update(lm_chis=a["chis"], lm_gap=gapc, lm_trials=np.array(a["trials"]), lm_offset_error=np.array([e0, e1]), lm_poses=a["poses"],
               lm_poses_dense=b["poses"])
    lines.append(dict(kind="oracle_lm", trials=a["trials"], chis=a["chis"].tolist(), gap=gapc.tolist(), offset_error=[list(e0), list(e1)],
                      poses_gap=float(np.abs(a["poses"] - b["poses"]).max())))
    print(lines[-1], flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "pointxy_calib_edges.npz"), **out)
    path = os.path.join(ROOT, "profiles", "pointxy_calib.jsonl")
    keep = []
    if os.path.exists(path):
        keep = [l for l in open(path).read().splitlines() if l.strip() and json.loads(l).get("kind") not in ("oracle_drift", "numeric_jacobian_truncation", "oracle_lm")]
    with open(path, "w") as f:
        for l in keep:
            f.write(l + "\n")
        for l in lines:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
