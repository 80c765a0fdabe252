"""Generator of tests/golden/sensor_calib_edges.npz and of the oracle-drift lines of profiles/sensor_calib.jsonl (CPU only; run from
the repository root: python tests/golden/make_sensor_calib_edges.py).  Needs the built CPU oracle (make -C oracle).

ONE graph of 700 EdgeSE2SensorCalib edges (calib_helpers.base_graph: 6 robot poses, pose 0 fixed, poses 2 and 3 of exactly the same
angle, 5 odometry edges, the laser offset in row 6 and an offset with a large lever arm |tl| ~ 47 in row 7); the graphs of the edge
counts 1, 255, 256, 257, 700 are its first n edges (one lane per edge, 256 threads per workgroup: one edge, either side of a
workgroup, and a partial last workgroup of 188), so one set of arrays serves them all:

  err, Ji, Jj, Jl            sensor_calib.py evaluated with mpmath at 60 digits, rounded to fp64 (the Jacobian blocks of the fixed
                             pose are zero, as the device writes them)
  drift [5][2]               per edge count: max abs of the SAME formulas evaluated in fp64 against them, over err and over Ji | Jj |
                             Jl.  The GPU tests bound the device against the fp64 restatement by 8 x this figure -- the
                             restatement's own, never the device's
  moved_x, moved_poses, moved_drift   a step over the free vertices (the oracle's oplus), the moved poses and the drift of the errors
                             there (the error-only evaluation of the GPU tests)
  The first N_SPECIAL = 48 edges are the golden edges proper.  For them:
  cd60_Ji, _Jj, _Jl          the central difference of the 60-digit error with step 1e-25 (truncation ~1e-50, far below fp64
                             rounding), rounded to fp64, blocks of the fixed pose included
  cd60_gap                   max abs of cd60 against the exact Jacobian at 60 digits: what rounding cd60 to fp64 leaves
  numeric_noise              max abs of the reference's central difference (delta = 1e-9) evaluated at 60 digits against the exact
                             Jacobian at 60 digits -- only the truncation error of the difference remains
  lm_*                       synthetic.make_calib_rig(**LM_ARGS): LM_ITERATIONS iterations of lm.optimize over the CPU oracle
                             (add_multi_edge_set) fed by sensor_calib.py, once with the oracle's solver and once solving densely:
                             the trials of both (asserted equal), chi2 per iteration, their relative gap (two equally valid runs
                             agree to a few 1e-15 and in single iterations to the last bit: the GPU test takes the run's LARGEST
                             gap as the scale of every iteration), the error of the laser offset at the initial guess and at the
                             result

Asserted here, on the inputs and in fp64 as the kernel writes the comparisons:
  * edges 0 .. 7 have an angle error within 1e-3 of +pi (four) and of -pi (four);
  * the special edges hold a pair with th1 == th2 (the block d e_t / d tl is exactly zero) and the large lever arm;
  * the raw angle th2 - th1 - thz lands on every branch of the wrap, and it, like the argument of every normalize_theta of the
    chain, stays 1e-6 away from the boundary (a device sin / cos one ulp off must not change the branch);
  * the drift of edge 0 is at least one eps of its largest entry (the graph of one edge is bounded by 8 x that drift alone: an edge
    whose fp64 evaluation happens to be exact would demand the host libm's bits of the device)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import sensor_calib as SC  # noqa: E402
from tests import calib_helpers as H  # noqa: E402
from tests.producer_metric import wrap_branch  # noqa: E402


def _margin(theta):
    """distance of theta from the wrap boundary pi + 2 pi k"""
    return abs((theta % (2 * np.pi)) - np.pi)


def assert_branches(g):
    seen = set()
    nt = lambda t: SC.normalize_theta(SC.FP64, t)
    for k in range(len(g["ci"])):
        x1, x2, L, z = g["poses"][g["ci"][k]], g["poses"][g["cj"][k]], g["poses"][g["cl"][k]], g["cmeas"][k]
        raw = x2[2] - x1[2] - z[2]
        seen.add(wrap_branch(raw))
        a1 = x1[2] + L[2]            # a = x1 L
        a2 = -nt(a1)                 # w = a^-1
        a3 = nt(a2) + x2[2]          # b = w x2
        a4 = nt(a3) + L[2]           # c = b L
        a5 = -z[2]                   # invm
        a6 = nt(a5) + nt(a4)         # d = invm c
        for a in (raw, a1, a2, a3, a4, a5, a6):
            assert _margin(a) >= 1e-6, (k, a)
    assert seen >= {"in", "floor", "floor+hi"}, seen
    return sorted(seen)


def drift(g, poses=None):
    a, b = H.producers(H.FP64, g, poses), H.producers(H.MP, g, poses)
    dJ = np.maximum.reduce([np.abs(a[s] - b[s]).max(axis=1) for s in range(3)])
    return b, (np.abs(a[3] - b[3]).max(axis=1), dJ)


def main():
    out, lines = {}, []
    g = H.base_graph()
    print("branches", assert_branches(g), flush=True)
    for k in H.GRAPH_KEYS:
        out[k] = np.asarray(g[k])
    (Mi, Mj, Ml, me), (de, dJ) = drift(g)
    eps = float(np.finfo(np.float64).eps)   # (the n = 1 graph is edge 0 alone: its drift must show the rounding level of the formulas)
    assert de[0] >= eps * np.abs(me[0]).max() and dJ[0] >= eps * max(np.abs(M[0]).max() for M in (Mi, Mj, Ml)), (de[0], dJ[0])
    near = np.abs(me[:8, 2])
    assert (np.pi - near < 1e-3).all() and (me[:8, 2] > 0).sum() == 4 and (me[:8, 2] < 0).sum() == 4, me[:8, 2]
    sp = H.take_edges(g, slice(0, H.N_SPECIAL))
    same = g["poses"][sp["ci"], 2] == g["poses"][sp["cj"], 2]
    assert same.any() and (np.abs(Ml[:H.N_SPECIAL][same][:, [0, 1, 3, 4]]).max() == 0.0)
    assert (sp["cl"] == H.LEVER_ROW).any() and np.hypot(*g["poses"][H.LEVER_ROW][:2]) > 40
    out.update(err=me, Ji=Mi, Jj=Mj, Jl=Ml)
    x = H.update_step(g, 21)
    moved = H.oplus(g, g["poses"], x)
    e64, emp = H.producers(H.FP64, g, poses=moved, jac=False), H.producers(H.MP, g, poses=moved, jac=False)
    dm = np.abs(e64 - emp).max(axis=1)
    out.update(moved_x=x, moved_poses=moved, drift=np.array([[de[:n].max(), dJ[:n].max()] for n in H.EDGE_COUNTS]),
               moved_drift=np.array([dm[:n].max() for n in H.EDGE_COUNTS]))
    for n, row, mv in zip(H.EDGE_COUNTS, out["drift"], out["moved_drift"]):
        lines.append(dict(kind="oracle_drift", graph="calib_%d" % n, edges=int(n), err=float(row[0]), J=float(row[1]), moved_err=float(mv),
                          err_max_abs=float(np.abs(me[:n]).max()), J_max_abs=float(max(np.abs(M[:n]).max() for M in (Mi, Mj, Ml)))))
        print(lines[-1], flush=True)
    # the golden edges proper: the exact Jacobian at 60 digits against two central differences of the 60-digit error
    cd = SC.numeric_edges(H.MP, sp["poses"], sp["ci"], sp["cj"], sp["cl"], sp["cmeas"], delta=H.MP.num(10) ** -25)
    nd = SC.numeric_edges(H.MP, sp["poses"], sp["ci"], sp["cj"], sp["cl"], sp["cmeas"])
    cd64 = [np.array([[float(v) for v in row] for row in N]) for N in cd]
    gap = noise = 0.0
    for k in range(H.N_SPECIAL):
        Js = SC.calib_jacobians(H.MP, sp["poses"][sp["ci"][k]], sp["poses"][sp["cj"][k]], sp["poses"][sp["cl"][k]], sp["cmeas"][k])
        for side in range(3):
            for r in range(3):
                for c in range(3):
                    gap = max(gap, abs(float(H.MP.num(cd64[side][k][r + 3 * c]) - Js[side][r][c])))
                    noise = max(noise, abs(float(nd[side][k][r + 3 * c] - Js[side][r][c])))
    out.update(cd60_Ji=cd64[0], cd60_Jj=cd64[1], cd60_Jl=cd64[2], cd60_gap=np.array(gap), numeric_noise=np.array(noise))
    lines.append(dict(kind="numeric_jacobian_truncation", delta=1e-9, max_abs=noise, cd60_gap=gap))
    print(lines[-1], flush=True)
    lg = H.lm_graph()
    a = H.oracle_lm_run(lg)
    b = H.oracle_lm_run(lg, dense=True)
    assert a["trials"] == b["trials"] and a["done"] == b["done"] == H.LM_ITERATIONS, (a["trials"], b["trials"])
    gapc = np.abs(a["chis"] - b["chis"]) / np.abs(b["chis"])
    e0, e1 = H.offset_error(lg, lg["poses"]), H.offset_error(lg, a["poses"])
    assert e1[0] <= H.LM_ARGS["noise"][0] and e1[1] <= H.LM_ARGS["noise"][1], e1
    assert e1[0] < e0[0] and e1[1] < e0[1] and a["chis"][-1] < a["chis"][0] and gapc.max() > 0, (a["chis"], a["trials"], e0, e1, gapc)
    out.update(lm_chis=a["chis"], lm_gap=gapc, lm_trials=np.array(a["trials"]), lm_offset_error=np.array([e0, e1]), lm_poses=a["poses"],
               lm_poses_dense=b["poses"])
    lines.append(dict(kind="oracle_lm", trials=a["trials"], chis=a["chis"].tolist(), gap=gapc.tolist(), offset_error=[list(e0), list(e1)],
                      poses_gap=float(np.abs(a["poses"] - b["poses"]).max())))
    print(lines[-1], flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sensor_calib_edges.npz"), **out)
    path = os.path.join(ROOT, "profiles", "sensor_calib.jsonl")
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
