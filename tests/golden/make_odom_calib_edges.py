"""Generator of tests/golden/odom_calib_edges.npz and of the oracle-drift lines of profiles/odom_calib.jsonl (CPU only; run from the
repository root: python tests/golden/make_odom_calib_edges.py).

ONE graph of 700 EdgeSE2OdomDifferentialCalib edges (odom_calib_helpers.base_graph: 6 robot poses, pose 0 fixed, two parameter
vertices (1.07, 0.94, 1.3) and (0.91, 1.12, 0.8) in rows 6 and 7, no EdgeSE2); the graphs of the edge counts 1, 63, 64, 65, 257, 700
are its first n edges, so one set of arrays serves them all:

  err, Ji, Jj, Jp            odom_calib.py evaluated with mpmath at 60 digits, rounded to fp64 (the Jacobian blocks of the fixed pose
                             are zero, as the device writes them)
  drift [6][4]               per edge count: max abs of the SAME formulas evaluated in fp64 against them, over err, Ji, Jj, Jp (per
                             ARRAY: Jp holds entries of order b S / D^2, far larger than the others').  The GPU tests bound the device
                             against the fp64 restatement by 8 x this figure -- the restatement's own, never the device's
  moved_x, moved_poses, moved_drift   a step over the free vertices (additive on the parameter rows), the moved table and the drift
                             of the errors there (the error-only evaluation of the GPU tests)
  absD, turning              |D| = |vr k_r - vl k_l| at the fixture's estimates and the branch each edge takes
  For the first N_SPECIAL = 40 edges:
  numeric_noise [2]          max abs of the reference's central difference (delta = 1e-9) evaluated at 60 digits against the exact
                             Jacobian at 60 digits -- only the truncation error of the difference remains -- over Ji | Jj and over Jp

Asserted here, on the inputs and in fp64 as the kernel writes the comparisons:
  * NO edge has |D| within 1e-8 max(|vl|, |vr|) of the 1e-7 branch point (there the reference's two probes straddle the branch and
    its numeric Jacobian means nothing): nothing is filtered, zero edges are left out of any comparison;
  * about a fifth of the edges take the straight branch with |D| < 1e-8, every other edge has |D| >= 1e-2; both kinds, both
    parameter vertices and both fixed sides are among the special edges;
  * edges 0 .. 7 have an angle error within 1e-3 of +pi (four) and of -pi (four); every tenth edge is a gross outlier;
  * every normalize_theta argument of the chain stays 1e-6 away from the wrap boundary (a device sin / cos one ulp off must not
    change the branch);
  * the drift of every array is non-zero at every edge count (the graph of one edge is bounded by 8 x the drift of that edge
    alone: an edge whose fp64 evaluation happens to be exact would demand the host libm's bits of the device)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import odom_calib as OC  # noqa: E402
from tests import odom_calib_helpers as H  # noqa: E402


def _margin(theta):
    """distance of theta from the wrap boundary pi + 2 pi k"""
    return abs((theta % (2 * np.pi)) - np.pi)


def assert_inputs(g):
    D, margin = OC.branch_margin(g["poses"], g["op"], g["omeas"])
    assert (margin > 1e-8).all(), margin.min()
    turning = D > OC.BRANCH
    n = len(D)
    assert 0.15 * n <= (~turning).sum() <= 0.25 * n and D[~turning].max() < 1e-8 and D[turning].min() >= 1e-2 * (1 - 1e-12), (D[~turning].max(), D[turning].min())
    nt = lambda t: OC.normalize_theta(OC.FP64, t)
    for k in range(n):
        x1, x2 = g["poses"][g["oi"][k]], g["poses"][g["oj"][k]]
        K = OC.convert_to_motion(OC.FP64, g["omeas"][k] * np.append(g["poses"][g["op"][k]][:2], 1.0), g["poses"][g["op"][k]][2])
        a1 = -K[2]                        # ki
        a2 = -x1[2]                       # w1
        a3 = nt(a1) + nt(a2)              # t = ki w1
        a4 = nt(a3) + x2[2]               # d = t x2
        for a in (a1, a2, a3, a4):
            assert _margin(a) >= 1e-6, (k, a)
    return D, turning


def drift(g, poses=None):
    a, b = H.producers(H.FP64, g, poses), H.producers(H.MP, g, poses)
    return b, [np.abs(a[s] - b[s]).max(axis=1) for s in (3, 0, 1, 2)]


def main():
    out, lines = {}, []
    g = H.base_graph()
    D, turning = assert_inputs(g)
    for k in H.GRAPH_KEYS:
        out[k] = np.asarray(g[k])
    (Mi, Mj, Mp, me), dr = drift(g)
    near = np.abs(me[:8, 2])
    assert (np.pi - near < 1e-3).all() and (me[:8, 2] > 0).sum() == 4 and (me[:8, 2] < 0).sum() == 4, me[:8, 2]
    sp = slice(0, H.N_SPECIAL)
    assert turning[sp].any() and (~turning[sp]).any() and (g["op"][sp] == H.PARAM_ROW_2).any() and (g["oi"][sp] == 0).any() and (g["oj"][sp] == 0).any()
    out.update(err=me, Ji=Mi, Jj=Mj, Jp=Mp, absD=D, turning=turning)
    x = H.update_step(g, 21)
    moved = H.oplus(g, g["poses"], x)
    Dm, marg = OC.branch_margin(moved, g["op"], g["omeas"])
    assert (marg > 1e-8).all() and ((Dm > OC.BRANCH) == turning).sum() < len(D)   # (the moved gains take straight edges into the turning branch)
    e64, emp = H.producers(H.FP64, g, poses=moved, jac=False), H.producers(H.MP, g, poses=moved, jac=False)
    dm = np.abs(e64 - emp).max(axis=1)
    table = np.array([[a[:n].max() for a in dr] for n in H.EDGE_COUNTS])
    assert (table > 0).all() and np.array([dm[:n].max() for n in H.EDGE_COUNTS]).min() > 0, table
    out.update(moved_x=x, moved_poses=moved, drift=table, moved_drift=np.array([dm[:n].max() for n in H.EDGE_COUNTS]))
    for n, row, mv in zip(H.EDGE_COUNTS, table, out["moved_drift"]):
        lines.append(dict(kind="oracle_drift", graph="odom_calib_%d" % n, edges=int(n), err=float(row[0]), Ji=float(row[1]), Jj=float(row[2]),
                          Jp=float(row[3]), moved_err=float(mv), err_max_abs=float(np.abs(me[:n]).max()),
                          Jp_max_abs=float(np.abs(Mp[:n]).max())))
        print(lines[-1], flush=True)
    s = H.take_edges(g, sp)
    nd = OC.numeric_edges(H.MP, s["poses"], s["oi"], s["oj"], s["op"], s["omeas"])
    noise = [0.0, 0.0]
    for k in range(H.N_SPECIAL):
        Js = OC.odom_calib_jacobians(H.MP, s["poses"][s["oi"][k]], s["poses"][s["oj"][k]], s["poses"][s["op"][k]], s["omeas"][k])
        for side in range(3):
            for r in range(3):
                for c in range(3):
                    noise[side // 2] = max(noise[side // 2], abs(float(nd[side][k][r + 3 * c] - Js[side][r][c])))
    out.update(numeric_noise=np.array(noise))
    lines.append(dict(kind="numeric_jacobian_truncation", delta=1e-9, max_abs_poses=noise[0], max_abs_params=noise[1],
                      Jp_max_abs=float(np.abs(Mp[sp]).max())))
    print(lines[-1], flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "odom_calib_edges.npz"), **out)
    path = os.path.join(ROOT, "profiles", "odom_calib.jsonl")
    keep = []
    if os.path.exists(path):
        keep = [l for l in open(path).read().splitlines() if l.strip() and json.loads(l).get("kind") not in ("oracle_drift", "numeric_jacobian_truncation")]
    with open(path, "w") as f:
        for l in keep:
            f.write(l + "\n")
        for l in lines:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
