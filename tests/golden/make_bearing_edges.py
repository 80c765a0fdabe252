"""Generator of tests/golden/bearing_edges.npz and of the oracle-drift lines of profiles/bearing_slam.jsonl (CPU only; run from the
repository root: python tests/golden/make_bearing_edges.py).  Needs the built CPU oracle (make -C oracle).

ONE graph of 300 bearing edges (bearing_helpers.base_graph: 4 poses with angles in the four quadrants, pose 0 fixed, 3 odometry
edges, 6 landmarks of which one is fixed, 24 EdgeSE2PointXY observations for the mixed tests); the graphs of the edge counts 1, 63,
64, 65, 255, 256, 257, 300 are its first n edges (one lane per edge, 64 lanes per wave, 256 threads per block: either side of a
wave and of a block, and a partial last block), so one set of arrays serves them all:

  graph_*                    the graph
  err, J0, J1                bearing.py evaluated with mpmath at 60 digits, rounded to fp64
  drift [8][2]               per edge count: max abs of the SAME formulas evaluated in fp64 against them, over err and over J0 | J1.
                             The GPU tests bound the device against the fp64 restatement by 8 x this figure -- the restatement's
                             own, never the device's
  moved_x, moved_poses, moved_points, moved_drift   a step over the free poses and landmarks (the oracle's oplus and plain
                             addition), the moved estimates and the drift of the errors there (the error-only evaluation)
  numeric_noise              max abs of the reference's central difference (delta = 1e-9) evaluated at 60 digits against the
                             analytic Jacobian at 60 digits -- only the truncation error of the difference remains
  lm_<mode>_*                synthetic.make_bearing_slam (bearing-only and beside the Cartesian observations): LM_ITERATIONS
                             iterations of lm.optimize over the CPU oracle fed by bearing.py, once with the oracle's solver and once
                             solving densely: the trials of both (asserted equal, with at least one rejected step), chi2 per
                             iteration, their relative gap, the pose error of the initial guess and of the result

Asserted here, on the inputs and in fp64 as the kernel writes the comparisons (the seed is chosen so that they hold):
  - every observation distance is at least 0.5, before and after the move; the pose angles cover the four quadrants
  - z - angle takes each of the wrap branches "in", "floor" (z - angle < -pi) and "floor+hi" (z - angle >= pi) in at least 10 edges,
    before and after the move the same branch per edge
  - no edge has |e| within 1e-6 of pi, before or after the move, and no central difference straddles the wrap: no edge needs to
    be excluded anywhere
  - the drift of the errors of the first edge is not zero, before or after the move: 8 x 0 would ask the device's sin, cos and
    atan2 for the bits of this host's libm, which no property of the formats supports"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import bearing as BE  # noqa: E402
from tests import bearing_helpers as H  # noqa: E402
from tests.producer_metric import wrap_branch  # noqa: E402


def raw_angles(g, poses, points):
    """z - atan2(deltay, deltax) in fp64, as the kernel forms it, and the distances."""
    raw, dist = [], []
    for k in range(len(g["bp"])):
        X, L = poses[g["bp"][k]], points[g["bl"][k]]
        c, s = np.cos(X[2]), np.sin(X[2])
        dx, dy = L[0] - X[0], L[1] - X[1]
        raw.append(g["zb"][k] - np.arctan2(-s * dx + c * dy, c * dx + s * dy))
        dist.append(np.hypot(dx, dy))
    return np.array(raw), np.array(dist)


def check_inputs(g, moved):
    """The assertions of the module docstring; returns the branch counts, or raises AssertionError."""
    quadrants = {(bool(np.cos(t) > 0), bool(np.sin(t) > 0)) for t in g["poses"][:, 2]}
    assert len(quadrants) == 4, quadrants
    branches = []
    for poses, points in ((g["poses"], g["points"]), moved):
        raw, dist = raw_angles(g, poses, points)
        assert dist.min() >= H.MIN_DISTANCE, dist.min()
        e = np.array([float(BE.normalize_theta(BE.FP64, r)) for r in raw])
        assert (np.pi - np.abs(e)).min() >= 1e-6
        branches.append([wrap_branch(r) for r in raw])
    assert branches[0] == branches[1]
    counts = {b: branches[0].count(b) for b in ("in", "floor", "floor+hi")}
    assert min(counts.values()) >= 10 and sum(counts.values()) == len(g["bp"]), counts
    return counts


def find_seed(limit=200):
    for seed in range(limit):
        g = H.base_graph(seed=seed)
        try:
            check_inputs(g, H.oplus(g, g["poses"], g["points"], H.update_step(g, 21)))
        except AssertionError:
            continue
        e64, emp = H.producers(H.FP64, H.take_edges(g, slice(0, 1)), jac=False), H.producers(H.MP, H.take_edges(g, slice(0, 1)), jac=False)
        mp, mq = H.oplus(g, g["poses"], g["points"], H.update_step(g, 21))
        f64, fmp = (H.producers(F, H.take_edges(g, slice(0, 1)), mp, mq, jac=False) for F in (H.FP64, H.MP))
        if e64[0, 0] != emp[0, 0] and f64[0, 0] != fmp[0, 0]:
            return seed
    raise SystemExit("no seed below %d meets the assertions" % limit)


def main():
    if "--find-seed" in sys.argv:
        print("seed", find_seed())
        return
    out, lines = {}, []
    g = H.base_graph()
    x = H.update_step(g, 21)
    moved = H.oplus(g, g["poses"], g["points"], x)
    counts = check_inputs(g, moved)
    print("branches", counts, flush=True)
    for k in H.GRAPH_KEYS:
        out["graph_" + k] = np.asarray(g[k])
    a, b = H.producers(H.FP64, g), H.producers(H.MP, g)
    de, dJ = np.abs(a[2] - b[2]).max(axis=1), np.maximum(np.abs(a[0] - b[0]).max(axis=1), np.abs(a[1] - b[1]).max(axis=1))
    out.update(J0=b[0], J1=b[1], err=b[2])
    e64, emp = (H.producers(F, g, moved[0], moved[1], jac=False) for F in (H.FP64, H.MP))
    dm = np.abs(e64 - emp).max(axis=1)
    assert de[0] > 0 and dm[0] > 0, (de[0], dm[0])
    out.update(moved_x=x, moved_poses=moved[0], moved_points=moved[1],
               drift=np.array([[de[:n].max(), dJ[:n].max()] for n in H.EDGE_COUNTS]),
               moved_drift=np.array([dm[:n].max() for n in H.EDGE_COUNTS]), moved_err=emp)
    for n, row, mv in zip(H.EDGE_COUNTS, out["drift"], out["moved_drift"]):
        lines.append(dict(kind="oracle_drift", graph="bearing_%d" % n, edges=int(n), err=float(row[0]), J=float(row[1]), moved_err=float(mv),
                          err_max_abs=float(np.abs(b[2][:n]).max()), J_max_abs=float(max(np.abs(b[0][:n]).max(), np.abs(b[1][:n]).max()))))
        print(lines[-1], flush=True)
    N0, N1 = BE.numeric_edges(H.MP, g["poses"], g["points"], g["bp"], g["bl"], g["zb"])
    noise = 0.0   # (against the analytic Jacobian at 60 digits, unrounded)
    for k in range(len(g["bp"])):
        A, B = BE.bearing_jacobians(H.MP, g["poses"][g["bp"][k]], g["points"][g["bl"][k]])
        noise = max(noise, max(abs(float(n_ - a_)) for n_, a_ in zip(list(N0[k]) + list(N1[k]), A + B)))
    out["numeric_noise"] = np.array(noise)
    lines.append(dict(kind="numeric_jacobian_truncation", delta=1e-9, max_abs=noise))
    print(lines[-1], flush=True)
    for mode in H.MODES:
        key = "bearing" if mode == "bearing-only" else "mixed"
        lg = H.lm_graph(mode)
        ra = H.oracle_lm_run(lg, lambda_init=H.LM_LAMBDA[mode])
        rb = H.oracle_lm_run(lg, dense=True, lambda_init=H.LM_LAMBDA[mode])
        assert ra["trials"] == rb["trials"] and ra["done"] == rb["done"] == H.LM_ITERATIONS, (ra["trials"], rb["trials"])
        gap = np.abs(ra["chis"] - rb["chis"]) / np.abs(rb["chis"])
        e0, e1 = H.pose_error(lg, lg["poses"]), H.pose_error(lg, ra["poses"])
        assert max(ra["trials"]) > 1 and e1 < e0 and ra["chis"][-1] < ra["chis"][0], (ra["chis"], ra["trials"], e0, e1)
        out.update({"lm_%s_chis" % key: ra["chis"], "lm_%s_gap" % key: gap, "lm_%s_trials" % key: np.array(ra["trials"]),
                    "lm_%s_pose_error" % key: np.array([e0, e1]), "lm_%s_poses" % key: ra["poses"], "lm_%s_poses_dense" % key: rb["poses"]})
        lines.append(dict(kind="oracle_lm", graph=mode, landmarks=int(lg["L"]), bearings=int(lg["B"]), xy=int(lg["M"]), trials=ra["trials"],
                          chis=ra["chis"].tolist(), gap=gap.tolist(), pose_error=[e0, e1], poses_gap=float(np.abs(ra["poses"] - rb["poses"]).max())))
        print(lines[-1], flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "bearing_edges.npz"), **out)
    path = os.path.join(ROOT, "profiles", "bearing_slam.jsonl")
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
