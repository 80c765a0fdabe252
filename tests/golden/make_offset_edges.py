"""Generator of tests/golden/offset_edges.npz and of the oracle-drift lines of profiles/offset_edges.jsonl (CPU only; run from the
repository root: python tests/golden/make_offset_edges.py).  Needs the built CPU oracle (make -C oracle).

Per kind (se2 = EdgeSE2Offset, type 18; se3 = EdgeSE3Offset, type 19) ONE graph of 300 offset edges (offset_helpers.base_graph: 4
poses, pose 0 fixed, 3 odometry edges, 3 parameter rows -- the identity, a rotation above 90 degrees, a general frame); the graphs
of the edge counts 1, 63, 64, 65, 255, 256, 257, 300 are its first n edges (one lane per edge, 64 lanes per wave, 256 threads per
block: either side of a wave and of a block, and a partial last block), so one set of arrays serves them all:

  <kind>_err, _J0, _J1       offset_edges.py evaluated with mpmath at 60 digits, rounded to fp64
  <kind>_drift [8][2]        per edge count: max abs of the SAME formulas evaluated in fp64 against them, over err and over J0 | J1.
                             The GPU tests bound the device against the fp64 restatement by 8 x this figure -- the restatement's own,
                             never the device's
  <kind>_moved_x, _moved_poses, _moved_drift   a step over the free poses (the oracle's oplus), the moved poses and the drift of
                             the errors there (the error-only evaluation of the GPU tests)
  se2_numeric_noise          type 18: max abs of the reference's central difference (delta = 1e-9) evaluated at 60 digits against
                             the analytic Jacobian at 60 digits -- only the truncation error of the difference remains
  lm_<kind>_*                synthetic.make_offset_rig(**LM_ARGS): LM_ITERATIONS iterations of lm.optimize over the CPU oracle fed by
                             offset_edges.py, once with the oracle's solver and once solving densely: the trials of both (asserted
                             equal, with at least one rejected step), chi2 per iteration, their relative gap, the pose error of the
                             initial guess and of the result

Asserted here, on the inputs and in fp64 as the kernels write the comparisons:
  se3   the 300 edges reach every outcome of pg_R_to_quat / pg_dq_dR that exists: trace > 0 (where qw = sqrt(tr + 1) / 2 is always
        positive) and the three largest-diagonal cases, each with the case's qw of either sign; in the largest-diagonal cases the
        two largest diagonal entries differ by at least 1e-3 (a tie could send device and reference down different branches)
  se2   thj + aj - thi - ai - thz lands on every branch of the wrap -- inside [-pi, pi), reduced by the floor, reduced to at least
        pi and brought back -- and it, like the argument of every normalize_theta of the chain, stays 1e-6 away from the boundary"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import offset_edges as OE  # noqa: E402
from tests import offset_helpers as H  # noqa: E402
from tests.producer_metric import wrap_branch  # noqa: E402


def assert_se3_branches(g):
    seen = set()
    for k in range(len(g["oi"])):
        R, _ = OE.se3_delta(OE.FP64, g["poses"][g["oi"][k]], g["poses"][g["oj"][k]], g["omeas"][k], g["offsets"][g["opf"][k]], g["offsets"][g["opt"][k]])
        case = OE.quat_case(OE.FP64, R)
        seen.add(case)
        if case[0] > 0:
            d = sorted([R[0][0], R[1][1], R[2][2]])
            assert d[2] - d[1] >= 1e-3, (k, d)
    want = {(0, 1)} | {(c, s) for c in (1, 2, 3) for s in (1, -1)}
    assert seen == want, sorted(want - seen)
    return sorted(seen)


def _margin(theta):
    """distance of theta from the wrap boundary pi + 2 pi k"""
    return abs((theta % (2 * np.pi)) - np.pi)


def assert_se2_branches(g):
    seen = set()
    for k in range(len(g["oi"])):
        xi, xj, z = g["poses"][g["oi"][k]], g["poses"][g["oj"][k]], g["omeas"][k]
        pi, pj = g["offsets"][g["opf"][k]], g["offsets"][g["opt"][k]]
        raw = xj[2] + pj[2] - xi[2] - pi[2] - z[2]
        seen.add(wrap_branch(raw))
        nt = lambda t: OE.normalize_theta(OE.FP64, t)
        a1 = xi[2] + pi[2]
        a2 = -nt(a1)
        a3 = -z[2]
        a4 = nt(a3) + nt(a2)
        a5 = xj[2] + pj[2]
        a6 = nt(a4) + nt(a5)
        for a in (raw, a1, a2, a3, a4, a5, a6):
            assert _margin(a) >= 1e-6, (k, a)
    assert seen >= {"in", "floor", "floor+hi"}, seen
    return sorted(seen)


def drift(g):
    a, b = H.producers(H.FP64, g), H.producers(H.MP, g)
    return b, (np.abs(a[2] - b[2]), np.maximum(np.abs(a[0] - b[0]).max(axis=1), np.abs(a[1] - b[1]).max(axis=1)))


def main():
    out, lines = {}, []
    for kind, _ in H.KINDS:
        g = H.base_graph(kind)
        branches = assert_se3_branches(g) if kind == "se3" else assert_se2_branches(g)
        print(kind, "branches", branches, flush=True)
        for k in H.GRAPH_KEYS:
            out["%s_%s" % (kind, k)] = np.asarray(g[k])
        (M0, M1, me), (de, dJ) = drift(g)
        out.update({kind + "_J0": M0, kind + "_J1": M1, kind + "_err": me})
        x = H.update_step(g, 21)
        moved = H.oplus(g, g["poses"], x)
        e64, emp = H.producers(H.FP64, g, poses=moved, jac=False), H.producers(H.MP, g, poses=moved, jac=False)
        dm = np.abs(e64 - emp)
        out.update({kind + "_moved_x": x, kind + "_moved_poses": moved,
                    kind + "_drift": np.array([[de[:n].max(), dJ[:n].max()] for n in H.EDGE_COUNTS]),
                    kind + "_moved_drift": np.array([dm[:n].max() for n in H.EDGE_COUNTS])})
        for n, row, mv in zip(H.EDGE_COUNTS, out[kind + "_drift"], out[kind + "_moved_drift"]):
            lines.append(dict(kind="oracle_drift", graph="%s_%d" % (kind, n), edges=int(n), err=float(row[0]), J=float(row[1]), moved_err=float(mv),
                              err_max_abs=float(np.abs(me[:n]).max()), J_max_abs=float(max(np.abs(M0[:n]).max(), np.abs(M1[:n]).max()))))
            print(lines[-1], flush=True)
        if kind == "se2":
            N0, N1 = OE.numeric_edges(H.MP, g["poses"], g["oi"], g["oj"], g["opf"], g["opt"], g["omeas"], g["offsets"])
            noise = 0.0   # (against the analytic Jacobian at 60 digits, unrounded)
            for k in range(len(g["oi"])):
                args = (g["poses"][g["oi"][k]], g["poses"][g["oj"][k]], g["omeas"][k], g["offsets"][g["opf"][k]], g["offsets"][g["opt"][k]])
                Ji, Jj = OE.se2_jacobians(H.MP, *args)
                for J, N in ((Ji, N0[k]), (Jj, N1[k])):
                    noise = max(noise, max(abs(float(N[r + 3 * c] - J[r][c])) for r in range(3) for c in range(3)))
            out["se2_numeric_noise"] = np.array(noise)
            lines.append(dict(kind="numeric_jacobian_truncation", delta=1e-9, max_abs=noise))
            print(lines[-1], flush=True)
        lg = H.lm_graph(kind)
        a = H.oracle_lm_run(lg, lambda_init=H.LM_LAMBDA[kind])
        b = H.oracle_lm_run(lg, dense=True, lambda_init=H.LM_LAMBDA[kind])
        assert a["trials"] == b["trials"] and a["done"] == b["done"] == H.LM_ITERATIONS, (a["trials"], b["trials"])
        gap = np.abs(a["chis"] - b["chis"]) / np.abs(b["chis"])
        e0, e1 = H.pose_error(lg, lg["poses"]), H.pose_error(lg, a["poses"])
        assert max(a["trials"]) > 1 and e1 < e0 and a["chis"][-1] < a["chis"][0], (a["chis"], a["trials"], e0, e1)
        out.update({"lm_%s_chis" % kind: a["chis"], "lm_%s_gap" % kind: gap, "lm_%s_trials" % kind: np.array(a["trials"]),
                    "lm_%s_pose_error" % kind: np.array([e0, e1]), "lm_%s_poses" % kind: a["poses"], "lm_%s_poses_dense" % kind: b["poses"]})
        lines.append(dict(kind="oracle_lm", graph=kind, trials=a["trials"], chis=a["chis"].tolist(), gap=gap.tolist(), pose_error=[e0, e1],
                          poses_gap=float(np.abs(a["poses"] - b["poses"]).max())))
        print(lines[-1], flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "offset_edges.npz"), **out)
    path = os.path.join(ROOT, "profiles", "offset_edges.jsonl")
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
