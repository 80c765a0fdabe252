"""Generator of tests/golden/gicp_edges.npz and of the oracle-drift lines of profiles/gicp_edges.jsonl (CPU only; run from the
repository root: python tests/golden/make_gicp_edges.py).  Needs the built CPU oracle (make -C oracle).

Per test graph of the device GICP front end (Edge_V_V_GICP, point-to-plane "pp" and plane-to-plane "pl"): the inputs,
gicp.gicp_edges evaluated with mpmath at 60 digits (rounded to fp64) and the drift of the SAME formulas evaluated in fp64 against
them -- max abs over err, over J0 | J1, over the plane-to-plane information.  The GPU tests bound the device against the fp64
restatement by 8 x the drift recorded here for the same graph -- the restatement's own figure, never the device's.

  pp1 ... pp300, pl1 ... pl300   gicp_helpers.base_graph: 3 scans, scan 0 fixed, pairs (0,1), (1,2), (0,2) and (2,1), two EdgeSE3
           odometry edges; one lane per edge, 64 lanes per wave, 256 threads per block: 63 / 64 / 65 and 255 / 256 / 257 sit on
           either side of a wave and of a block, 300 leaves a partial last block in the staged form
  moved    the same drift figures for every one of these graphs after a step over the free poses (the oracle's se3_oplus of the
           step moved_x: the error-only evaluation of the GPU tests), and the moved poses
  lm       synthetic.make_gicp(**gicp_helpers.LM_ARGS) in both modes: ten LM iterations (user_lambda_init = LM_LAMBDA) of
           lm.optimize over the CPU oracle fed by gicp.py, once with the oracle's own solver and once solving the full system
           densely: the trials of both (asserted equal, with at least one rejected step), chi2 per iteration, their relative gap, the relative-pose error of the
           initial guess and of the result (asserted: still descending at the last iteration, closer to the truth than the guess)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import gicp_helpers as H  # noqa: E402


def main():
    out, lines = {}, []
    for mode, plpl in H.MODES:
        for n in H.EDGE_COUNTS:
            name = H.graph_name(n, plpl)
            g = H.base_graph(n, plpl)
            (M0, M1, me, mo), fig = H.drift(g)
            for k in H.GRAPH_KEYS:
                if g[k] is not None:
                    out["%s_%s" % (name, k)] = g[k]
            out.update({name + "_ref_J0": M0, name + "_ref_J1": M1, name + "_ref_err": me, name + "_ref_omega": mo,
                        name + "_drift": np.array([fig["err"], fig["J"], fig["omega"]])})
            lines.append(dict(kind="oracle_drift", graph=name, edges=int(n), err_max_abs=float(np.abs(me).max()),
                              J_max_abs=float(max(np.abs(M0).max(), np.abs(M1).max())), omega_max_abs=float(np.abs(mo).max()), **fig))
            print(lines[-1], flush=True)
            x = H.update_step(g, 21)
            moved = O.se3_oplus(g["poses"], g["hidx"], x)
            (M0, M1, me, mo), fig = H.drift(dict(g, poses=moved))
            out.update({"moved_x": x, name + "_moved_poses": moved, name + "_moved_drift": np.array([fig["err"], fig["J"], fig["omega"]])})
            lines.append(dict(kind="oracle_drift", graph="moved " + name, edges=int(n), **fig))
            print(lines[-1], flush=True)
    for mode, plpl in H.MODES:
        g = H.lm_graph(mode)
        a = H.oracle_lm_run(g, lambda_init=H.LM_LAMBDA[mode])
        b = H.oracle_lm_run(g, dense=True, lambda_init=H.LM_LAMBDA[mode])
        assert a["trials"] == b["trials"] and a["done"] == b["done"] == H.LM_ITERATIONS, (a["trials"], b["trials"])
        gap = np.abs(a["chis"] - b["chis"]) / np.abs(b["chis"])
        e0, e1 = H.relative_pose_error(g["poses"], g["poses_true"]), H.relative_pose_error(a["poses"], g["poses_true"])
        assert a["chis"][-1] < (1.0 - 1e-3) * a["chis"][-2] and e1 < e0 and max(a["trials"]) > 1, (a["chis"], a["trials"], e0, e1)
        out.update({"lm_%s_chis" % mode: a["chis"], "lm_%s_gap" % mode: gap, "lm_%s_trials" % mode: np.array(a["trials"]),
                    "lm_%s_pose_error" % mode: np.array([e0, e1])})
        lines.append(dict(kind="oracle_drift", graph="lm " + mode, args={k: (list(map(list, v)) if k == "pairs" else v) for k, v in H.LM_ARGS.items()},
                          seed=H.LM_SEED[mode], lambda_init=H.LM_LAMBDA[mode], edges=int(len(g["gi"])), chi2=[float(v) for v in a["chis"]],
                          chi2_dense=[float(v) for v in b["chis"]], relative_chi2_gap=[float(v) for v in gap], trials=a["trials"],
                          trials_dense=b["trials"], pose_error_initial=e0, pose_error_final=e1))
        print(lines[-1], flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "gicp_edges.npz"), **out)
    path = os.path.join(ROOT, "profiles", "gicp_edges.jsonl")
    keep = []
    if os.path.exists(path):
        keep = [l for l in open(path).read().splitlines() if l.strip() and json.loads(l).get("kind") != "oracle_drift"]
    with open(path, "w") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")
        for l in keep:
            f.write(l + "\n")


if __name__ == "__main__":
    main()
