#!/usr/bin/env python
"""Sim3 pose graphs (EdgeSim3 over VertexSim3Expmap, openslam_g2o_amd.synthetic.make_sim3_graph): one Levenberg-Marquardt
iteration with the device front end (g2ohip_pg_set_edges type 10: estimates, errors and the numeric Jacobian stay on the
device) against the same library fed from the host, and the two producer kernels alone.

  device     warm-up, then --iterations LM iterations one by one: mean, min, max of their wall-clock ms, chi2 and trials
  kernels    HIP events of the library's kernel slots "pg_sim3_error" and "pg_sim3_jacobian": us per launch, evaluations of
             exp . mul . mul . log per second (1 per edge for the error, 28 per edge for the Jacobian)
  host-fed   the host producers are the scalar fp64 restatement of openslam_g2o_amd/sim3.py (the one the tests hold the device
             to), far too slow for the full graph: one linearization (errors + Jacobians) and one error evaluation are timed
             on the first --host-edges edges and scaled to the edge count, and one set_edge_data upload + build + solve of the
             full system is timed with the device's own Jacobians read back -- reported as an ESTIMATE of a host-fed iteration
             with one trial, labelled as such.

One JSON line per result on stdout, appended to --out if given.
  python tools/sim3_time.py [--poses 20000 --loop-every 50 --scale-drift 1e-5] [--iterations 10] [--host-edges 2000] [--out f]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openslam_g2o_amd import capi, lm, sim3 as S3, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=20000)
ap.add_argument("--loop-every", type=int, default=50)
ap.add_argument("--scale-drift", type=float, default=1e-5)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--iterations", type=int, default=10)
ap.add_argument("--kernel-reps", type=int, default=20)
ap.add_argument("--host-edges", type=int, default=2000)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def spread(v):
    return {"mean": float(np.mean(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


g = S.make_sim3_graph(args.poses, args.loop_every, args.scale_drift, args.seed)
m = len(g["vi"])
size = {"kind": "timing", "poses": args.poses, "edges": m, "loop_every": args.loop_every, "scale_drift": args.scale_drift}
s, graph = lm.setup_device_pose_graph(10, g["est"], g["hidx"], g["num_free"], g["vi"], g["vj"], g["meas"], g["info"],
                                      options={"use_graph": 1})
lm.optimize(graph, s, 2, "lm")                          # warm-up: lazy analysis, code loading, graph capture
s.pgSetEstimates(g["est"], g["hidx"])
times = []
done, chis, lams, trials = lm.optimize(graph, s, args.iterations, "lm", times=times)
emit(dict(size, what="lm_iteration", path="device_front_end", ms_per_lm_iteration=spread([1e3 * t for t in times]),
          lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))

s.setProfiling(1)
for jac in (True, False):
    s.pgLinearize(jac)
    s.sync()
    s.kernelTimes(reset=True)
    for r in range(args.kernel_reps):
        s.pgSetEstimates(g["est"], g["hidx"])           # (same table: only invalidates the evaluation)
        s.pgLinearize(jac)
    s.sync()
    kt = s.kernelTimes(reset=True)
    for slot, evals in (("pg_sim3_error", 1), ("pg_sim3_jacobian", 28)):
        t, n = kt.get(slot, (0.0, 0))
        if n:
            us = 1e6 * t / n
            emit(dict(size, what="kernel", kernel=slot, jacobians=bool(jac), launches=int(n), us_per_launch=us,
                      evaluations_per_second=evals * m / (1e-6 * us)))
s.setProfiling(0)

# host-fed estimate
k = min(args.host_edges, m)
t0 = time.perf_counter()
S3.edges(S3.FP64, g["est"], g["vi"][:k], g["vj"][:k], g["meas"][:k], g["hidx"])
t_lin = (time.perf_counter() - t0) * m / k
t0 = time.perf_counter()
S3.edges(S3.FP64, g["est"], g["vi"][:k], g["vj"][:k], g["meas"][:k], jac=False)
t_err = (time.perf_counter() - t0) * m / k
s.pgSetEstimates(g["est"], g["hidx"])
s.pgLinearize(True)
J0, J1, err = s.edgeData(s.pose_set, m, 7, 7, 7)
h = capi.HipBlockSolver(7, 3, 0)
kk = h.addEdgeSet(7, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
h.buildStructure(g["num_free"], 0, False)
solve = []
for r in range(4):
    h.sync()
    t0 = time.perf_counter()
    h.setEdgeData(kk, J0, J1, g["info"], err)
    h.buildSystem()
    h.setLambda(1.0, True)
    h.solve()
    h.restoreDiagonal()
    x = h.x()
    solve.append(time.perf_counter() - t0)
emit(dict(size, what="lm_iteration_estimate", path="host_fed_scalar_fp64_producers", sampled_edges=k,
          ms_linearize_scaled=1e3 * t_lin, ms_errors_scaled=1e3 * t_err, ms_upload_build_solve=1e3 * min(solve[1:]),
          ms_per_lm_iteration_one_trial=1e3 * (t_lin + t_err + min(solve[1:]))))
