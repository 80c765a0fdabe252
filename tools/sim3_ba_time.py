#!/usr/bin/env python
"""Sim3 bundle adjustment (EdgeSim3ProjectXYZ over VertexSim3Expmap / VertexSBAPointXYZ beside EdgeSim3,
openslam_g2o_amd.synthetic.make_sim3_ba): one Levenberg-Marquardt iteration with the device front end
(g2ohip_pg_set_sim3_project_edges: estimates, errors and the numeric Jacobians stay on the device) against the same library fed
from the host, and the two producer kernels alone.

  device     warm-up, then --iterations LM iterations one by one: mean, min, max of their wall-clock ms, chi2 and trials
  kernels    the two kernels of csrc/pg_sim3_project.inc share the library's kernel slot "pg_landmark_linearize"
             (g2ohip_kernel_time): an error-only linearization times pg_sim3_project_error_kernel alone, a full one both, and the
             Jacobian kernel is their difference -- us per launch, evaluations of the error per second (1 per edge for the error
             kernel, 20 per edge for the Jacobian kernel)
  host-fed   the host producers are the scalar fp64 restatement of openslam_g2o_amd/sim3.py (the one the tests hold the device
             to), far too slow for the full graph: one linearization (errors + Jacobians) and one error evaluation of the
             observations are timed on the first --host-edges edges and scaled to the edge count, the EdgeSim3 set is evaluated
             in full, and one set_edge_data upload + build + solve of the full system is timed with the device's own Jacobians
             read back -- reported as an ESTIMATE of a host-fed iteration with one trial, labelled as such.

At most 16 host threads (G2OHIP_HOST_THREADS and the BLAS / OpenMP pools are capped before anything is imported).
One JSON line per result on stdout, appended to --out if given.
  python tools/sim3_ba_time.py [--cams 1000 --points 20000 --obs 5] [--iterations 10] [--host-edges 2000] [--out f]"""
import argparse, json, os, sys, time
for _v, _d in (("G2OHIP_HOST_THREADS", 8), ("OMP_NUM_THREADS", 16), ("OPENBLAS_NUM_THREADS", 16), ("MKL_NUM_THREADS", 16)):
    try:
        os.environ[_v] = str(max(1, min(16, int(os.environ.get(_v, _d)))))
    except ValueError:
        os.environ[_v] = str(_d)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openslam_g2o_amd import capi, lm, sim3 as S3, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--cams", type=int, default=1000)
ap.add_argument("--points", type=int, default=20000)
ap.add_argument("--obs", type=int, default=5)
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


g = S.make_sim3_ba(args.cams, args.points, args.obs, args.seed, scale_drift=1e-4)
m0, m = len(g["vi"]), len(g["vp"])
size = {"kind": "timing", "cameras": args.cams, "points": args.points, "sim3_edges": m0, "observations": m}
s, graph = lm.setup_device_sim3_ba(g, options={"use_graph": 1})
k0, k1 = s.landmark_sets


def reset_estimates():
    s.pgSetEstimates(g["est"], g["hidx"])
    s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])


lm.optimize(graph, s, 2, "lm")                          # warm-up: lazy analysis, code loading, graph capture
reset_estimates()
times = []
done, chis, lams, trials = lm.optimize(graph, s, args.iterations, "lm", times=times)
emit(dict(size, what="lm_iteration", path="device_front_end", ms_per_lm_iteration=spread([1e3 * t for t in times]),
          lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))

s.setProfiling(1)
us = {}
for jac in (False, True):
    s.pgLinearize(jac)
    s.sync()
    s.kernelTimes(reset=True)
    for r in range(args.kernel_reps):
        s.pgSetEstimates(g["est"], g["hidx"])           # (same table: only invalidates the evaluation)
        s.pgLinearize(jac)
    s.sync()
    t, n = s.kernelTimes(reset=True).get("pg_landmark_linearize", (0.0, 0))
    us[jac] = 1e6 * t / max(n, 1)
s.setProfiling(0)
emit(dict(size, what="kernel", kernel="pg_sim3_project_error_kernel", slot="pg_landmark_linearize (error-only linearization)",
          launches=args.kernel_reps, us_per_launch=us[False], evaluations_per_second=m / (1e-6 * us[False])))
emit(dict(size, what="kernel", kernel="pg_sim3_project_jacobian_kernel", launches=args.kernel_reps,
          slot="pg_landmark_linearize (full linearization minus the error-only one)", us_per_launch=us[True] - us[False],
          us_both_kernels=us[True], evaluations_per_second=20 * m / (1e-6 * (us[True] - us[False]))))

# host-fed estimate
k = min(args.host_edges, m)
sub = (g["est"], g["points"], g["vp"][:k], g["vl"][:k], g["zl"][:k], g["intrinsics"])
t0 = time.perf_counter()
S3.project_edges(S3.FP64, *sub, g["hidx"], g["pt_hidx"])
t_lin = (time.perf_counter() - t0) * m / k
t0 = time.perf_counter()
S3.project_edges(S3.FP64, *sub, jac=False)
t_err = (time.perf_counter() - t0) * m / k
t0 = time.perf_counter()
S3.edges(S3.FP64, g["est"], g["vi"], g["vj"], g["meas"], g["hidx"])
t_lin += time.perf_counter() - t0
t0 = time.perf_counter()
S3.edges(S3.FP64, g["est"], g["vi"], g["vj"], g["meas"], jac=False)
t_err += time.perf_counter() - t0
reset_estimates()
s.pgLinearize(True)
A0, A1, aerr = s.edgeData(k0, m0, 7, 7, 7)
J0, J1, err = s.edgeData(k1, m, 2, 7, 3)
h = capi.HipBlockSolver(7, 3, 0)
ka = h.addEdgeSet(7, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
kb = h.addEdgeSet(2, g["hidx"][g["vp"]], g["pt_hidx"][g["vl"]])
h.buildStructure(g["nP"], g["nL"], True)
solve = []
for r in range(4):
    h.sync()
    t0 = time.perf_counter()
    h.setEdgeData(ka, A0, A1, g["info"], aerr)
    h.setEdgeData(kb, J0, J1, g["omega_l"], err)
    h.buildSystem()
    h.setLambda(1.0, True)
    h.solve()
    h.restoreDiagonal()
    x = h.x()
    solve.append(time.perf_counter() - t0)
emit(dict(size, what="lm_iteration_estimate", path="host_fed_scalar_fp64_producers", sampled_observations=k,
          ms_linearize_scaled=1e3 * t_lin, ms_errors_scaled=1e3 * t_err, ms_upload_build_solve=1e3 * min(solve[1:]),
          ms_per_lm_iteration_one_trial=1e3 * (t_lin + t_err + min(solve[1:]))))
