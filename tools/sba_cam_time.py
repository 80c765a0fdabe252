#!/usr/bin/env python
"""SBA-format bundle adjustment (EdgeProjectP2MC / EdgeProjectP2SC over VertexCam / VertexSBAPointXYZ,
openslam_g2o_amd.synthetic.make_sbacam_ba): Levenberg-Marquardt iterations with the device front end
(g2ohip_pg_set_cam_project_edges: estimates, errors and the analytic Jacobians stay on the device) and the producer kernel
alone, mono and stereo.

  device     warm-up, then --iterations LM iterations one by one: mean, min, max of their wall-clock ms, chi2 and trials
  kernel     pg_cam_project_linearize_kernel (csrc/pg_cam_project.inc) in the library's kernel slot "pg_landmark_linearize"
             (g2ohip_kernel_time): us per launch of an error-only and of a full linearization, mean over --kernel-reps
             launches, for both values of option pg_landmark_staged

At most 16 host threads (G2OHIP_HOST_THREADS and the BLAS / OpenMP pools are capped before anything is imported).
One JSON line per result on stdout, appended to --out if given.
  python tools/sba_cam_time.py [--cams 20000 --points 200000 --obs 5] [--iterations 10] [--out profiles/sba_cam.jsonl]"""
import argparse, json, os, sys
for _v, _d in (("G2OHIP_HOST_THREADS", 8), ("OMP_NUM_THREADS", 16), ("OPENBLAS_NUM_THREADS", 16), ("MKL_NUM_THREADS", 16)):
    try:
        os.environ[_v] = str(max(1, min(16, int(os.environ.get(_v, _d)))))
    except ValueError:
        os.environ[_v] = str(_d)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openslam_g2o_amd import lm, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--cams", type=int, default=20000)
ap.add_argument("--points", type=int, default=200000)
ap.add_argument("--obs", type=int, default=5)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--iterations", type=int, default=10)
ap.add_argument("--kernel-reps", type=int, default=20)
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


for stereo in (False, True):
    g = S.make_sbacam_ba(args.cams, args.points, args.obs, stereo=stereo, seed=args.seed)
    m = len(g["vp"])
    size = {"kind": "timing", "edge": "EdgeProjectP2SC" if stereo else "EdgeProjectP2MC", "cameras": args.cams, "points": args.points,
            "observations": m}
    s, graph = lm.setup_device_sbacam_ba(g, options={"use_graph": 1})
    lm.optimize(graph, s, 2, "lm")                          # warm-up: lazy analysis, code loading, graph capture
    s.pgSetEstimates(g["est"], g["hidx"])
    s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
    times = []
    done, chis, lams, trials = lm.optimize(graph, s, args.iterations, "lm", times=times)
    emit(dict(size, what="lm_iteration", path="device_front_end", ms_per_lm_iteration=spread([1e3 * t for t in times]),
              lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))
    for staged in (1, 0):
        s.setOption("pg_landmark_staged", staged)
        s.setProfiling(1)
        for jac in (False, True):
            s.pgSetEstimates(g["est"], g["hidx"])
            s.pgLinearize(jac)
            s.sync()
            s.kernelTimes(reset=True)
            per = []
            for r in range(args.kernel_reps):
                s.pgSetEstimates(g["est"], g["hidx"])       # (same table: only invalidates the evaluation)
                s.pgLinearize(jac)
                s.sync()
                t, n = s.kernelTimes(reset=True).get("pg_landmark_linearize", (0.0, 0))
                per.append(1e6 * t / max(n, 1))
            emit(dict(size, what="kernel", kernel="pg_cam_project_linearize_kernel", slot="pg_landmark_linearize", staged=staged,
                      jacobians=jac, us_per_launch=spread(per), edges_per_second=m / (1e-6 * float(np.mean(per)))))
        s.setProfiling(0)
    del s, graph
