#!/usr/bin/env python
"""Bearing-only landmark SLAM (EdgeSE2PointXYBearing, openslam_g2o_amd.synthetic.make_bearing_slam): Levenberg-Marquardt iterations
with the device front end (g2ohip_pg_set_bearing_edges: poses, landmarks, errors and Jacobians stay on the device), the same
library fed from the Python restatement (openslam_g2o_amd/bearing.py: J and err uploaded through setEdgeData with every
evaluation), and the producer kernel alone.  Record only: nothing is asserted.

  device     warm-up, then --iterations LM iterations one by one: mean, median, min, max of their wall-clock ms, chi2 and trials
  host_fed   the same iterations with the bearing set evaluated on the host (--host-poses / --host-landmarks cap its size: the
             restatement is Python; 0 = the full size), next to the device front end at that size
  kernel     pg_se2_bearing_linearize_kernel (csrc/pg_bearing.inc) in the library's kernel slot "pg_landmark_linearize": us per
             launch of an error-only and of a full linearization, median over --kernel-reps launches, for both values of
             pg_landmark_staged

At most 16 host threads.  One JSON line per result on stdout, appended to --out if given.
  python tools/bearing_slam_time.py [--poses 20000 --landmarks 100000] [--with-xy] [--iterations 10] [--out profiles/bearing_slam.jsonl]"""
import argparse, json, os, sys
for _v, _d in (("G2OHIP_HOST_THREADS", 8), ("OMP_NUM_THREADS", 16), ("OPENBLAS_NUM_THREADS", 16), ("MKL_NUM_THREADS", 16)):
    try:
        os.environ[_v] = str(max(1, min(16, int(os.environ.get(_v, _d)))))
    except ValueError:
        os.environ[_v] = str(_d)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openslam_g2o_amd import bearing as BE, capi, lm, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=20000)
ap.add_argument("--landmarks", type=int, default=100000)
ap.add_argument("--host-poses", type=int, default=400, help="poses of the host-fed comparison (0: the full size)")
ap.add_argument("--host-landmarks", type=int, default=2000)
ap.add_argument("--with-xy", action="store_true", help="the bearings beside the EdgeSE2PointXY observations")
ap.add_argument("--seed", type=int, default=42)
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
    return {"mean": float(np.mean(v)), "median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


class HostFed:
    """lm.py's graph protocol: the bearing set evaluated by bearing.py at the estimates read back, uploaded through setEdgeData."""

    def __init__(self, s, g, k):
        self.s, self.g, self.k, self.J = s, g, k, None

    def _feed(self, jac):
        g = self.g
        self.s.pgLinearize(jac)
        out = BE.bearing_edges(BE.FP64, self.s.pgGetEstimates(), self.s.pgGetLandmarkEstimates(), g["bp"], g["bl"], g["zb"], jac)
        if jac:
            self.J = out[:2]
        self.s.setEdgeData(self.k, self.J[0], self.J[1], g["omega_b"], out[2] if jac else out)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


def host_fed_setup(g):
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    sh = capi.HipBlockSolver(3, 2, 0)
    q0 = sh.addEdgeSet(3, h[g["vi"]], h[g["vj"]])
    qx = sh.addEdgeSet(2, h[g["vp"]], hl[g["vl"]]) if len(g["vp"]) else None
    qb = sh.addEdgeSet(1, h[g["bp"]], hl[g["bl"]])
    sh.buildStructure(g["nP"], g["nL"], True)
    sh.pgSetEdges(q0, 1, g["vi"], g["vj"], g["Z"], g["omega"])
    sh.pgSetEstimates(g["poses"], h)
    if qx is not None:
        sh.pgSetLandmarkEdges(qx, 3, g["vp"], g["vl"], g["zl"], g["omega_l"], None)
    sh.pgSetLandmarkEstimates(g["points"], hl)
    return sh, HostFed(sh, g, qb)


def sizes(g):
    return {"kind": "timing", "edge": "EdgeSE2PointXYBearing", "poses": int(g["n"]), "landmarks": int(g["L"]), "bearings": int(g["B"]),
            "xy_observations": int(g["M"]), "odometry_edges": len(g["vi"])}


g = S.make_bearing_slam(args.poses, args.landmarks, with_xy=args.with_xy, seed=args.seed)
size = sizes(g)
s, graph = lm.setup_device_landmark_slam(g)
lm.optimize(graph, s, 2, "lm")                          # warm-up: lazy analysis, code loading
s.pgSetEstimates(g["poses"], g["hidx"])
s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
times = []
done, chis, lams, trials = lm.optimize(graph, s, args.iterations, "lm", times=times)
emit(dict(size, what="lm_iteration", path="device_front_end", ms_per_lm_iteration=spread([1e3 * t for t in times]),
          lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))
for staged in (1, 0):
    s.setOption("pg_landmark_staged", staged)
    s.setProfiling(1)
    for jac in (False, True):
        s.pgSetEstimates(g["poses"], g["hidx"])
        s.pgLinearize(jac)
        s.sync()
        s.kernelTimes(reset=True)
        per = []
        for r in range(args.kernel_reps):
            s.pgSetEstimates(g["poses"], g["hidx"])
            s.pgLinearize(jac)
            s.sync()
            t, n = s.kernelTimes(reset=True).get("pg_landmark_linearize", (0.0, 0))
            per.append(1e6 * t / max(n, 1))
        emit(dict(size, what="kernel", kernel="pg_se2_bearing_linearize_kernel" + (" + pg_se2_pointxy_linearize_kernel" if args.with_xy else ""),
                  slot="pg_landmark_linearize", staged=staged, jacobians=jac, us_per_launch=spread(per),
                  edges_per_second=(g["B"] + g["M"]) / (1e-6 * float(np.median(per)))))
    s.setProfiling(0)
del s, graph
# the host-fed comparison at a size the Python restatement can evaluate, next to the device front end at the same size
gh = g if args.host_poses <= 0 else S.make_bearing_slam(args.host_poses, args.host_landmarks, with_xy=args.with_xy, seed=args.seed)
for path in ("device_front_end", "host_fed"):
    sh, gr = lm.setup_device_landmark_slam(gh) if path == "device_front_end" else host_fed_setup(gh)
    lm.optimize(gr, sh, 1, "lm")
    sh.pgSetEstimates(gh["poses"], gh["hidx"])
    sh.pgSetLandmarkEstimates(gh["points"], gh["pt_hidx"])
    times = []
    done, chis, lams, trials = lm.optimize(gr, sh, args.iterations, "lm", times=times)
    emit(dict(sizes(gh), what="lm_iteration", path=path, ms_per_lm_iteration=spread([1e3 * t for t in times]),
              lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))
    del sh, gr
