#!/usr/bin/env python
"""Sensor-offset pose-pose edges (EdgeSE2Offset / EdgeSE3Offset, openslam_g2o_amd.synthetic.make_offset_rig): Levenberg-Marquardt
iterations with the device front end (g2ohip_pg_set_offset_edges: poses, errors and Jacobians stay on the device), the same library
fed from the Python restatement (openslam_g2o_amd/offset_edges.py: J and err uploaded with every evaluation), and the producer
kernels alone.  Record only: nothing is asserted.

  device     warm-up, then --iterations LM iterations one by one: mean, min, max of their wall-clock ms, chi2 and trials
  host_fed   the same iterations with the offset set evaluated on the host (--host-poses caps its size: the restatement is
             Python), next to the device front end at that size
  kernel     pg_se2_offset_linearize_kernel / pg_se3_offset_linearize_kernel (csrc/pg_offset.inc) in the library's kernel slot
             "pg_landmark_linearize": us per launch of an error-only and of a full linearization, median over --kernel-reps launches,
             for both values of pg_landmark_staged
  scale      the existing pose-pose kernel (type 1 / 2) on the same edge count: it has no kernel slot, so the wall-clock us of a
             synchronised g2ohip_pg_linearize of a graph whose pose-pose set holds the offset edges' vertex pairs, beside the same
             call of the rig graph (odometry + offset producer), median over --kernel-reps calls

At most 16 host threads.  One JSON line per result on stdout, appended to --out if given.
  python tools/offset_edges_time.py [--poses 20000 --sensors 3 --edges-per-pose 2] [--iterations 10] [--out profiles/offset_edges.jsonl]"""
import argparse, json, os, sys, time
for _v, _d in (("G2OHIP_HOST_THREADS", 8), ("OMP_NUM_THREADS", 16), ("OPENBLAS_NUM_THREADS", 16), ("MKL_NUM_THREADS", 16)):
    try:
        os.environ[_v] = str(max(1, min(16, int(os.environ.get(_v, _d)))))
    except ValueError:
        os.environ[_v] = str(_d)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openslam_g2o_amd import capi, lm, offset_edges as OE, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=20000)
ap.add_argument("--sensors", type=int, default=3)
ap.add_argument("--edges-per-pose", type=int, default=2)
ap.add_argument("--host-poses", type=int, default=500, help="poses of the host-fed comparison")
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--iterations", type=int, default=10)
ap.add_argument("--kernel-reps", type=int, default=20)
ap.add_argument("--kinds", default="se2,se3")
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


def setup(g, options=None):
    return lm.setup_device_pose_graph(1 if g["kind"] == "se2" else 2, g["poses"], g["hidx"], g["nP"], g["vi"], g["vj"], g["Z"], g["omega"],
                                      options=options,
                                      offset_edges=(g["offset_type"], g["oi"], g["oj"], g["opf"], g["opt"], g["omeas"], g["oinfo"], g["offsets"]))


class HostFed:
    """lm.py's graph protocol: the offset set evaluated by offset_edges.py at the poses read back, uploaded through setEdgeData."""

    def __init__(self, s, g, k):
        self.s, self.g, self.k, self.J = s, g, k, None

    def _feed(self, jac):
        g = self.g
        self.s.pgLinearize(jac)
        out = OE.offset_edges(OE.FP64, g["offset_type"], self.s.pgGetEstimates(), g["oi"], g["oj"], g["opf"], g["opt"], g["omeas"], g["offsets"], jac)
        if jac:
            self.J = out[:2]
        self.s.setEdgeData(self.k, self.J[0], self.J[1], g["oinfo"], out[2] if jac else out)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


def wall_us(s, g, jac):
    per = []
    for r in range(args.kernel_reps + 1):
        s.pgSetEstimates(g["poses"], g["hidx"])         # (same table: only invalidates the evaluation)
        s.sync()
        t0 = time.perf_counter()
        s.pgLinearize(jac)
        s.sync()
        per.append(1e6 * (time.perf_counter() - t0))
    return per[1:]


for kind in args.kinds.split(","):
    g = S.make_offset_rig(kind, args.poses, args.sensors, args.edges_per_pose, seed=args.seed)
    m, d = len(g["oi"]), 3 if kind == "se2" else 6
    edge = "EdgeSE2Offset" if kind == "se2" else "EdgeSE3Offset"
    size = {"kind": "timing", "edge": edge, "poses": args.poses, "sensors": args.sensors, "offset_edges": m, "odometry_edges": len(g["vi"])}
    s, graph = setup(g, options={"use_graph": 1})
    lm.optimize(graph, s, 2, "lm")                          # warm-up: lazy analysis, code loading, graph capture
    s.pgSetEstimates(g["poses"], g["hidx"])
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
            emit(dict(size, what="kernel", kernel="pg_%s_offset_linearize_kernel" % kind, slot="pg_landmark_linearize", staged=staged,
                      jacobians=jac, us_per_launch=spread(per), edges_per_second=m / (1e-6 * float(np.median(per)))))
        s.setProfiling(0)
    s.setOption("pg_landmark_staged", 1)
    for jac in (False, True):
        emit(dict(size, what="scale", call="pg_linearize of the rig graph (odometry + offset producer), synchronised", jacobians=jac,
                  wall_us_per_call=spread(wall_us(s, g, jac))))
    del s, graph
    # the existing pose-pose kernel on the offset edges' vertex pairs (the measurements are used as they are: only the time matters)
    h = np.asarray(g["hidx"], np.int32)
    gp = dict(g, vi=g["oi"], vj=g["oj"], Z=g["omeas"], omega=g["oinfo"])
    sp, _ = lm.setup_device_pose_graph(1 if kind == "se2" else 2, gp["poses"], h, gp["nP"], gp["vi"], gp["vj"], gp["Z"], gp["omega"])
    for jac in (False, True):
        emit(dict(size, what="scale", call="pg_linearize of a type-%d set of the same edge count, synchronised" % (1 if kind == "se2" else 2),
                  jacobians=jac, wall_us_per_call=spread(wall_us(sp, gp, jac))))
    del sp
    # the host-fed comparison at a size the Python restatement can evaluate, next to the device front end at the same size
    gh = S.make_offset_rig(kind, args.host_poses, args.sensors, args.edges_per_pose, seed=args.seed)
    hh = np.asarray(gh["hidx"], np.int32)
    for path in ("device_front_end", "host_fed"):
        if path == "device_front_end":
            sh, gr = setup(gh)
        else:
            sh = capi.HipBlockSolver(d, 2 if d == 3 else 3, 0)
            q0 = sh.addEdgeSet(d, hh[gh["vi"]], hh[gh["vj"]])
            q1 = sh.addEdgeSet(d, hh[gh["oi"]], hh[gh["oj"]])
            sh.buildStructure(gh["nP"], 0, False)
            sh.pgSetEdges(q0, 1 if d == 3 else 2, gh["vi"], gh["vj"], gh["Z"], gh["omega"])
            sh.pgSetEstimates(gh["poses"], hh)
            gr = HostFed(sh, gh, q1)
        times = []
        done, chis, lams, trials = lm.optimize(gr, sh, args.iterations, "lm", times=times)
        emit(dict(size, poses=args.host_poses, offset_edges=len(gh["oi"]), odometry_edges=len(gh["vi"]), what="lm_iteration", path=path,
                  ms_per_lm_iteration=spread([1e3 * t for t in times]), lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))
        del sh, gr
