#!/usr/bin/env python
"""Odometry self-calibration (EdgeSE2OdomDifferentialCalib, openslam_g2o_amd.synthetic.make_calib_rig(odom_calib=True)):
Levenberg-Marquardt iterations with the device front end (g2ohip_pg_set_odom_calib_edges: table, errors and Jacobians stay on the
device), the same library with the new group fed from the Python restatement (openslam_g2o_amd/odom_calib.py: three Jacobian arrays
and err uploaded with every evaluation, the additive update applied on the host), the producer kernel alone, and the per-stage
split of one iteration.  The graph is the one of g2o/examples/calibration_odom_laser: no EdgeSE2; --with-calib 1 keeps the
EdgeSE2SensorCalib scan matches beside the new group (the example's graph), 0 leaves the new group alone (the laser offset fixed).
Record only: nothing is asserted.

  device     warm-up, then --iterations LM iterations one by one: mean, min, max of their wall-clock ms, chi2 and trials
  kernel     pg_se2_odom_calib_linearize_kernel (csrc/pg_odom_calib.inc) in the library's kernel slot "pg_landmark_linearize" (on the
             graph WITHOUT the type-21 group, which shares the slot): us per launch of an error-only and of a full linearization
             over --kernel-reps launches, for both values of pg_landmark_staged
  stages     every kernel slot of the library over --kernel-reps rounds of linearize + buildSystem + setLambda + solve.  The
             parameter vertex, like the laser offset, is a neighbour of EVERY edge: one diagonal block receives a term from every
             edge and every front of the factorisation carries its rows
  host_fed   --host-poses poses: the new group host-fed next to the device front end at that size

At most 16 host threads.  One JSON line per result on stdout, appended to --out if given.
  python tools/odom_calib_time.py [--poses 20000 --loops 2000] [--with-calib 1] [--out profiles/odom_calib.jsonl]"""
import argparse, json, os, sys
for _v, _d in (("G2OHIP_HOST_THREADS", 8), ("OMP_NUM_THREADS", 16), ("OPENBLAS_NUM_THREADS", 16), ("MKL_NUM_THREADS", 16)):
    try:
        os.environ[_v] = str(max(1, min(16, int(os.environ.get(_v, _d)))))
    except ValueError:
        os.environ[_v] = str(_d)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openslam_g2o_amd import capi, lm, odom_calib as OC, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=20000)
ap.add_argument("--loops", type=int, default=2000)
ap.add_argument("--with-calib", type=int, default=1)
ap.add_argument("--host-poses", type=int, default=500, help="poses of the host-fed comparison")
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--iterations", type=int, default=10)
ap.add_argument("--kernel-reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
PARTS = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
EMPTY = dict(vi=np.zeros(0, np.int32), vj=np.zeros(0, np.int32), Z=np.zeros((0, 3)), omega=np.zeros((0, 9)))


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def spread(v):
    return {"mean": float(np.mean(v)), "median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def rig(n_poses, loops, with_calib):
    g = dict(S.make_calib_rig(n_poses, loops=loops, seed=args.seed, odom_calib=True), **EMPTY)
    if not with_calib:                      # the new group alone: no scan matches, the (then unobserved) laser offset fixed
        g = {k: v for k, v in g.items() if k not in ("ci", "cj", "cl", "cmeas", "cinfo")}
        h = g["hidx"].copy()
        h[g["offset_row"]] = -1
        h[g["param_rows"]] -= 1
        g.update(hidx=h, nP=g["nP"] - 1)
    return g


def setup(g, options=None):
    cal = dict(vi=g["ci"], vj=g["cj"], vl=g["cl"], meas=g["cmeas"], info=g["cinfo"]) if "ci" in g else None
    return lm.setup_device_odom_calib_graph(g["poses"], g["hidx"], g["nP"], dict(vi=g["oi"], vj=g["oj"], vp=g["op"], meas=g["omeas"], info=g["oinfo"]),
                                            calib_edges=cal, options=options)


class HostFed:
    """lm.py's graph protocol: the new group's three sets evaluated by odom_calib.py at the table read back, uploaded through
    setEdgeData; the group is not bound, so the additive step of the parameter rows is applied on the host."""

    def __init__(self, s, g, ids):
        self.s, self.g, self.ids, self.J, self.stack = s, g, ids, None, []

    def _feed(self, jac):
        g = self.g
        self.s.pgLinearize(jac)
        out = OC.odom_calib_edges(OC.FP64, self.s.pgGetEstimates(), g["oi"], g["oj"], g["op"], g["omeas"], jac, g["hidx"])
        if jac:
            self.J = out[:3]
        Ji, Jj, Jp = self.J
        for k, (A, B) in zip(self.ids, ((Ji, Jj), (Ji, Jp), (Jj, Jp))):
            self.s.setEdgeData(k, A, B, g["oinfo"], out[3] if jac else out)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()

    def update(self):
        self.s.pgSetEstimates(OC.oplus(self.s.pgGetEstimates(), self.g["hidx"], self.s.x(), self.g["param_rows"]), self.g["hidx"])

    def push(self):
        self.stack.append(self.s.pgGetEstimates())

    def pop(self):
        self.s.pgSetEstimates(self.stack.pop(), self.g["hidx"])

    def discard_top(self):
        self.stack.pop()


g = rig(args.poses, args.loops, args.with_calib)
m = len(g["oi"])
size = {"kind": "timing", "edge": "EdgeSE2OdomDifferentialCalib", "poses": args.poses, "odom_calib_edges": m,
        "calib_edges": len(g["ci"]) if "ci" in g else 0, "odometry_edges": 0}
s, graph = setup(g, options={"use_graph": 1})
lm.optimize(graph, s, 2, "lm")                          # warm-up: lazy analysis, code loading, graph capture
s.pgSetEstimates(g["poses"], g["hidx"])
times = []
done, chis, lams, trials = lm.optimize(graph, s, args.iterations, "lm", times=times)
emit(dict(size, what="lm_iteration", path="device_front_end", ms_per_lm_iteration=spread([1e3 * t for t in times]),
          lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))
del s, graph
if not args.with_calib:                                 # (the producer alone in its slot)
    s, graph = setup(g)
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
            emit(dict(size, what="kernel", kernel="pg_se2_odom_calib_linearize_kernel", slot="pg_landmark_linearize", staged=staged, jacobians=jac,
                      us_per_launch=spread(per), edges_per_second=m / (1e-6 * float(np.median(per)))))
        s.setProfiling(0)
    del s, graph
# the per-stage split without captured launch sequences (every kernel in its slot)
s, graph = setup(g)
graph.linearize()
s.buildSystem()
lam = 1e-4 * s.maxDiagonal()
s.setLambda(lam, True)
s.solve()
s.restoreDiagonal()
s.sync()
s.setProfiling(1)
s.kernelTimes(reset=True)
for r in range(args.kernel_reps):
    s.pgSetEstimates(g["poses"], g["hidx"])
    graph.linearize()
    s.buildSystem()
    s.setLambda(lam, True)
    s.solve()
    s.restoreDiagonal()
s.sync()
kt = s.kernelTimes(reset=True)
s.setProfiling(0)
emit(dict(size, what="stages", rounds=args.kernel_reps, note="linearize + buildSystem + setLambda + solve; ms per round, launches per round",
          slots={k: [1e3 * t / args.kernel_reps, n / args.kernel_reps] for k, (t, n) in sorted(kt.items()) if n}, stats=s.stats()))
del s, graph
# the host-fed comparison at a size the Python restatement can evaluate, next to the device front end at the same size
gh = rig(args.host_poses, args.host_poses // 10, args.with_calib)
hh = np.asarray(gh["hidx"], np.int32)
for path in ("device_front_end", "host_fed"):
    if path == "device_front_end":
        sh, gr = setup(gh)
    else:
        sh = capi.HipBlockSolver(3, 2, 0)
        q0 = sh.addEdgeSet(3, hh[gh["vi"]], hh[gh["vj"]])
        kc, ko = [], []
        for ids, cols in ((kc, ("ci", "cj", "cl")), (ko, ("oi", "oj", "op"))):
            if cols[0] not in gh:
                continue
            a, b, c = (gh[k] for k in cols)
            for (u, v), pt in zip(((a, b), (a, c), (b, c)), PARTS):
                ids.append(sh.addEdgeSet(3, hh[u], hh[v]))
                sh.setEdgeSetParts(ids[-1], pt)
        sh.buildStructure(gh["nP"], 0, False)
        sh.pgSetEdges(q0, 1, gh["vi"], gh["vj"], gh["Z"], gh["omega"])
        sh.pgSetEstimates(gh["poses"], hh)
        if kc:
            sh.pgSetSensorCalibEdges(*kc, gh["ci"], gh["cj"], gh["cl"], gh["cmeas"], gh["cinfo"])
        gr = HostFed(sh, gh, ko)
    times = []
    done, chis, lams, trials = lm.optimize(gr, sh, args.iterations, "lm", times=times)
    emit(dict(size, poses=args.host_poses, odom_calib_edges=len(gh["oi"]), calib_edges=len(gh["ci"]) if "ci" in gh else 0, what="lm_iteration",
              path=path, ms_per_lm_iteration=spread([1e3 * t for t in times]), lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))
    del sh, gr
