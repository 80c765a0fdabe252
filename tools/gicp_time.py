#!/usr/bin/env python
"""GICP scan registration (Edge_V_V_GICP between VertexSE3, openslam_g2o_amd.synthetic.make_gicp): Levenberg-Marquardt iterations
with the device front end (g2ohip_pg_set_gicp_edges: poses, errors, Jacobians and the plane-to-plane information stay on the
device), the same library fed from the NumPy restatement (openslam_g2o_amd/gicp.py: J, err and the information uploaded with
every evaluation), and the producer kernel alone, point-to-plane and plane-to-plane.

  device     warm-up, then --iterations LM iterations one by one: mean, min, max of their wall-clock ms, chi2 and trials
  host_fed   the same iterations with the GICP set evaluated on the host (--host-edges caps its size: the restatement is Python)
  kernel     pg_gicp_linearize_kernel (csrc/pg_gicp.inc) in the library's kernel slot "pg_landmark_linearize": us per launch of
             an error-only and of a full linearization, mean over --kernel-reps launches, for both values of pg_landmark_staged

At most 16 host threads.  One JSON line per result on stdout, appended to --out if given.
  python tools/gicp_time.py [--scans 8 --points 100000] [--iterations 10] [--out profiles/gicp_edges.jsonl]"""
import argparse, json, os, sys, time
for _v, _d in (("G2OHIP_HOST_THREADS", 8), ("OMP_NUM_THREADS", 16), ("OPENBLAS_NUM_THREADS", 16), ("MKL_NUM_THREADS", 16)):
    try:
        os.environ[_v] = str(max(1, min(16, int(os.environ.get(_v, _d)))))
    except ValueError:
        os.environ[_v] = str(_d)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openslam_g2o_amd import gicp as G, lm, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=8)
ap.add_argument("--points", type=int, default=100000, help="correspondences per scan pair")
ap.add_argument("--host-edges", type=int, default=2000, help="correspondences per pair of the host-fed comparison")
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


class HostFed:
    """lm.py's graph protocol: the GICP set evaluated by gicp.py at the poses read back, uploaded through setEdgeData."""

    def __init__(self, s, g, k):
        self.s, self.g, self.k, self.J = s, g, k, None

    def _feed(self, jac):
        self.s.pgLinearize(jac)
        out = G.gicp_edges(G.FP64, self.s.pgGetEstimates(), self.g["gi"], self.g["gj"], self.g["gmeas"], self.g["gcov"], jac)
        if jac:
            self.J = out[:2]
        om = self.g["ginfo"] if out[-1] is None else out[-1]
        self.s.setEdgeData(self.k, self.J[0], self.J[1], om, out[-2])

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


for plpl in (False, True):
    mode = "plane_to_plane" if plpl else "point_to_plane"
    g = S.make_gicp(args.scans, args.points, plane_to_plane=plpl, seed=args.seed)
    m = len(g["gi"])
    size = {"kind": "timing", "edge": "Edge_V_V_GICP", "mode": mode, "scans": args.scans, "correspondences": m}
    s, graph = lm.setup_device_gicp(g, options={"use_graph": 1})
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
                s.pgSetEstimates(g["poses"], g["hidx"])     # (same table: only invalidates the evaluation)
                s.pgLinearize(jac)
                s.sync()
                t, n = s.kernelTimes(reset=True).get("pg_landmark_linearize", (0.0, 0))
                per.append(1e6 * t / max(n, 1))
            emit(dict(size, what="kernel", kernel="pg_gicp_linearize_kernel", slot="pg_landmark_linearize", staged=staged,
                      jacobians=jac, us_per_launch=spread(per), edges_per_second=m / (1e-6 * float(np.mean(per)))))
        s.setProfiling(0)
    del s, graph
    # the host-fed comparison at a size the Python restatement can evaluate, next to the device front end at the same size
    gh = S.make_gicp(args.scans, args.host_edges, plane_to_plane=plpl, seed=args.seed)
    from openslam_g2o_amd import capi
    h = np.asarray(gh["hidx"], np.int32)
    for path in ("device_front_end", "host_fed"):
        if path == "device_front_end":
            sh, gr = lm.setup_device_gicp(gh)
        else:
            sh = capi.HipBlockSolver(6, 3, 0)
            q0 = sh.addEdgeSet(6, h[gh["vi"]], h[gh["vj"]])
            q1 = sh.addEdgeSet(3, h[gh["gi"]], h[gh["gj"]])
            sh.buildStructure(gh["nP"], 0, False)
            sh.pgSetEdges(q0, 2, gh["vi"], gh["vj"], gh["Z"], gh["omega"])
            sh.pgSetEstimates(gh["poses"], h)
            gr = HostFed(sh, gh, q1)
        times = []
        done, chis, lams, trials = lm.optimize(gr, sh, args.iterations, "lm", times=times)
        emit(dict(size, correspondences=len(gh["gi"]), what="lm_iteration", path=path,
                  ms_per_lm_iteration=spread([1e3 * t for t in times]), lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))
        del sh, gr
