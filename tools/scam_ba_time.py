#!/usr/bin/env python
"""Stereo bundle adjustment over VertexSCam cameras (Edge_XYZ_VSC, openslam_g2o_amd.synthetic.make_scam_ba): Levenberg-Marquardt
iterations with the device front end (g2ohip_pg_set_scam_edges: cameras, points, errors and Jacobians stay on the device), the
producer kernel alone, the type-6 disparity set on the same shape for context, and the same library fed from the Python
restatement (openslam_g2o_amd/scam.py: J and err uploaded through setEdgeData with every evaluation).  Record only: nothing is
asserted.

  --drift    CPU only: the relative chi2 gap per LM iteration between two equally valid oracle runs (the oracle's Schur path and
             the full system solved densely) on the graphs of tests/test_gpu_scam.py, one "oracle_drift" line per graph
  lm         warm-up, then --iterations LM iterations one by one: min ... max of their wall-clock ms, chi2 and trials
  kernel     pg_scam_linearize_kernel (csrc/pg_scam.inc) in the library's kernel slot "pg_landmark_linearize": us per launch of
             an error-only and of a full linearization over --kernel-reps launches, for both values of pg_landmark_staged
  disparity  the same for pg_se3_point_linearize_kernel<6> (EdgeSE3PointXYZDisparity) on the same cameras, points and pairs
  host_fed   LM iterations with the stereo set evaluated on the host at --host-cams / --host-points, next to the device front end
             at that size

Without --step every GPU step runs as a child process of its own under `timeout`, one after the other, and the first that fails
ends the run.  At most 16 host threads.  One JSON line per result on stdout, appended to --out if given.
  python tools/scam_ba_time.py [--cams 20000 --points 200000 --spacing 2.56] [--out profiles/scam_edges.jsonl]
  python tools/scam_ba_time.py --drift [--out profiles/scam_edges.jsonl]"""
import argparse, json, os, subprocess, sys
for _v, _d in (("G2OHIP_HOST_THREADS", 8), ("OMP_NUM_THREADS", 16), ("OPENBLAS_NUM_THREADS", 16), ("MKL_NUM_THREADS", 16)):
    try:
        os.environ[_v] = str(max(1, min(16, int(os.environ.get(_v, _d)))))
    except ValueError:
        os.environ[_v] = str(_d)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

STEPS = (("lm", 300), ("kernel", 180), ("disparity", 180), ("host_fed", 300))   # (step, its time limit in seconds)

ap = argparse.ArgumentParser()
ap.add_argument("--cams", type=int, default=20000)
ap.add_argument("--points", type=int, default=200000)
ap.add_argument("--spacing", type=float, default=2.56, help="camera spacing: 2.56 gives five observations per point")
ap.add_argument("--host-cams", type=int, default=200)
ap.add_argument("--host-points", type=int, default=2000)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--iterations", type=int, default=10)
ap.add_argument("--kernel-reps", type=int, default=20)
ap.add_argument("--drift", action="store_true")
ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
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


if args.drift:
    from tests import scam_helpers as H
    for name, g, its in (("scam_ba_6_120", H.lm_graph(False), H.LM_ITERATIONS), ("scam_ba_6_120_gicp", H.lm_graph(True), H.JOINT_ITERATIONS)):
        ra, rb = H.oracle_lm_run(g, its), H.oracle_lm_run(g, its, dense=True)
        gap = (np.abs(ra["chis"] - rb["chis"]) / np.abs(rb["chis"])).tolist()
        emit(dict(what="oracle_drift", graph=name, cams=int(g["n"]), points=int(g["L"]), observations=int(g["M"]),
                  gicp=int(len(g["gi"])) if H.has_gicp(g) else 0, iterations=its, trials=ra["trials"], trials_dense=rb["trials"],
                  chi2=ra["chis"].tolist(), relative_chi2_gap=gap))
    sys.exit(0)

if args.step is None:
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + sys.argv[1:]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("step %s ended with status %d: stopping" % (step, rc), flush=True)
            sys.exit(rc)
    sys.exit(0)

from openslam_g2o_amd import capi, lm, scam as SC, synthetic as S


def sizes(g, edge="Edge_XYZ_VSC"):
    return {"kind": "timing", "edge": edge, "cams": int(g["n"]), "points": int(g["L"]), "observations": int(g["M"])}


def disparity_problem(g):
    """The same cameras, points and pairs observed through EdgeSE3PointXYZDisparity (type 6, identity offset)."""
    X, L = g["poses_true"][g["vp"]], g["points_true"][g["vl"]]
    d = L - X[:, 9:]
    q = np.stack([(X[:, 3 * r:3 * r + 3] * d).sum(axis=1) for r in range(3)], axis=1)
    fx, fy, cx, cy = g["kcam"][:4]
    out = dict(g, observation="disparity", kcam=g["kcam"][:4].copy(), offset=None)
    out["zl"] = np.stack([fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy, 1.0 / q[:, 2]], axis=1)
    return out


def kernel_times(g, name):
    s, graph = lm.setup_device_landmark_slam(g)
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
            emit(dict(sizes(g, name[0]), what="kernel", kernel=name[1], slot="pg_landmark_linearize", staged=staged, jacobians=jac,
                      us_per_launch=spread(per), edges_per_second=g["M"] / (1e-6 * float(np.median(per)))))
        s.setProfiling(0)


class HostFed:
    """lm.py's graph protocol: the stereo set evaluated by scam.py at the estimates read back, uploaded through setEdgeData."""

    def __init__(self, s, g, k):
        self.s, self.g, self.k, self.J = s, g, k, None

    def _feed(self, jac):
        g = self.g
        self.s.pgLinearize(jac)
        out = SC.scam_edges_numpy(self.s.pgGetEstimates(), self.s.pgGetLandmarkEstimates(), g["vp"], g["vl"], g["zl"], g["kcam"], jac)
        if jac:
            self.J = out[:2]
        self.s.setEdgeData(self.k, self.J[0], self.J[1], g["omega_l"], out[2] if jac else out)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


def host_fed_setup(g):
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    sh = capi.HipBlockSolver(6, 3, 0)
    q0 = sh.addEdgeSet(6, h[g["vi"]], h[g["vj"]])
    q1 = sh.addEdgeSet(3, h[g["vp"]], hl[g["vl"]])
    sh.buildStructure(g["nP"], g["nL"], True)
    sh.pgSetEdges(q0, 2, g["vi"], g["vj"], g["Z"], g["omega"])
    sh.pgSetEstimates(g["poses"], h)
    sh.pgSetLandmarkEstimates(g["points"], hl)
    return sh, HostFed(sh, g, q1)


def lm_times(g, path, warm):
    s, graph = lm.setup_device_landmark_slam(g) if path == "device_front_end" else host_fed_setup(g)
    lm.optimize(graph, s, warm, "lm")                   # warm-up: lazy analysis, code loading
    s.pgSetEstimates(g["poses"], g["hidx"])
    s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
    times = []
    done, chis, lams, trials = lm.optimize(graph, s, args.iterations, "lm", times=times)
    emit(dict(sizes(g), what="lm_iteration", path=path, ms_per_lm_iteration=spread([1e3 * t for t in times]),
              lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))


if args.step == "host_fed":
    gh = S.make_scam_ba(args.host_cams, args.host_points, seed=args.seed, spacing=args.spacing)
    for path in ("device_front_end", "host_fed"):
        lm_times(gh, path, 1)
else:
    g = S.make_scam_ba(args.cams, args.points, seed=args.seed, spacing=args.spacing)
    if args.step == "lm":
        lm_times(g, "device_front_end", 2)
    elif args.step == "kernel":
        kernel_times(g, ("Edge_XYZ_VSC", "pg_scam_linearize_kernel"))
    else:
        kernel_times(disparity_problem(g), ("EdgeSE3PointXYZDisparity", "pg_se3_point_linearize_kernel<6>"))
