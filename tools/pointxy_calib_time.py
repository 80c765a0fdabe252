#!/usr/bin/env python
"""Landmark self-calibration (EdgeSE2PointXYCalib, openslam_g2o_amd.synthetic.make_pointxy_calib_slam): the producer kernel alone in
its staged, direct and error-only forms, the type-3 producer (EdgeSE2PointXY) on the same poses, landmarks and pairs for context,
Levenberg-Marquardt iterations with the device front end (g2ohip_pg_set_pointxy_calib_edges: both tables, errors and Jacobians stay
on the device), and -- at a small size only -- the same library fed from the Python restatement (openslam_g2o_amd/pointxy_calib.py:
J and err uploaded through setEdgeData with every evaluation).  Record only: nothing is asserted.

  kernel     pg_se2_pointxy_calib_linearize_kernel (csrc/pg_pointxy_calib.inc) in the library's kernel slot
             "pg_landmark_linearize": us per launch of an error-only and of a full linearization, one warm-up launch and then
             --kernel-reps launches (median, min, max), for both values of pg_landmark_staged
  pointxy    the same for pg_se2_pointxy_linearize_kernel (type 3) on the same shape, and the ratio is left to the reader
  lm         warm-up, then --iterations LM iterations one by one: median, min, max of their wall-clock ms, chi2 and trials
  host_fed   LM iterations with the three sets evaluated on the host at --host-poses / --host-landmarks, next to the device front
             end at that size

Without --step every GPU step runs as a child process of its own under `timeout`, one after the other, and the first that fails
ends the run.  At most 16 host threads.  One JSON line per result on stdout, appended to --out if given.
  python tools/pointxy_calib_time.py [--poses 20000 --landmarks 70000] [--out profiles/pointxy_calib.jsonl]"""
import argparse, json, os, subprocess, sys
for _v, _d in (("G2OHIP_HOST_THREADS", 8), ("OMP_NUM_THREADS", 16), ("OPENBLAS_NUM_THREADS", 16), ("MKL_NUM_THREADS", 16)):
    try:
        os.environ[_v] = str(max(1, min(16, int(os.environ.get(_v, _d)))))
    except ValueError:
        os.environ[_v] = str(_d)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

STEPS = (("kernel", 180), ("pointxy", 180), ("lm", 400), ("host_fed", 300))   # (step, its time limit in seconds)

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=20000)
ap.add_argument("--landmarks", type=int, default=70000, help="70000 landmarks seen from 15 poses each: about 1 M observations")
ap.add_argument("--host-poses", type=int, default=200)
ap.add_argument("--host-landmarks", type=int, default=300)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--iterations", type=int, default=6)
ap.add_argument("--kernel-reps", type=int, default=20)
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


if args.step is None:
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + sys.argv[1:]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("step %s ended with status %d: stopping" % (step, rc), flush=True)
            sys.exit(rc)
    sys.exit(0)

from openslam_g2o_amd import capi, lm, pointxy_calib as PC, synthetic as S


def sizes(g, edge, n):
    return {"kind": "timing", "edge": edge, "poses": int(g["n"]), "landmarks": int(g["L"]), "observations": int(n)}


def pointxy_problem(g):
    """The same poses, landmarks and pairs observed through EdgeSE2PointXY (type 3): the calibrated sensor's measurements read as
    a centred sensor's (the timing does not depend on the values)."""
    out = {k: v for k, v in g.items() if k not in ("qp", "ql", "qc", "zq", "omega_q")}
    out.update(vp=g["qp"], vl=g["ql"], zl=g["zq"], omega_l=g["omega_q"], M=g["Q"])
    return out


def kernel_times(g, edge, kernel, n):
    s, graph = lm.setup_device_landmark_slam(g)
    for staged in (1, 0):
        s.setOption("pg_landmark_staged", staged)
        s.setProfiling(1)
        for jac in (False, True):
            s.pgSetEstimates(g["poses"], g["hidx"])
            s.pgLinearize(jac)                                # warm-up: code loading
            s.sync()
            s.kernelTimes(reset=True)
            per = []
            for r in range(args.kernel_reps):
                s.pgSetEstimates(g["poses"], g["hidx"])
                s.pgLinearize(jac)
                s.sync()
                t, k = s.kernelTimes(reset=True).get("pg_landmark_linearize", (0.0, 0))
                per.append(1e6 * t / max(k, 1))
            emit(dict(sizes(g, edge, n), what="kernel", kernel=kernel, slot="pg_landmark_linearize", staged=staged, jacobians=jac,
                      us_per_launch=spread(per), edges_per_second=n / (1e-6 * float(np.median(per)))))
        s.setProfiling(0)


class HostFed:
    """lm.py's graph protocol: the three sets evaluated by pointxy_calib.py at the estimates read back, uploaded through setEdgeData."""

    def __init__(self, s, g, ids):
        self.s, self.g, self.ids, self.J = s, g, ids, None

    def _feed(self, jac):
        g = self.g
        self.s.pgLinearize(jac)
        out = PC.pointxy_calib_edges(PC.FP64, self.s.pgGetEstimates(), self.s.pgGetLandmarkEstimates(), g["qp"], g["ql"], g["qc"], g["zq"],
                                     g["hidx"], g["pt_hidx"], jac)
        if jac:
            self.J = out[:3]
        err = out[3] if jac else out
        Jp, Jl, Jc = self.J
        for k, (A, B) in zip(self.ids, ((Jp, Jl), (Jp, Jc), (Jl, Jc))):
            self.s.setEdgeData(k, A, B, g["omega_q"], err)

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
    parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
    ids = []
    for (a, b), pt in zip(((h[g["qp"]], hl[g["ql"]]), (h[g["qp"]], h[g["qc"]]), (hl[g["ql"]], h[g["qc"]])), parts):
        ids.append(sh.addEdgeSet(2, a, b))
        sh.setEdgeSetParts(ids[-1], pt)
    sh.buildStructure(g["nP"], g["nL"], True)
    sh.pgSetEdges(q0, 1, g["vi"], g["vj"], g["Z"], g["omega"])
    sh.pgSetEstimates(g["poses"], h)
    sh.pgSetLandmarkEstimates(g["points"], hl)
    return sh, HostFed(sh, g, ids)


def lm_times(g, path, warm):
    s, graph = lm.setup_device_landmark_slam(g) if path == "device_front_end" else host_fed_setup(g)
    lm.optimize(graph, s, warm, "lm")                   # warm-up: lazy analysis, code loading
    s.pgSetEstimates(g["poses"], g["hidx"])
    s.pgSetLandmarkEstimates(g["points"], g["pt_hidx"])
    times = []
    done, chis, lams, trials = lm.optimize(graph, s, args.iterations, "lm", times=times)
    emit(dict(sizes(g, "EdgeSE2PointXYCalib", g["Q"]), what="lm_iteration", path=path, ms_per_lm_iteration=spread([1e3 * t for t in times]),
              lm_trials=[int(t) for t in trials], chi2=[float(c) for c in chis]))


if args.step == "host_fed":
    gh = S.make_pointxy_calib_slam(args.host_poses, args.host_landmarks, seed=args.seed)
    for path in ("device_front_end", "host_fed"):
        lm_times(gh, path, 1)
else:
    g = S.make_pointxy_calib_slam(args.poses, args.landmarks, seed=args.seed)
    if args.step == "lm":
        lm_times(g, "device_front_end", 1)
    elif args.step == "kernel":
        kernel_times(g, "EdgeSE2PointXYCalib", "pg_se2_pointxy_calib_linearize_kernel", g["Q"])
    else:
        kernel_times(pointxy_problem(g), "EdgeSE2PointXY", "pg_se2_pointxy_linearize_kernel", g["Q"])
