#!/usr/bin/env python
"""Stereo bundle adjustment (EdgeProjectXYZ2UVU, openslam_g2o_amd.synthetic.make_ba_problem(..., stereo_baseline=b)):

  default   ms per Levenberg-Marquardt iteration at --cameras / --points (x 5 observations), after a warm-up, median and range
            of at least --iterations iterations, for
              stereo_device          the device producer (g2ohip_ba_set_stereo_edges: estimates, errors, Jacobians stay on the device)
              stereo_host_numpy      the same library fed host arrays from the NumPy restatement (tests/stereo_helpers.py) through
                                     setEdgeData every trial, estimates / oplus / push / pop on the host
              mono_generic           EdgeProjectXYZ2UV on the device with ba_fused = 0 (the same generic path, d = 2)
              mono_fused             ... with the fused assembly (the headline path)
            then the stereo producer alone (the `linearize` stage timer of g2ohip_get_stats), both store forms, Jacobians on.
  --drift   CPU only: how far two equally valid oracle runs of tests/stereo_helpers.lm_test_graph() drift apart per LM iteration (the
            oracle's Schur path against the full system solved without elimination) -- the bound of
            tests/test_gpu_stereo_ba.py::test_lm_run_matches_oracle is ten times this.

One JSON line per result on stdout, appended to --out if given.
  python tools/ba_stereo_time.py [--drift] [--cameras 20000 --points 200000] [--iterations 10] [--out f]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openslam_g2o_amd import lm, synthetic as S
from tests import stereo_helpers as SH

ap = argparse.ArgumentParser()
ap.add_argument("--drift", action="store_true")
ap.add_argument("--cameras", type=int, default=20000)
ap.add_argument("--points", type=int, default=200000)
ap.add_argument("--baseline", type=float, default=0.2)
ap.add_argument("--iterations", type=int, default=10)
ap.add_argument("--kernel-reps", type=int, default=20)
ap.add_argument("--skip-host", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if args.drift:
    g = SH.lm_test_graph()
    a = SH.oracle_lm_run(g, 10, dense=False)
    b = SH.oracle_lm_run(g, 10, dense=True)
    emit({"what": "oracle_drift", "kind": "stereo", "cameras": g["P"], "points": g["L"], "observations": int(g["E"]),
          "relative_chi2_gap": [abs(x - y) / y for x, y in zip(a[1], b[1])], "chi2_schur": a[1], "trials_schur": a[3],
          "trials_full_system": b[3]})
    sys.exit(0)

from openslam_g2o_amd import capi


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def timed_run(graph, solver, reset, warmup=3):
    """ms of every LM iteration of one run of at least --iterations iterations from the initial estimates, after a warm-up run."""
    lm.optimize(graph, solver, warmup, "lm")            # lazy analysis, graph capture, allocations
    ms, chis, trials = [], [], []
    while len(ms) < args.iterations:
        reset()
        solver.sync()
        t = []
        done, c, _, tr = lm.optimize(graph, solver, args.iterations - len(ms), "lm", times=t)
        solver.sync()
        ms += [1e3 * x for x in t]
        chis += c
        trials += tr
    return ms, chis, trials


stereo = S.make_ba_problem(args.cameras, args.points, stereo_baseline=args.baseline)
mono = S.make_ba_problem(args.cameras, args.points)
size = {"cameras": stereo["P"], "points": stereo["L"], "observations": int(stereo["E"]), "baseline": args.baseline}
pt_h = np.arange(stereo["L"], dtype=np.int32)


def device_path(prob, name, options):
    s, graph = lm.setup_device_ba(prob, options=dict(options, use_graph=1))
    ms, chis, trials = timed_run(graph, s, lambda: s.baSetEstimates(prob["cams"], prob["cam_hidx"], prob["pts"], pt_h))
    emit(dict(size, what="lm_iteration", path=name, ms_per_lm_iteration=spread(ms), lm_trials=trials, chi2=chis))
    return s


s = device_path(stereo, "stereo_device", {})
# the producer alone, both store forms
s.setProfiling(1)
for staged in (1, 0):
    s.setOption("ba_stereo_staged", staged)
    us = []
    for r in range(args.kernel_reps + 2):
        s.baSetEstimates(stereo["cams"], stereo["cam_hidx"], stereo["pts"], pt_h)      # (same tables: only invalidates the evaluation)
        s.baLinearize(True)
        s.sync()
        if r >= 2:
            us.append(1e6 * s.stats()["timeLinearize"])
    nbytes = stereo["E"] * (8 + 8 * 3 + 8 * 30) + 8 * (12 * stereo["P"] + 3 * stereo["L"])
    sp = spread(us)
    emit(dict(size, what="stereo_linearize", staged=staged, jacobians=True, us_per_launch=sp, algorithmic_bytes=int(nbytes),
              bytes_per_second=nbytes / (1e-6 * sp["median"]) if sp["median"] > 0 else 0.0))
s.setProfiling(0)
del s
device_path(mono, "mono_generic", {"ba_fused": 0})
device_path(mono, "mono_fused", {})

if not args.skip_host:
    h = capi.HipBlockSolver(6, 3, 0)
    h.setOption("use_graph", 1)
    k = h.addEdgeSet(3, stereo["v0"], stereo["v1"])
    h.buildStructure(stereo["nP"], stereo["nL"], True)
    host = SH.HostStereoGraph(stereo, lambda J0, J1, om, err: h.setEdgeData(k, J0, J1, om, err), h.x, h.chi2)

    def reset_host():
        host.pr["cams"], host.pr["pts"] = stereo["cams"].copy(), stereo["pts"].copy()
    ms, chis, trials = timed_run(host, h, reset_host, warmup=1)
    emit(dict(size, what="lm_iteration", path="stereo_host_numpy", ms_per_lm_iteration=spread(ms), lm_trials=trials, chi2=chis))
