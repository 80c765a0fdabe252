#!/usr/bin/env python
"""Anchored inverse-depth bundle adjustment (EdgeProjectPSI2UV, openslam_g2o_amd.synthetic.make_ba_inverse_depth):

  ms per Levenberg-Marquardt iteration at --cameras / --points (x 5 observations), after a warm-up, median and range of at least
  --iterations iterations, for
    psi_device           the device producer (g2ohip_ba_set_inverse_depth_edges: estimates, errors, Jacobians stay on the device)
    psi_host_numpy       the same library and the same three edge sets fed host arrays from openslam_g2o_amd/psi2uv.py through
                         setEdgeData every evaluation; estimates, oplus, push / pop stay in the front end's tables on the device
    mono_generic         EdgeProjectXYZ2UV of the same scene on the device with ba_fused = 0 (the same generic assembly, one set)
  then the inverse-depth producer alone (the `linearize` / `residuals` stage timers of g2ohip_get_stats), with Jacobians and
  error-only, over --kernel-reps launches.

One JSON line per result on stdout, appended to --out if given.
  python tools/ba_psi_time.py [--cameras 20000 --points 200000] [--iterations 10] [--out profiles/ba_psi2uv.jsonl]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openslam_g2o_amd import capi, lm, psi2uv, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--cameras", type=int, default=20000)
ap.add_argument("--points", type=int, default=200000)
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


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def timed_run(graph, solver, reset, warmup=3):
    """ms of every LM iteration of runs of at least --iterations iterations from the initial estimates, after a warm-up run."""
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


psi = S.make_ba_inverse_depth(args.cameras, args.points)
mono = S.make_ba_problem(args.cameras, args.points)
size = {"cameras": psi["P"], "points": psi["L"], "observations": int(psi["E"])}
pt_h = np.arange(psi["L"], dtype=np.int32)


def device_path(prob, name, options):
    s, graph = lm.setup_device_ba(prob, options=dict(options, use_graph=1))
    ms, chis, trials = timed_run(graph, s, lambda: s.baSetEstimates(prob["cams"], prob["cam_hidx"], prob["pts"], pt_h))
    emit(dict(size, what="lm_iteration", path=name, ms_per_lm_iteration=spread(ms), lm_trials=trials, chi2=chis))
    return s


s = device_path(psi, "psi_device", {})
# the producer alone: with Jacobians (30 + 2 doubles per edge written) and error-only (2)
s.setProfiling(1)
for jac, stage in ((True, "timeLinearize"), (False, "timeResiduals")):
    us = []
    for r in range(args.kernel_reps + 2):
        s.baSetEstimates(psi["cams"], psi["cam_hidx"], psi["pts"], pt_h)      # (same tables: only invalidates the evaluation)
        s.baLinearize(jac)
        s.sync()
        if r >= 2:
            us.append(1e6 * s.stats()[stage])
    nbytes = psi["E"] * (3 * 4 + 8 * 2 + 8 * 2 + (8 * 30 if jac else 0)) + 8 * (12 * psi["P"] + 3 * psi["L"])
    sp = spread(us)
    emit(dict(size, what="psi_linearize", jacobians=jac, us_per_launch=sp, algorithmic_bytes=int(nbytes),
              bytes_per_second=nbytes / (1e-6 * sp["median"]) if sp["median"] > 0 else 0.0))
s.setProfiling(0)
del s
device_path(mono, "mono_generic", {"ba_fused": 0})


class HostFedGraph:
    """lm.py's graph protocol: the three sets fed from psi2uv.py through setEdgeData, the estimates in the device tables."""

    device_resident = False

    def __init__(self, s, prob, ids):
        self.s, self.g, self.ids, self.J = s, prob, ids, None
        self.om = S.ba_omega(prob)

    def _feed(self, jac):
        cams, pts = self.s.baGetEstimates()
        out = psi2uv.problem_edges(self.g, cams, pts, jac)
        if jac:
            self.J = out[:3]
        jp, jc, ja = self.J
        err = out[3] if jac else out
        for k, (a, b) in zip(self.ids, ((jp, jc), (jp, ja), (jc, ja))):
            self.s.setEdgeData(k, a, b, self.om, err)

    def linearize(self):
        self._feed(True)

    def compute_active_errors(self):
        self._feed(False)

    def chi2(self):
        return self.s.chi2()

    def update(self):
        self.s.baUpdate()

    def push(self):
        self.s.baPush()

    def pop(self):
        self.s.baPop()

    def discard_top(self):
        self.s.baDiscardTop()


if not args.skip_host:
    h = capi.HipBlockSolver(6, 3, 0)
    h.setOption("use_graph", 1)
    parts = (0, capi.PART_NO_VERTEX0 | capi.PART_NO_VERTEX1 | capi.PART_NO_CHI2, capi.PART_NO_VERTEX0 | capi.PART_NO_CHI2)
    ids = []
    for (v0, v1), pt in zip(psi["pairs"], parts):
        ids.append(h.addEdgeSet(2, v0, v1))
        h.setEdgeSetParts(ids[-1], pt)
    h.buildStructure(psi["nP"], psi["nL"], True)
    h.baSetEstimates(psi["cams"], psi["cam_hidx"], psi["pts"], pt_h)
    host = HostFedGraph(h, psi, ids)
    ms, chis, trials = timed_run(host, h, lambda: h.baSetEstimates(psi["cams"], psi["cam_hidx"], psi["pts"], pt_h), warmup=1)
    emit(dict(size, what="lm_iteration", path="psi_host_numpy", ms_per_lm_iteration=spread(ms), lm_trials=trials, chi2=chis))
