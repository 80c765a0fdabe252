"""Timing of the BA front end's pose-pose slot (EdgeSE3Expmap, g2ohip_ba_set_pose_edges) on the metric workload: 20 000 cameras,
200 000 points, 1 000 000 observations + odometry and loop-closure edges (synthetic.make_ba_odometry).  Appends to
profiles/ba_pose_edges.jsonl (one JSON object per line; --out for another file):

  iteration   ten LM iterations after two of warm-up, seconds per iteration (min / median / max), for
                device_resident   both sets produced on the device
                no_pose_set       the same graph without the pose set (what the front end could do before the slot existed)
                host_fed          the pose set from openslam_g2o_amd/se3expmap.py through setEdgeData, the cameras read back for
                                  every evaluation (what a caller without the slot has to do)
  stages      a second, profiled pass of five iterations per path (not the timed one: the event records are not free): seconds
              per iteration of every stage of g2ohip_get_stats and of every kernel slot of g2ohip_kernel_time, the launches per
              slot, and fused_path = neither the stand-alone landmark assembly nor the Hpl assembly was launched, i.e. the
              fused assembly and back-substitution of the projection set stayed in use
  producer    the evaluation stage of g2ohip_ba_linearize (stats: timeLinearize / timeResiduals) over twenty launches with and
              without the pose set bound, full linearization and error-only: the difference of the medians is the pose kernel
              (the stage timer covers the projection producer too; the front end has no slot of its own for the kernel)

Run on a machine with the GPU:  python tools/ba_pose_edges_time.py [--cams 20000 --points 200000 --iters 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import lm, se3expmap as X, synthetic as S  # noqa: E402


class Timed:
    """A graph of lm.optimize that notes when every iteration starts (its linearize call, behind a synchronisation)."""

    def __init__(self, graph, solver):
        self.g, self.s, self.t = graph, solver, []
        self.device_resident = getattr(graph, "device_resident", False)

    def linearize(self):
        self.s.sync()
        self.t.append(time.perf_counter())
        self.g.linearize()

    def __getattr__(self, name):
        return getattr(self.g, name)


class HostFedGraph:
    """The pose set fed from the host beside the device-resident projection set: cameras read back for every evaluation."""

    device_resident = False

    def __init__(self, s, prob, kp):
        self.s, self.pe, self.kp, self.J = s, prob["pose_edges"], kp, None

    def _feed(self, jac):
        cams, _ = self.s.baGetEstimates()
        out = X.pose_edges(cams, self.pe["vi"], self.pe["vj"], self.pe["meas"], jac)
        if jac:
            self.J = out[:2]
        self.s.setEdgeData(self.kp, self.J[0], self.J[1], self.pe["info"], out[2] if jac else out)

    def linearize(self):
        self._feed(True)
        self.s.baLinearize(True)

    def compute_active_errors(self):
        self._feed(False)
        self.s.baLinearize(False)

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


def host_fed(prob):
    from openslam_g2o_amd import capi
    pe = prob["pose_edges"]
    s = capi.HipBlockSolver(6, 3, 0)
    k = s.addEdgeSet(2, prob["v0"], prob["v1"])
    kp = s.addEdgeSet(6, pe["v0"], pe["v1"])
    s.buildStructure(prob["nP"], prob["nL"], True)
    s.baSetEdges(k, prob["cam_idx"], prob["pt_idx"], prob["meas"], None, prob["f"], prob["cx"], prob["cy"])
    s.baSetEstimates(prob["cams"], prob["cam_hidx"], prob["pts"], np.arange(prob["L"], dtype=np.int32))
    return s, HostFedGraph(s, prob, kp)


def summary(v):
    v = np.asarray(v, np.float64)
    return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()), n=int(len(v)))


def iterations(make, prob, iters, warmup=2):
    s, graph = make(prob)
    t = Timed(graph, s)
    done, chis, lams, trials = lm.optimize(t, s, warmup + iters, "lm")
    s.sync()
    stamps = t.t + [time.perf_counter()]
    per = np.diff(stamps)[warmup:]
    return dict(seconds=summary(per), iterations=int(done), trials=[int(x) for x in trials], chi2_first=float(chis[0]), chi2_last=float(chis[-1]))


STAGES = ("timeQuadraticForm", "timeSchurComplement", "timeNumericDecomposition", "timeLinearSolution", "timeBackSubstitution",
          "timeResiduals", "timeLinearize", "timeUpdate")


class Staged:
    """A graph of lm.optimize that adds up the stage times of g2ohip_get_stats once per LM trial, behind its update (the stages
    hold what the last call of each left)."""

    def __init__(self, graph, solver):
        self.g, self.s, self.sum, self.n = graph, solver, dict.fromkeys(STAGES, 0.0), 0
        self.device_resident = getattr(graph, "device_resident", False)

    def note(self):
        st = self.s.stats()
        for k in STAGES:
            self.sum[k] += st[k]
        self.n += 1

    def update(self):
        self.g.update()
        self.s.sync()
        self.note()                       # (behind the solve and the update of a trial: every stage of it has run)

    def __getattr__(self, name):
        return getattr(self.g, name)


def stages(make, prob, iters=5):
    s, graph = make(prob)
    lm.optimize(graph, s, 2, "lm")
    s.setProfiling(1)
    s.sync()
    s.kernelTimes(reset=True)
    t = Staged(graph, s)
    done, chis, lams, trials = lm.optimize(t, s, iters, "lm")
    s.sync()
    kt = s.kernelTimes(reset=True)
    return dict(iterations=int(done), trials=[int(x) for x in trials],
                stage_seconds_per_trial={k: v / max(t.n, 1) for k, v in t.sum.items()},
                kernel_seconds_per_iteration={k: v[0] / max(done, 1) for k, v in kt.items()},
                kernel_launches={k: int(v[1]) for k, v in kt.items()},
                fused_path=("assemble_vertex(landmark)" not in kt and "assemble_offdiag(Hpl)" not in kt))


def producer(prob, launches=20):
    out = {}
    pts_h = np.arange(prob["L"], dtype=np.int32)
    for name, pr in (("with_pose_set", prob), ("without_pose_set", {k: v for k, v in prob.items() if k != "pose_edges"})):
        s, _ = lm.setup_device_ba(pr)
        s.setProfiling(1)
        for jac, key, stat in ((True, "linearize", "timeLinearize"), (False, "residuals", "timeResiduals")):
            ts = []
            for _ in range(launches + 2):
                s.baSetEstimates(pr["cams"], pr["cam_hidx"], pr["pts"], pts_h)      # (same tables: invalidates the evaluation)
                s.baLinearize(jac)
                s.sync()
                ts.append(s.stats()[stat])
            out["%s_%s" % (key, name)] = summary(ts[2:])
    for key in ("linearize", "residuals"):
        out["pose_kernel_%s_median_difference" % key] = out[key + "_with_pose_set"]["median"] - out[key + "_without_pose_set"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=20000)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-every", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_pose_edges.jsonl"))
    a = ap.parse_args()
    prob = S.make_ba_odometry(a.cams, a.points, loop_every=a.loop_every)
    plain = {k: v for k, v in prob.items() if k != "pose_edges"}
    head = dict(cams=a.cams, points=a.points, observations=int(prob["E"]), pose_edges=int(prob["pose_edges"]["n"]), loop_every=a.loop_every)
    lines = []
    for name, make, pr in (("device_resident", lm.setup_device_ba, prob), ("no_pose_set", lm.setup_device_ba, plain), ("host_fed", host_fed, prob)):
        lines.append(dict(what="iteration", path=name, **head, **iterations(make, pr, a.iters)))
        print(json.dumps(lines[-1]), flush=True)
    for name, make, pr in (("device_resident", lm.setup_device_ba, prob), ("no_pose_set", lm.setup_device_ba, plain), ("host_fed", host_fed, prob)):
        lines.append(dict(what="stages", path=name, **head, **stages(make, pr)))
        print(json.dumps(lines[-1]), flush=True)
    lines.append(dict(what="producer", **head, **producer(prob)))
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
