"""Timing of the SBA group's pose-pose sets (EdgeSBACam / EdgeSBAScale, g2ohip_pg_set_cam_edges) on the metric workload: 20 000
cameras, 200 000 points, 1 000 000 observations + odometry and loop-closure EdgeSBACam edges and a handful of EdgeSBAScale edges
(synthetic.make_sbacam_ba with cam_edges / scale_edges).  Appends to profiles/sba_cam_edges.jsonl (one JSON object per line;
--out for another file):

  iteration   --iters LM iterations after two of warm-up, seconds per iteration (min / median / max), for
                device_resident   all three sets produced on the device
                no_pose_sets      the same graph without the two sets (what the front end could do before the slots existed)
                host_fed          the two sets evaluated on the host (the formulas of openslam_g2o_amd/sbacam.py, vectorised over
                                  the edges with NumPy) and uploaded through setEdgeData, the cameras read back for every
                                  evaluation (what a caller without the slots has to do)
  stages      seconds per iteration of every stage of g2ohip_get_stats over a second, profiled pass of the device-resident and
              the no_pose_sets path: where the difference goes
  producer    the "pg_landmark_linearize" kernel slot (it covers the projection producer and the new kernels) over twenty launches
              with and without the two sets bound, full linearization and error-only: the difference of the medians is the new
              kernels
  bit_equal   on the graphs of tests/golden/sbacam_pose_edges.npz: does the device equal the fp64 restatement bit for bit?

Run on a machine with the GPU:  python tools/sba_cam_edges_time.py [--cams 20000 --points 200000 --iters 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import lm, sbacam as SB, synthetic as S  # noqa: E402

DELTA = 1e-9


# ---- the formulas of sbacam.py over arrays of edges (timing only: the operation order inside NumPy's reductions is not pinned)
def _qmul(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=1)


def _qrot(q, v):
    uv = 2.0 * np.cross(q[:, :3], v)
    return v + q[:, 3:4] * uv + np.cross(q[:, :3], uv)


def _normalize_rotation(q):
    q = np.where(q[:, 3:4] < 0, -q, q)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _mul(a, b):
    return np.concatenate([a[:, :3] + _qrot(a[:, 3:], b[:, :3]), _normalize_rotation(_qmul(a[:, 3:], b[:, 3:]))], axis=1)


def _inverse(a):
    q = a[:, 3:] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([_qrot(q, -a[:, :3]), q], axis=1)


def _oplus(c, u):
    qr = np.concatenate([u[:, 3:], np.sqrt(1.0 - (u[:, 3:] ** 2).sum(axis=1, keepdims=True))], axis=1)
    p = _qmul(c[:, 3:], qr)
    return np.concatenate([c[:, :3] + u[:, :3], p / np.linalg.norm(p, axis=1, keepdims=True)], axis=1)


def _cam_error(ci, cj, zinv):
    return _mul(zinv, _mul(_inverse(ci), cj))[:, :6]


def _scale_error(ci, cj, z):
    return (z - np.linalg.norm(cj[:, :3] - ci[:, :3], axis=1))[:, None]


def host_edges(error, cams, vi, vj, hidx, d, jac):
    ci, cj = cams[vi], cams[vj]
    err = error(ci, cj)
    if not jac:
        return err
    n = len(vi)
    J = [np.zeros((n, 6 * d)), np.zeros((n, 6 * d))]
    for side in range(2):
        for c in range(6):
            u = np.zeros((n, 6))
            u[:, c] = DELTA
            base = cj if side else ci
            p, m = _oplus(base, u), _oplus(base, -u)
            diff = (error(ci, p) - error(ci, m)) if side else (error(p, cj) - error(m, cj))
            J[side][:, d * c:d * c + d] = diff * (1.0 / (2 * DELTA))
        J[side][hidx[vj if side else vi] < 0] = 0.0
    return J[0], J[1], err


class Timed:
    """A graph of lm.optimize that notes when every iteration starts (its linearize call, behind a synchronisation)."""

    def __init__(self, graph, solver):
        self.g, self.s, self.t = graph, solver, []

    def linearize(self):
        self.s.sync()
        self.t.append(time.perf_counter())
        self.g.linearize()

    def __getattr__(self, name):
        return getattr(self.g, name)


class HostFedGraph:
    def __init__(self, s, prob, kc, ks):
        self.s, self.p, self.kc, self.ks, self.J = s, prob, kc, ks, {}
        self.zinv = _inverse(np.concatenate([prob["cam_edges"]["meas"][:, :3], _normalize_rotation(prob["cam_edges"]["meas"][:, 3:])], axis=1))

    def _feed(self, jac):
        self.s.pgLinearize(jac)
        cams = self.s.pgGetEstimates()
        ce, se, h = self.p["cam_edges"], self.p["scale_edges"], self.p["hidx"]
        for k, e, d, fn in ((self.kc, ce, 6, lambda a, b: _cam_error(a, b, self.zinv)), (self.ks, se, 1, lambda a, b: _scale_error(a, b, se["meas"]))):
            r = host_edges(fn, cams, e["vi"], e["vj"], h, d, jac)
            if jac:
                self.J[k] = r[:2]
            self.s.setEdgeData(k, self.J[k][0], self.J[k][1], e["info"], r[2] if jac else r)

    linearize = lambda self: self._feed(True)
    compute_active_errors = lambda self: self._feed(False)
    chi2 = lambda self: self.s.chi2()
    update = lambda self: self.s.pgUpdate()
    push = lambda self: self.s.pgPush()
    pop = lambda self: self.s.pgPop()
    discard_top = lambda self: self.s.pgDiscardTop()


def host_fed_setup(prob):
    from openslam_g2o_amd import capi
    s = capi.HipBlockSolver(6, 3, 0)
    h, none = np.asarray(prob["hidx"], np.int32), np.zeros(0, np.int32)
    k0 = s.addEdgeSet(6, none, none)
    k1 = s.addEdgeSet(prob["zl"].shape[1], h[prob["vp"]], prob["pt_hidx"][prob["vl"]])
    kc = s.addEdgeSet(6, h[prob["cam_edges"]["vi"]], h[prob["cam_edges"]["vj"]])
    ks = s.addEdgeSet(1, h[prob["scale_edges"]["vi"]], h[prob["scale_edges"]["vj"]])
    s.buildStructure(prob["nP"], prob["nL"], True)
    s.pgSetEdges(k0, 12, none, none, np.zeros((0, 7)), np.zeros((0, 36)))
    s.pgSetEstimates(prob["est"], h)
    s.pgSetCamProjectEdges(k1, 11 + prob["zl"].shape[1], prob["vp"], prob["vl"], prob["zl"], prob["omega_l"], prob["intrinsics"])
    s.pgSetLandmarkEstimates(prob["points"], prob["pt_hidx"])
    return s, HostFedGraph(s, prob, kc, ks)


def run(name, s, graph, iters, profile=False):
    s.setProfiling(profile)
    t = Timed(graph, s)
    done, chis, _, trials = lm.optimize(t, s, iters + 2, "lm")
    s.sync()
    t.t.append(time.perf_counter())
    dt = np.diff(np.array(t.t))[2:]
    rec = dict(kind="stages" if profile else "iteration", path=name, iterations=int(len(dt)), chi2=[float(c) for c in chis],
               trials=[int(v) for v in trials], s_min=float(dt.min()), s_median=float(np.median(dt)), s_max=float(dt.max()))
    if profile:
        rec["stats_last_iteration"] = {k: float(v) for k, v in s.stats().items() if k.startswith("time")}
    return rec


def producer(prob, with_sets, launches=20):
    p = prob if with_sets else {k: v for k, v in prob.items() if k not in ("cam_edges", "scale_edges")}
    s, graph = lm.setup_device_sbacam_ba(p)
    out = {}
    for jac in (True, False):
        ts = []
        for _ in range(launches + 2):
            s.pgSetEstimates(p["est"], p["hidx"])
            s.sync()
            t0 = time.perf_counter()
            s.pgLinearize(jac)
            s.sync()
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts[2:])
        out["full" if jac else "error_only"] = dict(s_min=float(ts.min()), s_median=float(np.median(ts)), s_max=float(ts.max()))
    return out


def bit_equal():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sbacam_pose_edges.npz"))
    out = {}
    for name, scale in [("branch", False), ("coincident", True)] + [("c%d" % n, False) for n in (1, 21, 22, 257, 300)] + [("s%d" % n, True) for n in (1, 21, 22, 257, 300)]:
        g = {k: gold["%s_%s" % (name, k)] for k in ("est", "hidx", "vi", "vj", "meas", "info")}
        prob = dict(est=g["est"], hidx=g["hidx"], nP=int(g["hidx"].max()) + 1)
        prob["scale_edges" if scale else "cam_edges"] = dict(vi=g["vi"], vj=g["vj"], meas=g["meas"], info=g["info"])
        s, graph = lm.setup_device_sbacam_ba(prob)
        graph.linearize()
        dev = s.edgeData(s.scale_set if scale else s.cam_set, len(g["vi"]), 1 if scale else 6, 6, 6)
        ref = SB.pose_edges(SB.FP64, g["est"], g["vi"], g["vj"], g["meas"], g["hidx"], scale=scale)
        out[name] = bool(all(np.array_equal(a, b) for a, b in zip(dev, ref)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=20000)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--obs", type=int, default=5)
    ap.add_argument("--loop-every", type=int, default=10)
    ap.add_argument("--scale-edges", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--skip-host-fed", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sba_cam_edges.jsonl"))
    a = ap.parse_args()
    prob = S.make_sbacam_ba(a.cams, a.points, a.obs, seed=3, cam_edges=a.loop_every, scale_edges=a.scale_edges)
    plain = {k: v for k, v in prob.items() if k not in ("cam_edges", "scale_edges")}
    head = dict(cams=a.cams, points=a.points, observations=int(len(prob["vp"])), cam_edges=int(len(prob["cam_edges"]["vi"])),
                scale_edges=int(len(prob["scale_edges"]["vi"])), loop_every=a.loop_every)
    lines = [dict(kind="bit_equal", device_equals_fp64_restatement=bit_equal())]
    print(lines[-1], flush=True)
    for name, setup in (("device_resident", lambda: lm.setup_device_sbacam_ba(prob)), ("no_pose_sets", lambda: lm.setup_device_sbacam_ba(plain)),
                        ("host_fed", lambda: host_fed_setup(prob))):
        if name == "host_fed" and a.skip_host_fed:
            continue
        s, graph = setup()
        lines.append(dict(run(name, s, graph, a.iters), **head))
        print(lines[-1], flush=True)
        if name != "host_fed":
            s, graph = setup()
            lines.append(dict(run(name, s, graph, 5, profile=True), **head))
            print(lines[-1], flush=True)
    w, wo = producer(prob, True), producer(prob, False)
    lines.append(dict(kind="producer", with_sets=w, without_sets=wo,
                      new_kernels_full_s=w["full"]["s_median"] - wo["full"]["s_median"],
                      new_kernels_error_only_s=w["error_only"]["s_median"] - wo["error_only"]["s_median"], **head))
    print(lines[-1], flush=True)
    with open(a.out, "a") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
