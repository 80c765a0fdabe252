"""Test side of the structure-only bundle adjustment (g2ohip_ba_structure_only): the restatement of
openslam_g2o_amd/structure_only.py -- ONE body, generic over the arithmetic -- in fp64 (FP64) and with mpmath at 60 digits (MP);
the small graphs of the tests with every special case of a track; the device set-up; the goldens of tests/golden/structure_only.npz
(written by tests/golden/make_structure_only.py)."""
import json
import os

import mpmath as mp
import numpy as np

from openslam_g2o_amd import structure_only as SO
from openslam_g2o_amd.structure_only import FP64  # noqa: F401

DPS = 60
mp.mp.dps = DPS
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "structure_only.npz")
PROFILE = os.path.join(os.path.dirname(HERE), "profiles", "structure_only.jsonl")
MARGIN_FACTOR = 1000.0
# Outer iterations of the runs whose TRACES are compared.  Every decision of such a run has to clear its threshold by 1000 x the
# largest fp64-vs-60-digit difference of that quantity on the graph, and no graph of this shape does at more than one iteration:
#  - a point displaced by 0.5 starts at chi2 ~ 1e5, whose fp64 error (1e-9 .. 1e-8 measured) is the difference of the chi2 drops of
#    the graph, so every accepted drop has to exceed ~1e-5; a point that has converged drops chi2 by |b|^2 / H ~ 1e-12 per step
#    until |b| < 0.001 stops it (measured at ten iterations: margins 1e-12 .. 1e-20 on every seed at 1, 0.5 and 0.25 px noise);
#  - a mono track of ONE observation leaves H of rank 2, the first step divides rounding noise by mu = 0.01 along the ray, and
#    |b| of the second iteration differs by ~1e-5 between the arithmetics: 1000 x that is above the threshold 0.001 itself
#    (measured at two iterations: no seed of 48 on the fused mono graph).
# The first iteration holds every kind of decision -- |b| against 0.001 (point 149 stops there), the pivots, the chi2 drop, and
# rejected trials -- with the quantities computed from identical inputs in both arithmetics.  What later
# iterations add (mu and nu carried over, trial restarting, the stops on the way, lanes of a wave finishing at different times) is
# held by the TEN-iteration runs, whose traces are compared on every point as well, under the condition that fits them: every
# decision of the 60-digit run is at least 1000 x the fp64-vs-60-digit difference OF THAT DECISION away from its threshold (the
# error of the arithmetic at the place where the decision is taken, instead of the largest one anywhere on the graph).  The
# generator draws seeds, and shrinks the noise, until both conditions hold.
TRACE_ITERS = 1
THRESHOLD = {SO.DECISION_GRADIENT: SO.B_STOP, SO.DECISION_PIVOT: 0.0, SO.DECISION_RHO: 0.0}


class MP:
    name = "mp"
    sqrt = mp.sqrt
    isfinite = staticmethod(lambda x: bool(mp.isfinite(x)))

    @staticmethod
    def num(x):
        return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


# the graphs: name -> (stereo, specials (a 70-observation track, a fixed point, a repeated observation), general information,
# kernel (kind, delta), edge classes)
SPECS = {
    "mono_general": dict(stereo=False, specials=True, info=True, kernel=(1, 2.0), classes=False),
    "mono_fused": dict(stereo=False, specials=False, info=False, kernel=(0, 0.0), classes=False),
    "mono_classes": dict(stereo=False, specials=False, info=True, kernel=(0, 0.0), classes=True),
    "stereo_general": dict(stereo=True, specials=True, info=True, kernel=(1, 2.0), classes=False),
    "stereo_identity": dict(stereo=True, specials=False, info=False, kernel=(0, 0.0), classes=False),
    # the other two lane-group widths (the mean track length picks it: <= 2 -> 1 lane, <= 16 -> 4, above -> 8), on fewer points
    "mono_short": dict(stereo=False, specials=False, info=False, kernel=(0, 0.0), classes=False, L=83, cycle=(1, 2, 2, 1, 2)),
    "stereo_short": dict(stereo=True, specials=False, info=True, kernel=(1, 2.0), classes=False, L=83, cycle=(1, 2, 2, 1, 2)),
    "mono_long": dict(stereo=False, specials=False, info=True, kernel=(1, 2.0), classes=False, L=37, cycle=(21, 14, 28, 17)),
    "stereo_long": dict(stereo=True, specials=False, info=False, kernel=(0, 0.0), classes=False, L=37, cycle=(21, 14, 28, 17)),
}
P, L, F_PX, CX, CY, BASELINE = 7, 150, 1000.0, 320.0, 240.0, 0.3
TRACK_CYCLE = (1, 2, 5, 3, 7, 4)


def special(g):
    """Indices of (the outlier point of the graphs with the special tracks, the empty track, the point seen only by the fixed
    cameras, the converged start): the last four points."""
    n = len(g["pts"])
    return n - 4, n - 3, n - 2, n - 1


def make_graph(name, seed, noise=1.0, displace=0.5, zmin=3.0):
    """7 cameras (2 fixed), 150 points (fewer where SPECS says so), f = 1000, `noise` px on the observations, points displaced by up to `displace`.
    Every graph: track lengths 1, 2, 5 (and 3, 4, 7), a free point with an EMPTY track (147), a point seen only by the fixed
    cameras (148), a point that starts converged (149: exact observations, estimate = truth).  specials: point 0 has a track of
    70 (every camera ten times), point 1 is fixed, point 2's first observation is repeated, and point 146 (track of 5, the first
    observation 60 px off) starts half way between the truth and the optimum of the raw least squares: these graphs carry a Huber
    kernel, the weighted step goes towards the inliers and the raw chi2 rises (the generator keeps a seed only if some point's
    first trial is rejected)."""
    spec = SPECS[name]
    rng = np.random.default_rng(seed)
    d = 3 if spec["stereo"] else 2
    L, cycle = spec.get("L", 150), spec.get("cycle", TRACK_CYCLE)       # (the docstring's point numbers are those of L = 150)
    i_out, i_empty, i_fixedcam, i_conv = L - 4, L - 3, L - 2, L - 1
    cams = np.zeros((P, 12))
    cams[:, 0] = cams[:, 4] = cams[:, 8] = 1.0
    cams[:, 9] = -np.arange(P) * 0.5
    for c in range(2, P):    # free cameras: a small rotation about y and a shift (frozen here, whatever their state)
        a = 0.02 * rng.normal()
        cams[c, [0, 2, 6, 8]] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
        cams[c, 9:12] += 0.01 * rng.normal(size=3)
    true = np.stack([rng.uniform(-1.0, 4.0, L), rng.uniform(-0.5, 0.5, L), rng.uniform(zmin, 4.0, L)], axis=1)
    cam_idx, pt_idx = [], []
    for v in range(L):
        K = cycle[v % len(cycle)]
        first = int(rng.integers(0, P - min(K, P) + 1))
        track = [(first + j) % P for j in range(K)]           # (longer than P: cameras repeat)
        if v == i_empty:
            track = []
        elif v == i_fixedcam:
            track = [0, 1]
        elif spec["specials"] and v == 0:
            track = list(range(P)) * 10
        elif spec["specials"] and v == 2:
            track = [track[0]] + track
        cam_idx += track
        pt_idx += [v] * len(track)
    cam_idx, pt_idx = np.array(cam_idx, np.int32), np.array(pt_idx, np.int32)
    E = len(cam_idx)
    T, X = cams[cam_idx], true[pt_idx]
    xc = np.stack([T[:, 0 + r] * X[:, 0] + T[:, 3 + r] * X[:, 1] + T[:, 6 + r] * X[:, 2] + T[:, 9 + r] for r in range(3)], axis=1)
    cols = [xc[:, 0] / xc[:, 2] * F_PX + CX, xc[:, 1] / xc[:, 2] * F_PX + CY]
    if spec["stereo"]:
        cols.append((xc[:, 0] - BASELINE) / xc[:, 2] * F_PX + CX)
    meas = np.stack(cols, axis=1)
    if spec["classes"]:      # the second class: another camera model (its observations are rescaled to it) and a Huber kernel
        edge_class = (rng.uniform(size=E) < 0.4).astype(np.int32)
        class_params = np.array([[F_PX, CX, CY, 0.0, 0.0], [800.0, 300.0, 250.0, 1.0, 2.0]])
        c1 = edge_class == 1
        meas[c1, 0] = xc[c1, 0] / xc[c1, 2] * 800.0 + 300.0
        meas[c1, 1] = xc[c1, 1] / xc[c1, 2] * 800.0 + 250.0
    exact = pt_idx == i_conv
    meas[~exact] += noise * rng.normal(size=(E, d))[~exact]
    pts = true + rng.uniform(-displace, displace, (L, 3))
    pts[i_conv] = true[i_conv]
    pt_hidx = np.arange(L, dtype=np.int32)
    if spec["specials"]:
        pt_hidx[1] = -1
        pt_hidx[2:] -= 1
    if spec["specials"]:
        k146 = np.flatnonzero(pt_idx == i_out)
        meas[k146[0], 0] += 60.0
        sub = dict(cams=cams, pts=true[i_out:i_out + 1], meas=meas[k146], cam_idx=cam_idx[k146], pt_idx=np.zeros(len(k146), np.int32), f=F_PX,
                   cx=CX, cy=CY)
        if spec["stereo"]:
            sub.update(observation="stereo", baseline=BASELINE)
        ls = SO.to_f64(SO.structure_only(sub, 10, 10)[0])[0]
        pts[i_out] = 0.5 * (true[i_out] + ls)
    nL = int(pt_hidx.max()) + 1
    cam_hidx = np.arange(P, dtype=np.int32) - 2
    cam_hidx[:2] = -1
    nP = P - 2
    g = dict(P=P, L=L, E=E, nP=nP, nL=nL, f=F_PX, cx=CX, cy=CY, cams=cams, pts=pts, pts_true=true, meas=meas, cam_idx=cam_idx,
             pt_idx=pt_idx, cam_hidx=cam_hidx, pt_hidx=pt_hidx,
             v0=np.where(pt_hidx[pt_idx] < 0, -1, nP + pt_hidx[pt_idx]).astype(np.int32), v1=cam_hidx[cam_idx].astype(np.int32))
    if spec["stereo"]:
        g.update(observation="stereo", baseline=BASELINE)
    if spec["info"]:
        A = rng.normal(size=(E, d, d)) * 0.3
        g["info"] = (A @ A.transpose(0, 2, 1) + np.eye(d)).reshape(E, d * d)
    if spec["classes"]:
        g.update(class_params=class_params, edge_class=edge_class)
    return g


GRAPH_KEYS = ("cams", "pts", "pts_true", "meas", "cam_idx", "pt_idx", "cam_hidx", "pt_hidx", "v0", "v1", "info", "class_params", "edge_class")


def run(F, g, name, num_iters=TRACE_ITERS, num_max_trials=10, decisions=None):
    pts, trace, chi = SO.structure_only(g, num_iters, num_max_trials, SPECS[name]["kernel"], F, decisions)
    return pts, np.array(trace, np.int32), chi


def compare(g, name, num_iters=TRACE_ITERS, num_max_trials=10):
    """The fp64 run against the 60-digit run: traces, the drift of the points and of chi2 (largest absolute difference), and per
    kind of decision the smallest margin of the 60-digit run and the largest fp64-vs-60-digit difference of that quantity."""
    d64, dmp = [], []
    p64, t64, c64 = run(FP64, g, name, num_iters, num_max_trials, d64)
    pmp, tmp_, cmp_ = run(MP, g, name, num_iters, num_max_trials, dmp)
    out = dict(trace_equal=bool(np.array_equal(t64, tmp_)), trace=tmp_, pts=SO.to_f64(pmp), chi2=SO.to_f64(cmp_), pts64=SO.to_f64(p64),
               chi264=SO.to_f64(c64))
    out["drift_pts"] = float(max(abs(mp.mpf(a) - b) for ra, rb in zip(p64, pmp) for a, b in zip(ra, rb)))
    out["drift_chi2"] = float(max(abs(mp.mpf(a) - b) for ra, rb in zip(c64, cmp_) for a, b in zip(ra, rb)))
    same_path = len(d64) == len(dmp) and all(a[:2] == b[:2] for a, b in zip(d64, dmp))
    out["same_path"] = same_path
    out["decisions"] = np.array([(v, list(THRESHOLD).index(k), float(x)) for v, k, x in dmp], np.float64).reshape(-1, 3)
    margin, diff = {}, {}
    for k, thr in THRESHOLD.items():
        margin[k] = float(min([abs(x - mp.mpf(thr)) for _, kk, x in dmp if kk == k] or [mp.inf]))
        diff[k] = float(max([abs(mp.mpf(a[2]) - b[2]) for a, b in zip(d64, dmp) if b[1] == k] or [0.0])) if same_path else float("inf")
    out["margin"], out["diff"] = margin, diff
    out["margins_ok"] = same_path and all(margin[k] >= MARGIN_FACTOR * diff[k] for k in THRESHOLD)
    # per decision: (point, kind, value of the 60-digit run, |fp64 - 60 digits| of that decision)
    each = [(b[0], list(THRESHOLD).index(b[1]), float(b[2]), float(abs(mp.mpf(a[2]) - b[2]))) for a, b in zip(d64, dmp)] if same_path else []
    out["each"] = np.array(each, np.float64).reshape(-1, 4)
    out["each_ok"] = same_path and each_ok(out["each"])
    return out


def each_ok(each):
    thr = np.array([THRESHOLD[k] for k in THRESHOLD])[each[:, 1].astype(int)]
    return bool((np.abs(each[:, 2] - thr) >= MARGIN_FACTOR * each[:, 3]).all())


def load_golden():
    z = np.load(GOLDEN)
    out = {}
    for name in SPECS:
        g = {k: z["%s/%s" % (name, k)] for k in GRAPH_KEYS if "%s/%s" % (name, k) in z.files}
        g.update(P=P, L=len(g["pts"]), E=len(g["cam_idx"]), nP=P - 2, nL=int(g["pt_hidx"].max()) + 1, f=F_PX, cx=CX, cy=CY)
        if SPECS[name]["stereo"]:
            g.update(observation="stereo", baseline=BASELINE)
        ref = {k: z["%s/ref_%s" % (name, k)] for k in ("trace", "pts", "chi2", "drift", "decisions", "margin", "diff", "trace1", "pts1", "pts10", "chi210",
                                                             "drift10", "trace10", "each10")}
        out[name] = (g, ref)
    return out


def append_profile(record):
    with open(PROFILE, "a") as fh:
        fh.write(json.dumps(record, sort_keys=True) + "\n")


# ------------------------------------------------------------------------------------------------ device set-up
def setup_device(g, name, fused=True, device=0):
    """A HipBlockSolver with the graph bound to the BA front end.  Returns (solver, set id)."""
    from openslam_g2o_amd import capi
    spec = SPECS[name]
    s = capi.HipBlockSolver(6, 3, device)
    s.setOption("ba_fused", 1.0 if fused else 0.0)
    k = s.addEdgeSet(3 if spec["stereo"] else 2, g["v0"], g["v1"])
    s.buildStructure(g["nP"], g["nL"], True)
    info = g.get("info")
    if spec["stereo"]:
        s.baSetStereoEdges(k, g["cam_idx"], g["pt_idx"], g["meas"], info, g["f"], g["cx"], g["cy"], g["baseline"])
    elif spec["classes"]:
        s.baSetEdgesClasses(k, g["cam_idx"], g["pt_idx"], g["meas"], g["class_params"], g["edge_class"], info)
    else:
        s.baSetEdges(k, g["cam_idx"], g["pt_idx"], g["meas"], info, g["f"], g["cx"], g["cy"])
    s.baSetEstimates(g["cams"], g["cam_hidx"], g["pts"], g["pt_hidx"])
    if spec["kernel"][0] and not spec["classes"]:
        s.setRobustKernel(k, spec["kernel"][0], spec["kernel"][1])
    return s, k
