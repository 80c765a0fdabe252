"""Test side of the bearing-only observations (EdgeSE2PointXYBearing = type 20, g2ohip_pg_set_bearing_edges): the formulas of
openslam_g2o_amd/bearing.py (ONE body, operation for operation, generic over the arithmetic) evaluated in fp64 (FP64) and with
mpmath at 60 digits (MP), the graphs of the tests, the CPU oracle over the odometry, Cartesian and bearing sets and a host-fed
graph for lm.optimize."""
import os

import numpy as np

from openslam_g2o_amd import bearing as BE
from openslam_g2o_amd import offset_edges as OE
from openslam_g2o_amd import synthetic as S
from openslam_g2o_amd.bearing import FP64  # noqa: F401
from oracle import oracle as O
from tests import landmark_helpers as LH
from tests.sim3_helpers import MP  # noqa: F401

EDGE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 300)     # one lane per edge, 64 lanes per wave, 256 threads per block
DRIFT_FACTOR = 8.0                                    # device-vs-restatement bound = 8 x the recorded fp64-vs-mpmath drift
GRAPH_SEED = 13                                       # (a seed at which make_bearing_edges.py's assertions hold)
MIN_DISTANCE = 0.5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bearing_edges.npz")
GRAPH_KEYS = ("poses", "hidx", "points", "pt_hidx", "vi", "vj", "Z", "omega", "vp", "vl", "zl", "omega_l", "bp", "bl", "zb", "omega_b")
EDGE_KEYS = ("bp", "bl", "zb", "omega_b")
MODES = ("bearing-only", "with type-3 set")
# The LM comparison: seed, perturbation and user_lambda_init chosen from CPU runs alone (the oracle's solver and a dense solve) so
# that both take the same trials, reject at least one step and are still descending at the fifth iteration (bearing-only: trials
# 1, 8, 1, 3, 1; beside the Cartesian observations Gauss-Newton steps are rejected only from a start as far off as this one: 1,
# 8, 1, 1, 1).
LM_POSES, LM_LANDMARKS = 12, 10
LM_ARGS = {"bearing-only": dict(seed=5, perturb=(0.6, 0.25, 1.0)), "with type-3 set": dict(seed=1, perturb=(6.0, 2.0, 6.0))}
LM_LAMBDA = {"bearing-only": 1e-6, "with type-3 set": 1e-6}
LM_ITERATIONS = 5


def base_graph(n_edges=300, seed=None):
    """The base graph of the fixture and the GPU tests: 4 poses (pose 0 fixed) whose angles lie in the four quadrants, 3 odometry
    edges, 6 landmarks on a ring round them (landmark 5 fixed), 24 EdgeSE2PointXY observations (every pair once; the type-3 set of
    the mixed tests) and n_edges bearing edges that cycle over the 24 pose / landmark pairs.  Every observation distance is at
    least 0.5.  The even bearings are measured within 0.05 rad of the prediction, the odd ones are uniform in [-pi, pi), so that
    z - angle leaves [-pi, pi) on both sides."""
    rng = np.random.default_rng(GRAPH_SEED if seed is None else seed)
    poses = np.concatenate([rng.uniform(-1.0, 1.0, size=(4, 2)),
                            (np.array([0.6, 2.3, -2.5, -0.8]) + rng.uniform(-0.3, 0.3, size=4))[:, None]], axis=1)
    ring = 2.0 * np.pi * (np.arange(6) + rng.uniform(-0.3, 0.3, size=6)) / 6.0
    points = np.stack([np.cos(ring), np.sin(ring)], axis=1) * rng.uniform(3.0, 5.0, size=(6, 1))
    k = np.arange(n_edges)
    bp, bl = (k % 4).astype(np.int32), ((k // 4) % 6).astype(np.int32)
    d = points[bl] - poses[bp, :2]
    pred = np.arctan2(d[:, 1], d[:, 0]) - poses[bp, 2]
    pred = (pred + np.pi) % (2.0 * np.pi) - np.pi
    zb = np.where(k % 2 == 0, pred + rng.uniform(-0.05, 0.05, size=n_edges), rng.uniform(-np.pi, np.pi, size=n_edges))
    vi, vj = np.arange(3, dtype=np.int32), np.arange(1, 4, dtype=np.int32)
    Z = np.stack([OE.se2_compose(OE.se2_invert(poses[a]), poses[b]) for a, b in zip(vi, vj)]) + rng.normal(size=(3, 3)) * 0.02
    vp, vl = (np.arange(24) % 4).astype(np.int32), (np.arange(24) // 4).astype(np.int32)
    zl = LH.se2_pointxy_edges(poses, points, vp, vl, np.zeros((24, 2)), jac=False) + rng.normal(size=(24, 2)) * 0.05
    A = rng.normal(size=(2, 2)) * 0.2
    return dict(kind="se2", n=4, nP=3, L=6, nL=5, poses=poses, hidx=np.array([-1, 0, 1, 2], np.int32), points=points,
                pt_hidx=np.array([3, 4, 5, 6, 7, -1], np.int32), vi=vi, vj=vj, Z=Z, omega=np.tile(np.eye(3).reshape(1, -1), (3, 1)),
                vp=vp, vl=vl, zl=zl, omega_l=np.tile((np.eye(2) * 4.0 + A @ A.T).reshape(1, -1), (24, 1)), bp=bp, bl=bl, zb=zb,
                omega_b=4.0 + 0.5 * (k % 3))


def take_edges(g, idx):
    """g with the bearing edges idx only (a slice or an index array)."""
    out = dict(g)
    for k in EDGE_KEYS:
        out[k] = np.ascontiguousarray(np.asarray(g[k])[idx])
    return out


def load_graph(z, n=300, mode="with type-3 set"):
    """The fixture's graph with its first n bearing edges; mode "bearing-only": without the EdgeSE2PointXY observations."""
    g = {k: z["graph_" + k] for k in GRAPH_KEYS}
    g.update(kind="se2", n=len(g["hidx"]), nP=int((g["hidx"] >= 0).sum()), L=len(g["pt_hidx"]), nL=int((g["pt_hidx"] >= 0).sum()))
    return with_mode(take_edges(g, slice(0, n)), mode)


def with_mode(g, mode):
    if mode == "bearing-only":
        return dict(g, vp=np.zeros(0, np.int32), vl=np.zeros(0, np.int32), zl=np.zeros((0, 2)), omega_l=np.zeros((0, 4)))
    return g


def producers(F, g, poses=None, points=None, jac=True):
    """(J0, J1, err) of the bearing set, or err."""
    return BE.bearing_edges(F, g["poses"] if poses is None else poses, g["points"] if points is None else points, g["bp"], g["bl"],
                            g["zb"], jac)


def xy_edges(g, poses=None, points=None, jac=True):
    if len(g["vp"]) == 0:
        return (np.zeros((0, 6)), np.zeros((0, 4)), np.zeros((0, 2))) if jac else np.zeros((0, 2))
    return LH.se2_pointxy_edges(g["poses"] if poses is None else poses, g["points"] if points is None else points, g["vp"], g["vl"],
                                g["zl"], jac=jac)


def pose_edges(g, poses=None, jac=True):
    return O.se2_edges(g["poses"] if poses is None else poses, g["vi"], g["vj"], g["Z"], jac=jac)


def oplus(g, poses, points, x):
    """(poses, points) moved by the step x over the free poses and the free landmarks."""
    return O.se2_oplus(poses, g["hidx"], x), LH.points_oplus(points, g["pt_hidx"], x, 3 * g["nP"], g["nP"])


def update_step(g, seed):
    """A step over the free poses and landmarks that moves every estimate visibly."""
    rng = np.random.default_rng(seed)
    return np.concatenate([(rng.normal(size=(g["nP"], 3)) * np.array([0.1, 0.1, 0.05])).ravel(), rng.normal(size=2 * g["nL"]) * 0.1])


def oracle_bearing(g, schur=True):
    """OracleSolver with sets 0 = odometry, then the EdgeSE2PointXY set if the graph has one, then the bearing set; structure
    built.  Returns (oracle, id of the Cartesian set or None, id of the bearing set)."""
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    o = O.OracleSolver(3, 2, g["nP"], g["nL"], schur)
    o.set_dims(o.add_edge_set(3, h[g["vi"]], h[g["vj"]]), 3, 3)
    kx = None
    if len(g["vp"]):
        kx = o.add_edge_set(2, h[g["vp"]], hl[g["vl"]])
        o.set_dims(kx, 3, 2)
    kb = o.add_edge_set(1, h[g["bp"]], hl[g["bl"]])
    o.set_dims(kb, 3, 2)
    o.build_structure()
    return o, kx, kb


def feed_oracle(g, o, kx, kb, huber=0.0, poses=None, points=None):
    A0, A1, e0 = pose_edges(g, poses)
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    if kx is not None:
        B0, B1, e1 = xy_edges(g, poses, points)
        o.set_edge_data(kx, B0, B1, g["omega_l"], e1, huber)
    J0, J1, err = producers(FP64, g, poses, points)
    o.set_edge_data(kb, J0, J1, g["omega_b"], err, huber)
    return J0, J1, err


class HostBearingGraph:
    """The graph protocol of openslam_g2o_amd.lm with the estimates on the host, the odometry from the oracle's EdgeSE2, the
    Cartesian set from landmark_helpers and the bearing set from bearing.py in fp64.  feed(set, J0, J1, omega, err)."""

    def __init__(self, g, feed, get_x, chi2_fn, kx, kb):
        self.g, self.feed, self.get_x, self.chi2_fn, self.kx, self.kb = g, feed, get_x, chi2_fn, kx, kb
        self.poses, self.points = np.array(g["poses"], np.float64), np.array(g["points"], np.float64)
        self.stack = []
        self.J = None

    def _feed(self, jac):
        g = self.g
        if jac:
            A0, A1, e0 = pose_edges(g, self.poses)
            B0, B1, e1 = xy_edges(g, self.poses, self.points)
            J0, J1, err = producers(FP64, g, self.poses, self.points)
            self.J = (A0, A1, B0, B1, J0, J1)
        else:
            A0, A1, B0, B1, J0, J1 = self.J
            e0, e1 = pose_edges(g, self.poses, jac=False), xy_edges(g, self.poses, self.points, jac=False)
            err = producers(FP64, g, self.poses, self.points, jac=False)
        self.feed(0, A0, A1, g["omega"], e0)
        if self.kx is not None:
            self.feed(self.kx, B0, B1, g["omega_l"], e1)
        self.feed(self.kb, J0, J1, g["omega_b"], err)

    def linearize(self):
        self._feed(True)

    def compute_active_errors(self):
        self._feed(False)

    def chi2(self):
        return self.chi2_fn()

    def update(self):
        self.poses, self.points = oplus(self.g, self.poses, self.points, self.get_x())

    def push(self):
        self.stack.append((self.poses.copy(), self.points.copy()))

    def pop(self):
        self.poses, self.points = self.stack.pop()

    def discard_top(self):
        self.stack.pop()


def lm_graph(mode):
    return S.make_bearing_slam(LM_POSES, LM_LANDMARKS, with_xy=(mode != "bearing-only"), **LM_ARGS[mode])


def oracle_lm_run(g, iterations=LM_ITERATIONS, dense=False, lambda_init=0.0):
    """lm.optimize over the CPU oracle fed by the fp64 producers; dense: the same loop solving the full system with numpy's
    Cholesky.  Returns dict(done, chis, trials, poses, points)."""
    from openslam_g2o_amd import lm
    o, kx, kb = oracle_bearing(g, True)
    graph = HostBearingGraph(g, lambda k, J0, J1, om, err: o.set_edge_data(k, J0, J1, om, err), o.x, o.chi2, kx, kb)
    done, chis, lams, trials = lm.optimize(graph, LH.OracleLandmarkSolver(o, dense), iterations, "lm", user_lambda_init=lambda_init)
    return dict(done=done, chis=np.array(chis), trials=[int(t) for t in trials], poses=graph.poses.copy(), points=graph.points.copy())


def pose_error(g, poses):
    """max abs distance of the pose estimates from the truth, entry by entry (pose 0 is fixed at the truth: no gauge freedom)."""
    a, b = np.asarray(poses, np.float64).reshape(-1, 3), np.asarray(g["poses_true"], np.float64).reshape(-1, 3)
    diff = np.abs(a - b)
    diff[:, 2] = np.abs((a[:, 2] - b[:, 2] + np.pi) % (2 * np.pi) - np.pi)
    return float(diff.max())


def device_setup(g, huber=0.0, schur=True, options=None):
    """lm.setup_device_landmark_slam for a problem dict with a bearing set; returns (solver, graph)."""
    from openslam_g2o_amd import lm
    return lm.setup_device_landmark_slam(g, huber_delta=huber, schur=schur, options=options)
