"""Test side of the odometry self-calibration edges (EdgeSE2OdomDifferentialCalib = type 22, g2ohip_pg_set_odom_calib_edges): the
formulas of openslam_g2o_amd/odom_calib.py (ONE body, operation for operation, generic over the arithmetic) evaluated in fp64 (FP64)
and with mpmath at 60 digits (MP), the graphs of the tests, the CPU oracle over the three-vertex edges (add_multi_edge_set, one
multi-edge set per calibration group) and host-fed graphs for lm.optimize."""
import os

import numpy as np

from openslam_g2o_amd import odom_calib as OC
from openslam_g2o_amd import sensor_calib as SC
from openslam_g2o_amd import synthetic as S
from openslam_g2o_amd.odom_calib import FP64  # noqa: F401
from oracle import oracle as O
from tests.calib_helpers import DRIFT_FACTOR  # noqa: F401  (the project's rule: device-vs-restatement bound = 8 x the recorded drift)
from tests.sim3_helpers import MP  # noqa: F401

EDGE_COUNTS = (1, 63, 64, 65, 257, 700)               # one lane per edge: either side of a wave, past a workgroup of 256, the whole fixture
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "odom_calib_edges.npz")
GRAPH_KEYS = ("poses", "hidx", "oi", "oj", "op", "omeas", "oinfo")
EDGE_KEYS = ("oi", "oj", "op", "omeas", "oinfo")
GRAPH_SEED = 22
N_SPECIAL = 40                                        # the edges of the central-difference comparisons: every kind among them
# table of the base graph: 6 robot poses (pose 0 fixed), rows 6 and 7 two parameter vertices away from (1, 1, 1), k_l != k_r
POSE_ROWS, PARAM_ROW, PARAM_ROW_2 = 6, 6, 7
PARAMS = ((1.07, 0.94, 1.3), (0.91, 1.12, 0.8))
PAIRS = ((1, 2), (0, 1), (2, 3), (3, 2), (4, 1), (5, 0), (1, 4), (3, 5), (2, 4))   # (0, 1) / (5, 0): the fixed pose on either side; edge 0 has none
LM_ARGS = dict(n_poses=60, loops=30, perturb=(0.1, 0.03), noise=(0.02, 0.01), odom_calib=True)
LM_SEED = 5
LM_ITERATIONS = 10
# The run starts from a damping of 1e5 (chosen on the CPU oracle alone): from g2o's own initial damping it converges in six
# iterations, and from there on rounding noise decides every accept / reject, so two equally valid runs differ in their trial
# counts.  From 1e5 all ten iterations descend by at least 1e-3 of chi2 (CPU oracle run: 11194 ... 240.32, one trial each).
LM_LAMBDA_INIT = 1e5


def base_graph(n_edges=700, seed=GRAPH_SEED):
    """The base graph of the fixture and the GPU tests: 8 rows (above), no EdgeSE2, n_edges odometry-calibration edges that cycle
    over PAIRS; edge k names the second parameter vertex where k % 7 == 6.  Measurements are built in the CALIBRATED space
    (vl', vr') and divided by the gains of the edge's parameter estimate, so that D = vr k_r - vl k_l at the fixture's estimates
    is what the construction says up to rounding:
      k % 5 == 2 (a fifth)   STRAIGHT: vl' = vr', so |D| is a rounding error (< 1e-8);
      k % 10 == 9            a gross outlier: an arbitrary turn and distance;
      k < 8                  the turn th2 - th1 + pi -/+ 5e-4: the angle error within 1e-3 of -pi / +pi (four each);
      otherwise              the turn and distance of x1^-1 x2 plus a small perturbation.
    Every turning edge has |D| >= 1e-2 (a smaller one is pushed out to +-1e-2)."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((8, 3))
    poses[:6] = rng.normal(size=(6, 3)) * np.array([3.0, 3.0, 0.0]) + np.array([0, 0, 1.0]) * rng.uniform(-np.pi, np.pi, size=(6, 1))
    poses[PARAM_ROW], poses[PARAM_ROW_2] = PARAMS
    k = np.arange(n_edges)
    oi = np.array([PAIRS[a % len(PAIRS)][0] for a in k], np.int32)
    oj = np.array([PAIRS[a % len(PAIRS)][1] for a in k], np.int32)
    op = np.where(k % 7 == 6, PARAM_ROW_2, PARAM_ROW).astype(np.int32)
    dt = rng.uniform(0.5, 1.5, size=n_edges)
    small = rng.normal(size=(n_edges, 2)) * 0.05
    wild = np.stack([rng.uniform(-3.0, 3.0, size=n_edges), rng.uniform(0.2, 4.0, size=n_edges)], axis=1)
    omeas = np.zeros((n_edges, 3))
    for e in range(n_edges):
        x1, x2, (kl, kr, b) = poses[oi[e]], poses[oj[e]], poses[op[e]]
        rel = SC.predict(x1, x2, np.zeros(3))
        dist, turn = float(np.hypot(rel[0], rel[1])), float(rel[2])
        if e < 8:
            turn = float(x2[2] - x1[2]) + np.pi + (-5e-4 if e % 2 == 0 else 5e-4)
        elif e % 5 == 2:
            turn, dist = 0.0, min(dist, 2.0)   # (|v| < 10: 1e-8 |v| stays below the branch point's 1e-7)
        elif e % 10 == 9:
            turn, dist = wild[e]
        else:
            turn, dist = turn + small[e, 0], dist * (1.0 + small[e, 1])
        S_, D_ = 2.0 * dist / dt[e], b * turn / dt[e]
        if turn != 0.0 and abs(D_) < 1e-2:
            D_ = 1e-2 if D_ >= 0 else -1e-2
        omeas[e] = [0.5 * (S_ - D_) / kl, 0.5 * (S_ + D_) / kr, dt[e]]
    A = rng.normal(size=(3, 3)) * 0.2
    info = np.eye(3) * 4.0 + A @ A.T                                      # one full symmetric positive definite matrix
    z3 = np.zeros((0, 3))
    return dict(kind="se2", n=8, nP=7, poses=poses, hidx=np.array([-1, 0, 1, 2, 3, 4, 5, 6], np.int32), vi=np.zeros(0, np.int32),
                vj=np.zeros(0, np.int32), Z=z3, omega=np.zeros((0, 9)), oi=oi, oj=oj, op=op, omeas=omeas,
                oinfo=np.tile(info.reshape(1, -1), (n_edges, 1)), param_rows=np.array([PARAM_ROW, PARAM_ROW_2], np.int32))


def take_edges(g, idx):
    """g with the odometry-calibration edges idx only (a slice or an index array)."""
    out = dict(g)
    for k in EDGE_KEYS:
        out[k] = np.ascontiguousarray(np.asarray(g[k])[idx])
    return out


def load_graph(z, n=700):
    """The fixture's graph with its first n edges."""
    g = {k: z[k] for k in GRAPH_KEYS}
    g.update(kind="se2", n=len(g["hidx"]), nP=int((g["hidx"] >= 0).sum()), vi=np.zeros(0, np.int32), vj=np.zeros(0, np.int32),
             Z=np.zeros((0, 3)), omega=np.zeros((0, 9)), param_rows=np.array([PARAM_ROW, PARAM_ROW_2], np.int32))
    return take_edges(g, slice(0, n))


def producers(F, g, poses=None, jac=True, fixed_zero=True):
    """(Ji, Jj, Jp, err) of the odometry-calibration edges, or err; the blocks of fixed vertices zero, as the device writes them."""
    return OC.odom_calib_edges(F, g["poses"] if poses is None else poses, g["oi"], g["oj"], g["op"], g["omeas"], jac,
                               g["hidx"] if fixed_zero else None)


def calib_producers(g, poses=None, jac=True):
    return SC.calib_edges(FP64, g["poses"] if poses is None else poses, g["ci"], g["cj"], g["cl"], g["cmeas"], jac, g["hidx"])


def pose_edges(g, poses=None, jac=True):
    poses = g["poses"] if poses is None else poses
    if len(g["vi"]) == 0:
        z = np.zeros((0, 9))
        return (z, z, np.zeros((0, 3))) if jac else np.zeros((0, 3))
    return O.se2_edges(poses, g["vi"], g["vj"], g["Z"], jac=jac)


def oplus(g, poses, x):
    """One step over the table: VertexSE2's oplus, plain addition on the parameter rows."""
    return OC.oplus(poses, g["hidx"], x, g["param_rows"])


def update_step(g, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(g["nP"], 3)) * np.array([0.1, 0.1, 0.05])).ravel()


def oracle_graph(g):
    """OracleSolver(schur=False): set 0 = the EdgeSE2 set (possibly empty), one multi-edge set for the odometry-calibration edges
    and, where the graph has them (ci ...), one for the type-21 edges.  Returns (oracle, odometry-calibration id, type-21 id or
    None)."""
    h = np.asarray(g["hidx"], np.int32)
    o = O.OracleSolver(3, 2, g["nP"], 0, False)
    k0 = o.add_edge_set(3, h[g["vi"]], h[g["vj"]])
    o.set_dims(k0, 3, 3)
    m = o.add_multi_edge_set(3, np.stack([h[g["oi"]], h[g["oj"]], h[g["op"]]], axis=1))
    mc = o.add_multi_edge_set(3, np.stack([h[g["ci"]], h[g["cj"]], h[g["cl"]]], axis=1)) if "ci" in g else None
    o.build_structure()
    return o, m, mc


def feed_oracle(g, o, m, mc, huber=0.0, poses=None, jac=True, J=None):
    if jac:
        A0, A1, e0 = pose_edges(g, poses)
        Jo = producers(FP64, g, poses)
        Jc = calib_producers(g, poses) if mc is not None else None
    else:
        (A0, A1), Jo3, Jc3 = J
        e0 = pose_edges(g, poses, jac=False)
        Jo = tuple(Jo3) + (producers(FP64, g, poses, jac=False),)
        Jc = (tuple(Jc3) + (calib_producers(g, poses, jac=False),)) if mc is not None else None
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    o.set_multi_edge_data(m, list(Jo[:3]), g["oinfo"], Jo[3], huber, 1)
    if mc is not None:
        o.set_multi_edge_data(mc, list(Jc[:3]), g["cinfo"], Jc[3], huber, 1)
    return (A0, A1), Jo, Jc


class HostOdomCalibGraph:
    """The graph protocol of openslam_g2o_amd.lm with the table on the host and everything from the fp64 restatements, over the CPU
    oracle."""

    def __init__(self, g, o, m, mc, huber=0.0):
        self.g, self.o, self.m, self.mc, self.huber = g, o, m, mc, huber
        self.poses = np.array(g["poses"], np.float64).copy()
        self.stack, self.J = [], None

    def linearize(self):
        A, Jo, Jc = feed_oracle(self.g, self.o, self.m, self.mc, self.huber, self.poses)
        self.J = (A, Jo[:3], None if Jc is None else Jc[:3])

    def compute_active_errors(self):
        feed_oracle(self.g, self.o, self.m, self.mc, self.huber, self.poses, jac=False, J=self.J)

    def chi2(self):
        return self.o.chi2()

    def update(self):
        self.poses = oplus(self.g, self.poses, self.o.x())

    def push(self):
        self.stack.append(self.poses.copy())

    def pop(self):
        self.poses = self.stack.pop()

    def discard_top(self):
        self.stack.pop()


def lm_graph():
    return S.make_calib_rig(seed=LM_SEED, **LM_ARGS)


def oracle_lm_run(g, iterations=LM_ITERATIONS):
    """lm.optimize over the CPU oracle fed by the fp64 producers.  Returns dict(done, chis, trials, poses)."""
    from openslam_g2o_amd import lm
    from tests.landmark_helpers import OracleLandmarkSolver
    o, m, mc = oracle_graph(g)
    graph = HostOdomCalibGraph(g, o, m, mc)
    done, chis, lams, trials = lm.optimize(graph, OracleLandmarkSolver(o, False), iterations, "lm", user_lambda_init=LM_LAMBDA_INIT)
    return dict(done=done, chis=np.array(chis), trials=[int(t) for t in trials], poses=graph.poses.copy())


def odom_dict(g):
    return dict(vi=g["oi"], vj=g["oj"], vp=g["op"], meas=g["omeas"], info=g["oinfo"])


def calib_dict(g):
    return dict(vi=g["ci"], vj=g["cj"], vl=g["cl"], meas=g["cmeas"], info=g["cinfo"]) if "ci" in g else None


def without_odometry(g):
    """g without its EdgeSE2 edges: the graph of the reference's example."""
    return dict(g, vi=np.zeros(0, np.int32), vj=np.zeros(0, np.int32), Z=np.zeros((0, 3)), omega=np.zeros((0, 9)))


def device_setup(g, huber=0.0, options=None):
    """lm.setup_device_odom_calib_graph for a problem dict; returns (solver, graph)."""
    from openslam_g2o_amd import lm
    return lm.setup_device_odom_calib_graph(g["poses"], g["hidx"], g["nP"], odom_dict(g), g["vi"], g["vj"], g["Z"], g["omega"],
                                            calib_edges=calib_dict(g), huber_delta=huber, options=options)
