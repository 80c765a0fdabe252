"""Test side of the laser self-calibration edges (EdgeSE2SensorCalib = type 21, g2ohip_pg_set_sensor_calib_edges): the formulas of
openslam_g2o_amd/sensor_calib.py (ONE body, operation for operation, generic over the arithmetic) evaluated in fp64 (FP64) and with
mpmath at 60 digits (MP), the graphs of the tests, the CPU oracle over the odometry set and the three-vertex edges
(add_multi_edge_set) and host-fed graphs for lm.optimize."""
import os

import numpy as np

from openslam_g2o_amd import sensor_calib as SC
from openslam_g2o_amd import synthetic as S
from openslam_g2o_amd.sensor_calib import FP64  # noqa: F401
from oracle import oracle as O
from tests.sim3_helpers import MP  # noqa: F401

EDGE_COUNTS = (1, 255, 256, 257, 700)                 # one lane per edge, 256 threads per workgroup; 700: a partial last group of 188
DRIFT_FACTOR = 8.0                                    # device-vs-restatement bound = 8 x the recorded fp64-vs-mpmath drift
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sensor_calib_edges.npz")
GRAPH_KEYS = ("poses", "hidx", "vi", "vj", "Z", "omega", "ci", "cj", "cl", "cmeas", "cinfo")
EDGE_KEYS = ("ci", "cj", "cl", "cmeas", "cinfo")
GRAPH_SEED = 18                                       # (a seed at which make_sensor_calib_edges.py's assertions hold)
N_SPECIAL = 48                                        # the golden edges proper: the special cases come first
# pose table of the base graph: 6 robot poses (pose 0 fixed; poses 2 and 3 share their angle EXACTLY), row 6 the laser offset, row 7
# a second offset with a large lever arm
POSE_ROWS, OFFSET_ROW, LEVER_ROW = 6, 6, 7
PAIRS = ((0, 1), (1, 2), (2, 3), (3, 2), (4, 1), (5, 0), (1, 4), (3, 5), (2, 4))   # (0, 1) / (5, 0): the fixed pose on either side; (2, 3): th1 == th2
# The LM comparison: 60 poses, 59 + 30 calibration edges.  The seed is chosen from CPU runs alone (the oracle's solver) as one whose
# noise realisation leaves the calibrated offset within the measurement noise of the truth: with 89 scan matches against 59
# odometry edges of the same noise the offset's own standard deviation is of the order of that noise.
LM_ARGS = dict(n_poses=60, loops=30, perturb=(0.1, 0.03), noise=(0.02, 0.01))
LM_SEED = 5
LM_ITERATIONS = 8


def base_graph(n_edges=700, seed=GRAPH_SEED):
    """The base graph of the fixture and the GPU tests: 8 rows (above), 5 odometry edges and n_edges calibration edges that cycle
    over PAIRS.  Edge k uses the lever-arm offset (row 7) where k % 5 == 4, the ordinary one otherwise.  Three of four measurements
    are near the prediction; every fourth is an arbitrary relative pose, so that the angles reach every branch of the wrap.  Edges
    0 .. 7: the prediction turned by pi -/+ 5e-4 (four each), so that the angle error lies within 1e-3 of +pi and of -pi."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((8, 3))
    poses[:6] = rng.normal(size=(6, 3)) * np.array([3.0, 3.0, 0.0]) + np.array([0, 0, 1.0]) * rng.uniform(-np.pi, np.pi, size=(6, 1))
    poses[3, 2] = poses[2, 2]
    poses[OFFSET_ROW] = [0.3, 0.1, 0.2]
    poses[LEVER_ROW] = [-40.0, 25.0, -2.4]
    k = np.arange(n_edges)
    ci = np.array([PAIRS[a % len(PAIRS)][0] for a in k], np.int32)
    cj = np.array([PAIRS[a % len(PAIRS)][1] for a in k], np.int32)
    cl = np.where(k % 5 == 4, LEVER_ROW, OFFSET_ROW).astype(np.int32)
    cmeas = rng.normal(size=(n_edges, 3)) * np.array([2.0, 2.0, 0.0]) + np.array([0, 0, 1.0]) * rng.uniform(-np.pi, np.pi, size=(n_edges, 1))
    small = rng.normal(size=(n_edges, 3)) * 0.05
    for e in range(n_edges):
        if e % 4 != 3:
            pred = SC.predict(poses[ci[e]], poses[cj[e]], poses[cl[e]])
            cmeas[e] = SC.se2_mul(FP64, list(pred), list(small[e]))
        if e < 8:
            pred = SC.predict(poses[ci[e]], poses[cj[e]], poses[cl[e]])
            cmeas[e] = [pred[0], pred[1], SC.normalize_theta(FP64, pred[2] + np.pi + (-5e-4 if e % 2 == 0 else 5e-4))]
    vi, vj = np.arange(5, dtype=np.int32), np.arange(1, 6, dtype=np.int32)
    Z = np.stack([SC.predict(poses[a], poses[b], np.zeros(3)) for a, b in zip(vi, vj)])
    A = rng.normal(size=(3, 3)) * 0.2
    info = np.eye(3) * 4.0 + A @ A.T                                      # one full symmetric positive definite matrix
    return dict(kind="se2", n=8, nP=7, poses=poses, hidx=np.array([-1, 0, 1, 2, 3, 4, 5, 6], np.int32), vi=vi, vj=vj, Z=Z,
                omega=np.tile(np.eye(3).reshape(1, -1), (5, 1)), ci=ci, cj=cj, cl=cl, cmeas=cmeas, cinfo=np.tile(info.reshape(1, -1), (n_edges, 1)))


def take_edges(g, idx):
    """g with the calibration edges idx only (a slice or an index array)."""
    out = dict(g)
    for k in EDGE_KEYS:
        out[k] = np.ascontiguousarray(np.asarray(g[k])[idx])
    return out


def load_graph(z, n=700):
    """The fixture's graph with its first n calibration edges."""
    g = {k: z[k] for k in GRAPH_KEYS}
    g.update(kind="se2", n=len(g["hidx"]), nP=int((g["hidx"] >= 0).sum()))
    return take_edges(g, slice(0, n))


def producers(F, g, poses=None, jac=True, fixed_zero=True):
    """(Ji, Jj, Jl, err) of the calibration edges, or err; the blocks of fixed vertices zero, as the device writes them."""
    return SC.calib_edges(F, g["poses"] if poses is None else poses, g["ci"], g["cj"], g["cl"], g["cmeas"], jac,
                          g["hidx"] if fixed_zero else None)


def pose_edges(g, poses=None, jac=True):
    """The odometry set from the oracle's EdgeSE2."""
    poses = g["poses"] if poses is None else poses
    return O.se2_edges(poses, g["vi"], g["vj"], g["Z"], jac=jac)


def oplus(g, poses, x):
    return O.se2_oplus(poses, g["hidx"], x)


def update_step(g, seed):
    """A step over the free vertices that moves every estimate visibly."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(g["nP"], 3)) * np.array([0.1, 0.1, 0.05])).ravel()


def oracle_calib(g):
    """OracleSolver(schur=False) with set 0 = odometry and ONE multi-edge set of three-vertex edges, structure built.  Returns
    (oracle, multi-set id)."""
    h = np.asarray(g["hidx"], np.int32)
    o = O.OracleSolver(3, 2, g["nP"], 0, False)
    k0 = o.add_edge_set(3, h[g["vi"]], h[g["vj"]])
    o.set_dims(k0, 3, 3)
    m = o.add_multi_edge_set(3, np.stack([h[g["ci"]], h[g["cj"]], h[g["cl"]]], axis=1))
    o.build_structure()
    return o, m


def feed_oracle(g, o, m, huber=0.0, poses=None, jac=True, J=None):
    if jac:
        A0, A1, e0 = pose_edges(g, poses)
        Ji, Jj, Jl, err = producers(FP64, g, poses)
    else:
        (A0, A1), (Ji, Jj, Jl) = J
        e0, err = pose_edges(g, poses, jac=False), producers(FP64, g, poses, jac=False)
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    o.set_multi_edge_data(m, [Ji, Jj, Jl], g["cinfo"], err, huber, 1)
    return (A0, A1), (Ji, Jj, Jl), err


class HostCalibGraph:
    """The graph protocol of openslam_g2o_amd.lm with the poses on the host, the odometry from the oracle's EdgeSE2 and the
    calibration edges from sensor_calib.py in fp64, over the CPU oracle."""

    def __init__(self, g, o, m, huber=0.0):
        self.g, self.o, self.m, self.huber = g, o, m, huber
        self.poses = np.array(g["poses"], np.float64).copy()
        self.stack, self.J = [], None

    def linearize(self):
        A, J, _ = feed_oracle(self.g, self.o, self.m, self.huber, self.poses)
        self.J = (A, J)

    def compute_active_errors(self):
        feed_oracle(self.g, self.o, self.m, self.huber, self.poses, jac=False, J=self.J)

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


def oracle_lm_run(g, iterations=LM_ITERATIONS, dense=False, lambda_init=0.0):
    """lm.optimize over the CPU oracle fed by the fp64 producers; dense: the same loop solving the full system with numpy's
    Cholesky.  Returns dict(done, chis, trials, poses)."""
    from openslam_g2o_amd import lm
    from tests.landmark_helpers import OracleLandmarkSolver
    o, m = oracle_calib(g)
    graph = HostCalibGraph(g, o, m)
    done, chis, lams, trials = lm.optimize(graph, OracleLandmarkSolver(o, dense), iterations, "lm", user_lambda_init=lambda_init)
    return dict(done=done, chis=np.array(chis), trials=[int(t) for t in trials], poses=graph.poses.copy())


def offset_error(g, poses):
    """(|t - t_true|, |theta - theta_true|) of the laser offset row."""
    a, b = np.asarray(poses, np.float64).reshape(-1, 3)[g["offset_row"]], np.asarray(g["offset_true"], np.float64)
    return float(np.hypot(a[0] - b[0], a[1] - b[1])), float(abs((a[2] - b[2] + np.pi) % (2 * np.pi) - np.pi))


def calib_dict(g):
    return dict(vi=g["ci"], vj=g["cj"], vl=g["cl"], meas=g["cmeas"], info=g["cinfo"])


def device_setup(g, huber=0.0, options=None, **more):
    """lm.setup_device_pose_graph for a problem dict with calibration edges; returns (solver, graph)."""
    from openslam_g2o_amd import lm
    return lm.setup_device_pose_graph(1, g["poses"], g["hidx"], g["nP"], g["vi"], g["vj"], g["Z"], g["omega"], options=options,
                                      calib_edges=calib_dict(g), huber_delta=huber, **more)
