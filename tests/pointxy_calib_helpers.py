"""Test side of the landmark self-calibration edges (EdgeSE2PointXYCalib = type 24, g2ohip_pg_set_pointxy_calib_edges): the formulas
of openslam_g2o_amd/pointxy_calib.py (ONE body, operation for operation, generic over the arithmetic) evaluated in fp64 (FP64) and
with mpmath at 60 digits (MP), the graphs of the tests, the CPU oracle over the odometry set and the three-vertex edges
(add_multi_edge_set), a NumPy assembly of binary sets with parts, and host-fed graphs for lm.optimize."""
import os

import numpy as np

from openslam_g2o_amd import pointxy_calib as PC
from openslam_g2o_amd import sensor_calib as SC
from openslam_g2o_amd import synthetic as S
from openslam_g2o_amd.pointxy_calib import FP64  # noqa: F401
from oracle import oracle as O
from tests.sim3_helpers import MP  # noqa: F401

EDGE_COUNTS = (1, 255, 256, 257, 700)                 # one lane per edge, 256 threads per workgroup; 700: a partial last group of 188
DRIFT_FACTOR = 8.0                                    # device-vs-restatement bound = 8 x the recorded fp64-vs-mpmath drift
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointxy_calib_edges.npz")
GRAPH_KEYS = ("poses", "points", "hidx", "pt_hidx", "vi", "vj", "Z", "omega", "qp", "ql", "qc", "zq", "omega_q")
EDGE_KEYS = ("qp", "ql", "qc", "zq", "omega_q")
GRAPH_SEED = 11                                       # (a seed at which make_pointxy_calib_edges.py's assertions hold)
N_SPECIAL = 48                                        # the golden edges proper
# pose table of the base graph: 6 robot poses (pose 0 fixed), row 6 the calibration vertex, row 7 a second one with a large lever
# arm (|tc| = 40), row 8 a third with thc == 0 EXACTLY; 12 landmarks, landmark 0 fixed
POSE_ROWS, CALIB_ROW, LEVER_ROW, ZERO_ROW, N_POINTS = 6, 6, 7, 8, 12
# The LM comparison: about 40 poses and 30 landmarks, the offset starts at the identity.  with_xy: a second, centred point sensor
# beside the calibrated one.  Chosen from CPU runs alone (the oracle's solver): on laps of nearly constant curvature the odometry
# barely changes when every pose is moved by one body-frame transform, so without the second sensor the offset comes out only to
# about the measurement noise (0.05 .. 0.08 over seeds 1, 2, 3, 5, 7 against noise 0.05); with it, to 6e-4 at this seed.  Four
# iterations: every one still descends by far more than rounding and takes one trial (from the eighth on the accept / reject
# decisions of the CPU runs hang on the last bits).
LM_ARGS = dict(n_poses=40, n_landmarks=30, noise=0.05, perturb=(0.1, 0.02, 0.2), with_xy=True)
LM_SEED = 5
LM_ITERATIONS = 4


def base_graph(n_edges=700, seed=GRAPH_SEED):
    """The base graph of the fixture and the GPU tests: 9 pose rows (above), 12 landmarks, 5 odometry edges and n_edges three-vertex
    edges.  Edge k observes landmark (5 k + k // 6 + 1) % 12 from pose k % 6 through the lever-arm vertex where k % 5 == 4, the
    thc == 0 vertex where k % 7 == 3 and the ordinary one otherwise.  Three of four measurements are near the prediction; every
    fourth is arbitrary."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((9, 3))
    poses[:6] = rng.normal(size=(6, 3)) * np.array([3.0, 3.0, 0.0]) + np.array([0, 0, 1.0]) * rng.uniform(-np.pi, np.pi, size=(6, 1))
    poses[CALIB_ROW] = [0.3, 0.1, 0.2]
    poses[LEVER_ROW] = [-32.0, 24.0, -2.4]
    poses[ZERO_ROW] = [0.2, -0.1, 0.0]
    points = rng.normal(size=(N_POINTS, 2)) * 4.0
    k = np.arange(n_edges)
    qp = (k % 6).astype(np.int32)
    ql = ((5 * k + k // 6 + 1) % N_POINTS).astype(np.int32)              # (edge 0: the fixed pose 0 and the FREE landmark 1)
    qc = np.where(k % 5 == 4, LEVER_ROW, np.where(k % 7 == 3, ZERO_ROW, CALIB_ROW)).astype(np.int32)
    zq = rng.normal(size=(n_edges, 2)) * 3.0
    small = rng.normal(size=(n_edges, 2)) * 0.05
    for e in range(n_edges):
        if e % 4 != 3:
            zq[e] = PC.predict(poses[qp[e]], points[ql[e]], poses[qc[e]]) + small[e]
    vi, vj = np.arange(5, dtype=np.int32), np.arange(1, 6, dtype=np.int32)
    Z = np.stack([SC.predict(poses[a], poses[b], np.zeros(3)) for a, b in zip(vi, vj)])
    A = rng.normal(size=(2, 2)) * 0.2
    info = np.eye(2) * 4.0 + A @ A.T                                      # one full symmetric positive definite matrix
    hidx = np.array([-1, 0, 1, 2, 3, 4, 5, 6, 7], np.int32)
    pt_hidx = np.concatenate([[-1], 8 + np.arange(N_POINTS - 1)]).astype(np.int32)
    return finish(dict(poses=poses, points=points, hidx=hidx, pt_hidx=pt_hidx, vi=vi, vj=vj, Z=Z,
                       omega=np.tile(np.eye(3).reshape(1, -1), (5, 1)), qp=qp, ql=ql, qc=qc, zq=zq,
                       omega_q=np.tile(info.reshape(1, -1), (n_edges, 1))))


def finish(g):
    """The keys lm.setup_device_landmark_slam reads beside the arrays: no plain EdgeSE2PointXY observations."""
    g = dict(g)
    g.update(kind="se2", n=len(g["hidx"]), L=len(g["pt_hidx"]), nP=int((np.asarray(g["hidx"]) >= 0).sum()),
             nL=int((np.asarray(g["pt_hidx"]) >= 0).sum()), Q=len(g["qp"]))
    for key, shape in (("vp", (0,)), ("vl", (0,)), ("zl", (0, 2)), ("omega_l", (0, 4))):
        g.setdefault(key, np.zeros(shape, np.int32 if key in ("vp", "vl") else np.float64))
    return g


def take_edges(g, idx):
    """g with the three-vertex edges idx only (a slice or an index array)."""
    out = dict(g)
    for k in EDGE_KEYS:
        out[k] = np.ascontiguousarray(np.asarray(g[k])[idx])
    out["Q"] = len(out["qp"])
    return out


def load_graph(z, n=700):
    """The fixture's graph with its first n three-vertex edges."""
    return take_edges(finish({k: z[k] for k in GRAPH_KEYS}), slice(0, n))


def producers(F, g, poses=None, points=None, jac=True, fixed_zero=True):
    """(Jp, Jl, Jc, err) of the three-vertex edges, or err; the blocks of fixed vertices zero, as the device writes them."""
    return PC.pointxy_calib_edges(F, g["poses"] if poses is None else poses, g["points"] if points is None else points, g["qp"],
                                  g["ql"], g["qc"], g["zq"], g["hidx"] if fixed_zero else None, g["pt_hidx"] if fixed_zero else None, jac)


def pose_edges(g, poses=None, jac=True):
    """The odometry set from the oracle's EdgeSE2."""
    return O.se2_edges(g["poses"] if poses is None else poses, g["vi"], g["vj"], g["Z"], jac=jac)


def xy_edges(g, poses=None, points=None, jac=True):
    from tests.landmark_helpers import se2_pointxy_edges
    return se2_pointxy_edges(g["poses"] if poses is None else poses, g["points"] if points is None else points, g["vp"], g["vl"],
                             g["zl"], jac=jac)


def oplus(g, poses, points, x):
    from tests.landmark_helpers import points_oplus
    return O.se2_oplus(poses, g["hidx"], x), points_oplus(points, g["pt_hidx"], x, 3 * g["nP"], g["nP"])


def update_step(g, seed):
    """A step over the free poses, calibration vertices and landmarks that moves every estimate visibly."""
    rng = np.random.default_rng(seed)
    return np.concatenate([(rng.normal(size=(g["nP"], 3)) * np.array([0.1, 0.1, 0.05])).ravel(), rng.normal(size=2 * g["nL"]) * 0.1])


def multi_verts(g):
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    return np.stack([h[g["qp"]], hl[g["ql"]], h[g["qc"]]], axis=1)


def oracle_calib(g, schur=True):
    """OracleSolver with set 0 = odometry, (set 1 = the EdgeSE2PointXY observations if the graph has any) and ONE multi-edge set of
    three-vertex edges, structure built.  Returns (oracle, id of the Cartesian set or None, multi-set id)."""
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    o = O.OracleSolver(3, 2, g["nP"], g["nL"], schur)
    o.set_dims(o.add_edge_set(3, h[g["vi"]], h[g["vj"]]), 3, 3)
    kx = None
    if len(g["vp"]):
        kx = o.add_edge_set(2, h[g["vp"]], hl[g["vl"]])
        o.set_dims(kx, 3, 2)
    m = o.add_multi_edge_set(2, multi_verts(g))
    o.build_structure()
    return o, kx, m


def feed_oracle(g, o, kx, m, huber=0.0, poses=None, points=None, jac=True, J=None):
    if jac:
        A0, A1, e0 = pose_edges(g, poses)
        Jq = producers(FP64, g, poses, points)
        err, Jq = Jq[3], Jq[:3]
        B = xy_edges(g, poses, points) if kx is not None else None
    else:
        (A0, A1), Jq, B = J
        e0, err = pose_edges(g, poses, jac=False), producers(FP64, g, poses, points, jac=False)
        if kx is not None:
            B = (B[0], B[1], xy_edges(g, poses, points, jac=False))
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    if kx is not None:
        o.set_edge_data(kx, B[0], B[1], g["omega_l"], B[2], huber)
    o.set_multi_edge_data(m, list(Jq), g["omega_q"], err, huber, 1)
    return (A0, A1), Jq, B, err


def assemble_parts(n_total, sets):
    """Dense H, b and chi2 of binary edge sets with parts, as g2ohip_set_edge_set_parts states them (no robust kernel): per set
    (rows0, rows1, J0 [n][d x d0], J1 [n][d x d1], omega [n][d x d], err [n][d], parts); rows = first scalar row of the vertex in
    the system or -1 (fixed).  Bits: 1 / 2 = no diagonal block and no right-hand side for vertex 0 / vertex 1, 4 = not in chi2."""
    H, b, chi = np.zeros((n_total, n_total)), np.zeros(n_total), 0.0
    for r0, r1, J0, J1, om, err, parts in sets:
        n, d = err.shape
        d0, d1 = J0.shape[1] // d, J1.shape[1] // d
        for k in range(n):
            A, B = J0[k].reshape(d0, d).T, J1[k].reshape(d1, d).T
            W, e = om[k].reshape(d, d), err[k]
            if not parts & 4:
                chi += float(e @ W @ e)
            a, c = int(r0[k]), int(r1[k])
            if a >= 0 and not parts & 1:
                H[a:a + d0, a:a + d0] += A.T @ W @ A
                b[a:a + d0] -= A.T @ W @ e
            if c >= 0 and not parts & 2:
                H[c:c + d1, c:c + d1] += B.T @ W @ B
                b[c:c + d1] -= B.T @ W @ e
            if a >= 0 and c >= 0:
                H[a:a + d0, c:c + d1] += A.T @ W @ B
                H[c:c + d1, a:a + d0] += B.T @ W @ A
    return H, b, chi


def scalar_rows(g):
    """first scalar row in the full system of every pose row / landmark row (-1 fixed)"""
    h, hl = np.asarray(g["hidx"]), np.asarray(g["pt_hidx"])
    return np.where(h >= 0, 3 * h, -1), np.where(hl >= 0, 3 * g["nP"] + 2 * (hl - g["nP"]), -1)


class HostCalibGraph:
    """The graph protocol of openslam_g2o_amd.lm with the estimates on the host, the odometry from the oracle's EdgeSE2 and the
    three-vertex edges from pointxy_calib.py in fp64, over the CPU oracle."""

    def __init__(self, g, o, kx, m, huber=0.0):
        self.g, self.o, self.kx, self.m, self.huber = g, o, kx, m, huber
        self.poses, self.points = np.array(g["poses"], np.float64).copy(), np.array(g["points"], np.float64).copy()
        self.stack, self.J = [], None

    def linearize(self):
        A, Jq, B, _ = feed_oracle(self.g, self.o, self.kx, self.m, self.huber, self.poses, self.points)
        self.J = (A, Jq, B)

    def compute_active_errors(self):
        feed_oracle(self.g, self.o, self.kx, self.m, self.huber, self.poses, self.points, jac=False, J=self.J)

    def chi2(self):
        return self.o.chi2()

    def update(self):
        self.poses, self.points = oplus(self.g, self.poses, self.points, self.o.x())

    def push(self):
        self.stack.append((self.poses.copy(), self.points.copy()))

    def pop(self):
        self.poses, self.points = self.stack.pop()

    def discard_top(self):
        self.stack.pop()


def lm_graph():
    return S.make_pointxy_calib_slam(seed=LM_SEED, **LM_ARGS)


def oracle_lm_run(g, iterations=LM_ITERATIONS, dense=False):
    """lm.optimize over the CPU oracle fed by the fp64 producers; dense: the same loop solving the full system with numpy's
    Cholesky.  Returns dict(done, chis, trials, poses, points)."""
    from openslam_g2o_amd import lm
    from tests.landmark_helpers import OracleLandmarkSolver
    o, kx, m = oracle_calib(g)
    graph = HostCalibGraph(g, o, kx, m)
    done, chis, lams, trials = lm.optimize(graph, OracleLandmarkSolver(o, dense), iterations, "lm")
    return dict(done=done, chis=np.array(chis), trials=[int(t) for t in trials], poses=graph.poses.copy(), points=graph.points.copy())


def offset_error(g, poses):
    """(|t - t_true|, |theta - theta_true|) of the calibration row."""
    a, b = np.asarray(poses, np.float64).reshape(-1, 3)[g["calib_row"]], np.asarray(g["offset_true"], np.float64)
    return float(np.hypot(a[0] - b[0], a[1] - b[1])), float(abs((a[2] - b[2] + np.pi) % (2 * np.pi) - np.pi))


def device_setup(g, huber=0.0, schur=True, options=None):
    """lm.setup_device_landmark_slam for a problem dict with three-vertex edges; returns (solver, graph)."""
    from openslam_g2o_amd import lm
    return lm.setup_device_landmark_slam(g, huber_delta=huber, schur=schur, options=options)
