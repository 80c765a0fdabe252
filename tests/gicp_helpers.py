"""Test side of the GICP front end (Edge_V_V_GICP = type 15, g2ohip_pg_set_gicp_edges): the formulas of
openslam_g2o_amd/gicp.py (ONE body, operation for operation, generic over the arithmetic) evaluated in fp64 (FP64) and with
mpmath at 60 digits (MP), the graphs of the tests, the CPU oracle over both pose-pose sets and a host-fed graph for lm.optimize."""
import os

import numpy as np

from openslam_g2o_amd import synthetic as S
from openslam_g2o_amd.gicp import FP64, chi2, gicp_edges  # noqa: F401
from oracle import oracle as O
from tests.sim3_helpers import MP  # noqa: F401

EDGE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 300)     # one lane per edge, 64 lanes per wave, 256 threads per block
PAIRS = ((0, 1), (1, 2), (0, 2), (2, 1))              # (2, 1): the pair (1, 2) reversed, the transposed Hessian block
MODES = (("pp", False), ("pl", True))                 # point-to-plane, plane-to-plane
DRIFT_FACTOR = 8.0                                    # device-vs-restatement bound = 8 x the recorded fp64-vs-mpmath drift
# The LM comparison: seed, perturbation and user_lambda_init chosen from CPU runs alone (the oracle's solver and a dense solve)
# so that both take the same trials, reject at least one step (a pop after the information was rewritten) and are still descending
# at the tenth iteration.  With the default damping the runs converge to the last bit within seven iterations.
LM_ARGS = dict(n_scans=3, pts_per_pair=40, pairs=PAIRS, perturb=(4.0, 0.9))
LM_SEED = {"pp": 11, "pl": 20}
LM_ITERATIONS = 10
LM_LAMBDA = {"pp": 1e4, "pl": 1e5}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gicp_edges.npz")
GRAPH_KEYS = ("poses", "hidx", "vi", "vj", "Z", "omega", "gi", "gj", "gmeas", "ginfo", "gcov")


def graph_name(n, plpl):
    return "%s%d" % ("pl" if plpl else "pp", n)


def take_edges(g, idx):
    """g with the GICP edges idx only."""
    out = dict(g)
    for k in ("gi", "gj", "gmeas", "ginfo", "gcov", "normal0", "normal1"):
        out[k] = None if g[k] is None else np.ascontiguousarray(np.asarray(g[k])[idx])
    return out


def base_graph(n_edges, plpl, seed=None, **kw):
    """The base graph of the GPU tests: 3 scans, scan 0 fixed, two type-2 odometry edges, n_edges correspondences that cycle over
    the pairs (0, 1), (1, 2), (0, 2), (2, 1): edge 0 joins the fixed scan and a free one, edges 1 and 3 the same two scans in
    either order."""
    per = (n_edges + len(PAIRS) - 1) // len(PAIRS)
    g = S.make_gicp(3, per, pairs=PAIRS, plane_to_plane=plpl, seed=100 + n_edges if seed is None else seed, **kw)
    order = (np.arange(per)[:, None] + per * np.arange(len(PAIRS))[None, :]).reshape(-1)[:n_edges]
    return take_edges(g, order)


def load_graph(z, name):
    g = {k: z["%s_%s" % (name, k)] for k in GRAPH_KEYS if "%s_%s" % (name, k) in z}
    g.setdefault("gcov", None)
    g.update(kind="se3", nP=int((g["hidx"] >= 0).sum()), n=len(g["hidx"]), plane_to_plane=g["gcov"] is not None)
    return g


def producers(F, g, poses=None, jac=True):
    """(J0, J1, err, omega) of the GICP set -- omega: the set's information after the evaluation, the bound ginfo in
    point-to-plane mode -- or (err, omega)."""
    out = gicp_edges(F, g["poses"] if poses is None else poses, g["gi"], g["gj"], g["gmeas"], g.get("gcov"), jac)
    if out[-1] is None:
        out = out[:-1] + (np.asarray(g["ginfo"], np.float64).reshape(-1, 9),)
    return out


def drift(g):
    """fp64 against 60 digits: (mpmath values), max abs over err, over J0 | J1, over omega (0 in point-to-plane mode)."""
    a, b = producers(FP64, g), producers(MP, g)
    fig = dict(err=float(np.abs(a[2] - b[2]).max()), J=float(max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())),
               omega=float(np.abs(a[3] - b[3]).max()))
    return b, fig


def update_step(g, seed):
    """A step over the free poses that moves every estimate visibly (quaternion part well below 1)."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(g["nP"], 6)) * np.array([0.1] * 3 + [0.03] * 3)).ravel()


def pose_edges(g, poses=None, jac=True):
    poses = g["poses"] if poses is None else poses
    if len(g["vi"]) == 0:
        return (np.zeros((0, 36)), np.zeros((0, 36)), np.zeros((0, 6))) if jac else np.zeros((0, 6))
    return O.se3_edges(poses, g["vi"], g["vj"], g["Z"], jac=jac)


def oracle_gicp(g):
    """OracleSolver(schur=False) with sets 0 / 1 = odometry / GICP, structure built."""
    h = np.asarray(g["hidx"], np.int32)
    o = O.OracleSolver(6, 3, g["nP"], 0, False)
    k0 = o.add_edge_set(6, h[g["vi"]], h[g["vj"]])
    o.set_dims(k0, 6, 6)
    k1 = o.add_edge_set(3, h[g["gi"]], h[g["gj"]])
    o.set_dims(k1, 6, 6)
    o.build_structure()
    return o


def feed_oracle(g, o, huber=0.0, poses=None):
    A0, A1, e0 = pose_edges(g, poses)
    J0, J1, err, om = producers(FP64, g, poses)
    if len(e0):
        o.set_edge_data(0, A0, A1, g["omega"], e0)
    o.set_edge_data(1, J0, J1, om, err, huber)
    return J0, J1, err, om


class HostGicpGraph:
    """The graph protocol of openslam_g2o_amd.lm with the poses on the host, the odometry from the oracle's EdgeSE3 and the GICP
    set from gicp.py in fp64: feed(set, J0, J1, omega, err) hands every evaluation to a solver, get_x() reads its solution.
    In plane-to-plane mode every evaluation hands over a new omega, as the reference's computeError rewrites it."""

    def __init__(self, g, feed, get_x, chi2_fn):
        self.g, self.feed, self.get_x, self.chi2_fn = g, feed, get_x, chi2_fn
        self.poses = np.array(g["poses"], np.float64).copy()
        self.stack = []
        self.J = None

    def linearize(self):
        A0, A1, e0 = pose_edges(self.g, self.poses)
        J0, J1, err, om = producers(FP64, self.g, self.poses)
        self.J = (A0, A1, J0, J1)
        if len(e0):
            self.feed(0, A0, A1, self.g["omega"], e0)
        self.feed(1, J0, J1, om, err)

    def compute_active_errors(self):
        A0, A1, J0, J1 = self.J
        e0 = pose_edges(self.g, self.poses, jac=False)
        err, om = producers(FP64, self.g, self.poses, jac=False)
        if len(e0):
            self.feed(0, A0, A1, self.g["omega"], e0)
        self.feed(1, J0, J1, om, err)

    def chi2(self):
        return self.chi2_fn()

    def update(self):
        self.poses = O.se3_oplus(self.poses, self.g["hidx"], self.get_x())

    def push(self):
        self.stack.append(self.poses.copy())

    def pop(self):
        self.poses = self.stack.pop()

    def discard_top(self):
        self.stack.pop()


def lm_graph(mode):
    return S.make_gicp(plane_to_plane=dict(MODES)[mode], seed=LM_SEED[mode], **LM_ARGS)


def oracle_lm_run(g, iterations=LM_ITERATIONS, dense=False, lambda_init=0.0):
    """lm.optimize over the CPU oracle fed by the fp64 producers; dense: the same loop solving the full system with numpy's
    Cholesky.  Returns dict(chis, trials, poses)."""
    from openslam_g2o_amd import lm
    from tests.landmark_helpers import OracleLandmarkSolver
    o = oracle_gicp(g)
    graph = HostGicpGraph(g, lambda k, J0, J1, om, err: o.set_edge_data(k, J0, J1, om, err), o.x, o.chi2)
    done, chis, lams, trials = lm.optimize(graph, OracleLandmarkSolver(o, dense), iterations, "lm", user_lambda_init=lambda_init)
    return dict(done=done, chis=np.array(chis), trials=[int(t) for t in trials], poses=graph.poses.copy())


def relative_pose_error(poses, truth):
    """max abs over (R, t) of X0^-1 Xk against the same of the truth, over the scans k > 0."""
    def rel(T):
        T = np.asarray(T, np.float64).reshape(-1, 12)
        R, t = T[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1), T[:, 9:]
        return R[0].T @ R[1:], np.einsum("ij,nj->ni", R[0].T, t[1:] - t[0])
    (Ra, ta), (Rb, tb) = rel(poses), rel(truth)
    return float(max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max()))
