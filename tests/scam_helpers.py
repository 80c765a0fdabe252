"""Test side of the stereo observations of VertexSCam cameras (Edge_XYZ_VSC = type 23, g2ohip_pg_set_scam_edges): the formulas of
openslam_g2o_amd/scam.py (ONE body, operation for operation, generic over the arithmetic) evaluated in fp64 (FP64) and with mpmath
at 60 digits (MP), the graphs of the tests, the CPU oracle over the EdgeSE3, stereo, GICP and prior sets and a host graph for
lm.optimize."""
import os

import numpy as np

from openslam_g2o_amd import gicp as G
from openslam_g2o_amd import offset_edges as OE
from openslam_g2o_amd import scam as SC
from openslam_g2o_amd import synthetic as S
from openslam_g2o_amd.scam import FP64  # noqa: F401
from oracle import oracle as O
from tests import landmark_helpers as LH

EDGE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 300)     # one lane per edge, 64 lanes per wave, 256 threads per block
DRIFT_FACTOR = 8.0                                    # device-vs-restatement bound = 8 x the recorded fp64-vs-mpmath drift
GRAPH_SEED = 0                                        # (a seed at which make_scam_edges.py's assertions hold)
MIN_DEPTH = 1.0
KCAM = np.array(S.SCAM_KCAM)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scam_edges.npz")
GRAPH_KEYS = ("poses", "hidx", "points", "pt_hidx", "vi", "vj", "Z", "omega", "vp", "vl", "zl", "omega_l")
EDGE_KEYS = ("vp", "vl", "zl", "omega_l")
LM_CAMS, LM_POINTS, LM_ITERATIONS = 6, 120, 10        # the graph of the whole-run comparisons: make_scam_ba(6, 120)
JOINT_ITERATIONS = 5


def MP():
    """mpmath at 60 digits (tests/sim3_helpers.MP), imported on use."""
    from tests.sim3_helpers import MP as M
    return M


def base_graph(n_edges=300, seed=None):
    """The base graph of the fixture and the GPU tests: 4 cameras on a sphere of radius 6 round the origin, each looking at it
    with a tilt and a roll of its own (every camera looks down the world's z axis, so the rotations are more than 60 degrees from
    the identity, and far from each other; camera 0 fixed), 3 EdgeSE3 odometry
    edges, 12 points within 1.5 of the origin (point 11 fixed) and n_edges stereo observations that cycle over the 48 camera /
    point pairs, so pairs repeat with different measurements.  Every depth is about 6.  Measurements: mapPoint + N(0, 1) pixels
    (1 / 16 on the third row)."""
    rng = np.random.default_rng(GRAPH_SEED if seed is None else seed)
    dirs = np.array([[1.0, 0.2, 0.3], [-0.4, 1.0, 0.5], [-0.6, -0.8, 0.7], [0.3, -0.5, 1.0]]) + rng.uniform(-0.1, 0.1, size=(4, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    t = 6.0 * dirs + rng.uniform(-0.3, 0.3, size=(4, 3))
    R = np.zeros((4, 3, 3))
    for i in range(4):
        z = -dirs[i] + rng.uniform(-0.1, 0.1, size=3)
        z /= np.linalg.norm(z)
        x = np.cross(rng.normal(size=3), z)
        x /= np.linalg.norm(x)
        R[i] = np.stack([x, np.cross(z, x), z], axis=1)
    poses = S._iso_pack(R, t)
    points = rng.uniform(-1.0, 1.0, size=(12, 3)) * 1.5 / np.sqrt(3.0)
    k = np.arange(n_edges)
    vp, vl = (k % 4).astype(np.int32), ((k // 4) % 12).astype(np.int32)
    zl = SC.scam_edges_numpy(poses, points, vp, vl, np.zeros((n_edges, 3)), KCAM, jac=False)
    zl = zl + rng.normal(size=(n_edges, 3)) * np.array([1.0, 1.0, 1.0 / 16.0])
    vi, vj = np.arange(3, dtype=np.int32), np.arange(1, 4, dtype=np.int32)
    noise = S._iso_pack(S._exp_so3(rng.normal(size=(3, 3)) * 0.01)[0], rng.normal(size=(3, 3)) * 0.02)
    Z = np.stack([OE.se3_compose(OE.se3_compose(OE.se3_invert(poses[a]), poses[b]), nz) for a, b, nz in zip(vi, vj, noise)])
    A = rng.normal(size=(3, 3)) * 0.2
    W = np.eye(3) + A @ A.T
    return dict(kind="se3", observation="stereo_vsc", kcam=KCAM.copy(), n=4, nP=3, L=12, nL=11, E=3, M=n_edges, poses=poses,
                hidx=np.array([-1, 0, 1, 2], np.int32), points=points,
                pt_hidx=np.concatenate([3 + np.arange(11), [-1]]).astype(np.int32), vi=vi, vj=vj, Z=Z,
                omega=np.tile(np.eye(6).reshape(1, -1), (3, 1)), vp=vp, vl=vl, zl=zl,
                omega_l=W.reshape(1, 9) * (1.0 + 0.5 * (k % 3))[:, None])


def take_edges(g, idx):
    """g with the stereo observations idx only (a slice or an index array); every vertex stays."""
    out = dict(g)
    for k in EDGE_KEYS:
        out[k] = np.ascontiguousarray(np.asarray(g[k])[idx])
    out["M"] = len(out["vp"])
    return out


def load_graph(z, n=300):
    """The fixture's graph with its first n observations."""
    g = {k: z["graph_" + k] for k in GRAPH_KEYS}
    g.update(kind="se3", observation="stereo_vsc", kcam=KCAM.copy(), n=len(g["hidx"]), nP=int((g["hidx"] >= 0).sum()), L=len(g["pt_hidx"]),
             nL=int((g["pt_hidx"] >= 0).sum()), E=len(g["vi"]))
    return take_edges(g, slice(0, n))


def producers(F, g, poses=None, points=None, jac=True):
    """(J0, J1, err) of the stereo set, or err; F = FP64: the whole-array form of scam.py (the same bits as its scalar form)."""
    poses, points = g["poses"] if poses is None else poses, g["points"] if points is None else points
    if F is FP64:
        return SC.scam_edges_numpy(poses, points, g["vp"], g["vl"], g["zl"], g["kcam"], jac)
    return SC.scam_edges(F, poses, points, g["vp"], g["vl"], g["zl"], g["kcam"], jac)


def depths(g, poses=None, points=None):
    """q2 of every observation in fp64."""
    poses, points = g["poses"] if poses is None else poses, g["points"] if points is None else points
    return np.array([SC.camera_point(FP64, poses[a], points[b])[2] for a, b in zip(g["vp"], g["vl"])])


def pose_edges(g, poses=None, jac=True):
    if len(g["vi"]) == 0:
        return (np.zeros((0, 36)), np.zeros((0, 36)), np.zeros((0, 6))) if jac else np.zeros((0, 6))
    return O.se3_edges(g["poses"] if poses is None else poses, g["vi"], g["vj"], g["Z"], jac=jac)


def gicp_edges(g, poses=None, jac=True):
    return G.gicp_edges(FP64, g["poses"] if poses is None else poses, g["gi"], g["gj"], g["gmeas"], g.get("gcov"), jac=jac)


def oplus(g, poses, points, x):
    """(poses, points) moved by the step x over the free cameras (the oracle's oplus) and the free points (plain addition)."""
    return O.se3_oplus(poses, g["hidx"], x), LH.points_oplus(points, g["pt_hidx"], x, 6 * g["nP"], g["nP"])


def update_step(g, seed):
    """A step over the free cameras and points that moves every estimate visibly and keeps every depth near 6."""
    rng = np.random.default_rng(seed)
    return np.concatenate([(rng.normal(size=(g["nP"], 6)) * np.array([0.1, 0.1, 0.1, 0.02, 0.02, 0.02])).ravel(),
                           rng.normal(size=3 * g["nL"]) * 0.1])


def has_gicp(g):
    return g.get("gi") is not None


def has_prior(g):
    return g.get("prior") is not None


def oracle_scam(g, schur=True):
    """OracleSolver with sets 0 = EdgeSE3 (possibly empty), 1 = the stereo observations, then the GICP set and the prior set if
    the graph has them; structure built.  Returns (oracle, id of the GICP set or None, id of the prior set or None)."""
    h, hl = np.asarray(g["hidx"], np.int32), np.asarray(g["pt_hidx"], np.int32)
    o = O.OracleSolver(6, 3, g["nP"], g["nL"], schur)
    o.set_dims(o.add_edge_set(6, h[g["vi"]], h[g["vj"]]), 6, 6)
    o.set_dims(o.add_edge_set(3, h[g["vp"]], hl[g["vl"]]), 6, 3)
    kg = kq = None
    if has_gicp(g):
        kg = o.add_edge_set(3, h[g["gi"]], h[g["gj"]])
        o.set_dims(kg, 6, 6)
    if has_prior(g):
        kq = o.add_edge_set(6, h[g["vq"]], None)
        o.set_dims(kq, 6, 0)
    o.build_structure()
    return o, kg, kq


def prior_edges(g, poses=None, jac=True):
    from tests import prior_helpers as PH
    return PH.prior_edges(g, poses=poses, jac=jac)


def feed_oracle(g, o, kg, kq, huber=0.0, poses=None, points=None):
    A0, A1, e0 = pose_edges(g, poses)
    o.set_edge_data(0, A0, A1, g["omega"], e0)
    J0, J1, err = producers(FP64, g, poses, points)
    o.set_edge_data(1, J0, J1, g["omega_l"], err, huber)
    if kg is not None:
        G0, G1, eg = gicp_edges(g, poses)[:3]
        o.set_edge_data(kg, G0, G1, g["ginfo"], eg)
    if kq is not None:
        Q0, eq = prior_edges(g, poses)
        o.set_edge_data(kq, Q0, None, g["omega_q"], eq)
    return J0, J1, err


class HostScamGraph:
    """The graph protocol of openslam_g2o_amd.lm with the estimates on the host, the EdgeSE3 set from the oracle's edges, the
    stereo set from scam.py in fp64, the GICP set from gicp.py.  feed(set, J0, J1, omega, err)."""

    def __init__(self, g, feed, get_x, chi2_fn, kg, huber=0.0):
        self.g, self.feed, self.get_x, self.chi2_fn, self.kg = g, feed, get_x, chi2_fn, kg
        self.poses, self.points = np.array(g["poses"], np.float64), np.array(g["points"], np.float64)
        self.stack = []
        self.J = None

    def _feed(self, jac):
        g = self.g
        if jac:
            A0, A1, e0 = pose_edges(g, self.poses)
            J0, J1, err = producers(FP64, g, self.poses, self.points)
            self.J = [A0, A1, J0, J1]
            if self.kg is not None:
                G0, G1, eg = gicp_edges(g, self.poses)[:3]
                self.J += [G0, G1]
        else:
            e0 = pose_edges(g, self.poses, jac=False)
            err = producers(FP64, g, self.poses, self.points, jac=False)
            if self.kg is not None:
                eg = gicp_edges(g, self.poses, jac=False)
                eg = eg[0] if isinstance(eg, tuple) else eg
        self.feed(0, self.J[0], self.J[1], g["omega"], e0)
        self.feed(1, self.J[2], self.J[3], g["omega_l"], err)
        if self.kg is not None:
            self.feed(self.kg, self.J[4], self.J[5], g["ginfo"], eg)

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


def dx_tolerance(o, schur=True):
    """tests.helpers.dx_tolerance: max(TOL_DX, 4 cond eps) with cond of the system the oracle factorises -- the damped reduced pose
    system with the Schur complement, the damped pose block Hpp alone without it (same layout: upper block triangle by columns,
    column-major blocks)."""
    from tests import helpers
    if schur:
        return helpers.dx_tolerance(o)
    cp, ri = o.pattern("pp")
    p, nb = o.p, len(cp) - 1
    Hd = np.zeros((nb * p, nb * p))
    V = o.values("Hpp").reshape(-1, p, p)
    for c in range(nb):
        for q in range(cp[c], cp[c + 1]):
            r = ri[q]
            Hd[r * p:(r + 1) * p, c * p:(c + 1) * p] = V[q].T
            Hd[c * p:(c + 1) * p, r * p:(r + 1) * p] = V[q]
    ev = np.linalg.eigvalsh(Hd)
    cond = ev[-1] / ev[0]
    return max(helpers.TOL_DX, 4.0 * cond * np.finfo(float).eps), cond


def lm_graph(gicp=False):
    return S.make_scam_ba(LM_CAMS, LM_POINTS, gicp=gicp)


def oracle_lm_run(g, iterations=LM_ITERATIONS, dense=False, huber=0.0):
    """lm.optimize over the CPU oracle fed by the fp64 producers; dense: the same loop solving the full system with numpy's
    Cholesky.  Returns dict(done, chis, trials, poses, points)."""
    from openslam_g2o_amd import lm
    o, kg, _ = oracle_scam(g, True)

    def feed(k, J0, J1, om, err):
        o.set_edge_data(k, J0, J1, om, err, huber if k == 1 else 0.0)
    graph = HostScamGraph(g, feed, o.x, o.chi2, kg)
    done, chis, lams, trials = lm.optimize(graph, LH.OracleLandmarkSolver(o, dense), iterations, "lm")
    return dict(done=done, chis=np.array(chis), lams=np.array(lams), trials=[int(t) for t in trials], poses=graph.poses.copy(),
                points=graph.points.copy())


def device_setup(g, huber=0.0, schur=True, options=None):
    """lm.setup_device_landmark_slam for a problem dict with a stereo set; returns (solver, graph)."""
    from openslam_g2o_amd import lm
    return lm.setup_device_landmark_slam(g, huber_delta=huber, schur=schur, options=options)
