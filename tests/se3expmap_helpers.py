"""Test side of the BA front end's pose-pose slot (EdgeSE3Expmap, g2ohip_ba_set_pose_edges): the graphs of the tests, the
reference at 60 digits (tests/reference_mp.py for the group operations and the oplus; SE3Quat::log and adj written here from
g2o/types/slam3d/se3quat.h:178-215, 259-268 with mpmath, sharing no code with openslam_g2o_amd/se3expmap.py), the CPU oracle
over both sets and host-fed graphs for lm.optimize."""
import os

import mpmath as mp
import numpy as np

from openslam_g2o_amd import se3expmap as X
from openslam_g2o_amd import synthetic as S
from oracle import oracle as O
from tests import reference_mp as R

EDGE_COUNTS = (1, 65, 256, 257, 300)      # one lane per edge: a wave boundary, a full block, one over, a partial last block
DRIFT_FACTOR = 8.0                        # device-vs-restatement bound = 8 x the recorded fp64-vs-mpmath drift
BA = (8, 40)                              # the projection problem the pose edges stand beside: 8 cameras (0, 1 fixed), 40 points
LOG_SWITCH = mp.mpf(0.99999)              # the fp64 literal of SE3Quat::log
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "se3expmap_edges.npz")
LM_ARGS = dict(P=12, L=60, loop_every=4)
LM_ITERATIONS = 6
LM_HUBER = 10.0                           # width of the Huber kernel on the pose set (units of sqrt(e' Omega e))


# ------------------------------------------------------------------------------------------------ 60-digit reference
def mp_log(Xm):
    Rm, t = Xm
    d = (Rm[0][0] + Rm[1][1] + Rm[2][2] - 1) / 2
    dR = [Rm[2][1] - Rm[1][2], Rm[0][2] - Rm[2][0], Rm[1][0] - Rm[0][1]]
    I = [[mp.mpf(int(r == c)) for c in range(3)] for r in range(3)]
    if d > LOG_SWITCH:
        w = [v / 2 for v in dR]
        cf = mp.mpf(1) / 12
    else:
        th = mp.acos(d)
        w = [th / (2 * mp.sqrt(1 - d * d)) * v for v in dR]
        cf = (1 - th / (2 * mp.tan(th / 2))) / (th * th)
    Om = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    Om2 = R.mat3(Om, Om)
    Vi = [[I[r][c] - Om[r][c] / 2 + cf * Om2[r][c] for c in range(3)] for r in range(3)]
    return w + R.mv3(Vi, t), d


def mp_adj(Xm, sign=1):
    Rm, t = Xm
    Sk = [[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]
    SR = R.mat3(Sk, Rm)
    M = [[mp.mpf(0)] * 6 for _ in range(6)]
    for r in range(3):
        for c in range(3):
            M[r][c] = sign * Rm[r][c]
            M[3 + r][3 + c] = sign * Rm[r][c]
            M[3 + r][c] = sign * SR[r][c]
    return [M[r][c] for c in range(6) for r in range(6)]      # column-major


def mp_edge(Ti, Tj, C):
    """(J0 [36], J1 [36], err [6], d) of one edge at 60 digits."""
    Xi, Xj, Xc = R.iso(Ti), R.iso(Tj), R.iso(C)
    A = R.iso_mul(R.iso_inv(Xj), Xc)
    e, d = mp_log(R.iso_mul(A, Xi))
    return mp_adj(A), mp_adj(R.iso_mul(R.iso_inv(Xi), R.iso_inv(Xc)), -1), e, d


def mp_pose_edges(cams, vi, vj, meas, jac=True):
    """The edge list at 60 digits, rounded to fp64: (J0, J1, err, d) or (err, d)."""
    n = len(vi)
    J0, J1, err, dd = np.zeros((n, 36)), np.zeros((n, 36)), np.zeros((n, 6)), np.zeros(n)
    for k in range(n):
        a, b, e, d = mp_edge(cams[int(vi[k])], cams[int(vj[k])], meas[k])
        J0[k], J1[k], err[k], dd[k] = R.f64(a), R.f64(b), R.f64(e), float(d)
    return (J0, J1, err, dd) if jac else (err, dd)


def mp_oplus(cams, hidx, x):
    """VertexSE3Expmap::oplusImpl of the free cameras at 60 digits, rounded to fp64."""
    out = np.array(cams, np.float64).copy()
    for v, h in enumerate(hidx):
        if h >= 0:
            out[v] = R.f64(R.iso_pack(R.expmap_oplus(R.iso(cams[v]), R.V(x[6 * h:6 * h + 6]))))
    return out


# ------------------------------------------------------------------------------------------------ graphs
def _spd6(rng, n):
    W = rng.normal(size=(n, 6, 6))
    M = W @ W.transpose(0, 2, 1) + 6 * np.eye(6)
    return np.ascontiguousarray(M.transpose(0, 2, 1).reshape(n, 36))


def base_graph(n_edges):
    """make_ba_problem(*BA) with camera 2 moved onto camera 0 (fixed, identity rotation: two identical poses), and the first
    n_edges of a list of 300 pose edges between its 8 cameras: edge 0 has the fixed camera 0 as vertex 0, edge 1 as vertex 1,
    edges 2 and 3 join the same pair, edge 4 the same pair in the other order, edge 5 joins the identical cameras 0 and 2 with
    the identity as measurement (error exactly zero), edges 6 and 7 have a relative rotation of 1e-3 (small-angle branch).
    Every other measurement is Tj exp(x) Ti^-1 with |omega| in [0.05, 1.5], so that the error is about x."""
    prob = S.make_ba_problem(*BA)
    prob["cams"] = prob["cams"].copy()
    prob["cams"][2] = prob["cams"][0]
    rng = np.random.default_rng(300)
    N = 300
    head = [(0, 3), (4, 0), (3, 4), (3, 4), (4, 3), (0, 2), (5, 6), (7, 5)]
    a = rng.integers(2, 8, size=N)
    b = (a - 2 + rng.integers(1, 6, size=N)) % 6 + 2                  # another free camera
    vi, vj = a.astype(np.int32), b.astype(np.int32)
    for k, (p, q) in enumerate(head):
        vi[k], vj[k] = p, q
    axis = rng.normal(size=(N, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    ang = rng.uniform(0.05, 1.5, size=N)
    ang[6:8] = 1e-3
    x = np.concatenate([axis * ang[:, None], rng.normal(size=(N, 3)) * 0.3], axis=1)
    cams = prob["cams"]
    meas = X.pack(X.product(X.product(X.unpack(cams[vj]), X.unpack(X.exp(x))), X.inverse(X.unpack(cams[vi]))))
    meas[5] = (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    info = _spd6(rng, N)
    h = prob["cam_hidx"]
    sl = slice(0, n_edges)
    prob["pose_edges"] = dict(n=n_edges, vi=vi[sl].copy(), vj=vj[sl].copy(), v0=h[vi[sl]].astype(np.int32), v1=h[vj[sl]].astype(np.int32),
                              meas=np.ascontiguousarray(meas[sl]), info=np.ascontiguousarray(info[sl]))
    return prob


def load_graph(z, n):
    """base_graph(n) as the fixture holds it."""
    prob = S.make_ba_problem(*BA)
    prob["cams"] = z["cams"]
    h = prob["cam_hidx"]
    vi, vj = z["vi"][:n], z["vj"][:n]
    prob["pose_edges"] = dict(n=n, vi=vi, vj=vj, v0=h[vi].astype(np.int32), v1=h[vj].astype(np.int32), meas=z["meas"][:n], info=z["info"][:n])
    return prob


def producers(prob, cams=None, jac=True):
    pe = prob["pose_edges"]
    return X.pose_edges(prob["cams"] if cams is None else cams, pe["vi"], pe["vj"], pe["meas"], jac)


def lm_graph():
    """The graph of the whole-run comparisons: make_ba_odometry with its free cameras and points moved further from the optimum
    (as tests/stereo_helpers.lm_test_graph does), so that the iterations are still descending at the end."""
    g = S.make_ba_odometry(**LM_ARGS)
    rng = S.CounterRng(43)
    P, L = LM_ARGS["P"], LM_ARGS["L"]
    upd = np.zeros((P, 6))
    upd[:, 0:3] = 0.04 * np.stack([rng.normal(50, P), rng.normal(51, P), rng.normal(52, P)], axis=1)
    upd[:, 3:6] = 0.1 * np.stack([rng.normal(53, P), rng.normal(54, P), rng.normal(55, P)], axis=1)
    upd[g["cam_hidx"] < 0] = 0.0
    g["cams"] = S._apply_cam_update(g["cams"], upd)
    g["pts"] = g["pts"] + 0.3 * np.stack([rng.normal(56, L), rng.normal(57, L), rng.normal(58, L)], axis=1)
    return g


# ------------------------------------------------------------------------------------------------ the CPU oracle, both sets
def oracle_both(prob, schur=True):
    """OracleSolver with sets 0 / 1 = the (mono) projection set / the pose set, structure built."""
    pe = prob["pose_edges"]
    o = O.OracleSolver(6, 3, prob["nP"], prob["nL"], schur)
    k = o.add_edge_set(2, prob["v0"], prob["v1"])
    o.set_dims(k, 3, 6)
    k = o.add_edge_set(6, pe["v0"], pe["v1"])
    o.set_dims(k, 6, 6)
    o.build_structure()
    return o


class HostGraph:
    """The lm.py graph protocol with the estimates on the host: the projection set from synthetic.ba_linearize, the pose set from
    `pose_fn(cams, jac)` (se3expmap.py in fp64, or the 60-digit reference rounded to fp64).  feed(set, J0, J1, omega, err)."""

    def __init__(self, prob, feed, get_x, chi2, pose_fn):
        self.pr = dict(prob)
        self.feed, self.get_x, self._chi2, self.pose_fn = feed, get_x, chi2, pose_fn
        self.stack, self._J = [], None

    def _eval(self, jac):
        pe = self.pr["pose_edges"]
        if jac:
            Jp, Jc, e = S.ba_linearize(self.pr)
            A, B, pe_err = self.pose_fn(self.pr["cams"], True)
            self._J = (Jp, Jc, A, B)
        else:
            e, pe_err = S.ba_linearize(self.pr, jac=False), self.pose_fn(self.pr["cams"], False)
        Jp, Jc, A, B = self._J
        self.feed(0, Jp, Jc, S.ba_omega(self.pr), e)
        self.feed(1, A, B, pe["info"], pe_err)

    def linearize(self):
        self._eval(True)

    def compute_active_errors(self):
        self._eval(False)

    def chi2(self):
        return self._chi2()

    def update(self):
        self.pr = S.ba_oplus(self.pr, self.get_x())

    def push(self):
        self.stack.append((self.pr["cams"].copy(), self.pr["pts"].copy()))

    def pop(self):
        self.pr["cams"], self.pr["pts"] = self.stack.pop()

    def discard_top(self):
        self.stack.pop()


def oracle_lm_run(prob, pose_fn, iterations=LM_ITERATIONS, huber=0.0):
    """lm.optimize over the oracle with the pose set fed by pose_fn.  Returns dict(chis, trials, cams, pts)."""
    from openslam_g2o_amd import lm
    from tests.landmark_helpers import OracleLandmarkSolver
    o = oracle_both(prob)

    def feed(k, J0, J1, om, err):
        o.set_edge_data(k, J0, J1, om, err, huber if k == 1 else 0.0)
    g = HostGraph(prob, feed, o.x, o.chi2, pose_fn)
    done, chis, lams, trials = lm.optimize(g, OracleLandmarkSolver(o, False), iterations, "lm")
    return dict(done=done, chis=np.array(chis), trials=[int(t) for t in trials], cams=g.pr["cams"].copy(), pts=g.pr["pts"].copy())


def fp64_pose_fn(prob):
    pe = prob["pose_edges"]
    return lambda cams, jac: X.pose_edges(cams, pe["vi"], pe["vj"], pe["meas"], jac)


def mp_pose_fn(prob):
    pe = prob["pose_edges"]

    def fn(cams, jac):
        out = mp_pose_edges(cams, pe["vi"], pe["vj"], pe["meas"], jac)
        return out[:3] if jac else out[0]
    return fn
