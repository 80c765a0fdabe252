"""NumPy restatement of the stereo projection edge for the tests (and the host-fed baseline of tools/ba_stereo_time.py),
written from the formulas of the reference and independent of the kernel:

  EdgeProjectXYZ2UVU::computeError       g2o/types/sba/types_six_dof_expmap.h:181-200
  CameraParameters::stereocam_uvu_map    g2o/types/sba/types_six_dof_expmap.cpp:40, 77-82

  (x, y, z) = R X + t,  e = meas - (f x / z + cx, f y / z + cy, f (x - b) / z + cx)
  J0 (point, 3 x 3): rows 0-1 of EdgeProjectXYZ2UV::linearizeOplus (types_six_dof_expmap.cpp:288-326), row 2 =
                     -(1 / z) [f, 0, -f (x - b) / z] R
  J1 (pose, 3 x 6, update (omega, upsilon)): rows 0-1 as there, row 2 =
                     f [(x - b) y / z^2, -(1 + x (x - b) / z^2), y / z, -1 / z, 0, (x - b) / z^2]

The reference has no analytic Jacobian for this edge (linearizeOplus is commented out, types_six_dof_expmap.h:199); the formulas
are checked against central differences in tests/test_stereo_host.py.  Layouts as in g2ohip_set_edge_data: J0 [n][3 x 3],
J1 [n][3 x 6] column-major, err [n][3]; vertex 0 of an edge is the point, vertex 1 the pose."""
import numpy as np

from openslam_g2o_amd import synthetic as S
from oracle import oracle as O
from tests import landmark_helpers as LH

GRAPH = (40, 205)          # 5 observations per landmark: exactly 1025 observations
BASELINE = 0.2


def stereo_edges(cams, pts, cam_idx, pt_idx, meas, f, cx, cy, b, jac=True):
    T = np.asarray(cams, np.float64)[cam_idx]
    X = np.asarray(pts, np.float64)[pt_idx]
    R = T[:, 0:9].reshape(-1, 3, 3).transpose(0, 2, 1)
    Xc = np.einsum("nij,nj->ni", R, X) + T[:, 9:12]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    xr = x - b
    err = np.asarray(meas, np.float64) - np.stack([f * x / z + cx, f * y / z + cy, f * xr / z + cx], axis=1)
    if not jac:
        return err
    n = len(x)
    z2 = z * z
    tmp = np.zeros((n, 3, 3))
    tmp[:, 0, 0] = tmp[:, 1, 1] = tmp[:, 2, 0] = f
    tmp[:, 0, 2] = -f * x / z
    tmp[:, 1, 2] = -f * y / z
    tmp[:, 2, 2] = -f * xr / z
    A = (-1.0 / z)[:, None, None] * (tmp @ R)
    B = np.zeros((n, 3, 6))
    B[:, 0, 0] = f * x * y / z2
    B[:, 0, 1] = -f * (1 + x * x / z2)
    B[:, 0, 2] = f * y / z
    B[:, 0, 3] = -f / z
    B[:, 0, 5] = f * x / z2
    B[:, 1, 0] = f * (1 + y * y / z2)
    B[:, 1, 1] = -f * x * y / z2
    B[:, 1, 2] = -f * x / z
    B[:, 1, 4] = -f / z
    B[:, 1, 5] = f * y / z2
    B[:, 2, 0] = f * xr * y / z2
    B[:, 2, 1] = -f * (1 + x * xr / z2)
    B[:, 2, 2] = f * y / z
    B[:, 2, 3] = -f / z
    B[:, 2, 5] = f * xr / z2
    J0 = np.ascontiguousarray(A.transpose(0, 2, 1).reshape(n, 9))
    J1 = np.ascontiguousarray(B.transpose(0, 2, 1).reshape(n, 18))
    return J0, J1, err


def linearize(prob, cams=None, pts=None, jac=True):
    """(J0 [E][9], J1 [E][18], err [E][3]) of a stereo problem, or err alone."""
    cams = prob["cams"] if cams is None else cams
    pts = prob["pts"] if pts is None else pts
    return stereo_edges(cams, pts, prob["cam_idx"], prob["pt_idx"], prob["meas"], prob["f"], prob["cx"], prob["cy"], prob["baseline"],
                        jac=jac)


def omega(prob):
    """The problem's information matrices [E][9] column-major: prob["omega"] or identities."""
    if prob.get("omega") is not None:
        return np.asarray(prob["omega"], np.float64)
    return np.tile(np.eye(3).reshape(9), (prob["E"], 1))


def full_information(E):
    """E different symmetric positive definite 3 x 3 matrices with off-diagonal entries, column-major [E][9]."""
    rng = S.CounterRng(7)
    M = np.stack([rng.uniform(40 + i, E) - 0.5 for i in range(9)], axis=1).reshape(E, 3, 3)
    W = np.einsum("nij,nkj->nik", M, M) + np.diag([1.0, 0.8, 1.5])[None]
    return np.ascontiguousarray(W.transpose(0, 2, 1).reshape(E, 9))


def pt_hidx(prob):
    """Landmark index (0-based) of every point or -1: what g2ohip_ba_set_estimates takes."""
    return np.asarray(prob.get("pt_hidx", np.arange(prob["L"])), np.int32)


def graph(**kw):
    P, L = GRAPH
    return S.make_ba_problem(P, L, stereo_baseline=BASELINE, **kw)


def with_fixed_points(prob, k):
    """The first k points fixed: they leave the structure, their observations keep the pose side only."""
    g = dict(prob)
    h = np.arange(g["L"], dtype=np.int32) - k
    h[:k] = -1
    g["pt_hidx"] = h
    g["nL"] = g["L"] - k
    hp = h[g["pt_idx"]]
    g["v0"] = np.where(hp >= 0, g["nP"] + hp, -1).astype(np.int32)
    return g


def with_duplicate(prob, e):
    """Observation e a second time (another measurement of the same (pose, landmark) pair), appended."""
    g = dict(prob)
    for key in ("cam_idx", "pt_idx", "v0", "v1"):
        g[key] = np.concatenate([g[key], g[key][e:e + 1]])
    g["meas"] = np.concatenate([g["meas"], g["meas"][e:e + 1] + np.array([[0.7, -0.4, 0.9]])])
    g["E"] = g["E"] + 1
    return g


def truncated(prob, E):
    """The first E observations; points that lose all their observations are fixed and leave the structure, cameras that lose
    theirs stay (an empty block column of the pose system is regularised by the damping alone: producers-only use)."""
    g = dict(prob)
    for key in ("cam_idx", "pt_idx", "meas"):
        g[key] = g[key][:E]
    g["E"] = E
    seen = np.bincount(g["pt_idx"], minlength=g["L"]) > 0
    g["nL"] = int(seen.sum())
    g["pt_hidx"] = np.where(seen, np.cumsum(seen) - 1, -1).astype(np.int32)
    g["v0"] = (g["nP"] + g["pt_hidx"][g["pt_idx"]]).astype(np.int32)
    g["v1"] = g["cam_hidx"][g["cam_idx"]].astype(np.int32)
    return g


LM_PERTURB = (0.04, 0.1, 0.3)      # see lm_test_graph: rotation [rad], translation, points


def lm_test_graph():
    """The graph of the whole-run comparisons: graph() with its free cameras and its points moved further from the optimum
    (counter streams of their own), far enough that ten LM iterations are still descending at the end, so that every accept /
    reject decision is determined by the data and not by the last bits; every point stays in front of its cameras."""
    g = graph()
    rng = S.CounterRng(43)
    P, L = GRAPH
    rot, tr, pt = LM_PERTURB
    upd = np.zeros((P, 6))
    upd[:, 0:3] = rot * np.stack([rng.normal(50, P), rng.normal(51, P), rng.normal(52, P)], axis=1)
    upd[:, 3:6] = tr * np.stack([rng.normal(53, P), rng.normal(54, P), rng.normal(55, P)], axis=1)
    upd[g["cam_hidx"] < 0] = 0.0
    g["cams"] = S._apply_cam_update(g["cams"], upd)
    g["pts"] = g["pts"] + pt * np.stack([rng.normal(56, L), rng.normal(57, L), rng.normal(58, L)], axis=1)
    return g


def oracle_stereo(prob, schur=True):
    """OracleSolver with the problem's one edge set (error dimension 3, vertex 0 = point, vertex 1 = pose), structure built."""
    o = O.OracleSolver(6, 3, prob["nP"], prob["nL"], schur)
    k = o.add_edge_set(3, prob["v0"], prob["v1"])
    o.set_dims(k, 3, 6)
    o.build_structure()
    return o


def oplus(prob, x):
    """synthetic.ba_oplus for a problem whose points may be fixed (pt_hidx)."""
    if "pt_hidx" not in prob:
        return S.ba_oplus(prob, x)
    h = pt_hidx(prob)
    xl = np.zeros((prob["L"], 3))
    xl[h >= 0] = np.asarray(x)[6 * prob["nP"]:].reshape(-1, 3)[h[h >= 0]]
    full = dict(prob, nL=prob["L"])
    new = S.ba_oplus(full, np.concatenate([np.asarray(x)[:6 * prob["nP"]], xl.ravel()]))
    new["nL"] = prob["nL"]
    return new


class HostStereoGraph:
    """The lm.py graph protocol with the estimates on the host and the NumPy producers above.  `feed(J0, J1, omega, err)` hands
    the set's data to whichever solver is driven."""

    def __init__(self, prob, feed, get_x, chi2):
        self.pr = dict(prob)
        self.feed, self.get_x, self._chi2 = feed, get_x, chi2
        self.om = omega(prob)
        self.stack = []
        self._J = None

    def linearize(self):
        J0, J1, err = linearize(self.pr)
        self._J = (J0, J1)
        self.feed(J0, J1, self.om, err)

    def compute_active_errors(self):
        self.feed(self._J[0], self._J[1], self.om, linearize(self.pr, jac=False))

    def chi2(self):
        return self._chi2()

    def update(self):
        self.pr = oplus(self.pr, self.get_x())

    def push(self):
        self.stack.append((self.pr["cams"].copy(), self.pr["pts"].copy()))

    def pop(self):
        self.pr["cams"], self.pr["pts"] = self.stack.pop()

    def discard_top(self):
        self.stack.pop()


def oracle_lm_run(prob, iterations, huber=0.0, dense=False):
    """lm.optimize over the oracle + the NumPy producers (dense: the full system solved without elimination, see
    tests/landmark_helpers.OracleLandmarkSolver).  Returns (done, chis, lams, trials, graph)."""
    from openslam_g2o_amd import lm
    o = oracle_stereo(prob, True)

    def feed(J0, J1, om, err):
        o.set_edge_data(0, J0, J1, om, err, huber)
    g = HostStereoGraph(prob, feed, o.x, o.chi2)
    done, chis, lams, trials = lm.optimize(g, LH.OracleLandmarkSolver(o, dense), iterations, "lm")
    return done, chis, lams, trials, g
