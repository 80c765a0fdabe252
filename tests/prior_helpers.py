"""NumPy restatement of the unary pose priors and host-side graphs that carry them, for the tests of the device prior set
(g2ohip_pg_set_prior_edges):

  EdgeSE2Prior::computeError                      g2o/types/slam2d/edge_se2_prior.h:45-50 (its analytic Jacobian is compiled
                                                  out, :52-58; the restatement gives the exact derivative the disabled code states)
  EdgeSE2XYPrior::computeError / linearizeOplus   g2o/types/slam2d/edge_se2_xyprior.h:66-70, edge_se2_xyprior.cpp:60-63
  EdgeSE3Prior::computeError / linearizeOplus     g2o/types/slam3d/edge_se3_prior.cpp:94-107, computeEdgeSE3PriorGradient
                                                  (isometry3d_gradients.h:269-330), compute_dq_dR as oracle/g2o_oracle_types.c
                                                  re-derives it from the four-case rotation -> quaternion formulas

Layouts as in g2ohip_set_edge_data for a unary set: J0 [n][d x dim] column-major, err [n][d]; SE3 poses and measurements are
isometries [12] = R column-major | t."""
import numpy as np

from openslam_g2o_amd import g2o_io
from oracle import oracle as O
from tests import landmark_helpers as LH

IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def _normalize_theta(t):
    """normalize_theta (g2o/stuff/misc.h): into [-pi, pi)."""
    return (np.asarray(t) + np.pi) % (2.0 * np.pi) - np.pi


def se2_prior_edges(poses, vq, meas, jac=True):
    """e = (Z^-1 X).toVector(), computed as the reference does (SE2::inverse, then the product); J = [Rz' 0; 0 1]."""
    x, z = np.asarray(poses, np.float64)[vq], np.asarray(meas, np.float64)
    thi = _normalize_theta(-z[:, 2])                       # Z^-1 = (R(-th) (-t), -th)
    c, s = np.cos(thi), np.sin(thi)
    tix, tiy = c * (-z[:, 0]) - s * (-z[:, 1]), s * (-z[:, 0]) + c * (-z[:, 1])
    err = np.stack([tix + c * x[:, 0] - s * x[:, 1], tiy + s * x[:, 0] + c * x[:, 1], _normalize_theta(thi + x[:, 2])], axis=1)
    if not jac:
        return err
    o, l = np.zeros(len(x)), np.ones(len(x))
    J0 = np.stack([c, s, o, -s, c, o, o, o, l], axis=1)    # column-major 3x3 of [c -s 0; s c 0; 0 0 1] = [Rz' 0; 0 1]
    return J0, err


def se2_xy_prior_edges(poses, vq, meas, jac=True):
    """e = t - z, J = [1 0 0; 0 1 0]."""
    err = np.asarray(poses, np.float64)[vq][:, :2] - np.asarray(meas, np.float64)
    if not jac:
        return err
    return np.tile(np.array([1.0, 0, 0, 1, 0, 0]), (len(err), 1)), err


def _iso(T):
    T = np.asarray(T, np.float64).reshape(-1, 12)
    return T[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1), T[:, 9:]


def quat_case(R):
    """Branch of Eigen's rotation -> quaternion conversion: 0 (trace > 0) or 1 + index of the largest diagonal entry."""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return 1 + i


def _dq_dR(R):
    """d(qx, qy, qz) / d vec(R), 3 x 9 with vec column-major: the partials of the case formulas of dquat2mat.cpp:9-43."""
    D = np.zeros((3, 9))
    col = lambda a, b: a + 3 * b
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        w = 0.5 * np.sqrt(tr + 1.0)
        qw = w
        num = (R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1])
        pa, pb = (2, 0, 1), (1, 2, 0)
        for c in range(3):
            D[c, [col(0, 0), col(1, 1), col(2, 2)]] = -num[c] / (32.0 * w ** 3)
            D[c, col(pa[c], pb[c])] = 0.25 / w
            D[c, col(pb[c], pa[c])] = -0.25 / w
    else:
        if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
            i = 0
        elif R[1, 1] > R[2, 2]:
            i = 1
        else:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 0.5 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        qw = (R[k, j] - R[j, k]) / (4.0 * s)
        D[i, col(i, i)] = 1.0 / (8.0 * s)
        D[i, col(j, j)] = D[i, col(k, k)] = -1.0 / (8.0 * s)
        for c in (j, k):
            dd = (R[c, i] + R[i, c]) / (32.0 * s ** 3)
            D[c, col(c, i)] += 0.25 / s
            D[c, col(i, c)] += 0.25 / s
            D[c, col(i, i)] -= dd
            D[c, col(j, j)] += dd
            D[c, col(k, k)] += dd
    return -D if qw <= 0 else D


def se3_prior_edges(poses, vq, meas, offset=None, jac=True):
    """A = Z^-1 X, E = A P, e = toVectorMQT(E) (translation | vector part of the unit quaternion, w >= 0);
    J[0:3,0:3] = Ra, J[0:3,3:6] = Ra skew(tP), J[3:6,3:6] = dq_dR(Re) [Ra Sx(RP); Ra Sy(RP); Ra Sz(RP)]."""
    Rx, tx = _iso(np.asarray(poses, np.float64)[vq])
    Rz, tz = _iso(meas)
    Rp, tp = _iso(IDENTITY if offset is None else offset)
    Rp, tp = Rp[0], tp[0]
    Rzi = Rz.transpose(0, 2, 1)
    tzi = -np.einsum("nij,nj->ni", Rzi, tz)
    Ra = Rzi @ Rx
    ta = np.einsum("nij,nj->ni", Rzi, tx) + tzi
    Re = Ra @ Rp
    te = np.einsum("nij,j->ni", Ra, tp) + ta
    err = np.concatenate([te, g2o_io._R_to_quat(Re)[:, :3]], axis=1)
    if not jac:
        return err
    n = len(err)
    x, y, z = 2.0 * tp
    S = np.array([[0, z, -y], [-z, 0, x], [y, -x, 0]])                    # skew(tP), doubled (isometry3d_gradients.h:42-47)
    r = 2.0 * Rp
    Sxyz = [np.array([[0, 0, 0], -r[2], r[1]]), np.array([r[2], [0, 0, 0], -r[0]]), np.array([-r[1], r[0], [0, 0, 0]])]
    J = np.zeros((n, 6, 6))
    J[:, :3, :3] = Ra
    J[:, :3, 3:] = Ra @ S
    for e in range(n):
        D = _dq_dR(Re[e])
        for a in range(3):
            J[e, 3:, 3 + a] = D @ (Ra[e] @ Sxyz[a]).T.reshape(9)         # vec column-major
    return J.transpose(0, 2, 1).reshape(n, 36).copy(), err


PRIOR_DIM = {7: 3, 8: 2, 9: 6}


def prior_type(prob):
    if prob["kind"] == "se3":
        return 9
    return 8 if prob["prior"] == "xy" else 7


def prior_edges_of(ptype, poses, vq, zq, offset=None, jac=True):
    if ptype == 7:
        return se2_prior_edges(poses, vq, zq, jac=jac)
    if ptype == 8:
        return se2_xy_prior_edges(poses, vq, zq, jac=jac)
    return se3_prior_edges(poses, vq, zq, offset, jac=jac)


def prior_edges(prob, poses=None, jac=True):
    poses = prob["poses"] if poses is None else poses
    return prior_edges_of(prior_type(prob), poses, prob["vq"], prob["zq"], prob.get("prior_offset"), jac=jac)


def oracle_prior(prob, schur=True, with_priors=True):
    """OracleSolver with sets 0 / 1 / 2 = odometry / observations / unary prior set, structure built."""
    p, l = LH.dims(prob)
    (a, b), (c, d) = LH.edge_set_indices(prob)
    o = O.OracleSolver(p, l, prob["nP"], prob["nL"], schur)
    k0 = o.add_edge_set(p, a, b)
    o.set_dims(k0, p, p)
    k1 = o.add_edge_set(l, c, d)
    o.set_dims(k1, p, l)
    if with_priors:
        k2 = o.add_edge_set(PRIOR_DIM[prior_type(prob)], np.asarray(prob["hidx"], np.int32)[prob["vq"]])
        o.set_dims(k2, p, 0)
    o.build_structure()
    return o


def feed_oracle(prob, o, huber=0.0, poses=None, points=None, kind=1):
    """Hands the NumPy / oracle producers' data of all three sets to o; huber: the kernel (delta) of the PRIOR set."""
    A0, A1, e0 = LH.pose_edges(prob, poses=poses)
    B0, B1, e1 = LH.landmark_edges(prob, poses=poses, points=points)
    Q0, eq = prior_edges(prob, poses=poses)
    o.set_edge_data(0, A0, A1, prob["omega"], e0)
    o.set_edge_data(1, B0, B1, prob["omega_l"], e1)
    o.set_edge_data(2, Q0, None, prob["omega_q"], eq, huber)
    if huber > 0 and kind != 1:
        o.set_robust_kernel(2, kind)
    return (A0, A1, e0), (B0, B1, e1), (Q0, eq)


class HostPriorGraph(LH.HostLandmarkGraph):
    """HostLandmarkGraph that also feeds the unary prior set (set 2; J1 is None)."""

    def linearize(self):
        super().linearize()
        self._Q0, eq = prior_edges(self.pr)
        self.feed(2, self._Q0, None, self.pr["omega_q"], eq)

    def compute_active_errors(self):
        super().compute_active_errors()
        eq = prior_edges(self.pr, jac=False)
        if self.feed_err is not None:
            self.feed_err(2, eq)
        else:
            self.feed(2, self._Q0, None, self.pr["omega_q"], eq)


LM_SIZE = (70, 40)
LM_PERTURB = (4.0, 1.0, 5.0)
LM_SEED = 43


def lm_prior_graph(kind):
    """The graph of the whole-run comparison: the GPU tests' size with priors on the whole pose, initial estimates perturbed
    far enough (lm_test_graph-style) that ten LM iterations have decisions to take."""
    from openslam_g2o_amd import synthetic as S
    return S.make_landmark_slam(kind, LM_SIZE[0], LM_SIZE[1], priors="pose", prior_stride=10, perturb=LM_PERTURB, seed=LM_SEED)


def oracle_lm_run(prob, iterations, dense=False):
    """lm.optimize over the oracle + the NumPy producers, prior set included.  Returns (done, chis, lams, trials, graph)."""
    from openslam_g2o_amd import lm
    o = oracle_prior(prob, True)
    g = HostPriorGraph(prob, lambda k, J0, J1, om, err: o.set_edge_data(k, J0, J1, om, err), o.x, o.chi2)
    done, chis, lams, trials = lm.optimize(g, LH.OracleLandmarkSolver(o, dense), iterations, "lm")
    return done, chis, lams, trials, g
