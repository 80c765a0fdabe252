"""Host-side arithmetic of the reference's landmark self-calibration edge, for the generators, the file reader / writer and the
tests:

  EdgeSE2PointXYCalib::computeError                   g2o/types/slam2d/edge_se2_pointxy_calib.h:46-52
  SE2::operator*, SE2::inverse, normalize_theta       g2o/types/slam2d/se2.h, g2o/stuff/misc.h
  VertexSE2::oplusImpl                                t += u[0:2], theta = normalize_theta(theta + u[2])
  VertexPointXY::oplusImpl                            plain addition
  BaseMultiEdge::linearizeOplus (numeric)             g2o/core/base_multi_edge.hpp:63-116 (delta = 1e-9, central)

ONE body of formulas, written operation for operation and generic over the arithmetic F, as openslam_g2o_amd/sensor_calib.py is:
FP64 below (Python floats = IEEE doubles), the tests add mpmath at 60 digits (MP of tests/sim3_helpers).  F supplies num(x), sin and
cos.  The device kernel (csrc/pg_pointxy_calib.inc) states the same operations in HIP, in the same order, and shares no code with
this file.

A three-vertex edge over the pose x1 = (t1, th1), the landmark l = (lx, ly) and the sensor's mounting offset c = (tc, thc), a
VertexSE2; z the measured landmark position in the sensor frame:
    a = x1 c    w = a^-1    e = R(w.th) l + w.t - z
with SE2's product and inverse and normalize_theta in both.  The reference has no analytic Jacobian and differentiates
numerically; pointxy_calib_jacobians is the exact derivative with respect to the two oplusImpl: with Q = R(-(th1 + thc)) (its
angle taken as w.th), J = [0 -1; 1 0], d = l - t1 - R(th1) tc
    d e / d t1 = -Q          d e / d th1 = -J Q d - Q J R(th1) tc        (J_pose  2 x 3)
    d e / d l  =  Q                                                      (J_point 2 x 2)
    d e / d tc = -R(-thc)    d e / d thc = -J Q d                        (J_calib 2 x 3)
numeric_jacobians is the reference's central difference, for the comparison.

Layouts as in the C ABI: poses and the offset are (x, y, theta), landmarks and measurements (x, y); Jacobians are stored
column-major; vp / vc index the pose table, vl the landmark table."""
import numpy as np

from .offset_edges import normalize_theta, se2_inverse, se2_mul, se2_oplus  # noqa: F401
from .sim3 import DELTA64, FP64, _vec, to_f64  # noqa: F401

EDGE_TYPE = 24


def _chain(F, X1, L, C, Z):
    """(w, cq, sq, e) of the chain above."""
    X1, L, C, Z = (_vec(F, v) for v in (X1, L, C, Z))
    a = se2_mul(F, X1, C)
    w = se2_inverse(F, a)
    cq, sq = F.cos(w[2]), F.sin(w[2])
    e = [(cq * L[0] - sq * L[1]) + w[0] - Z[0], (sq * L[0] + cq * L[1]) + w[1] - Z[1]]
    return w, cq, sq, e


def pointxy_calib_error(F, X1, L, C, Z):
    return _chain(F, X1, L, C, Z)[3]


def pointxy_calib_jacobians(F, X1, L, C, Z):
    """The exact derivative (module docstring): (Jp 2 x 3, Jl 2 x 2, Jc 2 x 3) as row lists J[row][col]."""
    _, cq, sq, _ = _chain(F, X1, L, C, Z)
    X1, L, C = (_vec(F, v) for v in (X1, L, C))
    c1, s1 = F.cos(X1[2]), F.sin(X1[2])
    cc, sc = F.cos(C[2]), F.sin(C[2])
    r10, r11 = c1 * C[0] - s1 * C[1], s1 * C[0] + c1 * C[1]                 # R(th1) tc
    dx, dy = (L[0] - X1[0]) - r10, (L[1] - X1[1]) - r11                     # d
    jqd0, jqd1 = -(sq * dx) - cq * dy, cq * dx - sq * dy                    # J Q d
    a0, a1 = -r11, r10                                                      # J R(th1) tc
    qa0, qa1 = cq * a0 - sq * a1, sq * a0 + cq * a1
    Jp = [[-cq, sq, -jqd0 - qa0], [-sq, -cq, -jqd1 - qa1]]
    Jl = [[cq, -sq], [sq, cq]]
    Jc = [[-cc, -sc, -jqd0], [sc, -cc, -jqd1]]
    return Jp, Jl, Jc


def numeric_jacobians(F, X1, L, C, Z, delta=DELTA64):
    """BaseMultiEdge::linearizeOplus: per vertex and column d, (e(x [+] delta e_d) - e(x [+] -delta e_d)) * (1 / (2 delta))."""
    delta = F.num(delta)
    scalar = F.num(1.0) / (F.num(2.0) * delta)
    zero = F.num(0.0)
    out = []
    for side, dim in ((0, 3), (1, 2), (2, 3)):
        Jm = [[None] * dim for _ in range(2)]
        for d in range(dim):
            e = []
            for sgn in (delta, -delta):
                u = [zero] * dim
                u[d] = sgn
                V = [_vec(F, X1), _vec(F, L), _vec(F, C)]
                V[side] = se2_oplus(F, V[side], u) if dim == 3 else [V[side][0] + u[0], V[side][1] + u[1]]
                e.append(pointxy_calib_error(F, V[0], V[1], V[2], Z))
            for r in range(2):
                Jm[r][d] = scalar * (e[0][r] - e[1][r])
        out.append(Jm)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ whole edge lists
def _cm(Jm):
    return [Jm[r][c] for c in range(len(Jm[0])) for r in range(len(Jm))]


def pointxy_calib_edges(F, poses, points, vp, vl, vc, meas, hidx=None, hidx_l=None, jac=True):
    """(Jp [n][6], Jl [n][4], Jc [n][6], err [n][2]) of a whole edge list, rounded to fp64; jac=False: err alone.  hidx / hidx_l
    given: the Jacobian block of a fixed vertex (hidx == -1) is zero, as the device writes it."""
    n = len(vp)
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    meas = np.asarray(meas, np.float64).reshape(n, 2)
    err, J = np.zeros((n, 2)), [np.zeros((n, 6)), np.zeros((n, 4)), np.zeros((n, 6))]
    for k in range(n):
        v = (int(vp[k]), int(vl[k]), int(vc[k]))
        args = (poses[v[0]], points[v[1]], poses[v[2]], meas[k])
        err[k] = to_f64(pointxy_calib_error(F, *args))
        if jac:
            free = (hidx is None or hidx[v[0]] >= 0, hidx_l is None or hidx_l[v[1]] >= 0, hidx is None or hidx[v[2]] >= 0)
            for side, Jm in enumerate(pointxy_calib_jacobians(F, *args)):
                if free[side]:
                    J[side][k] = to_f64(_cm(Jm))
    return (J[0], J[1], J[2], err) if jac else err


def numeric_edges(F, poses, points, vp, vl, vc, meas, delta=DELTA64):
    """(Jp, Jl, Jc) [n][6 | 4 | 6] by the reference's central difference with step `delta`, NOT rounded (F's numbers as floats
    where F is FP64, mpmath numbers otherwise), column-major."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    meas = np.asarray(meas, np.float64).reshape(-1, 2)
    out = ([], [], [])
    for k in range(len(vp)):
        Js = numeric_jacobians(F, poses[int(vp[k])], points[int(vl[k])], poses[int(vc[k])], meas[k], delta)
        for side in range(3):
            out[side].append(_cm(Js[side]))
    return out


def predict(X1, L, C):
    """The noise-free measurement (x1 c)^-1 l, fp64."""
    return np.array(pointxy_calib_error(FP64, X1, L, C, (0.0, 0.0)))


from .offset_edges import chi2  # noqa: E402,F401  (sum of rho(e' Omega e), Huber or none)
