"""Host-side arithmetic of the reference's stereo observation of a 3-D point from a VertexSCam camera, for the generators and the
tests:

  VertexSCam::mapPoint / setKcam / setAll          g2o/types/icp/types_icp.h:253-366 (mapPoint :346-361)
  Edge_XYZ_VSC::computeError                       g2o/types/icp/types_icp.h:376-413
  VertexSE3::oplusImpl                             X <- X * fromVectorMQT(u)   (g2o/types/slam3d/vertex_se3.h, isometry3d_mappings.h)
  VertexSBAPointXYZ::oplusImpl                     plain addition
  BaseBinaryEdge::linearizeOplus (numeric)         g2o/core/base_binary_edge.hpp:132-201 (delta = 1e-9, central)

ONE body of formulas, written operation for operation and generic over the arithmetic F, as openslam_g2o_amd/bearing.py is: FP64
below (Python floats = IEEE doubles), the tests add mpmath at 60 digits (MP of tests/sim3_helpers).  F supplies num(x) and sqrt.
The device kernel (csrc/pg_scam.inc) states the same operations in HIP, in the same order, and shares no code with this file.

With the camera pose X = (R, t), camera-to-world as VertexSE3 holds it (an isometry [12] = R column-major | t), the point l and
kcam = (fx, fy, cx, cy, b) -- ONE for all cameras, VertexSCam::Kcam and VertexSCam::baseline are static members:
    d = l - t        q_r = R(0,r) d0 + R(1,r) d1 + R(2,r) d2        (q = R' (l - t), the point in the camera frame)
    mapPoint = ( fx q0 / q2 + cx,  fy q1 / q2 + cy,  fx (q0 - b) / q2 + cx )        e = mapPoint - z,  z = (u_left, v_left, u_right)
The reference differentiates this edge numerically (SCAM_ANALYTIC_JACOBIANS is commented out, types_icp.h:31); the analytic code
under that macro (types_icp.cpp:242-321) belongs to an older parametrisation with world-frame translation and is not the
derivative through VertexSE3::oplusImpl.  scam_jacobians is the exact derivative through that oplus: with h a column of
[-I | 2 [q]x | R'] (3 x 9: the six pose columns, then the three point columns) the output column is
    ( fx (h0 q2 - q0 h2) / q2^2,  fy (h1 q2 - q1 h2) / q2^2,  fx (h0 q2 - (q0 - b) h2) / q2^2 )
numeric_jacobians is the reference's central difference, for the comparison.  Neither has a guard for q2 <= 0.

Layouts as in the C ABI, with vertex 0 the camera and vertex 1 the point (the reference's edge has them the other way round):
J0 [n][3 x 6], J1 [n][3 x 3] column-major, err [n][3]; vp / vl index the pose and the point table."""
import numpy as np

from .sim3 import DELTA64, FP64, _vec, q_to_R, to_f64  # noqa: F401

EDGE_TYPE = 23


def camera_point(F, X, L):
    """q = R' (l - t): the point in the camera frame."""
    X, L = _vec(F, X), _vec(F, L)
    d = [L[0] - X[9], L[1] - X[10], L[2] - X[11]]
    return [X[3 * r] * d[0] + X[3 * r + 1] * d[1] + X[3 * r + 2] * d[2] for r in range(3)]


def map_point(F, X, L, kcam):
    """VertexSCam::mapPoint: (u_left, v_left, u_right)."""
    fx, fy, cx, cy, b = _vec(F, kcam)
    q = camera_point(F, X, L)
    qb = q[0] - b
    return [fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy, fx * qb / q[2] + cx]


def scam_error(F, X, L, kcam, z):
    z = _vec(F, z)
    m = map_point(F, X, L, kcam)
    return [m[i] - z[i] for i in range(3)]


def scam_jacobians(F, X, L, kcam):
    """The exact derivative (module docstring): (J0 [18], J1 [9]), column-major."""
    X = _vec(F, X)
    fx, fy, cx, cy, b = _vec(F, kcam)
    q = camera_point(F, X, L)
    qb = q[0] - b
    zero, two = F.num(0.0), F.num(2.0)
    cols = [[-F.num(1.0), zero, zero], [zero, -F.num(1.0), zero], [zero, zero, -F.num(1.0)],
            [zero, two * q[2], -(two * q[1])], [-(two * q[2]), zero, two * q[0]], [two * q[1], -(two * q[0]), zero],
            [X[0], X[3], X[6]], [X[1], X[4], X[7]], [X[2], X[5], X[8]]]
    q22 = q[2] * q[2]
    out = []
    for h in cols:
        out += [fx * (h[0] * q[2] - q[0] * h[2]) / q22, fy * (h[1] * q[2] - q[1] * h[2]) / q22, fx * (h[0] * q[2] - qb * h[2]) / q22]
    return out[:18], out[18:]


def se3_oplus(F, X, u):
    """VertexSE3::oplusImpl: X * fromVectorMQT(u), u = (t, qx, qy, qz), w = sqrt(1 - |q|^2) (the identity rotation when that is
    negative, as fromCompactQuaternion has it)."""
    X, u = _vec(F, X), _vec(F, u)
    one = F.num(1.0)
    w = one - (u[3] * u[3] + u[4] * u[4] + u[5] * u[5])
    if w < 0:
        S = [[one if i == j else F.num(0.0) for j in range(3)] for i in range(3)]
    else:
        S = q_to_R(F, [u[3], u[4], u[5], F.sqrt(w)])
    R = [[X[3 * c + r] for c in range(3)] for r in range(3)]
    out = [None] * 12
    for c in range(3):
        for r in range(3):
            out[3 * c + r] = R[r][0] * S[0][c] + R[r][1] * S[1][c] + R[r][2] * S[2][c]
    for r in range(3):
        out[9 + r] = R[r][0] * u[0] + R[r][1] * u[1] + R[r][2] * u[2] + X[9 + r]
    return out


def numeric_jacobians(F, X, L, kcam, z, delta=DELTA64):
    """BaseBinaryEdge::linearizeOplus: per vertex and column d, (e(x [+] delta e_d) - e(x [+] -delta e_d)) * (1 / (2 delta)); the
    camera through se3_oplus, the point by plain addition.  (J0 [18], J1 [9]), column-major."""
    delta = F.num(delta)
    scalar = F.num(1.0) / (F.num(2.0) * delta)
    zero = F.num(0.0)
    L = _vec(F, L)
    J0, J1 = [], []
    for d in range(6):
        e = []
        for sgn in (delta, -delta):
            u = [zero] * 6
            u[d] = sgn
            e.append(scam_error(F, se3_oplus(F, X, u), L, kcam, z))
        J0 += [scalar * (e[0][i] - e[1][i]) for i in range(3)]
    for d in range(3):
        e = []
        for sgn in (delta, -delta):
            Y = list(L)
            Y[d] = Y[d] + sgn
            e.append(scam_error(F, X, Y, kcam, z))
        J1 += [scalar * (e[0][i] - e[1][i]) for i in range(3)]
    return J0, J1


# ------------------------------------------------------------------------------------------------ whole edge lists
def scam_edges(F, poses, points, vp, vl, meas, kcam, jac=True):
    """(J0 [n][18], J1 [n][9], err [n][3]) of a whole edge list, rounded to fp64; jac=False: err alone.  Blocks of fixed vertices
    are evaluated like the others."""
    n = len(vp)
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    meas = np.asarray(meas, np.float64).reshape(n, 3)
    err, J0, J1 = np.zeros((n, 3)), np.zeros((n, 18)), np.zeros((n, 9))
    for k in range(n):
        X, L = poses[int(vp[k])], points[int(vl[k])]
        err[k] = to_f64(scam_error(F, X, L, kcam, meas[k]))
        if jac:
            A, B = scam_jacobians(F, X, L, kcam)
            J0[k] = to_f64(A)
            J1[k] = to_f64(B)
    return (J0, J1, err) if jac else err


def scam_edges_numpy(poses, points, vp, vl, meas, kcam, jac=True):
    """scam_edges(FP64, ...) over whole arrays: the same operations in the same order on every edge, so the same bits."""
    vp, vl = np.asarray(vp, np.int64), np.asarray(vl, np.int64)
    n = len(vp)
    X = np.asarray(poses, np.float64).reshape(-1, 12)[vp]
    L = np.asarray(points, np.float64).reshape(-1, 3)[vl]
    z = np.asarray(meas, np.float64).reshape(n, 3)
    fx, fy, cx, cy, b = (float(v) for v in kcam)
    d = [L[:, i] - X[:, 9 + i] for i in range(3)]
    q = [X[:, 3 * r] * d[0] + X[:, 3 * r + 1] * d[1] + X[:, 3 * r + 2] * d[2] for r in range(3)]
    qb = q[0] - b
    with np.errstate(all="ignore"):
        err = np.stack([fx * q[0] / q[2] + cx - z[:, 0], fy * q[1] / q[2] + cy - z[:, 1], fx * qb / q[2] + cx - z[:, 2]], axis=1)
        if not jac:
            return err
        zero, one = np.zeros(n), np.ones(n)
        cols = [[-one, zero, zero], [zero, -one, zero], [zero, zero, -one],
                [zero, 2.0 * q[2], -(2.0 * q[1])], [-(2.0 * q[2]), zero, 2.0 * q[0]], [2.0 * q[1], -(2.0 * q[0]), zero],
                [X[:, 0], X[:, 3], X[:, 6]], [X[:, 1], X[:, 4], X[:, 7]], [X[:, 2], X[:, 5], X[:, 8]]]
        q22 = q[2] * q[2]
        out = []
        for h in cols:
            out += [fx * (h[0] * q[2] - q[0] * h[2]) / q22, fy * (h[1] * q[2] - q[1] * h[2]) / q22, fx * (h[0] * q[2] - qb * h[2]) / q22]
    J = np.stack(out, axis=1)
    return np.ascontiguousarray(J[:, :18]), np.ascontiguousarray(J[:, 18:]), err


def numeric_edges(F, poses, points, vp, vl, meas, kcam, delta=DELTA64):
    """(J0 [n][18], J1 [n][9]) by the reference's central difference, NOT rounded (F's numbers as floats where F is FP64, mpmath
    numbers otherwise)."""
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    meas = np.asarray(meas, np.float64).reshape(-1, 3)
    J0, J1 = [], []
    for k in range(len(vp)):
        A, B = numeric_jacobians(F, poses[int(vp[k])], points[int(vl[k])], kcam, meas[k], delta)
        J0.append(A)
        J1.append(B)
    return J0, J1


def chi2(err, omega, huber=0.0):
    """sum of rho(e' omega e) in fp64 (rho = Huber of width `huber` on sqrt(e' omega e), or the identity)."""
    err = np.asarray(err, np.float64).reshape(-1, 3)
    e2 = np.einsum("ni,nij,nj->n", err, np.asarray(omega, np.float64).reshape(-1, 3, 3), err)
    if huber > 0:
        big = e2 > huber * huber
        e2 = np.where(big, 2.0 * huber * np.sqrt(np.where(big, e2, 1.0)) - huber * huber, e2)
    return float(e2.sum())
