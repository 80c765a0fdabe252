"""Host-side arithmetic of the reference's GICP correspondence edge, for the generators, the file reader / writer and the tests:

  EdgeGICP::makeRot0 / prec0 / cov0 (and ...1)           g2o/types/icp/types_icp.h:90-158
  Edge_V_V_GICP::computeError (and the pl_pl information)  g2o/types/icp/types_icp.h:183-233
  Edge_V_V_GICP::linearizeOplus (analytic)               g2o/types/icp/types_icp.cpp:173-202
  dRidx, dRidy, dRidz                                    g2o/types/icp/types_icp.cpp:47-55
  Edge_V_V_GICP::read (information R0' diag(.01, .01, 1) R0)   g2o/types/icp/types_icp.cpp:124-160

ONE body of formulas, written operation for operation and generic over the arithmetic F, as openslam_g2o_amd/sbacam.py is: FP64
below (Python floats = IEEE doubles), tests/gicp_helpers.py adds mpmath at 60 digits.  F supplies num(x).  There is no
data-dependent branch in any of it.  The device kernel (csrc/pg_gicp.inc) states the same operations in HIP, in the same order
and without contraction to fused multiply-adds, and shares no code with this file.

Layouts as in the C ABI: a pose is an isometry [12] = R column-major | t (VertexSE3); a measurement is (pos0, pos1); vertex 0 of
an edge is the frame of pos0, vertex 1 the frame of pos1; Jacobians are 3 x 6 (columns: t, then the quaternion's x, y, z of
VertexSE3::oplusImpl), stored column-major; cov is (cov0, cov1), 3 x 3 column-major each, read by their upper triangles."""
import numpy as np

from .sim3 import FP64, _vec, to_f64  # noqa: F401

UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _rot(F, T):
    """R[i][j] and t of an isometry [12]."""
    T = _vec(F, T)
    return [[T[i + 3 * j] for j in range(3)] for i in range(3)], T[9:12]


def transformed_point(F, X0, X1, pos1):
    """p1t = X0^-1 (X1 pos1): w = R1 pos1 + t1, then R0' w + (-(R0' t0))."""
    A, t0 = _rot(F, X0)
    B, t1 = _rot(F, X1)
    p1 = _vec(F, pos1)
    w = [(B[i][0] * p1[0] + B[i][1] * p1[1] + B[i][2] * p1[2]) + t1[i] for i in range(3)]
    out = []
    for i in range(3):
        ti = -(A[0][i] * t0[0] + A[1][i] * t0[1] + A[2][i] * t0[2])
        out.append((A[0][i] * w[0] + A[1][i] * w[1] + A[2][i] * w[2]) + ti)
    return out


def error(F, X0, X1, pos0, pos1):
    """computeError: e = p1t - pos0."""
    p1t, p0 = transformed_point(F, X0, X1, pos1), _vec(F, pos0)
    return [p1t[i] - p0[i] for i in range(3)]


def relative_rotation(F, X0, X1):
    """R = R0' R1 as R[i][j]."""
    A, _ = _rot(F, X0)
    B, _ = _rot(F, X1)
    return [[A[0][i] * B[0][j] + A[1][i] * B[1][j] + A[2][i] * B[2][j] for j in range(3)] for i in range(3)]


def jacobians(F, X0, X1, pos1):
    """linearizeOplus: J0 = [-I | dRidx p1t, dRidy p1t, dRidz p1t], J1 = [R | R dRidx' pos1, R dRidy' pos1, R dRidz' pos1] with
    dRidx = [0 0 0; 0 0 2; 0 -2 0], dRidy = [0 0 -2; 0 0 0; 2 0 0], dRidz = [0 2 0; -2 0 0; 0 0 0].  Row lists J[row][col]."""
    p1t = transformed_point(F, X0, X1, pos1)
    R = relative_rotation(F, X0, X1)
    p1 = _vec(F, pos1)
    zero, one = F.num(0.0), F.num(1.0)
    a2 = [v + v for v in p1t]
    b2 = [v + v for v in p1]
    c0 = [[-one, zero, zero], [zero, -one, zero], [zero, zero, -one],
          [zero, a2[2], -a2[1]], [-a2[2], zero, a2[0]], [a2[1], -a2[0], zero]]
    c1 = [[R[i][c] for i in range(3)] for c in range(3)]
    c1.append([R[i][2] * b2[1] - R[i][1] * b2[2] for i in range(3)])
    c1.append([R[i][0] * b2[2] - R[i][2] * b2[0] for i in range(3)])
    c1.append([R[i][1] * b2[0] - R[i][0] * b2[1] for i in range(3)])
    return [[c0[c][r] for c in range(6)] for r in range(3)], [[c1[c][r] for c in range(6)] for r in range(3)]


def plane_omega(F, X0, X1, cov):
    """The pl_pl information (cov0 + R cov1 R')^-1: T = R cov1, the upper triangle of M = cov0 + T R', its cofactors over the
    determinant.  cov = (cov0, cov1) [18], read by their upper triangles.  Returns O[i][j], symmetric to the bit."""
    cov = _vec(F, cov)
    R = relative_rotation(F, X0, X1)
    c0 = [cov[i + 3 * j] for i, j in UPPER]
    u = [cov[9 + i + 3 * j] for i, j in UPPER]
    C1 = [[u[0], u[1], u[2]], [u[1], u[3], u[4]], [u[2], u[4], u[5]]]
    T = [[R[i][0] * C1[0][j] + R[i][1] * C1[1][j] + R[i][2] * C1[2][j] for j in range(3)] for i in range(3)]
    ma, mb, mc, md, me, mf = [c0[k] + (T[i][0] * R[j][0] + T[i][1] * R[j][1] + T[i][2] * R[j][2]) for k, (i, j) in enumerate(UPPER)]
    k00, k01, k02 = md * mf - me * me, mc * me - mb * mf, mb * me - mc * md
    k11, k12, k22 = ma * mf - mc * mc, mb * mc - ma * me, ma * md - mb * mb
    det = (ma * k00 + mb * k01) + mc * k02
    o00, o01, o02, o11, o12, o22 = k00 / det, k01 / det, k02 / det, k11 / det, k12 / det, k22 / det
    return [[o00, o01, o02], [o01, o11, o12], [o02, o12, o22]]


# ------------------------------------------------------------------------------------------------ whole edge lists
def gicp_edges(F, poses, vi, vj, meas, cov=None, jac=True):
    """(J0 [n][18], J1 [n][18], err [n][3], omega) of a whole edge list, rounded to fp64; jac=False: (err, omega).  omega is
    [n][9] in plane-to-plane mode (cov [n][18] given) and None otherwise.  Blocks of fixed vertices are evaluated like the others."""
    n = len(vi)
    meas = np.asarray(meas, np.float64).reshape(n, 6)
    err = np.zeros((n, 3))
    J0, J1 = np.zeros((n, 18)), np.zeros((n, 18))
    omega = None if cov is None else np.zeros((n, 9))
    if cov is not None:
        cov = np.asarray(cov, np.float64).reshape(n, 18)
    for k in range(n):
        X0, X1 = poses[int(vi[k])], poses[int(vj[k])]
        err[k] = to_f64(error(F, X0, X1, meas[k, 0:3], meas[k, 3:6]))
        if cov is not None:
            O = plane_omega(F, X0, X1, cov[k])
            omega[k] = to_f64([O[r][c] for c in range(3) for r in range(3)])
        if jac:
            A, B = jacobians(F, X0, X1, meas[k, 3:6])
            J0[k] = to_f64([A[r][c] for c in range(6) for r in range(3)])
            J1[k] = to_f64([B[r][c] for c in range(6) for r in range(3)])
    return (J0, J1, err, omega) if jac else (err, omega)


def chi2(err, omega, huber=0.0):
    """sum of rho(e' Omega e) in fp64 (rho = Huber of width `huber` on sqrt(e' Omega e), or the identity)."""
    e2 = np.einsum("ni,nij,nj->n", err, np.asarray(omega).reshape(-1, 3, 3), err)
    if huber > 0:
        big = e2 > huber * huber
        e2 = np.where(big, 2.0 * huber * np.sqrt(np.where(big, e2, 1.0)) - huber * huber, e2)
    return float(e2.sum())


# ------------------------------------------------------------------------------------------------ EdgeGICP's builders (fp64)
def make_rot(normal):
    """makeRot0 / makeRot1: rows (normal x y, y, normal) with y = (0, 1, 0) - normal[1] normal, normalised.  Like the reference
    there is no guard for a normal along (0, 1, 0)."""
    n = np.asarray(normal, np.float64)
    y = np.array([0.0, 1.0, 0.0]) - n[1] * n
    y = y / np.linalg.norm(y)
    return np.stack([np.cross(n, y), y, n])


def prec(normal, e):
    """prec0 / prec1: R' diag(e, e, 1) R, the point-to-plane information."""
    R = make_rot(normal)
    return R.T @ np.diag([e, e, 1.0]) @ R


def cov(normal, e):
    """cov0 / cov1: R' diag(1, 1, e) R, the plane-to-plane covariance."""
    R = make_rot(normal)
    return R.T @ np.diag([1.0, 1.0, e]) @ R


def read_information(normal0):
    """The information Edge_V_V_GICP::read gives an edge: R0' diag(.01, .01, 1) R0."""
    return prec(normal0, 0.01)
