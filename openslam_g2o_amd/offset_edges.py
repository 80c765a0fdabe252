"""Host-side arithmetic of the reference's sensor-offset pose-pose edges, for the generators, the file reader / writer and the tests:

  EdgeSE3Offset::computeError / linearizeOplus   g2o/types/slam3d/edge_se3_offset.cpp:100-130
  computeEdgeSE3Gradient (Pi, Pj given)          g2o/types/slam3d/isometry3d_gradients.h:86-192 (the non-__clang__ branch)
  compute_dq_dR                                  g2o/types/slam3d/dquat2mat.cpp (the partials of the four case formulas)
  CacheSE3Offset::updateImpl                     g2o/types/slam3d/parameter_se3_offset.cpp:44-50 (n2w = X P, w2n = n2w^-1)
  EdgeSE2Offset::computeError                    g2o/types/slam2d/edge_se2_offset.cpp:96-100
  CacheSE2Offset::updateImpl                     g2o/types/slam2d/parameter_se2_offset.cpp:76-86
  SE2::operator*, SE2::inverse, normalize_theta  g2o/types/slam2d/se2.h, g2o/stuff/misc.h
  BaseBinaryEdge::linearizeOplus (numeric)       g2o/core/base_binary_edge.hpp:132-201 (delta = 1e-9, central)

ONE body of formulas, written operation for operation and generic over the arithmetic F, as openslam_g2o_amd/gicp.py is: FP64
below (Python floats = IEEE doubles), the tests add mpmath at 60 digits (MP of tests/sim3_helpers).  F supplies num(x), sqrt,
sin and cos.  The device kernels (csrc/pg_offset.inc) state the same operations in HIP, in the same order, and share no code with
this file.

Type 19 = EdgeSE3Offset: e = toVectorMQT(D), D = (Z^-1 (Xi Pi)^-1) (Xj Pj), the association of computeError.  The Jacobians are
computeEdgeSE3Gradient with A = Z^-1 Pi^-1, B = Xi^-1 Xj, C = Pj; dq_dR is taken at the rotation of D, the matrix the error's
quaternion came from (the reference forms E = (A B) C a second time: the same matrix up to rounding).

Type 18 = EdgeSE2Offset: e = (D.t, D.angle), D = (Z^-1 (Xi Pi)^-1) (Xj Pj) with SE2's products and normalize_theta after every
one of them.  The reference has no analytic Jacobian and differentiates numerically; se2_jacobians is the exact derivative with
respect to VertexSE2::oplusImpl (t += u_t, theta = normalize(theta + u_theta)): with si = ti + R(thi) pi, sj = tj + R(thj) pj,
M = R(thz + thi + ai)' and J = [0 -1; 1 0]
    d e_t / d ti = -M            d e_t / d thi = -J M (sj - si) - M J R(thi) pi        d e_th / d thi = -1
    d e_t / d tj =  M            d e_t / d thj =  M J R(thj) pj                        d e_th / d thj =  1
se2_numeric_jacobians is the reference's central difference, for the comparison.

Layouts as in the C ABI: an SE3 pose, measurement or offset is an isometry [12] = R column-major | t; an SE2 one is (x, y,
theta); Jacobians are d x d, stored column-major; param_from / param_to name rows of the offsets table."""
import math

import numpy as np

from .sim3 import DELTA64, FP64, R_to_q, _vec, to_f64  # noqa: F401

ERROR_DIM = {18: 3, 19: 6}
STRIDE = {18: 3, 19: 12}
POSE_TYPE = {18: 1, 19: 2}
KIND_TYPE = {"se2": 18, "se3": 19}
M_PI = math.pi


# ------------------------------------------------------------------------------------------------ isometries (type 19)
def _iso(F, T):
    """(R[i][j], t) of an isometry [12]."""
    T = _vec(F, T)
    return [[T[i + 3 * j] for j in range(3)] for i in range(3)], T[9:12]


def iso_mul(F, A, B):
    """A B: R[r][c] = ((0 + A[r][0] B[0][c]) + A[r][1] B[1][c]) + A[r][2] B[2][c]; t[r] = A[r][:] tB (left to right) + tA[r]."""
    (Ra, ta), (Rb, tb) = A, B
    R = [[None] * 3 for _ in range(3)]
    for c in range(3):
        for r in range(3):
            s = F.num(0.0)
            for m in range(3):
                s = s + Ra[r][m] * Rb[m][c]
            R[r][c] = s
    t = [Ra[r][0] * tb[0] + Ra[r][1] * tb[1] + Ra[r][2] * tb[2] + ta[r] for r in range(3)]
    return R, t


def iso_inv(F, A):
    """A^-1 = (R', -(R' t))."""
    Ra, ta = A
    R = [[Ra[c][r] for c in range(3)] for r in range(3)]
    return R, [-(R[r][0] * ta[0] + R[r][1] * ta[1] + R[r][2] * ta[2]) for r in range(3)]


def unit_quat(F, R):
    """Quaterniond(R) (Eigen's four cases), normalised, w >= 0 (toVectorMQT): (x, y, z, w)."""
    q = R_to_q(F, R)
    nrm = F.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    q = [v / nrm for v in q]
    return [-v for v in q] if q[3] < 0 else q


def dq_dR(F, R):
    """d(qx, qy, qz) / d vec(R), 3 x 9 with vec column-major, D[row][col]: the partials of the case formulas, negated where the
    case's qw is <= 0 (the error's quaternion is flipped to w >= 0)."""
    zero, one, half, quarter = F.num(0.0), F.num(1.0), F.num(0.5), F.num(0.25)
    D = [[zero] * 9 for _ in range(3)]
    col = lambda a, b: a + 3 * b
    tr = R[0][0] + R[1][1] + R[2][2]
    if tr > 0:
        w = half * F.sqrt(tr + one)
        qw = w
        num = (R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1])
        pa, pb = (2, 0, 1), (1, 2, 0)
        for c in range(3):
            dd = -num[c] / (F.num(32.0) * w * w * w)
            D[c][col(0, 0)] = D[c][col(1, 1)] = D[c][col(2, 2)] = dd
            D[c][col(pa[c], pb[c])] = quarter / w
            D[c][col(pb[c], pa[c])] = -(quarter / w)
    else:
        if R[0][0] > R[1][1] and R[0][0] > R[2][2]:
            i = 0
        elif R[1][1] > R[2][2]:
            i = 1
        else:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = half * F.sqrt(one + R[i][i] - R[j][j] - R[k][k])
        qw = (R[k][j] - R[j][k]) / (F.num(4.0) * s)
        e8 = one / (F.num(8.0) * s)
        D[i][col(i, i)] = e8
        D[i][col(j, j)] = -e8
        D[i][col(k, k)] = -e8
        for c in (j, k):
            num = R[c][i] + R[i][c]
            D[c][col(c, i)] = D[c][col(c, i)] + quarter / s
            D[c][col(i, c)] = D[c][col(i, c)] + quarter / s
            dd = num / (F.num(32.0) * s * s * s)
            D[c][col(i, i)] = D[c][col(i, i)] + (-dd)
            D[c][col(j, j)] = D[c][col(j, j)] + dd
            D[c][col(k, k)] = D[c][col(k, k)] + dd
    if qw <= 0:
        D = [[-v for v in row] for row in D]
    return D


def quat_case(F, R):
    """(case, sign) of unit_quat / dq_dR at R: case 0 (trace > 0) or 1 + index of the largest diagonal entry; sign +1 / -1 for a
    case qw > 0 / <= 0."""
    tr = R[0][0] + R[1][1] + R[2][2]
    if tr > 0:
        return 0, 1
    if R[0][0] > R[1][1] and R[0][0] > R[2][2]:
        i = 0
    elif R[1][1] > R[2][2]:
        i = 1
    else:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = F.num(0.5) * F.sqrt(F.num(1.0) + R[i][i] - R[j][j] - R[k][k])
    qw = (R[k][j] - R[j][k]) / (F.num(4.0) * s)
    return 1 + i, (1 if qw > 0 else -1)


def se3_delta(F, Xi, Xj, Z, Pi, Pj):
    """D = (Z^-1 (Xi Pi)^-1) (Xj Pj), isometries as (R, t)."""
    Zi = iso_inv(F, _iso(F, Z))
    w2n = iso_inv(F, iso_mul(F, _iso(F, Xi), _iso(F, Pi)))
    n2w = iso_mul(F, _iso(F, Xj), _iso(F, Pj))
    return iso_mul(F, iso_mul(F, Zi, w2n), n2w)


def se3_error(F, Xi, Xj, Z, Pi, Pj):
    """toVectorMQT(D): translation, then the vector part of the unit quaternion with w >= 0."""
    R, t = se3_delta(F, Xi, Xj, Z, Pi, Pj)
    return list(t) + unit_quat(F, R)[:3]


def _mat3(F, A, S):
    """A S, each entry ((0 + a0 s0) + a1 s1) + a2 s2."""
    out = [[None] * 3 for _ in range(3)]
    for c in range(3):
        for r in range(3):
            s = F.num(0.0)
            for m in range(3):
                s = s + A[r][m] * S[m][c]
            out[r][c] = s
    return out


def se3_jacobians(F, Xi, Xj, Z, Pi, Pj):
    """computeEdgeSE3Gradient: (Ji, Jj) as row lists J[row][col], 6 x 6."""
    zero = F.num(0.0)
    Re, _ = se3_delta(F, Xi, Xj, Z, Pi, Pj)
    C = _iso(F, Pj)
    A = iso_mul(F, iso_inv(F, _iso(F, Z)), iso_inv(F, _iso(F, Pi)))
    B = iso_mul(F, iso_inv(F, _iso(F, Xi)), _iso(F, Xj))
    AB, BC = iso_mul(F, A, B), iso_mul(F, B, C)
    Ra, Rab, (Rbc, tbc), (Rc, tc) = A[0], AB[0], BC, C
    D = dq_dR(F, Re)
    Ji = [[zero] * 6 for _ in range(6)]
    Jj = [[zero] * 6 for _ in range(6)]
    for r in range(3):
        for c in range(3):
            Ji[r][c] = -Ra[r][c]
            Jj[r][c] = Rab[r][c]
    x, y, z = (F.num(2.0) * v for v in tbc)
    T = _mat3(F, Ra, [[zero, -z, y], [z, zero, -x], [-y, x, zero]])            # dte/dqi = Ra skewT(tbc)
    x, y, z = (F.num(2.0) * v for v in tc)
    U = _mat3(F, Rab, [[zero, z, -y], [-z, zero, x], [y, -x, zero]])           # dte/dqj = Rab skew(tc)
    for r in range(3):
        for c in range(3):
            Ji[r][3 + c] = T[r][c]
            Jj[r][3 + c] = U[r][c]
    r2 = [[F.num(2.0) * Rbc[i][j] for j in range(3)] for i in range(3)]
    neg = lambda v: [-a for a in v]
    z3 = [zero, zero, zero]
    St = ([z3, r2[2], neg(r2[1])], [neg(r2[2]), z3, r2[0]], [r2[1], neg(r2[0]), z3])      # skewT(Sx, Sy, Sz, Rbc)
    c2 = [[F.num(2.0) * Rc[i][j] for j in range(3)] for i in range(3)]
    Sk = ([z3, neg(c2[2]), c2[1]], [c2[2], z3, neg(c2[0])], [neg(c2[1]), c2[0], z3])      # skew(Sx, Sy, Sz, Rc)
    for a in range(3):
        for J, L, S in ((Ji, Ra, St[a]), (Jj, Rab, Sk[a])):
            M = _mat3(F, L, S)
            for r in range(3):
                s = zero
                for m in range(9):
                    s = s + D[r][m] * M[m % 3][m // 3]                     # vec column-major
                J[3 + r][3 + a] = s
    return Ji, Jj


# ------------------------------------------------------------------------------------------------ SE2 (type 18)
def normalize_theta(F, theta):
    """normalize_theta (g2o/stuff/misc.h) into [-pi, pi), M_PI the double."""
    pi = F.num(M_PI)
    if theta >= -pi and theta < pi:
        return theta
    two = F.num(2.0)
    multiplier = F.num(math.floor(float(theta / (two * pi))))
    theta = theta - multiplier * two * pi
    if theta >= pi:
        theta = theta - two * pi
    if theta < -pi:
        theta = theta + two * pi
    return theta


def se2_inverse(F, a):
    th = normalize_theta(F, -a[2])
    c, s = F.cos(th), F.sin(th)
    return [c * (-a[0]) - s * (-a[1]), s * (-a[0]) + c * (-a[1]), th]


def se2_mul(F, a, b):
    c, s = F.cos(a[2]), F.sin(a[2])
    return [a[0] + c * b[0] - s * b[1], a[1] + s * b[0] + c * b[1], normalize_theta(F, a[2] + b[2])]


def _se2_chain(F, Xi, Xj, Z, Pi, Pj):
    """(T = Z^-1 (Xi Pi)^-1, D = T (Xj Pj))."""
    Xi, Xj, Z, Pi, Pj = (_vec(F, v) for v in (Xi, Xj, Z, Pi, Pj))
    invm = se2_inverse(F, Z)
    w2n = se2_inverse(F, se2_mul(F, Xi, Pi))
    n2w = se2_mul(F, Xj, Pj)
    T = se2_mul(F, invm, w2n)
    return T, se2_mul(F, T, n2w)


def se2_error(F, Xi, Xj, Z, Pi, Pj):
    return _se2_chain(F, Xi, Xj, Z, Pi, Pj)[1]


def se2_jacobians(F, Xi, Xj, Z, Pi, Pj):
    """The exact derivative (module docstring): (Ji, Jj) as row lists J[row][col], 3 x 3.  M = R(angle of Z^-1 (Xi Pi)^-1)."""
    T, _ = _se2_chain(F, Xi, Xj, Z, Pi, Pj)
    Xi, Xj, Pi, Pj = (_vec(F, v) for v in (Xi, Xj, Pi, Pj))
    zero, one = F.num(0.0), F.num(1.0)
    cm, sm = F.cos(T[2]), F.sin(T[2])
    ci, si = F.cos(Xi[2]), F.sin(Xi[2])
    cj, sj = F.cos(Xj[2]), F.sin(Xj[2])
    rpi = (ci * Pi[0] - si * Pi[1], si * Pi[0] + ci * Pi[1])
    rpj = (cj * Pj[0] - sj * Pj[1], sj * Pj[0] + cj * Pj[1])
    dx, dy = (Xj[0] + rpj[0]) - (Xi[0] + rpi[0]), (Xj[1] + rpj[1]) - (Xi[1] + rpi[1])
    a0, a1 = -rpi[1], rpi[0]                                   # J R(thi) pi
    b0, b1 = -rpj[1], rpj[0]                                   # J R(thj) pj
    jmd0, jmd1 = -(sm * dx) - cm * dy, cm * dx - sm * dy       # J M (sj - si)
    ma0, ma1 = cm * a0 - sm * a1, sm * a0 + cm * a1
    mb0, mb1 = cm * b0 - sm * b1, sm * b0 + cm * b1
    Ji = [[-cm, sm, -jmd0 - ma0], [-sm, -cm, -jmd1 - ma1], [zero, zero, -one]]
    Jj = [[cm, -sm, mb0], [sm, cm, mb1], [zero, zero, one]]
    return Ji, Jj


def se2_oplus(F, X, u):
    """VertexSE2::oplusImpl: t += u_t, theta = normalize_theta(theta + u_theta)."""
    X = _vec(F, X)
    return [X[0] + u[0], X[1] + u[1], normalize_theta(F, X[2] + u[2])]


def se2_numeric_jacobians(F, Xi, Xj, Z, Pi, Pj, delta=DELTA64):
    """BaseBinaryEdge::linearizeOplus: per vertex and column d, (e(x [+] delta e_d) - e(x [+] -delta e_d)) * (1 / (2 delta))."""
    delta = F.num(delta)
    scalar = F.num(1.0) / (F.num(2.0) * delta)
    zero = F.num(0.0)
    out = []
    for side in (0, 1):
        J = [[None] * 3 for _ in range(3)]
        for d in range(3):
            e = []
            for sgn in (delta, -delta):
                u = [zero, zero, zero]
                u[d] = sgn
                Yi = se2_oplus(F, Xi, u) if side == 0 else Xi
                Yj = se2_oplus(F, Xj, u) if side == 1 else Xj
                e.append(se2_error(F, Yi, Yj, Z, Pi, Pj))
            for r in range(3):
                J[r][d] = scalar * (e[0][r] - e[1][r])
        out.append(J)
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------ whole edge lists
def offset_edges(F, edge_type, poses, vi, vj, pfrom, pto, meas, offsets, jac=True):
    """(J0 [n][d d], J1 [n][d d], err [n][d]) of a whole edge list, rounded to fp64; jac=False: err alone.  edge_type 18 / 19.
    Blocks of fixed vertices are evaluated like the others."""
    d, ms = ERROR_DIM[edge_type], STRIDE[edge_type]
    n = len(vi)
    poses = np.asarray(poses, np.float64).reshape(-1, ms)
    meas = np.asarray(meas, np.float64).reshape(n, ms)
    offsets = np.asarray(offsets, np.float64).reshape(-1, ms)
    err_f, jac_f = (se2_error, se2_jacobians) if edge_type == 18 else (se3_error, se3_jacobians)
    err, J0, J1 = np.zeros((n, d)), np.zeros((n, d * d)), np.zeros((n, d * d))
    for k in range(n):
        args = (poses[int(vi[k])], poses[int(vj[k])], meas[k], offsets[int(pfrom[k])], offsets[int(pto[k])])
        err[k] = to_f64(err_f(F, *args))
        if jac:
            A, B = jac_f(F, *args)
            J0[k] = to_f64([A[r][c] for c in range(d) for r in range(d)])
            J1[k] = to_f64([B[r][c] for c in range(d) for r in range(d)])
    return (J0, J1, err) if jac else err


def numeric_edges(F, poses, vi, vj, pfrom, pto, meas, offsets, delta=DELTA64):
    """(J0, J1) [n][9] of a type-18 edge list by the reference's central difference, NOT rounded (F's numbers as floats where F is
    FP64, mpmath numbers otherwise), column-major."""
    poses, meas, offsets = (np.asarray(a, np.float64).reshape(-1, 3) for a in (poses, meas, offsets))
    J0, J1 = [], []
    for k in range(len(vi)):
        A, B = se2_numeric_jacobians(F, poses[int(vi[k])], poses[int(vj[k])], meas[k], offsets[int(pfrom[k])], offsets[int(pto[k])], delta)
        J0.append([A[r][c] for c in range(3) for r in range(3)])
        J1.append([B[r][c] for c in range(3) for r in range(3)])
    return J0, J1


def chi2(err, omega, huber=0.0):
    """sum of rho(e' Omega e) in fp64 (rho = Huber of width `huber` on sqrt(e' Omega e), or the identity)."""
    err = np.asarray(err, np.float64)
    d = err.shape[1]
    e2 = np.einsum("ni,nij,nj->n", err, np.asarray(omega, np.float64).reshape(-1, d, d), err)
    if huber > 0:
        big = e2 > huber * huber
        e2 = np.where(big, 2.0 * huber * np.sqrt(np.where(big, e2, 1.0)) - huber * huber, e2)
    return float(e2.sum())


# ------------------------------------------------------------------------------------------------ fp64 helpers of the generators
def se3_compose(A, B):
    """A B of isometries [12], fp64."""
    R, t = iso_mul(FP64, _iso(FP64, A), _iso(FP64, B))
    return np.array([R[i][j] for j in range(3) for i in range(3)] + list(t))


def se3_invert(A):
    R, t = iso_inv(FP64, _iso(FP64, A))
    return np.array([R[i][j] for j in range(3) for i in range(3)] + list(t))


def se2_compose(a, b):
    return np.array(se2_mul(FP64, _vec(FP64, a), _vec(FP64, b)))


def se2_invert(a):
    return np.array(se2_inverse(FP64, _vec(FP64, a)))
