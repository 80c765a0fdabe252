"""Host-side Sim3 arithmetic of the reference's 7-dof types, for the generators, the file reader / writer and the tests:

  Sim3(Vector7d) (exp), log(), inverse(), operator*      g2o/types/sim3/sim3.h:70-142, 148-230, 233-236, 266-272
  VertexSim3Expmap::oplusImpl                            g2o/types/sim3/types_seven_dof_expmap.h:56-65
  EdgeSim3::computeError                                 g2o/types/sim3/types_seven_dof_expmap.h:94-102
  EdgeSim3ProjectXYZ::computeError, Sim3::map, cam_map   g2o/types/sim3/types_seven_dof_expmap.h:126-133, :70-76, sim3.h:144-146
  BaseBinaryEdge::linearizeOplus (numeric branch)        g2o/core/base_binary_edge.hpp:132-201 (delta = 1e-9, central)
  Eigen: Quaternion(Matrix3), toRotationMatrix, quaternion product, quaternion * vector, 3x3 partial-pivot LU solve

ONE body of formulas, written operation for operation in the reference's order and generic over the arithmetic F: FP64 below
(Python floats = IEEE doubles, the functions of libm); tests/sim3_helpers.py adds mpmath at 60 digits.  F supplies num(x), sin,
cos, exp, log, acos, sqrt.  Constants the reference writes as fp64 literals (eps = 0.00001, delta = 1e-9, 1./6.) enter every
arithmetic as those fp64 values.  Every data-dependent choice -- the exp branch, the log branch, the case of the rotation ->
quaternion conversion, the pivot rows of the LU -- is appended to `trace` (when given), so that a test can assert that two
arithmetics took the same path.  The device kernels (csrc/pg_sim3.inc, csrc/pg_sim3_project.inc) state the same operations in
HIP and share no code with this file.

Layouts as in the C ABI: a Sim3 is 8 doubles (qx, qy, qz, qw, tx, ty, tz, s); a minimal vector is (omega[3], upsilon[3],
sigma); Jacobian blocks are 7x7 column-major."""
import math

import numpy as np

EPS64 = 0.00001        # the literal of sim3.h
DELTA64 = 1e-9         # the literal of base_binary_edge.hpp
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


class FP64:
    name = "fp64"
    sin, cos, exp, log, acos, sqrt = math.sin, math.cos, math.exp, math.log, math.acos, math.sqrt

    @staticmethod
    def num(x):
        return float(x)



def _vec(F, x):
    return [F.num(v) for v in x]


# ------------------------------------------------------------------------------------------------ Eigen pieces
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def q_mul(a, b):
    """Quaternion product, members (x, y, z, w)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def q_rot(q, v):
    """Quaternion * vector: uv = 2 (q.vec x v); v + w uv + q.vec x uv."""
    qv = [q[0], q[1], q[2]]
    uv = _cross(qv, v)
    uv = [u + u for u in uv]
    c = _cross(qv, uv)
    return [v[i] + q[3] * uv[i] + c[i] for i in range(3)]


def q_to_R(F, q):
    x, y, z, w = q
    one = F.num(1.0)
    tx, ty, tz = x + x, y + y, z + z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[one - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, one - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, one - (txx + tyy)]]


def R_to_q(F, R, trace=None):
    half, one = F.num(0.5), F.num(1.0)
    t = R[0][0] + R[1][1] + R[2][2]
    q = [None] * 4
    if t > 0:
        case = 0
        t = F.sqrt(t + one)
        q[3] = half * t
        t = half / t
        q[0] = (R[2][1] - R[1][2]) * t
        q[1] = (R[0][2] - R[2][0]) * t
        q[2] = (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        case = 1 + i
        t = F.sqrt(R[i][i] - R[j][j] - R[k][k] + one)
        q[i] = half * t
        t = half / t
        q[3] = (R[k][j] - R[j][k]) * t
        q[j] = (R[j][i] + R[i][j]) * t
        q[k] = (R[k][i] + R[i][k]) * t
    if trace is not None:
        trace.append(("quat", case))
    return q


def _skew(F, v):
    z = F.num(0.0)
    return [[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]]


def _matmul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _lu_solve(W, b, trace=None):
    """3x3 solve by LU with partial pivoting (the largest |entry| of the column, the first one on ties)."""
    A = [list(r) for r in W]
    x = list(b)
    piv = []
    for c in range(2):
        p = c
        for r in range(c + 1, 3):
            if abs(A[r][c]) > abs(A[p][c]):
                p = r
        piv.append(p)
        if p != c:
            A[c], A[p] = A[p], A[c]
            x[c], x[p] = x[p], x[c]
        for r in range(c + 1, 3):
            f = A[r][c] / A[c][c]
            for k in range(c + 1, 3):
                A[r][k] = A[r][k] - f * A[c][k]
            x[r] = x[r] - f * x[c]
    if trace is not None:
        trace.append(("lu", tuple(piv)))
    x[2] = x[2] / A[2][2]
    x[1] = (x[1] - A[1][2] * x[2]) / A[1][1]
    x[0] = (x[0] - A[0][1] * x[1] - A[0][2] * x[2]) / A[0][0]
    return x


# ------------------------------------------------------------------------------------------------ sim3.h
def _abc(F, sigma, s, theta, small_sigma, small_theta):
    """The coefficients A, B, C of W = A Omega + B Omega^2 + C I shared by exp and log (theta = the rotation angle)."""
    one = F.num(1.0)
    if small_sigma:
        C = one
        if small_theta:
            A = F.num(1. / 2.)
            B = F.num(1. / 6.)
        else:
            theta2 = theta * theta
            A = (one - F.cos(theta)) / theta2
            B = (theta - F.sin(theta)) / (theta2 * theta)
    else:
        C = (s - one) / sigma
        if small_theta:
            sigma2 = sigma * sigma
            A = ((sigma - one) * s + one) / sigma2
            B = ((F.num(0.5) * sigma2 - sigma + one) * s) / (sigma2 * sigma)
        else:
            a = s * F.sin(theta)
            b = s * F.cos(theta)
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (one - b) * theta) / (theta * c)
            B = (C - ((b - one) * sigma + a * theta) / c) * one / theta2
    return A, B, C


def sim3_exp(F, v, trace=None):
    """Sim3(const Vector7d&): branch 0..3 = (|sigma| < eps ? 0 : 2) + (theta < eps ? 0 : 1)."""
    v = _vec(F, v)
    eps, one = F.num(EPS64), F.num(1.0)
    omega, upsilon, sigma = v[0:3], v[3:6], v[6]
    theta = F.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    Om = _skew(F, omega)
    s = F.exp(sigma)
    Om2 = _matmul(Om, Om)
    small_sigma, small_theta = abs(sigma) < eps, theta < eps
    if trace is not None:
        trace.append(("exp", (0 if small_sigma else 2) + (0 if small_theta else 1)))
    A, B, C = _abc(F, sigma, s, theta, small_sigma, small_theta)
    eye = lambda i, j: one if i == j else F.num(0.0)
    if small_theta:
        R = [[eye(i, j) + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]
    else:
        k1 = F.sin(theta) / theta
        k2 = (one - F.cos(theta)) / (theta * theta)
        R = [[eye(i, j) + k1 * Om[i][j] + k2 * Om2[i][j] for j in range(3)] for i in range(3)]
    r = R_to_q(F, R, trace)
    W = [[A * Om[i][j] + B * Om2[i][j] + C * eye(i, j) for j in range(3)] for i in range(3)]
    t = [W[i][0] * upsilon[0] + W[i][1] * upsilon[1] + W[i][2] * upsilon[2] for i in range(3)]
    return r + t + [s]


def sim3_log(F, S, trace=None):
    """Sim3::log: branch 0..3 = (|sigma| < eps ? 0 : 2) + (d > 1 - eps ? 0 : 1)."""
    S = _vec(F, S)
    eps, one, half = F.num(EPS64), F.num(1.0), F.num(0.5)
    r, t, s = S[0:4], S[4:7], S[7]
    sigma = F.log(s)
    R = q_to_R(F, r)
    d = half * (R[0][0] + R[1][1] + R[2][2] - one)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    small_sigma, small_theta = abs(sigma) < eps, d > one - eps
    if trace is not None:
        trace.append(("log", (0 if small_sigma else 2) + (0 if small_theta else 1)))
    if small_theta:
        theta = None
        omega = [half * x for x in dR]
    else:
        theta = F.acos(d)
        k = theta / (F.num(2.0) * F.sqrt(one - d * d))
        omega = [k * x for x in dR]
    Om = _skew(F, omega)
    A, B, C = _abc(F, sigma, s, theta, small_sigma, small_theta)
    BOm = [[B * Om[i][j] for j in range(3)] for i in range(3)]
    BOm2 = _matmul(BOm, Om)
    eye = lambda i, j: one if i == j else F.num(0.0)
    W = [[A * Om[i][j] + BOm2[i][j] + C * eye(i, j) for j in range(3)] for i in range(3)]
    upsilon = _lu_solve(W, t, trace)
    return omega + upsilon + [sigma]


def sim3_inverse(F, S):
    S = _vec(F, S)
    r, t, s = S[0:4], S[4:7], S[7]
    rc = [-r[0], -r[1], -r[2], r[3]]
    k = F.num(-1.0) / s
    return rc + q_rot(rc, [k * x for x in t]) + [F.num(1.0) / s]


def sim3_mul(F, a, b):
    a, b = _vec(F, a), _vec(F, b)
    rt = q_rot(a[0:4], b[4:7])
    return q_mul(a[0:4], b[0:4]) + [a[7] * rt[i] + a[4 + i] for i in range(3)] + [a[7] * b[7]]


def sim3_error(F, si, sj, z, trace=None):
    """EdgeSim3::computeError: log(C * Si * Sj^-1)."""
    return sim3_log(F, sim3_mul(F, sim3_mul(F, z, si), sim3_inverse(F, sj)), trace)


def sim3_oplus(F, S, x, fix_scale=False, trace=None):
    """VertexSim3Expmap::oplusImpl: exp(x) * S, x[6] = 0 with fix_scale."""
    x = _vec(F, x)
    if fix_scale:
        x[6] = F.num(0.0)
    return sim3_mul(F, sim3_exp(F, x, trace), S)


def sim3_jacobians(F, si, sj, z, fixed=(False, False), fix_scale=False, trace=None):
    """The numeric branch of BaseBinaryEdge::linearizeOplus.  Returns (Ji, Jj) as 7x7 row lists J[row][col]; the block of a
    fixed vertex is zero."""
    delta = F.num(DELTA64)
    scalar = F.num(1.0) / (F.num(2.0) * delta)
    zero = F.num(0.0)
    out = []
    for side in range(2):
        J = [[zero] * 7 for _ in range(7)]
        if not fixed[side]:
            for c in range(7):
                add = [zero] * 7
                add[c] = delta
                p = sim3_oplus(F, (si, sj)[side], add, fix_scale, trace)
                e1 = sim3_error(F, p if side == 0 else si, p if side == 1 else sj, z, trace)
                add[c] = -delta
                p = sim3_oplus(F, (si, sj)[side], add, fix_scale, trace)
                e2 = sim3_error(F, p if side == 0 else si, p if side == 1 else sj, z, trace)
                for r in range(7):
                    J[r][c] = scalar * (e1[r] - e2[r])
        out.append(J)
    return out


# ------------------------------------------------------------------------------------------------ EdgeSim3ProjectXYZ
def sim3_map(F, S, X):
    """Sim3::map (sim3.h:144-146): s * (r * X) + t."""
    S, X = _vec(F, S), _vec(F, X)
    rX = q_rot(S[0:4], X)
    return [S[7] * rX[i] + S[4 + i] for i in range(3)]


def project_error(F, S, X, kc, z):
    """EdgeSim3ProjectXYZ::computeError (types_seven_dof_expmap.h:126-133): z - cam_map(project(S.map(X))), project = (x / z,
    y / z), cam_map(v)[i] = v[i] * focal_length[i] + principle_point[i]; kc = (fx, fy, cx, cy) of the observing vertex."""
    m = sim3_map(F, S, X)
    kc, z = _vec(F, kc), _vec(F, z)
    u, v = m[0] / m[2], m[1] / m[2]
    return [z[0] - (u * kc[0] + kc[2]), z[1] - (v * kc[1] + kc[3])]


def project_jacobians(F, S, X, kc, z, fixed=(False, False), fix_scale=False, trace=None):
    """The numeric branch of BaseBinaryEdge::linearizeOplus for EdgeSim3ProjectXYZ (which defines no Jacobian): the pose
    perturbed through oplusImpl, the point by plain addition (VertexSBAPointXYZ::oplusImpl).  Returns (Jpose 2x7, Jpoint 2x3) as
    row lists J[row][col] -- the pose first, as in the landmark slot of the C ABI (the reference's edge has the point as vertex 0);
    fixed = (pose fixed, point fixed): the block of a fixed vertex is zero."""
    delta = F.num(DELTA64)
    scalar = F.num(1.0) / (F.num(2.0) * delta)
    zero = F.num(0.0)
    X = _vec(F, X)
    Jp = [[zero] * 7 for _ in range(2)]
    Jx = [[zero] * 3 for _ in range(2)]
    if not fixed[0]:
        for c in range(7):
            add = [zero] * 7
            add[c] = delta
            e1 = project_error(F, sim3_oplus(F, S, add, fix_scale, trace), X, kc, z)
            add[c] = -delta
            e2 = project_error(F, sim3_oplus(F, S, add, fix_scale, trace), X, kc, z)
            for r in range(2):
                Jp[r][c] = (e1[r] - e2[r]) * scalar
    if not fixed[1]:
        for c in range(3):
            e1 = project_error(F, S, [X[i] + (delta if i == c else zero) for i in range(3)], kc, z)
            e2 = project_error(F, S, [X[i] + (-delta if i == c else zero) for i in range(3)], kc, z)
            for r in range(2):
                Jx[r][c] = (e1[r] - e2[r]) * scalar
    return Jp, Jx


def project_edges(F, poses, points, vp, vl, meas, intrinsics, pose_hidx=None, pt_hidx=None, fix_scale=False, jac=True, trace=None):
    """err [n][2] and (jac) J0 [n][14] (pose, 2x7), J1 [n][6] (point, 2x3) column-major of a whole EdgeSim3ProjectXYZ list, rounded
    to fp64; intrinsics [n_poses][4] = (fx, fy, cx, cy) indexed by vp; hidx < 0 = fixed vertex."""
    n = len(vp)
    err = np.zeros((n, 2))
    J0, J1 = np.zeros((n, 14)), np.zeros((n, 6))
    for k in range(n):
        a, b = int(vp[k]), int(vl[k])
        err[k] = to_f64(project_error(F, poses[a], points[b], intrinsics[a], meas[k]))
        if jac:
            fixed = (pose_hidx is not None and pose_hidx[a] < 0, pt_hidx is not None and pt_hidx[b] < 0)
            Jp, Jx = project_jacobians(F, poses[a], points[b], intrinsics[a], meas[k], fixed, fix_scale, trace)
            J0[k] = to_f64([Jp[r][c] for c in range(7) for r in range(2)])
            J1[k] = to_f64([Jx[r][c] for c in range(3) for r in range(2)])
    return (J0, J1, err) if jac else err


# ------------------------------------------------------------------------------------------------ whole edge lists
def to_f64(x):
    return np.array([float(v) for v in x], np.float64)


def edges(F, est, vi, vj, meas, hidx=None, fix_scale=False, jac=True, trace=None):
    """err [n][7] and (jac) J0, J1 [n][49] column-major of a whole edge list, rounded to fp64; hidx[v] < 0 = fixed vertex."""
    n = len(vi)
    err = np.zeros((n, 7))
    J0, J1 = np.zeros((n, 49)), np.zeros((n, 49))
    for k in range(n):
        a, b = int(vi[k]), int(vj[k])
        err[k] = to_f64(sim3_error(F, est[a], est[b], meas[k], trace))
        if jac:
            fixed = (hidx is not None and hidx[a] < 0, hidx is not None and hidx[b] < 0)
            Ji, Jj = sim3_jacobians(F, est[a], est[b], meas[k], fixed, fix_scale, trace)
            J0[k] = to_f64([Ji[r][c] for c in range(7) for r in range(7)])
            J1[k] = to_f64([Jj[r][c] for c in range(7) for r in range(7)])
    return (J0, J1, err) if jac else err


def update(F, est, hidx, x, fix_scale=False):
    """oplus of every free vertex with its 7 entries of the solution x; fixed vertices are returned as they are."""
    out = np.array(est, np.float64).copy()
    for v in range(len(est)):
        h = int(hidx[v])
        if h >= 0:
            out[v] = to_f64(sim3_oplus(F, est[v], x[7 * h:7 * h + 7], fix_scale))
    return out


def transform(S):
    """(R, t, s) of a stored Sim3 in fp64: q and -q are the same rotation (the quaternion is used as stored, not normalised,
    as Sim3::map does through Eigen's toRotationMatrix)."""
    S = np.asarray(S, np.float64)
    return np.array(q_to_R(FP64, list(S[0:4]))), S[4:7].copy(), float(S[7])


def chi2(err, info):
    e = np.asarray(err)
    return float(np.einsum("ni,nij,nj->", e, np.asarray(info).reshape(-1, 7, 7), e))
