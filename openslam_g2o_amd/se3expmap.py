"""Host-side arithmetic of the reference's pose-pose constraint between two VertexSE3Expmap, for the generators, the file
reader / writer, the host-fed baseline of tools/ba_pose_edges_time.py and the tests:

  EdgeSE3Expmap::computeError     g2o/types/sba/types_six_dof_expmap.h:111-130   e = log(Tj^-1 C Ti), Ti = vertex 0, Tj = vertex 1
  EdgeSE3Expmap::linearizeOplus   g2o/types/sba/types_six_dof_expmap.cpp:271-286 J0 = adj(Tj^-1 C), J1 = -adj(Ti^-1 C^-1)
  EdgeSE3Expmap::read / write     g2o/types/sba/types_six_dof_expmap.cpp:109-135 (the file holds the INVERSE of the measurement)
  SE3Quat::log / exp / adj        g2o/types/slam3d/se3quat.h:178-215, 223-257, 259-268
  VertexSE3Expmap::oplusImpl      T <- exp(u) T, u = (omega, upsilon)

fp64 NumPy over whole edge lists, written operation for operation like the device kernel (csrc/ba_pose_edge.inc): the same
products in the same order of summation, the same two formulas of the logarithm with the branch at d > 0.99999, no guard near a
rotation of pi and none for d outside [-1, 1], as in the reference.  The kernel states the same operations in HIP without
contraction to fused multiply-adds and shares no code with this file.  The Jacobians are the reference's adjoint form: the
derivative of the error at e = 0 only.

Layouts as in the C ABI: an isometry is [12] = R column-major | t (cameras: world -> camera); Jacobians 6 x 6 column-major,
columns and error in the order (omega, upsilon).  Internally an isometry is (R, t) with R[i][j] and t[i] arrays over the edges."""
import numpy as np

LOG_SWITCH = 0.99999      # SE3Quat::log
EXP_SWITCH = 0.00001      # SE3Quat::exp


def unpack(T):
    """[n][12] -> (R[i][j], t[i]), each an [n] array."""
    T = np.asarray(T, np.float64).reshape(-1, 12)
    return [[T[:, i + 3 * j] for j in range(3)] for i in range(3)], [T[:, 9 + i] for i in range(3)]


def pack(X):
    R, t = X
    return np.stack([R[i][j] for j in range(3) for i in range(3)] + list(t), axis=1)


def _mv(R, v):
    return [(R[i][0] * v[0] + R[i][1] * v[1]) + R[i][2] * v[2] for i in range(3)]


def inverse(X):
    """(R', -(R' t))."""
    R, t = X
    Rt = [[R[j][i] for j in range(3)] for i in range(3)]
    return Rt, [-v for v in _mv(Rt, t)]


def product(A, B):
    """A B = (Ra Rb, Ra tb + ta)."""
    Ra, ta = A
    Rb, tb = B
    R = [[(Ra[i][0] * Rb[0][j] + Ra[i][1] * Rb[1][j]) + Ra[i][2] * Rb[2][j] for j in range(3)] for i in range(3)]
    w = _mv(Ra, tb)
    return R, [w[i] + ta[i] for i in range(3)]


def log(X):
    """SE3Quat::log as (omega[3], upsilon[3]).  Omega^2 = omega omega' - |omega|^2 I is written out entry by entry."""
    R, t = X
    d = 0.5 * (((R[0][0] + R[1][1]) + R[2][2]) - 1.0)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    small = d > LOG_SWITCH
    with np.errstate(all="ignore"):       # (the formula of the other branch is evaluated for every edge and not taken)
        theta = np.arccos(d)
        sc = np.where(small, 0.5, theta / (2.0 * np.sqrt(1.0 - d * d)))
        cf = np.where(small, 1.0 / 12.0, (1.0 - theta / (2.0 * np.tan(theta / 2.0))) / (theta * theta))
    ox, oy, oz = sc * dR[0], sc * dR[1], sc * dR[2]
    xx, yy, zz, xy, xz, yz = ox * ox, oy * oy, oz * oz, ox * oy, ox * oz, oy * oz
    V = [[1.0 + cf * (-(yy + zz)), 0.5 * oz + cf * xy, -0.5 * oy + cf * xz],
         [-0.5 * oz + cf * xy, 1.0 + cf * (-(xx + zz)), 0.5 * ox + cf * yz],
         [0.5 * oy + cf * xz, -0.5 * ox + cf * yz, 1.0 + cf * (-(xx + yy))]]
    return [ox, oy, oz], _mv(V, t)


def adj(X, sign=1.0):
    """sign * [R 0; skew(t) R  R] as [n][36], column-major."""
    R, t = X
    zero = np.zeros_like(t[0])
    cols = [None] * 6
    for c in range(3):
        r = [R[0][c], R[1][c], R[2][c]]
        s = [t[1] * r[2] - t[2] * r[1], t[2] * r[0] - t[0] * r[2], t[0] * r[1] - t[1] * r[0]]
        cols[c] = [sign * v for v in r] + [sign * v for v in s]
        cols[3 + c] = [zero, zero, zero] + [sign * v for v in r]
    return np.stack([v for col in cols for v in col], axis=1)


def error(Ti, Tj, C):
    """computeError of whole lists of isometries [n][12]: [n][6] = (omega, upsilon) of log(Tj^-1 C Ti)."""
    w, u = log(product(product(inverse(unpack(Tj)), unpack(C)), unpack(Ti)))
    return np.stack(w + u, axis=1)


def jacobians(Ti, Tj, C):
    """linearizeOplus: (J0, J1), [n][36] each."""
    Xi, Xj, Xc = unpack(Ti), unpack(Tj), unpack(C)
    return adj(product(inverse(Xj), Xc)), adj(product(inverse(Xi), inverse(Xc)), -1.0)


def pose_edges(cams, vi, vj, meas, jac=True):
    """(J0 [n][36], J1 [n][36], err [n][6]) of an edge list over the camera table, or err alone.  Blocks of fixed vertices are
    evaluated like the others."""
    cams = np.asarray(cams, np.float64).reshape(-1, 12)
    meas = np.asarray(meas, np.float64).reshape(-1, 12)
    if len(meas) == 0:
        return (np.zeros((0, 36)), np.zeros((0, 36)), np.zeros((0, 6))) if jac else np.zeros((0, 6))
    Ti, Tj = cams[np.asarray(vi, np.int64)], cams[np.asarray(vj, np.int64)]
    err = error(Ti, Tj, meas)
    if not jac:
        return err
    J0, J1 = jacobians(Ti, Tj, meas)
    return J0, J1, err


def exp(u):
    """SE3Quat::exp of [n][6] = (omega, upsilon) as isometries [n][12]; kept as (R, V upsilon) like the project keeps its
    cameras (below the threshold I + Omega + Omega^2 is not re-normalised)."""
    u = np.asarray(u, np.float64).reshape(-1, 6)
    ox, oy, oz = u[:, 0], u[:, 1], u[:, 2]
    theta = np.sqrt((ox * ox + oy * oy) + oz * oz)
    small = theta < EXP_SWITCH
    th = np.where(small, 1.0, theta)
    a = np.where(small, 1.0, np.sin(th) / th)
    b = np.where(small, 1.0, (1.0 - np.cos(th)) / (th * th))
    c = np.where(small, 1.0, (th - np.sin(th)) / (th * th * th))
    zero = np.zeros_like(ox)
    Om = [[zero, -oz, oy], [oz, zero, -ox], [-oy, ox, zero]]
    xx, yy, zz, xy, xz, yz = ox * ox, oy * oy, oz * oz, ox * oy, ox * oz, oy * oz
    Om2 = [[-(yy + zz), xy, xz], [xy, -(xx + zz), yz], [xz, yz, -(xx + yy)]]
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    R = [[(eye[i][j] + a * Om[i][j]) + b * Om2[i][j] for j in range(3)] for i in range(3)]
    V = [[np.where(small, R[i][j], (eye[i][j] + b * Om[i][j]) + c * Om2[i][j]) for j in range(3)] for i in range(3)]
    return pack((R, _mv(V, [u[:, 3], u[:, 4], u[:, 5]])))


def oplus(T, u):
    """VertexSE3Expmap::oplusImpl: exp(u) T for [n][12] and [n][6]."""
    return pack(product(unpack(exp(u)), unpack(T)))


def relative_measurement(Ti, Tj):
    """The measurement C with zero error between the isometries: Tj^-1 C Ti = I, i.e. C = Tj Ti^-1."""
    return pack(product(unpack(Tj), inverse(unpack(Ti))))


# ------------------------------------------------------------------------------------------------ the file form (fp64)
def iso_to_vector7(T):
    """[n][12] -> (tx, ty, tz, qx, qy, qz, qw), unit quaternion with w >= 0 (SE3Quat::toVector after normalizeRotation)."""
    T = np.asarray(T, np.float64).reshape(-1, 12)
    out = np.zeros((len(T), 7))
    out[:, 0:3] = T[:, 9:12]
    for k, row in enumerate(T):
        R = row[:9].reshape(3, 3).T
        tr = R[0, 0] + R[1, 1] + R[2, 2]
        sq = [1 + 2 * R[a, a] - tr for a in range(3)] + [1 + tr]
        m = int(np.argmax(sq))
        q = np.zeros(4)
        for a in range(4):
            if a == m:
                q[a] = sq[m]
            elif m == 3 or a == 3:
                c = a if m == 3 else m
                b, a2 = (c + 2) % 3, (c + 1) % 3
                q[a] = R[b, a2] - R[a2, b]
            else:
                q[a] = R[a, m] + R[m, a]
        q /= np.linalg.norm(q)
        out[k, 3:7] = -q if q[3] < 0 else q
    return out


def vector7_to_iso(v):
    """(tx, ty, tz, qx, qy, qz, qw) -> [n][12]; the quaternion is normalised first (SE3Quat::fromVector)."""
    v = np.asarray(v, np.float64).reshape(-1, 7)
    q = v[:, 3:7] / np.linalg.norm(v[:, 3:7], axis=1)[:, None]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    return pack((R, [v[:, 0], v[:, 1], v[:, 2]]))


def invert(T):
    """The inverse isometries, [n][12]."""
    return pack(inverse(unpack(T)))


def chi2(err, omega, huber=0.0):
    """sum of rho(e' Omega e) in fp64 (rho = Huber of width `huber` on sqrt(e' Omega e), or the identity); omega [n][36]."""
    e2 = np.einsum("ni,nij,nj->n", err, np.asarray(omega).reshape(-1, 6, 6), err)
    if huber > 0:
        big = e2 > huber * huber
        e2 = np.where(big, 2.0 * huber * np.sqrt(np.where(big, e2, 1.0)) - huber * huber, e2)
    return float(e2.sum())
