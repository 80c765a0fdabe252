"""Extended-precision reference of the edge error functions, the vertex oplus operators and the robust kernels (test
infrastructure only, mpmath at 60 digits).  Written from the DEFINITIONS of the operations -- group composition, inverse,
"the unit quaternion with w >= 0 of a rotation", pinhole projection -- and shares no Jacobian formula with the kernels or
the C oracle: every Jacobian here is the central difference of an error function through an oplus function, evaluated
with a step of 1e-20 (truncation ~ step^2 = 1e-40, rounding ~ 1e-60 / 1e-20 = 1e-40, both far below fp64 rounding).

Where an operation is DEFINED with fp64 constants (M_PI in normalize_theta, 0.00001 in SE3Quat::exp, e2 <= delta^2 in the
robust kernels) the same fp64 constants are used here; the fixture generator keeps the inputs away from such switches or
exactly on them.

Layouts as in the project: SE2 (x, y, theta); isometries T[12] = R column-major | t; Jacobian blocks column-major."""
import math

import mpmath as mp

mp.mp.dps = 60
STEP = mp.mpf(10) ** -20
PI64 = mp.mpf(math.pi)            # M_PI, the fp64 constant normalize_theta is written with
EXP_SWITCH = mp.mpf(0.00001)      # the fp64 literal of SE3Quat::exp


def V(x):
    return [mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in x]


# ------------------------------------------------------------------------------------------------ SE2
def normalize_theta(t):
    """g2o's normalize_theta: into [-M_PI, M_PI) with the fp64 constant."""
    if -PI64 <= t < PI64:
        return t
    t = t - mp.floor(t / (2 * PI64)) * 2 * PI64
    if t >= PI64:
        t -= 2 * PI64
    if t < -PI64:
        t += 2 * PI64
    return t


def se2_inv(a):
    th = normalize_theta(-a[2])
    c, s = mp.cos(th), mp.sin(th)
    return [c * -a[0] - s * -a[1], s * -a[0] + c * -a[1], th]


def se2_mul(a, b):
    c, s = mp.cos(a[2]), mp.sin(a[2])
    return [a[0] + c * b[0] - s * b[1], a[1] + s * b[0] + c * b[1], normalize_theta(a[2] + b[2])]


def se2_error(xi, xj, z):
    """EdgeSE2: Z^-1 (Xi^-1 Xj) as (x, y, theta)."""
    return se2_mul(se2_inv(z), se2_mul(se2_inv(xi), xj))


def se2_oplus(p, u):
    return [p[0] + u[0], p[1] + u[1], normalize_theta(p[2] + u[2])]


def se2_point_error(x, l, z):
    """EdgeSE2PointXY: X^-1 l - z."""
    c, s = mp.cos(x[2]), mp.sin(x[2])
    dx, dy = l[0] - x[0], l[1] - x[1]
    return [c * dx + s * dy - z[0], -s * dx + c * dy - z[1]]


def point_oplus(l, u):
    return [a + b for a, b in zip(l, u)]


# ------------------------------------------------------------------------------------------------ SE3
def iso(T):
    """T[12] -> (R as 3 rows, t)."""
    T = V(T)
    return [[T[r + 3 * c] for c in range(3)] for r in range(3)], T[9:12]


def iso_pack(X):
    R, t = X
    return [R[r][c] for c in range(3) for r in range(3)] + list(t)


def mat3(A, B):
    return [[sum(A[r][m] * B[m][c] for m in range(3)) for c in range(3)] for r in range(3)]


def mv3(A, v):
    return [sum(A[r][m] * v[m] for m in range(3)) for r in range(3)]


def iso_mul(A, B):
    return mat3(A[0], B[0]), [a + b for a, b in zip(mv3(A[0], B[1]), A[1])]


def iso_inv(A):
    Rt = [[A[0][c][r] for c in range(3)] for r in range(3)]
    return Rt, [-v for v in mv3(Rt, A[1])]


def quat_to_R(w, x, y, z):
    """Rotation matrix of the (not necessarily unit) quaternion, as Eigen's toRotationMatrix writes it."""
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def R_to_quat(R):
    """(x, y, z, w), unit, w >= 0, of the rotation R.  From the definition 4 q q' = [[1 + 2 r_aa - tr, ...]]: the four
    squares 4 w^2 = 1 + tr, 4 q_a^2 = 1 + 2 r_aa - tr; the largest fixes the scale, the off-diagonal sums / differences the
    other three.  (Not the case split of Eigen's Quaterniond(Matrix3d): for a rotation every choice gives the same q.)"""
    tr = R[0][0] + R[1][1] + R[2][2]
    sq = [1 + 2 * R[a][a] - tr for a in range(3)] + [1 + tr]
    m = max(range(4), key=lambda a: sq[a])
    row = [0] * 4                       # row m of 4 q q'
    for a in range(4):
        if a == m:
            row[a] = sq[m]
        elif m == 3 or a == 3:          # 4 w q_c = r_ba - r_ab (c, b, a cyclic)
            c = a if m == 3 else m
            b, a2 = (c + 2) % 3, (c + 1) % 3
            row[a] = R[b][a2] - R[a2][b]
        else:
            row[a] = R[a][m] + R[m][a]
    n = mp.sqrt(sum(v * v for v in row))
    q = [v / n for v in row]
    if q[3] < 0:
        q = [-v for v in q]
    return q


def se3_error(Xi, Xj, Z):
    """EdgeSE3: toVectorMQT(Z^-1 Xi^-1 Xj) = translation, vector part of the unit quaternion with w >= 0."""
    E = iso_mul(iso_inv(Z), iso_mul(iso_inv(Xi), Xj))
    return list(E[1]) + R_to_quat(E[0])[:3]


def se3_error_quat_w(Xi, Xj, Z):
    E = iso_mul(iso_inv(Z), iso_mul(iso_inv(Xi), Xj))
    return R_to_quat(E[0])[3]


def se3_oplus(X, u):
    """VertexSE3: X * fromVectorMQT(u); the identity rotation when the vector part is longer than 1."""
    w2 = 1 - (u[3] * u[3] + u[4] * u[4] + u[5] * u[5])
    I = [[mp.mpf(int(r == c)) for c in range(3)] for r in range(3)]
    inc = I if w2 < 0 else quat_to_R(mp.sqrt(w2), u[3], u[4], u[5])
    return iso_mul(X, (inc, list(u[:3])))


def se3_point_error(X, l, z, off):
    """EdgeSE3PointXYZ with ParameterSE3Offset: (X off)^-1 l - z."""
    W = iso_inv(iso_mul(X, off))
    return [a + b - c for a, b, c in zip(mv3(W[0], l), W[1], z)]


# ------------------------------------------------------------------------------------------------ BA
def expmap_oplus(T, u):
    """VertexSE3Expmap: SE3Quat::exp(u) * T, u = (omega, upsilon); exp with its two formulas and the fp64 threshold, kept
    as (R, t) like the project keeps its cameras (below the threshold I + W + W^2 is not re-normalised)."""
    w, ups = u[:3], u[3:]
    theta = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Om = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    Om2 = mat3(Om, Om)
    I = [[mp.mpf(int(r == c)) for c in range(3)] for r in range(3)]
    if theta < EXP_SWITCH:
        R = [[I[r][c] + Om[r][c] + Om2[r][c] for c in range(3)] for r in range(3)]
        Vm = R
    else:
        a, b = mp.sin(theta) / theta, (1 - mp.cos(theta)) / theta ** 2
        cc = (theta - mp.sin(theta)) / theta ** 3
        R = [[I[r][c] + a * Om[r][c] + b * Om2[r][c] for c in range(3)] for r in range(3)]
        Vm = [[I[r][c] + b * Om[r][c] + cc * Om2[r][c] for c in range(3)] for r in range(3)]
    return iso_mul((R, mv3(Vm, ups)), T)


def project_error(T, X, z, f, cx, cy):
    """EdgeProjectXYZ2UV: z - (f * hom(T X) + c)."""
    p = [a + b for a, b in zip(mv3(T[0], X), T[1])]
    return [z[0] - (f * p[0] / p[2] + cx), z[1] - (f * p[1] / p[2] + cy)]


def camera_point(T, X):
    return [a + b for a, b in zip(mv3(T[0], X), T[1])]


# ------------------------------------------------------------------------------------------------ Jacobians
def jacobian(err, oplus, x, dim):
    """Central differences of u -> err(oplus(x, u)) at u = 0; column-major [d x dim]."""
    cols = []
    for k in range(dim):
        up = [STEP if i == k else mp.mpf(0) for i in range(dim)]
        um = [-v for v in up]
        ep, em = err(oplus(x, up)), err(oplus(x, um))
        cols.append([(a - b) / (2 * STEP) for a, b in zip(ep, em)])
    return [v for col in cols for v in col]


def se2_edge(xi, xj, z):
    xi, xj, z = V(xi), V(xj), V(z)
    return (jacobian(lambda a: se2_error(a, xj, z), se2_oplus, xi, 3),
            jacobian(lambda b: se2_error(xi, b, z), se2_oplus, xj, 3), se2_error(xi, xj, z))


def se3_edge(Ti, Tj, Tz):
    Xi, Xj, Z = iso(Ti), iso(Tj), iso(Tz)
    return (jacobian(lambda a: se3_error(a, Xj, Z), se3_oplus, Xi, 6),
            jacobian(lambda b: se3_error(Xi, b, Z), se3_oplus, Xj, 6), se3_error(Xi, Xj, Z))


def se2_point_edge(x, l, z):
    x, l, z = V(x), V(l), V(z)
    return (jacobian(lambda a: se2_point_error(a, l, z), se2_oplus, x, 3),
            jacobian(lambda b: se2_point_error(x, b, z), point_oplus, l, 2), se2_point_error(x, l, z))


def se3_point_edge(T, l, z, off):
    X, O, l, z = iso(T), iso(off), V(l), V(z)
    return (jacobian(lambda a: se3_point_error(a, l, z, O), se3_oplus, X, 6),
            jacobian(lambda b: se3_point_error(X, b, z, O), point_oplus, l, 3), se3_point_error(X, l, z, O))


def project_edge(T, X, z, f, cx, cy):
    """(J point [2x3], J camera [2x6], err): vertex 0 of EdgeProjectXYZ2UV is the point."""
    C, X, z = iso(T), V(X), V(z)
    f, cx, cy = mp.mpf(float(f)), mp.mpf(float(cx)), mp.mpf(float(cy))
    return (jacobian(lambda b: project_error(C, b, z, f, cx, cy), point_oplus, X, 3),
            jacobian(lambda a: project_error(a, X, z, f, cx, cy), expmap_oplus, C, 6), project_error(C, X, z, f, cx, cy))


# ------------------------------------------------------------------------------------------------ priors, camera, stereo
def se2_prior_error(x, z):
    """EdgeSE2Prior: (Z^-1 X) as (x, y, theta)."""
    return se2_mul(se2_inv(z), x)


def se2_xy_prior_error(x, z):
    """EdgeSE2XYPrior: t - z."""
    return [x[0] - z[0], x[1] - z[1]]


def se3_prior_error(X, Z, P):
    """EdgeSE3Prior with ParameterSE3Offset P: toVectorMQT(Z^-1 X P)."""
    E = iso_mul(iso_inv(Z), iso_mul(X, P))
    return list(E[1]) + R_to_quat(E[0])[:3]


def se3_prior_quat_w(X, Z, P):
    return R_to_quat(iso_mul(iso_inv(Z), iso_mul(X, P))[0])[3]


def camera_point_k(X, l, P, K):
    """p = K (X P)^-1 l, K = (fx, fy, cx, cy)."""
    W = iso_inv(iso_mul(X, P))
    q = [a + b for a, b in zip(mv3(W[0], l), W[1])]
    return [K[0] * q[0] + K[2] * q[2], K[1] * q[1] + K[3] * q[2], q[2]]


def camera_error(X, l, z, P, K, disparity):
    """EdgeSE3PointXYZDepth / EdgeSE3PointXYZDisparity: (p0 / p2, p1 / p2, p2 or 1 / p2) - z."""
    p = camera_point_k(X, l, P, K)
    return [p[0] / p[2] - z[0], p[1] / p[2] - z[1], (1 / p[2] if disparity else p[2]) - z[2]]


def stereo_error(T, X, z, f, cx, cy, b):
    """EdgeProjectXYZ2UVU: z - (f x / z + cx, f y / z + cy, f (x - b) / z + cx), (x, y, z) = T X."""
    p = camera_point(T, X)
    return [z[0] - (f * p[0] / p[2] + cx), z[1] - (f * p[1] / p[2] + cy), z[2] - (f * (p[0] - b) / p[2] + cx)]


def se2_prior_edge(x, z):
    """(J0 [3x3], None, err) of EdgeSE2Prior."""
    x, z = V(x), V(z)
    return jacobian(lambda a: se2_prior_error(a, z), se2_oplus, x, 3), None, se2_prior_error(x, z)


def se2_xy_prior_edge(x, z):
    """(J0 [2x3], None, err) of EdgeSE2XYPrior."""
    x, z = V(x), V(z)
    return jacobian(lambda a: se2_xy_prior_error(a, z), se2_oplus, x, 3), None, se2_xy_prior_error(x, z)


def se3_prior_edge(T, Tz, off):
    """(J0 [6x6], None, err) of EdgeSE3Prior."""
    X, Z, P = iso(T), iso(Tz), iso(off)
    return jacobian(lambda a: se3_prior_error(a, Z, P), se3_oplus, X, 6), None, se3_prior_error(X, Z, P)


def camera_edge(T, l, z, off, K, disparity):
    """(J pose [3x6], J landmark [3x3], err) of the depth / disparity edge."""
    X, P, l, z, K = iso(T), iso(off), V(l), V(z), V(K)
    return (jacobian(lambda a: camera_error(a, l, z, P, K, disparity), se3_oplus, X, 6),
            jacobian(lambda b: camera_error(X, b, z, P, K, disparity), point_oplus, l, 3), camera_error(X, l, z, P, K, disparity))


def stereo_edge(T, X, z, f, cx, cy, b):
    """(J point [3x3], J camera [3x6], err): vertex 0 of EdgeProjectXYZ2UVU is the point."""
    C, X, z = iso(T), V(X), V(z)
    f, cx, cy, b = (mp.mpf(float(v)) for v in (f, cx, cy, b))
    return (jacobian(lambda p: stereo_error(C, p, z, f, cx, cy, b), point_oplus, X, 3),
            jacobian(lambda a: stereo_error(a, X, z, f, cx, cy, b), expmap_oplus, C, 6), stereo_error(C, X, z, f, cx, cy, b))


# ------------------------------------------------------------------------------------------------ robust kernels
HUBER, PSEUDO_HUBER, CAUCHY, SATURATED, DCS = 1, 2, 3, 4, 5


def robust(kind, delta, e2):
    """(rho, rho') of g2o's robust kernels at the squared error e2; 0 = none.  DCS: delta is phi and rho' is the squared
    scale, as g2o defines it."""
    e2, d = mp.mpf(e2), mp.mpf(float(delta))
    d2 = d * d
    if kind == HUBER:
        return (e2, mp.mpf(1)) if e2 <= d2 else (2 * mp.sqrt(e2) * d - d2, d / mp.sqrt(e2))
    if kind == PSEUDO_HUBER:
        a = mp.sqrt(1 + e2 / d2)
        return 2 * d2 * (a - 1), 1 / a
    if kind == CAUCHY:
        return d2 * mp.log(1 + e2 / d2), 1 / (1 + e2 / d2)
    if kind == SATURATED:
        return (e2, mp.mpf(1)) if e2 <= d2 else (d2, mp.mpf(0))
    if kind == DCS:
        s = min(2 * d / (d + e2), mp.mpf(1))
        return s * e2 * s, s * s
    return e2, mp.mpf(1)


def f64(x):
    """Round to fp64 (nearest)."""
    if isinstance(x, (list, tuple)):
        return [f64(v) for v in x]
    return float(x)
