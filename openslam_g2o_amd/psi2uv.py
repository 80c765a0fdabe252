"""Host-side arithmetic of the reference's anchored inverse-depth observation, a three-vertex edge (point psi, observing pose T,
anchor pose A), for the generators, the host-fed baseline of tools/ba_psi_time.py and the tests:

  EdgeProjectPSI2UV::computeError     g2o/types/sba/types_six_dof_expmap.cpp:173-183  e = obs - cam_map(T A^-1 invert_depth(psi))
  EdgeProjectPSI2UV::linearizeOplus   g2o/types/sba/types_six_dof_expmap.cpp:185-233  d_proj_d_y, d_expy_d_y, d_Tinvpsi_d_psi
  invert_depth                        x_a = (psi0, psi1, 1) / psi2
  VertexSBAPointXYZ::oplusImpl        psi <- psi + u;   VertexSE3Expmap::oplusImpl  T <- exp(u) T (se3expmap.oplus)

With R_ca = R_T R_A', t_ca = t_T - R_ca t_A, y = R_ca x_a + t_ca:

  e        = z - (f y0 / y2 + cx, f y1 / y2 + cy)
  Jcam     = [f / y2, 0, -f y0 / y2^2; 0, f / y2, -f y1 / y2^2]
  J_point  = -Jcam [r1, r2, -R_ca x_a] / psi2        r1, r2 = the first two columns of R_ca
  J_pose   = -Jcam [-skew(y) | I]                    columns (omega, upsilon)
  J_anchor =  Jcam R_ca [-skew(x_a) | I]

fp64 NumPy over whole edge lists, written operation for operation like the device kernel (csrc/ba_psi.inc): the same products in
the same order of summation, no guard for psi2 == 0 or y2 <= 0, as in the reference.  The kernel states the same operations in
HIP without contraction to fused multiply-adds and shares no code with this file.

Layouts as in the C ABI: an isometry is [12] = R column-major | t (cameras: world -> camera); Jacobians 2 x 3 / 2 x 6
column-major."""
import numpy as np


def invert_depth(X):
    """[n][3] points (x, y, z) of one frame -> psi = (x / z, y / z, 1 / z); its own inverse."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    return np.stack([X[:, 0] / X[:, 2], X[:, 1] / X[:, 2], 1.0 / X[:, 2]], axis=1)


def to_world(psi, anchors):
    """The world points of psi [n][3] held in the frames of the isometries anchors [n][12]: A^-1 invert_depth(psi)."""
    x = invert_depth(psi)
    A = np.asarray(anchors, np.float64).reshape(-1, 12)
    R = A[:, 0:9].reshape(-1, 3, 3).transpose(0, 2, 1)
    return (R.transpose(0, 2, 1) @ (x - A[:, 9:12])[:, :, None])[:, :, 0]


def edges(cams, pts, cam_v, anchor_v, pt_v, meas, f, cx, cy, jac=True):
    """(J_point [n][6], J_pose [n][12], J_anchor [n][12], err [n][2]) of an edge list over the camera and point tables, or err
    alone.  Blocks of fixed vertices, and of edges observed by their own anchor, are evaluated like the others."""
    cams = np.asarray(cams, np.float64).reshape(-1, 12)
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    meas = np.asarray(meas, np.float64).reshape(-1, 2)
    n = len(meas)
    if n == 0:
        return (np.zeros((0, 6)), np.zeros((0, 12)), np.zeros((0, 12)), np.zeros((0, 2))) if jac else np.zeros((0, 2))
    T, A, p = cams[np.asarray(cam_v, np.int64)], cams[np.asarray(anchor_v, np.int64)], pts[np.asarray(pt_v, np.int64)]
    psi2 = p[:, 2]
    xa = [p[:, 0] / psi2, p[:, 1] / psi2, 1.0 / psi2]

    def el(M, i, j):
        return M[:, i + 3 * j]
    R = [[(el(T, i, 0) * el(A, j, 0) + el(T, i, 1) * el(A, j, 1)) + el(T, i, 2) * el(A, j, 2) for j in range(3)] for i in range(3)]
    rx = [(R[i][0] * xa[0] + R[i][1] * xa[1]) + R[i][2] * xa[2] for i in range(3)]
    ra = [(R[i][0] * A[:, 9] + R[i][1] * A[:, 10]) + R[i][2] * A[:, 11] for i in range(3)]
    y = [rx[i] + (T[:, 9 + i] - ra[i]) for i in range(3)]
    with np.errstate(all="ignore"):
        err = np.stack([meas[:, 0] - (y[0] / y[2] * f + cx), meas[:, 1] - (y[1] / y[2] * f + cy)], axis=1)
        if not jac:
            return err
        y2sq = y[2] * y[2]
        a, c0, c1 = f / y[2], -(f * y[0]) / y2sq, -(f * y[1]) / y2sq
        ip = 1.0 / psi2
        zero = np.zeros(n)
        jp = []
        for c in range(3):
            m = [(R[i][c] if c < 2 else -rx[i]) * ip for i in range(3)]
            jp += [-(a * m[0] + c0 * m[2]), -(a * m[1] + c1 * m[2])]
        jc = [-(c0 * y[1]), a * y[2] - c1 * y[1], -(a * y[2] - c0 * y[0]), c1 * y[0], a * y[1], -(a * y[0]), -a, zero, zero, -a, -c0, -c1]
        g0 = [a * R[0][j] + c0 * R[2][j] for j in range(3)]
        g1 = [a * R[1][j] + c1 * R[2][j] for j in range(3)]
        ja = [g0[2] * xa[1] - g0[1] * xa[2], g1[2] * xa[1] - g1[1] * xa[2], g0[0] * xa[2] - g0[2] * xa[0], g1[0] * xa[2] - g1[2] * xa[0],
              g0[1] * xa[0] - g0[0] * xa[1], g1[1] * xa[0] - g1[0] * xa[1], g0[0], g1[0], g0[1], g1[1], g0[2], g1[2]]
    return np.stack(jp, axis=1), np.stack(jc, axis=1), np.stack(ja, axis=1), err


def problem_edges(prob, cams=None, pts=None, jac=True):
    """edges() of a synthetic.make_ba_inverse_depth problem (or of other estimates over its tables)."""
    return edges(prob["cams"] if cams is None else cams, prob["pts"] if pts is None else pts, prob["cam_idx"], prob["anchor_idx"],
                 prob["pt_idx"], prob["meas"], prob["f"], prob["cx"], prob["cy"], jac)
