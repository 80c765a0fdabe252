"""Host restatement of the structure-only bundle adjustment the device runs in one launch (g2ohip_ba_structure_only,
csrc/ba_structure_only.inc):

  StructureOnlySolver<3>::calc(points, num_iters, num_max_trials)   g2o/solvers/structure_only/structure_only_solver.h:72-194
  EdgeProjectXYZ2UV::computeError / linearizeOplus (point block)    g2o/types/sba/types_six_dof_expmap.cpp:288-326
  EdgeProjectXYZ2UVU::computeError                                  g2o/types/sba/types_six_dof_expmap.h:181-200
  robust kernels (rho')                                             g2o/core/robust_kernel_impl.cpp:65-126

ONE body of formulas, generic over the arithmetic F: FP64 below (Python floats), tests/structure_only_helpers.py adds mpmath at
60 digits.  F supplies num(x), sqrt and isfinite.  The literals of the reference (mu = 0.01, nu = 2, 0.001, 1./3.) enter every
arithmetic as their fp64 values.  Every data-dependent decision -- |b| against 0.001, the smallest LDL' pivot against 0,
chi2 - new_chi2 against 0 -- is appended to `decisions` (when given) as (point, kind, value), so that a test can hold two
arithmetics to the same path and measure how far each decision was from its threshold.  The device kernel states the same
operations in HIP and shares no code with this file (it sums a track across lanes, so its rounding differs).

Input: a synthetic.make_ba_problem dictionary (mono, or stereo with observation = "stereo" and baseline), optionally with
  info [E][d * d] column-major information matrices (absent: identity),
  pt_hidx [L] (-1 = fixed point; absent: every point is free),
  class_params [C][5] = (f, cx, cy, kernel kind, delta) and edge_class [E] (mono only; they replace f, cx, cy and `kernel`).
A point's track is every edge that names it, in edge order, observations from fixed cameras included."""
import math

import numpy as np

MU0, NU0, B_STOP, THIRD = 0.01, 2.0, 0.001, 1.0 / 3.0
REASON_ITERS, REASON_GRADIENT, REASON_TRIALS, REASON_SKIPPED = 0, 1, 2, 3
DECISION_GRADIENT, DECISION_PIVOT, DECISION_RHO = "b_norm", "min_pivot", "chi2_drop"


class FP64:
    name = "fp64"
    sqrt = math.sqrt
    isfinite = math.isfinite

    @staticmethod
    def num(x):
        return float(x)


def robust_weight(F, kind, delta, e2):
    """rho'(e2) of robust_kernel_impl.cpp: 1 Huber, 2 PseudoHuber, 3 Cauchy, 4 Saturated, 5 DCS; 0 none."""
    one = F.num(1.0)
    if kind == 0:
        return one
    delta = F.num(delta)
    dsqr = delta * delta
    if kind == 1:
        return one if e2 <= dsqr else delta / F.sqrt(e2)
    if kind == 2:
        return one / F.sqrt(e2 / dsqr + one)
    if kind == 3:
        return one / (e2 / dsqr + one)
    if kind == 4:
        return one if e2 <= dsqr else F.num(0.0)
    if kind == 5:
        sc = (F.num(2.0) * delta) / (delta + e2)
        if sc >= one:
            sc = one
        return sc * sc
    raise ValueError("robust kernel kind %r" % (kind,))


def _camera_frame(T, X):
    return (T[0] * X[0] + T[3] * X[1] + T[6] * X[2] + T[9],
            T[1] * X[0] + T[4] * X[1] + T[7] * X[2] + T[10],
            T[2] * X[0] + T[5] * X[1] + T[8] * X[2] + T[11])


def edge_error(F, T, X, z, f, cx, cy, baseline=None, jac=False):
    """Error (2 or 3 rows) of one observation and, with jac, the point-side Jacobian A [d][3] (rows)."""
    x, y, zc = _camera_frame(T, X)
    if baseline is None:
        iz = F.num(1.0) / zc
        xz, yz = x * iz, y * iz
        r = [z[0] - (xz * f + cx), z[1] - (yz * f + cy)]
        rows = [[f, F.num(0.0), -xz * f], [F.num(0.0), f, -yz * f]]
    else:
        iz = F.num(1.0) / zc
        xr = x - baseline
        r = [z[0] - (x / zc * f + cx), z[1] - (y / zc * f + cy), z[2] - (xr / zc * f + cx)]
        rows = [[f, F.num(0.0), -x / zc * f], [F.num(0.0), f, -y / zc * f], [f, F.num(0.0), -xr / zc * f]]
    if not jac:
        return r, None
    A = [[-iz * (row[0] * T[0 + 3 * c] + row[1] * T[1 + 3 * c] + row[2] * T[2 + 3 * c]) for c in range(3)] for row in rows]
    return r, A


def _track_terms(F, track, X, lin):
    """chi2 = sum e' Omega e over the track; with lin also H = sum w A' Omega A (3 x 3, rows) and b = -sum w A' Omega e."""
    zero = F.num(0.0)
    chi = zero
    H = [[zero] * 3 for _ in range(3)]
    b = [zero] * 3
    for T, z, O, f, cx, cy, bl, kind, delta in track:
        r, A = edge_error(F, T, X, z, f, cx, cy, bl, lin)
        d = len(r)
        Or = [sum((O[i + d * j] * r[j] for j in range(d)), zero) for i in range(d)]
        e2 = sum((r[i] * Or[i] for i in range(d)), zero)
        chi = chi + e2
        if lin:
            w = robust_weight(F, kind, delta, e2)
            for c in range(3):
                b[c] = b[c] - w * sum((A[i][c] * Or[i] for i in range(d)), zero)
                OA = [w * sum((O[i + d * j] * A[j][c] for j in range(d)), zero) for i in range(d)]
                for a in range(3):
                    H[a][c] = H[a][c] + sum((A[i][a] * OA[i] for i in range(d)), zero)
    return chi, H, b


def ldlt3(F, H, mu, b):
    """Unpivoted LDL' of H + mu I (lower triangle) and the solve: (pivots, delta)."""
    a00, a10, a20, a11, a21, a22 = H[0][0] + mu, H[1][0], H[2][0], H[1][1] + mu, H[2][1], H[2][2] + mu
    d0 = a00
    l10, l20 = a10 / d0, a20 / d0
    d1 = a11 - l10 * a10
    t21 = a21 - l20 * a10
    l21 = t21 / d1
    d2 = a22 - l20 * a20 - l21 * t21
    y0 = b[0]
    y1 = b[1] - l10 * y0
    y2 = b[2] - l20 * y0 - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = y0 / d0 - l10 * x1 - l20 * x2
    return (d0, d1, d2), [x0, x1, x2]


def tracks(F, prob, kernel=(0, 0.0)):
    """Per point: the list of its observations (T, z, Omega, f, cx, cy, baseline or None, kernel kind, delta) in edge order."""
    stereo = prob.get("observation") == "stereo"
    d = 3 if stereo else 2
    cams = [[F.num(v) for v in row] for row in np.asarray(prob["cams"], np.float64)]
    meas = np.asarray(prob["meas"], np.float64).reshape(-1, d)
    info = prob.get("info")
    ident = [F.num(1.0 if i % (d + 1) == 0 else 0.0) for i in range(d * d)]
    cp, ec = prob.get("class_params"), prob.get("edge_class")
    bl = F.num(prob["baseline"]) if stereo else None
    out = [[] for _ in range(len(prob["pts"]))]
    for k, (c, p) in enumerate(zip(prob["cam_idx"], prob["pt_idx"])):
        if cp is not None:
            f, cx, cy, kind, delta = np.asarray(cp, np.float64).reshape(-1, 5)[ec[k]]
        else:
            f, cx, cy, (kind, delta) = prob["f"], prob["cx"], prob["cy"], kernel
        O = ident if info is None else [F.num(v) for v in np.asarray(info, np.float64).reshape(-1, d * d)[k]]
        out[p].append((cams[c], [F.num(v) for v in meas[k]], O, F.num(f), F.num(cx), F.num(cy), bl, int(kind), float(delta)))
    return out


def structure_only(prob, num_iters=10, num_max_trials=10, kernel=(0, 0.0), F=FP64, decisions=None):
    """The points after calc(points, num_iters, num_max_trials), the traces [L][4] = (outer iterations started, accepted steps,
    rejected trials, stop reason) and chi2 [L][2] = (before, after) -- entries of arithmetic F in lists (to_f64 converts)."""
    if num_iters < 0 or num_max_trials < 1:
        raise ValueError("num_iters >= 0 and num_max_trials >= 1")
    pts = [[F.num(v) for v in row] for row in np.asarray(prob["pts"], np.float64)]
    hidx = prob.get("pt_hidx")
    trs = tracks(F, prob, kernel)
    trace, chis = [], []
    for v, X in enumerate(pts):
        track = trs[v]
        if (hidx is not None and hidx[v] < 0) or not track:
            trace.append((0, 0, 0, REASON_SKIPPED))
            chis.append((F.num(0.0), F.num(0.0)))
            continue
        mu, nu = F.num(MU0), F.num(NU0)
        chi2, _, _ = _track_terms(F, track, X, False)
        before = chi2
        iters = accepted = rejected = 0
        reason = REASON_ITERS
        for _ in range(num_iters):
            iters += 1
            _, H, b = _track_terms(F, track, X, True)
            bn = F.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
            if decisions is not None:
                decisions.append((v, DECISION_GRADIENT, bn))
            if bn < F.num(B_STOP):
                reason = REASON_GRADIENT
                break
            trial = 0
            stop = False
            while True:
                piv, delta = ldlt3(F, H, mu, b)
                good = False
                if decisions is not None:
                    decisions.append((v, DECISION_PIVOT, min(piv)))
                if piv[0] > 0 and piv[1] > 0 and piv[2] > 0:
                    Xn = [X[i] + delta[i] for i in range(3)]
                    new_chi2, _, _ = _track_terms(F, track, Xn, False)
                    if decisions is not None:
                        decisions.append((v, DECISION_RHO, chi2 - new_chi2))
                    if chi2 - new_chi2 > 0 and F.isfinite(new_chi2):
                        good = True
                        chi2 = new_chi2
                        X = Xn
                if good:
                    mu = mu * F.num(THIRD)
                    nu = F.num(NU0)
                    accepted += 1
                    break
                mu = mu * nu
                nu = nu * F.num(2.0)
                rejected += 1
                trial += 1
                if trial >= num_max_trials:
                    stop = True
                    break
            if stop:
                reason = REASON_TRIALS
                break
        pts[v] = X
        trace.append((iters, accepted, rejected, reason))
        chis.append((before, chi2))
    return pts, trace, chis


def to_f64(rows):
    return np.array([[float(x) for x in r] for r in rows], np.float64)


def total_chi2(prob, kernel=(0, 0.0), F=FP64):
    """sum e' Omega e over EVERY edge (fixed points included), unrobustified."""
    pts = [[F.num(v) for v in row] for row in np.asarray(prob["pts"], np.float64)]
    return sum((_track_terms(F, t, pts[v], False)[0] for v, t in enumerate(tracks(F, prob, kernel))), F.num(0.0))
