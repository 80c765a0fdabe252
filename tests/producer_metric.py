"""Per-edge error metric and the fp64 branch predicates shared by tests/golden/make_producer_edges.py and the two
producer-reference tests (NumPy only).

METRIC.  For one edge (or vertex) e and one output block (err, J0, J1, updated vertex, H block):

    error_e = max_k |got[e, k] - ref[e, k]| / scale_e,      scale_e = max(1, max_k |ref[e, k]|, ops[e])

where ops[e] is stored in the fixture per edge: the largest magnitude among the operands that are added or subtracted
on the way to that block (the translations / positions / angles of the vertices, the measurement and the sensor offset of
that edge).  For EdgeSE2 the raw angles are operands too (normalize_theta subtracts multiples of 2 M_PI from them), so an
edge with angles of 1e4 rad is held 1e4 times more loosely than one inside [-pi, pi); in the update groups the translation
covers the rotation entries of the same vertex.  For the blocks of H and b (sums of products w J' J, w J' e) ops is the
largest, over the block's entries, of the sum of the magnitudes of the terms added into that entry (for the one-edge Hpl
block: its larger term); in b a term counts with max(|e|, |z|), e = z - proj being formed from the measurement.
The figure of a group is the worst edge's."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
CEILING = 1e-12          # TOL_J of the existing producer tests: no bound derived here may exceed it
MARGIN = 8.0


def per_edge(got, ref, ops):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    n = ref.shape[0]
    got, ref = got.reshape(n, -1), ref.reshape(n, -1)
    scale = np.maximum(1.0, np.maximum(np.abs(ref).max(axis=1), np.asarray(ops, np.float64).reshape(n)))
    return np.abs(got - ref).max(axis=1) / scale


def worst(got, ref, ops):
    e = per_edge(got, ref, ops)
    k = int(np.argmax(e))
    return float(e[k]), k


def per_row(got, ref, ops_rows, d):
    """Per edge AND per output row of a column-major d x dim block (dim = 1: the components of err): max over the row of
    |got - ref|, divided by max(max |ref row|, ops_rows[e, r]).  No floor of 1: the rows of one block carry different units
    (pixels beside metres beside 1 / metres), and a row of small entries is held to ITS size.  ops_rows [n][d] is stored in
    the fixture: the largest magnitude among the terms added or subtracted on the way to that row.  Returns [n][d]; a row whose
    reference and operands are all zero (a structural zero row) gives 0 where got is 0 too and inf otherwise."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    n = ref.shape[0]
    got, ref = got.reshape(n, -1, d), ref.reshape(n, -1, d)           # [e][column][row]
    scale = np.maximum(np.abs(ref).max(axis=1), np.asarray(ops_rows, np.float64).reshape(n, d))
    diff = np.abs(got - ref).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(diff == 0, 0.0, diff / scale)


def worst_row(got, ref, ops_rows, d):
    """(figure, edge, row) of the worst row of per_row."""
    e = per_row(got, ref, ops_rows, d)
    k, r = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[k, r]), int(k), int(r)


def bound(fx, key):
    """Device bound of fixture output `key`: MARGIN x the oracle's own worst per-edge error against the extended-precision
    reference; only where the oracle is exact (figure 0) the rounding floor of that output (floor_<key> eps, derived in
    tests/golden/make_producer_edges.py)."""
    o = float(fx["oracle_" + key])
    assert MARGIN * o <= CEILING, (key, o)
    if o > 0:
        return MARGIN * o
    assert float(fx["floor_" + key]) > 0, key
    return float(fx["floor_" + key]) * EPS


def ba_products_fp64(robustify, pre, J0, J1, err, par, h, l, nP, L):
    """Hpl / Hpp / Hll / b / chi2 from fp64 Jacobians, fp64 operations (robustify: the oracle's robust kernels, for the weights)."""
    E = len(h)
    A, B = J0.reshape(E, 3, 2).transpose(0, 2, 1), J1.reshape(E, 6, 2).transpose(0, 2, 1)     # [e][row][col]
    w, rho = np.ones(E), np.zeros(E)
    for k in range(E):
        e2 = err[k, 0] * err[k, 0] + err[k, 1] * err[k, 1]
        r = robustify(int(par[k, 3]), par[k, 4], e2) if par[k, 3] > 0 else (e2, 1.0, 0.0)
        rho[k], w[k] = r[0], r[1]
    Hpl = np.einsum("e,eri,erj->eji", w, B, A).reshape(E, 18)    # [e][c][r] -> column-major 6 x 3
    Hpl[np.asarray(h) < 0] = 0.0                                 # (a fixed camera has no block)
    Hpp, Hll, b = np.zeros((nP, 36)), np.zeros((L, 9)), np.zeros(6 * nP + 3 * L)
    for k in range(E):
        Hll[l[k]] += (w[k] * A[k].T @ A[k]).T.reshape(9)
        b[6 * nP + 3 * l[k]:6 * nP + 3 * l[k] + 3] -= w[k] * A[k].T @ err[k]
        if h[k] >= 0:
            Hpp[h[k]] += (w[k] * B[k].T @ B[k]).T.reshape(36)
            b[6 * h[k]:6 * h[k] + 6] -= w[k] * B[k].T @ err[k]
    return {pre + "_Hpl": Hpl, pre + "_Hpp": Hpp, pre + "_Hll": Hll, pre + "_b": b, pre + "_chi2": np.array([rho.sum()])}


# ---- the branch predicates in fp64, written as the kernels write them -------------------------------------------------
def _inv(T):
    R = T[:9].reshape(3, 3).T            # R[r, c]
    Rt = R.T.copy()
    t = np.array([-(Rt[r, 0] * T[9] + Rt[r, 1] * T[10] + Rt[r, 2] * T[11]) for r in range(3)])
    return Rt, t


def _mul(A, B):
    R = np.zeros((3, 3))
    for c in range(3):
        for r in range(3):
            s = 0.0
            for m in range(3):
                s += A[0][r, m] * B[0][m, c]
            R[r, c] = s
    t = np.array([A[0][r, 0] * B[1][0] + A[0][r, 1] * B[1][1] + A[0][r, 2] * B[1][2] + A[1][r] for r in range(3)])
    return R, t


def se3_branch(Ti, Tj, Tz):
    """(case, sign, tr, gap) of pg_R_to_quat / pg_dq_dR for one edge: case 0 (tr > 0) or 1 + index of the largest diagonal
    entry, sign = +1 / -1 for qw of the case formula > 0 / <= 0, gap = the two largest diagonal entries' difference."""
    Xj = (Tj[:9].reshape(3, 3).T, Tj[9:])
    E, _ = _mul(_inv(Tz), _mul(_inv(Ti), Xj))
    d = [E[0, 0], E[1, 1], E[2, 2]]
    tr = d[0] + d[1] + d[2]
    ds = sorted(d)
    gap = ds[2] - ds[1]
    if tr > 0:
        return 0, 1, tr, gap
    i = 0
    if (d[0] > d[1]) & (d[0] > d[2]):
        i = 0
    elif d[1] > d[2]:
        i = 1
    else:
        i = 2
    i2 = 0                                # (pg_R_to_quat's own selection: must agree away from ties)
    if d[1] > d[0]:
        i2 = 1
    if d[2] > d[i2]:
        i2 = 2
    assert i == i2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = 0.5 * np.sqrt(1.0 + d[i] - d[j] - d[k])
    qw = (E[k, j] - E[j, k]) / (4.0 * s)
    return 1 + i, (1 if qw > 0 else -1), tr, gap


def wrap_branch(theta):
    """Which way pg_normalize_theta goes for the fp64 angle theta: 'in', 'floor', 'floor+hi' (>= pi after the reduction)."""
    pi = np.pi
    if -pi <= theta < pi:
        return "in"
    t = theta - np.floor(theta / (2 * pi)) * 2 * pi
    if t >= pi:
        return "floor+hi"
    if t < -pi:
        return "floor+lo"
    return "floor"
