"""Writes tests/golden/sensor_edges.npz: branch-covering fp64 inputs for the unary priors (EdgeSE2Prior, EdgeSE2XYPrior,
EdgeSE3Prior over a ParameterSE3Offset), the depth / disparity camera edges and the stereo projection edge, their
extended-precision reference results (tests/reference_mp.py) rounded to fp64, per-ROW operand magnitudes, branch tags, and per
output the worst per-row error (tests/producer_metric.per_row) of the fp64 NumPy restatements (tests/prior_helpers.py,
landmark_camera_helpers.py, stereo_helpers.py) against that reference.  Run from the repository root:
    python tests/golden/make_sensor_edges.py        (deterministic; well under a minute)

Every group holds 513 edges, edge 0 between free vertices, so that the tails 1 / 255 / 256 / 257 / 513 are heads of it.

Per-row operand magnitudes (ops rows): the largest magnitude among the terms added or subtracted on the way to that row.
  prior3   err rows 0-2: the translations of pose, measurement and offset; rows 3-5: 1 (sums of rotation entries).
           J0 rows 0-2: max(1, 2 |t_offset|) (Ra and Ra skew(t_offset)); rows 3-5: 1.
  prior2   err rows 0-1: the positions of pose and measurement, times max(1, |theta_z|); row 2: the raw angles.  J0 rows
           0-1: max(1, |theta_z|); row 2: 1.  (normalize_theta subtracts multiples of 2 M_PI from the raw measurement angle
           in fp64 before cos / sin see it: at 1e4 rad the reduced angle, and with it Rz', is known to 1e4 eps.  That is the
           reference project's arithmetic, as for EdgeSE2 in make_producer_edges.py, so those edges are held |theta_z| times
           more loosely; with the positions alone as the scale the restatement itself is 1.4e-12 off on them.)
  camera   err: the measurement component, the projected value, and for rows 0-1 |f q / p2| and |c|.  J rows 0-1:
           max(|jp p2|, |p jp2|) / p2^2 over the row's columns; row 2: |jp2| (depth), |jp2| / p2^2 (disparity).
  stereo   err: the measurement component, |f x / z| (|f y / z|), |c|, and |f b / z| in row 2.  J rows: the largest product
           summed into an entry of the row, x - b counted as max(|x|, |b|).

Exclusions and moved inputs, all asserted below:
  * prior3 error rotations stay <= 179 degrees (qw >= 0.008), as in make_producer_edges.gen_se3.  The EXACT identity error
    (E = I bit for bit) is in the offset=None group: with a rotated offset Z^-1 X P = I holds up to rounding only.
  * prior2: the argument of the last normalize_theta, normalize(-theta_z) + theta, IS the error angle, so "exactly on +-M_PI"
    there is the jump of the error itself, excluded by the 1e-3 margin of the final angle; all exact hits are -theta_z = +-M_PI
    (at least 6).  The sums land on both sides of +-pi.  No estimate lies exactly on +-M_PI (see gen_se2).  Angles that
    normalize_theta reduces keep 1e-6 from its switch points.
  * camera: |l| / |p2| <= 400 (CAP): q = (X P)^-1 l cancels |l| down to the sensor-frame coordinates, and the projection
    divides by p2 twice.  |p2| >= 0.05 on every edge, also behind the sensor.
  * stereo: |X| / depth <= 25 and the error magnitudes of make_producer_edges.gen_ba (an edge far outside the image, and
    every edge of the far cluster, carries an error of at least f / 5, so that the robust weight is known to fp64)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_producer_edges as G                         # noqa: E402
from oracle import oracle as O                          # noqa: E402
from tests import landmark_camera_helpers as CH         # noqa: E402
from tests import prior_helpers as PH                   # noqa: E402
from tests import producer_metric as PM                 # noqa: E402
from tests import reference_mp as M                     # noqa: E402
from tests import stereo_helpers as SH                  # noqa: E402

mp = M.mp
OUT = os.path.join(HERE, "sensor_edges.npz")
PROFILE = os.path.join(ROOT, "profiles", "sensor_edges.jsonl")
N = 513
TAILS = (1, 255, 256, 257, 513)
MIN_PER_COMBO = 12
CAP = 400.0
WIDTH, HEIGHT = 640.0, 480.0
IDENT = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])

# Floors, in eps, where the restatement is EXACT (figure 0) and 8 x 0 bounds nothing:
#   prior2_J0   entries +-cos, +-sin, 0, 1: one library call each, no arithmetic -- the argument of lm2_J1 in
#               make_producer_edges.py (device sin / cos within 2 ulp <= 1 eps, + the reference's own rounding) -> 2 eps.
# (prior2xy is compared bit for bit and carries no bound at all.)
FLOORS = dict(prior2_J0=2)

STEREO_SETS = np.array([[1000.0, 320.0, 240.0, 0.5], [640.0, 300.5, 255.25, 0.075]])     # (f, cx, cy, b)
SET_DELTA = {1: 1.5, 2: 1.0, 3: 2.0, 4: 2.5, 5: 1.0}
CONFIGS = ("none", "set1", "set2", "set3", "set4", "set5", "edge")
CHI_N = (257, 513)
ASSEMBLED = {1: ("edge", "W")}          # stereo set -> (robust configuration, information) of its assembled system


def spd(rng, n, d):
    """n symmetric positive definite d x d matrices with off-diagonal entries, small integers (they compress), [n][d * d]."""
    A = rng.randint(-2, 3, (n, d, d)).astype(np.float64)
    W = A @ A.transpose(0, 2, 1) + d * np.eye(d)
    return np.ascontiguousarray(W.transpose(0, 2, 1).reshape(n, d * d))


def scales(a):
    """Operand magnitudes as stored: rounded to float32 (they are scales, not data; half the bytes)."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def rows_of(J, d):
    """column-major d x dim block (mp or float list) -> [row][col]."""
    dim = len(J) // d
    return [[J[r + d * c] for c in range(dim)] for r in range(d)]


class Products:
    """Hpp / Hll / Hpl / b in extended precision with the term-magnitude scales of make_producer_edges.gen_ba: H += w J' W J,
    b -= w J' W e; scale of an entry = the sum of the magnitudes of the terms added into it (Hpl: its largest term), of a
    block = its largest entry's; in b a term counts with ez = max(|e|, operands of e)."""

    def __init__(self, nP, nL, n, dl=3):
        self.nP, self.nL, self.dl = nP, nL, dl
        self.Hpp, self.Hpp_ops = [[mp.mpf(0)] * 36 for _ in range(nP)], np.zeros((nP, 36))
        self.Hll, self.Hll_ops = [[mp.mpf(0)] * 9 for _ in range(nL)], np.zeros((nL, 9))
        self.b, self.b_ops = [mp.mpf(0)] * (6 * nP + 3 * nL), np.zeros(6 * nP + 3 * nL)
        self.Hpl, self.Hpl_ops = np.zeros((n, 18)), np.zeros(n)

    def add(self, k, Jp, Jl, e, W, w, hp, hl, ez):
        d = len(e)
        Wm = [[mp.mpf(float(W[i + d * j])) for j in range(d)] for i in range(d)]
        aW = np.abs(np.asarray(W, np.float64).reshape(d, d).T)
        aez = np.asarray(ez, np.float64)
        wf = abs(float(w))
        blocks = []
        for J, dim, h, H, Hops, base in ((Jp, 6, hp, self.Hpp, self.Hpp_ops, 0), (Jl, 3, hl, self.Hll, self.Hll_ops, 6 * self.nP)):
            if J is None or h < 0:
                blocks.append(None)
                continue
            R = rows_of(J, d)
            WJ = [[w * sum(Wm[i][j] * R[j][c] for j in range(d)) for c in range(dim)] for i in range(d)]
            aJ = np.abs(np.array([[float(v) for v in row] for row in R]))
            Hops[h] += wf * (aJ.T @ aW @ aJ).T.reshape(-1)
            for c in range(dim):
                for r in range(dim):
                    H[h][r + dim * c] += sum(R[i][r] * WJ[i][c] for i in range(d))
                self.b[base + dim * h + c] -= sum(WJ[i][c] * e[i] for i in range(d))
            self.b_ops[base + dim * h:base + dim * h + dim] += wf * (aJ.T @ aW @ aez)
            blocks.append((R, WJ, aJ))
        if blocks[0] is not None and blocks[1] is not None:      # Hpl 6 x 3 column-major: Jp' (w W) Jl
            Rp, _, aJp = blocks[0]
            _, WJl, aJl = blocks[1]
            for c in range(3):
                for r in range(6):
                    self.Hpl[k, r + 6 * c] = float(sum(Rp[i][r] * WJl[i][c] for i in range(d)))
            self.Hpl_ops[k] = wf * float((aJp[:, :, None, None] * aW[:, None, :, None] * aJl[None, None, :, :]).max())

    def out(self, pre, hpl=False, hll=True):
        o = {pre + "_Hpp": np.array([M.f64(h) for h in self.Hpp]), pre + "_Hpp_ops": scales(self.Hpp_ops.max(axis=1)),
             pre + "_b": G.f64(self.b), pre + "_b_ops": scales(self.b_ops)}
        if hll:
            o.update({pre + "_Hll": np.array([M.f64(h) for h in self.Hll]), pre + "_Hll_ops": scales(self.Hll_ops.max(axis=1))})
        if hpl:
            o.update({pre + "_Hpl": self.Hpl, pre + "_Hpl_ops": scales(self.Hpl_ops)})
        return o


def products_fp64(pre, Jp, Jl, err, W, w, hp, hl, nP, nL, hpl=False, hll=True):
    """The same products from fp64 Jacobians with fp64 operations (the restatement's side of the figure)."""
    n, d = err.shape
    Wm = np.asarray(W).reshape(n, d, d).transpose(0, 2, 1)
    A = Jp.reshape(n, 6, d).transpose(0, 2, 1)
    B = None if Jl is None else Jl.reshape(n, 3, d).transpose(0, 2, 1)
    Hpp, Hll, b, Hpl = np.zeros((nP, 36)), np.zeros((nL, 9)), np.zeros(6 * nP + 3 * nL), np.zeros((n, 18))
    for k in range(n):
        if hp[k] >= 0:
            Hpp[hp[k]] += (w[k] * A[k].T @ Wm[k] @ A[k]).T.reshape(36)
            b[6 * hp[k]:6 * hp[k] + 6] -= w[k] * A[k].T @ Wm[k] @ err[k]
        if B is not None and hl[k] >= 0:
            Hll[hl[k]] += (w[k] * B[k].T @ Wm[k] @ B[k]).T.reshape(9)
            b[6 * nP + 3 * hl[k]:6 * nP + 3 * hl[k] + 3] -= w[k] * B[k].T @ Wm[k] @ err[k]
            if hp[k] >= 0:
                Hpl[k] = (w[k] * A[k].T @ Wm[k] @ B[k]).T.reshape(18)
    o = {pre + "_Hpp": Hpp, pre + "_b": b}
    if hll:
        o[pre + "_Hll"] = Hll
    if hpl:
        o[pre + "_Hpl"] = Hpl
    return o


# ================================================================================================ EdgeSE3Prior
def gen_prior3(rng):
    out, orc, cov = {}, {}, {}
    nP = 40
    mags = 10.0 ** np.linspace(-3, 3, nP)
    poses = np.array([G.rand_iso(rng, mags[v]) for v in range(nP)])
    hidx = np.arange(nP, dtype=np.int32) - 1                      # pose 0 fixed
    off = G.pack(G.axis_angle_R([0.3, -1.0, 0.5], 2.1), [0.4, -0.2, 1.1])
    ev = np.arange(nP - 1, dtype=np.int32)
    Zodo = np.array([G.mul_np(G.inv_np(poses[k]), poses[k + 1]) for k in range(nP - 1)])
    out.update(prior3_poses=poses, prior3_hidx=hidx, prior3_offset=off, prior3_vi=ev, prior3_vj=ev + 1, prior3_Zodo=Zodo)

    def rotations(n, full):
        R, tag = [], []
        for _ in range(60 if full else 20):
            R.append(G.axis_angle_R(rng.normal(size=3), np.deg2rad(rng.uniform(0, 179)))); tag.append("uniform")
        for i in range(3):
            for sgn in (1, -1):
                for _ in range(MIN_PER_COMBO + 2 if full else 3):
                    a = rng.normal(size=3) * 0.3
                    a[i] = sgn * (1.0 + abs(a[i]))
                    R.append(G.axis_angle_R(a, np.deg2rad(rng.uniform(125, 179)))); tag.append("case%d%s" % (i + 1, "+-"[sgn < 0]))
        for _ in range(24 if full else 4):
            tr = rng.choice([-1, 1]) * 1e-3 * rng.uniform(0.02, 1)
            R.append(G.axis_angle_R(rng.normal(size=3), np.arccos((tr - 1) / 2))); tag.append("tr~0")
        for _ in range(24 if full else 4):
            i, j = rng.choice(3, 2, replace=False)
            a = np.abs(rng.normal(size=3)) * 0.2
            a[i] = 1.0
            a[j] = np.sqrt(1.0 + rng.choice([-1, 1]) * 1e-3 * rng.uniform(0.02, 1))
            a *= rng.choice([-1, 1], 3)
            R.append(G.axis_angle_R(a, np.deg2rad(rng.uniform(150, 179)))); tag.append("diag~")
        while len(R) < n - 2:
            R.append(G.axis_angle_R(rng.normal(size=3), np.deg2rad(rng.uniform(0, 179)))); tag.append("fill")
        order = rng.permutation(len(R))
        return [R[i] for i in order] + [None, None], [tag[i] for i in order] + ["identity", "identity"]

    for pre, n, P in (("prior3", N, off), ("prior3n", 64, None)):
        Pm = IDENT if P is None else P
        Rs, tag = rotations(n, P is not None)
        vq = (1 + np.arange(n) % (nP - 1)).astype(np.int32)
        vq[5] = 0                                                 # one prior on the fixed pose
        Z = np.zeros((n, 12))
        for k in range(n):
            X = poses[vq[k]]
            if Rs[k] is None:                                     # the identity error
                if P is None and k == n - 1:                      # ... exactly: R = I in pose and measurement, the same t
                    X = G.pack(np.eye(3), np.array([3.0, -2.0, 0.5]))
                    vq[k] = nP                                    # (a pose of its own, appended below)
                Z[k] = G.mul_np(X, Pm) if P is not None else X.copy()
                continue
            E = G.pack(Rs[k], rng.normal(size=3) * mags[vq[k]] * 0.1)
            Z[k] = G.mul_np(G.mul_np(X, Pm), G.inv_np(E))         # Z^-1 X P = E up to rounding
        tbl, hx = poses, hidx
        if P is None:
            tbl = np.concatenate([poses, G.pack(np.eye(3), np.array([3.0, -2.0, 0.5]))[None]])
            hx = np.concatenate([hidx, [nP - 1]]).astype(np.int32)
            out.update(prior3n_poses=tbl, prior3n_hidx=hx)
        J0, err, case, sign, eops, jops = [], [], [], [], [], []
        for k in range(n):
            a, _, e = M.se3_prior_edge(tbl[vq[k]], Z[k], Pm)
            w = M.se3_prior_quat_w(M.iso(tbl[vq[k]]), M.iso(Z[k]), M.iso(Pm))
            assert w >= 0.008, (pre, k, tag[k], float(w))
            c, s, tr, gap = PM.se3_branch(IDENT, G.mul_np(tbl[vq[k]], Pm), Z[k])
            if tag[k] == "tr~0":
                assert abs(tr) < 2e-3
            if tag[k] == "diag~":
                assert c > 0 and gap < 2e-3, (k, c, gap)
            J0.append(M.f64(a)); err.append(M.f64(e)); case.append(c); sign.append(s)
            t = max(G.tmax(tbl[vq[k]], Z[k]), float(np.abs(Pm[9:]).max()))
            eops.append([t, t, t, 1.0, 1.0, 1.0])
            tp = max(1.0, 2.0 * float(np.abs(Pm[9:]).max()))
            jops.append([tp, tp, tp, 1.0, 1.0, 1.0])
        case, sign = np.array(case, np.int32), np.array(sign, np.int32)
        c = {}
        for cc in range(4):
            for s in (1, -1):
                cnt = int(((case == cc) & (sign == s)).sum())
                if cc == 0 and s == -1:
                    assert cnt == 0
                    continue
                assert cnt >= (MIN_PER_COMBO if P is not None else 1), (pre, cc, s, cnt)
                c["case%d/qw%s" % (cc, "+" if s > 0 else "-")] = cnt
        if P is not None:
            assert sum(t == "tr~0" for t in tag) == 24 and sum(t == "diag~" for t in tag) == 24
            assert sum(t == "uniform" for t in tag) == 60
            trs = [PM.se3_branch(IDENT, G.mul_np(tbl[vq[k]], Pm), Z[k])[2] for k in range(n) if tag[k] == "tr~0"]
            assert min(trs) < 0 < max(trs)
            c["tr~0"], c["diag~"], c["uniform"] = 24, 24, 60
            c["t_min"], c["t_max"] = float(mags.min()), float(mags.max())
        else:
            E = G.mul_np(G.inv_np(Z[n - 1]), tbl[vq[n - 1]])
            assert np.array_equal(E, IDENT)                       # the exact identity
            c["identity_exact"] = 1
        c["identity"] = 2
        c["on_fixed_pose"] = int((hx[vq] < 0).sum())
        c["most_priors_on_one_pose"] = int(np.bincount(vq).max())
        assert c["on_fixed_pose"] == 1 and c["most_priors_on_one_pose"] >= 2 and hx[vq[0]] >= 0
        cov[pre] = c
        out.update({pre + "_vq": vq, pre + "_Z": Z, pre + "_J0": np.array(J0), pre + "_err": np.array(err), pre + "_case": case,
                    pre + "_sign": sign, pre + "_err_ops": scales(eops), pre + "_J0_ops": scales(jops),
                    pre + "_boundary": np.array([t in ("tr~0", "diag~", "identity") for t in tag])})
        oJ, oe = PH.se3_prior_edges(tbl, vq, Z, P)
        orc.update({pre + "_J0": oJ, pre + "_err": oe})
        if P is not None:                                         # the assembled unary path: full SPD 6 x 6 information
            W = spd(rng, n, 6)
            pr = Products(nP - 1, 0, n)
            for k in range(n):
                a, _, e = M.se3_prior_edge(tbl[vq[k]], Z[k], Pm)
                pr.add(k, a, None, e, W[k], mp.mpf(1), hx[vq[k]], -1, np.maximum(np.abs(err[k]), eops[k]))
            out.update(pr.out(pre, hll=False), prior3_omega=W)
            orc.update(products_fp64(pre, oJ, None, oe, W, np.ones(n), hx[vq], None, nP - 1, 0, hll=False))
    return out, orc, cov


# ================================================================================================ EdgeSE2Prior / XYPrior
def gen_prior2(rng):
    pi = np.pi
    out, orc, cov = {}, {}, {}
    nP = 40
    th = rng.uniform(-pi, pi, nP)
    th[2], th[3] = pi / 2, -pi / 2
    th[36:40] = [4321.5, -15000.25, 9876.0, -2222.75]             # estimates thousands of radians out
    poses = np.column_stack([rng.normal(size=(nP, 2)) * 10.0 ** rng.uniform(-1, 2, (nP, 1)), th])
    assert not np.isin(np.abs(poses[:, 2]), [pi]).any()
    hidx = np.arange(nP, dtype=np.int32) - 1
    vq = (1 + np.arange(N) % (nP - 1)).astype(np.int32)
    vq[5] = 0
    tz = rng.uniform(-pi, pi, N)
    far = rng.choice(np.arange(10, N), 30, replace=False)
    tz[far] = rng.choice([-1, 1], 30) * rng.uniform(1e3, 2e4, 30)
    exact = [7, 8, 9, 100, 200, 254, 300, 400]
    tz[exact] = [pi, -pi, pi, -pi, pi, -pi, pi, -pi]              # -theta_z exactly on -M_PI / M_PI
    z = np.column_stack([poses[vq, :2] + rng.normal(size=(N, 2)) * 0.5, tz])
    br, sides, hits = {}, dict(above=0, below=0), 0
    for k in range(N):
        e = M.se2_prior_error(M.V(poses[vq[k]]), M.V(z[k]))
        if abs(abs(e[2]) - M.PI64) < 1e-3:                        # final angle too close to the jump: move the measurement
            assert k not in exact
            z[k, 2] += 0.01
            e = M.se2_prior_error(M.V(poses[vq[k]]), M.V(z[k]))
        assert abs(abs(e[2]) - M.PI64) >= 1e-3
        for raw in (-z[k, 2], poses[vq[k], 2]):
            if abs(raw) > pi:                                      # reduced angles keep 1e-6 from the switch points
                s = mp.mpf(float(raw))
                frac = s / (2 * M.PI64) - mp.floor(s / (2 * M.PI64))
                assert 1e-6 < frac < 1 - 1e-6 and abs(frac - 0.5) > 1e-6
        a = PM.wrap_branch(-z[k, 2])
        nz = float(M.normalize_theta(mp.mpf(float(-z[k, 2]))))
        sm = nz + poses[vq[k], 2]
        d = PM.wrap_branch(sm)
        br["inv:" + a] = br.get("inv:" + a, 0) + 1
        br["mul:" + d] = br.get("mul:" + d, 0) + 1
        hits += int(-z[k, 2] in (pi, -pi))
        assert sm not in (pi, -pi)
        if abs(sm) < 2 * pi:
            sides["above"] += int(sm >= pi)
            sides["below"] += int(sm < -pi)
    assert hits >= 6 and sides["above"] >= 10 and sides["below"] >= 10, (hits, sides)
    assert br.get("inv:floor", 0) + br.get("inv:floor+hi", 0) >= 10 and br.get("mul:floor", 0) + br.get("mul:floor+hi", 0) >= 10
    nfar = int(((np.abs(z[:, 2]) > 1e3) | (np.abs(poses[vq, 2]) > 1e3)).sum())
    assert nfar >= 30
    J0, err, eops, jops = [], [], [], []
    for k in range(N):
        a, _, e = M.se2_prior_edge(poses[vq[k]], z[k])
        J0.append(M.f64(a)); err.append(M.f64(e))
        t = max(np.abs(poses[vq[k], :2]).max(), np.abs(z[k, :2]).max())
        t *= max(1.0, abs(z[k, 2]))       # (Rz' multiplies them: a measurement angle of 1e4 rad holds these rows 1e4 times more loosely)
        eops.append([t, t, max(abs(poses[vq[k], 2]), abs(z[k, 2]))])
        jops.append([max(1.0, abs(z[k, 2]))] * 2 + [1.0])
    ev = np.arange(nP - 1, dtype=np.int32)
    Zodo = np.array([M.f64(M.se2_mul(M.se2_inv(M.V(poses[k])), M.V(poses[k + 1]))) for k in range(nP - 1)])
    out.update(prior2_poses=poses, prior2_hidx=hidx, prior2_vq=vq, prior2_Z=z, prior2_vi=ev, prior2_vj=ev + 1, prior2_Zodo=Zodo,
               prior2_J0=np.array(J0), prior2_err=np.array(err), prior2_err_ops=scales(eops), prior2_J0_ops=scales(jops),
               prior2_far=(np.abs(z[:, 2]) > 1e3) | (np.abs(poses[vq, 2]) > 1e3),
               prior2_exact=np.isin(np.arange(N), exact))
    oJ, oe = PH.se2_prior_edges(poses, vq, z)
    orc.update(prior2_J0=oJ, prior2_err=oe)
    cov["prior2"] = dict(br, exactly_on_M_PI=hits, far_angles=nfar, sum_above_pi=sides["above"], sum_below_minus_pi=sides["below"],
                         on_fixed_pose=int((hidx[vq] < 0).sum()))
    # ---- EdgeSE2XYPrior: bit for bit (J constants, err one IEEE subtraction)
    pos = rng.normal(size=(nP, 2)) * 10.0 ** np.linspace(-2, 4, nP)[:, None]
    p2 = np.column_stack([pos, rng.uniform(-pi, pi, nP)])
    zxy = p2[vq, :2] + rng.normal(size=(N, 2)) * np.abs(p2[vq, :2]) * 10.0 ** rng.uniform(-6, 0, (N, 1))
    J0, err = [], []
    for k in range(N):
        a, _, e = M.se2_xy_prior_edge(p2[vq[k]], zxy[k])
        J0.append(M.f64(a)); err.append(M.f64(e))
    J0, err = np.array(J0), np.array(err)
    oJ, oe = PH.se2_xy_prior_edges(p2, vq, zxy)
    assert np.array_equal(oJ, J0) and np.array_equal(oe, err)
    Zo2 = np.array([M.f64(M.se2_mul(M.se2_inv(M.V(p2[k])), M.V(p2[k + 1]))) for k in range(nP - 1)])
    out.update(prior2xy_poses=p2, prior2xy_Z=zxy, prior2xy_Zodo=Zo2, prior2xy_J0=J0, prior2xy_err=err)
    cov["prior2xy"] = dict(pos_min=float(np.abs(pos).min()), pos_max=float(np.abs(pos).max()), bitwise=1)
    return out, orc, cov


# ================================================================================================ depth / disparity
def camera_ops(poses, points, vp, vl, meas, offset, kcam, disparity):
    """ops rows of err, J0, J1 from the fp64 intermediates (the formulas of the module docstring)."""
    R, t = CH._iso(np.asarray(poses)[vp], np.float64)
    Ro, to = CH._iso(offset, np.float64)
    Ro, to = Ro[0], to[0]
    fx, fy, cx, cy = kcam
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    l = np.asarray(points)[vl]
    q = np.einsum("nji,nj->ni", R @ Ro, l - (np.einsum("nij,j->ni", R, to) + t))
    p = np.einsum("ij,nj->ni", K, q)
    p2 = p[:, 2]
    third = 1 / p2 if disparity else p2
    val = np.stack([p[:, 0] / p2, p[:, 1] / p2, third], axis=1)
    eops = np.maximum(np.abs(meas), np.abs(val))
    eops[:, 0] = np.maximum(eops[:, 0], np.maximum(np.abs(fx * q[:, 0] / p2), abs(cx)))
    eops[:, 1] = np.maximum(eops[:, 1], np.maximum(np.abs(fy * q[:, 1] / p2), abs(cy)))
    n = len(vp)
    Zl = np.einsum("nji,nj->ni", R, l - t)
    J = np.zeros((n, 3, 9))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = -1
    J[:, 0, 4], J[:, 0, 5] = -2 * Zl[:, 2], 2 * Zl[:, 1]
    J[:, 1, 3], J[:, 1, 5] = 2 * Zl[:, 2], -2 * Zl[:, 0]
    J[:, 2, 3], J[:, 2, 4] = -2 * Zl[:, 1], 2 * Zl[:, 0]
    J[:, :, 6:9] = R.transpose(0, 2, 1)
    Jp = np.einsum("ij,njk->nik", K @ Ro.T, J)
    P2 = p2[:, None, None]
    T = np.empty((n, 3, 9))
    T[:, 0:2, :] = np.maximum(np.abs(Jp[:, 0:2, :] * P2), np.abs(p[:, 0:2, None] * Jp[:, 2:3, :])) / (P2 * P2)
    T[:, 2, :] = np.abs(Jp[:, 2, :]) / ((p2 * p2)[:, None] if disparity else 1.0)
    return eops, T[:, :, 0:6].max(axis=2), T[:, :, 6:9].max(axis=2), p, np.abs(l).max(axis=1) / np.abs(p2)


def gen_camera(rng):
    out, orc, cov = {}, {}, {}
    nP, nL = 40, 60
    kcam = np.array([520.9, 480.3, 325.1, 249.7])                 # fx != fy
    off = G.pack(G.axis_angle_R([0.3, -1.0, 0.5], 2.1), [0.4, -0.2, 1.1])
    base = G.pack(G.axis_angle_R([0.2, 1.0, -0.4], 1.3), [9.0, -12.0, 6.0])
    poses = []
    for v in range(nP):                                           # a tight cluster: every pose sees every landmark at its depth
        d = G.pack(G.axis_angle_R(rng.normal(size=3), rng.uniform(0, 0.002)), rng.normal(size=3) * 0.0005)
        poses.append(base if v == 1 else G.mul_np(base, d))
    poses = np.array(poses)
    n2w = G.mul_np(base, off)
    Rn, tn = n2w[:9].reshape(3, 3).T, n2w[9:]
    pts = np.zeros((nL, 3))
    nominal = np.zeros(nL)
    for i in range(nL):                                           # 40 in front, 20 behind; |depth| log-spaced 0.05 .. 50
        front = i < 40
        m, j = (40, i) if front else (20, i - 40)
        d = 0.054 * (50.0 / 0.054) ** (j / (m - 1.0))
        d = d if front else -d
        wide = i % 3 == 0                                         # a third well outside the image, up to three widths out
        u = rng.choice([-1, 1], 2) * (rng.uniform(1.5, 3.6, 2) if wide else rng.uniform(0, 0.3, 2))
        pts[i] = Rn @ np.array([u[0] * d, u[1] * d, d]) + tn
        nominal[i] = d
    first = 1 * nL + 5                                            # edge 0: a free pose and a free landmark
    rest = rng.permutation(nP * nL)
    pairs = np.concatenate([[first], rest[rest != first][:N - 1]])
    vp, vl = (pairs // nL).astype(np.int32), (pairs % nL).astype(np.int32)
    hidx = np.arange(nP, dtype=np.int32) - 1                      # pose 0 fixed
    pt_hidx = (nP - 1) + np.arange(nL, dtype=np.int32) - 3        # landmarks 0..2 fixed
    pt_hidx[:3] = -1
    ev = np.arange(nP - 1, dtype=np.int32)
    Zodo = np.array([G.mul_np(G.inv_np(poses[k]), poses[k + 1]) for k in range(nP - 1)])
    W = spd(rng, N, 3)
    out.update(cam_poses=poses, cam_points=pts, cam_hidx=hidx, cam_pt_hidx=pt_hidx, cam_vp=vp, cam_vl=vl, cam_offset=off, cam_kcam=kcam,
               cam_vi=ev, cam_vj=ev + 1, cam_Zodo=Zodo, cam_omega=W)
    noise = rng.normal(size=(N, 3))
    for pre, disparity in (("depth", False), ("disparity", True)):
        _, _, _, p, ratio = camera_ops(poses, pts, vp, vl, np.zeros((N, 3)), off, kcam, disparity)
        p2 = p[:, 2]
        assert np.abs(p2).min() >= 0.05 and ratio.max() <= CAP, (np.abs(p2).min(), ratio.max())
        val = np.stack([p[:, 0] / p2, p[:, 1] / p2, 1 / p2 if disparity else p2], axis=1)
        zl = val + noise * np.stack([np.full(N, 0.5), np.full(N, 0.5), 0.01 * np.abs(val[:, 2])], axis=1)
        eops, j0ops, j1ops, _, _ = camera_ops(poses, pts, vp, vl, zl, off, kcam, disparity)
        outside = (val[:, 0] < 0) | (val[:, 0] > WIDTH) | (val[:, 1] < 0) | (val[:, 1] > HEIGHT)
        tag = np.where(p2 < 0, 2, np.where(outside, 1, 0)).astype(np.int32)      # 0 front inside, 1 front outside, 2 behind
        J0, J1, err, Jm = [], [], [], []
        for k in range(N):
            a, b, e = M.camera_edge(poses[vp[k]], pts[vl[k]], zl[k], off, kcam, disparity)
            J0.append(M.f64(a)); J1.append(M.f64(b)); err.append(M.f64(e)); Jm.append((a, b, e))
        c = dict(front_inside=int((tag == 0).sum()), front_outside=int((tag == 1).sum()), behind=int((tag == 2).sum()),
                 behind_points=int((nominal < 0).sum()), outside=int(outside.sum()), min_abs_p2=float(np.abs(p2).min()),
                 max_abs_p2=float(np.abs(p2).max()), max_l_over_p2=float(ratio.max()),
                 max_widths_out=float(np.abs(val[:, 0] - kcam[2]).max() / WIDTH),
                 fixed_pose_edges=int((hidx[vp] < 0).sum()), fixed_landmark_edges=int((pt_hidx[vl] < 0).sum()))
        assert c["behind_points"] >= 20 and c["behind"] >= 20 and c["outside"] >= N // 4 and c["front_inside"] >= 100
        assert c["fixed_pose_edges"] > 0 and c["fixed_landmark_edges"] > 0 and c["min_abs_p2"] < 0.06 and c["max_abs_p2"] > 45
        assert hidx[vp[0]] >= 0 and pt_hidx[vl[0]] >= 0
        cov[pre] = c
        out.update({pre + "_zl": zl, pre + "_J0": np.array(J0), pre + "_J1": np.array(J1), pre + "_err": np.array(err),
                    pre + "_err_ops": scales(eops), pre + "_J0_ops": scales(j0ops), pre + "_J1_ops": scales(j1ops), pre + "_tag": tag})
        oJ0, oJ1, oe = CH.camera_edges(poses, pts, vp, vl, zl, off, kcam, disparity)
        orc.update({pre + "_J0": oJ0, pre + "_J1": oJ1, pre + "_err": oe})
        if disparity:                                             # the assembled landmark path: full SPD 3 x 3 information
            nPf, nLf = nP - 1, nL - 3
            pr = Products(nPf, nLf, N)
            hl = np.where(pt_hidx[vl] >= 0, pt_hidx[vl] - nPf, -1)
            for k in range(N):
                a, b, e = Jm[k]
                pr.add(k, a, b, e, W[k], mp.mpf(1), hidx[vp[k]], hl[k], np.maximum(np.abs(err[k]), eops[k]))
            out.update(pr.out(pre))
            orc.update(products_fp64(pre, oJ0, oJ1, oe, W, np.ones(N), hidx[vp], hl, nPf, nLf))
    return out, orc, cov


# ================================================================================================ stereo
def stereo_ops(cams, pts, cam_idx, pt_idx, meas, f, cx, cy, b):
    T, X = cams[cam_idx], pts[pt_idx]
    R = T[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    Xc = np.einsum("nij,nj->ni", R, X) + T[:, 9:]
    x, y, z = np.abs(Xc[:, 0]), np.abs(Xc[:, 1]), np.abs(Xc[:, 2])
    xb = np.maximum(x, abs(b))
    am = np.abs(meas)
    eops = np.stack([np.maximum.reduce([am[:, 0], f * x / z, np.full(len(x), abs(cx))]),
                     np.maximum.reduce([am[:, 1], f * y / z, np.full(len(x), abs(cy))]),
                     np.maximum.reduce([am[:, 2], f * x / z, f * abs(b) / z, np.full(len(x), abs(cx))])], axis=1)
    z2 = z * z
    j1 = np.stack([np.maximum.reduce([f * (1 + x * x / z2), f * x * y / z2, f * y / z]),
                   np.maximum.reduce([f * (1 + y * y / z2), f * x * y / z2, f * x / z]),
                   np.maximum.reduce([f * (1 + x * xb / z2), f * xb * y / z2, f * y / z, f * xb / z2])], axis=1)
    aR = np.abs(R)
    tmp = np.zeros((len(x), 3, 3))
    tmp[:, 0, 0] = tmp[:, 1, 1] = tmp[:, 2, 0] = f
    tmp[:, 0, 2], tmp[:, 1, 2], tmp[:, 2, 2] = f * x / z, f * y / z, f * xb / z
    j0 = (tmp[:, :, :, None] * aR[:, None, :, :]).max(axis=(2, 3)) / z[:, None]
    return eops, j0, j1


def gen_stereo(rng):
    out, orc, cov = {}, {}, {}
    cams, pts, cam_idx, pt_idx = [], [], [], []
    for centre, ncam, npt, dlo, dhi in ((np.zeros(3), 12, 34, 0.02, 50.0), (np.array([8e3, -1e4, 6e3]), 5, 21, 600.0, 3000.0)):
        c0, p0 = len(cams), len(pts)
        for c in range(ncam):
            R = G.axis_angle_R(rng.normal(size=3), rng.uniform(0, 0.002 if dlo < 1 else 0.05)) @ G.axis_angle_R([0.2, 1.0, -0.4], 1.3)
            pos = centre + rng.normal(size=3) * (0.0005 if dlo < 1 else 3.0)
            cams.append(G.pack(R, -R @ pos))
        Rm = cams[c0][:9].reshape(3, 3).T
        for p in range(npt):
            d = dlo * (dhi / dlo) ** (p / (npt - 1.0))
            u = rng.uniform(-1, 1, 2) * ((12.0 if dlo < 1 else 2.0) if p % 3 == 0 else 0.3)
            X = Rm.T @ (np.array([u[0] * d, u[1] * d, d]) - cams[c0][9:])
            pts.append(X)
            for c in range(ncam):
                cam_idx.append(c0 + c); pt_idx.append(p0 + p)
    cams, pts = np.array(cams), np.array(pts)
    assert len(cam_idx) == N
    order = np.concatenate([[0], 1 + rng.permutation(N - 1)])
    cam_idx, pt_idx = np.array(cam_idx, np.int32)[order], np.array(pt_idx, np.int32)[order]
    P, L = len(cams), len(pts)
    cam_hidx = np.full(P, -1, np.int32)
    free = [c for c in range(P) if c not in (1, 13)]              # one fixed camera per cluster
    cam_hidx[free] = np.arange(len(free), dtype=np.int32)
    nP = len(free)
    pt_hidx = np.full(L, -1, np.int32)
    freep = [p for p in range(L) if p not in (3, 7, 40)]          # three fixed points
    pt_hidx[freep] = np.arange(len(freep), dtype=np.int32)
    nL = len(freep)
    assert cam_hidx[cam_idx[0]] >= 0 and pt_hidx[pt_idx[0]] >= 0 and P <= 40 and L <= 60
    unit = rng.normal(size=(N, 3))
    # Gross errors and the per-edge (kind, delta) table.  An edge whose projection lies further than f from the principal point
    # under the first intrinsics set (the near points seen with the 0.5 baseline: f b / z up to 25 f), and every edge of the
    # far cluster, must carry a large error (module docstring) and is an outlier of every delta; the others are inliers of
    # every delta.  Kinds and deltas cycle over each of the two classes by rank, so that every (kind, delta) group keeps
    # edges on both sides of its threshold in a head of 257 edges too.
    f0, cx0, cy0, b0 = STEREO_SETS[0]
    proj0 = -SH.stereo_edges(cams, pts, cam_idx, pt_idx, np.zeros((N, 3)), f0, cx0, cy0, b0, jac=False)
    forced = (np.abs(proj0 - np.array([cx0, cy0, cx0])).max(axis=1) > f0) | (cam_idx >= 12)
    basemag = np.where(forced, 30.0, 0.25)
    rank = np.where(forced, np.cumsum(forced) - 1, np.cumsum(~forced) - 1)
    rk_kinds = np.where(forced, rank % 6, 1 + rank % 5).astype(np.int32)
    rk_deltas = np.array([1.5, 2.5])[np.where(forced, rank // 6, rank // 5) % 2]
    rk_deltas[rk_kinds == 0] = 1.0
    Wfull = spd(rng, N, 3) / 4.0
    Weye = np.tile(np.eye(3).reshape(9), (N, 1))
    out.update(st_cams=cams, st_pts=pts, st_cam_idx=cam_idx, st_pt_idx=pt_idx, st_cam_hidx=cam_hidx, st_pt_hidx=pt_hidx, st_sets=STEREO_SETS,
               st_rk_kinds=rk_kinds, st_rk_deltas=rk_deltas, st_omega=Wfull,
               st_set_deltas=np.array([SET_DELTA[k] for k in range(1, 6)]))
    hp, hl = cam_hidx[cam_idx], pt_hidx[pt_idx]
    for si, (f, cx, cy, b) in enumerate(STEREO_SETS):
        pre = "st%d" % si
        meas = np.zeros((N, 3))
        J0, J1, err, Jm = [], [], [], []
        zmin, ratio = 1e300, 0.0
        fm = [mp.mpf(float(v)) for v in (f, cx, cy, b)]
        for k in range(N):
            T, X = cams[cam_idx[k]], pts[pt_idx[k]]
            pc = M.camera_point(M.iso(T), M.V(X))
            zmin, ratio = min(zmin, float(pc[2])), max(ratio, float(np.abs(X).max() / pc[2]))
            assert pc[2] > 0 and np.abs(X).max() / pc[2] <= 25
            proj = -np.array(M.f64(M.stereo_error(M.iso(T), M.V(X), [0, 0, 0], *fm)))
            fu = max(abs(proj[0] - cx), abs(proj[1] - cy), abs(proj[2] - cx))
            if cam_idx[k] >= 12:
                fu = max(fu, 1.001 * f)
            meas[k] = proj + unit[k] * max(basemag[k], 0.2 * fu if fu > f else 0.0)
            a, bb, e = M.stereo_edge(T, X, meas[k], f, cx, cy, b)
            J0.append(M.f64(a)); J1.append(M.f64(bb)); err.append(M.f64(e)); Jm.append((a, bb, e))
        eops, j0ops, j1ops = stereo_ops(cams, pts, cam_idx, pt_idx, meas, f, cx, cy, b)
        out.update({pre + "_meas": meas, pre + "_J0": np.array(J0), pre + "_J1": np.array(J1), pre + "_err": np.array(err),
                    pre + "_err_ops": scales(eops), pre + "_J0_ops": scales(j0ops), pre + "_J1_ops": scales(j1ops)})
        oJ0, oJ1, oe = SH.stereo_edges(cams, pts, cam_idx, pt_idx, meas, f, cx, cy, b)
        orc.update({pre + "_J0": oJ0, pre + "_J1": oJ1, pre + "_err": oe})
        # ---- chi2 that rides along: robust kinds 0-5 as the set's kernel and per edge, identity and full information
        chi, chi_ops, chi_o = np.zeros((2, len(CONFIGS), len(CHI_N))), np.zeros((2, len(CONFIGS), len(CHI_N))), np.zeros((2, len(CONFIGS), len(CHI_N)))
        sides, weights = {}, {}
        for wi, (wname, W) in enumerate((("I", Weye), ("W", Wfull))):
            e2 = []
            for k in range(N):
                e = Jm[k][2]
                e2.append(sum(e[i] * mp.mpf(float(W[k, i + 3 * j])) * e[j] for i in range(3) for j in range(3)))
            Wm = W.reshape(N, 3, 3)
            e2f = np.einsum("ni,nji,nj->n", oe, Wm, oe)
            for ci, cfg in enumerate(CONFIGS):
                kinds = rk_kinds if cfg == "edge" else np.full(N, 0 if cfg == "none" else int(cfg[3:]), np.int32)
                deltas = rk_deltas if cfg == "edge" else np.array([SET_DELTA.get(int(kk), 1.0) for kk in kinds])
                rw = [M.robust(int(kinds[k]), deltas[k], e2[k]) for k in range(N)]
                ro = [O.robustify(int(kinds[k]), deltas[k], e2f[k]) if kinds[k] > 0 else (e2f[k], 1.0, 0.0) for k in range(N)]
                weights[(wname, cfg)] = ([r[1] for r in rw], np.array([r[1] for r in ro]))
                for ni, n in enumerate(CHI_N):
                    chi[wi, ci, ni] = float(sum(r[0] for r in rw[:n]))
                    chi_ops[wi, ci, ni] = float(sum(abs(r[0]) for r in rw[:n]))
                    chi_o[wi, ci, ni] = sum(r[0] for r in ro[:n])
                    for k in range(n):
                        if kinds[k] == 0:
                            continue
                        d2 = mp.mpf(float(deltas[k])) ** (1 if kinds[k] == 5 else 2)      # (DCS switches at e2 = phi)
                        if kinds[k] in (1, 4):
                            assert abs(e2[k] / d2 - 1) > 1e-6
                        s = "%s:%s:n%d:k%d:d%g:%s" % (wname, cfg, n, kinds[k], deltas[k], "<=" if e2[k] <= d2 else ">")
                        sides[s] = sides.get(s, 0) + 1
        keys = set(s.rsplit(":", 1)[0] for s in sides)
        for s in keys:
            assert sides.get(s + ":<=", 0) >= 5 and sides.get(s + ":>", 0) >= 5, (s, sides.get(s + ":<="), sides.get(s + ":>"))
        assert len(keys) == 2 * len(CHI_N) * (5 + 10)
        out.update({pre + "_chi2": chi, pre + "_chi2_ops": chi_ops})
        orc[pre + "_chi2"] = chi_o
        # ---- the assembled system of this set
        if si not in ASSEMBLED:
            cov[pre] = dict(edges=N, min_depth=zmin, max_X_over_depth=ratio, min_side=min(sides.values()), robust_groups=len(keys))
            continue
        cfg, wname = ASSEMBLED[si]
        W = Weye if wname == "I" else Wfull
        wm, wo = weights[(wname, cfg)]
        pr = Products(nP, nL, N)
        for k in range(N):
            a, bb, e = Jm[k]
            pr.add(k, bb, a, e, W[k], wm[k], hp[k], hl[k], np.maximum(np.abs(err[k]), eops[k]))
        out.update(pr.out(pre, hpl=True))
        out[pre + "_w"] = G.f64(wm)
        orc.update(products_fp64(pre, oJ1, oJ0, oe, W, wo, hp, hl, nP, nL, hpl=True))
        cov[pre] = dict(edges=N, min_depth=zmin, max_X_over_depth=ratio, fixed_cameras=int((cam_hidx < 0).sum()),
                        fixed_points=int((pt_hidx < 0).sum()), fixed_camera_edges=int((hp < 0).sum()), fixed_point_edges=int((hl < 0).sum()),
                        min_side=min(sides.values()), robust_groups=len(keys), zero_weights=int(sum(1 for v in wm if v == 0)))
        assert cov[pre]["fixed_cameras"] == 2 and cov[pre]["fixed_points"] == 3 and cov[pre]["fixed_point_edges"] > 0
    return out, orc, cov


ROW_KEYS = {"prior3": (("J0", 6), ("err", 6)), "prior3n": (("J0", 6), ("err", 6)), "prior2": (("J0", 3), ("err", 3)),
            "depth": (("J0", 3), ("J1", 3), ("err", 3)), "disparity": (("J0", 3), ("J1", 3), ("err", 3)),
            "st0": (("J0", 3), ("J1", 3), ("err", 3)), "st1": (("J0", 3), ("J1", 3), ("err", 3))}
BLOCK_KEYS = {"prior3": ("Hpp", "b"), "disparity": ("Hpp", "Hll", "b"), "st0": ("chi2",),
              "st1": ("Hpl", "Hpp", "Hll", "b", "chi2")}


def block_figure(key, got, out):
    ref, ops = out[key], out[key + "_ops"]
    if key.endswith("_b") or key.endswith("_chi2"):
        ref, ops, got = np.asarray(ref).reshape(-1, 1), np.asarray(ops).reshape(-1), np.asarray(got).reshape(-1, 1)
    return PM.worst(got, ref, ops)[0]


def main():
    rng = np.random.RandomState(20241020)
    fx, figures, coverage = {}, {}, {}
    for name, gen in (("prior3", gen_prior3), ("prior2", gen_prior2), ("camera", gen_camera), ("stereo", gen_stereo)):
        out, orc, cov = gen(rng)
        fx.update(out)
        coverage[name] = cov
        for pre, keys in ROW_KEYS.items():
            for what, d in keys:
                key = pre + "_" + what
                if key in orc:
                    figures[key] = PM.worst_row(orc[key], out[key], out[key + "_ops"], d)[0]
        for pre, keys in BLOCK_KEYS.items():
            for what in keys:
                key = pre + "_" + what
                if key in orc:
                    figures[key] = block_figure(key, orc[key], out)
        print(name, json.dumps(cov))
    coverage["tails"] = list(TAILS)
    lines = []
    for key in sorted(figures):
        assert figures[key] > 0 or key in FLOORS, (key, figures[key])
        floor = FLOORS.get(key, 0) if figures[key] == 0 else 0
        fx["oracle_" + key] = np.float64(figures[key])
        fx["floor_" + key] = np.float64(floor)
        lines.append(dict(output=key, who="oracle_fp64_vs_mp60", worst=figures[key], floor_eps=floor,
                          bound=PM.MARGIN * figures[key] if figures[key] > 0 else floor * PM.EPS))
        print("%-16s restatement %.3e  bound %.3e" % (key, figures[key], lines[-1]["bound"]))
    for key in sorted(figures):      # a restatement that cannot stay a factor MARGIN below the ceiling: move the input
        assert PM.MARGIN * figures[key] <= PM.CEILING, (key, figures[key])
    fx["coverage_json"] = np.array(json.dumps(coverage, sort_keys=True))
    np.savez_compressed(OUT, **fx)
    keep = []
    if os.path.exists(PROFILE):
        keep = [l for l in open(PROFILE).read().splitlines() if l.strip() and json.loads(l).get("who") != "oracle_fp64_vs_mp60"]
    with open(PROFILE, "w") as fh:
        for l in lines:
            fh.write(json.dumps(l) + "\n")
        for l in keep:
            fh.write(l + "\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
