"""Writes tests/golden/producer_edges.npz: fp64 inputs that take every data-dependent branch of the device producers and
vertex updates, the extended-precision reference results (tests/reference_mp.py) rounded to fp64, and per group and output
the worst per-edge error (tests/producer_metric.py) of the CPU oracle's fp64 evaluation against that reference.  Run from
the repository root:  python tests/golden/make_producer_edges.py   (deterministic; about ten seconds).

Exclusions, all by construction of the inputs and asserted below:
  * EdgeSE3 error rotations stay <= 179 degrees (w >= 0.008): toVectorMQT's w >= 0 convention is discontinuous at 180.
  * The FINAL angle of an EdgeSE2 error keeps 1e-3 rad from +-pi (the central difference would straddle the jump of
    normalize_theta); the INTERMEDIATE sums sit on both sides of +-pi and exactly on it, which is harmless: a different
    side there changes the intermediate by 2 pi and nothing after it.
  * Angles that normalize_theta reduces keep 1e-6 from the switch points unless they sit exactly on one where fp64 and the
    reference agree (theta == M_PI, theta == -M_PI).
  * |u_q|^2 of a VertexSE3 update keeps 1e-3 from 1 unless it is exactly 1; theta of a camera update keeps a relative 1e-6
    from 0.00001; e2 of an edge whose error a device producer computes keeps a relative 1e-6 from delta^2.
  * BA points keep |X| / depth <= 25: z = R X + t cancels |X| down to the depth, and the projection divides by it twice.
Where the reference project itself loses digits, the fixture records it instead of hiding it:
  * SE3Quat::exp above its threshold evaluates (1 - cos theta) / theta^2 and (theta - sin theta) / theta^3 with cancellation
    (relative 1e-6 / 1e-5 at theta = 1e-5): the translation V upsilon is off by ~ eps |upsilon| / theta there, 7e-13 of the
    vertex's scale for |upsilon| = 10 in the oracle's fp64 evaluation.  That is g2o's arithmetic, not a kernel matter, and
    such an input cannot carry a bound below the ceiling: the updates just above the threshold have |upsilon| ~ 1e-3.
  * Below the threshold g2o passes I + W + W^2 through a unit quaternion; the project keeps cameras as (R, t) and does not
    re-normalise (difference O(theta^2) <= 5e-11, oracle/g2o_oracle_types.c header).  The reference here follows the
    project's stated representation."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as O                      # noqa: E402
from tests import landmark_helpers as LH            # noqa: E402
from tests import producer_metric as PM             # noqa: E402
from tests import reference_mp as M                 # noqa: E402

mp = M.mp
OUT = os.path.join(HERE, "producer_edges.npz")
PROFILE = os.path.join(ROOT, "profiles", "producer_edges.jsonl")
MIN_PER_COMBO = 12        # edges per (quaternion case, sign of qw) combination
TAILS = (1, 255, 256, 257, 513)

# Floors, in eps, for the outputs on which the oracle's fp64 evaluation is EXACT (figure 0), where 8 x 0 bounds nothing.  Every
# other output is bounded by 8 x the oracle's figure alone.
#   lm2_J1          entries +-cos(theta), +-sin(theta): one library call each, no arithmetic.  The device library's sin / cos
#                   are within 2 ulp, an ulp of a number below 1 is at most eps / 2: 2 ulp <= 1 eps; + the reference's own
#                   rounding to fp64 (eps / 2) -> 2 eps.
#   upd_pts, upd_lm2_pts, upd_lm3_pts
#                   one IEEE addition per entry, correctly rounded on both sides: the same number; 1 eps = one rounding.
FLOORS = dict(lm2_J1=2, upd_pts=1, upd_lm2_pts=1, upd_lm3_pts=1)


def f64(v):
    return np.array(M.f64(list(v)), np.float64)


def quat_R(q):
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q)
    return np.array([[float(v) for v in row] for row in M.quat_to_R(*[mp.mpf(float(x)) for x in (q[3], q[0], q[1], q[2])])])


def pack(R, t):
    return np.concatenate([np.asarray(R).T.reshape(9), np.asarray(t, np.float64)])


def rand_iso(rng, tmag):
    return pack(quat_R(rng.normal(size=4)), rng.normal(size=3) * tmag)


def axis_angle_R(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return quat_R(np.concatenate([np.sin(ang / 2) * a, [np.cos(ang / 2)]]))


def inv_np(T):
    R = T[:9].reshape(3, 3).T
    return pack(R.T, -R.T @ T[9:])


def mul_np(A, B):
    Ra, Rb = A[:9].reshape(3, 3).T, B[:9].reshape(3, 3).T
    return pack(Ra @ Rb, Ra @ B[9:] + A[9:])


def tmax(*Ts):
    return max(float(np.abs(T[9:]).max()) for T in Ts)


# ================================================================================================ SE3 pose-pose
def gen_se3(rng):
    Ti, Tj, Tz, tag = [], [], [], []

    def add(Rerr, name, tmag):
        xi, xj = rand_iso(rng, tmag), rand_iso(rng, tmag)
        E = pack(Rerr, rng.normal(size=3) * tmag * 0.1)
        z = mul_np(mul_np(inv_np(xi), xj), inv_np(E))           # Z^-1 Xi^-1 Xj = E up to rounding
        Ti.append(xi); Tj.append(xj); Tz.append(z); tag.append(name)

    mags = lambda: 10.0 ** rng.uniform(-3, 3)
    for _ in range(60):                                          # the whole of SO(3), angle uniform up to 179 degrees
        add(axis_angle_R(rng.normal(size=3), np.deg2rad(rng.uniform(0, 179))), "uniform", mags())
    for i in range(3):                                           # large angles about +- a dominant axis: cases 1..3, both signs
        for sgn in (1, -1):
            for _ in range(MIN_PER_COMBO + 2):
                a = rng.normal(size=3) * 0.3
                a[i] = sgn * (1.0 + abs(a[i]))
                add(axis_angle_R(a, np.deg2rad(rng.uniform(125, 179))), "case%d%s" % (i + 1, "+-"[sgn < 0]), mags())
    for _ in range(24):                                          # boundary: tr within 1e-3 of 0 (both sides)
        tr = rng.choice([-1, 1]) * 1e-3 * rng.uniform(0.02, 1)
        add(axis_angle_R(rng.normal(size=3), np.arccos((tr - 1) / 2)), "tr~0", mags())
    for _ in range(24):                                          # boundary: two diagonal entries within 1e-3 (tr < 0)
        i, j = rng.choice(3, 2, replace=False)
        a = np.abs(rng.normal(size=3)) * 0.2
        a[i] = 1.0
        a[j] = np.sqrt(1.0 + rng.choice([-1, 1]) * 1e-3 * rng.uniform(0.02, 1))
        a *= rng.choice([-1, 1], 3)
        add(axis_angle_R(a, np.deg2rad(rng.uniform(150, 179))), "diag~", mags())
    # the identity error: exactly (R = I everywhere) and up to rounding (Z = I, Xi = Xj)
    I = pack(np.eye(3), np.zeros(3))
    x = pack(np.eye(3), np.array([3.0, -2.0, 0.5]))
    Ti.append(x); Tj.append(x.copy()); Tz.append(I); tag.append("identity")
    x = rand_iso(rng, 5.0)
    Ti.append(x); Tj.append(x.copy()); Tz.append(I.copy()); tag.append("identity")
    n = len(Ti)
    poses = np.zeros((2 * n, 12))
    poses[0::2], poses[1::2] = np.array(Ti), np.array(Tj)
    vi, vj = np.arange(0, 2 * n, 2, dtype=np.int32), np.arange(1, 2 * n, 2, dtype=np.int32)
    Z = np.array(Tz)
    hidx = np.arange(2 * n, dtype=np.int32) - 1                  # vertex 0 fixed
    J0, J1, err, ops, case, sign = [], [], [], [], [], []
    for k in range(n):
        a, b, e = M.se3_edge(poses[vi[k]], poses[vj[k]], Z[k])
        w = M.se3_error_quat_w(M.iso(poses[vi[k]]), M.iso(poses[vj[k]]), M.iso(Z[k]))
        assert w >= 0.008, (k, tag[k], float(w))                 # margin from 180 degrees
        c, s, tr, gap = PM.se3_branch(poses[vi[k]], poses[vj[k]], Z[k])
        if tag[k] == "tr~0":
            assert abs(tr) < 2e-3
        if tag[k] == "diag~":
            assert c > 0 and gap < 2e-3, (k, c, gap)
        J0.append(M.f64(a)); J1.append(M.f64(b)); err.append(M.f64(e)); case.append(c); sign.append(s)
        ops.append(tmax(poses[vi[k]], poses[vj[k]], Z[k]))
    case, sign = np.array(case, np.int32), np.array(sign, np.int32)
    cov = {}
    for c in range(4):
        for s in (1, -1):
            cnt = int(((case == c) & (sign == s)).sum())
            if c == 0 and s == -1:
                assert cnt == 0                                  # tr > 0: qw = sqrt(tr + 1) / 2 > 0 always
                continue
            assert cnt >= MIN_PER_COMBO, (c, s, cnt)
            cov["case%d/qw%s" % (c, "+" if s > 0 else "-")] = cnt
    bnd = np.array([t in ("tr~0", "diag~", "identity") for t in tag])
    out = dict(se3_poses=poses, se3_hidx=hidx, se3_vi=vi, se3_vj=vj, se3_Z=Z, se3_J0=np.array(J0), se3_J1=np.array(J1),
               se3_err=np.array(err), se3_ops=np.array(ops), se3_case=case, se3_sign=sign, se3_boundary=bnd)
    oJ0, oJ1, oe = O.se3_edges(poses, vi, vj, Z)
    return out, dict(se3_J0=oJ0, se3_J1=oJ1, se3_err=oe), cov


# ================================================================================================ SE2 pose-pose
def gen_se2(rng):
    pi = np.pi
    rows = []                      # (xi, xj, z)
    for _ in range(60):            # angles anywhere in [-pi, pi): the sums land on both sides of +-pi
        rows.append((rng.uniform(-pi, pi), rng.uniform(-pi, pi), rng.uniform(-pi, pi)))
    for _ in range(30):            # thousands of radians out, either sign
        rows.append(tuple(rng.choice([-1, 1]) * rng.uniform(1e3, 2e4) if rng.rand() < 0.6 else rng.uniform(-pi, pi) for _ in range(3)))
    # exactly on the switch points: -z = M_PI and = -M_PI; (-xi) + xj = M_PI and = -M_PI.  (Never an ESTIMATE exactly on
    # +-M_PI: VertexSE2::oplus wraps by 2 M_PI, not 2 pi, so theta + h and theta - h would differ by 2.4e-16 there and the
    # central difference means nothing; estimates on +-M_PI are in the update group instead.)
    rows += [(0.3, 0.9, -pi), (0.5, 0.7, pi), (-pi / 2, pi / 2, 0.4), (pi / 2, -pi / 2, -0.7), (-pi / 2, pi / 2, -pi), (pi / 2, -pi / 2, pi)]
    n0 = len(rows)
    xi = np.array([[*(rng.normal(size=2) * 10.0 ** rng.uniform(-1, 2)), r[0]] for r in rows])
    xj = np.array([[*(rng.normal(size=2) * 10.0 ** rng.uniform(-1, 2)), r[1]] for r in rows])
    z = np.array([[*(rng.normal(size=2) * 5.0), r[2]] for r in rows])
    keep, branches = [], {}
    for k in range(n0):
        e = M.se2_error(M.V(xi[k]), M.V(xj[k]), M.V(z[k]))
        if abs(abs(e[2]) - M.PI64) < 1e-3:                       # final angle too close to the jump: move the measurement
            z[k, 2] += 0.01
            e = M.se2_error(M.V(xi[k]), M.V(xj[k]), M.V(z[k]))
        assert abs(abs(e[2]) - M.PI64) >= 1e-3
        keep.append(k)
        # the four normalisations of the chain in fp64, as the kernel performs them
        a = PM.wrap_branch(-z[k, 2]); b = PM.wrap_branch(-xi[k, 2])
        ni = float(M.normalize_theta(mp.mpf(-xi[k, 2]))); nz = float(M.normalize_theta(mp.mpf(-z[k, 2])))
        c = PM.wrap_branch(ni + xj[k, 2])
        nt = float(M.normalize_theta(mp.mpf(ni + xj[k, 2])))
        d = PM.wrap_branch(nz + nt)
        for name, th in (("inv", a), ("inv", b), ("mul", c), ("mul", d)):
            branches[name + ":" + th] = branches.get(name + ":" + th, 0) + 1
        for th in (-z[k, 2], -xi[k, 2], ni + xj[k, 2], nz + nt):
            if th in (pi, -pi):
                branches["exactly+-pi"] = branches.get("exactly+-pi", 0) + 1
    assert branches.get("exactly+-pi", 0) >= 6 and branches.get("mul:floor", 0) + branches.get("mul:floor+hi", 0) >= 10
    assert branches.get("inv:floor", 0) + branches.get("inv:floor+hi", 0) >= 10
    n = n0
    poses = np.zeros((2 * n, 3))
    poses[0::2], poses[1::2] = xi, xj
    vi, vj = np.arange(0, 2 * n, 2, dtype=np.int32), np.arange(1, 2 * n, 2, dtype=np.int32)
    hidx = np.arange(2 * n, dtype=np.int32) - 1
    J0, J1, err, ops = [], [], [], []
    for k in range(n):
        a, b, e = M.se2_edge(xi[k], xj[k], z[k])
        J0.append(M.f64(a)); J1.append(M.f64(b)); err.append(M.f64(e))
        ops.append(max(np.abs(xi[k]).max(), np.abs(xj[k]).max(), np.abs(z[k]).max()))
    out = dict(se2_poses=poses, se2_hidx=hidx, se2_vi=vi, se2_vj=vj, se2_Z=z, se2_J0=np.array(J0), se2_J1=np.array(J1),
               se2_err=np.array(err), se2_ops=np.array(ops), se2_boundary=np.arange(n) >= n - 6)
    # (se2_ops includes the raw angles, which normalize_theta subtracts multiples of 2 M_PI from: on the edges with angles
    # of 1e4 rad the blocks are held to 1e-4 * bound of their own entries, on the others to the bound itself)
    oJ0, oJ1, oe = O.se2_edges(poses, vi, vj, z)
    return out, dict(se2_J0=oJ0, se2_J1=oJ1, se2_err=oe), branches


# ================================================================================================ landmark edges
def gen_landmarks(rng):
    out, orc, cov = {}, {}, {}
    nP, nL, nE = 40, 60, TAILS[-1]
    first = 1 * nL + 5                                           # edge 0 (the n = 1 run): a free pose and a free landmark
    rest = rng.permutation(nP * nL)
    pairs = np.concatenate([[first], rest[rest != first][:nE - 1]])
    vp, vl = (pairs // nL).astype(np.int32), (pairs % nL).astype(np.int32)
    assert len(set(zip(vp.tolist(), vl.tolist()))) == nE
    hidx = np.arange(nP, dtype=np.int32) - 1                     # pose 0 fixed
    pt_hidx = (nP - 1) + np.arange(nL, dtype=np.int32) - 3       # landmarks 0..2 fixed
    pt_hidx[:3] = -1
    ev = np.arange(nP - 1, dtype=np.int32)                       # odometry chain (bound first; pinned by the pose-pose groups)
    # ---- 2-D
    poses = np.column_stack([rng.normal(size=(nP, 2)) * 20, rng.uniform(-np.pi, np.pi, nP)])
    # (pose angles inside [-pi, pi), where VertexSE2::oplus keeps them: the Jacobian through oplus of an angle far outside
    # is the Jacobian at the angle reduced with the fp64 M_PI, 1e-13 away; far-out angles are in the pose-pose group)
    pts = rng.normal(size=(nL, 2)) * 30                          # in front of, beside and behind every pose
    zl = np.array([M.f64(M.se2_point_error(M.V(poses[vp[k]]), M.V(pts[vl[k]]), [0, 0])) for k in range(nE)]) + rng.normal(size=(nE, 2)) * 0.3
    J0, J1, err, ops = [], [], [], []
    for k in range(nE):
        a, b, e = M.se2_point_edge(poses[vp[k]], pts[vl[k]], zl[k])
        J0.append(M.f64(a)); J1.append(M.f64(b)); err.append(M.f64(e))
        ops.append(max(np.abs(poses[vp[k], :2]).max(), np.abs(pts[vl[k]]).max(), np.abs(zl[k]).max()))
    Zo = np.zeros((nP - 1, 3))
    out.update(lm2_poses=poses, lm2_points=pts, lm2_hidx=hidx, lm2_pt_hidx=pt_hidx, lm2_vp=vp, lm2_vl=vl, lm2_zl=zl, lm2_vi=ev,
               lm2_vj=ev + 1, lm2_Z=Zo, lm2_J0=np.array(J0), lm2_J1=np.array(J1), lm2_err=np.array(err), lm2_ops=np.array(ops))
    a, b, e = LH.se2_pointxy_edges(poses, pts, vp, vl, zl)
    orc.update(lm2_J0=a, lm2_J1=b, lm2_err=e)
    # ---- 3-D, sensor offset with a non-trivial rotation
    poses3 = np.array([rand_iso(rng, 20.0) for _ in range(nP)])  # rotations anywhere in SO(3)
    pts3 = rng.normal(size=(nL, 3)) * 30
    off = pack(axis_angle_R([0.3, -1.0, 0.5], 2.1), [0.4, -0.2, 1.1])
    Om = M.iso(off)
    zl3 = np.array([M.f64(M.se3_point_error(M.iso(poses3[vp[k]]), M.V(pts3[vl[k]]), [0, 0, 0], Om)) for k in range(nE)])
    side = dict(front=int((zl3[:, 2] > 0).sum()), behind=int((zl3[:, 2] < 0).sum()),
                beside=int((np.abs(zl3[:, 2]) < np.abs(zl3[:, :2]).max(axis=1)).sum()))
    assert min(side.values()) >= 50
    zl3 = zl3 + rng.normal(size=(nE, 3)) * 0.3
    J0, J1, err, ops = [], [], [], []
    for k in range(nE):
        a, b, e = M.se3_point_edge(poses3[vp[k]], pts3[vl[k]], zl3[k], off)
        J0.append(M.f64(a)); J1.append(M.f64(b)); err.append(M.f64(e))
        ops.append(max(np.abs(poses3[vp[k], 9:]).max(), np.abs(pts3[vl[k]]).max(), np.abs(zl3[k]).max(), np.abs(off[9:]).max()))
    Z3 = np.array([mul_np(inv_np(poses3[k]), poses3[k + 1]) for k in range(nP - 1)])
    out.update(lm3_poses=poses3, lm3_points=pts3, lm3_hidx=hidx, lm3_pt_hidx=pt_hidx, lm3_vp=vp, lm3_vl=vl, lm3_zl=zl3, lm3_vi=ev,
               lm3_vj=ev + 1, lm3_Z=Z3, lm3_offset=off, lm3_J0=np.array(J0), lm3_J1=np.array(J1), lm3_err=np.array(err),
               lm3_ops=np.array(ops))
    a, b, e = LH.se3_pointxyz_edges(poses3, pts3, vp, vl, zl3, off)
    orc.update(lm3_J0=a, lm3_J1=b, lm3_err=e)
    # ---- the landmark-graph vertex update (pg_points_update_kernel beside the pose update): x over 39 free poses and 57
    # free landmarks, three landmarks and one pose fixed
    for pre, dp, dl, P0 in (("lm2", 3, 2, pts), ("lm3", 6, 3, pts3)):
        nf = nP - 1
        x = np.concatenate([rng.normal(size=dp * nf) * 0.05, (rng.normal(size=(nL - 3, dl)) * 10.0 ** rng.uniform(-6, 2, (nL - 3, 1))).reshape(-1)])
        ref, uo = P0.copy(), np.abs(P0).max(axis=1)
        for v in range(nL):
            if pt_hidx[v] >= 0:
                u = x[dp * nf + dl * (pt_hidx[v] - nf):dp * nf + dl * (pt_hidx[v] - nf + 1)]
                ref[v] = M.f64(M.point_oplus(M.V(P0[v]), M.V(u)))
                uo[v] = max(uo[v], np.abs(u).max())
        out.update({"upd_%s_x" % pre: x, "upd_%s_pts" % pre: ref, "upd_%s_pts_ops" % pre: uo})
        orc["upd_%s_pts" % pre] = LH.points_oplus(P0, pt_hidx, x, dp * nf, nf)
    cov.update(dict(("tail%d" % t, t) for t in TAILS), **side)
    cov["fixed_pose_edges"] = int((hidx[vp] < 0).sum())
    cov["fixed_landmark_edges"] = int((pt_hidx[vl] < 0).sum())
    assert cov["fixed_pose_edges"] > 0 and cov["fixed_landmark_edges"] > 0
    return out, orc, cov


# ================================================================================================ BA projection
BA_CLASSES = np.array([[1000.0, 320.0, 240.0, 0, 0.0],           # (f, cx, cy, kernel kind, delta)
                       [640.0, 300.5, 255.25, 1, 1.5],
                       [1500.0, 512.0, 384.0, 3, 2.0],
                       [640.0, 300.5, 255.25, 2, 1.0]])
BA1_HUBER = 2.5                                                  # the one-class variant: class 0's intrinsics, Huber


def gen_ba(rng):
    cams, pts, cam_idx, pt_idx, depth_of = [], [], [], [], []
    # cluster A: cameras near the origin, |X| ~ 1 .. 50, depths from 0.02; cluster B: the scene 1e4 away, depths 600 .. 3000
    for centre, ncam, npt, dlo, dhi in ((np.zeros(3), 8, 28, 0.02, 50.0), (np.array([8e3, -1e4, 6e3]), 4, 12, 600.0, 3000.0)):
        c0, p0 = len(cams), len(pts)
        for c in range(ncam):
            R = axis_angle_R(rng.normal(size=3), rng.uniform(0, 0.002 if dlo < 1 else 0.05)) @ axis_angle_R([0.2, 1.0, -0.4], 1.3)
            pos = centre + rng.normal(size=3) * (0.0005 if dlo < 1 else 3.0)       # camera centre in the world
            cams.append(pack(R, -R @ pos))
        Rm = cams[c0][:9].reshape(3, 3).T
        for p in range(npt):
            d = dlo * (dhi / dlo) ** (p / (npt - 1.0))           # depth, log-spaced
            u = rng.uniform(-1, 1, 2) * ((12.0 if dlo < 1 else 2.0) if p % 3 == 0 else 0.3)            # x/z, y/z: well outside the image or inside it
            pc = np.array([u[0] * d, u[1] * d, d])
            X = Rm.T @ (pc - cams[c0][9:])
            pts.append(X)
            for c in range(ncam):
                cam_idx.append(c0 + c); pt_idx.append(p0 + p)
    cams, pts = np.array(cams), np.array(pts)
    cam_idx, pt_idx = np.array(cam_idx, np.int32), np.array(pt_idx, np.int32)
    E, P, L = len(cam_idx), len(cams), len(pts)
    cam_hidx = np.full(P, -1, np.int32)
    free = [c for c in range(P) if c not in (0, 8)]              # one fixed camera per cluster
    cam_hidx[free] = np.arange(len(free), dtype=np.int32)
    nP = len(free)
    cls = rng.randint(0, len(BA_CLASSES), E).astype(np.int32)
    unit = rng.normal(size=(E, 2))
    base = np.where(rng.rand(E) < 0.3, 30.0, 0.7)                # pixels; 30 % outliers: both sides of every delta
    out, orc, cov = {}, {}, {}
    out.update(ba_cams=cams, ba_pts=pts, ba_cam_idx=cam_idx, ba_pt_idx=pt_idx, ba_cam_hidx=cam_hidx, ba_edge_class=cls,
               ba_classes=BA_CLASSES, ba1_huber=np.float64(BA1_HUBER))
    for pre, klass in (("ba", cls), ("ba1", np.zeros(E, np.int32))):
        par = BA_CLASSES[klass].copy()
        if pre == "ba1":
            par[:, 3], par[:, 4] = 1, BA1_HUBER
        meas = np.zeros((E, 2))
        J0, J1, err, ops, wts, rhos, Jm = [], [], [], [], [], [], []
        zmin, ratio, uvmax, sides = 1e300, 0.0, 0.0, {}
        for k in range(E):
            T, X = cams[cam_idx[k]], pts[pt_idx[k]]
            f, cx, cy, kind, delta = par[k]
            pc = M.camera_point(M.iso(T), M.V(X))
            zmin, ratio = min(zmin, float(pc[2])), max(ratio, float(np.abs(X).max() / pc[2]))
            uvmax = max(uvmax, abs(float(pc[0] / pc[2])), abs(float(pc[1] / pc[2])))
            assert pc[2] > 0 and np.abs(X).max() / pc[2] <= 25
            proj = M.f64(M.project_error(M.iso(T), M.V(X), [0, 0], f, cx, cy))
            # the error is the difference of two numbers of |f u + c| pixels and inherits their absolute rounding (times
            # |X| / depth from the cancellation in z): where the projection lies far outside the image an error of a pixel
            # would be known to 1e-11 of itself, and with it the robust weight and b.  Those edges carry an error of a
            # fifth of their distance from the principal point, at least f / 5 (they are outliers of any delta); so do all
            # edges of the far cluster, whose projections are known to 1e-14 of themselves at best
            fu = max(abs(-proj[0] - cx), abs(-proj[1] - cy))
            if cam_idx[k] >= 8:                                  # (the far cluster: |X| / depth ~ 16 on every edge)
                fu = max(fu, 1.001 * f)
            meas[k] = -np.array(proj) + unit[k] * max(base[k], 0.2 * fu if fu > f else 0.0)
            a, b, e = M.project_edge(T, X, meas[k], f, cx, cy)
            e2 = e[0] * e[0] + e[1] * e[1]
            if kind in (1, 4):
                assert abs(e2 / mp.mpf(delta) ** 2 - 1) > 1e-6
            if kind > 0:
                s = "k%d:%s" % (kind, "e2<=d2" if e2 <= mp.mpf(delta) ** 2 else "e2>d2")
                sides[s] = sides.get(s, 0) + 1
            rho, w = M.robust(int(kind), delta, e2)
            J0.append(M.f64(a)); J1.append(M.f64(b)); err.append(M.f64(e)); wts.append(w); rhos.append(rho); Jm.append((a, b, e))
            ops.append(max(np.abs(X).max(), np.abs(T[9:]).max(), np.abs(meas[k]).max(), cx, cy))
        assert all(v >= 5 for v in sides.values()) and len(sides) == 2 * len(set(par[:, 3]) - {0}), sides
        # products in extended precision: Hpl per edge, Hpp per free camera, Hll per point, b.  Scale of an entry: the sum
        # of the magnitudes of the terms w J J' added into it (Hpl: the larger of its two terms); of a block: its largest
        # entry's.  b = -sum w J' (z - proj): its terms are formed from z and proj, so a term counts with max(|e|, |z|)
        Hpl, Hpl_ops = np.zeros((E, 18)), np.zeros(E)
        Hpp, Hpp_ops = [[mp.mpf(0)] * 36 for _ in range(nP)], np.zeros((nP, 36))
        Hll, Hll_ops = [[mp.mpf(0)] * 9 for _ in range(L)], np.zeros((L, 9))
        bb, b_ops = [mp.mpf(0)] * (6 * nP + 3 * L), np.zeros(6 * nP + 3 * L)
        for k in range(E):
            A, B, e = Jm[k]
            w, h, l = wts[k], cam_hidx[cam_idx[k]], pt_idx[k]
            Ac = lambda r, c: A[r + 2 * c]
            Bc = lambda r, c: B[r + 2 * c]
            ez = [max(abs(float(e[i])), abs(meas[k, i])) for i in range(2)]
            for c in range(3):
                for r in range(3):
                    v = w * (Ac(0, r) * Ac(0, c) + Ac(1, r) * Ac(1, c))
                    Hll[l][r + 3 * c] += v; Hll_ops[l, r + 3 * c] += abs(float(w * Ac(0, r) * Ac(0, c))) + abs(float(w * Ac(1, r) * Ac(1, c)))
                v = w * (Ac(0, c) * e[0] + Ac(1, c) * e[1])
                bb[6 * nP + 3 * l + c] -= v; b_ops[6 * nP + 3 * l + c] += float(w) * (abs(float(Ac(0, c))) * ez[0] + abs(float(Ac(1, c))) * ez[1])
            if h < 0:
                continue
            for c in range(6):
                for r in range(6):
                    v = w * (Bc(0, r) * Bc(0, c) + Bc(1, r) * Bc(1, c))
                    Hpp[h][r + 6 * c] += v; Hpp_ops[h, r + 6 * c] += abs(float(w * Bc(0, r) * Bc(0, c))) + abs(float(w * Bc(1, r) * Bc(1, c)))
                v = w * (Bc(0, c) * e[0] + Bc(1, c) * e[1])
                bb[6 * h + c] -= v; b_ops[6 * h + c] += float(w) * (abs(float(Bc(0, c))) * ez[0] + abs(float(Bc(1, c))) * ez[1])
            for c in range(3):                                   # Hpl block 6 x 3 column-major: B' (w I) A
                for r in range(6):
                    t0, t1 = w * Bc(0, r) * Ac(0, c), w * Bc(1, r) * Ac(1, c)
                    Hpl[k, r + 6 * c] = float(t0 + t1)
                    Hpl_ops[k] = max(Hpl_ops[k], abs(float(t0)), abs(float(t1)))
        chi2 = sum(rhos)
        out.update({pre + "_meas": meas, pre + "_J0": np.array(J0), pre + "_J1": np.array(J1), pre + "_err": np.array(err),
                    pre + "_ops": np.array(ops), pre + "_w": f64(wts), pre + "_Hpl": Hpl, pre + "_Hpl_ops": Hpl_ops,
                    pre + "_Hpp": np.array([M.f64(h) for h in Hpp]), pre + "_Hpp_ops": Hpp_ops.max(axis=1),
                    pre + "_Hll": np.array([M.f64(h) for h in Hll]), pre + "_Hll_ops": Hll_ops.max(axis=1),
                    pre + "_b": f64(bb), pre + "_b_ops": b_ops, pre + "_chi2": np.float64(float(chi2)),
                    pre + "_chi2_ops": np.float64(float(sum(abs(r) for r in rhos)))})
        # the oracle's fp64 evaluation: its C producers per class, its robust kernels, the same products in fp64
        oJ0, oJ1, oe = np.zeros((E, 6)), np.zeros((E, 12)), np.zeros((E, 2))
        for c in range(len(BA_CLASSES)):
            sel = np.nonzero(klass == c)[0]
            if len(sel):
                f, cx, cy = par[sel[0], :3]
                oJ0[sel], oJ1[sel], oe[sel] = O.ba_edges(cams, pts, cam_idx[sel], pt_idx[sel], meas[sel], f, cx, cy)
        orc.update({pre + "_J0": oJ0, pre + "_J1": oJ1, pre + "_err": oe})
        orc.update(PM.ba_products_fp64(O.robustify, pre, oJ0, oJ1, oe, par, cam_hidx[cam_idx], pt_idx, nP, L))
        cov[pre] = dict(edges=E, min_depth=zmin, max_X_over_depth=ratio, max_uv=uvmax, world_max=float(np.abs(pts).max()), **sides)
    return out, orc, cov


# ================================================================================================ vertex updates
def gen_updates(rng):
    out, orc, cov = {}, {}, {}
    # ---- VertexSE3: |u_q| = 0, 1e-9, 0.5, 0.999, 1 (exactly: axis-aligned), 1.5
    us, names = [], []
    for length in (0.0, 1e-9, 0.5, 0.999, 1.5):
        for _ in range(4):
            a = rng.normal(size=3)
            us.append(np.concatenate([rng.normal(size=3) * 10.0 ** rng.uniform(-2, 2), a / np.linalg.norm(a) * length]))
            names.append(length)
    for ax in range(3):
        for sg in (1.0, -1.0):
            v = np.zeros(3); v[ax] = sg
            us.append(np.concatenate([rng.normal(size=3), v])); names.append(1.0)
    us.append(np.zeros(6)); names.append(0.0)                    # the zero update
    us = np.array(us)
    nv = len(us) + 2
    poses = np.array([rand_iso(rng, 10.0 ** rng.uniform(-1, 2)) for _ in range(nv)])
    hidx = np.full(nv, -1, np.int32)                             # vertices 0 and 7 fixed
    freev = [v for v in range(nv) if v not in (0, 7)]
    hidx[freev] = rng.permutation(len(freev)).astype(np.int32)
    ref, ops, side = poses.copy(), np.zeros(nv), dict(w_neg=0, w_zero=0, w_pos=0)
    for v in freev:
        u = us[hidx[v]]
        n2 = sum(mp.mpf(float(x)) ** 2 for x in u[3:])
        assert n2 == 1 or abs(n2 - 1) >= 1e-3
        n2f = u[3] * u[3] + u[4] * u[4] + u[5] * u[5]
        side["w_neg" if 1 - n2f < 0 else ("w_zero" if 1 - n2f == 0 else "w_pos")] += 1
        ref[v] = M.f64(M.iso_pack(M.se3_oplus(M.iso(poses[v]), M.V(u))))
        ops[v] = max(np.abs(poses[v, 9:]).max(), np.abs(u[:3]).max())
    assert side["w_neg"] >= 4 and side["w_zero"] >= 6
    out.update(upd_se3_poses=poses, upd_se3_hidx=hidx, upd_se3_x=us.reshape(-1), upd_se3=ref, upd_se3_ops=ops)
    orc["upd_se3"] = O.se3_oplus(poses, hidx, us.reshape(-1))
    cov["se3_update"] = side
    # ---- VertexSE2: sums across the wrap, exactly on it, thousands of radians out
    pi = np.pi
    th = [(3.0, 0.5), (-3.0, -0.5), (3.0, 0.1), (-3.1, 0.05), (pi / 2, pi / 2), (-pi / 2, -pi / 2), (pi, 0.0), (-pi, 0.0),
          (0.25, 5000.0), (-0.5, -12345.0), (2.0, 2 * pi * 700 + 1.5), (1.0, -2 * pi * 300 - 3.0), (0.1, 0.0), (3.1, 6.3)]
    nv2 = len(th) + 1
    p2 = np.column_stack([rng.normal(size=(nv2, 2)) * 50, np.array([0.7] + [a for a, _ in th])])
    h2 = np.arange(nv2, dtype=np.int32) - 1                      # vertex 0 fixed
    x2 = np.column_stack([rng.normal(size=(len(th), 2)), np.array([b for _, b in th])]).reshape(-1)
    r2, o2, wr = p2.copy(), np.zeros(nv2), {}
    for v in range(1, nv2):
        u = x2[3 * (v - 1):3 * v]
        s = mp.mpf(float(p2[v, 2])) + mp.mpf(float(u[2]))
        sf = p2[v, 2] + u[2]
        if sf not in (pi, -pi):                                  # margins from the switch points (sum exact or far from them)
            assert abs(abs(s) - M.PI64) > 1e-6
            frac = s / (2 * M.PI64) - mp.floor(s / (2 * M.PI64))
            assert abs(s) < M.PI64 or (1e-6 < frac < 1 - 1e-6 and abs(frac - 0.5) > 1e-6)
        else:
            assert s == mp.mpf(sf)
        wr[PM.wrap_branch(sf)] = wr.get(PM.wrap_branch(sf), 0) + 1
        r2[v] = M.f64(M.se2_oplus(M.V(p2[v]), M.V(u)))
        o2[v] = max(np.abs(p2[v]).max(), np.abs(u).max())
    assert wr.get("floor", 0) >= 2 and wr.get("floor+hi", 0) >= 2 and wr.get("in", 0) >= 2
    out.update(upd_se2_poses=p2, upd_se2_hidx=h2, upd_se2_x=x2, upd_se2=r2, upd_se2_ops=o2)
    orc["upd_se2"] = O.se2_oplus(p2, h2, x2)
    cov["se2_update"] = wr
    # ---- VertexSE3Expmap (theta = 0, 1e-12, just below / above 0.00001, 1, close to pi, 10) and the points
    thetas = [0.0, 1e-12, 0.00001 * (1 - 4e-6), 0.00001 * (1 + 4e-6), 1.0, np.pi - 1e-3, 10.0]
    uc = []
    for t in thetas:
        for _ in range(3):
            a = rng.normal(size=3)
            # (just above the threshold SE3Quat::exp loses digits: see the module docstring; upsilon small there)
            ups = 1e-3 if 0.00001 <= t < 0.001 else 10.0 ** rng.uniform(-2, 1)
            uc.append(np.concatenate([a / np.linalg.norm(a) * t, rng.normal(size=3) * ups]))
    uc.append(np.zeros(6))
    uc = np.array(uc)
    nc = len(uc) + 1
    cams = np.array([rand_iso(rng, 10.0 ** rng.uniform(-1, 2)) for _ in range(nc)])
    hc = np.arange(nc, dtype=np.int32) - 1                       # camera 0 fixed
    rc, oc, sd = cams.copy(), np.zeros(nc), dict(small=0, large=0)
    for v in range(1, nc):
        u = uc[v - 1]
        t = mp.sqrt(sum(mp.mpf(float(x)) ** 2 for x in u[:3]))
        tf = np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
        assert abs(t / M.EXP_SWITCH - 1) >= 1e-6 and (t < M.EXP_SWITCH) == (tf < 0.00001)
        sd["small" if tf < 0.00001 else "large"] += 1
        rc[v] = M.f64(M.iso_pack(M.expmap_oplus(M.iso(cams[v]), M.V(u))))
        oc[v] = max(np.abs(cams[v, 9:]).max(), np.abs(u[3:]).max())
    npt = 9
    pts = rng.normal(size=(npt, 3)) * 10.0 ** rng.uniform(0, 4, (npt, 1))
    hp = np.arange(npt, dtype=np.int32) - 1                      # point 0 fixed; every free point observed once (see the test)
    xl = rng.normal(size=(npt - 1, 3)) * 10.0 ** rng.uniform(-6, 2, (npt - 1, 1))
    rp, op = pts.copy(), np.abs(pts).max(axis=1)
    for v in range(1, npt):
        rp[v] = M.f64(M.point_oplus(M.V(pts[v]), M.V(xl[v - 1])))
    out.update(upd_cam_cams=cams, upd_cam_hidx=hc, upd_cam_x=uc.reshape(-1), upd_cam=rc, upd_cam_ops=oc, upd_pts_pts=pts,
               upd_pts_hidx=hp, upd_pts_x=xl.reshape(-1), upd_pts=rp, upd_pts_ops=op)
    oc_, op_ = O.ba_oplus(cams, pts, hc, hp, np.concatenate([uc.reshape(-1), xl.reshape(-1)]), 6 * (nc - 1))
    orc.update(upd_cam=oc_, upd_pts=op_)
    cov["camera_update"] = sd
    return out, orc, cov


# ================================================================================================ robust kernels
def gen_robust(rng):
    """Generic path (setEdgeData): pose dimension 3, error dimension 3, identity information, every edge between its own
    two vertices.  Errors (0,0,0), (delta/2,0,0), (delta,0,0) -- e2 == delta^2 on every side: delta*delta + 0 + 0 --
    and (3 delta, delta, 0), with delta the edge's own delta for the per-edge run."""
    kinds, deltas, errs = [], [], []
    for kind in (0, 1, 2, 3, 4, 5):
        for delta in (0.5, 1.5, 3.0):
            for lev in range(4):
                kinds.append(kind); deltas.append(delta)
                errs.append([(0, 0, 0), (delta / 2, 0, 0), (delta, 0, 0), (3 * delta, delta, 0)][lev])
    n = len(kinds)
    kinds, deltas, errs = np.array(kinds, np.int32), np.array(deltas), np.array(errs, np.float64)
    J0 = rng.randint(-3, 4, (n, 9)).astype(np.float64)           # small integers: J' J and J' e carry no rounding of their own
    J1 = rng.randint(-3, 4, (n, 9)).astype(np.float64)
    SET_DELTA = 1.5
    runs = [("edge", kinds, deltas)] + [("set%d" % k, np.full(n, k, np.int32), np.full(n, SET_DELTA)) for k in range(1, 6)]
    out = dict(rob_J0=J0, rob_J1=J1, rob_err=errs, rob_kinds=kinds, rob_deltas=deltas, rob_set_delta=np.float64(SET_DELTA))
    orc, cov = {}, {}
    for name, kk, dd in runs:
        H, b, chi, Ho, bo, chio = np.zeros((2 * n, 9)), np.zeros(6 * n), mp.mpf(0), np.zeros((2 * n, 9)), np.zeros(6 * n), 0.0
        for k in range(n):
            e = M.V(errs[k])
            e2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
            rho, w = M.robust(int(kk[k]), dd[k], e2)
            chi += rho
            e2f = float(errs[k] @ errs[k])
            r = O.robustify(int(kk[k]), dd[k], e2f) if kk[k] > 0 else (e2f, 1.0, 0.0)
            chio += r[0]
            side = "k%d:%s" % (kk[k], "==" if e2f == dd[k] * dd[k] else ("<" if e2f < dd[k] * dd[k] else ">"))
            if name == "edge" or dd[k] == SET_DELTA:
                cov[name + ":" + side] = cov.get(name + ":" + side, 0) + 1
            for v, J in ((2 * k, J0[k]), (2 * k + 1, J1[k])):
                Jm = J.reshape(3, 3).T
                JJ, Je = Jm.T @ Jm, Jm.T @ errs[k]
                H[v] = [float(w * mp.mpf(float(x))) for x in JJ.T.reshape(9)]
                b[3 * v:3 * v + 3] = [float(-w * mp.mpf(float(x))) for x in Je]
                Ho[v], bo[3 * v:3 * v + 3] = r[1] * JJ.T.reshape(9), -r[1] * Je
        out.update({"rob_%s_Hpp" % name: H, "rob_%s_b" % name: b, "rob_%s_chi2" % name: np.float64(float(chi))})
        orc.update({"rob_%s_Hpp" % name: Ho, "rob_%s_b" % name: bo, "rob_%s_chi2" % name: np.array([chio])})
    for k in range(1, 6):
        for s in ("<", "==", ">"):
            assert cov.get("edge:k%d:%s" % (k, s), 0) >= 3 and cov.get("set%d:k%d:%s" % (k, k, s), 0) >= 1, (k, s, cov)
    return out, orc, cov


def main():
    rng = np.random.RandomState(20240917)
    fx, figures, coverage = {}, {}, {}
    for name, gen in (("se3", gen_se3), ("se2", gen_se2), ("landmarks", gen_landmarks), ("ba", gen_ba), ("updates", gen_updates),
                      ("robust", gen_robust)):
        out, orc, cov = gen(rng)
        fx.update(out)
        coverage[name] = cov
        for key, got in orc.items():
            if key.startswith("rob_"):
                base = "rob_" + key.split("_")[-1]
                ref = out[key]
                ops = np.zeros(len(np.atleast_1d(ref))) if not key.endswith("chi2") else np.zeros(1)
                ref = np.atleast_1d(ref).reshape(len(ops), -1)
                fig = PM.worst(np.asarray(got).reshape(ref.shape), ref, ops)[0]
                figures[base] = max(figures.get(base, 0.0), fig)
                continue
            ref = out[key]
            if key.endswith("chi2"):
                ref, ops = np.array([[float(ref)]]), np.array([float(out[key + "_ops"])])
                got = np.asarray(got).reshape(1, 1)
            elif key.endswith("_b"):
                ref, ops, got = np.asarray(ref).reshape(-1, 1), out[key + "_ops"], np.asarray(got).reshape(-1, 1)
            elif key + "_ops" in out:
                ops = out[key + "_ops"]
            else:
                ops = out[key.rsplit("_", 1)[0] + "_ops"]
            figures[key] = PM.worst(got, ref, ops)[0]
        print(name, json.dumps(cov))
    lines = []
    for key in sorted(figures):
        fx["oracle_" + key] = np.float64(figures[key])
        assert (figures[key] == 0) == (key in FLOORS), (key, figures[key])
        fx["floor_" + key] = np.float64(FLOORS.get(key, 0))
        lines.append(dict(output=key, who="oracle_fp64_vs_mp60", worst_per_edge=figures[key], floor_eps=FLOORS.get(key, 0),
                          bound=PM.MARGIN * figures[key] if figures[key] > 0 else FLOORS[key] * PM.EPS))
        print("%-10s oracle %.3e  bound %.3e" % (key, figures[key], lines[-1]["bound"]))
    for key in sorted(figures):      # an oracle that cannot stay a factor MARGIN below the ceiling: move the input or fix the oracle
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
