"""Deterministic synthetic bundle-adjustment generator + host-side input producers.

The scene is the deterministic-window variant of g2o's `ba_demo`
(g2o/examples/ba/ba_demo.cpp:151-256) defined in SURVEY.md section 8d: focal length 1000,
principal point (320,240), information I_2; pose k sits at (k*s, 0, 0) with identity
rotation; landmark j is centred at pose c_j = floor(j*P/L), drawn uniformly in the box
x in t_c +- 1.5, y in +-0.5, z in [3,4] and observed by the 5 poses c_j-2..c_j+2 (window
shifted at the ends); pixel noise N(0,1); initial point perturbation N(0,0.05^2), pose
perturbation N(0,0.01^2) translation / N(0,0.005^2) rotation; poses 0 and 1 fixed
(ba_demo.cpp:182-184).  Randomness is a counter-based splitmix64 stream (seed 42) so the
same numbers come out of any vectorised or scalar implementation.

The error / Jacobian / oplus formulas are the host-side restatement of
EdgeProjectXYZ2UV (g2o/types/sba/types_six_dof_expmap.cpp:288-326, .h:139-147),
VertexSE3Expmap::oplusImpl (.h:101-104, SE3Quat::exp g2o/types/slam3d/se3quat.h:223-257)
and VertexSBAPointXYZ::oplusImpl (g2o/types/sba/types_sba.h:151-155): they are *input
producers* for the solver, not part of the accelerated path.
"""
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = x
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


class CounterRng:
    """u(stream, i): uniform in [0,1) from splitmix64(seed, stream, i)."""

    def __init__(self, seed=42):
        self.seed = np.uint64(seed)

    def uniform(self, stream, n):
        with np.errstate(over="ignore"):
            idx = np.arange(n, dtype=np.uint64)
            key = _splitmix64(self.seed * np.uint64(0x100000001B3) + np.uint64(stream))
            z = _splitmix64(key ^ (idx * np.uint64(0xD6E8FEB86659FD93) & _M64))
        return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)

    def normal(self, stream, n):
        u1 = self.uniform(2 * stream, n)
        u2 = self.uniform(2 * stream + 1, n)
        return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


def _exp_so3(w):
    """Rodrigues as in SE3Quat::exp; w: [n,3] -> R [n,3,3], V [n,3,3]."""
    n = len(w)
    theta = np.linalg.norm(w, axis=1)
    Om = np.zeros((n, 3, 3))
    Om[:, 0, 1], Om[:, 0, 2] = -w[:, 2], w[:, 1]
    Om[:, 1, 0], Om[:, 1, 2] = w[:, 2], -w[:, 0]
    Om[:, 2, 0], Om[:, 2, 1] = -w[:, 1], w[:, 0]
    Om2 = Om @ Om
    I = np.eye(3)[None]
    small = theta < 0.00001
    th = np.where(small, 1.0, theta)
    a = (np.sin(th) / th)[:, None, None]
    b = ((1 - np.cos(th)) / (th * th))[:, None, None]
    c = ((th - np.sin(th)) / (th ** 3))[:, None, None]
    R = I + a * Om + b * Om2
    V = I + b * Om + c * Om2
    Rs = I + Om + Om2
    R = np.where(small[:, None, None], Rs, R)
    V = np.where(small[:, None, None], Rs, V)
    return R, V


def make_ba_problem(P, L, seed=42, spacing=0.5, obs_per_landmark=5, outlier_frac=0.0,
                    f=1000.0, cx=320.0, cy=240.0, stereo_baseline=None):
    """stereo_baseline = b: the observations are those of EdgeProjectXYZ2UVU (types_six_dof_expmap.h:181-200) -- the dictionary
    gains observation = "stereo", baseline = b and meas [E][3] with u_right = f (x - b) / z + cx in its third column (noise:
    normal stream 15 = uniform streams 30 / 31, outliers uniform over the image width from uniform stream 32; none of them used
    otherwise).  Everything else, and
    the whole dictionary without the argument, is as before."""
    rng = CounterRng(seed)
    K = obs_per_landmark
    assert P >= K
    j = np.arange(L, dtype=np.int64)
    c = (j * P) // L
    lo = np.clip(c - K // 2, 0, P - K)
    cam_idx = (lo[:, None] + np.arange(K)[None, :]).reshape(-1).astype(np.int32)       # landmark-major edges
    pt_idx = np.repeat(np.arange(L, dtype=np.int32), K)
    E = L * K
    true_pts = np.stack([c * spacing + (rng.uniform(1, L) * 3.0 - 1.5),
                         rng.uniform(2, L) - 0.5,
                         3.0 + rng.uniform(3, L)], axis=1)
    # true cameras: world->camera, R = I, t = -position
    cams_true = np.zeros((P, 12))
    cams_true[:, 0] = cams_true[:, 4] = cams_true[:, 8] = 1.0
    cams_true[:, 9] = -np.arange(P) * spacing
    # observations
    Xc = true_pts[pt_idx] + cams_true[cam_idx, 9:12]
    meas = np.stack([Xc[:, 0] / Xc[:, 2] * f + cx, Xc[:, 1] / Xc[:, 2] * f + cy], axis=1)
    meas[:, 0] += rng.normal(4, E)
    meas[:, 1] += rng.normal(5, E)
    if outlier_frac > 0:                      # ba_demo.cpp:222-227: uniform in the image
        is_out = rng.uniform(20, E) < outlier_frac
        meas[is_out, 0] = rng.uniform(21, E)[is_out] * 640.0
        meas[is_out, 1] = rng.uniform(22, E)[is_out] * 480.0
    # initial estimates
    pts = true_pts + 0.05 * np.stack([rng.normal(6, L), rng.normal(7, L), rng.normal(8, L)], axis=1)
    upd = np.zeros((P, 6))
    upd[:, 0:3] = 0.005 * np.stack([rng.normal(9, P), rng.normal(10, P), rng.normal(11, P)], axis=1)
    upd[:, 3:6] = 0.01 * np.stack([rng.normal(12, P), rng.normal(13, P), rng.normal(14, P)], axis=1)
    upd[:2] = 0.0                             # fixed poses keep the true value
    cams = _apply_cam_update(cams_true, upd)
    cam_hidx = np.arange(P, dtype=np.int32) - 2
    cam_hidx[:2] = -1
    nP = P - 2
    prob = dict(P=P, L=L, E=E, nP=nP, nL=L, f=f, cx=cx, cy=cy, cams=cams, pts=pts, meas=meas,
                cam_idx=cam_idx, pt_idx=pt_idx, cam_hidx=cam_hidx,
                v0=(nP + pt_idx).astype(np.int32),        # EdgeProjectXYZ2UV: vertex 0 = point
                v1=cam_hidx[cam_idx].astype(np.int32))    # vertex 1 = pose (types_six_dof_expmap.h:133)
    if stereo_baseline is not None:
        ur = (Xc[:, 0] - stereo_baseline) / Xc[:, 2] * f + cx + rng.normal(15, E)
        if outlier_frac > 0:
            ur[is_out] = rng.uniform(32, E)[is_out] * 640.0
        prob.update(observation="stereo", baseline=float(stereo_baseline), meas=np.concatenate([meas, ur[:, None]], axis=1))
    return prob


def make_ba_odometry(P, L, loop_every=10, sigma_rot=0.002, sigma_trans=0.01, seed=42, **ba_args):
    """make_ba_problem(P, L, seed=seed, **ba_args) -- mono, or stereo with stereo_baseline -- with a set of EdgeSE3Expmap
    constraints between its cameras (types_six_dof_expmap.h:111-130) under the key pose_edges: odometry between consecutive
    cameras (k, k + 1) and loop closures (k, k + loop_every) for every loop_every-th camera k; pairs of two fixed cameras are
    left out.  The measurement of an edge (vertex 0 = Ti, vertex 1 = Tj) is Tj exp(noise) Ti^-1 of the TRUE cameras -- the
    true relative pose times a small exp(noise), placed so that the error at the truth, log(Tj^-1 C Ti), is the noise itself
    wherever the cameras stand (omega ~ N(0, sigma_rot^2), upsilon ~ N(0, sigma_trans^2): normal streams 60 .. 65) -- and
    the information diag(1 / sigma_rot^2 x 3, 1 / sigma_trans^2 x 3) of every edge.
    pose_edges = dict(n, vi, vj (indices into cams), v0, v1 (hessian indices, -1 = fixed), meas [n][12], info [n][36])."""
    from . import se3expmap as X
    prob = make_ba_problem(P, L, seed=seed, **ba_args)
    spacing = ba_args.get("spacing", 0.5)
    truth = np.zeros((P, 12))
    truth[:, 0] = truth[:, 4] = truth[:, 8] = 1.0
    truth[:, 9] = -np.arange(P) * spacing
    k = np.arange(P - 1)
    lk = np.arange(0, max(P - loop_every, 0), loop_every)
    vi = np.concatenate([k, lk]).astype(np.int32)
    vj = np.concatenate([k + 1, lk + loop_every]).astype(np.int32)
    h = prob["cam_hidx"]
    keep = (h[vi] >= 0) | (h[vj] >= 0)
    vi, vj = vi[keep], vj[keep]
    n = len(vi)
    rng = CounterRng(seed)
    noise = np.stack([sigma_rot * rng.normal(60 + i, n) for i in range(3)] + [sigma_trans * rng.normal(63 + i, n) for i in range(3)], axis=1)
    meas = X.pack(X.product(X.product(X.unpack(truth[vj]), X.unpack(X.exp(noise))), X.inverse(X.unpack(truth[vi]))))
    info = np.tile(np.diag([1.0 / sigma_rot ** 2] * 3 + [1.0 / sigma_trans ** 2] * 3).reshape(36), (n, 1))
    prob["pose_edges"] = dict(n=n, vi=vi, vj=vj, v0=h[vi].astype(np.int32), v1=h[vj].astype(np.int32), meas=meas, info=info)
    return prob


def make_ba_inverse_depth(P, L, seed=42, **ba_args):
    """make_ba_problem(P, L, seed=seed, **ba_args) (mono) in the anchored inverse-depth parametrisation of EdgeProjectPSI2UV
    (types_six_dof_expmap.h:158-178; g2o/examples/ba_anchored_inverse_depth): the anchor of a point is its first observing camera,
    pts [L][3] holds psi = invert_depth(T_anchor X) of the initial estimates, so that psi2uv.to_world(pts, cams[pt_anchor]) is the
    XYZ scene.  The dictionary gains observation = "inverse_depth", pt_anchor [L], anchor_idx [E] = pt_anchor[pt_idx] and pairs =
    the (v0, v1) hessian indices of the three binary sets that stand for the three-vertex edge -- (point, pose), (point, anchor),
    (pose, anchor) -- with -1 on every camera side of an edge observed by its own anchor (its two camera Jacobians cancel); v0 / v1
    are those of the (point, pose) pair.  Everything else is make_ba_problem's."""
    from . import psi2uv
    assert "stereo_baseline" not in ba_args
    prob = make_ba_problem(P, L, seed=seed, **ba_args)
    cam_idx, pt_idx, h, nP = prob["cam_idx"], prob["pt_idx"], prob["cam_hidx"], prob["nP"]
    K = prob["E"] // L
    pt_anchor = cam_idx.reshape(L, K)[:, 0].astype(np.int32)
    anchor_idx = pt_anchor[pt_idx]
    A = prob["cams"][pt_anchor]
    R = A[:, 0:9].reshape(-1, 3, 3).transpose(0, 2, 1)
    prob["pts"] = psi2uv.invert_depth((R @ prob["pts"][:, :, None])[:, :, 0] + A[:, 9:12])
    own = cam_idx == anchor_idx
    vp = (nP + pt_idx).astype(np.int32)
    vc = np.where(own, -1, h[cam_idx]).astype(np.int32)
    va = np.where(own, -1, h[anchor_idx]).astype(np.int32)
    prob.update(observation="inverse_depth", pt_anchor=pt_anchor, anchor_idx=anchor_idx.astype(np.int32), v0=vp, v1=vc,
                pairs=[(vp, vc), (vp, va), (vc, va)])
    return prob


def make_ba_loops(P, L, laps=4, hubs=3, drop=0.2, seed=7, spacing=0.5, f=1000.0, cx=320.0, cy=240.0, hub_stride=3):
    """A bundle-adjustment graph that is NOT a band: the camera runs `laps` times back and forth along the same line
    (poses of different laps stand at the same places and see the same points -- loop closures everywhere, the reduced
    pose system couples every lap with every other: separators and frontal matrices several times the band case), a
    fraction `drop` of the observations is missing (ragged observation lists, 2 .. 5 laps long) and `hubs` distant points
    are seen by every third pose (`hub_stride`; lists far longer than a wavefront).  Same dictionary as make_ba_problem."""
    rng = CounterRng(seed)
    M = max(P // laps, 6)                                   # positions along the line
    c = np.arange(P, dtype=np.int64)
    lap = c // M
    s_c = np.where(lap % 2 == 0, c % M, M - 1 - (c % M))  # position index of pose c
    pos_of = [np.flatnonzero(s_c == s) for s in range(M)]  # poses standing at position s
    Lr = L - hubs
    j = np.arange(Lr, dtype=np.int64)
    p_j = (j * M) // max(Lr, 1)
    cam_l, pt_l = [], []
    keep_u = rng.uniform(30, Lr * 5 * (laps + 1)).reshape(Lr, -1)
    for jj in range(Lr):
        obs = np.concatenate([pos_of[s] for s in range(max(p_j[jj] - 2, 0), min(p_j[jj] + 3, M))])
        obs.sort()
        k = keep_u[jj, :len(obs)] >= drop
        if k.sum() < 2:
            k[:2] = True
        obs = obs[k]
        cam_l.append(obs)
        pt_l.append(np.full(len(obs), jj))
    for h in range(hubs):
        obs = np.arange(h, P, hub_stride)
        cam_l.append(obs)
        pt_l.append(np.full(len(obs), Lr + h))
    cam_idx = np.concatenate(cam_l).astype(np.int32)
    pt_idx = np.concatenate(pt_l).astype(np.int32)
    E = len(cam_idx)
    true_pts = np.zeros((L, 3))
    true_pts[:Lr] = np.stack([p_j * spacing + (rng.uniform(1, Lr) * 2.0 - 1.0), rng.uniform(2, Lr) - 0.5, 3.0 + rng.uniform(3, Lr)], axis=1)
    for h in range(hubs):
        true_pts[Lr + h] = [0.5 * M * spacing + 3.0 * (h - hubs / 2.0), 1.0 * h, 60.0 + 5.0 * h]
    cams_true = np.zeros((P, 12))
    cams_true[:, 0] = cams_true[:, 4] = cams_true[:, 8] = 1.0
    cams_true[:, 9] = -s_c * spacing
    cams_true[:, 10] = -0.03 * lap
    Xc = true_pts[pt_idx] + cams_true[cam_idx, 9:12]
    meas = np.stack([Xc[:, 0] / Xc[:, 2] * f + cx, Xc[:, 1] / Xc[:, 2] * f + cy], axis=1)
    meas[:, 0] += rng.normal(4, E)
    meas[:, 1] += rng.normal(5, E)
    pts = true_pts + 0.05 * np.stack([rng.normal(6, L), rng.normal(7, L), rng.normal(8, L)], axis=1)
    upd = np.zeros((P, 6))
    upd[:, 0:3] = 0.005 * np.stack([rng.normal(9, P), rng.normal(10, P), rng.normal(11, P)], axis=1)
    upd[:, 3:6] = 0.01 * np.stack([rng.normal(12, P), rng.normal(13, P), rng.normal(14, P)], axis=1)
    upd[:2] = 0.0
    cams = _apply_cam_update(cams_true, upd)
    cam_hidx = np.arange(P, dtype=np.int32) - 2
    cam_hidx[:2] = -1
    nP = P - 2
    return dict(P=P, L=L, E=E, nP=nP, nL=L, f=f, cx=cx, cy=cy, cams=cams, pts=pts, meas=meas,
                cam_idx=cam_idx, pt_idx=pt_idx, cam_hidx=cam_hidx,
                v0=(nP + pt_idx).astype(np.int32), v1=cam_hidx[cam_idx].astype(np.int32))


def make_ba_grid(P, pts_per_cam=10, radius=0.9, seed=11, spacing=0.5, f=1000.0, cx=320.0, cy=240.0):
    """A bundle-adjustment graph with VISIBILITY BY DISTANCE (round 6; the shape of an aerial survey / a street grid seen from above,
    after g2o's ba_demo geometry, g2o/examples/ba/ba_demo.cpp:151-256, and the visibility lists of a BAL file,
    g2o/examples/bal/bal_example.cpp:294-406): G x G cameras stand on a square lattice (pitch `spacing`) in the plane z = 0 and
    look along +z, `pts_per_cam` points per camera are spread uniformly over the area at depth 3 .. 4, and a point is observed by
    EVERY camera within the horizontal distance `radius` of it (6 .. 13 observations per point at the defaults: ragged lists).  Two
    cameras share points when they are closer than 2 x radius: every camera is coupled to ~40 others, the reduced pose system is
    a two-dimensional mesh with a wide stencil -- real fill, separators of hundreds of columns, frontal matrices far beyond the
    24-column register fronts of the camera-trajectory graphs.  P is rounded down to a square.  Same dictionary as
    make_ba_problem (edges point-major, cameras row-major on the lattice, the first two cameras fixed)."""
    rng = CounterRng(seed)
    G = int(np.floor(np.sqrt(P)))
    P = G * G
    L = P * pts_per_cam
    side = (G - 1) * spacing
    px = rng.uniform(1, L) * side
    py = rng.uniform(2, L) * side
    true_pts = np.stack([px, py, 3.0 + rng.uniform(3, L)], axis=1)
    reach = int(np.ceil(radius / spacing))
    off = np.arange(-reach, reach + 1)
    oi, oj = np.meshgrid(off, off, indexing="ij")
    oi, oj = oi.reshape(-1), oj.reshape(-1)
    ci = np.rint(px / spacing).astype(np.int64)[:, None] + oi[None, :]
    cj = np.rint(py / spacing).astype(np.int64)[:, None] + oj[None, :]
    d2 = (ci * spacing - px[:, None]) ** 2 + (cj * spacing - py[:, None]) ** 2
    vis = (ci >= 0) & (ci < G) & (cj >= 0) & (cj < G) & (d2 <= radius * radius)
    cam_all = (ci * G + cj)
    # point-major edge list, cameras ascending inside a list
    order = np.argsort(np.where(vis, cam_all, np.iinfo(np.int64).max), axis=1, kind="stable")
    cam_sorted = np.take_along_axis(cam_all, order, axis=1)
    vis_sorted = np.take_along_axis(vis, order, axis=1)
    cam_idx = cam_sorted[vis_sorted].astype(np.int32)
    pt_idx = np.repeat(np.arange(L, dtype=np.int32), vis_sorted.sum(axis=1))
    assert vis_sorted.sum(axis=1).min() >= 2, "a point with fewer than two observations"
    E = len(cam_idx)
    cams_true = np.zeros((P, 12))
    cams_true[:, 0] = cams_true[:, 4] = cams_true[:, 8] = 1.0
    cams_true[:, 9] = -(np.arange(P) // G) * spacing
    cams_true[:, 10] = -(np.arange(P) % G) * spacing
    Xc = true_pts[pt_idx] + cams_true[cam_idx, 9:12]
    meas = np.stack([Xc[:, 0] / Xc[:, 2] * f + cx, Xc[:, 1] / Xc[:, 2] * f + cy], axis=1)
    meas[:, 0] += rng.normal(4, E)
    meas[:, 1] += rng.normal(5, E)
    pts = true_pts + 0.05 * np.stack([rng.normal(6, L), rng.normal(7, L), rng.normal(8, L)], axis=1)
    upd = np.zeros((P, 6))
    upd[:, 0:3] = 0.005 * np.stack([rng.normal(9, P), rng.normal(10, P), rng.normal(11, P)], axis=1)
    upd[:, 3:6] = 0.01 * np.stack([rng.normal(12, P), rng.normal(13, P), rng.normal(14, P)], axis=1)
    upd[:2] = 0.0
    cams = _apply_cam_update(cams_true, upd)
    cam_hidx = np.arange(P, dtype=np.int32) - 2
    cam_hidx[:2] = -1
    nP = P - 2
    return dict(P=P, L=L, E=E, nP=nP, nL=L, f=f, cx=cx, cy=cy, cams=cams, pts=pts, meas=meas,
                cam_idx=cam_idx, pt_idx=pt_idx, cam_hidx=cam_hidx,
                v0=(nP + pt_idx).astype(np.int32), v1=cam_hidx[cam_idx].astype(np.int32))


def _apply_cam_update(cams, upd):
    """estimate <- exp(update) * estimate, update = (omega, upsilon)."""
    R, V = _exp_so3(upd[:, 0:3])
    Rold = cams[:, 0:9].reshape(-1, 3, 3).transpose(0, 2, 1)       # stored column-major
    told = cams[:, 9:12]
    Rn = R @ Rold
    tn = (R @ told[:, :, None])[:, :, 0] + (V @ upd[:, 3:6, None])[:, :, 0]
    out = np.empty_like(cams)
    out[:, 0:9] = Rn.transpose(0, 2, 1).reshape(-1, 9)
    out[:, 9:12] = tn
    return out


def ba_linearize(prob, jac=True):
    """Returns (Jpt [E,6] 2x3 col-major, Jcam [E,12] 2x6 col-major, err [E,2]) or err only."""
    cams, pts = prob["cams"], prob["pts"]
    f, cx, cy = prob["f"], prob["cx"], prob["cy"]
    T = cams[prob["cam_idx"]]
    X = pts[prob["pt_idx"]]
    R = T[:, 0:9].reshape(-1, 3, 3).transpose(0, 2, 1)
    Xc = (R @ X[:, :, None])[:, :, 0] + T[:, 9:12]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    err = np.stack([prob["meas"][:, 0] - (x / z * f + cx), prob["meas"][:, 1] - (y / z * f + cy)], axis=1)
    if not jac:
        return err
    E = len(x)
    z2 = z * z
    tmp = np.zeros((E, 2, 3))
    tmp[:, 0, 0] = f
    tmp[:, 0, 2] = -x / z * f
    tmp[:, 1, 1] = f
    tmp[:, 1, 2] = -y / z * f
    A = (-1.0 / z)[:, None, None] * (tmp @ R)
    Jpt = np.ascontiguousarray(A.transpose(0, 2, 1).reshape(E, 6))          # column-major 2x3
    B = np.zeros((E, 2, 6))
    B[:, 0, 0] = x * y / z2 * f
    B[:, 0, 1] = -(1 + (x * x / z2)) * f
    B[:, 0, 2] = y / z * f
    B[:, 0, 3] = -1.0 / z * f
    B[:, 0, 5] = x / z2 * f
    B[:, 1, 0] = (1 + y * y / z2) * f
    B[:, 1, 1] = -x * y / z2 * f
    B[:, 1, 2] = -x / z * f
    B[:, 1, 4] = -1.0 / z * f
    B[:, 1, 5] = y / z2 * f
    Jcam = np.ascontiguousarray(B.transpose(0, 2, 1).reshape(E, 12))
    return Jpt, Jcam, err


def ba_omega(prob):
    om = np.zeros((prob["E"], 4))
    om[:, 0] = om[:, 3] = 1.0
    return om


def ba_oplus(prob, x):
    """Apply a solver update (poses then landmarks) and return a new problem dict."""
    nP = prob["nP"]
    xp = x[:6 * nP].reshape(nP, 6)
    xl = x[6 * nP:].reshape(prob["nL"], 3)
    upd = np.zeros((prob["P"], 6))
    free = prob["cam_hidx"] >= 0
    upd[free] = xp[prob["cam_hidx"][free]]
    new = dict(prob)
    new["cams"] = _apply_cam_update(prob["cams"], upd)
    new["pts"] = prob["pts"] + xl
    return new


def _quat_to_rot(q):
    """Unit quaternions [n,4] (x, y, z, w) -> rotation matrices [n,3,3]."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - z * w); R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w); R[:, 2, 1] = 2 * (y * z + x * w); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _iso_pack(R, t):
    """[n,3,3], [n,3] -> [n,12] (R column-major | t): the isometry layout of the device front ends and the oracle."""
    return np.concatenate([R.transpose(0, 2, 1).reshape(-1, 9), t], axis=1)


def make_sphere(nodes_per_level=50, laps=50, radius=100.0, noise_translation=0.01, noise_rotation=0.005, seed=42):
    """The generator of BASELINE.json's config 2 in its stated size: g2o's `create_sphere` with its defaults
    (g2o/examples/sphere/create_sphere.cpp:55-57: 50 nodes per lap x 50 laps = 2 500 VertexSE3 on a sphere of radius 100;
    :99-147 odometry edges between successive vertices and three loop closures per vertex to the lap before; :149-176
    measurement noise sigma_t = 0.01, sigma_r = 0.005 on the quaternion's vector part with w = 1 - |v| before the
    normalisation; :178-185 initial estimates by chaining the NOISY odometry), with this module's counter-based RNG instead
    of the reference's unseeded sampler.  Vertex 0 is fixed.  Returns isometries as [n,12] (R column-major | t)."""
    n = nodes_per_level * laps
    idx = np.arange(n)
    nn, f = idx % nodes_per_level, idx // nodes_per_level
    az = -np.pi + 2.0 * nn * np.pi / nodes_per_level
    ay = -0.5 * np.pi + (idx + 1) * np.pi / n                 # (the reference uses the post-incremented id here)
    cz, sz, cy, sy = np.cos(az), np.sin(az), np.cos(ay), np.sin(ay)
    Rz = np.zeros((n, 3, 3)); Ry = np.zeros((n, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = cz, -sz, sz, cz, 1.0
    Ry[:, 0, 0], Ry[:, 0, 2], Ry[:, 2, 0], Ry[:, 2, 2], Ry[:, 1, 1] = cy, sy, -sy, cy, 1.0
    R = Rz @ Ry
    t = R[:, :, 0] * radius
    vi = [np.arange(n - 1)]
    vj = [np.arange(1, n)]
    for lap in range(1, laps):
        for d in (-1, 0, 1):
            a = (lap - 1) * nodes_per_level + np.arange(nodes_per_level)
            b = lap * nodes_per_level + np.arange(nodes_per_level) + d
            if lap == laps - 1 and d == 1:
                continue
            vi.append(a)
            vj.append(b)
    # (the reference emits the three closures of a vertex together; the order of the edges only matters for the noise stream)
    vi, vj = np.concatenate(vi).astype(np.int32), np.concatenate(vj).astype(np.int32)
    E = len(vi)
    Rt = R.transpose(0, 2, 1)
    Rm = Rt[vi] @ R[vj]                                          # from^-1 * to
    tm = np.einsum("nij,nj->ni", Rt[vi], t[vj] - t[vi])
    rng = CounterRng(seed)
    qv = np.stack([rng.normal(100 + c, E) for c in range(3)], axis=1) * noise_rotation
    qw = np.maximum(1.0 - np.linalg.norm(qv, axis=1), 0.0)
    q = np.concatenate([qv, qw[:, None]], axis=1)
    q /= np.linalg.norm(q, axis=1)[:, None]
    Rm = Rm @ _quat_to_rot(q)
    tm = tm + np.stack([rng.normal(110 + c, E) for c in range(3)], axis=1) * noise_translation
    # initial estimates: vertex 0 at its true pose, the others by chaining the noisy odometry (EdgeSE3::initialEstimate)
    Re, te = np.empty_like(R), np.empty_like(t)
    Re[0], te[0] = R[0], t[0]
    for i in range(1, n):
        Re[i] = Re[i - 1] @ Rm[i - 1]
        te[i] = Re[i - 1] @ tm[i - 1] + te[i - 1]
    info = np.zeros((6, 6))
    info[:3, :3] = np.eye(3) / noise_translation ** 2
    info[3:, 3:] = np.eye(3) / noise_rotation ** 2
    hidx = np.arange(n, dtype=np.int32) - 1                      # vertex 0 fixed
    return dict(n=n, nP=n - 1, E=E, vi=vi, vj=vj, poses=_iso_pack(Re, te), poses_true=_iso_pack(R, t), Z=_iso_pack(Rm, tm),
                omega=np.tile(info.T.reshape(1, 36), (E, 1)), hidx=hidx)


def _wrap(theta):
    """normalize_theta (g2o/stuff/misc.h): into [-pi, pi)."""
    return (np.asarray(theta) + np.pi) % (2.0 * np.pi) - np.pi


def make_landmark_slam(kind, n_poses, n_landmarks, laps=3, sensor_range=4.0, window=2, max_obs=None, seed=42,
                       noise_odometry=(0.02, 0.01), noise_landmark=0.05, outlier_frac=0.0, perturb=(0.1, 0.02, 0.2),
                       closure_stride=5, fixed_landmarks=0, observation="xyz", kcam=(525.0, 515.0, 319.5, 239.5), z_min=1.0, *,
                       priors=None, prior_stride=10, noise_prior=(0.3, 0.05), gauge="fixed"):
    """Landmark SLAM graph: odometry between poses plus point landmarks observed from them.
    kind "se2": VertexSE2 / VertexPointXY with EdgeSE2 + EdgeSE2PointXY; "se3": VertexSE3 / VertexPointXYZ with EdgeSE3 +
    EdgeSE3PointXYZ and one non-identity sensor offset (ParameterSE3Offset).
    The robot drives `laps` times round the same loop (radius chosen for a step of ~1 between poses; in 3-D the loop also
    rises and falls), so every place is revisited.  Edges: odometry between successive poses and a loop closure to the pose
    one lap earlier every `closure_stride` poses.  Landmark j sits within half the sensor range of the pose c_j = floor(j *
    per_lap / n_landmarks) and is observed from the poses c_j - window .. c_j + window of EVERY lap that are within
    `sensor_range` of it (at least from the nearest of them), at most `max_obs` of them.  Measurements carry Gaussian noise
    (noise_odometry = (translation, rotation) sigma, noise_landmark sigma; the information matrices match), a fraction
    `outlier_frac` of the observations gets a gross error on top; the initial estimates are the ground truth perturbed
    by N(0, perturb = (pose translation, pose rotation, landmark)).  Pose 0 is fixed (gauge) and the first `fixed_landmarks`
    landmarks.  Counter-based RNG: the same seed gives the same graph anywhere.  Ground truth: poses_true, points_true.
    Layout: SE2 poses (x, y, theta), SE3 poses / measurements isometries [12]; hidx / pt_hidx hessian indices (landmarks
    behind the poses: nP + number among the free landmarks; -1 fixed).
    observation = "depth" | "disparity" (kind "se3" only): the observations are EdgeSE3PointXYZDepth / EdgeSE3PointXYZDisparity
    of one forward-looking camera (ParameterCamera: the returned `offset` and `kcam` = (fx, fy, cx, cy)), measurements (u, v,
    depth) / (u, v, 1 / depth).  Landmark j then lies in front of the camera of its anchor pose, and of the candidate
    observers only those are kept that see it at a sensor-frame depth in [z_min, sensor_range], z_min > 0, both at the ground
    truth and at the initial estimates (the reference has no guard for a point behind the image plane); a landmark left with
    no observation is an error.  Information: the reference's defaults diag(1, 1, 100) (depth) / diag(1, 1, 1000) (disparity);
    the noise matches them: sigma 1 pixel, 0.1 m, 1000^-1/2 m^-1.  Outliers: up to 50 pixels and half the depth / disparity
    range.  The dict then also carries `observation` and `kcam`.
    priors = "pose" | "xy": unary priors on poses (GPS-like fixes) -- EdgeSE2Prior / EdgeSE3Prior on the whole pose, or
    EdgeSE2XYPrior on the position alone ("xy": kind "se2" only) -- on every `prior_stride`-th pose (0, stride, 2 stride, ...)
    PLUS a second, independently measured one on pose `prior_stride`, so that one vertex carries two priors.  Measurements:
    the ground truth with noise_prior = (translation, rotation) sigma, matching information matrices; the 3-D prior is taken
    through a lever arm `prior_offset` (ParameterSE3Offset, distinct from the sensor `offset`): Z = X prior_offset noise.  The
    dict then also carries prior (= priors), vq (pose of every prior), zq ([n][3 | 2 | 12]), omega_q and, 3-D, prior_offset.
    gauge = "free" (needs priors): no pose is fixed, every hidx >= 0 and nP = n; the priors alone hold the gauge.  With
    priors=None and gauge="fixed" the dict is what it was before these options existed."""
    if kind not in ("se2", "se3"):
        raise ValueError("kind must be 'se2' or 'se3'")
    if priors not in (None, "pose", "xy"):
        raise ValueError("priors must be None, 'pose' or 'xy'")
    if priors == "xy" and kind != "se2":
        raise ValueError("priors = 'xy' (EdgeSE2XYPrior) belongs to kind 'se2'")
    if gauge not in ("fixed", "free"):
        raise ValueError("gauge must be 'fixed' or 'free'")
    if gauge == "free" and priors is None:
        raise ValueError("gauge = 'free' needs priors: nothing else holds the gauge")
    if priors is not None and int(prior_stride) < 1:
        raise ValueError("prior_stride must be at least 1")
    if observation not in ("xyz", "depth", "disparity"):
        raise ValueError("observation must be 'xyz', 'depth' or 'disparity'")
    se2 = kind == "se2"
    camera = observation != "xyz"
    if camera and se2:
        raise ValueError("depth / disparity observations belong to kind 'se3'")
    if camera and not z_min > 0:
        raise ValueError("z_min must be positive")
    rng = CounterRng(seed)
    n, L = int(n_poses), int(n_landmarks)
    per_lap = max(4, n // laps)
    radius = per_lap / (2.0 * np.pi)
    k = np.arange(n)
    ang = 2.0 * np.pi * (k % per_lap) / per_lap
    lap = k // per_lap
    wob = 0.15 * np.sin(3.0 * ang + 0.7 * lap)                      # laps differ a little: revisits are near, not identical
    px, py = (radius + wob) * np.cos(ang), (radius + wob) * np.sin(ang)
    yaw = ang + 0.5 * np.pi
    dl = 2 if se2 else 3
    if se2:
        pos = np.stack([px, py], axis=1)
        poses_true = np.stack([px, py, _wrap(yaw)], axis=1)
    else:
        pz = 0.1 * radius * np.sin(2.0 * ang) + 0.05 * lap
        pos = np.stack([px, py, pz], axis=1)
        R = _exp_so3(np.stack([0.05 * np.sin(ang), 0.05 * np.cos(2 * ang), yaw], axis=1))[0]
        poses_true = _iso_pack(R, pos)
    # landmarks around their anchor pose (first lap)
    anchor = np.minimum((np.arange(L) * per_lap) // max(L, 1), per_lap - 1)
    off = np.stack([rng.uniform(200 + c, L) for c in range(dl)], axis=1) * 2.0 - 1.0
    points_true = pos[anchor] + off * (0.5 * sensor_range / np.sqrt(dl))
    # candidate observers: the window round the anchor in every lap
    n_laps = (n + per_lap - 1) // per_lap
    dw = np.arange(-window, window + 1)
    cand = (anchor[:, None, None] + dw[None, None, :]) % per_lap + per_lap * np.arange(n_laps)[None, :, None]
    cand = cand.reshape(L, -1)
    dist = np.linalg.norm(pos[np.minimum(cand, n - 1)] - points_true[:, None, :], axis=2)
    dist = np.where(cand < n, dist, np.inf)
    seen = dist <= sensor_range
    seen[np.arange(L), np.argmin(dist, axis=1)] = True              # every landmark is observed at least once
    if camera:
        # a camera looking along the robot's x axis (image x to the right, y down), slightly tilted and off-centre
        Ro = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]]) @ _exp_so3(np.array([[0.05, -0.03, 0.04]]))[0][0]
        to = np.array([0.2, -0.1, 0.3])
        u = (off + 1.0) * 0.5
        depth = sensor_range * (0.5 + 0.4 * u[:, 0])
        q = np.stack([0.6 * depth * (2.0 * u[:, 1] - 1.0), 0.4 * depth * (2.0 * u[:, 2] - 1.0), depth], axis=1)
        points_true = np.einsum("nij,nj->ni", R[anchor] @ Ro, q) + np.einsum("nij,j->ni", R[anchor], to) + pos[anchor]
        # the initial estimates (the same draws as below) decide with the ground truth which observations are kept
        Ri = R @ _exp_so3(np.stack([rng.normal(223 + c, n) for c in range(3)], axis=1) * perturb[1])[0]
        ti = pos + perturb[0] * np.stack([rng.normal(220 + c, n) for c in range(3)], axis=1)
        Ri[0], ti[0] = R[0], pos[0]
        pi = points_true + perturb[2] * np.stack([rng.normal(250 + c, L) for c in range(dl)], axis=1)
        pi[:fixed_landmarks] = points_true[:fixed_landmarks]
        seen = cand < n
        cc = np.minimum(cand, n - 1)
        for Rx, tx, px_ in ((R, pos, points_true), (Ri, ti, pi)):
            zax = Rx[cc] @ Ro[:, 2]                                     # the camera's viewing direction in the world
            z = np.einsum("lki,lki->lk", zax, px_[:, None, :] - (np.einsum("lkij,j->lki", Rx[cc], to) + tx[cc]))
            seen &= (z >= z_min) & (z <= sensor_range)
        if not seen.any(axis=1).all():
            raise ValueError("landmark %d is seen by no candidate pose at a depth in [z_min, sensor_range]: smaller perturb or "
                             "z_min, larger window or sensor_range" % int(np.argmin(seen.any(axis=1))))
    if max_obs is not None:
        seen &= np.cumsum(seen, axis=1) <= max_obs
    lm_i, slot = np.nonzero(seen)
    vp = cand[lm_i, slot].astype(np.int32)
    vl = lm_i.astype(np.int32)
    order = np.lexsort((vl, vp))                                    # observations in the order the robot makes them
    vp, vl = vp[order], vl[order]
    M = len(vp)
    # odometry + loop closures
    a = [np.arange(n - 1)]
    b = [np.arange(1, n)]
    if n > per_lap:
        c = np.arange(per_lap, n, max(1, closure_stride))
        a.append(c - per_lap)
        b.append(c)
    vi, vj = np.concatenate(a).astype(np.int32), np.concatenate(b).astype(np.int32)
    E = len(vi)
    st, sr = noise_odometry
    if se2:
        c, s = np.cos(poses_true[vi, 2]), np.sin(poses_true[vi, 2])
        d = poses_true[vj, :2] - poses_true[vi, :2]
        Z = np.stack([c * d[:, 0] + s * d[:, 1] + st * rng.normal(210, E), -s * d[:, 0] + c * d[:, 1] + st * rng.normal(211, E),
                      _wrap(poses_true[vj, 2] - poses_true[vi, 2] + sr * rng.normal(212, E))], axis=1)
        info = np.diag([1 / st ** 2, 1 / st ** 2, 1 / sr ** 2])
        c, s = np.cos(poses_true[vp, 2]), np.sin(poses_true[vp, 2])
        d = points_true[vl] - poses_true[vp, :2]
        zl = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1)
        offset = None
        poses = poses_true + np.stack([perturb[0] * rng.normal(220, n), perturb[0] * rng.normal(221, n), perturb[1] * rng.normal(222, n)], axis=1)
        poses[:, 2] = _wrap(poses[:, 2])
    else:
        Rt = R.transpose(0, 2, 1)
        Rm = Rt[vi] @ R[vj] @ _exp_so3(np.stack([rng.normal(213 + q, E) for q in range(3)], axis=1) * sr)[0]
        tm = np.einsum("nij,nj->ni", Rt[vi], pos[vj] - pos[vi]) + st * np.stack([rng.normal(210 + q, E) for q in range(3)], axis=1)
        Z = _iso_pack(Rm, tm)
        info = np.zeros((6, 6))
        info[:3, :3] = np.eye(3) / st ** 2
        info[3:, 3:] = np.eye(3) / (0.5 * sr) ** 2                  # (the error's rotation part is the quaternion vector: half the angle)
        if not camera:
            Ro = _exp_so3(np.array([[0.1, -0.2, 0.3]]))[0][0]       # the sensor is mounted off-centre and rotated
            to = np.array([0.2, -0.1, 0.3])
        offset = _iso_pack(Ro[None], to[None])[0]
        Rn = R[vp] @ Ro                                             # n2w = X * offset
        tn = np.einsum("nij,j->ni", R[vp], to) + pos[vp]
        zl = np.einsum("nji,nj->ni", Rn, points_true[vl] - tn)
        Rp = R @ _exp_so3(np.stack([rng.normal(223 + q, n) for q in range(3)], axis=1) * perturb[1])[0]
        poses = _iso_pack(Rp, pos + perturb[0] * np.stack([rng.normal(220 + q, n) for q in range(3)], axis=1))
    poses[0] = poses_true[0]
    if camera:
        fx, fy, cx, cy = (float(v) for v in kcam)
        third = zl[:, 2] if observation == "depth" else 1.0 / zl[:, 2]
        zl = np.stack([(fx * zl[:, 0] + cx * zl[:, 2]) / zl[:, 2], (fy * zl[:, 1] + cy * zl[:, 2]) / zl[:, 2], third], axis=1)
        info_l = np.diag([1.0, 1.0, 100.0 if observation == "depth" else 1000.0])
        gross = np.array([50.0, 50.0, 0.5 * sensor_range if observation == "depth" else 0.5 / z_min])
        zl = zl + np.stack([rng.normal(230 + q, M) for q in range(dl)], axis=1) / np.sqrt(np.diag(info_l))
    else:
        info_l = np.eye(dl) / noise_landmark ** 2
        gross = sensor_range
        zl = zl + noise_landmark * np.stack([rng.normal(230 + q, M) for q in range(dl)], axis=1)
    if outlier_frac > 0:
        bad = rng.uniform(240, M) < outlier_frac
        zl = zl + bad[:, None] * gross * (np.stack([rng.uniform(241 + q, M) for q in range(dl)], axis=1) * 2.0 - 1.0)
    points = points_true + perturb[2] * np.stack([rng.normal(250 + q, L) for q in range(dl)], axis=1)
    points[:fixed_landmarks] = points_true[:fixed_landmarks]
    hidx = np.arange(n, dtype=np.int32) - 1                         # pose 0 fixed
    nP, nL = n - 1, L - int(fixed_landmarks)
    if gauge == "free":
        hidx, nP = np.arange(n, dtype=np.int32), n
    pt_hidx = np.where(np.arange(L) < fixed_landmarks, -1, nP + np.arange(L) - int(fixed_landmarks)).astype(np.int32)
    dp = 3 if se2 else 6
    out = dict(kind=kind, n=n, L=L, nP=nP, nL=nL, E=E, M=M, vi=vi, vj=vj, Z=Z, omega=np.tile(info.T.reshape(1, dp * dp), (E, 1)),
               vp=vp, vl=vl, zl=zl, omega_l=np.tile(info_l.reshape(1, dl * dl), (M, 1)),
               offset=offset, poses=poses, poses_true=poses_true, points=points, points_true=points_true, hidx=hidx,
               pt_hidx=pt_hidx)
    if camera:
        out.update(observation=observation, kcam=np.array([float(v) for v in kcam]))
    if priors is not None:
        stride = int(prior_stride)
        vq = np.concatenate([np.arange(0, n, stride), [stride] if stride < n else []]).astype(np.int32)
        Q = len(vq)
        pt, pr = noise_prior
        if se2:
            xy = poses_true[vq, :2] + pt * np.stack([rng.normal(260, Q), rng.normal(261, Q)], axis=1)
            if priors == "xy":
                zq, info_q = xy, np.eye(2) / pt ** 2
            else:
                zq = np.concatenate([xy, _wrap(poses_true[vq, 2] + pr * rng.normal(262, Q))[:, None]], axis=1)
                info_q = np.diag([1 / pt ** 2, 1 / pt ** 2, 1 / pr ** 2])
        else:
            Rq = _exp_so3(np.array([[-0.2, 0.15, 0.1]]))[0][0]       # the lever arm of the prior's sensor (a GPS antenna)
            tq = np.array([-0.3, 0.2, 0.1])
            out.update(prior_offset=_iso_pack(Rq[None], tq[None])[0])
            Rz = R[vq] @ Rq @ _exp_so3(np.stack([rng.normal(263 + q, Q) for q in range(3)], axis=1) * pr)[0]
            tz = np.einsum("nij,j->ni", R[vq], tq) + pos[vq] + pt * np.stack([rng.normal(260 + q, Q) for q in range(3)], axis=1)
            zq = _iso_pack(Rz, tz)
            info_q = np.zeros((6, 6))
            info_q[:3, :3] = np.eye(3) / pt ** 2
            info_q[3:, 3:] = np.eye(3) / (0.5 * pr) ** 2              # (quaternion vector: half the angle)
        out.update(prior=priors, vq=vq, zq=zq, omega_q=np.tile(info_q.reshape(1, -1), (Q, 1)))
    return out


def make_sim3_graph(n, loop_every, scale_drift, seed, fix_scale=False, noise=1.0):
    """A closed monocular trajectory as a 7-dof pose graph (VertexSim3Expmap / EdgeSim3, g2o/types/sim3): n poses on two laps
    of a circle, looking at its centre; the estimate of a pose is the world -> camera Sim3 (qx, qy, qz, qw, tx, ty, tz, s)
    with s = 1.  Odometry edges (k, k + 1), the closing edge (n - 1, 0) and, every loop_every poses of the first lap, a loop
    closure to the pose one lap later.  The measurement of (i, j) is exp(noise) Sj Si^-1 of the ground truth, so that
    EdgeSim3::computeError = log(C Si Sj^-1) vanishes there without noise (noise = 0; the standard deviations 0.01 rotation,
    0.02 translation, 0.01 log-scale are multiplied by it).  The initial estimate chains the odometry from pose 0 and
    multiplies the scale by (1 + scale_drift) at every step -- the drift monocular odometry accumulates and a loop closure has to
    take out again; with fix_scale (VertexSim3Expmap::_fix_scale for every vertex: the optimisation cannot move s) the drift
    is left out and the scales stay 1.  Vertex 0 is fixed.  Deterministic from seed.
    Returns est, est_true [n][8], hidx, num_free, vi, vj, meas [m][8], info [m][49], fix_scale."""
    from . import sim3 as S3
    F = S3.FP64
    rng = CounterRng(seed)
    lap = max(2, n // 2)
    ang = 2.0 * np.pi * np.arange(n) / lap
    radius = 0.25 * lap
    wob = 0.05 * rng.normal(1, n)
    true = np.zeros((n, 8))
    for k in range(n):
        c = np.array([radius * np.cos(ang[k]), radius * np.sin(ang[k]), 0.3 * np.sin(3 * ang[k]) + wob[k]])
        z = -c / np.linalg.norm(c)                                   # optical axis towards the centre
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        Rcw = np.stack([x, np.cross(z, x), z])                       # rows: camera axes in the world
        q = S3.R_to_q(F, Rcw.tolist())
        true[k] = q + list(-Rcw @ c) + [1.0]
    vi = list(range(n - 1)) + [n - 1] + [k for k in range(0, n - lap, max(1, loop_every))]
    vj = list(range(1, n)) + [0] + [k + lap for k in range(0, n - lap, max(1, loop_every))]
    m = len(vi)
    sd = noise * np.array([0.01] * 3 + [0.02] * 3 + [0.01])
    nz = np.stack([rng.normal(10 + c, m) for c in range(7)], axis=1) * sd
    meas = np.zeros((m, 8))
    for e in range(m):
        rel = S3.sim3_mul(F, true[vj[e]], S3.sim3_inverse(F, true[vi[e]]))
        meas[e] = S3.to_f64(S3.sim3_mul(F, S3.sim3_exp(F, nz[e]), rel) if noise else rel)
    info = np.tile(np.diag([1e4] * 3 + [2500.0] * 3 + [1e4]).reshape(49), (m, 1))
    est = true.copy()
    drift = [0.0] * 6 + [0.0 if fix_scale else float(np.log1p(scale_drift))]
    for k in range(n - 1):                                           # Sj = C Si along the odometry
        est[k + 1] = S3.to_f64(S3.sim3_mul(F, S3.sim3_exp(F, drift), S3.sim3_mul(F, meas[k], est[k])))
    hidx = np.arange(n, dtype=np.int32) - 1
    return dict(est=est, est_true=true, hidx=hidx, num_free=n - 1, vi=np.asarray(vi, np.int32), vj=np.asarray(vj, np.int32),
                meas=meas, info=info, fix_scale=bool(fix_scale))


def make_sim3_ba(n_cams, n_points, obs_per_point, seed, sim3_edges=True, fix_scale=False, pixel_noise=0.5, scale_drift=0.01):
    """Monocular loop closing with map points (BlockSolver_7_3): the cameras of make_sim3_graph(n_cams, ...) -- a drifting
    closed trajectory of VertexSim3Expmap, initial estimates chained along the noisy odometry -- observing VertexSBAPointXYZ
    points through EdgeSim3ProjectXYZ.  Every camera has intrinsics of its own (fx != fy, non-zero cx, cy, all different between
    cameras: VertexSim3Expmap::_focal_length / _principle_point).  The points lie in a ball around the centre the cameras look
    at, 0.2 of the trajectory's radius wide, so that every point is in front of every camera with a depth >= 1 in camera units
    (checked for the true and for the initial poses; n_cams >= 12); point j is observed by obs_per_point cameras spread over the
    trajectory, measurement = its projection through the TRUE camera + pixel_noise * N(0, 1), information = identity.  The
    initial points are the true ones + 0.02 * N(0, 1).  The first two cameras are fixed (the gauge of a similarity
    reconstruction).  sim3_edges=False leaves the EdgeSim3 set empty (keyframes and points, no constraints between keyframes);
    the initial poses are the same.  Deterministic from seed.
    Returns the keys of make_sim3_graph (hidx / num_free for two fixed cameras) plus nP, nL, points, points_true [L][3], pt_hidx,
    vp, vl, zl [m][2], omega_l [m][4], intrinsics [n_cams][4] = (fx, fy, cx, cy)."""
    from . import sim3 as S3
    F = S3.FP64
    if obs_per_point < 1 or obs_per_point > n_cams:
        raise ValueError("make_sim3_ba: 1 <= obs_per_point <= n_cams")
    g = make_sim3_graph(n_cams, max(1, n_cams // 4), scale_drift, seed, fix_scale)
    rng = CounterRng(seed + 1)
    radius = 0.25 * max(2, n_cams // 2)
    d = np.stack([rng.normal(40 + c, n_points) for c in range(3)], axis=1)
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    pts_true = d * (0.2 * radius * rng.uniform(43, n_points) ** (1.0 / 3.0))[:, None]
    pts = pts_true + 0.02 * np.stack([rng.normal(44 + c, n_points) for c in range(3)], axis=1)
    k = np.arange(n_cams)
    intr = np.stack([480.0 + 7.0 * k, 510.0 + 5.0 * k, 320.0 + 3.0 * k, 240.0 - 2.0 * k], axis=1)
    stride = max(1, n_cams // obs_per_point)
    start = np.minimum((rng.uniform(47, n_points) * n_cams).astype(np.int64), n_cams - 1)
    vp = ((start[:, None] + stride * np.arange(obs_per_point)[None, :]) % n_cams).reshape(-1).astype(np.int32)
    vl = np.repeat(np.arange(n_points, dtype=np.int32), obs_per_point)
    m = len(vp)
    zero2 = np.zeros((m, 2))
    zl = -S3.project_edges(F, g["est_true"], pts_true, vp, vl, zero2, intr, jac=False)        # e = z - proj: z = 0 gives -proj
    zl = zl + pixel_noise * np.stack([rng.normal(48 + c, m) for c in range(2)], axis=1)
    for poses, X in ((g["est_true"], pts_true), (g["est"], pts)):
        depth = np.array([S3.sim3_map(F, poses[vp[e]], X[vl[e]])[2] for e in range(m)])
        if not (depth >= 1.0).all():
            raise ValueError("make_sim3_ba: an observed depth below 1 camera unit (%g): use n_cams >= 12" % depth.min())
    hidx = np.maximum(np.arange(n_cams, dtype=np.int32) - 2, -1)
    nP = n_cams - 2
    out = dict(g)
    if not sim3_edges:
        out.update(vi=np.zeros(0, np.int32), vj=np.zeros(0, np.int32), meas=np.zeros((0, 8)), info=np.zeros((0, 49)))
    out.update(hidx=hidx, num_free=nP, nP=nP, nL=n_points, points=pts, points_true=pts_true,
               pt_hidx=(nP + np.arange(n_points)).astype(np.int32), vp=vp, vl=vl, zl=zl,
               omega_l=np.tile(np.eye(2).reshape(1, 4), (m, 1)), intrinsics=intr)
    return out


def _sbacam_project(cams, X, vp, vl, intr, stereo):
    """(proj [m][2|3], depth [m]) of points X[vl] in the cameras cams[vp], vectorised (the scalar statement is sbacam.py's)."""
    from .g2o_io import _quat_to_R
    R = _quat_to_R(cams[:, 3:7])[vp]
    pc = np.einsum("mji,mj->mi", R, X[vl] - cams[vp, 0:3])             # R' (X - t)
    k = intr[vp]
    cols = [(k[:, 0] * pc[:, 0] + k[:, 2] * pc[:, 2]) / pc[:, 2], (k[:, 1] * pc[:, 1] + k[:, 3] * pc[:, 2]) / pc[:, 2]]
    if stereo:
        cols.append((k[:, 0] * (pc[:, 0] - k[:, 4]) + k[:, 2] * pc[:, 2]) / pc[:, 2])
    return np.stack(cols, axis=1), pc[:, 2]


def make_sbacam_ba(n_cams, n_points, obs_per_point, stereo=False, seed=0, pixel_noise=0.2, cam_edges=None, scale_edges=None,
                   sigma_trans=0.01, sigma_rot=0.002, sigma_scale=0.01):
    """Bundle adjustment in the reference's SBA format (BlockSolver_6_3): VertexCam cameras (camera-to-world, (tx, ty, tz, qx,
    qy, qz, qw)) on a closed trajectory -- a circle of radius 4 with a vertical wave -- looking at the centre, observing
    VertexSBAPointXYZ points of a ball of radius 1 around it through EdgeProjectP2MC (stereo=False, measurement (u, v)) or
    EdgeProjectP2SC (stereo=True, (u, v, u_right)).  Every camera has intrinsics and a baseline of its own (fx != fy, non-zero
    cx, cy, all different between cameras: SBACam::Kcam / baseline), so every observed depth is 2.5 ... 5.5 camera units (checked
    for the true and the initial cameras).  Point j is observed by obs_per_point cameras spread over the trajectory, measurement
    = its projection through the TRUE camera + pixel_noise * N(0, 1), information = identity (the .g2o format stores none:
    types_sba.cpp:204-244).  Initial cameras: the true ones moved by 0.05 * N(0, 1) in t and a small quaternion 0.02 * N(0, 1)
    through SBACam::update; initial points: the true ones + 0.02 * N(0, 1).  The first camera is fixed at its true pose.
    Deterministic from seed.
    cam_edges = k (an int; None: none) adds EdgeSBACam constraints: odometry between consecutive cameras (i, i + 1) and, for
    k >= 2, loop edges (i, (i + k) mod n_cams) for i = 0, k, 2k, ...; the measurement is the true relative pose Ci^-1 Cj moved by
    sigma_trans * N(0, 1) in t and a small quaternion sigma_rot * N(0, 1) through SBACam::update, information = diag(1 /
    sigma_trans^2 x 3, 1 / sigma_rot^2 x 3).  scale_edges = m (None: none) adds m EdgeSBAScale constraints between cameras half a
    trajectory apart: the true distance + sigma_scale * N(0, 1), information 1 / sigma_scale^2.  n_points = 0 gives a pure
    camera graph (no points, no observations).  With both at None the problem is the one of earlier versions, bit for bit.
    Returns est [n_cams][7], est_true, points [L][3], points_true, hidx, pt_hidx, vp, vl, zl [m][2|3], omega_l [m][4|9],
    intrinsics [n_cams][5] = (fx, fy, cx, cy, baseline), nP, nL, stereo and, when asked for, cam_edges = dict(vi, vj, meas
    [n][7], info [n][36]), scale_edges = dict(vi, vj, meas [n], info [n])."""
    from . import sbacam as SB
    from .g2o_io import _R_to_quat
    from .sim3 import FP64 as F
    if obs_per_point < 1 or obs_per_point > n_cams:
        raise ValueError("make_sbacam_ba: 1 <= obs_per_point <= n_cams")
    rng = CounterRng(seed + 1)
    d = 3 if stereo else 2
    ang = 2.0 * np.pi * np.arange(n_cams) / n_cams
    centre = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), 0.5 * np.sin(2.0 * ang)], axis=1)
    zc = -centre / np.linalg.norm(centre, axis=1, keepdims=True)       # the optical axis looks at the origin
    xc = np.cross(zc, [0.0, 0.0, 1.0])
    xc /= np.linalg.norm(xc, axis=1, keepdims=True)
    yc = np.cross(zc, xc)
    est_true = np.concatenate([centre, _R_to_quat(np.stack([xc, yc, zc], axis=2))], axis=1)   # camera-to-world: columns = the camera's axes
    step = np.concatenate([0.05 * np.stack([rng.normal(60 + c, n_cams) for c in range(3)], axis=1),
                           0.02 * np.stack([rng.normal(63 + c, n_cams) for c in range(3)], axis=1)], axis=1)
    hidx = (np.arange(n_cams, dtype=np.int32) - 1).astype(np.int32)
    nP = n_cams - 1
    est = SB.update(F, est_true, hidx, step[1:].reshape(-1))
    u = np.stack([rng.normal(40 + c, n_points) for c in range(3)], axis=1)
    u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-12)
    pts_true = u * (rng.uniform(43, n_points) ** (1.0 / 3.0))[:, None]
    pts = pts_true + 0.02 * np.stack([rng.normal(44 + c, n_points) for c in range(3)], axis=1)
    k = np.arange(n_cams)
    intr = np.stack([480.0 + 7.0 * k, 510.0 + 5.0 * k, 320.0 + 3.0 * k, 240.0 - 2.0 * k, 0.10 + 0.01 * k], axis=1)
    stride = max(1, n_cams // obs_per_point)
    start = np.minimum((rng.uniform(47, n_points) * n_cams).astype(np.int64), n_cams - 1)
    vp = ((start[:, None] + stride * np.arange(obs_per_point)[None, :]) % n_cams).reshape(-1).astype(np.int32)
    vl = np.repeat(np.arange(n_points, dtype=np.int32), obs_per_point)
    m = len(vp)
    zl = _sbacam_project(est_true, pts_true, vp, vl, intr, stereo)[0]
    zl = zl + pixel_noise * np.stack([rng.normal(48 + c, m) for c in range(d)], axis=1)
    for cams, X in ((est_true, pts_true), (est, pts)):
        depth = _sbacam_project(cams, X, vp, vl, intr, stereo)[1]
        if not ((depth >= 2.5) & (depth <= 5.5)).all():
            raise ValueError("make_sbacam_ba: an observed depth outside 2.5 ... 5.5 camera units (%g ... %g)" % (depth.min(), depth.max()))
    out = dict(est=est, est_true=est_true, points=pts, points_true=pts_true, hidx=hidx,
               pt_hidx=(nP + np.arange(n_points)).astype(np.int32), vp=vp, vl=vl, zl=zl,
               omega_l=np.tile(np.eye(d).reshape(1, d * d), (m, 1)), intrinsics=intr, nP=nP, nL=n_points, stereo=bool(stereo))
    if cam_edges is not None:
        k = int(cam_edges)
        pairs = [(i, i + 1) for i in range(n_cams - 1)]
        if k >= 2:
            pairs += [(i, (i + k) % n_cams) for i in range(0, n_cams, k) if (i + k) % n_cams != i]
        vi, vj = np.array([a for a, _ in pairs], np.int32), np.array([b for _, b in pairs], np.int32)
        ne = len(pairs)
        noise = np.concatenate([sigma_trans * np.stack([rng.normal(70 + c, ne) for c in range(3)], axis=1),
                                sigma_rot * np.stack([rng.normal(73 + c, ne) for c in range(3)], axis=1)], axis=1)
        meas = np.zeros((ne, 7))
        for e in range(ne):
            rel = SB.se3_mul(F, SB.se3_inverse(F, list(est_true[vi[e]])), list(est_true[vj[e]]))
            meas[e] = SB.oplus(F, rel, noise[e])
        info = np.diag([1.0 / sigma_trans ** 2] * 3 + [1.0 / sigma_rot ** 2] * 3).reshape(1, 36)
        out["cam_edges"] = dict(vi=vi, vj=vj, meas=meas, info=np.tile(info, (ne, 1)))
    if scale_edges is not None:
        ns = int(scale_edges)
        vi = (np.arange(ns, dtype=np.int32) * max(1, n_cams // max(1, 2 * ns))) % n_cams
        vj = ((vi + n_cams // 2) % n_cams).astype(np.int32)
        dist = np.linalg.norm(est_true[vj, 0:3] - est_true[vi, 0:3], axis=1)
        out["scale_edges"] = dict(vi=vi.astype(np.int32), vj=vj, meas=dist + sigma_scale * rng.normal(76, ns),
                                  info=np.full(ns, 1.0 / sigma_scale ** 2))
    return out


_GICP_PLANES = np.array([[1.0, 0.1, 0.2, 6.0], [0.1, 0.5, 1.0, 2.5], [-0.3, 0.2, 1.0, 3.0], [-1.0, 0.3, 0.4, 5.0], [0.2, 0.6, -1.0, 2.0]])


def make_gicp(n_scans, pts_per_pair, pairs=None, plane_to_plane=False, seed=0, odometry=True, noise_point=0.01, noise_normal=0.01,
              perturb=(0.15, 0.06), epsilon=0.01):
    """Scan registration with Edge_V_V_GICP between VertexSE3 (g2o/examples/icp/gicp_demo.cpp at more than two poses): n_scans
    scans on a short trajectory (0.4 units and a few hundredths of a radian from scan to scan) see points on five planes; every
    entry (a, b) of `pairs` (default: the consecutive scans) carries pts_per_pair correspondences: a world point on one of the
    planes, its position in scan a (pos0) and in scan b (pos1), each + noise_point * N(0, 1), and the plane's unit normal in
    either frame + noise_normal * N(0, 1), normalised.  Information = EdgeGICP::prec0(epsilon) of normal0 (what
    Edge_V_V_GICP::read builds with epsilon = .01); plane_to_plane: cov = (cov0(epsilon), cov1(epsilon)) as well.  The normals
    stay on the host.  Initial poses: the true ones multiplied from the right by a motion of perturb[0] * N(0, 1) in t and
    the rotation vector perturb[1] * N(0, 1); scan 0 is fixed at its true pose.  odometry: type-2 EdgeSE3 edges
    between consecutive scans (noise 0.05 / 0.02, information diag(400, ..., 2500, ...)); without them the arrays are empty and
    the registration is held by the correspondences alone.  Deterministic from seed.
    Returns kind = "se3", n, nP, poses [n][12], poses_true, hidx, vi, vj, Z, omega (odometry), gi, gj, gmeas [m][6], ginfo
    [m][9], gcov [m][18] or None, normal0, normal1 [m][3], plane_to_plane."""
    from . import gicp as G
    if n_scans < 2 or pts_per_pair < 1:
        raise ValueError("make_gicp: at least two scans and one correspondence per pair")
    pairs = [(s, s + 1) for s in range(n_scans - 1)] if pairs is None else [(int(a), int(b)) for a, b in pairs]
    if any(a == b or min(a, b) < 0 or max(a, b) >= n_scans for a, b in pairs):
        raise ValueError("make_gicp: a pair is two different scans")
    rng = CounterRng(seed + 1)
    s = np.arange(n_scans)
    t = np.stack([0.4 * s, 0.1 * np.sin(1.3 * s), 0.05 * np.cos(0.7 * s)], axis=1)
    R = _exp_so3(np.stack([0.03 * np.sin(0.9 * s), 0.02 * s, 0.05 * np.cos(1.1 * s) - 0.05], axis=1))[0]
    step = np.concatenate([perturb[0] * np.stack([rng.normal(10 + c, n_scans) for c in range(3)], axis=1),
                           perturb[1] * np.stack([rng.normal(13 + c, n_scans) for c in range(3)], axis=1)], axis=1)
    step[0] = 0.0
    Re, te = R @ _exp_so3(step[:, 3:])[0], np.einsum("nij,nj->ni", R, step[:, :3]) + t
    m = len(pairs) * pts_per_pair
    gi = np.repeat(np.array([a for a, _ in pairs], np.int32), pts_per_pair)
    gj = np.repeat(np.array([b for _, b in pairs], np.int32), pts_per_pair)
    nrm = _GICP_PLANES[:, :3] / np.linalg.norm(_GICP_PLANES[:, :3], axis=1, keepdims=True)
    pl = np.minimum((rng.uniform(20, m) * len(nrm)).astype(np.int64), len(nrm) - 1)
    n_w = nrm[pl]
    e1 = np.cross(n_w, [0.0, 1.0, 0.3])
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(n_w, e1)
    x_w = n_w * _GICP_PLANES[pl, 3:4] + e1 * (4.0 * rng.uniform(21, m) - 2.0)[:, None] + e2 * (4.0 * rng.uniform(22, m) - 2.0)[:, None]
    Rt = R.transpose(0, 2, 1)

    def seen(v, k0):
        p = np.einsum("nij,nj->ni", Rt[v], x_w - t[v]) + noise_point * np.stack([rng.normal(k0 + c, m) for c in range(3)], axis=1)
        nn = np.einsum("nij,nj->ni", Rt[v], n_w) + noise_normal * np.stack([rng.normal(k0 + 3 + c, m) for c in range(3)], axis=1)
        return p, nn / np.linalg.norm(nn, axis=1, keepdims=True)
    pos0, normal0 = seen(gi, 30)
    pos1, normal1 = seen(gj, 40)
    if max(np.abs(normal0[:, 1]).max(), np.abs(normal1[:, 1]).max()) > 0.95:
        raise ValueError("make_gicp: a normal along (0, 1, 0), where EdgeGICP::makeRot0 is ill-conditioned")
    ginfo = np.stack([G.prec(nv, epsilon).T.reshape(9) for nv in normal0])
    gcov = None
    if plane_to_plane:
        gcov = np.stack([np.concatenate([G.cov(a, epsilon).T.reshape(9), G.cov(b, epsilon).T.reshape(9)]) for a, b in zip(normal0, normal1)])
    if odometry:
        vi, vj = np.arange(n_scans - 1, dtype=np.int32), np.arange(1, n_scans, dtype=np.int32)
        ne = n_scans - 1
        zq = 0.02 * np.stack([rng.normal(53 + c, ne) for c in range(3)], axis=1)
        zq = np.concatenate([zq, np.sqrt(1.0 - (zq * zq).sum(axis=1))[:, None]], axis=1)
        Rm = Rt[vi] @ R[vj] @ _quat_to_rot(zq)
        tm = np.einsum("nij,nj->ni", Rt[vi], t[vj] - t[vi]) + 0.05 * np.stack([rng.normal(50 + c, ne) for c in range(3)], axis=1)
        Z = _iso_pack(Rm, tm)
        omega = np.tile(np.diag([400.0] * 3 + [2500.0] * 3).reshape(1, 36), (ne, 1))
    else:
        vi = vj = np.zeros(0, np.int32)
        Z, omega = np.zeros((0, 12)), np.zeros((0, 36))
    return dict(kind="se3", n=n_scans, nP=n_scans - 1, poses=_iso_pack(Re, te), poses_true=_iso_pack(R, t),
                hidx=(np.arange(n_scans, dtype=np.int32) - 1).astype(np.int32), vi=vi, vj=vj, Z=Z, omega=omega, gi=gi, gj=gj,
                gmeas=np.concatenate([pos0, pos1], axis=1), ginfo=ginfo, gcov=gcov, normal0=normal0, normal1=normal1,
                plane_to_plane=bool(plane_to_plane), pairs=pairs)


def _se2_mul(a, b):
    """SE2 products of rows (x, y, theta), the angle wrapped into [-pi, pi)."""
    c, s = np.cos(a[:, 2]), np.sin(a[:, 2])
    th = (a[:, 2] + b[:, 2] + np.pi) % (2.0 * np.pi) - np.pi
    return np.stack([a[:, 0] + c * b[:, 0] - s * b[:, 1], a[:, 1] + s * b[:, 0] + c * b[:, 1], th], axis=1)


def _se2_inv(a):
    c, s = np.cos(a[:, 2]), np.sin(a[:, 2])
    th = (-a[:, 2] + np.pi) % (2.0 * np.pi) - np.pi
    return np.stack([-(c * a[:, 0] + s * a[:, 1]), s * a[:, 0] - c * a[:, 1], th], axis=1)


def _iso_mul(A, B):
    (Ra, ta), (Rb, tb) = A, B
    return Ra @ Rb, np.einsum("nij,nj->ni", Ra, tb) + ta


def _iso_inv(A):
    Rt = A[0].transpose(0, 2, 1)
    return Rt, -np.einsum("nij,nj->ni", Rt, A[1])


def make_offset_rig(kind="se3", n_poses=12, n_sensors=2, edges_per_pose=3, seed=0, noise=(0.02, 0.01), perturb=(0.2, 0.08),
                    offsets=None):
    """A multi-sensor rig with EdgeSE2Offset / EdgeSE3Offset edges (what g2o_simulator3d's pose sensor with offset writes): n_poses
    poses on a winding trajectory with odometry between consecutive poses (type 1 / 2), n_sensors frames mounted on the body with
    distinct, non-trivial offsets (`offsets` [n_sensors][3 | 12] replaces the built-in ones), and n_poses * edges_per_pose offset
    edges.  Edge e of pose k runs from sensor (k + e) % n_sensors on pose k to sensor (k + 2 e + 1) % n_sensors on pose k + 1 + e
    (past the end: wrapped to the first poses), so the list holds edges with from != to parameter (and, with one sensor or where
    the two coincide, from == to) and edges from and to the fixed pose 0; the LAST edge is edge 0 reversed, pose 1 -> pose 0 with
    the parameters swapped: a vertex pair in both orders.  Measurement = (Xi Pi)^-1 (Xj Pj) of the true poses times a motion of
    noise[0] * N(0, 1) in t and noise[1] * N(0, 1) in the rotation (vector); information diag(1 / noise^2).  Initial poses: the true
    ones times a motion of perturb[0] / perturb[1]; pose 0 is fixed at its true pose.  Deterministic from seed.
    Returns kind, n, nP, poses, poses_true, hidx, vi, vj, Z, omega (odometry), offset_type (18 | 19), oi, oj, opf, opt, omeas,
    oinfo, offsets."""
    if kind not in ("se2", "se3") or n_poses < 3 or n_sensors < 1 or edges_per_pose < 1 or edges_per_pose > n_poses - 2:
        raise ValueError("make_offset_rig: kind se2 | se3, n_poses >= 3, n_sensors >= 1, 1 <= edges_per_pose <= n_poses - 2")
    se3 = kind == "se3"
    rng = CounterRng(seed + 1)
    n, d, ms = n_poses, (6 if se3 else 3), (12 if se3 else 3)
    s = np.arange(n, dtype=np.float64)
    k = np.repeat(np.arange(n), edges_per_pose)
    e = np.tile(np.arange(edges_per_pose), n)
    oi, oj = k.astype(np.int32), ((k + 1 + e) % n).astype(np.int32)
    opf, opt = ((k + e) % n_sensors).astype(np.int32), ((k + 2 * e + 1) % n_sensors).astype(np.int32)
    oi[-1], oj[-1], opf[-1], opt[-1] = oj[0], oi[0], opt[0], opf[0]
    vi, vj = np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    m = len(oi)
    q = np.arange(n_sensors, dtype=np.float64)

    def motion(stream, count, scale):
        return np.concatenate([scale[0] * np.stack([rng.normal(stream + c, count) for c in range(3 if se3 else 2)], axis=1),
                               scale[1] * np.stack([rng.normal(stream + 3 + c, count) for c in range(3 if se3 else 1)], axis=1)], axis=1)

    if se3:
        X = (_exp_so3(np.stack([0.3 * np.sin(0.9 * s), 0.25 * np.sin(0.37 * s), 0.6 * np.sin(0.21 * s)], axis=1))[0],
             np.stack([0.5 * s, np.sin(0.3 * s), 0.2 * np.cos(0.2 * s)], axis=1))
        if offsets is None:
            P = (_exp_so3(np.stack([0.4 + 0.5 * q, -0.3 + 0.35 * q, 0.9 - 0.7 * q], axis=1))[0],
                 np.stack([0.3 + 0.1 * q, -0.2 + 0.15 * q, 0.1 + 0.05 * q * q], axis=1))
        else:
            T = np.asarray(offsets, np.float64).reshape(n_sensors, 12)
            P = (T[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1), T[:, 9:])
        take = lambda A, idx: (A[0][idx], A[1][idx])
        expm = lambda v: (_exp_so3(v[:, 3:])[0], v[:, :3])
        Z0 = _iso_mul(_iso_mul(_iso_inv(take(X, vi)), take(X, vj)), expm(motion(10, n - 1, noise)))
        Zo = _iso_mul(_iso_mul(_iso_inv(_iso_mul(take(X, oi), take(P, opf))), _iso_mul(take(X, oj), take(P, opt))), expm(motion(20, m, noise)))
        step = motion(30, n, perturb)
        step[0] = 0.0
        Xe = _iso_mul(X, expm(step))
        pack = lambda A: _iso_pack(A[0], A[1])
    else:
        X = np.stack([0.5 * s, np.sin(0.3 * s), 0.4 * np.sin(0.21 * s) + 0.05 * s], axis=1)
        X[:, 2] = (X[:, 2] + np.pi) % (2.0 * np.pi) - np.pi
        P = np.stack([0.3 + 0.1 * q, -0.2 + 0.15 * q, 0.7 - 1.1 * q], axis=1) if offsets is None else np.asarray(offsets, np.float64).reshape(n_sensors, 3)
        Z0 = _se2_mul(_se2_mul(_se2_inv(X[vi]), X[vj]), motion(10, n - 1, noise))
        Zo = _se2_mul(_se2_mul(_se2_inv(_se2_mul(X[oi], P[opf])), _se2_mul(X[oj], P[opt])), motion(20, m, noise))
        step = motion(30, n, perturb)
        step[0] = 0.0
        Xe = _se2_mul(X, step)
        pack = lambda A: A
    nt = 3 if se3 else 2
    w = np.diag([1.0 / noise[0] ** 2] * nt + [1.0 / noise[1] ** 2] * (d - nt))
    return dict(kind=kind, n=n, nP=n - 1, poses=pack(Xe), poses_true=pack(X), hidx=(np.arange(n, dtype=np.int32) - 1).astype(np.int32),
                vi=vi, vj=vj, Z=pack(Z0), omega=np.tile(w.reshape(1, d * d), (n - 1, 1)), offset_type=19 if se3 else 18, oi=oi, oj=oj,
                opf=opf, opt=opt, omeas=pack(Zo), oinfo=np.tile(w.reshape(1, d * d), (m, 1)), offsets=pack(P).reshape(n_sensors, ms).copy())


def make_bearing_slam(n_poses, n_landmarks, with_xy=False, seed=42, noise=0.02, perturb=(0.1, 0.02, 0.2), min_parallax=0.2,
                      min_distance=0.5, **landmark_args):
    """2-D landmark SLAM with bearing-only observations (EdgeSE2PointXYBearing, what g2o_simulator2d's bearing sensor writes), built
    on make_landmark_slam("se2", n_poses, n_landmarks, seed=seed, perturb=perturb, **landmark_args): the same trajectory, odometry,
    landmarks and observing pairs.  Every Cartesian observation (vp, vl) becomes a bearing (bp, bl, zb): the angle of the landmark
    in the frame of the true pose plus noise * N(0, 1), wrapped into [-pi, pi); omega_b = 1 / noise^2.  No bearing is taken from
    closer than min_distance, at the ground truth or at the initial estimates (the Jacobian grows like 1 / distance and the
    reference has no guard at distance 0).
    with_xy=True: the bearings stand beside the Cartesian observations (vp, vl, zl, omega_l unchanged: a point sensor and a
    bearing sensor).  with_xy=False: bearing-only SLAM, the Cartesian keys are dropped (vp, vl of length 0, zl [0][2], omega_l
    [0][4], M = 0); a bearing fixes a landmark only along one line, so every free landmark keeps at least two bearings whose
    world-frame directions -- as lines, modulo pi -- differ by at least min_parallax, at the ground truth and at the initial
    estimates; landmarks that cannot meet this are dropped together with their observations (otherwise their 2x2 block is
    singular and the Schur complement has nothing to invert) and the landmark table is renumbered.
    Returns the dict of make_landmark_slam plus bp, bl, zb [m], omega_b [m], B = m."""
    g = make_landmark_slam("se2", n_poses, n_landmarks, seed=seed, perturb=perturb, **landmark_args)
    rng = CounterRng(seed)
    vp, vl = g["vp"], g["vl"]

    def geometry(poses, points):
        d = points[vl] - poses[vp, :2]
        return np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0])
    (r_t, w_t), (r_e, w_e) = geometry(g["poses_true"], g["points_true"]), geometry(g["poses"], g["points"])
    keep = (r_t >= min_distance) & (r_e >= min_distance)
    L = g["L"]
    lm_keep = np.ones(L, bool)
    if not with_xy:
        # the kept observations of every landmark side by side (padded with NaN), then all pairs of a row at once
        idx = np.nonzero(keep)[0]
        idx = idx[np.argsort(vl[idx], kind="stable")]
        count = np.bincount(vl[idx], minlength=L)
        slot = np.arange(len(idx)) - np.repeat(np.cumsum(count) - count, count)
        for w in (w_t, w_e):
            a = np.full((L, max(int(count.max()), 1)), np.nan)
            a[vl[idx], slot] = w[idx] % np.pi
            diff = np.abs(a[:, :, None] - a[:, None, :])
            with np.errstate(invalid="ignore"):
                spread = np.nan_to_num(np.fmax.reduce(np.fmax.reduce(np.minimum(diff, np.pi - diff), axis=2), axis=1), nan=-1.0)
            lm_keep &= (spread >= min_parallax) | (g["pt_hidx"] < 0)
        keep &= lm_keep[vl]
    bp, bl = vp[keep].astype(np.int32), vl[keep].astype(np.int32)
    c, s = np.cos(g["poses_true"][bp, 2]), np.sin(g["poses_true"][bp, 2])
    d = g["points_true"][bl] - g["poses_true"][bp, :2]
    m = len(bp)
    zb = _wrap(np.arctan2(-s * d[:, 0] + c * d[:, 1], c * d[:, 0] + s * d[:, 1]) + noise * rng.normal(270, len(vp))[keep])
    out = dict(g)
    if not with_xy:
        new = np.cumsum(lm_keep) - 1
        bl = new[bl].astype(np.int32)
        free = lm_keep & (g["pt_hidx"] >= 0)
        pt_hidx = np.where(free, g["nP"] + np.cumsum(free) - 1, -1)[lm_keep].astype(np.int32)
        out.update(L=int(lm_keep.sum()), nL=int(free.sum()), points=g["points"][lm_keep], points_true=g["points_true"][lm_keep],
                   pt_hidx=pt_hidx, vp=np.zeros(0, np.int32), vl=np.zeros(0, np.int32), zl=np.zeros((0, 2)), omega_l=np.zeros((0, 4)), M=0)
    out.update(bp=bp, bl=bl, zb=zb, omega_b=np.full(m, 1.0 / noise ** 2), B=m)
    return out


def make_pointxy_calib_slam(n_poses, n_landmarks, offset=(0.3, 0.1, 0.2), fix_offset=False, with_xy=False, seed=42, noise=0.05,
                            **landmark_args):
    """2-D landmark SLAM whose point sensor is mounted off the robot's centre by an unknown offset that is estimated with the map
    (EdgeSE2PointXYCalib), built on make_landmark_slam("se2", n_poses, n_landmarks, seed=seed, **landmark_args): the same
    trajectory -- laps round a loop, so it keeps turning and the offset is observable --, odometry, landmarks and observing pairs.
    The calibration vertex c is ONE extra row of the pose table, behind the poses (row n_poses; calib_row); its true value is
    `offset`, its initial estimate the identity (fix_offset=True: it is fixed at the truth, hessian index -1).  Every Cartesian
    observation (vp, vl) becomes a three-vertex edge (qp, ql, qc): zq = (x_true c_true)^-1 l_true + noise * N(0, 1), omega_q =
    I / noise^2.  with_xy=True keeps the plain observations beside them (a second, centred point sensor); with_xy=False drops
    them (vp, vl of length 0, zl [0][2], omega_l [0][4], M = 0).
    Returns the dict of make_landmark_slam (n, nP, hidx, poses, poses_true one row longer, pt_hidx moved behind the new free
    vertex) plus qp, ql, qc, zq [m][2], omega_q [m][4], Q = m, calib_row, offset_true."""
    g = make_landmark_slam("se2", n_poses, n_landmarks, seed=seed, **landmark_args)
    rng = CounterRng(seed)
    n = g["n"]
    off = np.asarray(offset, np.float64)
    free = 0 if fix_offset else 1
    out = dict(g)
    out.update(n=n + 1, nP=g["nP"] + free, poses=np.vstack([g["poses"], off if fix_offset else np.zeros(3)]),
               poses_true=np.vstack([g["poses_true"], off]), hidx=np.append(g["hidx"], -1 if fix_offset else g["nP"]).astype(np.int32),
               pt_hidx=np.where(g["pt_hidx"] >= 0, g["pt_hidx"] + free, -1).astype(np.int32))
    qp, ql = g["vp"].astype(np.int32), g["vl"].astype(np.int32)
    m = len(qp)
    X, Lm = g["poses_true"][qp], g["points_true"][ql]                     # (x_true c_true)^-1 l_true, all edges at once
    c1, s1 = np.cos(X[:, 2]), np.sin(X[:, 2])
    dx, dy = Lm[:, 0] - (X[:, 0] + c1 * off[0] - s1 * off[1]), Lm[:, 1] - (X[:, 1] + s1 * off[0] + c1 * off[1])
    cq, sq = np.cos(X[:, 2] + off[2]), np.sin(X[:, 2] + off[2])
    zq = np.stack([cq * dx + sq * dy, -sq * dx + cq * dy], axis=1)
    zq = zq + noise * np.stack([rng.normal(280, m), rng.normal(281, m)], axis=1)
    if not with_xy:
        out.update(vp=np.zeros(0, np.int32), vl=np.zeros(0, np.int32), zl=np.zeros((0, 2)), omega_l=np.zeros((0, 4)), M=0)
    out.update(qp=qp, ql=ql, qc=np.full(m, n, np.int32), zq=zq, omega_q=np.tile((np.eye(2) / noise ** 2).reshape(1, 4), (m, 1)), Q=m,
               calib_row=n, offset_true=off)
    return out


def make_calib_rig(n_poses=40, loops=21, seed=0, noise=(0.02, 0.01), perturb=(0.1, 0.03), offset=(0.3, 0.1, 0.2), fix_offset=False,
                   wrap_every=0, pairs=None, odom_calib=False, n_params=1, params=(1.06, 0.93, 1.25)):
    """Simultaneous calibration, localisation and mapping in 2-D (what g2o/examples/calibration_odom_laser optimises): n_poses
    robot poses on a trajectory that keeps turning (so that the laser's mounting offset is observable), EdgeSE2 odometry between
    consecutive poses, and three-vertex EdgeSE2SensorCalib scan-match edges (x1, x2, L) between consecutive poses and at `loops`
    loop closures.  The laser offset L is an ordinary VertexSE2: row n_poses of the ONE pose table [n_poses + 1][3], so every
    calibration edge names the same row `offset_row` as its third vertex.  pairs [m][2]: the pose pairs of the calibration
    edges instead of the built-in consecutive + loop-closure ones.
    Odometry = X_k^-1 X_{k+1}, scan match = (X_i L)^-1 (X_j L) of the true values, each times a motion of noise[0] * N(0, 1) in t and
    noise[1] * N(0, 1) in theta; information diag(1 / noise^2).  Initial poses: the true ones times a motion of perturb[0] /
    perturb[1]; pose 0 is fixed at its true pose.  The true offset is `offset`, its initial guess the identity; fix_offset=True
    holds L fixed at the truth (hessian index -1: plain scan-match SLAM through the same edges).  wrap_every = w > 0: every w-th
    calibration edge measures an angle off by pi -/+ 1e-3 (alternating), so that its angle error lands just inside +pi or just
    inside -pi: gross outliers on both sides of the wrap (for a robust kernel).  Deterministic from seed.
    odom_calib=True adds the other half of that example's graph: n_params rows of VertexOdomDifferentialParams (k_l, k_r, b)
    behind the offset row (ADDITIVE rows: estimate += step, no angle wrap) and one three-vertex EdgeSE2OdomDifferentialCalib per
    consecutive pose pair (edge k names parameter row k % n_params: n_params robots taking turns).  The trajectory is then built
    from arcs of length 0.5 held for dt = 0.8 + 0.1 (k % 5), every fifth one STRAIGHT, so that the true motions are exactly what
    OdomConvert::convertToMotion produces; the wheel velocities are those of the noisy motion (translation noise alone on the
    straight segments) by OdomConvert::convertToVelocity (wheel base 1), rescaled to a robot of the true parameters `params`
    (+ 0.04 r (1, -1, 2) for robot r), as sclam_helpers.cpp:93-94 generates them.  Initial estimate (1, 1, 1), as setToOriginImpl.
    The default arguments produce the arrays they always did.
    Returns kind ("se2"), n (rows of the pose table), n_poses, offset_row, nP, poses, poses_true, hidx, vi, vj, Z, omega
    (odometry), ci, cj, cl, cmeas, cinfo (calibration edges), offset_true; with odom_calib also oi, oj, op, omeas, oinfo
    (odometry-calibration edges), param_rows, params_true."""
    if n_poses < 3 or loops < 0:
        raise ValueError("make_calib_rig: n_poses >= 3, loops >= 0")
    rng = CounterRng(seed + 1)
    n = n_poses
    s = np.arange(n, dtype=np.float64)
    th = 0.35 * s + 0.3 * np.sin(0.5 * s)
    step = 0.5 * np.stack([np.cos(th), np.sin(th)], axis=1)
    X = np.concatenate([np.concatenate([np.zeros((1, 2)), np.cumsum(step[:-1], axis=0)]), th[:, None]], axis=1)
    if odom_calib:
        if n_params < 1:
            raise ValueError("make_calib_rig: n_params >= 1")
        from . import odom_calib as OC
        dth = np.diff(th)
        dth[np.arange(n - 1) % 5 == 4] = 0.0
        dts = 0.8 + 0.1 * (np.arange(n - 1) % 5)
        vtrue = np.stack([[(0.5 - 0.5 * a) / t, (0.5 + 0.5 * a) / t, t] for a, t in zip(dth, dts)])   # S dt / 2 = 0.5, D dt = dth
        M = np.stack([OC.convert_to_motion(OC.FP64, v, 1.0) for v in vtrue])
        X = np.zeros((n, 3))
        X[0, 2] = th[0]
        for k in range(n - 1):
            X[k + 1] = _se2_mul(X[k:k + 1], M[k:k + 1])[0]
    X[:, 2] = (X[:, 2] + np.pi) % (2.0 * np.pi) - np.pi
    Lt = np.asarray(offset, np.float64).reshape(1, 3)
    vi, vj = np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    if pairs is None:
        e = np.arange(loops)
        li = (5 * e) % (n - 2)
        lj = li + 2 + (3 * e) % (n - li - 2)
        ci, cj = np.concatenate([vi, li]).astype(np.int32), np.concatenate([vj, lj]).astype(np.int32)
    else:
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        ci, cj = pairs[:, 0].copy(), pairs[:, 1].copy()
    m = len(ci)

    def motion(stream, count, scale):
        return np.stack([scale[0] * rng.normal(stream, count), scale[0] * rng.normal(stream + 1, count), scale[1] * rng.normal(stream + 3, count)], axis=1)

    Z0 = _se2_mul(_se2_mul(_se2_inv(X[vi]), X[vj]), motion(10, n - 1, noise))
    Lm = np.repeat(Lt, m, axis=0)
    Zc = _se2_mul(_se2_mul(_se2_inv(_se2_mul(X[ci], Lm)), _se2_mul(X[cj], Lm)), motion(20, m, noise))
    if wrap_every > 0:
        k = np.arange(0, m, wrap_every)
        Zc[k, 2] += np.pi + np.where((k // wrap_every) % 2 == 0, -1e-3, 1e-3)
        Zc[:, 2] = (Zc[:, 2] + np.pi) % (2.0 * np.pi) - np.pi
    dX = motion(30, n, perturb)
    dX[0] = 0.0
    Xe = _se2_mul(X, dX)
    poses = np.concatenate([Xe, Lt if fix_offset else np.zeros((1, 3))])
    hidx = np.concatenate([np.arange(n, dtype=np.int32) - 1, [-1 if fix_offset else n - 1]]).astype(np.int32)
    w = np.diag([1.0 / noise[0] ** 2] * 2 + [1.0 / noise[1] ** 2])
    if odom_calib:
        nz = motion(40, n - 1, noise)
        straight = dth == 0.0
        nz[straight, 1:] = 0.0
        Mn = _se2_mul(M, nz)
        ptrue = np.stack([np.asarray(params, np.float64) + 0.04 * r * np.array([1.0, -1.0, 2.0]) for r in range(n_params)])
        op = (n + 1 + np.arange(n - 1) % n_params).astype(np.int32)
        omeas = np.zeros((n - 1, 3))
        for k in range(n - 1):
            v1 = OC.convert_to_velocity(OC.FP64, Mn[k], dts[k])
            kl, kr, b = ptrue[k % n_params]
            S1, D1 = v1[0] + v1[1], v1[1] - v1[0]
            omeas[k] = [0.5 * (S1 - b * D1) / kl, 0.5 * (S1 + b * D1) / kr, dts[k]]
        free = n - 1 + (0 if fix_offset else 1)
        return dict(kind="se2", n=n + 1 + n_params, n_poses=n, offset_row=n, nP=free + n_params,
                    poses=np.concatenate([poses, np.ones((n_params, 3))]), poses_true=np.concatenate([X, Lt, ptrue]),
                    hidx=np.concatenate([hidx, free + np.arange(n_params)]).astype(np.int32), vi=vi, vj=vj, Z=Z0,
                    omega=np.tile(w.reshape(1, 9), (n - 1, 1)), ci=ci, cj=cj, cl=np.full(m, n, np.int32), cmeas=Zc,
                    cinfo=np.tile(w.reshape(1, 9), (m, 1)), offset_true=Lt[0].copy(), oi=vi.copy(), oj=vj.copy(), op=op, omeas=omeas,
                    oinfo=np.tile(w.reshape(1, 9), (n - 1, 1)), param_rows=np.arange(n + 1, n + 1 + n_params, dtype=np.int32),
                    params_true=ptrue)
    return dict(kind="se2", n=n + 1, n_poses=n, offset_row=n, nP=n - 1 + (0 if fix_offset else 1), poses=poses,
                poses_true=np.concatenate([X, Lt]), hidx=hidx, vi=vi, vj=vj, Z=Z0, omega=np.tile(w.reshape(1, 9), (n - 1, 1)), ci=ci, cj=cj,
                cl=np.full(m, n, np.int32), cmeas=Zc, cinfo=np.tile(w.reshape(1, 9), (m, 1)), offset_true=Lt[0].copy())


SCAM_KCAM = (500.0, 500.0, 320.0, 240.0, 0.075)   # sba_demo.cpp:189-191: focal length, principal point (640 x 480 image), baseline


def make_scam_ba(n_cams, n_points, fixed=2, gicp=False, outlier_frac=0.0, seed=0, pixel_noise=1.0, point_noise=1.0, spacing=0.04,
                 perturb=(0.0, 0.0), fixed_points=0, gicp_pts_per_pair=20, gicp_noise=(0.01, 0.01), epsilon=0.01):
    """Stereo bundle adjustment with Edge_XYZ_VSC between VertexSCam cameras and VertexSBAPointXYZ points, after
    g2o/examples/sba/sba_demo.cpp:179-341 at any size: n_cams cameras on a line (camera i at (i * spacing - 1, 0, 0), identity
    rotation, looking down +z; the first `fixed` of them are fixed -- the gauge, there is no pose-pose edge), n_points candidate
    points 10 to 11 units ahead (x over the cameras' span widened by 0.5 to the left and 2.5 to the right, y in [-0.5, 0.5]), ONE
    kcam = SCAM_KCAM = (fx, fy, cx, cy, baseline) = (500, 500, 320, 240, 0.075) for all cameras.  A camera observes a point when
    the left projection lies inside the 640 x 480 image (0 <= u < 640, 0 <= v < 480); points seen by fewer than two cameras are
    dropped and the table is renumbered.  Measurements (u_left, v_left, u_right) = VertexSCam::mapPoint of the true point +
    pixel_noise * N(0, 1) on the first two rows and pixel_noise / 16 * N(0, 1) on the third; a fraction outlier_frac of them is
    first replaced by (U(64, 640), U(0, 480), u - U(0, 64)) as the demo does.  Information: the identity.  Initial estimates: the
    points at the truth + point_noise * N(0, 1) per coordinate, the free cameras at the truth multiplied from the right by a motion
    of perturb[0] * N(0, 1) in t and the rotation vector perturb[1] * N(0, 1) (the demo: none).  The first fixed_points points
    are fixed.  Edges are point-major, cameras ascending within a point.
    gicp=True (the graph of g2o/examples/icp/gicp_sba_demo.cpp): gicp_pts_per_pair Edge_V_V_GICP correspondences between every two
    consecutive cameras, as make_gicp makes them (points on its planes seen from both cameras with gicp_noise = (point, normal)
    sigma, point-to-plane information EdgeGICP::prec0(epsilon)); the dict then also carries gi, gj, gmeas, ginfo, gcov = None,
    normal0, normal1 -- the keys lm.setup_device_gicp reads.
    Returns kind = "se3", observation = "stereo_vsc", kcam [5], n, nP, L, nL, M, E = 0, poses [n][12], poses_true, hidx, points
    [L][3], points_true, pt_hidx, vp, vl, zl [M][3], omega_l [M][9], outlier [M] (bool) and an EMPTY EdgeSE3 set vi, vj, Z [0][12],
    omega [0][36].  Deterministic from seed (counter-based RNG)."""
    n, L0, fixed = int(n_cams), int(n_points), int(fixed)
    if n < 2 or L0 < 1 or not 1 <= fixed < n:
        raise ValueError("make_scam_ba: at least two cameras, one point and 1 <= fixed < n_cams")
    rng = CounterRng(seed + 7)
    fx, fy, cx, cy, b = SCAM_KCAM
    tx = np.arange(n) * float(spacing) - 1.0
    span = tx[-1] - tx[0]
    P = np.stack([tx[0] - 0.5 + rng.uniform(1, L0) * (span + 3.0), rng.uniform(2, L0) - 0.5, rng.uniform(3, L0) + 10.0], axis=1)
    # the cameras that see a point form a range of the line: candidates from the pinhole bounds, one camera wider on either side,
    # then the projection itself decides
    lo = np.floor((P[:, 0] - (640.0 - cx) * P[:, 2] / fx - tx[0]) / spacing).astype(np.int64) - 1
    hi = np.ceil((P[:, 0] + cx * P[:, 2] / fx - tx[0]) / spacing).astype(np.int64) + 1
    lo, hi = np.clip(lo, 0, n), np.clip(hi + 1, 0, n)
    cnt = np.maximum(hi - lo, 0)
    pl = np.repeat(np.arange(L0), cnt)
    pc = (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)).astype(np.int64)

    def project(X, cams):
        q0, q1, q2 = X[:, 0] - tx[cams], X[:, 1], X[:, 2]
        return np.stack([fx * q0 / q2 + cx, fy * q1 / q2 + cy, fx * (q0 - b) / q2 + cx], axis=1)
    z = project(P[pl], pc)
    inside = (z[:, 0] >= 0) & (z[:, 1] >= 0) & (z[:, 0] < 640) & (z[:, 1] < 480)
    pl, pc, z = pl[inside], pc[inside], z[inside]
    keep = np.bincount(pl, minlength=L0) >= 2
    sel = keep[pl]
    pl, pc, z = pl[sel], pc[sel], z[sel]
    L = int(keep.sum())
    if L <= int(fixed_points):
        raise ValueError("make_scam_ba: fewer points seen by two cameras than fixed_points + 1")
    renum = np.cumsum(keep) - 1
    vl, vp = renum[pl].astype(np.int32), pc.astype(np.int32)
    pts_true = P[keep]
    M = len(vp)
    outlier = rng.uniform(4, M) < outlier_frac
    zo = np.stack([64.0 + 576.0 * rng.uniform(5, M), 480.0 * rng.uniform(6, M), 64.0 * rng.uniform(7, M)], axis=1)
    zo[:, 2] = zo[:, 0] - zo[:, 2]
    z = np.where(outlier[:, None], zo, z)
    z = z + pixel_noise * np.stack([rng.normal(8, M), rng.normal(9, M), rng.normal(10, M) / 16.0], axis=1)
    pts = pts_true + point_noise * np.stack([rng.normal(11 + c, L) for c in range(3)], axis=1)
    t = np.stack([tx, np.zeros(n), np.zeros(n)], axis=1)
    R = np.tile(np.eye(3)[None], (n, 1, 1))
    step = np.concatenate([perturb[0] * np.stack([rng.normal(14 + c, n) for c in range(3)], axis=1),
                           perturb[1] * np.stack([rng.normal(17 + c, n) for c in range(3)], axis=1)], axis=1)
    step[:fixed] = 0.0
    Re, te = R @ _exp_so3(step[:, 3:])[0], np.einsum("nij,nj->ni", R, step[:, :3]) + t
    hidx = np.where(np.arange(n) < fixed, -1, np.arange(n) - fixed).astype(np.int32)
    nL = L - int(fixed_points)
    pt_hidx = np.where(np.arange(L) < int(fixed_points), -1, n - fixed + np.arange(L) - int(fixed_points)).astype(np.int32)
    out = dict(kind="se3", observation="stereo_vsc", kcam=np.array(SCAM_KCAM), n=n, nP=n - fixed, L=L, nL=nL, M=M, E=0,
               poses=_iso_pack(Re, te), poses_true=_iso_pack(R, t), hidx=hidx, points=pts, points_true=pts_true, pt_hidx=pt_hidx,
               vp=vp, vl=vl, zl=z, omega_l=np.tile(np.eye(3).reshape(1, 9), (M, 1)), outlier=outlier, vi=np.zeros(0, np.int32),
               vj=np.zeros(0, np.int32), Z=np.zeros((0, 12)), omega=np.zeros((0, 36)))
    if gicp:
        from . import gicp as G
        m = (n - 1) * int(gicp_pts_per_pair)
        gi = np.repeat(np.arange(n - 1, dtype=np.int32), int(gicp_pts_per_pair))
        gj = gi + 1
        nrm = _GICP_PLANES[:, :3] / np.linalg.norm(_GICP_PLANES[:, :3], axis=1, keepdims=True)
        pln = np.minimum((rng.uniform(20, m) * len(nrm)).astype(np.int64), len(nrm) - 1)
        n_w = nrm[pln]
        e1 = np.cross(n_w, [0.0, 1.0, 0.3])
        e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
        e2 = np.cross(n_w, e1)
        x_w = n_w * _GICP_PLANES[pln, 3:4] + e1 * (4.0 * rng.uniform(21, m) - 2.0)[:, None] + e2 * (4.0 * rng.uniform(22, m) - 2.0)[:, None]

        def seen(v, k0):   # (identity rotations)
            p = x_w - t[v] + gicp_noise[0] * np.stack([rng.normal(k0 + c, m) for c in range(3)], axis=1)
            nn = n_w + gicp_noise[1] * np.stack([rng.normal(k0 + 3 + c, m) for c in range(3)], axis=1)
            return p, nn / np.linalg.norm(nn, axis=1, keepdims=True)
        pos0, normal0 = seen(gi, 30)
        pos1, normal1 = seen(gj, 40)
        out.update(gi=gi, gj=gj.astype(np.int32), gmeas=np.concatenate([pos0, pos1], axis=1),
                   ginfo=np.stack([G.prec(nv, epsilon).T.reshape(9) for nv in normal0]), gcov=None, normal0=normal0, normal1=normal1,
                   plane_to_plane=False)
    return out
