"""Test side of the SBA-format front end (pose type 12 = VertexCam, landmark types 13 / 14 = EdgeProjectP2MC / EdgeProjectP2SC,
g2ohip_pg_set_cam_project_edges): the formulas of openslam_g2o_amd/sbacam.py (ONE body, operation for operation, generic over
the arithmetic) evaluated in fp64 (FP64) and with mpmath at 60 digits (MP), the graphs of the tests and a host-fed graph for
lm.optimize."""
import numpy as np

from openslam_g2o_amd.sbacam import (FP64, camera_point, moved_points, oplus, project_edges, project_error,  # noqa: F401
                                     project_jacobians, to_f64, transform, update)
from tests.sim3_helpers import MP, mp  # noqa: F401

EDGE_COUNTS = (1, 65, 256, 257, 300)        # one lane per edge, 256 threads per block (tests/test_gpu_sbacam.py)
BA_ARGS = dict(n_cams=12, n_points=60, obs_per_point=4, seed=7)
HUBER = 3.0
ITERATIONS = 5
RUNS = [("mono", False, 0.0), ("mono_huber", False, HUBER), ("stereo", True, 0.0), ("stereo_huber", True, HUBER)]


def graph_name(n, stereo):
    return "%s%d" % ("s" if stereo else "m", n)


def random_graph(n_edges, seed, stereo):
    """n_edges observations over few cameras and few points (every vertex shared by many edges).  Cameras: camera-to-world,
    rotations of ~0.3 rad about random axes, centres 3.5 ... 5.5 units behind the points of a unit ball, so every pz is 2 ... 7
    (asserted: order 1 or more); intrinsics and baselines that differ from camera to camera (a wrong table index is an error of
    whole pixels); measurements = projection + N(0, 2) pixels, information matrices that differ per edge.  With more than one
    edge: camera 0 and point 0 are fixed, edge 0 = (fixed camera, free point), edge 1 = (free camera, fixed point), edges 2 and
    3 observe the same (camera, point) pair.  One edge: one free camera, one free point."""
    rng = np.random.default_rng(seed)
    d = 3 if stereo else 2
    nv = 1 if n_edges == 1 else min(5, n_edges)
    npt = 1 if n_edges == 1 else min(6, n_edges)
    cams = np.zeros((nv, 7))
    for v in range(nv):
        w = rng.normal(size=3) * 0.15
        q = np.concatenate([w, [np.sqrt(1.0 - w @ w)]])
        cams[v] = np.concatenate([rng.normal(size=2) * 0.5, [-rng.uniform(3.5, 5.5)], q / np.linalg.norm(q)])
    u = rng.normal(size=(npt, 3))
    points = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.2, 1.0, npt)[:, None]
    k = np.arange(nv)
    intr = np.stack([450.0 + 23.0 * k, 520.0 - 17.0 * k, 300.0 + 11.0 * k, 250.0 - 13.0 * k, 0.08 + 0.015 * k], axis=1)
    vp = rng.integers(0, nv, n_edges).astype(np.int32)
    vl = rng.integers(0, npt, n_edges).astype(np.int32)
    if n_edges > 1:
        vp[:4], vl[:4] = (0, 1, 2, 2), (1, 0, 2, 2)
        hidx = np.arange(nv, dtype=np.int32) - 1
        pt_hidx = np.where(np.arange(npt) == 0, -1, nv - 1 + np.arange(npt) - 1).astype(np.int32)
    else:
        vp[0] = vl[0] = 0
        hidx, pt_hidx = np.zeros(1, np.int32), np.ones(1, np.int32)
    proj = project_edges(FP64, cams, points, vp, vl, np.zeros((n_edges, d)), intr, stereo, jac=False)
    meas = np.round((proj + 2.0 * rng.normal(size=(n_edges, d))) * 8.0) / 8.0      # (eighths of a pixel: the file stays small)
    depth = np.array([camera_point(FP64, cams[vp[e]], points[vl[e]])[2] for e in range(n_edges)])
    assert depth.min() > 1.5, depth.min()
    A = rng.integers(-2, 3, size=(n_edges, d, d)).astype(np.float64)               # (small integers, for the same reason)
    info = (A @ A.transpose(0, 2, 1) + 2 * np.eye(d)).reshape(n_edges, d * d)
    nP = int(hidx.max()) + 1
    return dict(est=cams, points=points, hidx=hidx, pt_hidx=pt_hidx, vp=vp, vl=vl, zl=meas, omega_l=info, intrinsics=intr,
                nP=nP, nL=int((pt_hidx >= 0).sum()), stereo=bool(stereo))


def producers(F, g, jac=True, cams=None, points=None):
    return project_edges(F, g["est"] if cams is None else cams, g["points"] if points is None else points, g["vp"], g["vl"],
                         g["zl"], g["intrinsics"], g["zl"].shape[1] == 3, jac)


def update_step(g, seed):
    """A step x over the whole system of g (6 per free camera, 3 per free point) of a size that moves every estimate visibly;
    |x[3:6]| is a few hundredths: well below 1."""
    rng = np.random.default_rng(seed)
    xp = rng.normal(size=(g["nP"], 6)) * np.array([0.1] * 3 + [0.03] * 3)
    xl = rng.normal(size=(g["nL"], 3)) * 0.1
    assert np.linalg.norm(xp[:, 3:], axis=1).max() < 0.2
    return np.concatenate([xp.ravel(), xl.ravel()])


def transform_gap(a, b):
    """max abs over (R, t) between two camera tables."""
    d = 0.0
    for ca, cb in zip(a, b):
        (Ra, ta), (Rb, tb) = transform(ca), transform(cb)
        d = max(d, np.abs(Ra - Rb).max(), np.abs(ta - tb).max())
    return float(d)


# ------------------------------------------------------------------------------------------------ host-fed graph for lm.optimize
class HostSbacamBAGraph:
    """The graph protocol of openslam_g2o_amd.lm with cameras and points on the host and the producers of sbacam.py in
    arithmetic F: feed(J0, J1, err) hands every evaluation of the observation set to a solver, get_x() reads its solution."""

    def __init__(self, F, g, feed, get_x, chi2_fn):
        self.F, self.g, self.feed, self.get_x, self.chi2_fn = F, g, feed, get_x, chi2_fn
        self.est = np.array(g["est"], np.float64).copy()
        self.points = np.array(g["points"], np.float64).copy()
        self.stack = []
        self.J = None

    def linearize(self):
        J0, J1, err = producers(self.F, self.g, True, self.est, self.points)
        self.J = (J0, J1)
        self.feed(J0, J1, err)

    def compute_active_errors(self):
        self.feed(self.J[0], self.J[1], producers(self.F, self.g, False, self.est, self.points))

    def chi2(self):
        return self.chi2_fn()

    def update(self):
        x = self.get_x()
        self.est = update(self.F, self.est, self.g["hidx"], x)
        self.points = moved_points(self.points, self.g["pt_hidx"], self.g["nP"], x)

    def push(self):
        self.stack.append((self.est.copy(), self.points.copy()))

    def pop(self):
        self.est, self.points = self.stack.pop()

    def discard_top(self):
        self.stack.pop()
