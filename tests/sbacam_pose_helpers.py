"""Test side of the SBA group's pose-pose constraints (g2ohip_pg_set_cam_edges: type 16 = EdgeSBACam, 17 = EdgeSBAScale, each a set
of its own beside a type-12 pose set): the formulas of openslam_g2o_amd/sbacam.py (ONE body, operation for operation, generic
over the arithmetic) evaluated in fp64 (FP64) and with mpmath at 60 digits (MP), the graphs of the tests and a host-fed graph for
lm.optimize.

Lane mapping of the device kernels: the EdgeSBACam Jacobian runs one lane per (edge, side, column), 12 lanes per edge, 256
threads per block -- 21 edges (252 lanes) fill one block and the 22nd straddles it; the error kernels and the EdgeSBAScale kernel
run one lane per edge -- 257 is one past a block; 300 leaves partial last blocks in both."""
import numpy as np

from openslam_g2o_amd.sbacam import (FP64, cam_edge_error, inverse_measurements, oplus, pose_edges, project_edges,  # noqa: F401
                                     se3_inverse, se3_mul, to_f64, update)
from tests.sbacam_helpers import moved_points, transform_gap  # noqa: F401
from tests.sim3_helpers import MP, mp  # noqa: F401

EDGE_COUNTS = (1, 21, 22, 257, 300)
LM_ARGS = dict(n_cams=12, n_points=60, obs_per_point=4, seed=7, cam_edges=4, scale_edges=2)
HUBER = 0.5          # on the EdgeSBACam set: sqrt(chi2) of an edge at the start is well above it
ITERATIONS = 10
# lm.optimize starts from user_lambda_init = LM_LAMBDA: with the default (1e-5 x the largest diagonal entry) this small problem is
# at its minimum after three iterations, and every later accept / reject decision compares chi2 values that differ by less than
# the noise of the numeric Jacobians -- no two arithmetics agree on those.  From 1e7 the damping comes down by a factor of three
# per accepted step and chi2 still falls by 4 % in the tenth iteration: every decision of the ten is far from a tie.
LM_LAMBDA = 1e7
CAM_KEYS = ("est", "hidx", "vi", "vj", "meas", "info")


def _quat(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(0.5 * angle), [np.cos(0.5 * angle)]])


def _random_cam(rng, spread=3.0):
    return np.concatenate([rng.normal(size=3) * spread, _quat(rng.normal(size=3), rng.uniform(0.2, 1.2))])


def _noisy_relative(rng, ci, cj, st=0.05, sr=0.02):
    """The relative pose Ci^-1 Cj moved by a small step through SBACam::update: a measurement with an error of a few 1e-2."""
    rel = se3_mul(FP64, se3_inverse(FP64, list(ci)), list(cj))
    return to_f64(oplus(FP64, rel, np.concatenate([rng.normal(size=3) * st, rng.normal(size=3) * sr])))


def _info6(rng, n):
    A = rng.normal(size=(n, 6, 6))
    return (A @ A.transpose(0, 2, 1) + 6 * np.eye(6)).reshape(n, 36)


def branch_graph(seed=3):
    """EdgeSBACam, hand-made.  Vertex 0 is fixed.  Edges:
      0 (0, 1) fixed vertex on side 0        1 (2, 0) fixed vertex on side 1        2 (1, 2) both free
      3 (1, 2) the same pair again, another measurement                              4 (2, 1) the pair in the other order
      5 (3, 4) camera 4 is stored with the quaternion -q: normalizeRotation flips in the FIRST product (Ci^-1 Cj)
      6 (5, 6) relative rotation of 2.6 rad against a measurement of -2.6 rad about the same axis: Zinv (Ci^-1 Cj) turns by
               5.2 rad, w = cos(2.6) < 0: the flip in the SECOND product only
      7 (1, 3) the measurement quaternion given as -2.5 q: w < 0 and norm != 1 (flip at binding)
      8 (7, 8) the measurement is the state and e = 0 exactly: C7 = identity, C8 = (t, (0, 0.6, 0, 0.8)), 0.36 + 0.64 = 1
      9 (9, 10) translations of order 1e3
    trace per edge = (flip at binding, flip in product 1, flip in product 2): asserted by the generator."""
    rng = np.random.default_rng(seed)
    nv = 11
    est = np.array([_random_cam(rng) for _ in range(nv)])
    est[4, 3:] = -est[4, 3:]
    axis = np.array([0.3, -0.5, 0.8])
    est[5] = np.concatenate([[0.5, -1.0, 2.0], _quat(axis, 0.0)])
    est[6] = np.concatenate([[1.5, 0.3, 1.0], _quat(axis, 2.6)])
    est[7] = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    est[8] = (1.25, -0.5, 2.0, 0.0, 0.6, 0.0, 0.8)
    est[9, :3] = (1234.5, -2345.25, 987.125)
    est[10, :3] = (1230.75, -2349.5, 990.0)
    pairs = [(0, 1), (2, 0), (1, 2), (1, 2), (2, 1), (3, 4), (5, 6), (1, 3), (7, 8), (9, 10)]
    vi, vj = np.array([a for a, _ in pairs], np.int32), np.array([b for _, b in pairs], np.int32)
    meas = np.array([_noisy_relative(rng, est[a], est[b]) for a, b in pairs])
    meas[6] = np.concatenate([rng.normal(size=3), _quat(axis, -2.6)])
    meas[7, 3:] = -2.5 * meas[7, 3:]
    meas[8] = est[8]
    hidx = np.arange(nv, dtype=np.int32) - 1
    return dict(est=est, hidx=hidx, vi=vi, vj=vj, meas=meas, info=_info6(rng, len(pairs)), nP=nv - 1)


BRANCH_TRACE = {5: (False, True, False), 6: (False, False, True), 7: (True, False, False), 0: (False, False, False)}


def random_graph(n_edges, seed):
    """n_edges EdgeSBACam edges over few cameras (every camera shared by many edges), camera 0 fixed and present on both sides,
    measurements = the relative pose moved by a small step."""
    rng = np.random.default_rng(seed)
    nv = max(2, min(9, n_edges + 1))
    est = np.array([_random_cam(rng) for _ in range(nv)])
    vi = rng.integers(0, nv, n_edges).astype(np.int32)
    vj = ((vi + 1 + rng.integers(0, nv - 1, n_edges)) % nv).astype(np.int32)
    if n_edges >= 2:
        vi[:2], vj[:2] = (0, 1), (1, 0)
    else:
        vi[0], vj[0] = 1, 0
    meas = np.array([_noisy_relative(rng, est[a], est[b]) for a, b in zip(vi, vj)])
    return dict(est=est, hidx=np.arange(nv, dtype=np.int32) - 1, vi=vi, vj=vj, meas=meas, info=_info6(rng, n_edges), nP=nv - 1)


def random_scale_graph(n_edges, seed, est):
    """n_edges EdgeSBAScale edges over the camera table `est` of the EdgeSBACam graph of the same size (so that both sets can be
    bound on one handle), camera 0 fixed and on both sides; measurement = the distance + N(0, 0.05)."""
    rng = np.random.default_rng(seed)
    nv = len(est)
    vi = rng.integers(0, nv, n_edges).astype(np.int32)
    vj = ((vi + 1 + rng.integers(0, nv - 1, n_edges)) % nv).astype(np.int32)
    if n_edges >= 2:
        vi[:2], vj[:2] = (0, 1), (1, 0)
    else:
        vi[0], vj[0] = 1, 0
    meas = np.linalg.norm(est[vj, :3] - est[vi, :3], axis=1) + 0.05 * rng.normal(size=n_edges)
    return dict(est=est, hidx=np.arange(nv, dtype=np.int32) - 1, vi=vi, vj=vj, meas=meas, info=rng.uniform(0.5, 4.0, n_edges), nP=nv - 1)


def coincident_scale_graph():
    """One EdgeSBAScale edge between two free cameras at the same position: |dt| = 0, e = z; every perturbed evaluation has
    |dt| = delta for both signs, so the Jacobian is zero -- finite throughout."""
    rng = np.random.default_rng(9)
    est = np.array([_random_cam(rng), _random_cam(rng)])
    est[1, :3] = est[0, :3]
    return dict(est=est, hidx=np.arange(2, dtype=np.int32), vi=np.array([0], np.int32), vj=np.array([1], np.int32),
                meas=np.array([0.75]), info=np.array([2.0]), nP=2)


def cam_graphs():
    g = dict(branch=branch_graph())
    for i, n in enumerate(EDGE_COUNTS):
        g["c%d" % n] = random_graph(n, 30 + i)
    return g


def scale_graphs():
    g = dict(coincident=coincident_scale_graph())
    for i, n in enumerate(EDGE_COUNTS):
        g["s%d" % n] = random_scale_graph(n, 50 + i, random_graph(n, 30 + i)["est"])
    return g


def producers(F, g, scale, jac=True, cams=None, trace=None):
    return pose_edges(F, g["est"] if cams is None else cams, g["vi"], g["vj"], g["meas"], g["hidx"], scale=scale, jac=jac, trace=trace)


def lm_problem(points=True):
    from openslam_g2o_amd import synthetic as S
    g = S.make_sbacam_ba(**LM_ARGS)
    if not points:
        g = S.make_sbacam_ba(**dict(LM_ARGS, n_points=0, obs_per_point=1))
    return g


# ------------------------------------------------------------------------------------------------ host-fed graph for lm.optimize
class HostSbacamPoseGraph:
    """The graph protocol of openslam_g2o_amd.lm with cameras (and points) on the host and the producers of sbacam.py in
    arithmetic F.  feed(name, J0, J1, err) hands an evaluation of the set `name` ("obs", "cam", "scale") to a solver; get_x()
    reads its solution.  With device_obs the observation set is NOT fed (it stays device-resident in the same solver): the graph
    then reads the cameras back through read_cams() before every evaluation and moves nothing itself."""

    def __init__(self, F, g, feed, get_x, chi2_fn):
        self.F, self.g, self.feed, self.get_x, self.chi2_fn = F, g, feed, get_x, chi2_fn
        self.est = np.array(g["est"], np.float64).copy()
        self.points = np.array(g["points"], np.float64).copy()
        self.with_points = len(g["vp"]) > 0
        self.stack = []
        self.J = {}

    def _eval(self, jac):
        g = self.g
        if self.with_points:
            r = project_edges(self.F, self.est, self.points, g["vp"], g["vl"], g["zl"], g["intrinsics"], g["zl"].shape[1] == 3, jac)
            self._hand("obs", r, jac)
        for name, key, scale in (("cam", "cam_edges", False), ("scale", "scale_edges", True)):
            e = g.get(key)
            if e is not None:
                r = pose_edges(self.F, self.est, e["vi"], e["vj"], e["meas"], g["hidx"], scale=scale, jac=jac)
                self._hand(name, r, jac)

    def _hand(self, name, r, jac):
        if jac:
            self.J[name] = (r[0], r[1])
            self.feed(name, r[0], r[1], r[2])
        else:
            self.feed(name, self.J[name][0], self.J[name][1], r)

    def linearize(self):
        self._eval(True)

    def compute_active_errors(self):
        self._eval(False)

    def chi2(self):
        return self.chi2_fn()

    def update(self):
        x = self.get_x()
        self.est = update(self.F, self.est, self.g["hidx"], x)
        if self.with_points:
            self.points = moved_points(self.points, self.g["pt_hidx"], self.g["nP"], x)

    def push(self):
        self.stack.append((self.est.copy(), self.points.copy()))

    def pop(self):
        self.est, self.points = self.stack.pop()

    def discard_top(self):
        self.stack.pop()
