"""Test side of the Sim3 pose-pose edge (g2ohip_pg_set_edges type 10): the formulas of openslam_g2o_amd/sim3.py -- ONE body,
operation for operation in the reference's order, generic over the arithmetic -- evaluated in fp64 (FP64) and with mpmath at
60 digits (MP), the same delta and the same branches chosen by the same comparisons; the graphs of the tests (every exp / log
branch class, shared and fixed vertices) and a host-fed graph for lm.optimize."""
import mpmath as mp
import numpy as np

from openslam_g2o_amd.sim3 import (DELTA64, EPS64, FP64, IDENTITY, chi2, edges, q_to_R, sim3_error, sim3_exp,  # noqa: F401
                                   sim3_inverse, sim3_jacobians, sim3_log, sim3_mul, sim3_oplus, to_f64, transform, update)

DPS = 60
mp.mp.dps = DPS


class MP:
    name = "mp"
    sin, cos, exp, log, acos, sqrt = mp.sin, mp.cos, mp.exp, mp.log, mp.acos, mp.sqrt

    @staticmethod
    def num(x):
        return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


# ------------------------------------------------------------------------------------------------ branch-class inputs
# |sigma| outside [1e-6, 1e-4], theta outside [1e-3, 2e-2]: away from eps = 1e-5 on sigma and theta, and from d = cos(theta) >
# 1 - 1e-5 (theta ~ 4.47e-3) of log
SMALL_SIGMA, BIG_SIGMA = 3e-7, 0.21
SMALL_THETA, BIG_THETA = 4e-7, 0.83


def branch_vector(branch, rng):
    """A minimal vector whose exp takes `branch` and whose exp's log takes the same-numbered branch."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    theta = BIG_THETA if branch & 1 else SMALL_THETA
    sigma = BIG_SIGMA if branch & 2 else SMALL_SIGMA
    return np.concatenate([axis * theta * rng.uniform(0.8, 1.2), rng.normal(size=3), [sigma * rng.choice([-1.0, 1.0])]])


def branch_class_graph(seed=5, exact_zero=True):
    """16 edges over 17 vertices + one: for every log branch b (0..3) of the error, four edges whose measurement C makes
    C Si Sj^-1 = exp(branch_vector(b)) up to rounding, with vertex 0 (fixed) on side 0 of the first and on side 1 of the second;
    the last edge has C = Sj Si^-1 formed so that the error is EXACTLY zero (Si = identity, C = Sj: C * I * Sj^-1 has r = q q*,
    t = 0 exactly when Sj has t = 0, s = 1 and a quaternion whose product with its conjugate rounds to (0, 0, 0, 1))."""
    rng = np.random.default_rng(seed)
    nv = 18
    est = np.zeros((nv, 8))
    for v in range(nv):
        x = np.concatenate([rng.normal(size=3) * 0.6, rng.normal(size=3) * 2.0, [rng.normal() * 0.3]])
        est[v] = to_f64(sim3_exp(FP64, x))
    est[16] = IDENTITY
    est[17] = (0.0, 0.6, 0.0, 0.8, 0.0, 0.0, 0.0, 1.0)       # 0.36 + 0.64 = 1 exactly in fp64
    vi, vj, meas = [], [], []
    for b in range(4):
        for m in range(4):
            k = 4 * b + m
            i, j = (0, k + 1) if m == 0 else ((k + 1, 0) if m == 1 else (k, k + 1))
            E = sim3_exp(FP64, branch_vector(b, rng))
            C = sim3_mul(FP64, sim3_mul(FP64, E, est[j]), sim3_inverse(FP64, est[i]))
            vi.append(i)
            vj.append(j)
            meas.append(to_f64(C))
    if exact_zero:
        vi.append(16)
        vj.append(17)
        meas.append(est[17].copy())
    hidx = np.arange(nv, dtype=np.int32) - 1                   # vertex 0 fixed
    A = rng.normal(size=(len(vi), 7, 7))
    info = (A @ A.transpose(0, 2, 1) + 7 * np.eye(7)).reshape(len(vi), 49)
    return dict(est=est, hidx=hidx, vi=np.array(vi, np.int32), vj=np.array(vj, np.int32), meas=np.array(meas), info=info,
                num_free=nv - 1)


def random_graph(n_edges, seed, n_vertices=None):
    """n_edges edges over few vertices (every vertex shared by many edges), vertex 0 fixed and present on both sides,
    measurements = relative pose times exp(noise): generic branch (3, 3) errors."""
    rng = np.random.default_rng(seed)
    nv = n_vertices or max(2, min(12, n_edges + 1))
    est = np.zeros((nv, 8))
    for v in range(nv):
        est[v] = to_f64(sim3_exp(FP64, np.concatenate([rng.normal(size=3) * 0.5, rng.normal(size=3) * 3.0, [rng.normal() * 0.2]])))
    vi = rng.integers(0, nv, n_edges).astype(np.int32)
    vj = ((vi + 1 + rng.integers(0, nv - 1, n_edges)) % nv).astype(np.int32)
    if n_edges >= 2:
        vi[0], vj[0] = 0, 1
        vi[1], vj[1] = 1, 0
    meas = np.zeros((n_edges, 8))
    for k in range(n_edges):
        noise = np.concatenate([rng.normal(size=3) * 0.05, rng.normal(size=3) * 0.1, [rng.normal() * 0.05]])
        rel = sim3_mul(FP64, est[vj[k]], sim3_inverse(FP64, est[vi[k]]))
        meas[k] = to_f64(sim3_mul(FP64, sim3_exp(FP64, noise), rel))
    A = rng.normal(size=(n_edges, 7, 7))
    info = (A @ A.transpose(0, 2, 1) + 7 * np.eye(7)).reshape(n_edges, 49)
    return dict(est=est, hidx=np.arange(nv, dtype=np.int32) - 1, vi=vi, vj=vj, meas=meas, info=info, num_free=nv - 1)


# ------------------------------------------------------------------------------------------------ host-fed graph for lm.optimize
class HostSim3Graph:
    """The graph protocol of openslam_g2o_amd.lm with the estimates on the host and the producers of this file in arithmetic
    F: feed(J0, J1, err) hands every evaluation to a solver (set_edge_data), get_x() reads its solution."""

    def __init__(self, F, g, feed, get_x, chi2_fn, fix_scale=False):
        self.F, self.g, self.feed, self.get_x, self.chi2_fn, self.fix_scale = F, g, feed, get_x, chi2_fn, fix_scale
        self.est = np.array(g["est"], np.float64).copy()
        self.stack = []
        self.J = None

    def linearize(self):
        J0, J1, err = edges(self.F, self.est, self.g["vi"], self.g["vj"], self.g["meas"], self.g["hidx"], self.fix_scale)
        self.J = (J0, J1)
        self.feed(J0, J1, err)

    def compute_active_errors(self):
        err = edges(self.F, self.est, self.g["vi"], self.g["vj"], self.g["meas"], jac=False)
        self.feed(self.J[0], self.J[1], err)

    def chi2(self):
        return self.chi2_fn()

    def update(self):
        self.est = update(self.F, self.est, self.g["hidx"], self.get_x(), self.fix_scale)

    def push(self):
        self.stack.append(self.est.copy())

    def pop(self):
        self.est = self.stack.pop()

    def discard_top(self):
        self.stack.pop()
