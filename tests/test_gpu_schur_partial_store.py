"""Schur tiles: how a lane group writes its partial block (schur_tile_dests).  With lane groups of 8, and of 4 with row halves, the
sum over the entry parts is a reduce-scatter that leaves the lane ge with the 16-byte pieces ge, GE + ge, ... of its row part, and
those go out as whole-group stores; the triangle body picks the same pieces with selects; the right-hand-side rows of a diagonal
destination are one store.  Every other width keeps one store per piece.  The stored bytes and their addresses are the same in
all forms, so the checks are the ones of tests/test_gpu_schur_diag_sym.py: Hschur, bschur, Dinv at 1e-12 and dx at dx_tolerance
against the CPU oracle with the reduction un-folded -- and two consecutive solves have to agree bit for bit.

What a shape makes the destination loop do is read from the planner's tables rebuilt on the host (tools/probe/schur_diag_plan.py):
the lane-group width, the number of tiles and of destinations (a ragged last round, fewer destinations than one wave has lane
groups, a single destination) and the kinds of waves (all lane groups diagonal, none, mixed)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import ba_case, dx_tolerance, hip_ba, oracle_ba, relerr
from openslam_g2o_amd import synthetic as S

pytestmark = pytest.mark.gpu

TOL_MAT = 1e-12
UNFOLDED = {"fuse_schur_reduce": 0}


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _census(v0, v1, nP, p=6, l=3):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probe", "schur_diag_plan.py")
    spec = importlib.util.spec_from_file_location("schur_diag_plan", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    c = mod.census(np.asarray(v0, np.int64) - nP, v1, nP, PD=p, LD=l)
    w = c["orders"]["round"]
    print("census: G", c["G"], "entries per partial %.2f" % c["avg"], "tiles", c["n_tiles"], "destinations", c["n_td"],
          "waves all-diagonal / all-off-diagonal / mixed", w["all_diag"], w["all_off"], w["mixed"])
    return c, w


def _device_copy(s, which):
    import torch
    from openslam_g2o_amd.distributed import tensor_from_device_ptr
    ptr, n = s.deviceArray(which)
    s.sync()
    return tensor_from_device_ptr(ptr, n, torch.device("cuda:0")).cpu().numpy().copy()


def _solve(s, back=True):
    capi = _capi()
    s.solveSchur()
    out = dict(bschur=_device_copy(s, capi.ARR_BSCHUR))
    ok = s.solveReduced()
    out.update(Hschur=s.values(capi.HSCHUR).copy(), Dinv=s.values(capi.DINV).copy())
    if ok and back:
        s.solveBackSubstitute()
        out["dx"] = np.array(s.x(), copy=True)
    return ok, out


def _check_solve(s, o, name, expect_ok=True):
    """The damping is set on both sides.  The figures are printed before they are held to their bounds; the second solve of the
    same system has to reproduce every array of the first to the bit."""
    ok, a = _solve(s)
    ok2, b = _solve(s)
    ok_o = o.solve()
    figs = dict(Hschur=relerr(a["Hschur"], o.values("Hschur")), Dinv=relerr(a["Dinv"], o.values("Dinv")),
                bschur=relerr(a["bschur"][:len(o.bschur())], o.bschur()))
    tol = cond = None
    if ok and ok_o:
        tol, cond = dx_tolerance(o)
        figs.update(dx=relerr(a["dx"], o.x()), dx_tol=tol)
    same = {k: bool(np.array_equal(a[k], b[k])) for k in a}
    print(name, "ok", ok, ok2, ok_o, figs, "second solve bit-identical", same)
    assert ok is ok_o and ok2 is ok and ok_o is expect_ok, (name, ok, ok2, ok_o)
    assert figs["Hschur"] < TOL_MAT and figs["Dinv"] < TOL_MAT and figs["bschur"] < TOL_MAT, figs
    if ok_o:
        assert figs["dx"] < tol, (figs, cond)
    assert sorted(a) == sorted(b) and all(same.values()), same


def _check(s, o, lam, name):
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    _check_solve(s, o, name)
    s.restoreDiagonal()
    o.restore_diagonal()


def _generic(p, l, d, nP, lm, cam, seed):
    """Random Jacobians through the generic edge-data path (schur_tile_kernel<p, l, G>: Hpl, Hll and b_l read from memory), identity
    information; observation k is landmark lm[k] seen by pose cam[k]; a chain of pose-pose edges keeps the poses connected."""
    capi = _capi()
    rng = np.random.default_rng(seed)
    nL = int(np.max(lm)) + 1
    v0, v1 = (nP + np.asarray(lm)).astype(np.int32), np.asarray(cam).astype(np.int32)
    E = len(v0)
    J0, J1 = rng.normal(size=(E, d * l)), rng.normal(size=(E, d * p))
    om = np.tile(np.eye(d).reshape(-1), (E, 1))
    err = rng.normal(size=(E, d))
    a, b = np.arange(0, nP - 1, dtype=np.int32), np.arange(1, nP, dtype=np.int32)
    n = len(a)
    JA, JB = rng.normal(size=(n, p * p)), rng.normal(size=(n, p * p))
    O2 = np.tile(np.eye(p).reshape(-1), (n, 1))
    e2 = rng.normal(size=(n, p))
    s = capi.HipBlockSolver(p, l, 0)
    s.setOption("fuse_schur_reduce", 0)
    k0, k1 = s.addEdgeSet(d, v0, v1), s.addEdgeSet(p, a, b)
    s.buildStructure(nP, nL, True)
    o = O.OracleSolver(p, l, nP, nL, True)
    q0 = o.add_edge_set(d, v0, v1); o.set_dims(q0, l, p)
    q1 = o.add_edge_set(p, a, b); o.set_dims(q1, p, p)
    o.build_structure()
    s.setEdgeData(k0, J0, J1, om, err); o.set_edge_data(q0, J0, J1, om, err)
    s.setEdgeData(k1, JA, JB, O2, e2); o.set_edge_data(q1, JA, JB, O2, e2)
    s.buildSystem()
    o.build_system()
    return s, o, v0, v1


def _lists(sets, copies):
    """copies landmarks per pose set: landmark ids and poses of the observations."""
    lm, cam, j = [], [], 0
    for ps in sets:
        for _ in range(copies):
            lm += [j] * len(ps)
            cam += list(ps)
            j += 1
    return np.array(lm), np.array(cam)


# (name, poses, pose sets of the landmarks, landmarks per set, destinations of the one tile, waves all-diagonal / none / mixed)
RAGGED = [
    # two poses that share every landmark: (0,0), (1,1), (1,0) -- fewer destinations than a wave has lane groups, one mixed wave
    ("3 destinations", 2, [(0, 1)], 40, 3, (0, 0, 1)),
    # five poses, eight of their ten pairs: 13 = 8 + 5 destinations -- wave 0 holds the five diagonal and three others, wave 1 is
    # not full (five of its eight lane groups run)
    ("13 destinations", 5, [(0, 1, 2), (2, 3, 4), (0, 3), (1, 4)], 12, 13, (0, 1, 1)),
    # every landmark is seen by pose 0 alone (pose 1 hangs on the pose-pose edge): ONE destination, diagonal, one lane group runs
    ("1 destination", 2, [(0,)], 20, 1, (1, 0, 0)),
]


@pytest.mark.parametrize("name,nP,sets,copies,n_td,waves", RAGGED, ids=[r[0].replace(" ", "_") for r in RAGGED])
def test_ragged_rounds_of_one_tile(name, nP, sets, copies, n_td, waves):
    """Lane groups of 8 (more than 16 entries per partial block) on ONE tile whose destination count is not a multiple of the
    eight lane groups of a wave, below them, and one: the lanes past the last destination store nothing."""
    lm, cam = _lists(sets, copies)
    s, o, v0, v1 = _generic(6, 3, 2, nP, lm, cam, 11 + n_td)
    c, w = _census(v0, v1, nP)
    assert c["G"] == 8 and c["n_tiles"] == 1 and c["n_td"] == n_td, (c["G"], c["n_tiles"], c["n_td"])
    assert (w["all_diag"], w["all_off"], w["mixed"]) == waves, w
    # (few observations of a 3-dof point by 2-dof measurements: the damping keeps the landmark blocks well conditioned)
    _check(s, o, 1e-1 * o.max_diagonal(), name)


def test_one_destination_one_entry():
    """The smallest tile there is: one landmark seen by one pose -- one destination with one entry, one lane per destination."""
    s, o, v0, v1 = _generic(6, 3, 2, 2, np.array([0]), np.array([0]), 3)
    c, w = _census(v0, v1, 2)
    assert c["G"] == 1 and c["n_tiles"] == 1 and c["n_td"] == 1 and c["n_ent"] == 1
    _check(s, o, 1e-1 * o.max_diagonal(), "one entry")


def _ba(P, L, G):
    pr = ba_case(P, L)
    c, w = _census(pr["v0"], pr["v1"], pr["nP"])
    assert c["G"] == G, (c["G"], c["avg"])
    assert w["all_diag"] > 0 and w["all_off"] > 0 and w["mixed"] > 0, w     # an all-diagonal wave round and a mixed one
    return pr


def test_width_8_generic_and_fused():
    """G = 8, the benchmark's width (two row halves x four entry parts: 64-byte runs per store, reduce-scatter over lane ^ 1 and
    lane ^ 2), with all-diagonal, mixed and off-diagonal waves and 12 tiles of ~33 destinations (a second round of one or two):
    the generic tile kernel on Jacobian arrays and the fused one, which evaluates Hpl from the estimates."""
    from openslam_g2o_amd import lm
    pr = _ba(40, 400, 8)
    o = oracle_ba(pr)
    o.build_system()
    lam = 1e-3 * o.max_diagonal()
    s = hip_ba(pr, options=UNFOLDED)
    s.buildSystem()
    _check(s, o, lam, "generic")
    sf, g = lm.setup_device_ba(pr, options=UNFOLDED)
    g.linearize()
    sf.buildSystem()
    _check(sf, o, lam, "fused")


def test_width_4_row_halves():
    """G = 4 (two row halves x two entry parts: 32-byte runs, four whole-group stores and the ninth piece from the lane ge = 0)."""
    pr = _ba(60, 120, 4)
    o = oracle_ba(pr)
    o.build_system()
    s = hip_ba(pr, options=UNFOLDED)
    s.buildSystem()
    _check(s, o, 1e-3 * o.max_diagonal(), "G = 4")


def test_width_1_keeps_the_plain_store():
    """G = 1 (at most two entries per partial block): one lane per destination stores its whole block."""
    pr = S.make_ba_grid(100, pts_per_cam=3, radius=0.55)
    Jp, Jc, err = S.ba_linearize(pr)
    pr.update(Jp=Jp, Jc=Jc, err=err, omega=S.ba_omega(pr))
    c, w = _census(pr["v0"], pr["v1"], pr["nP"])
    assert c["G"] == 1 and w["all_diag"] > 0 and w["mixed"] > 0, (c["G"], w)
    o = oracle_ba(pr)
    o.build_system()
    s = hip_ba(pr, options=UNFOLDED)
    s.buildSystem()
    _check(s, o, 1e-3 * o.max_diagonal(), "grid")


@pytest.mark.parametrize("p,l,G", [(6, 3, 8), (7, 3, 4)])
def test_generic_families(p, l, G):
    """Random Jacobian arrays: (6, 3) with lane groups of 8 takes the new store, (7, 3) -- an odd pose dimension has no row halves
    and 49 doubles per block -- keeps one store per double."""
    nP, nL, K = (24, 320, 6) if p == 6 else (40, 150, 4)
    rng = np.random.default_rng(1000 * p + 10 * l)
    first = rng.integers(0, nP - K, size=nL)
    if p == 6:
        first = np.sort(first)       # (neighbouring landmarks see the same poses: 19 entries per partial block)
    cam = (first[:, None] + np.arange(K)[None, :]).reshape(-1)
    s, o, v0, v1 = _generic(p, l, 2, nP, np.repeat(np.arange(nL), K), cam, 7 * p + l)
    c, w = _census(v0, v1, nP, p, l)
    assert c["G"] == G, (c["G"], c["avg"])
    assert w["all_diag"] > 0 and w["mixed"] + w["all_off"] > 0, w
    _check(s, o, 1e-3 * o.max_diagonal(), "%d_%d" % (p, l))


def test_negative_damping_signed_tiles():
    """Negative damping: a tile with a landmark block that is not positive definite keeps the general body with the rows scaled
    by Sg = diag(+-1), on a shape whose waves otherwise take the triangle body -- the reduce-scatter feeds the stores there too.
    (a) lambda = -10 max diag(H): the reduced solve fails like the oracle's, what the tiles wrote still equals the oracle's.
    (b) a negative landmark damping between the eigenvalues of the landmark blocks with a pose damping that keeps the reduced
    system positive definite: dx is compared as well."""
    pr = _ba(40, 400, 8)
    s, o = hip_ba(pr, options=UNFOLDED), oracle_ba(pr)
    s.buildSystem()
    o.build_system()
    lam = -10.0 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    _check_solve(s, o, "negative lambda", expect_ok=False)
    s.restoreDiagonal()
    o.restore_diagonal()
    ev = np.linalg.eigvalsh(o.values("Hll").reshape(-1, 3, 3))
    allev = np.sort(ev.reshape(-1))
    best = None
    for a, b in zip(allev[:-1], allev[1:]):
        mid = 0.5 * (a + b)
        indef = int(((ev[:, 0] < mid) & (ev[:, 2] > mid)).sum())
        if indef >= 50 and (best is None or (b - a) / mid > best[0]):
            best = ((b - a) / mid, mid, indef)
    assert best is not None
    lam_l = -float(best[1])
    gap = float(np.abs(ev + lam_l).min())
    lam_p = 100.0 * float(np.abs(o.dense_full()).max()) ** 2 / gap
    s.setLambdaSplit(lam_p, lam_l, True)
    o.set_lambda_split(lam_p, lam_l, True)
    _check_solve(s, o, "indefinite landmark blocks")
    s.restoreDiagonal()
    o.restore_diagonal()
