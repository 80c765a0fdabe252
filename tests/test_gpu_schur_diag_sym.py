"""Schur tiles: a diagonal destination sums V_s V_s', and where every lane group of a wave holds one the destination loop
accumulates a triangle only and rebuilds the block once per destination (schur_tile_dests; build_structure puts the diagonal
destinations of a round first).  Every lane-group form against the CPU oracle with the reduction un-folded
(fuse_schur_reduce = 0: Hschur is materialised): Hschur, bschur, Dinv at 1e-12, dx at dx_tolerance, and every diagonal block of
Hschur exactly symmetric.

Which body a shape reaches is not guessed: every case first runs the host-only census of tools/probe/schur_diag_plan.py (the
planner's tile tables rebuilt in numpy) on its own observation list and requires the intended lane-group width G and, under the
planner's destination order, at least one wave whose lane groups are all diagonal (triangle body, partner exchange), one with
none (general body without the rhs term) and one mixed wave (general body).  The census' tile and partial-block counts equal the
library's at the benchmark's configuration (profiles/schur_diag_sym.txt).

The random-Jacobian cases use identity information: J' J is assembled exactly symmetric, a general J' W J is not (its two
triangles round differently), and the symmetry check is about what the tiles subtract from Hpp."""
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


def _plan():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probe", "schur_diag_plan.py")
    spec = importlib.util.spec_from_file_location("schur_diag_plan", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _require_waves(name, v0, v1, nP, G, p=6, l=3):
    """The shape runs with lane groups of G lanes and holds all three kinds of waves."""
    c = _plan().census(np.asarray(v0, np.int64) - nP, v1, nP, PD=p, LD=l)
    w = c["orders"]["round"]
    print(name, "census: G", c["G"], "entries per partial %.2f" % c["avg"], "tiles", c["n_tiles"], "waves all-diagonal / all-off-diagonal / mixed",
          w["all_diag"], w["all_off"], w["mixed"], "diagonal entries in all-diagonal waves %.2f" % (w["cov"] / c["n_diag_ent"]))
    assert c["G"] == G, (name, c["G"], c["avg"])
    assert w["all_diag"] > 0 and w["all_off"] > 0 and w["mixed"] > 0, (name, w)


def _device_copy(s, which):
    import torch
    from openslam_g2o_amd.distributed import tensor_from_device_ptr
    ptr, n = s.deviceArray(which)
    s.sync()
    return tensor_from_device_ptr(ptr, n, torch.device("cuda:0")).cpu().numpy().copy()


def _diag_blocks(s, capi, p):
    cp, ri = s.pattern(capi.HSCHUR)
    V = s.values(capi.HSCHUR).reshape(-1, p, p)
    return [V[q] for c in range(len(cp) - 1) for q in range(cp[c], cp[c + 1]) if ri[q] == c]


def _check_solve(s, o, p, name, expect_ok=True):
    """The damping is set on both sides.  Split interface on the device (bschur is read before the reduced solve); the figures
    are printed before they are held to their bounds.  Hschur, bschur, Dinv and the symmetry always; dx whenever the oracle's
    solve succeeds; the status against the oracle's."""
    capi = _capi()
    s.solveSchur()
    bs = _device_copy(s, capi.ARR_BSCHUR)
    ok = s.solveReduced()
    ok_o = o.solve()
    figs = dict(Hschur=relerr(s.values(capi.HSCHUR), o.values("Hschur")), Dinv=relerr(s.values(capi.DINV), o.values("Dinv")),
                bschur=relerr(bs[:len(o.bschur())], o.bschur()))
    tol = cond = None
    if ok and ok_o:
        s.solveBackSubstitute()
        tol, cond = dx_tolerance(o)
        figs.update(dx=relerr(s.x(), o.x()), dx_tol=tol)
    blocks = _diag_blocks(s, capi, p)
    asym = sum(not np.array_equal(B, B.T) for B in blocks)
    print(name, "ok", ok, ok_o, figs, "diagonal blocks", len(blocks), "not symmetric", asym)
    assert ok is ok_o and ok_o is expect_ok, (name, ok, ok_o)
    assert figs["Hschur"] < TOL_MAT and figs["Dinv"] < TOL_MAT and figs["bschur"] < TOL_MAT, figs
    if ok_o:
        assert figs["dx"] < tol, (figs, cond)
    assert len(blocks) == s.pattern(capi.HSCHUR)[0].shape[0] - 1 and asym == 0


def _check(s, o, p, lam, name):
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    _check_solve(s, o, p, name)
    s.restoreDiagonal()
    o.restore_diagonal()


def _subset(pr, keep):
    out = dict(pr)
    for k in ("v0", "v1", "Jp", "Jc", "omega", "err", "cam_idx", "pt_idx", "meas"):
        out[k] = pr[k][keep]
    out["E"] = int(keep.sum())
    return out


def test_chain_ba_two_row_halves_four_entry_parts():
    """G = 8 (the benchmark's width: more than 16 entries per partial block): 40 poses / 400 landmarks with five observations
    each, 12 tiles of ~33 destinations for the 32 lane groups of a round, 8-9 diagonal ones per tile -- wave 0 of a tile is
    all-diagonal (the VSlot::PERM load of both row halves, the lane ^ 12 exchange), the others mixed or off-diagonal.  The generic
    tile kernel (Hpl from memory) and the fused one (Hpl evaluated by the tile from the estimates) run the same loop."""
    from openslam_g2o_amd import lm
    pr = ba_case(40, 400)
    _require_waves("chain G = 8", pr["v0"], pr["v1"], pr["nP"], 8)
    o = oracle_ba(pr)
    o.build_system()
    lam = 1e-3 * o.max_diagonal()
    s = hip_ba(pr, options=UNFOLDED)
    s.buildSystem()
    _check(s, o, 6, lam, "generic")
    sf, g = lm.setup_device_ba(pr, options=UNFOLDED)
    g.linearize()
    sf.buildSystem()
    _check(sf, o, 6, lam, "fused")


def test_chain_ba_two_row_halves_two_entry_parts():
    """G = 4 (2 to 16 entries per partial block): two landmarks per pose, so a tile's 35 landmarks touch ~20 poses and its
    diagonal destinations fill the 16 lane groups of wave 0 (partner half at lane ^ 2)."""
    pr = ba_case(60, 120)
    _require_waves("chain G = 4", pr["v0"], pr["v1"], pr["nP"], 4)
    o = oracle_ba(pr)
    o.build_system()
    s = hip_ba(pr, options=UNFOLDED)
    s.buildSystem()
    _check(s, o, 6, 1e-3 * o.max_diagonal(), "chain G = 4")


def test_mixed_list_lengths():
    """Landmarks seen once (a diagonal entry and nothing else), twice, and five times in one problem: the diagonal lists are
    several times longer than the off-diagonal ones, and a tile (four landmarks per pose) holds more diagonal destinations than
    a wave has lane groups."""
    pr = ba_case(120, 480)
    lmk = pr["pt_idx"]
    nth = np.arange(pr["E"]) - np.searchsorted(lmk, lmk)              # position inside the landmark's list
    keep = np.ones(pr["E"], bool)
    keep[(lmk % 3 == 1) & (nth >= 1)] = False                          # K = 1
    keep[(lmk % 3 == 2) & (nth >= 2)] = False                          # K = 2
    pr = _subset(pr, keep)
    counts = np.bincount(pr["pt_idx"], minlength=pr["nL"])
    assert set(np.unique(counts)) >= {1, 2, 5}
    _require_waves("mixed", pr["v0"], pr["v1"], pr["nP"], 4)
    o = oracle_ba(pr)
    o.build_system()
    s = hip_ba(pr, options=UNFOLDED)
    s.buildSystem()
    _check(s, o, 6, 1e-3 * o.max_diagonal(), "mixed")


def _generic(p, l, d, nP, nL, cam, K, seed, G):
    """Random Jacobians through the generic edge-data path (as test_block_solver_dimension_families), identity information; a
    chain of pose-pose edges keeps the poses connected."""
    capi = _capi()
    rng = np.random.default_rng(seed)
    v0, v1 = (nP + np.repeat(np.arange(nL), K)).astype(np.int32), cam.astype(np.int32)
    _require_waves("%d_%d" % (p, l), v0, v1, nP, G, p, l)
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
    return s, o


@pytest.mark.parametrize("p,l,d", [(3, 2, 2), (7, 3, 2)])
def test_odd_pose_dimension_families(p, l, d):
    """BlockSolver_3_2 and _7_3: an odd pose dimension has no row halves (one lane owns all rows of a destination, here with four
    entry parts): the lower triangle is accumulated and mirrored in registers."""
    nP, nL, K = 40, 150, 4
    rng = np.random.default_rng(1000 * p + 10 * l + d)
    cam = (rng.integers(0, nP - K, size=nL)[:, None] + np.arange(K)[None, :]).reshape(-1)
    s, o = _generic(p, l, d, nP, nL, cam, K, 7 * p + l, 4)
    _check(s, o, p, 1e-3 * o.max_diagonal(), "%d_%d" % (p, l))


def test_one_lane_per_destination():
    """At most two entries per partial block on average: one lane per destination (G = 1), 64 destinations per wave.  A small
    grid (visibility by a distance that leaves two to five observations per point, so that a tile holds more than 64 diagonal
    destinations) and a graph of landmarks seen by two random poses each."""
    pr = S.make_ba_grid(100, pts_per_cam=3, radius=0.55)
    Jp, Jc, err = S.ba_linearize(pr)
    pr.update(Jp=Jp, Jc=Jc, err=err, omega=S.ba_omega(pr))
    _require_waves("grid", pr["v0"], pr["v1"], pr["nP"], 1)
    o = oracle_ba(pr)
    o.build_system()
    s = hip_ba(pr, options=UNFOLDED)
    s.buildSystem()
    _check(s, o, 6, 1e-3 * o.max_diagonal(), "grid")
    rng = np.random.default_rng(5)
    nP, nL = 200, 400
    cam = np.stack([rng.integers(0, nP // 2, size=nL), rng.integers(nP // 2, nP, size=nL)], axis=1).reshape(-1)
    s, o = _generic(6, 3, 2, nP, nL, cam, 2, 5, 1)
    # two observations of a 3-dof point by 2-dof measurements leave the landmark blocks near singular without damping
    _check(s, o, 6, 1e-1 * o.max_diagonal(), "two random poses per landmark")


def test_negative_lambda_takes_the_signed_tiles():
    """Negative damping (block_solver.hpp:563-604 allows it): the tiles with a landmark block that is not positive definite
    scale the rows by Sg = diag(+-1) and keep the general body -- on a shape whose waves would otherwise take the triangle body.
    (a) lambda = -10 max diag(H) on everything: the reduced system is not positive definite, the status is the oracle's, and what
    the tiles wrote (Hschur, bschur, Dinv) still equals the oracle's.  (b) a negative landmark damping between the eigenvalues
    of the landmark blocks with a pose damping that keeps the reduced system positive definite
    (test_indefinite_landmark_blocks_take_the_signed_split): the solve succeeds and dx is compared too.  (c) an ordinary solve
    afterwards: the flag is per solve."""
    pr = ba_case(40, 400)
    _require_waves("negative lambda", pr["v0"], pr["v1"], pr["nP"], 8)
    s, o = hip_ba(pr, options=UNFOLDED), oracle_ba(pr)
    s.buildSystem()
    o.build_system()
    lam = -10.0 * o.max_diagonal()
    s.setLambda(lam, True)
    o.set_lambda(lam, True)
    _check_solve(s, o, 6, "negative lambda", expect_ok=False)
    assert s.solve() is False
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
    _check_solve(s, o, 6, "indefinite landmark blocks")
    s.restoreDiagonal()
    o.restore_diagonal()
    _check(s, o, 6, 1e-3 * o.max_diagonal(), "after the negative lambda")
