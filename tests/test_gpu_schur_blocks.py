"""The Schur complement and the landmark back-substitution block by block against a 60-digit reference
(tests/golden/schur_blocks.npz, written by tests/golden/make_schur_blocks.py; inputs, census and measure in
tests/schur_helpers.py).  No reference is evaluated here and no oracle library is read: the inputs are rebuilt from their
seeds, their SHA-256 is the fixture's, and every device stage runs on pinned inputs:

  1. assembly (generic edge-data path): values(HPP / HPL / HLL), b() and the three patterns bit for bit the exact assembly of the
     helper, whose hash the fixture holds -- what follows is the Schur stage alone;
  2. setLambda, solveSchur: Dinv, every block of Hschur and of bschur against its own scale;
  3. setX([pinned x_p, 0]) and solveBackSubstitute alone: x_l block by block, no factorisation in front of it;
  4. (at most 60 poses) solve() on a fresh handle at its defaults: bschur as solve() left it, then x_p and x_l;
  5. every diagonal block of Hschur exactly symmetric (the assembled Hpp is, being exact; the tiles subtract V V').

The bound of (case, output) is 8 x the larger of the two CPU figures the fixture records; figures are printed before they are
held, one line "SCHURBLK {json}" per output (the device rows of profiles/schur_blocks.jsonl are these lines from a pytest -s run).

Which kernel a path reaches, and from what that is asserted:
  schur_tile_kernel<P, L, G>      path "split": generic edge data (no BA front end is bound), the tiles always run
                                  (solve_schur_impl); (P, L) is the handle's, G = pick_group of the census, asserted per case
                                  (1, 4, 8), with the three kinds of waves where the case is there for them
  schur_reduce_kernel             path "split": option fuse_schur_reduce = 0 and solveSchur (which materialises Hschur with
                                  any option); on the path "solve" again through values(HSCHUR) (ensure_hschur)
  schur_rhs_kernel                path "solve": defaults (fuse_schur_reduce = 1), one GPU, direct solver, and the census' partial
                                  blocks at most 6 per destination (virtual_reduced_ok), asserted; ARR_BSCHUR is what it wrote
  back_substitute_kernel<P, L>    paths "split" and "solve" (no BA front end: the generic kernel), and path "operator" (Dinv b_l
                                  for the operator's right-hand side)
  landmark_inverse_kernel<L>      path "operator": the tiles invert their landmarks themselves, so only schurOperatorPrepare
                                  launches this kernel (with back_substitute_kernel for Dinv b_l); Dinv and bschur after it,
                                  for the (P, L) the matrix-free operator is instantiated for
  mf_pose_kernel<P, L>            path "operator": it is the writer of ARR_BSCHUR there (b_p - Hpl (Dinv b_l), pose by pose over the
                                  pose-major lists of Hpl), from the Dinv of landmark_inverse_kernel and the Dinv b_l of
                                  back_substitute_kernel: a bschur figure over its bound on this path alone points at it
  ba_schur_tile_kernel<G, FLL, CLS>   test_fused_ba_schur_stage: option ba_fused = 1 with estimates bound (one class: CLS = false,
                                  G of the census; class table: CLS = true, G mapped to 1 or 8).  FLL = true: ba_fuse_landmarks = 1
                                  and the first solveSchur after buildSystem, nothing having read Hll, b or the errors in between
                                  (build_system leaves the landmark side to the tiles).  FLL = false: the second damping after
                                  maxDiagonal(), a reader that puts Hll into memory (ensure_ll) as the LM loop does between its
                                  trials, and both dampings with ba_fuse_landmarks = 0
  ba_back_substitute_slots_kernel<CLS>   ba_fuse_landmarks = 1;   ba_back_substitute_kernel<G, CLS>   ba_fuse_landmarks = 0
                                  (solve_back_substitute_impl chooses by that option while the estimates are unchanged)
stats() holds the dimensions only; the tile tables and the fused path's flags are not exported, so tile and partial-block counts are
the census' and the fused reach rests on the options and the call order above.  The two constants copied from the
library (kFuseReduceMaxPartials, schur_tile_bytes: tests/schur_helpers.py) are held to its sources by
tests/test_schur_reference_host.py."""
import json

import numpy as np
import pytest

from tests import schur_helpers as H

pytestmark = pytest.mark.gpu

NAMES = sorted(H.CASES)
OPERATOR_DIMS = ((6, 3), (3, 2), (7, 3))
FUSE_REDUCE_MAX_PARTIALS = H.FUSE_REDUCE_MAX_PARTIALS


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _device_copy(s, which):
    import torch
    from openslam_g2o_amd.distributed import tensor_from_device_ptr
    ptr, n = s.deviceArray(which)
    s.sync()
    return tensor_from_device_ptr(ptr, n, torch.device("cuda:0")).cpu().numpy().copy()


def _hold(k, cen, path, output, got, ref_name=None, failures=None):
    assert failures is not None
    ref_name = ref_name or output
    f = H.figures(got, k["ref"][ref_name], k["scale"][ref_name])
    worst = int(np.argmax(f))
    bound = k["bound"][ref_name]
    print("SCHURBLK " + json.dumps(dict(case=k["name"], path=path, output=output, G=cen["G"], device=float(f.max()), block=worst,
                                        bound=bound, cpu_oracle=k["cpu"][ref_name][0], cpu_numpy=k["cpu"][ref_name][1],
                                        device_over_cpu=float(f.max()) / max(max(k["cpu"][ref_name]), 1e-300))))
    if not f.max() <= bound:
        failures.append((path, output, worst, float(f.max()), bound))


def _assert_assembly(capi, s, k):
    """The device's system is the helper's exact assembly bit for bit, and that is the one the fixture was computed for."""
    c, a = k["c"], k["a"]
    assert H.input_hash(c) == k["input_sha"]
    got = dict(pp=s.pattern(capi.HPP), pl=s.pattern(capi.HPL), hs=s.pattern(capi.HSCHUR), b=s.b(),
               Hpp=s.values(capi.HPP).reshape(-1, c["p"] * c["p"]), Hpl=s.values(capi.HPL).reshape(-1, c["p"] * c["l"]),
               Hll=s.values(capi.HLL).reshape(-1, c["l"] * c["l"]))
    for w in ("pp", "pl", "hs"):
        assert np.array_equal(got[w][0], a[w][0]) and np.array_equal(got[w][1], a[w][1]), w
    for w in ("Hpp", "Hpl", "Hll", "b"):
        assert np.array_equal(got[w], a[w]), w + " is not the exact assembly bit for bit"
    assert H.assembled_hash(got) == k["assembled_sha"]
    st = s.stats()
    assert st["hessianPoseDimension"] == c["nP"] * c["p"] and st["hessianLandmarkDimension"] == c["nL"] * c["l"], st


def _symmetric_diagonal(k, Hs):
    cp, ri = k["a"]["hs"][0], k["a"]["hs"][1]
    diag = [q for col in range(k["c"]["nP"]) for q in range(cp[col], cp[col + 1]) if ri[q] == col]
    assert len(diag) == k["c"]["nP"]
    bad = [q for q in diag if not np.array_equal(Hs[q], Hs[q].T)]
    assert not bad, ("diagonal blocks of Hschur that are not symmetric", bad[:8])


@pytest.mark.parametrize("name", NAMES)
def test_schur_stage_on_pinned_inputs(name):
    capi = _capi()
    k = H.load_case(name)
    c, a = k["c"], k["a"]
    p, l, nP, nL = c["p"], c["l"], c["nP"], c["nL"]
    cen = H.census_of(c, a)
    H.assert_census(name, c, cen)
    failures = []
    # ---- split interface, the reduction un-folded
    s = H.device_solver(capi, c, {"fuse_schur_reduce": 0})
    _assert_assembly(capi, s, k)
    s.setLambda(c["lam"], True)
    s.solveSchur()
    Hs = H.hschur_blocks(s.values(capi.HSCHUR), p)
    _hold(k, cen, "split", "Dinv", s.values(capi.DINV).reshape(nL, l, l).transpose(0, 2, 1), failures=failures)
    _hold(k, cen, "split", "Hschur", Hs, failures=failures)
    _hold(k, cen, "split", "bschur", _device_copy(s, capi.ARR_BSCHUR)[:nP * p].reshape(nP, p), failures=failures)
    _symmetric_diagonal(k, Hs)
    s.setX(np.concatenate([c["xp"], np.zeros(nL * l)]))
    s.solveBackSubstitute()
    x = s.x()
    assert np.array_equal(x[:nP * p], c["xp"])                    # the pinned poses are what the kernel read
    _hold(k, cen, "split", "xl", x[nP * p:].reshape(nL, l), failures=failures)
    # ---- landmark_inverse_kernel: only the matrix-free operator's preparation launches it
    if (p, l) in OPERATOR_DIMS:
        s.schurOperatorPrepare()
        _hold(k, cen, "operator", "Dinv", s.values(capi.DINV).reshape(nL, l, l).transpose(0, 2, 1), failures=failures)
        _hold(k, cen, "operator", "bschur", _device_copy(s, capi.ARR_BSCHUR)[:nP * p].reshape(nP, p), failures=failures)
    # ---- solve() at defaults: the reduction folded into the factorisation, bschur by schur_rhs_kernel
    if nP <= H.FULL_SOLVE_MAX_POSES:
        assert cen["n_td"] <= FUSE_REDUCE_MAX_PARTIALS * len(a["hs"][1])
        s2 = H.device_solver(capi, c)
        s2.setLambda(c["lam"], True)
        assert s2.solve() is True
        _hold(k, cen, "solve", "bschur", _device_copy(s2, capi.ARR_BSCHUR)[:nP * p].reshape(nP, p), failures=failures)
        x2 = s2.x()
        _hold(k, cen, "solve", "xp", x2[:nP * p].reshape(nP, p), "xp_solved", failures=failures)
        _hold(k, cen, "solve", "xl", x2[nP * p:].reshape(nL, l), "xl_solved", failures=failures)
        Hs2 = H.hschur_blocks(s2.values(capi.HSCHUR), p)         # ensure_hschur: the reduction after the fact
        _hold(k, cen, "solve", "Hschur", Hs2, failures=failures)
        _symmetric_diagonal(k, Hs2)
    assert not failures, failures


@pytest.mark.parametrize("fuse_landmarks", [1, 0])
@pytest.mark.parametrize("name", H.FUSED_CASES)
def test_fused_ba_schur_stage(name, fuse_landmarks):
    """The fused BA tiles and both BA back-substitution kernels from the estimates (the reference chains projection, robust
    weight, products and Schur complement at 60 digits; the scales carry the operand sums of the assembled terms)."""
    from openslam_g2o_amd import lm
    capi = _capi()
    k = H.load_fused_case(name)
    c, st = k["c"], k["st"]
    nP, nL = c["nP"], c["nL"]
    assert H.fused_input_hash(c) == k["input_sha"]
    cen = H.census_of(dict(c, lam=0.0), st)
    assert cen["G"] == (8 if name == "ba_chain" else 4) and cen["n_tiles"] >= 2
    s = H.device_fused(capi, lm, c, {"ba_fused": 1, "ba_fuse_landmarks": fuse_landmarks, "fuse_schur_reduce": 0})
    for w, which in (("pl", capi.HPL), ("hs", capi.HSCHUR)):
        cp, ri = s.pattern(which)
        assert np.array_equal(cp, st[w][0]) and np.array_equal(ri, st[w][1]), w
    failures = []
    for i, lam in enumerate(H.FUSED_LAMBDAS):
        path = "fused_ll%d_%s" % (fuse_landmarks, "FLL" if (fuse_landmarks and i == 0) else "noFLL")
        if i > 0:
            s.restoreDiagonal()
            assert s.maxDiagonal() > 0.0                            # a reader of Hll: the next tiles find it in memory
        s.setLambda(lam, True)
        s.solveSchur()
        Hs = H.hschur_blocks(s.values(capi.HSCHUR), 6)
        _hold(k, cen, path, "Dinv", s.values(capi.DINV).reshape(nL, 3, 3).transpose(0, 2, 1), "Dinv@%d" % i, failures)
        _hold(k, cen, path, "Hschur", Hs, "Hschur@%d" % i, failures)
        _hold(k, cen, path, "bschur", _device_copy(s, capi.ARR_BSCHUR)[:nP * 6].reshape(nP, 6), "bschur@%d" % i, failures)
        _symmetric_diagonal(dict(a=st, c=c), Hs)
        s.setX(np.concatenate([c["xp"], np.zeros(nL * 3)]))
        s.solveBackSubstitute()
        x = s.x()
        assert np.array_equal(x[:nP * 6], c["xp"])
        _hold(k, cen, path, "xl", x[nP * 6:].reshape(nL, 3), "xl@%d" % i, failures)
    assert not failures, failures
