"""CPU: the fixture tests/golden/pcg_steps.npz against its own source and against the oracle.

  * the extended-precision PCG (tests/pcg_helpers.py) run to convergence equals the extended-precision direct solve, on the
    pose system and on the reduced system against the full one;
  * the oracle's fp64 PCG stays inside the figures the generator stored, and those stay a factor 8 below 1e-12;
  * the coverage record of the fixture lists every block-row count, block size and scenario;
  * the generator reproduces the committed fixture array for array."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import pcg_helpers as H
from tests import producer_metric as PM
from tests.golden import make_pcg_steps as G

mp = H.mp
FX = dict(np.load(G.OUT))


def _ints(blk):
    return [[[int(v) for v in r] for r in B] for B in blk]


def test_mp_pcg_run_to_convergence_is_the_mp_direct_solve():
    for bs, nb in ((3, 12), (7, 1), (6, 5)):
        inp = H.chain_inputs(100 + nb, nb, bs)
        blocks, b = H.chain_system(inp, nb, bs)
        cp, row, blk = H.blocks_to_ccs(nb, blocks)
        r = H.PcgMp(nb, bs, cp, row, _ints(blk), b).run(tolerance=1e-100, absolute=False, max_iter=200)
        xd = H.direct_solve_mp(nb, bs, cp, row, _ints(blk), b)
        assert max(abs(a - c) for a, c in zip(r["x_last"], xd)) < mp.mpf("1e-40") * max(abs(c) for c in xd)
        assert r["iterations"] == H.stop_iteration(r["dn"], r["d0"]) and r["residual"] == r["dn"][-1] / 2
        # the carried residual is the stopping level of an absolute-tolerance solve, and only of such a solve
        lvl = r["dn"][2] * mp.mpf("1.5") if nb > 1 else None
        if lvl is not None:
            s = H.PcgMp(nb, bs, cp, row, _ints(blk), b)
            assert s.run(tolerance=1e-100, absolute=True, residual=lvl)["iterations"] == 2
            assert s.run(tolerance=1e-100, absolute=False, residual=lvl, max_iter=7)["iterations"] == 7
    # reduced operator: the PCG on S solves the pose part of the full system
    p, l, nP, nL = 3, 2, 16, 24
    inp = H.reduced_inputs(7, p, l, nP, nL)
    pp, obs, Hll, b = H.reduced_system(inp, p, l, nP, nL)
    S, bs_ = H.reduced_operator_mp(nP, p, l, pp, obs, Hll, H.LAMBDA, b)
    cp, row, blk = H.blocks_to_ccs(nP, S)
    r = H.PcgMp(nP, p, cp, row, blk, bs_).run(tolerance=1e-100, absolute=False, max_iter=300)
    n = nP * p + nL * l
    A = mp.matrix(n, n)
    for i in range(n):
        e = np.zeros(n, np.int64)
        e[i] = 1
        colv = H.full_product(pp, obs, Hll, p, l, nP, nL, H.LAMBDA, e)
        for j in range(n):
            A[j, i] = mp.mpf(int(colv[j]))
    xd = mp.lu_solve(A, mp.matrix([mp.mpf(int(v)) for v in b]))
    assert max(abs(r["x_last"][i] - xd[i]) for i in range(nP * p)) < mp.mpf("1e-40") * max(abs(xd[i]) for i in range(nP * p))


def _oracle_chain(bs, nb):
    name = H.chain_case_name(bs, nb)
    inp = H.chain_inputs(int(FX[name + "_seed"]), nb, bs)
    blocks, b = H.chain_system(inp, nb, bs)
    cp, row, blk = H.blocks_to_ccs(nb, blocks)
    return name, cp, row, H.ccs_values(blk), b.astype(np.float64)


def _inside(key, fig):
    stored = float(FX["oracle_" + key])
    print("oracle", key, fig, "stored", stored)
    assert fig <= stored * (1 + 1e-9) and PM.MARGIN * fig <= PM.CEILING, (key, fig, stored)
    assert PM.bound(FX, key) <= PM.CEILING


def test_oracle_pcg_stays_inside_its_recorded_figures():
    for bs in sorted(H.CHAIN_BS):
        for nb in H.CHAIN_BS[bs]:
            name, cp, row, val, b = _oracle_chain(bs, nb)
            for k in H.STEPS:
                ok, x, it, _ = O.pcg_solve_blocks(nb, bs, cp, row, val, b, tolerance=1e-300, absolute=False, max_iter=k)
                assert ok
                _inside("%s_x%d" % (name, k), H.figure(x, FX["%s_x%d" % (name, k)]))
            # the oracle's stopping rule gives the stored counts: relative, and the carried residual from solve to solve
            want, res, floor = FX[name + "_it_carried"], -1.0, 0
            for j, (tol, absolute) in enumerate(((1e-6, False), (1e-20, True), (1e-20, True))):
                ok, x, it, res = O.pcg_solve_blocks(nb, bs, cp, row, val, b, tolerance=tol, absolute=absolute, residual=res)
                assert ok and (it == want[j] if want[j] >= 0 else it >= floor), (name, j, it, want)
                floor = it
            res, its = -1.0, []
            for j in range(3):
                ok, x, it, res = O.pcg_solve_blocks(nb, bs, cp, row, val, b, residual=res)
                its.append(it)
            assert its == FX[name + "_it_default"].tolist()
    for bs in sorted(H.CHAIN_BS):
        name = "diag_b%d" % bs
        inp = H.diag_inputs(int(FX[name + "_seed"]), bs)
        blocks, b = H.diag_system(inp, bs)
        cp, row, blk = H.blocks_to_ccs(len(inp["Ju"]), blocks)
        ok, x, it, _ = O.pcg_solve_blocks(len(inp["Ju"]), bs, cp, row, H.ccs_values(blk), b.astype(np.float64), tolerance=1e-6, absolute=False)
        assert ok and it == 1
        _inside(name + "_x", float(H.figure_per_block(x, FX[name + "_x"], bs).max()))


def test_coverage_of_the_fixture():
    cov = json.loads(str(FX["coverage_json"]))
    chains = {(c["bs"], c["nb"]) for c in cov["chain"]}
    assert chains >= {(bs, nb) for bs in (3, 6) for nb in (1, 255, 256, 257, 513)} | {(7, 1), (7, 257)}
    assert set(cov["scenarios"]) >= {"steps", "relative", "carried", "default"} and cov["steps"] == [1, 2, 3, 8]
    for c in cov["chain"]:
        if c["nb"] > 1:
            assert 0.05 * c["nb"] <= c["closures"] <= 0.15 * c["nb"]
            assert c["it_steps"] == [1, 2, 3, 8] and min(c["it_carried"]) > 8 and c["it_carried"][0] < c["it_carried"][2]
            assert c["it_loose"][1] < c["it_rel"]
        assert ("%s_x8" % c["case"]) in FX and ("oracle_%s_x8" % c["case"]) in FX
    assert {c["bs"] for c in cov["diag"]} == {3, 6, 7}
    for c in cov["diag"]:
        assert c["blocks"] == 300 and c["cond_min"] < 1.5 and c["cond_max"] >= 1e8
    assert {(c["p"], c["l"]) for c in cov["reduced"]} == {(3, 2), (6, 3), (7, 3)}
    for c in cov["reduced"]:
        assert c["poses"] == 257 and c["landmarks"] == 600 and c["obs_per_landmark"] == [2, 4] and len(c["blind_poses"]) == 2
        for key in ("Sdiag", "Sv", "bs", "x1", "x2", "x3"):
            assert float(FX["oracle_%s_%s" % (c["case"], key)]) > 0


def test_generator_reproduces_the_committed_fixture():
    fx, lines = G.generate()
    assert sorted(fx) == sorted(FX)
    for key in sorted(fx):
        assert np.array_equal(np.asarray(fx[key]), FX[key]), key
    stored = [json.loads(l) for l in open(G.PROFILE).read().splitlines() if l.strip()]
    assert [l for l in stored if l.get("who") == G.WHO] == lines
    # every dn of the fixture keeps its distance from every stopping level it is compared with (the margin of the exact counts)
    for c in json.loads(str(FX["coverage_json"]))["chain"]:
        dn = FX[c["case"] + "_dn"]
        levels = [1e-6 * dn[0]] + [0.5 * dn[k] for k in c["it_carried"][:2] if k >= 0 and c["nb"] > 1]
        for lvl in levels:
            assert np.all(np.abs(dn / lvl - 1) > G.THRESHOLD_MARGIN)
