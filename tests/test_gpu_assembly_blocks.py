"""The generic quadratic-form assembly (assemble_vertex_kernel, assemble_offdiag_kernel) and the scalars of the LM loop
(chi2_kernel, scale_partial_kernel, lambda_kernel, maxdiag_partial_kernel, gather_diag_kernel, the spmv kernels of
multiplyHessian) block by block against a 60-digit reference (tests/golden/assembly_blocks.npz, written by
tests/golden/make_assembly_blocks.py; inputs, census and measure in tests/assembly_helpers.py).  No reference is evaluated here:
the inputs are rebuilt from their seeds and every output is held to 8 x the larger of the two CPU figures the fixture records.
One line "ASMBLK {json}" per output is printed before it is held (the device rows of profiles/assembly_blocks.jsonl are these
lines from a pytest -s run).  Everything goes through capi.HipBlockSolver; the kernels a case reaches are the census' rows
(tests/test_assembly_reference_host.py holds them to the dispatch tables)."""
import json

import numpy as np
import pytest

from tests import assembly_helpers as H

pytestmark = pytest.mark.gpu

BLOCK_CASES = [n for n in H.NAMES if H.make_case(n)["kind"] in ("blocks", "single")]
CHI2_CASES = [n for n in H.NAMES if H.make_case(n)["kind"] == "chi2"]


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _hold(k, output, got, failures, build=1):
    f = H.figures(got, k["ref"][output], k["scale"][output])
    worst = int(np.argmax(f))
    print("ASMBLK " + json.dumps(dict(path="device", case=k["name"], output=output, build=build, device=float(f.max()), block=worst,
                                      bound=k["bound"][output], cpu_oracle=k["cpu"][output][0], cpu_numpy=k["cpu"][output][1])))
    if not f.max() <= k["bound"][output]:
        failures.append((k["name"], output, build, worst, float(f.max()), k["bound"][output]))


def _read(capi, s, c, st):
    for which, name in ((capi.HPP, "pp"),) + (((capi.HPL, "pl"),) if c["nL"] else ()):
        cp, ri = s.pattern(which)
        assert np.array_equal(cp, st[name][0]) and np.array_equal(ri, st[name][1]), name
    return H.device_outputs(c, st, s.values(capi.HPP), s.values(capi.HPL) if c["nL"] else None, s.values(capi.HLL) if c["nL"] else None,
                            s.b(), s.chi2())


@pytest.mark.parametrize("name", BLOCK_CASES)
def test_assembled_blocks_and_chi2(name):
    """Hpp, Hpl, Hll, b and chi2 after buildSystem, and again after a second buildSystem (the first set overwrites); blocks
    without a contributor stay zero (their scale is 0); robust_single: the weight read back from every diagonal and
    off-diagonal block; the Schur families: H x with and without virtual damping."""
    capi = _capi()
    k = H.load_case(name)
    c, st = k["c"], k["st"]
    s = H.device_solver(capi, c)
    failures = []
    for build in (1, 2):
        s.buildSystem()
        got = _read(capi, s, c, st)
        for o in ("Hpp", "Hpl", "Hll", "b", "chi2"):
            if o in k["ref"]:
                _hold(k, o, got[o], failures, build)
        if c["kind"] == "single":
            f = H.fixture()
            w = H.weights_from_blocks(c, st, got["Hpp"], f[name + "/single_idx"], f[name + "/single_M"])
            _hold(k, "w_diag", np.concatenate([w[0], w[2]]), failures, build)
            _hold(k, "w_off", w[1], failures, build)
    if name in H.HX_CASES:
        for i, lam in enumerate(c["lams"]):
            s.setLambdaSplit(lam[0], lam[1], False)
            _hold(k, "Hx%d" % i, H.split_b(c, s.multiplyHessian(c["x"])), failures)
        s.restoreDiagonal()
    s.close()
    assert not failures, failures


@pytest.mark.parametrize("name", CHI2_CASES)
def test_chi2_per_dimension_and_size(name):
    capi = _capi()
    k = H.load_case(name)
    s = H.device_solver(capi, k["c"])
    s.buildSystem()
    failures = []
    _hold(k, "chi2", [s.chi2()], failures)
    s.close()
    assert not failures, failures


def test_chi2_grid_stride_loop_is_exact():
    """n = 1024 * 256 + 257 edges of dimension 1 with dyadic errors: every partial sum is exact, the result the integer sum."""
    capi = _capi()
    c = H.make_case("chi2_exact")
    assert H.input_hash(c) == str(H.fixture()["chi2_exact/input_sha"])
    s = H.device_solver(capi, c)
    s.buildSystem()
    got = s.chi2()
    s.close()
    assert got == float(H.fixture()["chi2_exact/exact_chi2"])


@pytest.mark.parametrize("size", H.SCALE_SIZES)
def test_compute_scale(size):
    capi = _capi()
    k = H.load_case("scale_n%d" % size)
    c = k["c"]
    s = H.device_solver(capi, c)
    s.buildSystem()
    assert s.vectorSize() == size and np.array_equal(s.b(), c["b_exact"])
    s.setX(c["x"])
    failures = []
    _hold(k, "scale", [s.computeScale(c["lam"])], failures)
    s.close()
    assert not failures, failures


def _diag_index(c, st):
    """Positions of the scalar diagonal in values(HPP) and values(HLL)."""
    p, l = c["p"], c["l"]
    ip = np.array([st["pp"][2][(v, v)] * p * p + j * (p + 1) for v in range(c["nP"]) for j in range(p)])
    il = np.array([v * l * l + j * (l + 1) for v in range(c["nL"]) for j in range(l)], dtype=np.int64)
    return ip, il


@pytest.mark.parametrize("name", ("fam_3_3", "fam_3_2", "g4_p6"))
def test_damping_is_exact_on_a_structure_without_schur(name):
    """setLambda / setLambdaSplit / restoreDiagonal on a structure built schur=False (lambda_kernel on Hpp through diag_blk and on
    Hll without it): fl(d + lambda) on the diagonal, every other entry and the restored matrix bit for bit; maxDiagonal and
    diagonal are the max and the gather of the device's own values."""
    capi = _capi()
    c = H.make_case(name)
    st = H.structure(c)
    s = H.device_solver(capi, c, schur=False)
    s.buildSystem()
    ip, il = _diag_index(c, st)
    read = lambda: (s.values(capi.HPP).copy(), s.values(capi.HLL).copy() if c["nL"] else np.zeros(0))
    P0, L0 = read()
    diag0 = np.concatenate([P0[ip], L0[il]])
    assert np.array_equal(s.diagonal(), diag0) and s.maxDiagonal() == np.abs(diag0).max()
    lam1, lam2, lam3 = 0.1 * np.abs(diag0).max(), 3.7e-5, 1.9
    s.setLambda(lam1, True)
    P1, L1 = read()
    EP, EL = P0.copy(), L0.copy()
    EP[ip] = P0[ip] + lam1
    EL[il] = L0[il] + lam1
    assert np.array_equal(P1, EP) and np.array_equal(L1, EL)
    assert np.array_equal(s.diagonal(), np.concatenate([EP[ip], EL[il]])) and s.maxDiagonal() == np.abs(np.concatenate([EP[ip], EL[il]])).max()
    s.restoreDiagonal()
    P, L = read()
    assert np.array_equal(P, P0) and np.array_equal(L, L0)
    # two dampings in a row as the LM loop does them: the first with a backup, the second on top of it without
    s.setLambda(lam2, True)
    s.setLambda(lam3, False)
    P2, L2 = read()
    EP[ip] = (P0[ip] + lam2) + lam3
    EL[il] = (L0[il] + lam2) + lam3
    assert np.array_equal(P2, EP) and np.array_equal(L2, EL)
    s.restoreDiagonal()
    P, L = read()
    assert np.array_equal(P, P0) and np.array_equal(L, L0)
    s.setLambdaSplit(lam2, lam3, True)
    P3, L3 = read()
    EP[ip] = P0[ip] + lam2
    EL[il] = L0[il] + lam3
    assert np.array_equal(P3, EP) and np.array_equal(L3, EL)
    s.restoreDiagonal()
    P, L = read()
    assert np.array_equal(P, P0) and np.array_equal(L, L0)
    s.close()


@pytest.mark.parametrize("name", ("fam_6_3", "fam_3_2"))
def test_virtual_damping_on_a_schur_structure(name):
    """Schur: Hpp and Hll stay untouched, maxDiagonal and diagonal add the virtual lambda with one rounding."""
    capi = _capi()
    c = H.make_case(name)
    st = H.structure(c)
    s = H.device_solver(capi, c)
    s.buildSystem()
    ip, il = _diag_index(c, st)
    P0, L0 = s.values(capi.HPP).copy(), s.values(capi.HLL).copy()
    lp, ll = c["lams"][1]
    s.setLambdaSplit(lp, ll, True)
    want = np.concatenate([P0[ip] + lp, L0[il] + ll])
    assert np.array_equal(s.diagonal(), want)
    assert s.maxDiagonal() == max((np.abs(P0[ip]) + lp).max(), (np.abs(L0[il]) + ll).max())
    s.restoreDiagonal()
    assert np.array_equal(s.values(capi.HPP), P0) and np.array_equal(s.values(capi.HLL), L0)
    assert np.array_equal(s.diagonal(), np.concatenate([P0[ip], L0[il]]))
    s.close()
