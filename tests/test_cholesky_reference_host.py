"""The sparse-Cholesky solve fixture on the CPU (tests/golden/cholesky_solve.npz, tests/cholesky_helpers.py): the rebuilt
matrices are the generator's, the stored reference carries its certificate, the two reference methods agree, fp64 on the CPU
stays within the margin the device is held to, the measure is invariant under D A D, and four wrong results that the check this
replaces -- one global relerr < 1e-10 against an fp64 solve -- lets through fail the per-block measure."""
import numpy as np
import pytest

from tests import cholesky_helpers as H

OLD_TOLERANCE = 1e-10


@pytest.mark.parametrize("case,bs", H.PARAMS)
def test_rebuilt_matrix_and_right_hand_sides_are_the_generators(case, bs):
    c = H.load_case(case, bs)
    assert c["sha"] == c["stored_sha"]
    assert int(H.fixture()[H.key(case, bs) + "/nb"]) == c["nb"]
    for rhs in H.RHS:
        b = c[rhs]["b"]
        assert np.array_equal(b * 8.0, np.round(b * 8.0))
        assert len(c[rhs]["hi"]) == c["n"] and len(c[rhs]["s"]) == c["nb"]
    imp = c["impulse"]["b"].reshape(c["nb"], bs)
    assert np.all(imp[0] != 0) and np.all(imp[-1] != 0) and not imp[1:-1].any()


@pytest.mark.parametrize("case,bs", H.PARAMS)
def test_stored_reference_carries_its_certificate(case, bs):
    """|b - A xref| <= 2^-120 (|A| |xref| + |b|) componentwise for xref = hi + lo + lo2, in exact integer arithmetic; the three
    terms do not overlap (hi = fl(xref), lo = fl(xref - hi))."""
    c = H.load_case(case, bs)
    for rhs in H.RHS:
        r = c[rhs]
        assert H.certificate(c, r["hi"], r["lo"], r["lo2"], r["b"]), rhs
        assert np.array_equal(r["hi"] + r["lo"], r["hi"]) and np.array_equal(r["lo"] + r["lo2"], r["lo"])
        assert np.all(r["s"] > 0)


def test_a_perturbed_reference_misses_the_certificate():
    """The certificate is no formality: one component moved by 2^-100 of itself fails it."""
    c = H.load_case("grid", 3)
    r = c["dense"]
    lo2 = r["lo2"].copy()
    lo2[17] += r["hi"][17] * 2.0 ** -100
    assert not H.certificate(c, r["hi"], r["lo"], lo2, r["b"])


def test_refinement_and_direct_60_digit_solve_agree():
    """band, block size 6: iterative refinement with exact residuals against the dense 60-digit Cholesky of
    make_inverse_blocks.cholesky_rows, to 2^-100 s per block (two methods with no code in common)."""
    c = H.load_case("band", 6)
    for rhs in H.RHS:
        r = c[rhs]
        diff = (r["hi"] - r["dir_hi"]) + ((r["lo"] - r["dir_lo"]) + r["lo2"])
        worst = (H.block_max(diff, 6) / r["s"]).max()
        print("CHOLSOLVE_REF", rhs, "refinement - direct: %.3g s (2^%.1f)" % (worst, np.log2(max(worst, 1e-300))))
        assert worst <= 2.0 ** -100


@pytest.mark.parametrize("case,bs", H.PARAMS)
def test_fp64_on_the_cpu_against_the_reference(case, bs):
    """SciPy's Cholesky with two triangular solves and the oracle, recomputed here: both within the margin the device is held
    to (8 x the larger stored figure; another BLAS sums in another order), and the reference's rounding to fp64 lies below one
    unit of the measure."""
    c = H.load_case(case, bs)
    A = H.dense(c)
    for rhs in H.RHS:
        r = c[rhs]
        fs = H.ratios(H.scipy_cholesky_solve(A, r["b"]), c, rhs).max()
        fo = H.ratios(H.oracle_solve(c, r["b"]), c, rhs).max()
        print("CHOLSOLVE_CPU", case, bs, rhs, "scipy %.3g (stored %.3g) oracle %.3g (stored %.3g)" % (fs, r["cpu_scipy"], fo, r["cpu_oracle"]))
        assert 0 < fs <= r["bound"] and 0 < fo <= r["bound"]
        assert r["cpu_oracle"] / 8 <= fo <= 8 * r["cpu_oracle"]
        assert np.all(H.block_max(r["hi"], bs) <= r["s"])
        assert H.relerr_old(H.scipy_cholesky_solve(A, r["b"]), r["hi"]) < OLD_TOLERANCE


def test_graded_figures_equal_the_ungraded_ones():
    """The invariance the measure was chosen for.  The scales and the reference of band_graded are those of band scaled by D
    (exactly, for the impulse: D^-1 b is b / 2^10 there; the dense right-hand sides are the same numbers, hence different vectors in
    band's coordinates).  The CPU figures the bound is taken from agree within a factor 2, bit for bit for the impulse;
    under |Z| |A| |x| on its own fp64 inverse the graded matrix (condition ~1e17) has no usable figure at all."""
    a, g = H.load_case("band", 6), H.load_case("band_graded", 6)
    D = H.graded_scale(a["nb"])
    assert np.array_equal(g["impulse"]["s"] * D * 2.0 ** H.GRADE, a["impulse"]["s"])
    assert np.array_equal(g["impulse"]["hi"] * np.repeat(D, 6) * 2.0 ** H.GRADE, a["impulse"]["hi"])
    for name in ("cpu_scipy", "cpu_oracle"):
        assert g["impulse"][name] == a["impulse"][name]
    for rhs in H.RHS:
        fa = max(a[rhs]["cpu_scipy"], a[rhs]["cpu_oracle"])
        fg = max(g[rhs]["cpu_scipy"], g[rhs]["cpu_oracle"])
        assert 0.5 <= fg / fa <= 2.0, (rhs, fa, fg)
    tail = H.block_max(g["dense"]["hi"], 6)
    assert tail.min() < 1e-5 * tail.max()                        # (the graded solution spans 2^-20 between neighbouring blocks)


# ================================================================================================ seeded faults
def _old_passes_new_fails(c, rhs, x):
    r = c[rhs]
    x64 = np.linalg.solve(H.dense(c), r["b"])
    old = H.relerr_old(x, x64)
    new = H.ratios(x, c, rhs).max()
    print("CHOLSOLVE_FAULT", c["case"], c["bs"], rhs, "old relerr %.3g, new figure %.3g (bound %.3g)" % (old, new, r["bound"]))
    assert old < OLD_TOLERANCE, "the old check was expected to let this through"
    assert new > r["bound"]


def _tail_block(c, rhs, level):
    """The block (not the first or last) whose largest entry is nearest to `level` times the largest entry of the solution."""
    tail = H.block_max(c[rhs]["hi"], c["bs"])
    return 1 + int(np.argmin(np.abs(np.log10(tail[1:-1] / tail.max()) - np.log10(level))))


@pytest.mark.parametrize("bs", H.CASES["decay"])
def test_zeroed_block_of_the_factor_passes_the_old_check_and_fails_the_new(bs):
    """decay, impulse: x from a dense factor whose off-diagonal block (i, i - 1) is zero, where the solution has decayed to 1e-12
    of its largest entry.  (The one-prior Laplacians have no such tail -- a harmonic function on a chain does not decay --, which
    is why the fixture has this case.)"""
    import scipy.linalg as sl
    c = H.load_case("decay", bs)
    i = _tail_block(c, "impulse", 1e-12)
    L = np.linalg.cholesky(H.dense(c))
    assert np.abs(L[bs * i:bs * (i + 1), bs * (i - 1):bs * i]).max() > 0.05 * np.abs(L[bs * i:bs * (i + 1), bs * i:bs * (i + 1)]).max()
    L[bs * i:bs * (i + 1), bs * (i - 1):bs * i] = 0.0
    b = c["impulse"]["b"]
    x = sl.solve_triangular(L, sl.solve_triangular(L, b, lower=True), lower=True, trans="T")
    _old_passes_new_fails(c, "impulse", x)


@pytest.mark.parametrize("bs", H.CASES["decay"])
def test_decayed_tail_returned_as_zero_passes_the_old_check_and_fails_the_new(bs):
    c = H.load_case("decay", bs)
    x = c["impulse"]["hi"].copy().reshape(c["nb"], bs)
    tail = H.block_max(c["impulse"]["hi"], bs)
    sel = tail < OLD_TOLERANCE * tail.max()
    assert 4 <= sel.sum() < c["nb"]
    x[sel] = 0.0
    _old_passes_new_fails(c, "impulse", x.reshape(-1))


@pytest.mark.parametrize("bs", H.CASES["decay"])
def test_two_exchanged_tail_blocks_pass_the_old_check_and_fail_the_new(bs):
    c = H.load_case("decay", bs)
    i = _tail_block(c, "impulse", 1e-12)
    x = c["impulse"]["hi"].copy().reshape(c["nb"], bs)
    x[[i, i + 1]] = x[[i + 1, i]]
    _old_passes_new_fails(c, "impulse", x.reshape(-1))


@pytest.mark.parametrize("rhs", H.RHS)
def test_relative_error_on_the_smallest_block_passes_the_old_check_and_fails_the_new(rhs):
    """band_graded: 1e-9 relative error on the block of the smallest scale."""
    c = H.load_case("band_graded", 6)
    r = c[rhs]
    i = int(np.argmin(r["s"]))
    x = r["hi"].copy()
    x[6 * i:6 * (i + 1)] *= 1.0 + 1e-9
    old = H.relerr_old(x, r["hi"])
    new = H.ratios(x, c, rhs).max()
    print("CHOLSOLVE_FAULT band_graded 6", rhs, "old relerr %.3g, new figure %.3g (bound %.3g)" % (old, new, r["bound"]))
    assert old < OLD_TOLERANCE and new > r["bound"]
