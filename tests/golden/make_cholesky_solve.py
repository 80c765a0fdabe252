"""Writes tests/golden/cholesky_solve.npz: the solution x = A^-1 b of the matrices and right-hand sides of
tests/cholesky_helpers.py to more than 120 bits, the per-block scales of the measure and what fp64 on the CPU attains under it.
Run offline (python -m tests.golden.make_cholesky_solve, a few minutes on 16 cores); no test imports this file.  The archive
has fixed member dates and the BLAS runs on one thread, so a second run reproduces it byte for byte.

Per case and block size, under the key prefix "<case>_b<bs>/":
  nb, sha                       blocks; SHA-256 of the rebuilt matrix and right-hand sides (the matrix itself is not stored)
and per right-hand side, under "<case>_b<bs>/<rhs>/":
  hi, lo, lo2 [n]               xref = hi + lo + lo2 exactly; hi = fl(xref), lo = fl(xref - hi); lo2 in fp32 where the certificate
                                holds with it (everywhere but the decayed components of `decay`), in fp64 otherwise
  s, sa [nb]                    per block max of |Z| d (d' |xref|) (the measure) and of |Z| |A| |xref| (for information)
  cpu_scipy, cpu_oracle         worst err_i (units of u s_i) of SciPy's Cholesky + two triangular solves and of the oracle
  cpu_scipy_sa, cpu_oracle_sa   the same under sa
  dir_hi, dir_lo [n]            band, block size 6: the direct 60-digit solve (cholesky_rows of make_inverse_blocks.py)

The reference is iterative refinement: xref = x0 + x1 + ..., every term an fp64 Cholesky solve of the exactly evaluated
residual (integer arithmetic: all inputs are dyadic), at least four terms and until the residual is below 2^-160; the sum is
then cut to three fp64 numbers per component and stored only if the certificate of tests/cholesky_helpers.py holds for exactly
what is stored.  band_graded is refined in the coordinates of band (D is a power of two)."""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"

import io                    # noqa: E402
import json                  # noqa: E402
import multiprocessing       # noqa: E402
import sys                   # noqa: E402
import zipfile               # noqa: E402

import numpy as np           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import cholesky_helpers as H      # noqa: E402

REFINE_BITS = 160
MAX_TERMS = 8


def refine(EM, cho, b):
    """(hi, lo, lo2, terms used) for the matrix behind EM / cho and right-hand side b."""
    import scipy.linalg as sl
    terms = [sl.cho_solve(cho, b)]
    while True:
        X, e = H.sum_int(terms)
        R, T, er = EM.residual(X, e, b)
        if len(terms) >= 4 and H.certified(R, T, REFINE_BITS):
            break
        assert len(terms) < MAX_TERMS, "the refinement does not converge"
        terms.append(sl.cho_solve(cho, H.from_int(R, er)))
    hi, lo, lo2 = H.triple_of(X, e)
    for third in (lo2.astype(np.float32), lo2):                  # the third term in fp32 where that keeps the certificate (the archive's size)
        X3, e3 = H.sum_int([hi, lo, third.astype(np.float64)])
        R, T, _ = EM.residual(X3, e3, b)
        if H.certified(R, T):
            return hi, lo, third, len(terms)
    raise AssertionError("the stored reference misses its certificate")


def direct_solve(m, b):
    """(hi, lo) of the 60-digit solve by the dense up-looking Cholesky of make_inverse_blocks.py."""
    import mpmath as mp
    from tests.golden import make_inverse_blocks as MI
    mpf = mp.mpf
    A = H.dense(m)
    n = m["n"]
    low = [{int(j): mpf(float(A[i, j])) for j in np.flatnonzero(A[i, :i + 1])} for i in range(n)]
    L = MI.cholesky_rows(low, n)
    y = [None] * n
    for i in range(n):
        v = mpf(float(b[i]))
        for j, lij in L[i].items():
            if j != i:
                v -= lij * y[j]
        y[i] = v / L[i][i]
    cols = [dict() for _ in range(n)]
    for i in range(n):
        for j, v in L[i].items():
            if j != i:
                cols[j][i] = v
    x = [None] * n
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k, lki in cols[i].items():
            v -= lki * x[k]
        x[i] = v / L[i][i]
    hi = np.array([float(v) for v in x])
    lo = np.array([float(v - mpf(float(h))) for v, h in zip(x, hi)])
    return hi, lo


def reference(job):
    import scipy.linalg as sl
    case, bs = job
    m = H.matrix(case, bs)
    m0, D = H.unscaled(m)
    A0 = H.dense(m0)
    EM = H.ExactMatrix(A0)
    cho = sl.cho_factor(A0, lower=True)
    Z0 = sl.cho_solve(cho, np.eye(m["n"]))
    Ag = H.dense(m)
    out = dict(nb=np.int32(m["nb"]), sha=np.array(m["sha"]))
    recs = []
    cond = float(np.abs(A0).sum(axis=0).max() * np.abs(Z0).sum(axis=0).max())
    for rhs in H.RHS:
        b = m["b"][rhs]
        hi, lo, lo2, nterms = refine(EM, cho, b if D is None else b / D)
        s, sa = H.scales(A0, Z0, hi, bs)
        if D is not None:                                        # x = D^-1 y, and both scales change as x does
            hi, lo, lo2 = hi / D, lo / D, (lo2 / D).astype(lo2.dtype)
            s, sa = s / D[::bs], sa / D[::bs]
        r = dict(hi=hi, lo=lo, lo2=lo2, s=s, sa=sa)
        c = dict(bs=bs)
        c[rhs] = r
        xs, xo = H.scipy_cholesky_solve(Ag, b), H.oracle_solve(m, b)
        for name, x in (("cpu_scipy", xs), ("cpu_oracle", xo)):
            r[name] = np.float64(H.ratios(x, c, rhs).max())
            r[name + "_sa"] = np.float64(H.ratios(x, c, rhs, "sa").max())
        if case == "band" and bs == 6:
            r["dir_hi"], r["dir_lo"] = direct_solve(m, b)
        for name, v in r.items():
            out[rhs + "/" + name] = v
        tail = np.abs(hi).reshape(-1, bs).max(axis=1)
        recs.append(dict(path="cpu", case=case, bs=bs, rhs=rhs, n=m["n"], cond1=cond, terms=nterms,
                         cpu_scipy=float(r["cpu_scipy"]), cpu_oracle=float(r["cpu_oracle"]), cpu_scipy_sa=float(r["cpu_scipy_sa"]),
                         cpu_oracle_sa=float(r["cpu_oracle_sa"]), smallest_block_over_max=float(tail.min() / tail.max()),
                         old_relerr_scipy=float(H.relerr_old(xs, hi))))
    return H.key(case, bs), out, recs


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates (byte-stable)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    jobs = sorted(H.PARAMS, key=lambda j: (j != ("band", 6), -H.matrix(*j)["n"]))          # the 60-digit solve first, then by size
    with multiprocessing.Pool(min(16, os.cpu_count() or 1, len(jobs))) as pool:
        results = pool.map(reference, jobs, chunksize=1)
    arrays, recs = {}, []
    for k, out, rec in sorted(results, key=lambda r: r[0]):
        for name, v in out.items():
            arrays[k + "/" + name] = v
        recs += rec
    for rec in recs:
        print(json.dumps(rec))
    write_npz(H.FIXTURE, arrays)
    print("wrote", H.FIXTURE, os.path.getsize(H.FIXTURE), "bytes")
    assert os.path.getsize(H.FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "schur_blocks.npz"))
    # profiles/cholesky_solve.jsonl: the CPU rows are rewritten, the device rows (the CHOLSOLVE lines of tests/test_gpu_cholesky_solve.py) kept
    prof = os.path.join(ROOT, "profiles", "cholesky_solve.jsonl")
    kept = []
    if os.path.exists(prof):
        with open(prof) as f:
            kept = [line for line in f if line.strip() and json.loads(line).get("path") != "cpu"]
    with open(prof, "w") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")
        f.writelines(kept)


if __name__ == "__main__":
    main()
