"""Writes tests/golden/inverse_blocks.npz: blocks of A^-1 at 60 digits (mpmath, as tests/reference_mp.py) for the matrices of
tests/inverse_helpers.py, the per-block scales of the measure, and what plain fp64 on the CPU attains under it.  Run offline
(python -m tests.golden.make_inverse_blocks, a few minutes on 8 cores); no test imports this file.

Per case and block size, under the key prefix "<case>_b<bs>/":
  nb, cp, ri, vals      the matrix, upper block CCS with column-major blocks (as g2ohip_ls_solve_pattern takes it)
  vi vj a0 J1 W ui ua UW the generic edges that assemble to it exactly (tests/inverse_helpers.py)
  pairs [np][2]         the stored pairs (r <= c): the matrix's pattern, then the far-apart pairs; the tests request both
                        orientations (inverse_helpers.requests)
  Z [np][bs][bs]        the reference blocks, rounded once to fp64
  s [np]                max entry of block (r, c) of |Z| |A| |Z|, evaluated at 60 digits
  cpu_numpy, cpu_oracle worst err_i (units of u s_i) of NumPy's Cholesky + triangular solves and of the oracle's column solves

The reference is a dense Cholesky factorisation in the natural order that skips structural zeros, then one pair of triangular
solves per column; it shares no code with sparse_cholesky.hip or oracle/g2o_oracle.c.  The generator checks at 60 digits that
the fp64 assembly of every matrix is exact and that A Z = I to 1e-50."""
import json
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import inverse_helpers as H      # noqa: E402

mp.mp.dps = 60
mpf = mp.mpf
ZERO = mpf(0)


def assemble_mp(E):
    """The edges of inverse_helpers.assemble in mpmath (fp64 inputs are exact mpf values)."""
    bs, nb = E["bs"], E["nb"]
    conv = lambda B: mp.matrix([[mpf(float(v)) for v in row] for row in B])
    blocks = {(i, i): mp.zeros(bs, bs) for i in range(nb)}
    for k in range(len(E["vi"])):
        i, j = int(E["vi"][k]), int(E["vj"][k])
        a, J1, W = mpf(float(E["a0"][k])), conv(E["J1"][k]), conv(E["W"][k])
        blocks[(i, i)] += a * a * W
        blocks[(j, j)] += J1.T * W * J1
        blocks[(i, j)] = blocks.get((i, j), mp.zeros(bs, bs)) + a * (W * J1)
    for k in range(len(E["ui"])):
        i = int(E["ui"][k])
        blocks[(i, i)] += mpf(float(E["ua"][k])) ** 2 * conv(E["UW"][k])
    return blocks


def cholesky_rows(A, n):
    """Up-looking Cholesky: A as rows {column <= row: value}; returns L as rows {column: value} with structural zeros skipped.
    Row i solves L[:i, :i] x = a_i by column-oriented forward substitution over the columns built so far."""
    rows = [None] * n
    cols = [dict() for _ in range(n)]                            # column j of L below the diagonal: {row: value}
    for i in range(n):
        w = [ZERO] * (i + 1)
        for j, v in A[i].items():
            w[j] = v
        row = {}
        d = w[i]
        for j in range(i):
            if not w[j]:
                continue
            x = w[j] / rows[j][j]
            row[j] = x
            d -= x * x
            for k, lkj in cols[j].items():
                if k < i:
                    w[k] -= lkj * x
        assert d > 0, "not positive definite"
        row[i] = mp.sqrt(d)
        rows[i] = row
        for j, x in row.items():
            if j != i:
                cols[j][i] = x
    return rows


def reference(case, bs):
    E = H.make_edges(case, bs)
    nb, n = E["nb"], E["nb"] * bs
    blocks = H.assemble(E)
    bm = assemble_mp(E)
    for k, B in blocks.items():                                  # the fp64 assembly is exact
        for r in range(bs):
            for c in range(bs):
                assert mpf(float(B[r, c])) == bm[k][r, c], (case, bs, k)
    pairs = H.unique_pairs(case, bs, nb, blocks)
    key, out, rec = reference_of_blocks(case, bs, nb, blocks, pairs)
    for name in ("vi", "vj", "a0", "J1", "W", "ui", "ua", "UW"):
        out[name] = E[name]
    return key, out, rec


def legacy_reference(bs):
    """The unrounded block-tridiagonal matrix of test_inverse_blocks_inside_and_outside_the_pattern_on_both_seams
    (tests/test_gpu_marginals.py) with that test's requests: only the CPU figures are kept (key legacy_tridiag_b<bs>)."""
    A, pairs = H.legacy_tridiagonal(bs)
    nb = H.CHAIN_NB
    blocks = {(r, c): A[bs * r:bs * (r + 1), bs * c:bs * (c + 1)] for c in range(nb) for r in ([c - 1, c] if c else [c])}
    key, out, rec = reference_of_blocks("legacy_tridiag", bs, nb, blocks, [(min(p), max(p)) for p in dict.fromkeys(map(tuple, map(sorted, pairs)))])
    return key, dict(cpu_numpy=out["cpu_numpy"], cpu_oracle=out["cpu_oracle"]), rec


def reference_of_blocks(case, bs, nb, blocks, pairs):
    n = nb * bs
    cp, ri, vals = H.to_ccs(nb, blocks)
    # scalar rows of the lower triangle {col: value} and of the full |A|
    low = [dict() for _ in range(n)]
    full = [dict() for _ in range(n)]
    for (br, bc), B in blocks.items():
        for r in range(bs):
            for c in range(bs):
                v = float(B[r, c])
                if v == 0.0:
                    continue
                i, j = br * bs + r, bc * bs + c
                if br == bc:
                    full[i][j] = mpf(v)
                    if j <= i:
                        low[i][j] = mpf(v)
                else:
                    full[i][j] = mpf(v)
                    full[j][i] = mpf(v)
                    low[j][i] = mpf(v)
    L = cholesky_rows(low, n)
    Lcols = [dict() for _ in range(n)]                           # columns of L for the transposed solve
    for i in range(n):
        for j, v in L[i].items():
            Lcols[j][i] = v
    Z = [None] * n
    for c in range(n):
        y = [ZERO] * n
        for i in range(c, n):
            v = mpf(1) if i == c else ZERO
            Li = L[i]
            for j, lij in Li.items():
                if j != i and j >= c:
                    yj = y[j]
                    if yj:
                        v -= lij * yj
            y[i] = v / Li[i] if v else ZERO
        z = [ZERO] * n
        for i in range(n - 1, -1, -1):
            v = y[i]
            for k, lki in Lcols[i].items():
                if k != i:
                    zk = z[k]
                    if zk:
                        v -= lki * zk
            z[i] = v / L[i][i]
        Z[c] = z                                                 # column c (= row c: symmetric)
    # A Z = I at 60 digits (sampled columns)
    for c in range(0, n, max(1, n // 7)):
        for i in range(n):
            r = mp.fsum(a * Z[c][j] for j, a in full[i].items()) - (1 if i == c else 0)
            assert abs(r) < mpf(10) ** -50 * max(1, abs(Z[c][c])) * max(abs(a) for a in full[i].values()), (case, bs, i, c, r)
    absZ = [[abs(v) for v in col] for col in Z]
    T = {}                                                       # rows of |Z| |A| for the scalar rows that are needed

    def trow(i):
        if i not in T:
            zi = absZ[i]
            out = [ZERO] * n
            for k in range(n):
                zik = zi[k]
                if zik:
                    for l, a in full[k].items():
                        out[l] += zik * abs(a)
            T[i] = out
        return T[i]

    Zb = np.zeros((len(pairs), bs, bs))
    s = np.zeros(len(pairs))
    for q, (br, bc) in enumerate(pairs):
        worst = ZERO
        for r in range(bs):
            t = trow(br * bs + r)
            for c in range(bs):
                Zb[q, r, c] = float(Z[bc * bs + c][br * bs + r])
                worst = max(worst, mp.fdot(t, absZ[bc * bs + c]))
        s[q] = float(worst)
    out = dict(nb=np.int32(nb), cp=cp, ri=ri, vals=vals, pairs=np.array(pairs, np.int32), Z=Zb, s=s)
    # what fp64 on the CPU attains
    from oracle import oracle as O
    c = dict(nb=nb, bs=bs, cp=cp, ri=ri, vals=vals)
    rows, cols, idx, tr = H.requests(pairs)
    Zreq = np.array([Zb[i].T if t else Zb[i] for i, t in zip(idx, tr)])
    A = H.dense_from_ccs(nb, bs, cp, ri, vals)
    rn = H.ratios(H.blocks_of(H.numpy_inverse(A), bs, rows, cols), Zreq, s[idx])
    ro = H.ratios(H.oracle_blocks(O, c, rows, cols), Zreq, s[idx])
    out["cpu_numpy"], out["cpu_oracle"] = np.float64(rn.max()), np.float64(ro.max())
    zmax = max(max(col) for col in absZ)
    rec = dict(case=case, bs=bs, n=n, requests=int(len(rows)), cond=float(np.linalg.cond(A)), cpu_numpy=float(rn.max()),
               cpu_oracle=float(ro.max()), corner_over_max=float(max(abs(Z[n - 1 - c][r]) for r in range(bs) for c in range(bs)) / zmax),
               smallest_block_over_max=float(np.abs(Zb).reshape(len(pairs), -1).max(axis=1).min() / float(zmax)))
    return H.key(case, bs), out, rec


def _run(job):
    return legacy_reference(job[1]) if job[0] == "legacy_tridiag" else reference(*job)


def main():
    jobs = [(case, bs) for bs in (7, 6, 3) for case in H.CASES + H.EXTRA_CASES] + [("legacy_tridiag", 6), ("legacy_tridiag", 3)]
    with multiprocessing.Pool(min(8, len(jobs))) as pool:
        results = pool.map(_run, jobs, chunksize=1)
    arrays, recs = {}, []
    for k, out, rec in sorted(results, key=lambda r: r[0]):
        for name, v in out.items():
            arrays[k + "/" + name] = v
        recs.append(rec)
        print(json.dumps(rec))
    np.savez_compressed(H.FIXTURE, **arrays)
    print("wrote", H.FIXTURE, os.path.getsize(H.FIXTURE), "bytes")
    # profiles/inverse_blocks.jsonl: the CPU rows are rewritten, the device rows (the INVBLK lines of tests/test_gpu_inverse_blocks.py) kept
    prof = os.path.join(ROOT, "profiles", "inverse_blocks.jsonl")
    kept = []
    if os.path.exists(prof):
        with open(prof) as f:
            kept = [line for line in f if line.strip() and json.loads(line).get("path") != "cpu"]
    with open(prof, "w") as f:
        for rec in recs:
            f.write(json.dumps(dict(rec, path="cpu")) + "\n")
        f.writelines(kept)


if __name__ == "__main__":
    main()
