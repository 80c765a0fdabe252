"""Writes tests/golden/schur_blocks.npz (and schur_blocks_fused.npz for the fused BA cases, keys "<case>/<output>@<damping index>"
with the same suffixes): the Schur stage of the cases of tests/schur_helpers.py at 60 digits (mpmath), the
per-block scales of the measure, and what plain fp64 on the CPU attains under it.  Run offline
(python tests/golden/make_schur_blocks.py, a few minutes on 8 cores); no test imports this file.  The archive is written with
fixed member dates, so a second run reproduces it byte for byte.

Per case, under the key prefix "<case>/" (blocks in natural (row, column) layout, rounded once to fp64):
  input_sha, assembled_sha   SHA-256 of the rebuilt inputs and of their exact fp64 assembly (schur_helpers.input_hash /
                             assembled_hash): the tests rebuild both and compare
  Dinv [nL][l][l]            (Hll_l + lambda I)^-1
  Hschur [nnz][p][p]         Hpp + lambda I - sum_l Hpl_il Dinv_l Hpl_jl' on the library's pattern (upper block CCS)
  bschur [nP][p]             b_p - sum_l Hpl_il Dinv_l b_l
  xl [nL][l]                 Dinv_l (b_l - sum_i Hpl_il' x_i) for the pinned x_p of the case (schur_helpers.make_case)
  xp_solved, xl_solved       Hschur^-1 bschur by a dense Cholesky factorisation, and the landmarks behind it
  <output>_s                 the scale of every block (the measure in the head of tests/schur_helpers.py), at 60 digits
  <output>_cpu [2]           the worst figure of the oracle and of NumPy in the tiles' order (schur_helpers.*_evaluation)
  <output>_floor             0 unless both CPU figures are 0: then 0.5, the figure of a result rounded once (|ref| <= s for every
                             output, so one rounding of the exact value is at most 0.5 u s); the bound is 8 x the larger

Asserted here at 60 digits: the fp64 assembly of every case is exact; the full system [Hpp + lambda I, Hpl; Hpl', Hll + lambda I]
[x_p; x_l] = b holds to 1e-50 for the solved x_p (rows of the ORIGINAL system: the Schur loop of the reference is not what is
checked against); every CPU figure of the exact-assembly cases is at most 64 u s (the fused cases carry their
producers' fp64 error, up to 340 u s on the producer group: no limit there); the census and coverage conditions of every case.  The reference shares no
code with block_solver.hip or oracle/g2o_oracle.c."""
import io
import json
import multiprocessing
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import schur_helpers as H      # noqa: E402

mp.mp.dps = 60
mpf = mp.mpf
ZERO = mpf(0)
CPU_LIMIT = 64.0


def M(a):
    return [[mpf(float(v)) for v in row] for row in np.atleast_2d(a)]


def V(a):
    return [mpf(float(v)) for v in a]


def mm(A, B):
    Bt = list(zip(*B))
    return [[mp.fdot(r, c) for c in Bt] for r in A]


def mv(A, x):
    return [mp.fdot(r, x) for r in A]


def T(A):
    return [list(r) for r in zip(*A)]


def absm(A):
    return [[abs(v) for v in r] for r in A]


def add(A, B, sign=1):
    return [[a + sign * b for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def mmax(A):
    return max(max(r) for r in A)


def inverse_small(A):
    """Gauss-Jordan with partial pivoting at 60 digits."""
    n = len(A)
    W = [list(A[i]) + [mpf(1) if i == j else ZERO for j in range(n)] for i in range(n)]
    for c in range(n):
        piv = max(range(c, n), key=lambda i: abs(W[i][c]))
        W[c], W[piv] = W[piv], W[c]
        ip = 1 / W[c][c]
        W[c] = [v * ip for v in W[c]]
        for i in range(n):
            if i != c and W[i][c]:
                f = W[i][c]
                W[i] = [a - f * b for a, b in zip(W[i], W[c])]
    return [r[n:] for r in W]


def assemble_mp(c):
    """The edges of schur_helpers.assemble at 60 digits, edge by edge: ({(i, j): Hpp}, {(i, landmark): Hpl}, [Hll], bp, bl)."""
    p, l, d, nP, nL = c["p"], c["l"], c["d"], c["nP"], c["nL"]
    z = lambda r, k: [[ZERO] * k for _ in range(r)]
    Hpp, Hpl, Hll = {}, {}, [z(l, l) for _ in range(nL)]
    bp, bl = [[ZERO] * p for _ in range(nP)], [[ZERO] * l for _ in range(nL)]
    col = lambda J, dim, dd: T([V(J[k * dd:(k + 1) * dd]) for k in range(dim)])       # column-major dd x dim -> rows
    for e in range(len(c["v0"])):
        j, i = int(c["v0"][e]) - nP, int(c["v1"][e])
        A0, A1, Om = col(c["J0"][e], l, d), col(c["J1"][e], p, d), M(c["om"][e].reshape(d, d))
        we = mv(Om, V(c["err"][e]))
        OA0 = mm(Om, A0)
        Hll[j] = add(Hll[j], mm(T(A0), OA0))
        bl[j] = [a - b for a, b in zip(bl[j], mv(T(A0), we))]
        if i >= 0:
            Hpp[(i, i)] = add(Hpp.get((i, i), z(p, p)), mm(T(A1), mm(Om, A1)))
            Hpl[(i, j)] = add(Hpl.get((i, j), z(p, l)), mm(T(A1), OA0))
            bp[i] = [a - b for a, b in zip(bp[i], mv(T(A1), we))]
    for e in range(len(c["ca"])):
        i, j = int(c["ca"][e]), int(c["cb"][e])
        A, B, Om = col(c["JA"][e], p, p), col(c["JB"][e], p, p), M(c["O2"][e].reshape(p, p))
        we = mv(Om, V(c["e2"][e]))
        OB = mm(Om, B)
        Hpp[(i, i)] = add(Hpp.get((i, i), z(p, p)), mm(T(A), mm(Om, A)))
        Hpp[(j, j)] = add(Hpp.get((j, j), z(p, p)), mm(T(B), OB))
        Hpp[(i, j)] = add(Hpp.get((i, j), z(p, p)), mm(T(A), OB))
        bp[i] = [a - b for a, b in zip(bp[i], mv(T(A), we))]
        bp[j] = [a - b for a, b in zip(bp[j], mv(T(B), we))]
    return Hpp, Hpl, Hll, bp, bl


def same(Amp, Afp):
    Afp = np.atleast_2d(Afp)
    return all(Amp[r][k] == mpf(float(Afp[r, k])) for r in range(len(Amp)) for k in range(len(Amp[0])))


def cholesky(A):
    n = len(A)
    L = [[ZERO] * n for _ in range(n)]
    for i in range(n):
        Li = L[i]
        for j in range(i + 1):
            s = A[i][j] - (mp.fdot(Li[:j], L[j][:j]) if j else ZERO)
            if i == j:
                assert s > 0, "the reduced system is not positive definite"
                Li[j] = mp.sqrt(s)
            else:
                Li[j] = s / L[j][j]
    return L


def chol_solve(L, Lt, b, first=0):
    """x of L L' x = b; b is zero before row `first`."""
    n = len(L)
    y = [ZERO] * n
    for i in range(first, n):
        y[i] = (b[i] - mp.fdot(L[i][first:i], y[first:i])) / L[i][i]
    x = [ZERO] * n
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - mp.fdot(Lt[i][i + 1:], x[i + 1:])) / L[i][i]
    return x


def f64(A):
    return np.array([[float(v) for v in r] for r in A]) if A and isinstance(A[0], list) else np.array([float(v) for v in A])


def schur_part(p, l, nP, nL, lam, Hpp, Hpl, Hll, bp, bl, lists, hs, xpin, mag=None):
    """Dinv, Hschur, bschur and x_l for the pinned x_p at 60 digits with the scales of the measure.  mag: the magnitudes that
    stand for |Hpp|, |Hpl|, |Hll|, |b_p|, |b_l| in the scales (the operand sums of a fused case); None: the absolute values."""
    if mag is None:
        mag = dict(Hpp={k: absm(B) for k, B in Hpp.items()}, Hpl={k: absm(B) for k, B in Hpl.items()}, Hll=[absm(B) for B in Hll],
                   bp=[[abs(v) for v in b] for b in bp], bl=[[abs(v) for v in b] for b in bl])
    eye = lambda n: [[lam if i == j else ZERO for j in range(n)] for i in range(n)]
    D = [add(Hll[j], eye(l)) for j in range(nL)]
    Dinv = [inverse_small(D[j]) for j in range(nL)]
    W = [mm(mm(absm(Dinv[j]), add(mag["Hll"][j], eye(l))), absm(Dinv[j])) for j in range(nL)]
    nnz = len(hs)
    Hs = [None] * nnz
    Ss = [None] * nnz
    for (r, cc), q in hs.items():
        B = Hpp.get((r, cc))
        B = [[ZERO] * p for _ in range(p)] if B is None else [list(row) for row in B]
        S = mag["Hpp"].get((r, cc))
        S = [[ZERO] * p for _ in range(p)] if S is None else [list(row) for row in S]
        if r == cc:
            for k in range(p):
                B[k][k] += lam
                S[k][k] += lam
        Hs[q], Ss[q] = B, S
    bs = [list(v) for v in bp]
    bss = [list(v) for v in mag["bp"]]
    xl, xls = [], []
    for j, w in enumerate(lists):
        Bs = [Hpl[(i, j)] for i in w]
        Ba = [mag["Hpl"][(i, j)] for i in w]
        Db = mv(Dinv[j], bl[j])
        Wb = mv(W[j], mag["bl"][j])
        r, ra = list(bl[j]), list(mag["bl"][j])
        for k, i1 in enumerate(w):
            BD, BW = mm(Bs[k], Dinv[j]), mm(Ba[k], W[j])
            bs[i1] = [x - y for x, y in zip(bs[i1], mv(Bs[k], Db))]
            bss[i1] = [x + y for x, y in zip(bss[i1], mv(Ba[k], Wb))]
            for k2 in range(k, len(w)):
                q = hs[(i1, w[k2])]
                Hs[q] = add(Hs[q], mm(BD, T(Bs[k2])), -1)
                Ss[q] = add(Ss[q], mm(BW, T(Ba[k2])))
            r = [x - y for x, y in zip(r, mv(T(Bs[k]), xpin[i1]))]
            ra = [x + y for x, y in zip(ra, mv(T(Ba[k]), [abs(v) for v in xpin[i1]]))]
        xl.append(mv(Dinv[j], r))
        xls.append(mv(W[j], ra))
    out = dict(Dinv=np.array([f64(B) for B in Dinv]), Dinv_s=np.array([float(mmax(B)) for B in W]),
               Hschur=np.array([f64(B) for B in Hs]), Hschur_s=np.array([float(mmax(B)) for B in Ss]),
               bschur=f64(bs), bschur_s=np.array([float(max(v)) for v in bss]),
               xl=f64(xl), xl_s=np.array([float(max(v)) for v in xls]))
    return out, Hs, bs, D, Dinv, W


def fused_reference(name):
    """A fused BA case from the estimates: project_edge and robust of tests/reference_mp.py per observation, the products, then
    schur_part at both dampings with the operand sums as magnitudes (the head of make_producer_edges.gen_ba defines them)."""
    from tests import reference_mp as R
    c = H.make_fused_case(name)
    st = H.fused_structure(c)
    nP, nL, E = c["nP"], c["nL"], c["E"]
    z = lambda r, k: [[ZERO] * k for _ in range(r)]
    Hpp, Hpl, Hll = {(i, i): z(6, 6) for i in range(nP)}, {}, [z(3, 3) for _ in range(nL)]
    mHpp, mHpl, mHll = {(i, i): z(6, 6) for i in range(nP)}, {}, [z(3, 3) for _ in range(nL)]
    bp, bl = [[ZERO] * 6 for _ in range(nP)], [[ZERO] * 3 for _ in range(nL)]
    mbp, mbl = [[ZERO] * 6 for _ in range(nP)], [[ZERO] * 3 for _ in range(nL)]
    sides = {}
    for k in range(E):
        Tc, X = c["cams"][c["cam_idx"][k]], c["pts"][c["pt_idx"][k]]
        f, cx, cy, kind, delta = c["classes"][c["edge_class"][k]]
        pc = R.camera_point(R.iso(Tc), R.V(X))
        assert pc[2] > 0 and np.abs(X).max() / pc[2] <= 25, (name, k)                      # the generator's exclusions
        A, B, e = R.project_edge(Tc, X, c["meas"][k], f, cx, cy)
        e2 = e[0] * e[0] + e[1] * e[1]
        if int(kind) in (1, 4):
            assert abs(e2 / mpf(float(delta)) ** 2 - 1) > 1e-6, (name, k)
            side = e2 <= mpf(float(delta)) ** 2
            sides[side] = sides.get(side, 0) + 1
        w = R.robust(int(kind), delta, e2)[1]
        ez = [max(abs(e[i]), abs(mpf(float(c["meas"][k, i])))) for i in range(2)]
        A = [[A[r + 2 * q] for q in range(3)] for r in range(2)]                          # column-major 2 x 3 -> rows
        B = [[B[r + 2 * q] for q in range(6)] for r in range(2)]
        j, h = int(c["pt_idx"][k]), int(c["v1"][k])
        for r in range(3):
            for q in range(3):
                t0, t1 = w * A[0][r] * A[0][q], w * A[1][r] * A[1][q]
                Hll[j][r][q] += t0 + t1
                mHll[j][r][q] += abs(t0) + abs(t1)
            bl[j][r] -= w * (A[0][r] * e[0] + A[1][r] * e[1])
            mbl[j][r] += w * (abs(A[0][r]) * ez[0] + abs(A[1][r]) * ez[1])
        if h < 0:
            continue
        Hpl[(h, j)], mHpl[(h, j)] = z(6, 3), z(6, 3)
        for r in range(6):
            for q in range(6):
                t0, t1 = w * B[0][r] * B[0][q], w * B[1][r] * B[1][q]
                Hpp[(h, h)][r][q] += t0 + t1
                mHpp[(h, h)][r][q] += abs(t0) + abs(t1)
            for q in range(3):
                t0, t1 = w * B[0][r] * A[0][q], w * B[1][r] * A[1][q]
                Hpl[(h, j)][r][q] = t0 + t1
                mHpl[(h, j)][r][q] = abs(t0) + abs(t1)
            bp[h][r] -= w * (B[0][r] * e[0] + B[1][r] * e[1])
            mbp[h][r] += w * (abs(B[0][r]) * ez[0] + abs(B[1][r]) * ez[1])
    assert len(sides) == 2 and min(sides.values()) >= 5, (name, sides)                   # both sides of the Huber threshold
    assert set(Hpl) == set(st["pl"][2])
    xpin = [V(c["xp"][i * 6:(i + 1) * 6]) for i in range(nP)]
    from oracle import oracle as O
    out = dict(input_sha=np.array(H.fused_input_hash(c)))
    rec = dict(case=name, path="cpu", p=6, l=3, lam=list(H.FUSED_LAMBDAS), huber_sides=[int(sides[True]), int(sides[False])])
    for i, lam in enumerate(H.FUSED_LAMBDAS):
        part = schur_part(6, 3, nP, nL, mpf(lam), Hpp, Hpl, Hll, bp, bl, st["lists"], st["hs"][2], xpin,
                          dict(Hpp=mHpp, Hpl=mHpl, Hll=mHll, bp=mbp, bl=mbl))[0]
        eo, en, cen = H.fused_cpu_evaluations(O, c, st, lam)
        rec.update(G=cen["G"], tiles=cen["n_tiles"], partial_blocks=cen["n_td"], waves=[cen["all_diag"], cen["all_off"], cen["mixed"]])
        for o in H.OUTPUTS:
            key = "%s@%d" % (o, i)
            figs = [float(H.figures(e[o], part[o], part[o + "_s"]).max()) for e in (eo, en)]
            out[key], out[key + "_s"], out[key + "_cpu"] = part[o], part[o + "_s"], np.array(figs)
            out[key + "_floor"] = np.float64(0.5 if max(figs) == 0.0 else 0.0)
            rec[key] = dict(oracle=figs[0], numpy=figs[1])
    return name, out, rec


def reference(name):
    c = H.make_case(name)
    a = H.assemble(c)
    p, l, nP, nL = c["p"], c["l"], c["nP"], c["nL"]
    lam = mpf(c["lam"])
    # ---- the fp64 assembly is exact
    Hpp, Hpl, Hll, bp, bl = assemble_mp(c)
    assert set(Hpp) == set(a["pp"][2]) and set(Hpl) == set(a["pl"][2]), name
    for k, q in a["pp"][2].items():
        assert same(Hpp[k], a["HppB"][q]), (name, "Hpp", k)
    for k, q in a["pl"][2].items():
        assert same(Hpl[k], a["HplB"][q]), (name, "Hpl", k)
    for j in range(nL):
        assert same(Hll[j], a["HllB"][j]) and same([bl[j]], a["bl"][j]), (name, "Hll", j)
    for i in range(nP):
        assert same([bp[i]], a["bp"][i]), (name, "b", i)
    cen = H.census_of(c, a)
    H.assert_census(name, c, cen)
    xpin = [V(c["xp"][i * p:(i + 1) * p]) for i in range(nP)]
    out, Hs, bs, D, Dinv, W = schur_part(p, l, nP, nL, lam, Hpp, Hpl, Hll, bp, bl, a["lists"], a["hs"][2], xpin)
    lists, hs, nnz = a["lists"], a["hs"][2], len(a["hs"][1])
    with_solve = nP <= H.FULL_SOLVE_MAX_POSES
    if with_solve:
        n = nP * p
        A = [[ZERO] * n for _ in range(n)]
        for (r, cc), q in hs.items():
            for i in range(p):
                for k in range(p):
                    A[r * p + i][cc * p + k] = Hs[q][i][k]
                    A[cc * p + k][r * p + i] = Hs[q][i][k]
        for (r, cc), q in hs.items():                            # the reference block itself is symmetric on the diagonal
            if r == cc:
                assert all(abs(Hs[q][i][k] - Hs[q][k][i]) <= mpf(10) ** -55 * abs(Hs[q][i][i]) for i in range(p) for k in range(p))
        L = cholesky(A)
        Lt = T(L)
        rhs = [v for b in bs for v in b]
        x = chol_solve(L, Lt, rhs)
        absA = absm(A)
        t = mv(absA, [abs(v) for v in x])                        # |Hs| |x_p|
        sx = [ZERO] * n                                          # |Hs^-1| (|Hs| |x_p|), column by column of the inverse
        for k in range(n):
            e = [ZERO] * n
            e[k] = mpf(1)
            z = chol_solve(L, Lt, e, first=k)
            sx[k] = mp.fdot([abs(v) for v in z], t)              # row k of the (symmetric) inverse
        xs = [x[i * p:(i + 1) * p] for i in range(nP)]
        xls2, xlss2 = [], []
        for j, w in enumerate(lists):
            r, ra = list(bl[j]), [abs(v) for v in bl[j]]
            for i1 in w:
                r = [u - v for u, v in zip(r, mv(T(Hpl[(i1, j)]), xs[i1]))]
                ra = [u + v for u, v in zip(ra, mv(T(absm(Hpl[(i1, j)])), [abs(v) for v in xs[i1]]))]
            xls2.append(mv(Dinv[j], r))
            xlss2.append(mv(W[j], ra))
        # ---- the rows of the ORIGINAL system at 60 digits
        tiny = mpf(10) ** -50
        res_p = [[ZERO] * p for _ in range(nP)]
        mag_p = [[ZERO] * p for _ in range(nP)]
        for (r, cc), B in Hpp.items():
            Bl = [list(row) for row in B]
            if r == cc:
                for k in range(p):
                    Bl[k][k] += lam
            res_p[r] = [u + v for u, v in zip(res_p[r], mv(Bl, xs[cc]))]
            mag_p[r] = [u + v for u, v in zip(mag_p[r], mv(absm(Bl), [abs(v) for v in xs[cc]]))]
            if r != cc:
                res_p[cc] = [u + v for u, v in zip(res_p[cc], mv(T(Bl), xs[r]))]
                mag_p[cc] = [u + v for u, v in zip(mag_p[cc], mv(T(absm(Bl)), [abs(v) for v in xs[r]]))]
        for j, w in enumerate(lists):
            rl = mv(D[j], xls2[j])
            ml = mv(absm(D[j]), [abs(v) for v in xls2[j]])
            for i1 in w:
                B = Hpl[(i1, j)]
                res_p[i1] = [u + v for u, v in zip(res_p[i1], mv(B, xls2[j]))]
                mag_p[i1] = [u + v for u, v in zip(mag_p[i1], mv(absm(B), [abs(v) for v in xls2[j]]))]
                rl = [u + v for u, v in zip(rl, mv(T(B), xs[i1]))]
                ml = [u + v for u, v in zip(ml, mv(T(absm(B)), [abs(v) for v in xs[i1]]))]
            for k in range(l):
                assert abs(rl[k] - bl[j][k]) <= tiny * (ml[k] + abs(bl[j][k])), (name, "landmark row", j, k)
        for i in range(nP):
            for k in range(p):
                assert abs(res_p[i][k] - bp[i][k]) <= tiny * (mag_p[i][k] + abs(bp[i][k])), (name, "pose row", i, k)
        out.update(xp_solved=f64(xs), xp_solved_s=np.array([float(max(sx[i * p:(i + 1) * p])) for i in range(nP)]),
                   xl_solved=f64(xls2), xl_solved_s=np.array([float(max(v)) for v in xlss2]))
    # ---- what fp64 on the CPU attains
    from oracle import oracle as O
    ev = (H.oracle_evaluation(O, c, a, with_solve), H.numpy_evaluation(c, a, cen, with_solve))
    rec = dict(case=name, path="cpu", p=p, l=l, G=cen["G"], tiles=cen["n_tiles"], partial_blocks=cen["n_td"], destinations=nnz,
               waves=[cen["all_diag"], cen["all_off"], cen["mixed"]], lam=c["lam"])
    for o in [k for k in out if not k.endswith("_s")]:
        figs = [float(H.figures(e[o], out[o], out[o + "_s"]).max()) for e in ev]
        assert max(figs) <= CPU_LIMIT, (name, o, figs)
        out[o + "_cpu"] = np.array(figs)
        out[o + "_floor"] = np.float64(0.5 if max(figs) == 0.0 else 0.0)
        rec[o] = dict(oracle=figs[0], numpy=figs[1])
        assert np.all(np.abs(out[o]).reshape(len(out[o]), -1).max(axis=1) <= out[o + "_s"] * (1 + 1e-15)), (name, o)
    Dn = a["HllB"] + c["lam"] * np.eye(l)
    big = np.abs(out["Hschur"]).reshape(nnz, -1).max(axis=1)
    cov = H.coverage(c, a)
    rec.update(cond_landmark=float(np.linalg.cond(Dn).max()), blocks_below_1e10=int((big < 1e-10 * big.max()).sum()),
               seen=[int(v) for v in cov["seen"]], fixed_obs=cov["fixed_obs"])
    out["input_sha"] = np.array(H.input_hash(c))
    out["assembled_sha"] = np.array(H.assembled_hash(a))
    out["blocks_below_1e10"] = np.int64(rec["blocks_below_1e10"])
    out["cond_landmark"] = np.float64(rec["cond_landmark"])
    return name, out, rec


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


def _run(name):
    return fused_reference(name) if name in H.FUSED_CASES else reference(name)


def main():
    names = sys.argv[1:] or ["ba_chain"] + sorted(H.CASES, key=lambda n: -H.make_case(n)["nP"] * H.CASES[n][0]) + ["ba_prod1", "ba_prodc"]
    with multiprocessing.Pool(min(8, len(names))) as pool:
        results = pool.map(_run, names, chunksize=1)
    arrays, recs = {}, []
    for k, out, rec in sorted(results, key=lambda r: r[0]):
        for name, v in out.items():
            arrays[k + "/" + name] = v
        recs.append(rec)
        print(json.dumps(rec))
    if sys.argv[1:]:
        return                                                   # (a partial run writes nothing)
    # two archives, each below the size limit of a committed file: the generic cases, and the fused BA cases
    for path, keep in ((H.FIXTURE, lambda k: k.split("/")[0] not in H.FUSED_CASES), (H.FUSED_FIXTURE, lambda k: k.split("/")[0] in H.FUSED_CASES)):
        write_npz(path, {k: v for k, v in arrays.items() if keep(k)})
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1000000
    # profiles/schur_blocks.jsonl: the CPU rows are rewritten, the device rows (the SCHURBLK lines of tests/test_gpu_schur_blocks.py) kept
    prof = os.path.join(ROOT, "profiles", "schur_blocks.jsonl")
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
