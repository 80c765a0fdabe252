"""Writes tests/golden/sharded_solve.npz: the references of the sharded-solve tests (tests/sharded_helpers.py holds the inputs, the
census and the measure).  Run offline (python tests/golden/make_sharded_solve.py, about a minute); the host test borrows oracle_solve() from here and nothing else.  The
archive has fixed member dates: a second run reproduces it byte for byte.

  chain_cameras                       the chain length sharded_helpers.chain_cameras() found
  <case>/input_sha                    SHA-256 of the rebuilt inputs
  <case>/w<N>/census_<name>           the census of the partition for N ranks
  <case>/lam<i>/x_hi, x_lo, x_lo2     the solution (x_p, x_l) of the FULL system [[Hpp + lambda I, Hpl], [Hpl', Hll + lambda I]] x = b by
                                      iterative refinement with exact integer residuals (make_cholesky_solve.refine over sharded_helpers.ExactBig), stored only with
                                      the certificate |b - A xref| <= 2^-120 (|A| |xref| + |b|): no elimination order, no partition
  <case>/lam<i>/w<N>/<kind>/r<r>/H, H_s, b, b_s
                                      rank r's summand of the boundary blocks sharded_helpers.ref_blocks() and of the boundary b_p of
                                      the widened lists, from its own landmarks only, at 60 digits (mpmath), with the scales of the
                                      measure; kind "subtree" (landmarks by owner, damping by consumer) or "replicated" (landmark
                                      ranges, rank 0 damps)
  chain/op/...                        the matrix-free operator (operator_reference below)
  <case>/lam<i>/w<N>/<kind>/cpu_<q>   q in H, b, xp, xl: [oracle, NumPy restatement] worst figures (the oracle solves on one rank: it
                                      has figures for xp and xl only, 0 elsewhere)
The CPU rows also go to profiles/sharded_solve.jsonl; the device rows there are the SHARDED lines of the GPU test."""
import json
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import cholesky_helpers as CH      # noqa: E402
from tests import sharded_helpers as H        # noqa: E402
from tests.golden.make_cholesky_solve import refine, write_npz      # noqa: E402

mp.mp.dps = 60
P, L = H.P, H.L


def M(a):
    return mp.matrix(np.atleast_2d(a).tolist())


def f64(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def absm(m):
    return m.apply(abs)


def summand_reference(a, lam, damp, pairs, poses, raw=False):
    """Rank's summands at 60 digits with their scales: (H [n][6][6], H_s [n], b [n][6], b_s [n]); raw: the mpmath matrices
    (blocks, their entrywise scales, vectors, their scales) instead."""
    want = {pr: k for k, pr in enumerate(pairs)}
    wp = {int(i): k for k, i in enumerate(poses)}
    Hm = [mp.zeros(P, P) for _ in pairs]
    Hs = [mp.zeros(P, P) for _ in pairs]
    for (i, j), k in want.items():
        if i == j:
            Hm[k] = M(a["Hpp"][i]) + (mp.mpf(lam) * mp.eye(P) if damp[i] else mp.zeros(P, P))
            Hs[k] = absm(Hm[k])
    bm = [M(a["bp"][i]).T for i in poses]
    bs = [absm(v) for v in bm]
    for j, w in enumerate(a["lists"]):
        if not any(i in wp for i in w) and not any((i1, i2) in want for k, i1 in enumerate(w) for i2 in w[k:]):
            continue
        Dm = M(a["Hll"][j]) + mp.mpf(lam) * mp.eye(L)
        Dinv = Dm ** -1
        W = absm(Dinv) * absm(Dm) * absm(Dinv)
        bl = M(a["bl"][j]).T
        for k, i1 in enumerate(w):
            B1 = M(a["Hpl"][(i1, j)])
            if i1 in wp:
                bm[wp[i1]] = bm[wp[i1]] - B1 * (Dinv * bl)
                bs[wp[i1]] = bs[wp[i1]] + absm(B1) * (W * absm(bl))
            for i2 in w[k:]:
                q = want.get((i1, i2))
                if q is not None:
                    B2 = M(a["Hpl"][(i2, j)])
                    Hm[q] = Hm[q] - B1 * Dinv * B2.T
                    Hs[q] = Hs[q] + absm(B1) * W * absm(B2).T
    if raw:
        return Hm, Hs, bm, bs
    mx = lambda m: float(max(m)) if len(m) else 0.0
    return (np.array([f64(m) for m in Hm]).reshape(-1, P, P), np.array([mx(m) for m in Hs]),
            np.array([f64(v).reshape(-1) for v in bm]).reshape(-1, P), np.array([mx(v) for v in bs]))


def operator_reference(c, a, pts, out, recs):
    """<case>/op/: the diagonal blocks of Hschur, bschur and Hschur d (d = sharded_helpers.operator_vector) of the whole system at
    60 digits with the Hschur / bschur scales (the product under sum_j S_ij |d_j|), and per world the CPU figures [oracle on one
    rank, NumPy per rank in landmark ranges summed in rank order]."""
    from oracle import oracle as O
    from tests import schur_helpers as SH
    nP, lam = c["nP"], H.LAMBDAS[H.OPERATOR_LAMBDA]
    pairs, d = H.all_pairs(pts[2], nP), H.operator_vector(c)
    Hm, Hs, bm, bs = summand_reference(a, lam, np.ones(nP, bool), pairs, np.arange(nP), raw=True)
    q = [mp.zeros(P, 1) for _ in range(nP)]
    qs = [mp.zeros(P, 1) for _ in range(nP)]
    for k, (r, cc) in enumerate(pairs):
        q[r] += Hm[k] * M(d[cc]).T
        qs[r] += Hs[k] * absm(M(d[cc]).T)
        if r != cc:
            q[cc] += Hm[k].T * M(d[r]).T
            qs[cc] += Hs[k].T * absm(M(d[r]).T)
    diag = [k for k, (r, cc) in enumerate(pairs) if r == cc]
    assert [pairs[k][0] for k in diag] == list(range(nP))
    vec = lambda v: np.array([float(x) for x in v])
    ref = dict(diag=np.array([f64(Hm[k]) for k in diag]), diag_s=np.array([float(max(Hs[k])) for k in diag]),
               b=np.array([vec(v) for v in bm]), b_s=np.array([float(max(v)) for v in bs]),
               q=np.array([vec(v) for v in q]), q_s=np.array([float(max(v)) for v in qs]))
    pre = c["name"] + "/op/"
    for name, v in ref.items():
        out[pre + name] = v
    o = O.OracleSolver(P, L, nP, c["nL"], True)
    k0 = o.add_edge_set(H.D, c["v0"], c["v1"])
    o.set_dims(k0, L, P)
    o.build_structure()
    o.set_edge_data(k0, c["Jp"], c["Jc"], c["omega"], c["err"])
    o.build_system()
    o.set_lambda(lam, True)
    o.solve_schur()
    cp, ri = o.pattern("hs")
    opairs = [(int(ri[k]), cc) for cc in range(nP) for k in range(cp[cc], cp[cc + 1])]
    assert opairs == pairs
    Ho = dict(zip(opairs, SH.hschur_blocks(o.values("Hschur"), P)))
    ev_o = dict(diag=np.array([Ho[(i, i)] for i in range(nP)]), b=o.bschur().reshape(nP, P), q=H.product(Ho, pairs, d))
    for w in H.WORLDS:
        _, tot = H.numpy_operator(c, pts[w], w, lam)
        rec = dict(path="cpu", case=c["name"], world=w, kind="operator", lam=lam)
        for name in ("diag", "b", "q"):
            figs = [float(H.figures(e[name], ref[name], ref[name + "_s"]).max()) for e in (ev_o, tot)]
            assert max(figs) <= 64.0, (name, figs)
            out["%sw%d/cpu_%s" % (pre, w, name)] = np.array(figs)
            rec[name] = figs
        recs.append(rec)
        print(json.dumps(rec))


def oracle_solve(c, lam):
    from oracle import oracle as O
    o = O.OracleSolver(P, L, c["nP"], c["nL"], True)
    q = o.add_edge_set(H.D, c["v0"], c["v1"])
    o.set_dims(q, L, P)
    o.build_structure()
    o.set_edge_data(q, c["Jp"], c["Jc"], c["omega"], c["err"])
    o.build_system()
    o.set_lambda(lam, True)
    assert o.solve()
    return o.x()


def main():
    import scipy.linalg as sl
    out = dict(chain_cameras=np.int32(H.chain_cameras()))
    recs = []
    for name in H.CASES:
        c = H.make_case(name)
        nP, nL = c["nP"], c["nL"]
        out[name + "/input_sha"] = np.array(H.input_hash(c))
        a = H.assemble(c)
        pts = {}
        for w in H.WORLDS:
            pts[w] = H.partition(c["v1"], c["v0"].astype(np.int64) - nP, nP, nL, w)
            cen = H.census_of(pts[w], w)
            assert H.census_ok(cen) and cen["halo"] == 0 and cen["boundary_owned"] == 0 and cen["bposes_owned"] == 0, (name, w, cen)
            for q, v in cen.items():
                out["%s/w%d/census_%s" % (name, w, q)] = np.array(v, np.int32)
            recs.append(dict(path="cpu", case=name, world=w, census=cen))
        if name == H.OPERATOR_CASE:
            operator_reference(c, a, pts, out, recs)
        for i, lam in enumerate(H.LAMBDAS):
            A, b = H.full_system(a, nP, nL, lam)
            EM = H.ExactBig(A)
            hi, lo, lo2, nterms = refine(EM, sl.cho_factor(A, lower=True), b)
            pre = "%s/lam%d/" % (name, i)
            out[pre + "x_hi"], out[pre + "x_lo"], out[pre + "x_lo2"] = hi, lo, lo2
            sp, sl_ = H.solution_scales(c, lam, hi[:nP * P], hi[nP * P:])
            k = dict(c=c, x={i: dict(hi=hi, lo=lo, sp=sp, sl=sl_)})
            xo = oracle_solve(c, lam)
            fo = [float(v.max()) for v in H.x_figures(k, i, xo[:nP * P], xo[nP * P:])]
            for w in H.WORLDS:
                pt = pts[w]
                keys = pt["keys"]
                for kind, path in (("subtree", "halo_wide"), ("replicated", "replicated")):
                    bl_idx, bp_idx, _ = H.exchange_lists(pt, w, "halo_wide")
                    sel = H.ref_blocks(pt, w, c)
                    pairs = [(int(keys[q] % nP), int(keys[q] // nP)) for q in bl_idx[sel]]
                    res = H.numpy_schedule(c, pt, w, lam, path)
                    fH = fb = 0.0
                    for r in range(w):
                        ar = H.assemble(c, H.rank_landmarks(pt, c, w, r, path))
                        Hr, Hs, br, bs = summand_reference(ar, lam, H.damped(pt, nP, w, r, path), pairs, bp_idx)
                        p2 = "%sw%d/%s/r%d/" % (pre, w, kind, r)
                        out[p2 + "H"], out[p2 + "H_s"], out[p2 + "b"], out[p2 + "b_s"] = Hr, Hs, br, bs
                        fH = max(fH, float(H.figures(res["summands"][r]["H"][sel], Hr, Hs).max()))
                        fb = max(fb, float(H.figures(res["summands"][r]["b"], br, bs).max()))
                    fx = [float(v.max()) for v in H.x_figures(k, i, res["xp"], res["xl"])]
                    p2 = "%sw%d/%s/" % (pre, w, kind)
                    out[p2 + "cpu_H"], out[p2 + "cpu_b"] = np.array([0.0, fH]), np.array([0.0, fb])
                    out[p2 + "cpu_xp"], out[p2 + "cpu_xl"] = np.array([fo[0], fx[0]]), np.array([fo[1], fx[1]])
                    rec = dict(path="cpu", case=name, world=w, kind=kind, lam=lam, refinement_terms=nterms, H=[0.0, fH], b=[0.0, fb],
                               xp=[fo[0], fx[0]], xl=[fo[1], fx[1]])
                    assert max(fH, fb, fo[0], fo[1], fx[0], fx[1]) <= 64.0, rec
                    recs.append(rec)
                    print(json.dumps(rec))
    write_npz(H.FIXTURE, out)
    print("wrote", H.FIXTURE, os.path.getsize(H.FIXTURE), "bytes")
    assert os.path.getsize(H.FIXTURE) < 1 << 20
    prof = os.path.join(ROOT, "profiles", "sharded_solve.jsonl")
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
