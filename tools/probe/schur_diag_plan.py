#!/usr/bin/env python3
"""Host-only count behind profiles/schur_diag_sym.txt: how much of the Schur tiles' destination loop is diagonal work.

census() rebuilds the tile tables of BlockSolver::build_structure (greedy landmark-range tiles under the LDS budget, destinations
of a tile longest list first, the diagonal ones first inside a round) for any observation list in numpy -- no device, no library --
and counts, for the lane-group width G the solver would pick:
  * the share of entries with s1 == s2,
  * per tile: is the longest list a diagonal one, longest diagonal / longest off-diagonal list,
  * round 0: lane groups with a diagonal destination per wave,
  * the waves by kind (all lane groups diagonal: the wave vote of schur_tile_dests takes the triangle body; none; mixed), the
    share of diagonal entries in all-diagonal waves, and the fused multiply-adds issued per wave-step under three orders.
tests/test_gpu_schur_diag_sym.py uses census() to establish which body its shapes reach.  (Landmarks split over tiles -- more
observations than a tile holds -- are not modelled.)
   python tools/probe/schur_diag_plan.py [poses landmarks [obs_per_landmark]]      (synthetic.make_ba_problem's observation lists)"""
import sys

import numpy as np

NT = 256


def pick_group(avg):
    return 1 if avg <= 2.0 else (4 if avg <= 16.0 else 8)


def _order(c, dg, kind, ngroups):
    o = np.argsort(-c, kind="stable")
    if kind == "parent":
        return o
    if kind == "all":
        return np.concatenate([o[dg[o]], o[~dg[o]]])
    out = []
    for r0 in range(0, len(o), ngroups):
        ch = o[r0:r0 + ngroups]
        out.append(np.concatenate([ch[dg[ch]], ch[~dg[ch]]]))
    return np.concatenate(out)


ORDERS = (("parent", "longest first (parent)"), ("round", "longest first, diagonal first inside a round (this change)"),
          ("all", "all diagonal first, then longest first"))


def census(lm, pose, nP, PD=6, LD=3, budget=39 * 1024, force_group=0):
    """lm, pose: landmark and pose (Hessian index, < 0: fixed) of every observation."""
    lm, pose = np.asarray(lm, np.int64), np.asarray(pose, np.int64)
    keep = pose >= 0
    key = np.unique(lm[keep] * nP + pose[keep])               # one Hpl block per (landmark, pose), poses ascending per landmark
    lm, pose = key // nP, key % nP
    L = int(lm.max()) + 1 if len(lm) else 0
    nobs = np.bincount(lm, minlength=L)
    first = np.concatenate([[0], np.cumsum(nobs)])
    PL = PD * LD
    DPB = ((LD * LD + 1) & ~1) + ((LD * LD + LD + 1) & ~1)
    BPB = (LD + 1) & ~1
    add = nobs * PL * 8 + DPB * 8 + BPB * 8 + nobs * (nobs + 1) // 2 * 14
    assert add.max() <= budget, "a landmark that would be split over tiles"
    tile_of = np.zeros(L, np.int64)
    t = used = l0 = 0
    for i in range(L):
        if i > l0 and used + add[i] > budget:
            t, used, l0 = t + 1, 0, i
        used += add[i]
        tile_of[i] = t
    n_tiles = t + 1
    rows, cols, tls = [], [], []
    for K in np.unique(nobs):
        if K == 0:
            continue
        sel = np.flatnonzero(nobs == K)
        ps = pose[first[sel][:, None] + np.arange(K)[None, :]]
        a, b = np.triu_indices(K)
        rows.append(ps[:, a].reshape(-1))
        cols.append(ps[:, b].reshape(-1))
        tls.append(np.repeat(tile_of[sel], len(a)))
    row, col, tl = np.concatenate(rows), np.concatenate(cols), np.concatenate(tls)
    n_ent = len(row)
    uk, cnt = np.unique((tl * nP + col) * nP + row, return_counts=True)   # tile, then block order of the column-major pattern
    d_tile = uk // (nP * nP)
    d_diag = (uk // nP) % nP == uk % nP
    n_td = len(uk)
    avg = n_ent / n_td
    G = force_group or pick_group(avg)
    GC = 2 if (G >= 2 and PD % 2 == 0) else 1
    GE, ngroups, gpw = G // GC, NT // G, 64 // G
    NR = PD // GC
    # fused multiply-adds per lane and entry: the block (general: NR * PD elements; triangle body: NR (NR + 1) at GC = 2,
    # PD (PD + 1) / 2 at GC = 1), and the rhs term of a diagonal entry (NR * LD) -- in the general body every lane group of a
    # wave steps through it as soon as ONE of the wave's destinations is diagonal
    fma_gen, fma_rhs = NR * PD * LD, NR * LD
    fma_sym = (NR * (NR + 1) if GC == 2 else PD * (PD + 1) // 2) * LD
    bounds = np.flatnonzero(np.diff(d_tile)) + 1
    starts, ends = np.concatenate([[0], bounds]), np.concatenate([bounds, [n_td]])
    res = {k: dict(cov=0, steps=0, fma=0, all_diag=0, all_off=0, mixed=0) for k, _ in ORDERS}
    longest_is_diag, ratio, rounds = 0, [], []
    hist = np.zeros((NT // 64, gpw + 1), np.int64)
    for s, e in zip(starts, ends):
        c, dg = cnt[s:e], d_diag[s:e]
        longest_is_diag += bool(dg[np.argmax(c)])
        if (~dg).any() and dg.any():
            ratio.append(c[dg].max() / c[~dg].max())
        rounds.append(-(-len(c) // ngroups))
        for kind, _ in ORDERS:
            o = _order(c, dg, kind, ngroups)
            r = res[kind]
            for w0 in range(0, len(o), gpw):
                w = o[w0:w0 + gpw]
                steps = -(-c[w].max() // GE)                  # the wave's lane groups run in lockstep
                nd = int(dg[w].sum())
                sym = nd == len(w)
                r["all_diag" if sym else ("all_off" if nd == 0 else "mixed")] += 1
                if sym:
                    r["cov"] += c[w].sum()
                r["steps"] += steps
                # (the parent has no triangle body: an all-diagonal wave costs the general body there)
                r["fma"] += steps * ((fma_sym + fma_rhs) if sym and kind != "parent" else (fma_gen + (fma_rhs if nd else 0)))
                if kind == "parent" and w0 < ngroups:
                    hist[(w0 // gpw) % (NT // 64), nd] += 1
    return dict(G=G, GC=GC, GE=GE, ngroups=ngroups, gpw=gpw, n_tiles=n_tiles, n_td=n_td, n_ent=n_ent, avg=avg,
                n_diag_ent=int(cnt[d_diag].sum()), n_diag_td=int(d_diag.sum()), longest_is_diag=longest_is_diag,
                ratio=np.array(ratio), rounds=np.array(rounds), hist=hist, orders=res)


def chain_observations(P, L, K):
    """synthetic.make_ba_problem: landmark j is seen by K consecutive cameras; cameras 0 and 1 are fixed."""
    j = np.arange(L, dtype=np.int64)
    lo = np.clip((j * P) // L - K // 2, 0, P - K)
    pose = (lo[:, None] + np.arange(K)[None, :] - 2).reshape(-1)
    return np.repeat(j, K), pose, P - 2


def main():
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    lm, pose, nP = chain_observations(P, L, K)
    c = census(lm, pose, nP)
    print("problem: %d poses, %d landmarks, %d observations per landmark" % (P, L, K))
    print("tiles %d, partial blocks %d, entries %d, entries per partial %.2f -> lane group G = %d (%d lane groups per wave, %d per round)"
          % (c["n_tiles"], c["n_td"], c["n_ent"], c["avg"], c["G"], c["gpw"], c["ngroups"]))
    print("entries with s1 == s2: %d of %d = %.1f %%;  diagonal partial blocks: %d of %d = %.1f %%"
          % (c["n_diag_ent"], c["n_ent"], 100.0 * c["n_diag_ent"] / c["n_ent"], c["n_diag_td"], c["n_td"], 100.0 * c["n_diag_td"] / c["n_td"]))
    print("tiles whose longest list is a diagonal one: %d of %d = %.1f %%" % (c["longest_is_diag"], c["n_tiles"], 100.0 * c["longest_is_diag"] / c["n_tiles"]))
    r = c["ratio"]
    print("longest diagonal / longest off-diagonal list per tile: min %.2f  median %.2f  mean %.2f  max %.2f" % (r.min(), np.median(r), r.mean(), r.max()))
    print("rounds per tile: mean %.2f, max %d;  destinations per tile: mean %.1f" % (c["rounds"].mean(), c["rounds"].max(), c["n_td"] / c["n_tiles"]))
    print("round 0, parent order: tiles by the number of lane groups with a diagonal destination, per wave (columns 0 .. %d)" % c["gpw"])
    for w in range(NT // 64):
        print("  wave %d: %s" % (w, " ".join("%6d" % v for v in c["hist"][w])))
    print("destination order: waves all-diagonal / all-off-diagonal / mixed | share of diagonal entries in all-diagonal waves | wave-steps | "
          "fused multiply-adds issued per lane over all wave-steps (parent order, general body only = 1)")
    o = c["orders"]
    for kind, name in ORDERS:
        r = o[kind]
        print("  %-60s %6d / %6d / %6d | %5.1f %% | %9d | %11d" % (name, r["all_diag"], r["all_off"], r["mixed"], 100.0 * r["cov"] / c["n_diag_ent"],
                                                                  r["steps"], r["fma"]))
    print("  (this change / parent order: %.3f)" % (o["round"]["fma"] / o["parent"]["fma"]))


if __name__ == "__main__":
    main()
