"""Writes tests/golden/pcg_steps.npz: seeds and shapes of integer systems (tests/pcg_helpers.py), the extended-precision
iterates of LinearSolverPCG::solve on them rounded to fp64, the iteration counts of its stopping rule, and per case and
output the figure max |got - ref| / max |ref| of the CPU oracle's fp64 PCG (oracle/g2o_oracle.c) against that reference.
Run from the repository root:  python tests/golden/make_pcg_steps.py   (deterministic; about 50 seconds).

Groups
  chain_b<bs>_n<nb>   a chain with ~10 % closures, nb in 1, 255, 256, 257, 513 block rows (block size 7: 1 and 257).  Stored:
                      x_k (k = 1, 2, 3, 8), dn_0 .. dn_K, and the iteration counts
                        it_rel       tolerance 1e-6, relative;
                        it_carried   three solves: relative 1e-6; then twice absolute with tolerance 1e-20, which stops at
                                     the carried 0.5 dn of the solve before;
                        it_loose     absolute with tolerance 1e-2 on a fresh solver, then absolute 1e-6 without init() between:
                                     the second stops at the carried 0.5 dn of the first (after init() it is it_rel);
                        it_default   three solves with the library defaults (tolerance 1e-6, absolute: the carried residual is
                                     below 1e-6 dn_0, so every solve stops where the first does).
  diag_b<bs>          300 diagonal blocks, unary edges only, block condition numbers 1 .. 1e8: x = A_ii^-1 b_i, one iteration.
  red_b<p>            257 poses, 600 landmarks: diagonal blocks of S, S v, b_s, x_k (k = 1, 2, 3) of the PCG on S, it_rel.

Margins, asserted here and relied on by the GPU tests for EXACT iteration counts: no dn_k lies within a relative 1e-6 of a
stopping level it is compared with (fp64 carries dn to ~1e-13).  If one does, move the seed, not the margin.

Below the fp64 floor the iteration count is not a property of the operation: once dn_k <= 1e-20 dn_0 in the reference (a
one-block system is solved by its first iteration, the exact dn_1 is 0 up to the 60 digits), fp64 iterates on its own
rounding residue.  it_steps[k] = k while dn_(k-1) > 1e-20 dn_0 and -1 from there on ("at most k"); a stopping level below
1e-20 dn_0 is stored as -1 in it_carried.  Only the nb = 1 cases have such entries.

Bounds: tests/producer_metric.py's MARGIN (8) x the oracle's figure, never above CEILING (1e-12), asserted for every stored
output.  No stored output is reproduced exactly by the oracle (asserted), so there is no rounding floor to state: FLOORS is
empty and a figure of 0 is a reason to move the seed."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as O                      # noqa: E402
from tests import pcg_helpers as H                  # noqa: E402
from tests import producer_metric as PM             # noqa: E402

mp = H.mp
OUT = os.path.join(HERE, "pcg_steps.npz")
PROFILE = os.path.join(ROOT, "profiles", "pcg_steps.jsonl")
WHO = "oracle_fp64_vs_mp60"
SEED0 = 20250311
REL_TOL = 1e-6
CARRIED_TOL = 1e-20
LOOSE_TOL = 1e-2
RUN_TO = 1e-10                      # relative level the recorded dn sequence runs down to
THRESHOLD_MARGIN = 1e-6
FP64_FLOOR = mp.mpf("1e-20")        # relative to dn_0: below it dn is rounding residue in fp64
FLOORS = {}


def seed_of(group, bs, nb=0):
    return SEED0 + 1000 * {"chain": 1, "diag": 2, "red": 3}[group] + 10 * nb + bs


def clear_of(dn, level, what):
    """No recorded dn_k within THRESHOLD_MARGIN (relative) of a stopping level."""
    for k, v in enumerate(dn):
        assert abs(v / level - 1) > THRESHOLD_MARGIN, (what, k, float(v), float(level))


def oracle_generic(p, l, nP, nL, schur, sets):
    """The oracle's BlockSolver fed through add_edge_set / set_edge_data (sets: (d, v0, v1, dim0, dim1, J0, J1, err))."""
    o = O.OracleSolver(p, l, nP, nL, schur=schur)
    ids = []
    for d, v0, v1, dim0, dim1, J0, J1, err in sets:
        k = o.add_edge_set(d, v0, v1)
        o.set_dims(k, dim0, dim1)
        ids.append(k)
    o.build_structure()
    for k, (d, v0, v1, dim0, dim1, J0, J1, err) in zip(ids, sets):
        o.set_edge_data(k, H.col(J0), None if J1 is None else H.col(J1), H.eye_info(len(v0), d), H.col(err))
    o.build_system()
    o.set_lambda(float(H.LAMBDA), True)
    return o


def same_matrix(o, which, nb, blocks, bs):
    """The oracle's matrix is the int64 one, entry for entry (so all three sides start from the same numbers)."""
    cp, row = o.pattern(which)
    val = o.values("Hpp" if which == "pp" else "Hschur").reshape(-1, bs * bs)
    cp2, row2, blk = H.blocks_to_ccs(nb, blocks)
    assert np.array_equal(cp, cp2) and np.array_equal(row, row2), which
    assert np.array_equal(val, H.ccs_values(blk)), which
    return cp, row, val


def recorded_enough(dn):
    """The dn sequence holds iteration 8 and the stops of the three carried solves."""
    if len(dn) <= max(H.STEPS):
        return False
    level, k = mp.mpf(REL_TOL) * dn[0], 0
    for _ in range(3):
        while k < len(dn) and dn[k] > level:
            k += 1
        if k == len(dn):
            return False
        level = mp.mpf("0.5") * dn[k]
    return True


def add_figure(figs, name, fig):
    assert fig > 0 or name in FLOORS, ("the oracle reproduces %s exactly: state a floor or move the seed" % name)
    assert PM.MARGIN * fig <= PM.CEILING, (name, fig)
    figs[name] = fig


def gen_chain(bs, nb, fx, figs, cov):
    name, seed = H.chain_case_name(bs, nb), seed_of("chain", bs, nb)
    inp = H.chain_inputs(seed, nb, bs)
    blocks, b = H.chain_system(inp, nb, bs)
    sets = [(bs, np.arange(nb, dtype=np.int32), None, bs, 0, inp["Ju"], None, inp["eu"])]
    if len(inp["vi"]):
        sets.append((bs, inp["vi"], inp["vj"], bs, bs, inp["J0"], inp["J1"], inp["e"]))
    o = oracle_generic(bs, H.LANDMARK_DIM[bs], nb, 0, False, sets)
    cp, row, val = same_matrix(o, "pp", nb, blocks, bs)
    assert np.array_equal(o.b(), b.astype(np.float64))
    _, _, blk = H.blocks_to_ccs(nb, blocks)
    solver = H.PcgMp(nb, bs, cp, row, [[[int(v) for v in r] for r in B] for B in blk], b)
    # one run holds every scenario: x_0 = 0 in every solve, so the solves differ in their stopping level only.  Run to a level
    # below every one of them (one block: the eight iterations of the step test)
    if nb == 1:
        r = solver.run(tolerance=0.0, absolute=False, max_iter=max(H.STEPS), keep=H.STEPS)
    else:
        r = solver.run(tolerance=RUN_TO, absolute=False, keep=H.STEPS, until=recorded_enough)
    dn = r["dn"]
    dn0 = dn[0]
    level = mp.mpf(REL_TOL) * dn0
    clear_of(dn, level, name + " rel")
    it_rel = H.stop_iteration(dn, level)
    carried, prev = [it_rel], it_rel
    for _ in range(2):
        lvl = mp.mpf("0.5") * dn[prev]
        assert lvl > mp.mpf(CARRIED_TOL) * dn0 or nb == 1
        if lvl <= FP64_FLOOR * dn0:
            carried.append(-1)
            continue
        clear_of(dn, lvl, name + " carried")
        prev = H.stop_iteration(dn, lvl)
        carried.append(prev)
    # a loose first solve (absolute, tolerance 1e-2: relative on a fresh solver), then tolerance 1e-6 absolute: the second stops at
    # the carried 0.5 dn of the first, well above 1e-6 dn_0 -- unless init() came between, which forgets the carry
    clear_of(dn, mp.mpf(LOOSE_TOL) * dn0, name + " loose")
    loose = [H.stop_iteration(dn, mp.mpf(LOOSE_TOL) * dn0)]
    lvl = mp.mpf("0.5") * dn[loose[0]]
    if lvl <= FP64_FLOOR * dn0:
        loose.append(-1)
    else:
        assert lvl > level
        clear_of(dn, lvl, name + " after loose")
        loose.append(H.stop_iteration(dn, lvl))
        assert loose[1] < it_rel
    # library defaults: d0 = max(1e-6 dn_0, carried 0.5 dn) = 1e-6 dn_0 since the carried residual is below it
    assert mp.mpf("0.5") * dn[it_rel] < level
    default = [it_rel] * 3
    it_steps = [k if (k - 1 < len(dn) and dn[k - 1] > FP64_FLOOR * dn0) else -1 for k in H.STEPS]
    assert nb == 1 or (min(it_steps) > 0 and min(carried) > 0), (name, it_steps, carried)
    fx.update({name + "_seed": np.int64(seed), name + "_dn": H.f64(dn), name + "_it_rel": np.int32(it_rel),
               name + "_it_carried": np.array(carried, np.int32), name + "_it_default": np.array(default, np.int32), name + "_it_loose": np.array(loose, np.int32),
               name + "_it_steps": np.array(it_steps, np.int32)})
    for k in H.STEPS:
        xk = r["x"].get(k, r["x_last"])                          # (a solve that ends before k: x stays where it ended)
        ref = H.f64(xk)
        fx["%s_x%d" % (name, k)] = ref
        ok, xo, ito, _ = O.pcg_solve_blocks(nb, bs, cp, row, val, b.astype(np.float64), tolerance=1e-300, absolute=False, max_iter=k)
        assert ok and (ito == k or it_steps[H.STEPS.index(k)] < 0), (name, k, ito)
        add_figure(figs, "%s_x%d" % (name, k), H.figure(xo, ref))
    ok, _, ito, _ = O.pcg_solve_blocks(nb, bs, cp, row, val, b.astype(np.float64), tolerance=REL_TOL, absolute=False)
    assert ok and ito == it_rel, (name, ito, it_rel)
    cov["chain"].append(dict(case=name, nb=nb, bs=bs, edges=int(len(inp["vi"])), closures=int(len(inp["vi"]) - (nb - 1)),
                             it_rel=it_rel, it_carried=carried, it_default=default, it_loose=loose, it_steps=it_steps))


def gen_diag(bs, fx, figs, cov):
    name, seed = "diag_b%d" % bs, seed_of("diag", bs)
    inp = H.diag_inputs(seed, bs)
    blocks, b = H.diag_system(inp, bs)
    n = len(inp["Ju"])
    o = oracle_generic(bs, H.LANDMARK_DIM[bs], n, 0, False, [(bs, np.arange(n, dtype=np.int32), None, bs, 0, inp["Ju"], None, inp["eu"])])
    cp, row, val = same_matrix(o, "pp", n, blocks, bs)
    assert np.array_equal(o.b(), b.astype(np.float64))
    x = []
    for i in range(n):
        inv = H._inverse([[int(v) for v in r] for r in blocks[(i, i)]])
        x += H._mul_block(inv, [mp.mpf(int(v)) for v in b], i * bs, bs)
    ref = H.f64(x)
    cond = np.array([np.linalg.cond(blocks[(i, i)].astype(np.float64)) for i in range(n)])
    assert cond.min() < 1.5 and cond.max() > 1e8 * 0.5 and all(((cond >= 10.0 ** e) & (cond < 10.0 ** (e + 2))).sum() >= 10 for e in (0, 2, 4, 6))
    ok, xo, ito, _ = O.pcg_solve_blocks(n, bs, cp, row, val, b.astype(np.float64), tolerance=REL_TOL, absolute=False)
    assert ok and ito == 1
    fx.update({name + "_seed": np.int64(seed), name + "_x": ref})
    add_figure(figs, name + "_x", float(H.figure_per_block(xo, ref, bs).max()))
    cov["diag"].append(dict(case=name, bs=bs, blocks=n, cond_min=float(cond.min()), cond_max=float(cond.max())))


def gen_reduced(p, fx, figs, cov):
    l = H.LANDMARK_DIM[p]
    nP, nL = H.RED_POSES, H.RED_LANDMARKS
    name, seed = "red_b%d" % p, seed_of("red", p)
    inp = H.reduced_inputs(seed, p, l)
    pp, obs, Hll, b = H.reduced_system(inp, p, l)
    nobs = np.bincount(inp["ll"], minlength=nL)
    seen = np.bincount(inp["lp"], minlength=nP)
    assert nobs.min() >= 2 and nobs.max() <= 4 and sorted(np.nonzero(seen == 0)[0].tolist()) == sorted(inp["blind"].tolist())
    sets = [(p, inp["vi"], inp["vj"], p, p, inp["J0"], inp["J1"], inp["e"]),
            (p, inp["blind"], None, p, 0, inp["Ju"], None, inp["eu"]),
            (l, nP + inp["ll"], inp["lp"], l, p, inp["Jl"], inp["Jp"], inp["el"])]
    o = oracle_generic(p, l, nP, nL, True, sets)
    assert np.array_equal(o.b(), b.astype(np.float64))
    cp0, row0, blk0 = H.blocks_to_ccs(nP, {k: v + (H.LAMBDA * np.eye(p, dtype=np.int64) if k[0] == k[1] else 0) for k, v in pp.items()})
    assert np.array_equal(o.values("Hpp").reshape(-1, p * p), H.ccs_values(blk0))
    assert np.array_equal(o.values("Hll").reshape(nL, l * l),
                          H.ccs_values([Hll[j] + H.LAMBDA * np.eye(l, dtype=np.int64) for j in range(nL)]))
    S, bs_ = H.reduced_operator_mp(nP, p, l, pp, obs, Hll, H.LAMBDA, b)
    cp, row, blk = H.blocks_to_ccs(nP, S)
    o.solve_schur()
    ocp, orow = o.pattern("hs")
    assert np.array_equal(cp, ocp) and np.array_equal(row, orow)
    oval = o.values("Hschur").reshape(-1, p * p)
    diag_q = [int(cp[c + 1]) - 1 for c in range(nP)]               # (rows increase: the diagonal block ends its column)
    Sdiag = H.ccs_values([blk[q] for q in diag_q])
    v = [mp.mpf(int(t)) for t in inp["v"]]
    solver = H.PcgMp(nP, p, cp, row, blk, bs_)
    Sv = H.f64(solver.mult(v))
    r = solver.run(tolerance=REL_TOL, absolute=False, keep=(1, 2, 3))
    it_rel = r["iterations"]
    assert it_rel > 3
    clear_of(r["dn"], mp.mpf(REL_TOL) * r["dn"][0], name)
    fx.update({name + "_seed": np.int64(seed), name + "_Sdiag": Sdiag, name + "_v": inp["v"], name + "_Sv": Sv, name + "_bs": H.f64(bs_),
               name + "_it_rel": np.int32(it_rel), name + "_dn": H.f64(r["dn"])})
    add_figure(figs, name + "_Sdiag", H.figure(oval[diag_q], Sdiag))
    add_figure(figs, name + "_bs", H.figure(o.bschur(), fx[name + "_bs"]))
    osv = np.zeros(nP * p)
    vf = inp["v"].astype(np.float64)
    for c in range(nP):
        for q in range(cp[c], cp[c + 1]):
            rr, B = int(row[q]), oval[q].reshape(p, p).T
            osv[rr * p:(rr + 1) * p] += B @ vf[c * p:(c + 1) * p]
            if rr != c:
                osv[c * p:(c + 1) * p] += B.T @ vf[rr * p:(rr + 1) * p]
    add_figure(figs, name + "_Sv", H.figure(osv, Sv))
    for k in (1, 2, 3):
        fx["%s_x%d" % (name, k)] = H.f64(r["x"][k])
        ok, xo, ito, _ = O.pcg_solve_blocks(nP, p, cp, row, oval, o.bschur(), tolerance=1e-300, absolute=False, max_iter=k)
        assert ok and ito == k
        add_figure(figs, "%s_x%d" % (name, k), H.figure(xo, fx["%s_x%d" % (name, k)]))
    ok, _, ito, _ = O.pcg_solve_blocks(nP, p, cp, row, oval, o.bschur(), tolerance=REL_TOL, absolute=False)
    assert ok and ito == it_rel, (name, ito, it_rel)
    cov["reduced"].append(dict(case=name, p=p, l=l, poses=nP, landmarks=nL, observations=int(len(inp["lp"])),
                               obs_per_landmark=[int(nobs.min()), int(nobs.max())], blind_poses=inp["blind"].tolist(), it_rel=it_rel))


def generate(verbose=False):
    """(fixture dict, profile lines)."""
    fx, figs = {}, {}
    cov = dict(chain=[], diag=[], reduced=[], scenarios=["steps", "relative", "carried", "default", "loose_then_init"], steps=list(H.STEPS))
    t0 = time.time()
    for bs in sorted(H.CHAIN_BS):
        for nb in H.CHAIN_BS[bs]:
            gen_chain(bs, nb, fx, figs, cov)
            if verbose:
                print("%-16s %5.1f s" % (H.chain_case_name(bs, nb), time.time() - t0), json.dumps(cov["chain"][-1]))
    for bs in sorted(H.CHAIN_BS):
        gen_diag(bs, fx, figs, cov)
        if verbose:
            print("diag_b%d          %5.1f s" % (bs, time.time() - t0), json.dumps(cov["diag"][-1]))
    for p in sorted(H.CHAIN_BS):
        gen_reduced(p, fx, figs, cov)
        if verbose:
            print("red_b%d           %5.1f s" % (p, time.time() - t0), json.dumps(cov["reduced"][-1]))
    lines = []
    for key in sorted(figs):
        fx["oracle_" + key] = np.float64(figs[key])
        fx["floor_" + key] = np.float64(FLOORS.get(key, 0))
        lines.append(dict(output=key, who=WHO, figure=figs[key], floor_eps=FLOORS.get(key, 0),
                          bound=PM.MARGIN * figs[key] if figs[key] > 0 else FLOORS[key] * PM.EPS))
    fx["lambda"] = np.int64(H.LAMBDA)
    fx["coverage_json"] = np.array(json.dumps(cov, sort_keys=True))
    return fx, lines


def main():
    fx, lines = generate(verbose=True)
    for l in lines:
        print("%-22s oracle %.3e  bound %.3e" % (l["output"], l["figure"], l["bound"]))
    np.savez_compressed(OUT, **fx)
    keep = []
    if os.path.exists(PROFILE):
        keep = [l for l in open(PROFILE).read().splitlines() if l.strip() and json.loads(l).get("who") != WHO]
    with open(PROFILE, "w") as fh:
        for l in lines:
            fh.write(json.dumps(l) + "\n")
        for l in keep:
            fh.write(l + "\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
