"""The sharded solve, phase by phase, against a 120-bit reference (tests/sharded_helpers.py: inputs, census, lock-step driver,
measure; tests/golden/sharded_solve.npz: references and the CPU figures behind the bounds).

One process, no spawn, no threads: `world` ShardedBlockSolver handles share the torch stream, their own phase generators
(ShardedBlockSolver.solve_phases) are stepped side by side, and every all-reduce is a sum in fp64 in rank order on the host with
each rank's summand kept.  Paths: "halo" (subtree, native exchange: the default), "halo_wide" (the same with the widened lists of
sharded_helpers, the only way to a keep flag of 0 and to a non-empty halo), "full" (subtree, x_exchange = "full"), "replicated".

What a rank holds for poses it neither owns nor shares nor has in its halo (halo paths, mask_solution = 0): include/g2ohip.h
promises valid x_p "for its own and the shared poses" and nothing for the others; nothing is asserted about them here.
Boundary blocks after unpack: on the "full" path from Hschur; on the native paths the factorisation may read them from storage
behind Hpp (the virtual source of exchange_setup), so the driver lets every rank run exchange_pack(1) once more behind unpack(1),
which reads them from wherever they live (sharded_helpers.lockstep_solve).  "Shared poses are bit-identical" compares values the
ranks computed each on their own (the shared top is factorised redundantly); a halo pose is compared with its owner's value from
BEFORE unpack(3), the owner's summand of the last collective.  On "halo_wide" the product's sequence is not run unmodified: the
driver inserts one write before exchange_pack(3) (sharded_helpers._poison_foreign_halo), the only way to give `hmine` something
to multiply.  The subtree-root buffer (ARR_EXCHANGE) is laid out in
elimination order, which neither getPartition nor stats() describes: it is held by its effect on x alone.
Each line `SHARDED {json}` is a device row of profiles/sharded_solve.jsonl."""
import json

import numpy as np
import pytest

from tests import sharded_helpers as H

pytestmark = pytest.mark.gpu
P, L = H.P, H.L


def _blocks(v):
    return np.asarray(v).reshape(-1, P, P).transpose(0, 2, 1)


def _row(case, world, path, solve, rank, quantity, fig, bound, cpu, failures):
    print("SHARDED " + json.dumps(dict(path="device", case=case, world=world, schedule=path, solve=solve, rank=rank, quantity=quantity,
                                       figure=float(fig), bound=float(bound), cpu=[float(v) for v in cpu])))
    if not fig <= bound:
        failures.append((quantity, "solve %d" % solve, "rank %d" % rank, float(fig), float(bound)))


@pytest.mark.parametrize("path", H.PATHS)
@pytest.mark.parametrize("world", H.WORLDS)
@pytest.mark.parametrize("case", H.CASES)
def test_sharded_solve_phase_by_phase(case, world, path):
    import torch
    from openslam_g2o_amd import capi
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    k = H.load_case(case)
    c, pt = k["c"], k["pt"][world]
    nP, nL = c["nP"], c["nL"]
    kind = "replicated" if path == "replicated" else "subtree"
    hs = H.make_handles(c, world, path, dev)
    bl_w, bp_w, _ = H.exchange_lists(pt, world, "halo_wide")
    bl, bp, halo = H.exchange_lists(pt, world, path)
    sel = H.ref_blocks(pt, world, c)
    own_sel = sel < len(pt["boundary"])                          # the stored references that belong to the partition's own list
    # ---- preconditions: the census, from the handles' own partition, and the exact assembly
    cen = k["census"][world]
    for r, s in enumerate(hs):
        my = H.rank_landmarks(pt, c, world, r, path)
        assert np.array_equal(s.lm_index, my) and len(my) >= 1
        if kind == "subtree":
            po, cons = s.local.getPartition()
            assert np.array_equal(po, pt["pose_owner"]) and np.array_equal(cons, pt["consumer"])
            assert [int((po == q).sum()) for q in range(world)] == cen["owned"] and int((po < 0).sum()) == cen["shared"] > 0
            assert min(cen["owned"]) >= 1
            assert np.array_equal(s.boundary, bl) and np.array_equal(s.bposes, bp) and np.array_equal(s.halo, halo)
            assert len(pt["boundary"]) == cen["boundary"] > 0 and len(pt["bposes"]) == cen["bposes"] > 0 and len(pt["halo"]) == cen["halo"]
            if path == "halo_wide":                              # a halo of `world` poses with `world` different owners, keep flags of 0
                assert len(halo) == world and sorted(po[halo].tolist()) == list(range(world))
                assert (cons[bl[-world:]] >= 0).all() and (po[bp[-world:]] >= 0).all()
        s.buildSystem()
        a = H.assemble(c, my)
        want = H.device_layout(a, s.local.pattern(capi.HPP), s.local.pattern(capi.HPL))
        got = (s.local.values(capi.HPP), s.local.values(capi.HPL), s.local.values(capi.HLL), s.local.b())
        for name, g, w_ in zip(("Hpp", "Hpl", "Hll", "b"), got, want):
            assert np.array_equal(g, w_), "rank %d: %s is not the exact assembly bit for bit" % (r, name)
    po, cons = pt["pose_owner"], pt["consumer"]
    failures, first = [], None
    for solve, i in enumerate((0, 1, 0)):
        lam = H.LAMBDAS[i]
        for s in hs:
            s.setLambda(lam, True)
        held = [] if path in ("halo", "halo_wide") else None
        status, log = H.lockstep_solve(hs, held)
        assert all(st is True for st in status), status
        xs = [s.local.x() for s in hs]
        # ---- summands
        if kind == "subtree" and path != "full":
            assert len(log) % 3 == 0
            e = log[-3][0]
            nb = len(bl) * P * P
            sH = [_blocks(v[:nb]) for v in e["summands"]]
            sb = [v[nb:].reshape(-1, P) for v in e["summands"]]
            pick = sel if path == "halo_wide" else sel[own_sel]
            refsel = np.ones(len(sel), bool) if path == "halo_wide" else own_sel
            nbp = len(bp)
        elif path == "full":
            sH = [_blocks(v) for v in log[0][0]["summands"]]
            sb = [v.reshape(nP, P)[bp] for v in log[1][0]["summands"]]
            pick, refsel, nbp = sel[own_sel], own_sel, len(bp)
        else:
            sH = [_blocks(v)[bl_w] for v in log[0][0]["summands"]]
            sb = [v.reshape(nP, P)[bp_w] for v in log[0][1]["summands"]]
            pick, refsel, nbp = sel, np.ones(len(sel), bool), len(bp_w)
        for r in range(world):
            ref = k["sum"][(i, world, kind, r)]
            fH = H.figures(sH[r][pick], ref["H"][refsel], ref["H_s"][refsel])
            fb = H.figures(sb[r], ref["b"][:nbp], ref["b_s"][:nbp])
            for q, f in (("H", fH), ("b", fb)):
                bd, cpu = H.bound(k, i, world, path, q)
                _row(case, world, path, solve, r, "summand_" + q, f.max(), bd, cpu, failures)
        # ---- after unpack
        if kind == "subtree":
            tot_b = (log[-3][0]["total"][len(bl) * P * P:] if path != "full" else log[1][0]["total"]).reshape(-1, P)
            for r, s in enumerate(hs):
                bs = s._device_tensor(capi.ARR_BSCHUR).cpu().numpy().reshape(nP, P)
                poses = bp if path != "full" else np.arange(nP)
                keep = (po[poses] == r) | (po[poses] < 0)
                assert np.array_equal(bs[poses][keep], tot_b[keep]), "rank %d does not hold the sum of a boundary b_p it consumes" % r
                assert not bs[poses][~keep].any(), "rank %d holds a boundary b_p it does not consume" % r
                if held is not None:                             # the native paths: what exchange_pack(1) reads back behind unpack(1)
                    nb = len(bl) * P * P
                    tot = _blocks(log[-3][0]["total"][:nb])
                    Hd = _blocks(held[-1][r][:nb])
                    hk = (cons[bl] == r) | (cons[bl] < 0)
                    assert np.array_equal(Hd[hk], tot[hk]), "rank %d does not hold the sum of a boundary block it consumes" % r
                    assert not Hd[~hk].any(), "rank %d holds a boundary block it does not consume (largest entry %.3e)" % (r, np.abs(Hd[~hk]).max())
                    assert np.array_equal(held[-1][r][nb:].reshape(-1, P), tot_b * keep[:, None])
                if path == "full":
                    Hd = _blocks(s._subtree_tensors()["H"].cpu().numpy())[bl]
                    tot = _blocks(log[0][0]["total"])
                    hk = (cons[bl] == r) | (cons[bl] < 0)
                    assert np.array_equal(Hd[hk], tot[hk]) and not Hd[~hk].any(), "rank %d: boundary blocks after unpack" % r
        # ---- solution
        shared = np.flatnonzero(po < 0)
        for r, s in enumerate(hs):
            xp, xl = xs[r][:nP * P].reshape(nP, P), xs[r][nP * P:].reshape(-1, L)
            if path in ("halo", "halo_wide"):
                valid = (po == r) | (po < 0)
                valid[halo] = True
            else:
                valid = np.ones(nP, bool)
            full_l = np.zeros((nL, L))
            full_l[s.lm_index] = xl
            ep, el = H.x_figures(k, i, np.where(valid[:, None], xp, (k["x"][i]["hi"][:nP * P]).reshape(nP, P)), full_l)
            for q, f in (("xp", ep[valid]), ("xl", el[s.lm_index])):
                bd, cpu = H.bound(k, i, world, path, q)
                _row(case, world, path, solve, r, q, f.max(), bd, cpu, failures)
            x0 = xs[0][:nP * P].reshape(nP, P)
            if kind == "subtree":
                assert np.array_equal(xp[shared], x0[shared]), "shared poses differ between rank 0 and rank %d" % r
                if path in ("halo", "halo_wide"):
                    # the owner's value as it was BEFORE unpack(3) is the owner's summand of the last collective; the other
                    # ranks' summands of that entry are exactly zero (hmine), whatever they hold there (halo_wide: a poison)
                    for q, h in enumerate(halo):
                        own = log[-1][0]["summands"][po[h]][q * P:(q + 1) * P]
                        assert np.array_equal(xp[h], own), "halo pose %d on rank %d is not its owner's value (off by %.3e)" % (h, r, np.abs(xp[h] - own).max())
                        if po[h] != r:
                            mine = log[-1][0]["summands"][r][q * P:(q + 1) * P]
                            assert not mine.any(), "rank %d adds %.3e to halo pose %d, which it does not own" % (r, np.abs(mine).max(), h)
            if path in ("full", "replicated"):
                assert np.array_equal(xp, x0), "x_p differs between rank 0 and rank %d" % r
        for s in hs:
            s.restoreDiagonal()
        promised = []                                            # x_p where it is promised, and the own landmarks
        for r in range(world):
            v = (po == r) | (po < 0) if path in ("halo", "halo_wide") else np.ones(nP, bool)
            v[halo] = True
            promised.append(np.r_[xs[r][:nP * P].reshape(nP, P)[v].ravel(), xs[r][nP * P:]])
        if solve == 0:
            first = promised
        elif solve == 2:                                         # the stale-sum check: back at the first damping, the first result bit for bit
            for r in range(world):
                assert np.array_equal(promised[r], first[r]), "rank %d: the third solve does not repeat the first" % r
    assert not failures, failures


@pytest.mark.parametrize("world", H.WORLDS)
def test_matrix_free_operator_per_rank(world):
    """schurOperatorPrepare / schurOperatorApply per rank in mode "pcg" (landmarks sharded by range): the sums over the ranks, in
    rank order, of bschur, of the diagonal blocks (ARR_SCHUR_DIAG) and of the product with a pinned dyadic vector against the
    60-digit references of the whole system under the Hschur / bschur scales; and only rank 0's summand carries lambda_p: for a
    pose none of a rank's landmarks sees, the rank's diagonal block is exactly lambda I on rank 0 and exactly zero elsewhere, its
    bschur and its row of the product exactly zero on the ranks above 0."""
    import torch
    from openslam_g2o_amd import capi, distributed as DI
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    k = H.load_case(H.OPERATOR_CASE)
    c, pt, op = k["c"], k["pt"][world], H.load_operator()
    nP, lam = c["nP"], H.LAMBDAS[H.OPERATOR_LAMBDA]
    d = H.operator_vector(c)
    dt = torch.from_numpy(d.reshape(-1).copy()).to(dev)
    parts, _ = H.numpy_operator(c, pt, world, lam)               # (only `touched` is used: which poses a rank's landmarks see)
    tot, failures = None, []
    for r in range(world):
        s = DI.ShardedBlockSolver(P, L, rank=r, world=world, comm=H.NoComm(), mode="pcg")
        s.setup_ba(c, torch_device=dev, fused=False)
        assert np.array_equal(s.lm_index, H.rank_landmarks(pt, c, world, r, "replicated")) and len(s.lm_index) >= 1
        s.buildSystem()
        s.setLambda(lam, True)
        s.local.schurOperatorPrepare()
        qt = torch.zeros_like(dt)
        s.local.schurOperatorApply(dt.data_ptr(), qt.data_ptr())
        torch.cuda.synchronize()
        got = dict(diag=_blocks(s._device_tensor(capi.ARR_SCHUR_DIAG).cpu().numpy()), b=s._device_tensor(capi.ARR_BSCHUR).cpu().numpy().reshape(nP, P),
                   q=qt.cpu().numpy().reshape(nP, P))
        bare = ~parts[r]["touched"]
        assert bare.any() and (~bare).any()
        want = lam * np.eye(P) if r == 0 else np.zeros((P, P))
        assert all(np.array_equal(B, want) for B in got["diag"][bare]), "rank %d: the diagonal block of a pose it does not see" % r
        assert not got["b"][bare].any()
        if r > 0:
            assert not got["q"][bare].any(), "rank %d damps a pose in the product" % r
        else:
            assert np.array_equal(got["q"][bare], lam * d[bare])
        tot = got if tot is None else {q: tot[q] + got[q] for q in tot}
        s.restoreDiagonal()
    for q in ("diag", "b", "q"):
        f = H.figures(tot[q], op[q], op[q + "_s"])
        bd, cpu = H.operator_bound(op, world, q)
        _row(H.OPERATOR_CASE, world, "pcg", 0, -1, "operator_" + q, f.max(), bd, cpu, failures)
    assert not failures, failures
