"""Inputs, exact assembly, census, lock-step driver and measure of the sharded-solve tests (tests/golden/make_sharded_solve.py,
tests/test_sharded_reference_host.py, tests/test_gpu_sharded_phases.py).

INPUTS.  The exact-assembly recipe of tests/schur_helpers.py on the generic edge-data path of ShardedBlockSolver.setup_ba
(fused=False), family (6, 3): the observation lists of openslam_g2o_amd.synthetic (a camera chain with landmarks; in the `loops`
case the chain runs back and forth, so the reduced pattern is not a band), Jacobian entries integers in [-3, 3], the information
the identity (`chain`) or a small integer SPD block (`loops`), errors multiples of 1/8, lambda a power of two; `contrast` is
`chain` with the camera Jacobians of a few poses scaled by 2^-48 (scaled_poses), so that a boundary block and some x_p lie far
below the largest.  Hpp, Hpl, Hll and b
of every rank are then exact in fp64 in any order, and every test starts by holding the device to them bit for bit.

CENSUS.  The partition comes from g2ohip_partition_poses, which is host only.  For every clique of poses that co-observe a
landmark lies on one root-to-leaf path of the elimination tree, a landmark's owned poses all belong to ONE subtree below the cut:
with this partitioner every boundary block and every boundary pose is shared (keep flag 1 on every rank) and the halo is EMPTY,
for both cases and for the further topologies tests/test_sharded_reference_host.py pins (grid, hubs, random long-range landmarks).  The keep flags and the halo entries of the native exchange are
therefore reached only through the `halo_wide` path of these tests: the driver registers, on top of the partition's own lists, the
first owned pose of every rank as a halo pose and as a boundary pose, and its diagonal block as a boundary block (consumer = the
owner: keep 0 everywhere else), and sets the x_p of such a halo pose to HALO_POISON on the ranks that do not own it just before
exchange_pack(3), so that the hmine factor multiplies something.  That is a schedule the exchange entry points document and the partitioner never asks for.

MEASURE.  Per block, u = 2^-53, no floor and no global scale:
    summand of a boundary block (i, j) on rank r   max |got - ref| / (u s),  s = max(|Hpp_r,ij + lambda_r I| + sum_{l on r} |Hpl_il| W_l |Hpl_jl|')
    summand of boundary b_p,i on rank r            s = max(|b_r,i| + sum_{l on r} |Hpl_il| W_l |b_l|)       (W_l of schur_helpers)
    x_p                                            cholesky_helpers.scales on the reduced system: |Z| d (d' |xref_p|) per pose
    x_l                                            max W_l (|b_l| + sum_i |Hpl_il|' |xref_i|)
the first two at 60 digits from the rank's own operands (stored), the last two in fp64 from reference quantities.  A summand
whose scale is 0 must be exactly 0.  The bound of a quantity is 8 x the larger of the CPU figures the fixture records (the
oracle's single-rank solve for x; the NumPy restatement of the sharded schedule, numpy_schedule), 8 x 0.5 where both are 0."""
import hashlib
import os

import numpy as np

from tests import cholesky_helpers as CH

U = 2.0 ** -53
MARGIN = 8.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sharded_solve.npz")
P, L, D = 6, 3, 2
WORLDS = (2, 3, 4)
LAMBDAS = (1.0, 2.0 ** -10)
CASES = ("chain", "loops", "contrast")
PATHS = ("halo", "halo_wide", "full", "replicated")
CHAIN_SEARCH_FROM = 64
LANDMARKS_PER_POSE = 4
LOOPS = dict(P=66, L=200, laps=4)
MAX_REF_BLOCKS = 30                                              # boundary blocks with a stored summand reference per (case, world)
_SEED = {"chain": 8100, "loops": 8200, "contrast": 8400}
CONTRAST_SHIFT = -48                                             # camera Jacobians of the scaled poses of `contrast`: 2^-48
_cache = {}


def _capi():
    from openslam_g2o_amd import capi
    return capi


def _spd(rng, d):
    M = rng.randint(-1, 2, (d, d)).astype(np.float64)
    return M @ M.T + np.eye(d)


def topology(name, cameras=None):
    from openslam_g2o_amd import synthetic as S
    if name in ("chain", "contrast"):
        n = cameras or chain_cameras()
        pr = S.make_ba_problem(n, LANDMARKS_PER_POSE * n)
    else:
        pr = S.make_ba_loops(LOOPS["P"], LOOPS["L"], laps=LOOPS["laps"], hubs=0)
    return pr["nP"], pr["nL"], pr["v0"].astype(np.int32), pr["v1"].astype(np.int32)


def partition(v1, lm, nP, nL, world):
    """The pre-pass of ShardedBlockSolver.setup_ba (mode subtree) on the host."""
    from openslam_g2o_amd import distributed as DI
    prow, pcol, plm = DI.coobservation_pairs(v1, lm)
    colptr, rowidx, keys = DI.reduced_pattern(prow, pcol, nP)
    po, cons = _capi().partition_poses(P, colptr, rowidx, world)
    lo = DI.assign_landmarks(v1, lm, po, nL, world)
    bnd = DI.boundary_blocks(keys, cons, prow, pcol, plm, lo, nP)
    bposes, halo = DI.boundary_poses(v1, lm, po, lo)
    return dict(pose_owner=po, consumer=cons, lm_owner=lo, boundary=bnd, bposes=bposes, halo=halo, keys=keys, colptr=colptr, rowidx=rowidx)


def census_of(pt, world):
    po, cons = pt["pose_owner"], pt["consumer"]
    return dict(owned=[int((po == r).sum()) for r in range(world)], shared=int((po < 0).sum()), boundary=int(len(pt["boundary"])),
                bposes=int(len(pt["bposes"])), halo=int(len(pt["halo"])), landmarks=[int((pt["lm_owner"] == r).sum()) for r in range(world)],
                boundary_owned=int((cons[pt["boundary"]] >= 0).sum()), bposes_owned=int((po[pt["bposes"]] >= 0).sum()))


def census_ok(cen):
    """What a case must keep (the halo condition of the partition's own list cannot hold: see the head)."""
    return min(cen["owned"]) >= 1 and cen["shared"] > 0 and cen["boundary"] > 0 and cen["bposes"] > 0 and min(cen["landmarks"]) >= 1


def chain_cameras():
    """The smallest chain, searched upward from CHAIN_SEARCH_FROM cameras, whose partition passes census_ok for every world."""
    if "chain_n" not in _cache:
        from openslam_g2o_amd import synthetic as S
        n = CHAIN_SEARCH_FROM
        while True:
            pr = S.make_ba_problem(n, LANDMARKS_PER_POSE * n)
            v0, v1 = pr["v0"].astype(np.int64), pr["v1"]
            if all(census_ok(census_of(partition(v1, v0 - pr["nP"], pr["nP"], pr["nL"], w), w)) for w in WORLDS):
                break
            n += 1
            assert n < 200
        _cache["chain_n"] = n
    return _cache["chain_n"]


def scaled_poses(nP, nL, v0, v1):
    """The poses of `contrast` whose camera Jacobians are scaled by 2^CONTRAST_SHIFT: the first two neighbouring poses that are
    shared for every world (their common block is a boundary block far below the largest), and the widened halo poses of every
    world (wide_poses).  The partition depends on the observation lists alone, not on the values."""
    pts = [partition(v1, v0.astype(np.int64) - nP, nP, nL, w) for w in WORLDS]
    both = np.flatnonzero(np.all([(pt["pose_owner"][:-1] < 0) & (pt["pose_owner"][1:] < 0) for pt in pts], axis=0))
    assert len(both), "no two neighbouring poses are shared for every world"
    out = {int(both[0]), int(both[0]) + 1}
    for pt, w in zip(pts, WORLDS):
        out |= set(wide_poses(pt, w).tolist())
    return np.array(sorted(out))


def make_case(name, cameras=None):
    """The problem dictionary setup_ba takes (nP, nL, v0, v1, Jp [E][6], Jc [E][12], omega [E][4], err [E][2])."""
    nP, nL, v0, v1 = topology(name, cameras)
    rng = np.random.RandomState(_SEED[name])
    E = len(v0)
    Jp = rng.randint(-3, 4, (E, D * L)).astype(np.float64)
    Jc = rng.randint(-3, 4, (E, D * P)).astype(np.float64)
    om = np.array([(_spd(rng, D) if name == "loops" else np.eye(D)).reshape(-1) for _ in range(E)])
    err = rng.randint(-16, 17, (E, D)) / 8.0
    c = dict(name=name, nP=nP, nL=nL, v0=v0, v1=v1, Jp=Jp, Jc=Jc, omega=om, err=err)
    if name == "contrast":                                       # (a power of two: the assembly stays exact)
        c["scaled"] = scaled_poses(nP, nL, v0, v1)
        Jc[np.isin(v1, c["scaled"])] *= 2.0 ** CONTRAST_SHIFT
    return c


def sha256_of(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def input_hash(c):
    return sha256_of([c[k] for k in ("v0", "v1", "Jp", "Jc", "omega", "err")] + [np.array(LAMBDAS)])


# ================================================================================================ exact assembly
def _mats(J, d, dim):
    return J.reshape(len(J), dim, d).transpose(0, 2, 1)


def assemble(c, my=None):
    """The system of the landmarks `my` (global ids, ascending; None: all) and their edges, exact in fp64: Hpp [nP][6][6] (diagonal
    blocks), bp [nP][6], Hll [n][3][3], bl [n][3], lists (per local landmark its free poses, ascending) and Hpl {(pose, local
    landmark): [6][3]}, blocks in natural (row, column) layout."""
    nP, nL = c["nP"], c["nL"]
    my = np.arange(nL) if my is None else np.asarray(my)
    loc = np.full(nL, -1, np.int64)
    loc[my] = np.arange(len(my))
    lm = loc[c["v0"].astype(np.int64) - nP]
    sel = lm >= 0
    lm, pose = lm[sel], c["v1"][sel]
    A0, A1 = _mats(c["Jp"][sel], D, L), _mats(c["Jc"][sel], D, P)
    Om = c["omega"][sel].reshape(-1, D, D)
    we = np.einsum("eij,ej->ei", Om, c["err"][sel])
    free = pose >= 0
    Hll, bl = np.zeros((len(my), L, L)), np.zeros((len(my), L))
    np.add.at(Hll, lm, np.einsum("eia,eij,ejb->eab", A0, Om, A0))
    np.add.at(bl, lm, -np.einsum("eia,ei->ea", A0, we))
    Hpp, bp = np.zeros((nP, P, P)), np.zeros((nP, P))
    np.add.at(Hpp, pose[free], np.einsum("eia,eij,ejb->eab", A1[free], Om[free], A1[free]))
    np.add.at(bp, pose[free], -np.einsum("eia,ei->ea", A1[free], we[free]))
    blk = np.einsum("eia,eij,ejb->eab", A1[free], Om[free], A0[free])
    Hpl = {}
    for k, (i, j) in enumerate(zip(pose[free].tolist(), lm[free].tolist())):
        Hpl[(i, j)] = Hpl.get((i, j), 0.0) + blk[k]
    lists = [[] for _ in range(len(my))]
    for (i, j) in sorted(Hpl):
        lists[j].append(i)
    return dict(Hpp=Hpp, bp=bp, Hll=Hll, bl=bl, Hpl=Hpl, lists=lists, my=my, mask=sel)


def device_layout(a, pp, pl):
    """(Hpp, Hpl, Hll, b) of an assembly in the library's layout on the patterns (colptr, rowidx) it reports."""
    tr = lambda X: np.ascontiguousarray(np.asarray(X).transpose(0, 2, 1)).reshape(len(X), -1)
    cp, ri = pp
    Hpp = np.array([a["Hpp"][c] if ri[q] == c else np.zeros((P, P)) for c in range(len(cp) - 1) for q in range(cp[c], cp[c + 1])])
    cp, ri = pl
    Hpl = [a["Hpl"][(int(ri[q]), j)] for j in range(len(cp) - 1) for q in range(cp[j], cp[j + 1])]
    assert len(Hpl) == len(a["Hpl"])
    return tr(Hpp).reshape(-1), tr(np.array(Hpl).reshape(-1, P, L)).reshape(-1), tr(a["Hll"]).reshape(-1), np.concatenate([a["bp"].reshape(-1), a["bl"].reshape(-1)])


def full_system(a, nP, nL, lam):
    """(A, b) of the un-reduced system [[Hpp + lambda I, Hpl], [Hpl', Hll + lambda I]] of an assembly, dense."""
    n = nP * P + nL * L
    A = np.zeros((n, n))
    for i in range(nP):
        A[i * P:(i + 1) * P, i * P:(i + 1) * P] = a["Hpp"][i] + lam * np.eye(P)
    for j in range(nL):
        o = nP * P + j * L
        A[o:o + L, o:o + L] = a["Hll"][j] + lam * np.eye(L)
    for (i, j), B in a["Hpl"].items():
        o = nP * P + j * L
        A[i * P:(i + 1) * P, o:o + L] = B
        A[o:o + L, i * P:(i + 1) * P] = B.T
    return A, np.concatenate([a["bp"].reshape(-1), a["bl"].reshape(-1)])


class ExactBig:
    """cholesky_helpers.ExactMatrix without its limits (a common power of two of at most 2^40, row sums below 2^38): the nonzeros
    of a dyadic matrix as Python integers at their common lowest exponent, products through object arrays.  Same residual()."""

    def __init__(self, A):
        self.rows, self.cols = np.nonzero(A)
        v = A[self.rows, self.cols]
        self.e = CH.lsb_exponent(v)
        self.v = CH.to_int(v, self.e)
        self.va = np.array([abs(int(x)) for x in self.v], object)
        self.n = A.shape[0]

    def _dot(self, v, X):
        out = np.zeros(self.n, object)
        np.add.at(out, self.rows, v * np.asarray(X, object)[self.cols])
        return out

    def residual(self, X, e, b):
        """(R, T, er) with b - A X 2^e = R 2^er and |A| |X| 2^e + |b| = T 2^er, all exact."""
        er = e + self.e
        B = CH.to_int(b, er)
        Xa = np.array([abs(int(x)) for x in X], object)
        return B - self._dot(self.v, X), self._dot(self.va, Xa) + np.array([abs(int(x)) for x in B], object), er


# ================================================================================================ the schedule's lists
def rank_landmarks(pt, c, world, rank, path):
    if path == "replicated":
        from openslam_g2o_amd import distributed as DI
        lo, hi = DI.landmark_range(c["nL"], world, rank)
        return np.arange(lo, hi)
    return np.flatnonzero(pt["lm_owner"] == rank)


def damped(pt, nP, world, rank, path):
    """The poses whose diagonal rank `rank` damps (BlockSolver's lam_mask; rank 0 alone in replicated mode)."""
    if path == "replicated":
        return np.full(nP, rank == 0)
    o = pt["consumer"][pt["colptr"][1:] - 1]                      # the diagonal block closes its column
    return (o == rank) | ((o < 0) & (rank == 0))


def wide_poses(pt, world):
    """The first owned pose of every rank."""
    return np.array([int(np.flatnonzero(pt["pose_owner"] == r)[0]) for r in range(world)])


def exchange_lists(pt, world, path):
    """(boundary blocks, boundary poses, halo poses) the schedule of `path` registers."""
    b, bp, h = pt["boundary"], pt["bposes"], pt["halo"]
    if path == "halo_wide":
        w = wide_poses(pt, world)
        diag = np.searchsorted(pt["keys"], w.astype(np.int64) * len(pt["pose_owner"]) + w)
        assert not set(diag) & set(b.tolist()) and not set(w) & set(bp.tolist())
        return np.r_[b, diag], np.r_[bp, w], np.r_[h, w]
    return b, bp, h


def ref_blocks(pt, world, c=None):
    """Indices into exchange_lists(..., "halo_wide")[0] of the blocks whose summand has a stored reference: at most MAX_REF_BLOCKS
    of the partition's own, evenly spread, with (case `contrast`) every boundary block between two scaled poses, and the widened
    ones."""
    nb = len(pt["boundary"])
    own = np.linspace(0, nb - 1, min(nb, MAX_REF_BLOCKS)).round().astype(np.int64)
    if c is not None and "scaled" in c:
        nP = len(pt["pose_owner"])
        k = pt["keys"][pt["boundary"]]
        own = np.r_[own, np.flatnonzero(np.isin(k % nP, c["scaled"]) & np.isin(k // nP, c["scaled"]))]
    return np.r_[np.unique(own), nb + np.arange(world)]


# ================================================================================================ NumPy restatement
def W_of(Dm, Dinv):
    return np.abs(Dinv) @ np.abs(Dm) @ np.abs(Dinv)


def rank_schur(a, lam, damp, blocks, poses, nP):
    """Rank's partial Schur sums in fp64, landmark by landmark: {(i, j): [6][6]} for the (row, column) pairs `blocks`, [len(poses)][6]."""
    Dinv = np.linalg.inv(a["Hll"] + lam * np.eye(L))
    want = {b: np.zeros((P, P)) for b in blocks}
    for (i, j) in want:
        if i == j:
            want[(i, j)] = a["Hpp"][i] + (lam * np.eye(P) if damp[i] else 0.0)
    bs = {int(i): a["bp"][i].copy() for i in poses}
    for j, w in enumerate(a["lists"]):
        for k, i1 in enumerate(w):
            V = a["Hpl"][(i1, j)] @ Dinv[j]
            if i1 in bs:
                bs[i1] = bs[i1] - V @ a["bl"][j]
            for i2 in w[k:]:
                if (i1, i2) in want:
                    want[(i1, i2)] = want[(i1, i2)] - V @ a["Hpl"][(i2, j)].T
    return want, np.array([bs[int(i)] for i in poses]).reshape(len(poses), P), Dinv


def numpy_schedule(c, pt, world, lam, path="halo", faults=(), state=None):
    """The sharded schedule restated in NumPy: per-rank partial Schur sums of the whole reduced system in fp64, the sum over the
    ranks in rank order for what the schedule exchanges, the keep masks, SciPy's Cholesky of the reduced system, back-substitution
    by owner.  Returns dict(xp [nP][6], xps [rank] (what a rank holds), xl [nL][3], summands [rank] dict(H, b), Hsum, bsum, held
    [rank] (boundary blocks after unpack), ...).  `state`: the result of the solve before, for the fault "stale"; `faults` seeds
    wrong results: "stale", "no_keep", "halo_zero", "halo_swap"."""
    nP, nL = c["nP"], c["nL"]
    keys = pt["keys"]
    pairs = [(int(k % nP), int(k // nP)) for k in keys]
    bl_idx, bp_idx, halo = exchange_lists(pt, world, "halo_wide" if path == "replicated" else path)   # (replicated: everything is summed; the lists pick what is measured)
    bpairs = [pairs[q] for q in bl_idx]
    po, cons = pt["pose_owner"], pt["consumer"]
    parts = []
    for r in range(world):
        a = assemble(c, rank_landmarks(pt, c, world, r, path))
        H, b, Dinv = rank_schur(a, lam, damped(pt, nP, world, r, path), pairs, np.arange(nP), nP)
        parts.append(dict(a=a, H=H, b=b, Dinv=Dinv))
    summ = [dict(H=np.array([parts[r]["H"][bp_] for bp_ in bpairs]).reshape(-1, P, P), b=parts[r]["b"][bp_idx].copy()) for r in range(world)]
    Hsum, bsum = summ[0]["H"].copy(), summ[0]["b"].copy()
    for r in range(1, world):
        Hsum, bsum = Hsum + summ[r]["H"], bsum + summ[r]["b"]
    small = int(np.argmin(np.abs(Hsum).reshape(len(Hsum), -1).max(axis=1))) if len(Hsum) else 0
    if "stale" in faults:                                        # one small boundary block summed twice: the sum of the solve before
        Hsum[small] = Hsum[small] + state["Hsum"][small]         # is still held by a rank that does not re-form the block
    hkeep = [(cons[bl_idx] == r) | (cons[bl_idx] < 0) for r in range(world)]
    held = [Hsum * hkeep[r][:, None, None] for r in range(world)]
    if "no_keep" in faults:                                      # a boundary block kept on a rank that does not consume it
        for r in range(world):
            if (~hkeep[r]).any():
                k = int(np.flatnonzero(~hkeep[r])[0])
                held[r][k] = Hsum[k]
    # the reduced system as its consumers see it (every block is consumed on one rank or on all alike)
    Hs = np.zeros((nP * P, nP * P))
    if path == "replicated":
        for q, (i, j) in enumerate(pairs):
            t = parts[0]["H"][(i, j)]
            for r in range(1, world):
                t = t + parts[r]["H"][(i, j)]
            Hs[i * P:(i + 1) * P, j * P:(j + 1) * P] = t
        bs = parts[0]["b"].copy()
        for r in range(1, world):
            bs = bs + parts[r]["b"]
    else:
        for q, (i, j) in enumerate(pairs):
            Hs[i * P:(i + 1) * P, j * P:(j + 1) * P] = parts[max(cons[q], 0)]["H"][(i, j)]
        bs = np.array([parts[max(po[i], 0)]["b"][i] for i in range(nP)])
        for k, q in enumerate(bl_idx):
            i, j = pairs[q]
            Hs[i * P:(i + 1) * P, j * P:(j + 1) * P] = Hsum[k]
        bs[bp_idx] = bsum
    for i in range(nP):
        Hs[i * P:(i + 1) * P, :i * P] = Hs[:i * P, i * P:(i + 1) * P].T
    xp = CH.scipy_cholesky_solve(Hs, bs.reshape(-1)).reshape(nP, P)
    xps = [xp.copy() for _ in range(world)]
    if len(halo) and path != "replicated":
        for r in range(world):
            other = [int(h) for h in halo if po[h] != r]
            if "halo_zero" in faults and other:
                xps[r][other[0]] = 0.0
            if "halo_swap" in faults and len(other) >= 2:
                xps[r][other[:2]] = xps[r][other[1::-1]]
    xl = np.zeros((nL, L))
    for r in range(world):
        a = parts[r]["a"]
        for j, w in enumerate(a["lists"]):
            rr = a["bl"][j].copy()
            for i in w:
                rr = rr - a["Hpl"][(i, j)].T @ xps[r][i]
            xl[a["my"][j]] = parts[r]["Dinv"][j] @ rr
    return dict(xp=xp, xps=xps, xl=xl, summands=summ, Hsum=Hsum, bsum=bsum, held=held, hkeep=hkeep, small=small, lists=(bl_idx, bp_idx, halo))


# ================================================================================================ the matrix-free operator
OPERATOR_CASE, OPERATOR_LAMBDA = "chain", 0                      # (case, index into LAMBDAS) of the operator test


def operator_vector(c):
    """The pinned dyadic vector the operator is applied to: [nP][6], entries of mixed magnitude."""
    rng = np.random.RandomState(8300)
    n = c["nP"] * P
    return (rng.randint(-7, 8, n) * 2.0 ** rng.randint(-6, 4, n)).reshape(c["nP"], P)


def all_pairs(pt, nP):
    return [(int(k % nP), int(k // nP)) for k in pt["keys"]]


def product(Hd, pairs, d):
    """[nP][6] of the symmetric block matrix {pair: block} (upper blocks) times d, accumulated in the pairs' order."""
    q = np.zeros_like(d)
    for (r, cc) in pairs:
        q[r] = q[r] + Hd[(r, cc)] @ d[cc]
        if r != cc:
            q[cc] = q[cc] + Hd[(r, cc)].T @ d[r]
    return q


def numpy_operator(c, pt, world, lam):
    """What every rank contributes in mode "pcg" (landmark ranges, rank 0 alone damps the poses), in fp64: per rank dict(diag
    [nP][6][6], b [nP][6], q [nP][6]) and their sums in rank order."""
    nP = c["nP"]
    pairs, d = all_pairs(pt, nP), operator_vector(c)
    parts = []
    for r in range(world):
        a = assemble(c, rank_landmarks(pt, c, world, r, "replicated"))
        Hd, b, _ = rank_schur(a, lam, np.full(nP, r == 0), pairs, np.arange(nP), nP)
        parts.append(dict(diag=np.array([Hd[(i, i)] for i in range(nP)]), b=b, q=product(Hd, pairs, d), touched=np.abs(a["Hpp"]).reshape(nP, -1).any(axis=1)))
    tot = {q: parts[0][q].copy() for q in ("diag", "b", "q")}
    for r in range(1, world):
        for q in tot:
            tot[q] = tot[q] + parts[r][q]
    return parts, tot


def load_operator():
    f = fixture()
    pre = OPERATOR_CASE + "/op/"
    out = {q: f[pre + q] for q in ("diag", "diag_s", "b", "b_s", "q", "q_s")}
    out["cpu"] = {(w, q): f["%sw%d/cpu_%s" % (pre, w, q)] for w in WORLDS for q in ("diag", "b", "q")}
    return out


def operator_bound(op, w, q):
    cpu = op["cpu"][(w, q)]
    return MARGIN * (float(cpu.max()) if float(cpu.max()) > 0 else 0.5), cpu


# ================================================================================================ measure
def figures(got, ref, scale):
    """max |got - ref| / (u s) per block; a block of scale 0 counts 0 if it is exactly 0 and inf otherwise."""
    got, ref, scale = np.asarray(got, np.float64), np.asarray(ref), np.asarray(scale, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if len(ref) == 0:
        return np.zeros(0)
    e = np.abs(got - ref).reshape(len(ref), -1).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, e / (U * np.where(scale > 0, scale, 1.0)), np.where(e == 0, 0.0, np.inf))


def solution_scales(c, lam, xp, xl):
    """(s of x_p per pose, s of x_l per landmark) in fp64 from reference quantities (the measure in the head)."""
    a = assemble(c)
    nP = c["nP"]
    Dm = a["Hll"] + lam * np.eye(L)
    Dinv = np.linalg.inv(Dm)
    Hs = np.zeros((nP * P, nP * P))
    for i in range(nP):
        Hs[i * P:(i + 1) * P, i * P:(i + 1) * P] = a["Hpp"][i] + lam * np.eye(P)
    sl = np.zeros(c["nL"])
    xp = np.asarray(xp).reshape(nP, P)
    for j, w in enumerate(a["lists"]):
        W = W_of(Dm[j], Dinv[j])
        t = np.abs(a["bl"][j])
        for k, i1 in enumerate(w):
            V = a["Hpl"][(i1, j)] @ Dinv[j]
            t = t + np.abs(a["Hpl"][(i1, j)]).T @ np.abs(xp[i1])
            for i2 in w:
                Hs[i1 * P:(i1 + 1) * P, i2 * P:(i2 + 1) * P] -= V @ a["Hpl"][(i2, j)].T
        sl[j] = (W @ t).max()
    Z = np.linalg.inv(Hs)
    return CH.scales(Hs, Z, xp.reshape(-1), P)[0], sl


def old_tolerances_pass(xp, xl, xp_ref, xl_ref, tol=1e-9):
    """The checks this replaces: tol max|x| over the whole vector, 1e-9 max|x_p| on the poses."""
    x, xr = np.r_[np.ravel(xp), np.ravel(xl)], np.r_[np.ravel(xp_ref), np.ravel(xl_ref)]
    return bool(np.abs(x - xr).max() <= tol * np.abs(xr).max() and np.abs(np.ravel(xp) - np.ravel(xp_ref)).max() <= 1e-9 * np.abs(xp_ref).max())


# ================================================================================================ fixture
def fixture():
    if "f" not in _cache:
        with np.load(FIXTURE) as f:
            _cache["f"] = {k: f[k] for k in f.files}
    return _cache["f"]


def load_case(name):
    """c (make_case at the stored size), per world the partition and census, and the stored references; read-only, shared."""
    if ("case", name) in _cache:
        return _cache[("case", name)]
    f = fixture()
    c = make_case(name, int(f["chain_cameras"]))
    k = dict(c=c, input_sha=str(f[name + "/input_sha"]), pt={}, census={}, x={}, sum={}, cpu={})
    for w in WORLDS:
        k["pt"][w] = partition(c["v1"], c["v0"].astype(np.int64) - c["nP"], c["nP"], c["nL"], w)
        k["census"][w] = {q: f["%s/w%d/census_%s" % (name, w, q)].tolist() for q in ("owned", "shared", "boundary", "bposes", "halo", "landmarks")}
    for i, lam in enumerate(LAMBDAS):
        g = lambda q: f["%s/lam%d/%s" % (name, i, q)].astype(np.float64)
        xr = g("x_hi"), g("x_lo")
        sp, sl = solution_scales(c, lam, xr[0][:c["nP"] * P], xr[0][c["nP"] * P:])
        k["x"][i] = dict(hi=xr[0], lo=xr[1], lo2=g("x_lo2"), sp=sp, sl=sl)
        for w in WORLDS:
            for path in ("subtree", "replicated"):
                for r in range(w):
                    pre = "%s/lam%d/w%d/%s/r%d/" % (name, i, w, path, r)
                    if pre + "H" in f:
                        k["sum"][(i, w, path, r)] = {q: f[pre + q] for q in ("H", "H_s", "b", "b_s")}
                for q in ("H", "b", "xp", "xl"):
                    key = "%s/lam%d/w%d/%s/cpu_%s" % (name, i, w, path, q)
                    if key in f:
                        k["cpu"][(i, w, path, q)] = f[key]
    _cache[("case", name)] = k
    return k


def bound(k, i, w, path, q):
    cpu = k["cpu"][(i, w, "replicated" if path == "replicated" else "subtree", q)]
    return MARGIN * (float(cpu.max()) if float(cpu.max()) > 0 else 0.5), cpu


def x_figures(k, i, xp, xl):
    """Per-pose and per-landmark figures of a solution against the 120-bit reference (x - hi first, then lo)."""
    r, n = k["x"][i], k["c"]["nP"] * P
    ep = np.abs((np.ravel(xp) - r["hi"][:n]) - r["lo"][:n]).reshape(-1, P).max(axis=1) / (U * r["sp"])
    el = np.abs((np.ravel(xl) - r["hi"][n:]) - r["lo"][n:]).reshape(-1, L).max(axis=1) / (U * r["sl"])
    return ep, el


# ================================================================================================ the lock-step driver
class NoComm:
    """The comm of a handle that is driven in lock-step: never called."""
    world, force = 0, False

    def __getattr__(self, name):
        raise AssertionError("the lock-step driver makes no collective call (%s)" % name)


def make_handles(c, world, path, torch_device):
    """`world` ShardedBlockSolvers in this process on the torch stream, built and (native halo paths) with the exchange set up."""
    from openslam_g2o_amd import distributed as DI
    hs = []
    for r in range(world):
        if path == "replicated":
            s = DI.ShardedBlockSolver(P, L, rank=r, world=world, comm=NoComm(), mode="replicated")
        else:
            s = DI.ShardedBlockSolver(P, L, rank=r, world=world, comm=NoComm(), mode="subtree", x_exchange="full" if path == "full" else "halo")
        s.setup_ba(c, torch_device=torch_device, fused=False)
        hs.append(s)
    if path == "halo_wide":
        pt = dict(pose_owner=hs[0].pose_owner, consumer=hs[0].consumer, boundary=hs[0].boundary, bposes=hs[0].bposes, halo=hs[0].halo,
                  keys=reduced_keys(c))
        b, bp, h = exchange_lists(pt, world, path)
        for s in hs:
            s.boundary, s.bposes, s.halo = b, bp, h
            _poison_foreign_halo(s, h)
    return hs


HALO_POISON = 0.5


def _poison_foreign_halo(s, halo):
    """A rank's landmarks never see a halo pose of the widened list, so its x_p there would be 0 and the `hmine` factor of
    exchange_halo_kernel would multiply nothing: just before pack(3) the x_p of the halo poses this rank does NOT own is set to
    HALO_POISON (on the solver's stream).  With the factor the sum is the owner's value and unpack(3) overwrites the poison."""
    import torch
    from openslam_g2o_amd import capi
    foreign = torch.from_numpy(np.asarray(halo)[s.pose_owner[halo] != s.rank].astype(np.int64))
    pack = s.local.exchangePack

    def poisoned_pack(which):
        if which == 3:
            x = s._device_tensor(capi.ARR_X)[:s.local.nP * P].view(-1, P)
            x[foreign.to(x.device)] = HALO_POISON
        pack(which)
    s.local.exchangePack = poisoned_pack


def reduced_keys(c):
    from openslam_g2o_amd import distributed as DI
    prow, pcol, _ = DI.coobservation_pairs(c["v1"], c["v0"].astype(np.int64) - c["nP"])
    return DI.reduced_pattern(prow, pcol, c["nP"])[2]


def lockstep_solve(hs, held=None):
    """Step the handles' own phase generators side by side.  At every collective: keep a copy of each rank's summand, sum them in
    fp64 in rank order 0 .. N-1 on the host and write the sum back to all of them.  Returns (status per rank, collectives): one
    entry per collective, a list over the buffers of it, each dict(summands [rank] array, total).
    held: a list; on the native halo paths it receives, per attempt, what every rank holds in its boundary blocks and boundary b_p
    after unpack(1): at the collective of the subtree roots (the first point where the driver has the ranks again) each rank
    runs exchange_pack(1) once more, which reads them from wherever the factorisation reads them, into ARR_XBOUNDARY.  (With
    sharded_merge = 1, the default, and every boundary shared -- the plain "halo" path -- ARR_XBOUNDARY is the tail of the
    subtree-root buffer that is about to be summed: the extra pack writes into it.  On the phased schedule nothing reads that
    tail after unpack(1), neither unpack_exchange nor the factorisation, so the sum of the held values that ends up there is
    never used.)"""
    import torch
    from openslam_g2o_amd import distributed as DI
    gens = [s.solve_phases() for s in hs]
    status, sent, log = [None] * len(hs), [None] * len(hs), []
    items = []
    for g in gens:
        items.append(next(g))
    while True:
        torch.cuda.synchronize()
        if isinstance(items[0], DI.LocalStatus):
            assert all(isinstance(it, DI.LocalStatus) for it in items)
            sent = [all(it.ok for it in items)] * len(hs)
        else:
            assert len(set(len(it) for it in items)) == 1
            if held is not None and all(getattr(s, "_native", False) and it[0] is s._nxbuf for s, it in zip(hs, items)):
                for s in hs:
                    s.local.exchangePack(1)
                torch.cuda.synchronize()
                held.append([s._nbuf1.detach().cpu().numpy().copy() for s in hs])
            entry = []
            for q in range(len(items[0])):
                summ = [it[q].detach().cpu().numpy().copy() for it in items]
                total = summ[0].copy()
                for v in summ[1:]:
                    total = total + v
                for it in items:
                    it[q].copy_(torch.from_numpy(total))
                entry.append(dict(summands=summ, total=total))
            torch.cuda.synchronize()
            log.append(entry)
            sent = [None] * len(hs)
        done = 0
        for r, g in enumerate(gens):
            try:
                items[r] = g.send(sent[r])
            except StopIteration as e:
                status[r] = e.value
                done += 1
        assert done in (0, len(hs)), "the ranks left the schedule at different collectives"
        if done:
            return status, log
