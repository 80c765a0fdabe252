"""Inputs, census, evaluations and the measure of the assembly-stage tests (tests/golden/make_assembly_blocks.py,
tests/test_assembly_reference_host.py, tests/test_gpu_assembly_blocks.py): the generic quadratic-form assembly of edge data
(J0, J1, Omega, e) into Hpp, Hpl, Hll and b, and the scalars of the LM loop (chi2, computeScale, H x).

INPUTS (NumPy only, fixed seeds).  A case is a solver family (p, l), vertex counts and a list of edge sets as addEdgeSet takes
them.  Every vertex has a scale 10^U(-3, 3) that multiplies its Jacobians, errors are drawn over the same decades, the
information is a full SPD matrix Q diag(s) Q' with condition up to 1e4, parallel edges come in nearly cancelling pairs.  Robust
edges get their squared error placed at a chosen ratio to delta^2 (DCS: to delta, where its switch delta + e2 = 2 delta sits) by
scaling the error; the generator asserts at 60 digits that every e2 keeps a relative 1e-6 from the switch or sits exactly on it
(identity information, dyadic error).  Two cases are exact on purpose: `chi2_exact` (dyadic errors, identity information, an
integer sum) and the pinned x of computeScale / multiplyHessian.

MEASURE.  A block of an output is held to its own operand sum s, evaluated at 60 digits:
    figure = max |got - ref| / (u s),   u = 2^-53,
    H block (i, j)    max entry of  sum_e |A|' w^_e |Omega| |B|
    b_v               max entry of  sum_e |J|' w^_e |Omega| |e|
    chi2              sum_e max(rho' |e|' |Omega| |e|, rho)
    computeScale      sum_i |x_i| (|lambda x_i| + |b_i|)
    (H x)_v           max entry of  (|H| + |lambda| I) |x|  over the block row
with w^_e = w_e (1 + kappa_e |d ln w / d ln e2|), kappa_e = (|e|' |Omega| |e|) / e2: the weight's own sensitivity to the rounding
of e2 is part of the scale.  No floor and no global scale; a block whose scale is 0 (no contributor, saturated weights only) must
be reproduced exactly.  The bound of (case, output) is 8 x the larger figure of two fp64 evaluations on the CPU that the fixture
records (0.5, one rounding, where both are 0): the oracle, and NumPy summing in the kernels' order (lane g of a vertex takes entries g, g + G, ..., then the butterfly
(l0 + l1) + (l2 + l3) ...; off-diagonal destinations entry by entry; later sets added to the stored block; chi2 and computeScale
as grid-stride partial sums, the workgroup tree, then the partials in order).

UNREACHABLE.  computeScale at vector size 1: the smallest handle is one pose of dimension 3 (BlockSolver's constructor takes
pose_dim 3, 6 or 7 and build_structure needs one pose), so the sizes are 3, 255, 257, 513.  Every row of both dispatch tables
is reached (UNREACHED_ROWS is empty)."""
import os
import re

import numpy as np

from tests.schur_helpers import MARGIN, ROOT, U, _ccs, sha256_of

FIXTURE = os.path.join(ROOT, "tests", "golden", "assembly_blocks.npz")
SOURCE = os.path.join(ROOT, "openslam_g2o_amd", "csrc", "block_solver.hip")
K_THREADS = 256                                                  # kThreads (csrc/common.h)
MAX_PARTIALS = 1024                                              # std::min(1024, grid_for(n)) of chi2() / compute_scale()
PART_NO_VERTEX0, PART_NO_VERTEX1, PART_NO_CHI2 = 1, 2, 4
THRESHOLD_MARGIN = 1e-6
RATIOS = (1e-8, 1e-2, 0.3, 3.0, 1e2, 1e8)                        # e2 / delta^2 (DCS: e2 / delta)
EDGE_DELTA = {1: 2.0, 2: 0.7, 3: 1.3, 4: 2.0, 5: 4.0}            # the delta of a kind where every edge brings its own kernel
UNREACHED_ROWS = {"vertex": (), "offdiag": ()}
SCALE_SIZES = (3, 255, 257, 513)
CHI2_DIMS = {1: 3, 2: 3, 3: 3, 6: 6, 7: 7}                       # error dimension -> pose dimension of the unary set
CHI2_SIZES = (1, 255, 256, 257, 513)
EXACT_N = 1024 * 256 + 257


def pick_group(avg):
    """pick_group of csrc/block_solver.hip (the host test holds this copy to the source)."""
    return 1 if avg <= 2.0 else (4 if avg <= 16.0 else 8)


def parse_tables():
    """(rows of dispatch_vertex, rows of dispatch_offdiag, thresholds of pick_group) read out of the source."""
    src = open(SOURCE).read()
    body = lambda name: src[src.index("void " + name + "("):].split("throw ArgFailure")[0]
    vert = [tuple(map(int, m)) for m in re.findall(r"row\(ic<(\d+)>, ic<(\d+)>\)", body("dispatch_vertex"))]
    off = [tuple(map(int, m)) for m in re.findall(r"row\(ic<(\d+)>, ic<(\d+)>, ic<(\d+)>\)", body("dispatch_offdiag"))]
    m = re.search(r"int pick_group\(double avg\) \{ return avg <= ([\d.]+) \? (\d+) : \(avg <= ([\d.]+) \? (\d+) : (\d+)\); \}", src)
    return vert, off, (float(m.group(1)), int(m.group(2)), float(m.group(3)), int(m.group(4)), int(m.group(5)))


# ================================================================================================ inputs
class _Case:
    def __init__(self, name, p, l, nP, nL, schur, seed):
        self.rng = np.random.RandomState(seed)
        self.c = dict(name=name, p=p, l=l, nP=nP, nL=nL, schur=schur, sets=[], multi=None, x=None, lams=(), kind="blocks")
        self.vs = 10.0 ** self.rng.uniform(-3, 3, nP + nL)

    def dim(self, v):
        free = None if v is None else v[v >= 0]
        return self.c["p"] if free is None or len(free) == 0 or free[0] < self.c["nP"] else self.c["l"]

    def omega(self, n, d, identity=False):
        if identity:
            return np.tile(np.eye(d).reshape(-1), (n, 1))
        out = np.zeros((n, d, d))
        for k in range(n):
            Q = np.linalg.qr(self.rng.randn(d, d))[0]
            M = (Q * 10.0 ** (self.rng.uniform(0, 4) * self.rng.uniform(0, 1, d))) @ Q.T * 10.0 ** self.rng.uniform(-2, 2)
            out[k] = 0.5 * (M + M.T)
        return out.reshape(n, d * d)

    def add(self, d, v0, v1=None, kind=0, delta=1.0, per_edge=False, parts=0, threshold_edges=0, share=None, plain_err=False):
        """One edge set.  per_edge: kinds k % 6 with EDGE_DELTA; threshold_edges: that many extra copies of the first edges whose e2
        sits exactly on the switch; share: (omega, err) of another set (the sets of one n-ary edge)."""
        rng, c = self.rng, self.c
        v0 = np.asarray(v0, np.int32)
        unary = v1 is None
        v1a = None if unary else np.asarray(v1, np.int32)
        if threshold_edges:
            v0 = np.concatenate([v0, v0[:threshold_edges]])
            v1a = None if unary else np.concatenate([v1a, v1a[:threshold_edges]])
        n = len(v0)
        d0, d1 = self.dim(v0), (0 if unary else self.dim(v1a))
        sc = lambda v: np.where(v >= 0, self.vs[np.maximum(v, 0)], 1.0)[:, None]
        J0 = rng.uniform(-1, 1, (n, d * d0)) * sc(v0)
        J1 = None if unary else rng.uniform(-1, 1, (n, d * d1)) * sc(v1a)
        if share is None:
            om = self.omega(n, d)
            err = rng.uniform(-1, 1, (n, d)) * (1.0 if plain_err else 10.0 ** rng.uniform(-3, 3, (n, 1)))
        else:
            om, err = share
        # parallel edges (same pair, consecutive) as nearly cancelling pairs
        if not unary and share is None:
            for k in range(1, n):
                if v0[k] == v0[k - 1] and v1a[k] == v1a[k - 1] and k % 2 == 1:
                    J0[k], om[k] = J0[k - 1], om[k - 1]
                    J1[k] = -J1[k - 1] * (1.0 + 2.0 ** -10 * rng.randint(1, 9))
                    err[k] = -err[k - 1] * (1.0 + 2.0 ** -9)
        kinds = deltas = None
        on_switch = np.zeros(n, bool)
        if per_edge:
            kinds = (np.arange(n) % 6).astype(np.int32)
            if threshold_edges:
                kinds[n - threshold_edges:] = np.array([1, 4, 5] * threshold_edges, np.int32)[:threshold_edges]
            deltas = np.array([EDGE_DELTA.get(int(k), 1.0) for k in kinds])
        if (per_edge or kind) and share is None:
            ratio = np.array(RATIOS)[rng.permutation(n) % len(RATIOS)]
            for k in range(n):
                kk, dd = (int(kinds[k]), float(deltas[k])) if per_edge else (kind, delta)
                if kk == 0:
                    continue
                O = om[k].reshape(d, d)
                e2 = float(err[k] @ O @ err[k])
                err[k] *= np.sqrt(ratio[k] * (dd if kk == 5 else dd * dd) / e2)
            if threshold_edges:                                  # e2 = 4 exactly: delta 2 (Huber, Saturated), phi 4 (DCS)
                sel = np.arange(n - threshold_edges, n)
                om[sel] = np.eye(d).reshape(-1)
                err[sel] = 0.0
                err[sel, 0] = 2.0
                on_switch[sel] = True
        c["sets"].append(dict(d=d, n=n, v0=v0, v1=v1a, d0=d0, d1=d1, J0=J0, J1=J1, om=om, err=err, kind=kind, delta=float(delta),
                              kinds=kinds, deltas=deltas, parts=parts, on_switch=on_switch))
        return c["sets"][-1]


def _pairs(rng, nA, nB, counts, offset, npairs=None):
    """Edges (a, offset + b): pair number i is repeated counts[i % len(counts)] times in a row (parallel edges)."""
    v0, v1 = [], []
    for i in range(npairs or max(nA, nB) * 2):
        a, b = int(rng.randint(nA)), int(rng.randint(nB))
        for _ in range(counts[i % len(counts)]):
            v0.append(a)
            v1.append(offset + b)
    return np.array(v0, np.int32), np.array(v1, np.int32)


def _family(name, p, l, nP, nL, seed, pose_ds, pl_ds, unary_pose_d, unary_lm_d, npairs=None):
    """A Schur family with every assembly row it reaches: pose-landmark sets in both vertex orders, pose-pose sets in both
    orders, an empty set in between, unary sets; pose nP - 1 and landmark nL - 1 have no contributor; destinations with 1, 2
    and 5 entries; every later set adds to the blocks of the first."""
    B = _Case(name, p, l, nP, nL, True, seed)
    rng = B.rng
    pa, lb = _pairs(rng, nP - 1, nL - 1, (1, 2, 5), nP, npairs)
    pa[::7] = -1                                                 # fixed cameras
    for i, d in enumerate(pl_ds):
        sel = slice(None) if i == 0 else slice(0, len(pa) // 2)
        if i % 2 == 0:
            B.add(d, lb[sel], pa[sel], kind=(1 if i == 0 else 0), delta=1.5)          # vertex 0 the landmark: stored transposed
        else:
            B.add(d, pa[sel], lb[sel])
        if i == 0:
            B.add(pl_ds[0], np.zeros(0, np.int32), np.zeros(0, np.int32))             # the empty set
    a, b = _pairs(rng, nP - 1, nP - 2, (1, 2, 5), 0)
    b = np.where(b >= a, b + 1, b).astype(np.int32)              # no self loops
    for i, d in enumerate(pose_ds):
        sel = slice(None) if i == 0 else slice(0, len(a) // 2)
        B.add(d, a[sel], b[sel], kind=(3 if i == 1 else 0), delta=0.8)
    if unary_pose_d:
        B.add(unary_pose_d, rng.randint(0, nP - 1, nP).astype(np.int32), None)
    if unary_lm_d:
        B.add(unary_lm_d, (nP + rng.randint(0, nL - 1, nL)).astype(np.int32), None)
    c = B.c
    c["x"] = rng.uniform(-1, 1, nP * p + nL * l) / np.repeat(B.vs, [p] * nP + [l] * nL)
    c["lams"] = ((0.0, 0.0), (float(np.float64(0.3) * B.vs[0] ** 2), float(np.float64(0.7) * B.vs[nP] ** 2)))
    return c


def _group_case(name, G, p, ds, seed):
    """Pose-only sets whose contributor lists have the lengths 0, 1, G - 1, G, G + 1, 3 G + 1 on the first six poses and a filler
    length on the others that puts the average where pick_group gives G; nV G is no multiple of 256, so the last workgroup ends in
    whole idle lane groups (v = gt / G: a lane group is never partly active; the idle groups run the butterfly on zeros)."""
    nV = {1: 70, 4: 65, 8: 33}[G]
    fill = {1: 2, 4: 6, 8: 20}[G]
    B = _Case(name, p, 0, nV, 0, False, seed)
    want = np.array([0, 1, G - 1, G, G + 1, 3 * G + 1] + [fill] * (nV - 6))
    a = np.arange(6, 20, dtype=np.int32)                          # a short chain: the off-diagonal kernel beside the vertex kernel
    b = a + 1
    a[::3], b[::3] = b[::3].copy(), a[::3].copy()                # every third edge with v0 > v1
    deg = np.bincount(np.concatenate([a, b]), minlength=nV)
    v0, v1 = list(a), list(b)
    for v in range(nV):
        for i in range(max(0, int(want[v] - deg[v]))):           # half-fixed edges on alternating sides fill the lists up
            v0.append(v if i % 2 == 0 else -1)
            v1.append(-1 if i % 2 == 0 else v)
    order = B.rng.permutation(len(v0))
    v0, v1 = np.array(v0, np.int32)[order], np.array(v1, np.int32)[order]
    for i, d in enumerate(ds):
        B.add(d, v0, v1, kind=(2 if i == 0 else 0), delta=1.1)
    B.c["want"] = np.maximum(want, deg)
    B.c["G"] = G
    return B.c


def _chi2_case(D, n, seed):
    p = CHI2_DIMS[D]
    B = _Case("chi2_D%d_n%d" % (D, n), p, 0, 2, 0, False, seed)
    B.add(D, (np.arange(n) % 2).astype(np.int32), None, per_edge=True)
    B.c["kind"] = "chi2"
    return B.c


def _exact_case():
    """kind 0, D = 1, identity information, errors k / 8: e2 = k^2 / 64 and every partial sum an integer / 64 below 2^53."""
    B = _Case("chi2_exact", 3, 0, 2, 0, False, 9100)
    n = EXACT_N
    err = B.rng.randint(-64, 65, (n, 1)) / 8.0
    B.c["sets"].append(dict(d=1, n=n, v0=(np.arange(n) % 2).astype(np.int32), v1=None, d0=3, d1=0,
                            J0=B.rng.randint(-3, 4, (n, 3)).astype(np.float64), J1=None, om=np.ones((n, 1)), err=err, kind=0, delta=1.0,
                            kinds=None, deltas=None, parts=0, on_switch=np.zeros(n, bool)))
    B.c["kind"] = "exact"
    return B.c


def _scale_case(size, seed):
    """b exact (one unary edge per vertex, identity information, dyadic Jacobian and error), x and lambda pinned and not dyadic,
    lambda x and b of opposite sign on a third of the entries."""
    nP, nL = (size // 3, 0) if size % 3 == 0 else ((size - 2) // 3, 1)
    l = 2 if nL else 0
    B = _Case("scale_n%d" % size, 3, l, nP, nL, False, seed)
    rng = B.rng
    for d, lo, nv in ((3, 0, nP), (2, nP, nL)):
        if nv == 0:
            continue
        dim = 3 if lo == 0 else 2
        B.c["sets"].append(dict(d=d, n=nv, v0=np.arange(lo, lo + nv, dtype=np.int32), v1=None, d0=dim, d1=0,
                                J0=rng.randint(-3, 4, (nv, d * dim)).astype(np.float64), J1=None, om=np.tile(np.eye(d).reshape(-1), (nv, 1)),
                                err=rng.randint(-16, 17, (nv, d)) / 8.0, kind=0, delta=1.0, kinds=None, deltas=None, parts=0,
                                on_switch=np.zeros(nv, bool)))
    b = np.concatenate([-np.einsum("nad,nd->na", e["J0"].reshape(e["n"], e["d0"], e["d"]), e["err"]).reshape(-1) for e in B.c["sets"]])
    x = np.abs(rng.uniform(-1, 1, size)) * 10.0 ** rng.uniform(-2, 2, size)
    sign = np.where(b < 0, -1.0, 1.0) * np.where(np.arange(size) % 3 == 0, -1.0, 1.0)
    B.c["x"], B.c["b_exact"], B.c["lam"] = x * sign, b, 0.37
    B.c["kind"] = "scale"
    return B.c


def _nary_case():
    """Three-vertex edges (point, pose, anchor) as the three binary sets ba_psi.inc documents: (point, pose) parts 0,
    (point, anchor) parts NO_VERTEX0 | NO_VERTEX1 | NO_CHI2, (pose, anchor) parts NO_VERTEX0 | NO_CHI2; Huber on all three."""
    nP, nL, n = 10, 14, 40
    B = _Case("nary_6_3", 6, 3, nP, nL, True, 9200)
    rng = B.rng
    pt = (nP + rng.randint(0, nL, n)).astype(np.int32)
    pose = rng.randint(0, nP, n).astype(np.int32)
    anchor = ((pose + 1 + rng.randint(0, nP - 1, n)) % nP).astype(np.int32)
    pose[::9] = -1
    s0 = B.add(2, pt, pose, kind=1, delta=1.0)
    sh = (s0["om"], s0["err"])
    s1 = B.add(2, pt, anchor, kind=1, delta=1.0, parts=7, share=sh)
    s2 = B.add(2, pose, anchor, kind=1, delta=1.0, parts=5, share=sh)
    s1["J0"] = s0["J0"]
    s2["J0"], s2["J1"] = s0["J1"], s1["J1"]
    B.c["multi"] = dict(sets=(0, 1, 2), verts=np.stack([pt, pose, anchor], axis=1).astype(np.int32))
    return B.c


def _robust_set_case():
    B = _Case("robust_set", 6, 3, 6, 10, True, 9300)
    rng = B.rng
    for kind in (1, 2, 3, 4, 5):
        lm = (6 + rng.randint(0, 10, 36)).astype(np.int32)
        ps = rng.randint(0, 6, 36).astype(np.int32)
        B.add(2, lm, ps, kind=kind, delta=(0.9, 2.5, 0.4, 1.7, 3.0)[kind - 1])
    return B.c


def _robust_edge_case():
    B = _Case("robust_edge", 6, 3, 6, 10, True, 9301)
    rng = B.rng
    B.add(3, rng.randint(0, 6, 48).astype(np.int32), (6 + rng.randint(0, 10, 48)).astype(np.int32), per_edge=True, threshold_edges=6)
    a = rng.randint(0, 6, 36).astype(np.int32)
    b = ((a + 1 + rng.randint(0, 5, 36)) % 6).astype(np.int32)
    B.add(6, a, b, per_edge=True, threshold_edges=3)
    return B.c


def _robust_single_case():
    """One edge per block: pose-pose edges (2 k, 2 k + 1), every second one given as (2 k + 1, 2 k); every edge its own kernel."""
    n = 36
    B = _Case("robust_single", 3, 0, 2 * n, 0, False, 9302)
    a, b = 2 * np.arange(n, dtype=np.int32), 2 * np.arange(n, dtype=np.int32) + 1
    a[1::2], b[1::2] = b[1::2].copy(), a[1::2].copy()
    B.add(3, a, b, per_edge=True, plain_err=True)
    B.c["kind"] = "single"
    return B.c


def _builders():
    t = {
        "fam_6_3": lambda: _family("fam_6_3", 6, 3, 12, 20, 9001, (6, 1, 2, 3), (2, 3, 1), 6, 3),
        "fam_3_2": lambda: _family("fam_3_2", 3, 2, 40, 110, 9002, (3, 2), (2, 1), 1, 3, npairs=340),
        "fam_7_3": lambda: _family("fam_7_3", 7, 3, 8, 12, 9003, (7,), (2, 3), 0, 0),
        "fam_3_3": lambda: _family("fam_3_3", 3, 3, 8, 12, 9004, (3,), (3, 2), 0, 0),
        "nary_6_3": _nary_case, "robust_set": _robust_set_case, "robust_edge": _robust_edge_case, "robust_single": _robust_single_case,
        "chi2_exact": _exact_case,
    }
    for gi, G in enumerate((1, 4, 8)):
        t["g%d_p3" % G] = lambda G=G, gi=gi: _group_case("g%d_p3" % G, G, 3, (2,), 9400 + gi)
        t["g%d_p6" % G] = lambda G=G, gi=gi: _group_case("g%d_p6" % G, G, 6, (2, 3, 6, 1), 9410 + gi)
        t["g%d_p7" % G] = lambda G=G, gi=gi: _group_case("g%d_p7" % G, G, 7, (7,), 9420 + gi)
    for i, D in enumerate(sorted(CHI2_DIMS)):
        for j, n in enumerate(CHI2_SIZES):
            t["chi2_D%d_n%d" % (D, n)] = lambda D=D, n=n, s=9500 + 10 * i + j: _chi2_case(D, n, s)
    for i, size in enumerate(SCALE_SIZES):
        t["scale_n%d" % size] = lambda size=size, s=9600 + i: _scale_case(size, s)
    return t


BUILDERS = _builders()
NAMES = sorted(BUILDERS)
HX_CASES = ("fam_6_3", "fam_3_2", "fam_7_3")
_cases = {}


def make_case(name):
    if name not in _cases:
        c = BUILDERS[name]()
        for s in c["sets"]:
            for v in s.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _cases[name] = c
    return _cases[name]


def input_hash(c):
    arr = [np.array([c["p"], c["l"], c["nP"], c["nL"], int(c["schur"])])]
    for s in c["sets"]:
        arr.append(np.array([s["d"], s["n"], s["kind"], s["parts"]]))
        arr.append(np.float64(s["delta"]))
        arr += [s[k] for k in ("v0", "v1", "J0", "J1", "om", "err", "kinds", "deltas") if s[k] is not None]
    if c["x"] is not None:
        arr.append(c["x"])
    return sha256_of(arr)


def outputs_of(c):
    """The outputs a case holds by figure."""
    if c["kind"] == "chi2":
        return ("chi2",)
    if c["kind"] == "scale":
        return ("scale",)
    if c["kind"] == "exact":
        return ()
    out = ["Hpp", "b", "chi2"] + (["Hpl", "Hll"] if c["nL"] else [])
    if c["kind"] == "single":
        out += ["w_diag", "w_off"]                               # (w_diag: every edge twice, vertex 0 then vertex 1)
    if c["name"] in HX_CASES:
        out += ["Hx0", "Hx1"]
    return tuple(out)


# ================================================================================================ structure and census
def structure(c):
    """What build_structure derives: the patterns pp / pl as (colptr, rowidx, slots) and per set the contributor lists in edge
    order -- vp[v] / vl[j] = [(edge, side)], op / ol {destination block: [(edge, transposed)]} -- with the lane-group widths."""
    nP, nL = c["nP"], c["nL"]
    kpp, kpl = [(i, i) for i in range(nP)], []
    for s in c["sets"]:
        if s["v1"] is None:
            continue
        for a, b in zip(s["v0"].tolist(), s["v1"].tolist()):
            if a < 0 or b < 0:
                continue
            if a < nP and b < nP:
                kpp.append((min(a, b), max(a, b)))
            else:
                kpl.append((b, a - nP) if a >= nP else (a, b - nP))
    pp, pl = _ccs(nP, kpp), _ccs(max(nL, 0), kpl)
    per = []
    for s in c["sets"]:
        vp, vl, op, ol = [[] for _ in range(nP)], [[] for _ in range(nL)], {}, {}
        v1 = s["v1"] if s["v1"] is not None else np.full(s["n"], -1)
        for k, (a, b) in enumerate(zip(s["v0"].tolist(), v1.tolist())):
            for side, v, bit in ((0, a, 1), (1, b, 2)):
                if v >= 0 and not s["parts"] & bit:
                    (vl[v - nP] if v >= nP else vp[v]).append((k, side))
            if a >= 0 and b >= 0:
                if a < nP and b < nP:
                    op.setdefault(pp[2][(min(a, b), max(a, b))], []).append((k, a > b))
                else:
                    ol.setdefault(pl[2][(b, a - nP) if a >= nP else (a, b - nP)], []).append((k, a >= nP))
        n_vp, n_vl = sum(map(len, vp)), sum(map(len, vl))
        per.append(dict(vp=vp, vl=vl, op=op, ol=ol, Gp=pick_group(n_vp / max(1, nP)) if n_vp else None,
                        Gl=pick_group(n_vl / max(1, nL)) if n_vl else None))
    return dict(pp=pp, pl=pl, per=per)


def rows_reached(c, st):
    """(vertex rows (d, dv), off-diagonal rows (d, rows, cols)) the case launches."""
    vert, off = set(), set()
    for s, q in zip(c["sets"], st["per"]):
        if s["n"] == 0:
            continue
        if q["Gp"]:
            vert.add((s["d"], c["p"]))
        if q["Gl"]:
            vert.add((s["d"], c["l"]))
        if q["op"]:
            off.add((s["d"], c["p"], c["p"]))
        if q["ol"]:
            off.add((s["d"], c["p"], c["l"]))
    return vert, off


def census(c, st):
    """Per case: the lane-group widths with the rows they run on, contributor-list lengths, entries per destination, transposed
    entries."""
    out = dict(groups=set(), lens=set(), dst=set(), tr_pp=0, tr_pl=0, plain_pl=0, n_op=0, n_ol=0)
    for s, q in zip(c["sets"], st["per"]):
        if s["n"] == 0:
            continue
        if q["Gp"]:
            out["groups"].add((q["Gp"], s["d"], c["p"]))
            out["lens"] |= set(len(w) for w in q["vp"])
        if q["Gl"]:
            out["groups"].add((q["Gl"], s["d"], c["l"]))
        for w in list(q["op"].values()) + list(q["ol"].values()):
            out["dst"].add(len(w))
        out["tr_pp"] += sum(t for w in q["op"].values() for _, t in w)
        out["tr_pl"] += sum(t for w in q["ol"].values() for _, t in w)
        out["plain_pl"] += sum(not t for w in q["ol"].values() for _, t in w)
        out["n_op"], out["n_ol"] = max(out["n_op"], len(st["pp"][1]) - c["nP"]), max(out["n_ol"], len(st["pl"][1]))
    return out


# ================================================================================================ evaluation
def _kernel_of(s, k):
    return (int(s["kinds"][k]), float(s["deltas"][k])) if s["kinds"] is not None else (s["kind"], s["delta"])


def robust_fp64(kind, delta, e2):
    """(rho, rho') as the kernels write them in fp64 (robust_rho / robust_weight of csrc/block_solver.hip)."""
    dsqr = delta * delta
    if kind == 1:
        return (e2, 1.0) if e2 <= dsqr else (2.0 * np.sqrt(e2) * delta - dsqr, delta / np.sqrt(e2))
    if kind == 2:
        return 2.0 * dsqr * (np.sqrt(e2 / dsqr + 1.0) - 1.0), 1.0 / np.sqrt(e2 / dsqr + 1.0)
    if kind == 3:
        return dsqr * np.log(e2 / dsqr + 1.0), 1.0 / (e2 / dsqr + 1.0)
    if kind == 4:
        return (e2, 1.0) if e2 <= dsqr else (dsqr, 0.0)
    if kind == 5:
        sc = min((2.0 * delta) / (delta + e2), 1.0)
        return sc * e2 * sc, sc * sc
    return e2, 1.0


def weight_sensitivity(kind, delta, e2):
    """|d ln rho' / d ln e2| (any number type)."""
    d2 = delta * delta
    if kind == 1:
        return 0 if e2 <= d2 else 0.5
    if kind == 2:
        return (e2 / d2) / (1 + e2 / d2) / 2
    if kind == 3:
        return (e2 / d2) / (1 + e2 / d2)
    if kind == 5:
        return 0 if 2 * delta >= delta + e2 else 2 * e2 / (delta + e2)
    return 0


def _mm_t(A, M):
    """[n][d][a]' [n][d][b] -> [n][a][b], sums over d in order, elementwise operations only (no BLAS: the same bits everywhere)."""
    out = A[:, 0, :, None] * M[:, 0, None, :]
    for i in range(1, A.shape[1]):
        out = out + A[:, i, :, None] * M[:, i, None, :]
    return out


def _mm(O, J):
    """[n][d][d] [n][d][a] -> [n][d][a]."""
    out = O[:, :, 0, None] * J[:, 0, None, :]
    for j in range(1, O.shape[2]):
        out = out + O[:, :, j, None] * J[:, j, None, :]
    return out


def _lane_sum(terms, G, zero):
    lanes = []
    for g in range(G):
        acc = zero
        for t in terms[g::G]:
            acc = acc + t
        lanes.append(acc)
    while len(lanes) > 1:
        lanes = [lanes[i] + lanes[i + 1] for i in range(0, len(lanes), 2)]
    return lanes[0]


def _grid_sum(v, zero):
    """Grid-stride partial sums over min(1024, ceil(n / 256)) workgroups of 256, the workgroup's tree, the partials in order."""
    n = len(v)
    nb = min(MAX_PARTIALS, (n + K_THREADS - 1) // K_THREADS)
    per = nb * K_THREADS
    pad = np.concatenate([v, np.full((-n) % per, zero, dtype=v.dtype)]).reshape(-1, nb, K_THREADS)
    s = np.full((nb, K_THREADS), zero, dtype=v.dtype)
    for it in range(pad.shape[0]):
        s = s + pad[it]
    o = K_THREADS // 2
    while o > 0:
        s = s[:, :o] + s[:, o:2 * o]
        o //= 2
    tot = zero
    for b in range(nb):
        tot = tot + s[b, 0]
    return tot


def evaluate(c, st, mode, want_blocks=True):
    """The assembly of a case, summed in the kernels' order: mode "np" in fp64, mode "mp" at 60 digits with the scales.
    dict(Hpp [nnz][p][p] (row, column), Hpl [nnz][p][l], Hll [nL][l][l], bp [nP][p], bl [nL][l], chi2, w [set][edge]) and in
    mode "mp" the same names with the suffix _s."""
    mpm = mode == "mp"
    if mpm:
        import mpmath as mp
        from tests import reference_mp as R
        conv = np.vectorize(lambda v: mp.mpf(float(v)), otypes=[object])
        zero = mp.mpf(0)
        dt = object
    else:
        conv, zero, dt = (lambda a: np.asarray(a, np.float64)), 0.0, np.float64
    p, l, nP, nL = c["p"], c["l"], c["nP"], c["nL"]
    Z = lambda *shape: np.full(shape, zero, dtype=dt)
    names = dict(Hpp=(len(st["pp"][1]), p, p), Hpl=(len(st["pl"][1]), p, l), Hll=(nL, l, l), bp=(nP, p), bl=(nL, l))
    out = {k: Z(*shp) for k, shp in names.items()}
    if mpm:
        out.update({k + "_s": Z(*shp) for k, shp in names.items()})
        out["chi2_s"] = zero
    out["chi2"] = zero
    out["w"] = []
    for s, q in zip(c["sets"], st["per"]):
        n, d = s["n"], s["d"]
        if n == 0:
            out["w"].append(np.zeros(0))
            continue
        O = conv(s["om"]).reshape(n, d, d).transpose(0, 2, 1)
        r = conv(s["err"])
        Or = _mm(O, r[:, :, None])[:, :, 0]
        e2 = (r * Or).sum(axis=1) if mpm else _mm_t(r[:, :, None], Or[:, :, None])[:, 0, 0]
        w, rho, what = Z(n), Z(n), Z(n)
        aO, ar = np.abs(O), np.abs(r)
        aOr = _mm(aO, ar[:, :, None])[:, :, 0]
        for k in range(n):
            kind, delta = _kernel_of(s, k)
            if mpm:
                rho[k], w[k] = R.robust(kind, delta, e2[k])
                kappa = (ar[k] * aOr[k]).sum() / e2[k] if e2[k] != 0 else zero
                what[k] = w[k] * (1 + kappa * weight_sensitivity(kind, mp.mpf(delta), e2[k]))
                out["chi2_s"] = out["chi2_s"] + (0 if s["parts"] & 4 else max(w[k] * (ar[k] * aOr[k]).sum(), rho[k]))
            else:
                rho[k], w[k] = robust_fp64(kind, delta, float(e2[k]))
        out["w"].append(w)
        if not s["parts"] & 4:
            out["chi2"] = out["chi2"] + (rho.sum() if mpm else _grid_sum(rho, 0.0))
        if not want_blocks:
            continue
        J = [conv(s["J0"]).reshape(n, s["d0"], d).transpose(0, 2, 1),
             None if s["J1"] is None else conv(s["J1"]).reshape(n, s["d1"], d).transpose(0, 2, 1)]
        wO = lambda M, ww: ww[:, None, None] * M
        diag, rhs, diag_s, rhs_s = [None, None], [None, None], [None, None], [None, None]
        for side in (0, 1):
            if J[side] is None:
                continue
            diag[side] = _mm_t(J[side], wO(_mm(O, J[side]), w))
            rhs[side] = zero - w[:, None] * _mm_t(J[side], Or[:, :, None])[:, :, 0]
            if mpm:
                aJ = np.abs(J[side])
                diag_s[side] = _mm_t(aJ, wO(_mm(aO, aJ), what))
                rhs_s[side] = what[:, None] * _mm_t(aJ, aOr[:, :, None])[:, :, 0]
        for lists, G, Hn, bn, slot in ((q["vp"], q["Gp"], "Hpp", "bp", lambda v: st["pp"][2][(v, v)]), (q["vl"], q["Gl"], "Hll", "bl", lambda v: v)):
            if not G:
                continue
            for v, w_ in enumerate(lists):
                if not w_:
                    continue
                out[Hn][slot(v)] = out[Hn][slot(v)] + _lane_sum([diag[sd][k] for k, sd in w_], G, zero)
                out[bn][v] = out[bn][v] + _lane_sum([rhs[sd][k] for k, sd in w_], G, zero)
                if mpm:
                    out[Hn + "_s"][slot(v)] = out[Hn + "_s"][slot(v)] + sum(diag_s[sd][k] for k, sd in w_)
                    out[bn + "_s"][v] = out[bn + "_s"][v] + sum(rhs_s[sd][k] for k, sd in w_)
        if J[1] is not None and (q["op"] or q["ol"]):
            off = [_mm_t(J[0], wO(_mm(O, J[1]), w)), _mm_t(J[1], wO(_mm(O, J[0]), w))]      # plain, transposed
            if mpm:
                aJ0, aJ1 = np.abs(J[0]), np.abs(J[1])
                off_s = [_mm_t(aJ0, wO(_mm(aO, aJ1), what)), _mm_t(aJ1, wO(_mm(aO, aJ0), what))]
            for dsts, Hn in ((q["op"], "Hpp"), (q["ol"], "Hpl")):
                for blk, w_ in dsts.items():
                    out[Hn][blk] = out[Hn][blk] + _lane_sum([off[int(t)][k] for k, t in w_], 1, zero)
                    if mpm:
                        out[Hn + "_s"][blk] = out[Hn + "_s"][blk] + sum(off_s[int(t)][k] for k, t in w_)
    return out


def multiply(c, st, ev, x, lam, dt=np.float64, absolute=False):
    """H x of the assembled blocks (upper block patterns, symmetric), damping (lambda_pose, lambda_landmark) on the diagonal:
    per vertex block [nP + nL] rows of dimension p / l as one flat vector.  absolute: (|H| + |lambda|) |x|."""
    p, l, nP, nL = c["p"], c["l"], c["nP"], c["nL"]
    f = np.abs if absolute else (lambda a: a)
    x = f(np.asarray(x, dtype=dt))
    y = np.concatenate([np.full(nP * p, f(lam[0]), dtype=dt), np.full(nL * l, f(lam[1]), dtype=dt)]) * x
    xp, xl = x[:nP * p].reshape(nP, p), x[nP * p:].reshape(nL, l)
    yp, yl = y[:nP * p].reshape(nP, p), y[nP * p:].reshape(nL, l)

    def mv(B, v):
        acc = B[:, 0] * v[0]
        for j in range(1, B.shape[1]):
            acc = acc + B[:, j] * v[j]
        return acc
    cp, ri, _ = st["pp"]
    for col in range(nP):
        for qq in range(cp[col], cp[col + 1]):
            B, r = f(ev["Hpp"][qq]), ri[qq]
            yp[r] = yp[r] + mv(B, xp[col])
            if r != col:
                yp[col] = yp[col] + mv(B.T, xp[r])
    cp, ri, _ = st["pl"]
    for col in range(nL):
        for qq in range(cp[col], cp[col + 1]):
            B, r = f(ev["Hpl"][qq]), ri[qq]
            yp[r] = yp[r] + mv(B, xl[col])
            yl[col] = yl[col] + mv(B.T, xp[r])
        yl[col] = yl[col] + mv(f(ev["Hll"][col]), xl[col])
    return y


def single_blocks(c, st):
    """robust_single: per edge (block of its vertex 0, its off-diagonal block, transposed, block of its vertex 1)."""
    e, slots = c["sets"][0], st["pp"][2]
    return [(slots[(int(a), int(a))], slots[(int(min(a, b)), int(max(a, b)))], bool(a > b), slots[(int(b), int(b))])
            for a, b in zip(e["v0"], e["v1"])]


def weights_from_blocks(c, st, Hpp, idx, M):
    """robust_single: per edge the weight its diagonal blocks (row 0: vertex 0, the J0 side of the vertex kernel; row 2: vertex 1,
    the J1 side) and its off-diagonal block (row 1) were assembled with, read back as H[i] / (A' Omega B)[i] at the entries
    idx [3][n][2] with the least cancellation; M [3][n] those entries of A' Omega B (60 digits, rounded)."""
    out = np.zeros((3, len(M[0])))
    for k, (q0, qo, _, q1) in enumerate(single_blocks(c, st)):
        for row, q in enumerate((q0, qo, q1)):
            out[row, k] = Hpp[q][tuple(idx[row][k])] / M[row][k]
    return out


def threshold_census(c):
    """(robust edges, edges exactly on their switch, edges closer than THRESHOLD_MARGIN to it without sitting on it), e2 at 60
    digits: the switch is e2 = delta^2 (Huber, Saturated) or e2 = delta (DCS); PseudoHuber and Cauchy have none."""
    import mpmath as mp
    from tests import reference_mp  # noqa: F401  (sets the working precision)
    n_rob = n_on = n_bad = 0
    for s in c["sets"]:
        d = s["d"]
        for k in range(s["n"]):
            kind, delta = _kernel_of(s, k)
            if kind == 0:
                continue
            n_rob += 1
            if kind in (2, 3):
                continue
            O = [[mp.mpf(float(s["om"][k][i + d * j])) for j in range(d)] for i in range(d)]
            r = [mp.mpf(float(v)) for v in s["err"][k]]
            e2 = sum(r[i] * O[i][j] * r[j] for i in range(d) for j in range(d))
            sw = mp.mpf(delta) if kind == 5 else mp.mpf(delta) ** 2
            if e2 == sw:
                n_on += 1
            elif abs(e2 - sw) < THRESHOLD_MARGIN * sw:
                n_bad += 1
    return n_rob, n_on, n_bad


# ================================================================================================ fixture and measure
_cache = {}


def fixture():
    if "f" not in _cache:
        with np.load(FIXTURE) as f:
            _cache["f"] = {k: f[k] for k in f.files}
    return _cache["f"]


def blocks_of(c, ev):
    """An evaluation's arrays under the names of the outputs: b = pose blocks then landmark blocks, as lists of blocks."""
    out = {k: ev[k] for k in ("Hpp", "Hpl", "Hll") if k in ev and len(ev[k])}
    if "bp" in ev:
        out["b"] = [v for v in ev["bp"]] + [v for v in ev["bl"]]
    return out


def figures(got, ref, scale):
    """max |got - ref| / (u s) per block (lists of arrays or scalars); a block of scale 0 has to be reproduced exactly."""
    f = np.zeros(len(ref))
    for i, (g, r, s) in enumerate(zip(got, ref, scale)):
        err = float(np.max(np.abs(np.asarray(g, np.float64) - np.asarray(r, np.float64))))
        f[i] = (0.0 if err == 0.0 else np.inf) if s == 0 else err / (U * float(s))
    return f


def split_b(c, b):
    nP, p, nL, l = c["nP"], c["p"], c["nL"], c["l"]
    return [v for v in np.asarray(b[:nP * p]).reshape(nP, p)] + [v for v in np.asarray(b[nP * p:]).reshape(nL, l)]


def load_case(name):
    """c, st, ref {output: blocks}, scale {output: per block}, cpu {output: (oracle, numpy)}, bound {output}."""
    if name in _cache:
        return _cache[name]
    f = fixture()
    c = make_case(name)
    st = structure(c)
    g = lambda k: f[name + "/" + k]
    k = dict(name=name, c=c, st=st, input_sha=str(g("input_sha")), ref={}, scale={}, cpu={}, bound={})
    for o in outputs_of(c):
        ref = g(o)
        if o in ("b", "Hx0", "Hx1"):
            ref = split_b(c, ref)
        k["ref"][o], k["scale"][o] = ref, g(o + "_s")
        k["cpu"][o] = (float(g(o + "_cpu")[0]), float(g(o + "_cpu")[1]))
        k["bound"][o] = MARGIN * max(max(k["cpu"][o]), float(g(o + "_floor")))
    _cache[name] = k
    return k


def device_outputs(c, st, Hpp, Hpl, Hll, b, chi2):
    """Library arrays (column-major blocks) -> the outputs' blocks."""
    p, l = c["p"], c["l"]
    out = dict(Hpp=np.asarray(Hpp).reshape(-1, p, p).transpose(0, 2, 1), b=split_b(c, b), chi2=[chi2])
    if c["nL"]:
        out["Hpl"] = np.asarray(Hpl).reshape(-1, l, p).transpose(0, 2, 1)
        out["Hll"] = np.asarray(Hll).reshape(-1, l, l).transpose(0, 2, 1)
    return out


# ================================================================================================ fp64 on the CPU
def oracle_solver(O, c):
    """oracle.OracleSolver with the case's edges, built.  A set whose edges bring their own kernels becomes one oracle set per
    (kind, delta); the three sets of an n-ary arrangement become one multi-edge set."""
    o = O.OracleSolver(c["p"], c["l"], c["nP"], c["nL"], c["schur"])
    skip = c["multi"]["sets"] if c["multi"] else ()
    todo = []
    for i, s in enumerate(c["sets"]):
        if s["n"] == 0 or i in skip:
            continue
        groups = [(s["kind"], s["delta"], np.arange(s["n"]))] if s["kinds"] is None else \
            [(int(kk), EDGE_DELTA.get(int(kk), 1.0), np.flatnonzero(s["kinds"] == kk)) for kk in np.unique(s["kinds"])]
        for kind, delta, sel in groups:
            q = o.add_edge_set(s["d"], s["v0"][sel], None if s["v1"] is None else s["v1"][sel])
            o.set_dims(q, s["d0"], s["d1"])
            todo.append((q, s, sel, kind, delta))
    if c["multi"]:
        m = o.add_multi_edge_set(c["sets"][0]["d"], c["multi"]["verts"])
    o.build_structure()
    for q, s, sel, kind, delta in todo:
        o.set_edge_data(q, s["J0"][sel], None if s["J1"] is None else s["J1"][sel], s["om"][sel], s["err"][sel], delta if kind else 0.0)
        if kind:
            o.set_robust_kernel(q, kind)
    if c["multi"]:
        s0, s1, s2 = (c["sets"][i] for i in c["multi"]["sets"])
        o.set_multi_edge_data(m, [s0["J0"], s0["J1"], s1["J1"]], s0["om"], s0["err"], s0["delta"], s0["kind"])
    o.build_system()
    return o


def oracle_evaluation(O, c, st):
    o = oracle_solver(O, c)
    for which in ("pp",) + (("pl",) if c["nL"] else ()):
        cp, ri = o.pattern(which)
        assert np.array_equal(cp, st[which][0]) and np.array_equal(ri, st[which][1]), which
    out = device_outputs(c, st, o.values("Hpp"), o.values("Hpl") if c["nL"] else None, o.values("Hll") if c["nL"] else None, o.b(), o.chi2())
    out["_o"] = o
    return out


def numpy_outputs(c, st, ev):
    out = blocks_of(c, ev)
    out["chi2"] = [ev["chi2"]]
    return out


def scale_numpy(c, b):
    x = c["x"]
    return _grid_sum(x * (c["lam"] * x + b), 0.0)


# ================================================================================================ the device
def device_solver(capi, c, schur=None):
    """HipBlockSolver with the case's edge sets, parts and kernels, structure built, edge data set (buildSystem is the caller's)."""
    s = capi.HipBlockSolver(c["p"], c["l"], 0)
    ids = [s.addEdgeSet(e["d"], e["v0"], e["v1"]) for e in c["sets"]]
    for q, e in zip(ids, c["sets"]):
        if e["parts"]:
            s.setEdgeSetParts(q, e["parts"])
    s.buildStructure(c["nP"], c["nL"], c["schur"] if schur is None else schur)
    for q, e in zip(ids, c["sets"]):
        if e["n"] == 0:
            continue
        s.setEdgeData(q, e["J0"], e["J1"], e["om"], e["err"])
        if e["kinds"] is not None:
            s.setRobustKernelPerEdge(q, e["kinds"], e["deltas"])
        elif e["kind"]:
            s.setRobustKernel(q, e["kind"], e["delta"])
    return s
