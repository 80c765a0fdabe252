"""Inputs, exact assembly, tile census and the measure of the Schur-stage tests (tests/golden/make_schur_blocks.py,
tests/test_schur_reference_host.py, tests/test_gpu_schur_blocks.py).

INPUTS (NumPy only, fixed seeds).  A case is one landmark edge set (vertex 0 the landmark, vertex 1 the observing pose or -1
for a fixed camera) and one pose-pose chain (i, i + 1) that keeps the poses connected.  Every Jacobian entry is an integer in
[-3, 3] (times the power-of-two scale of its vertex in the `contrast` case), the information is the identity or a small integer
SPD matrix, the errors are multiples of 1/8 and lambda is a power of two: Hpp, Hpl, Hll and b are sums of products of such
numbers and exact in fp64 in any order.  assemble() evaluates them in NumPy in the layout the library returns; the fixture holds
the SHA-256 of the inputs and of the assembled arrays, the generator proves the exactness at 60 digits, and the device must
reproduce the arrays bit for bit before anything of the Schur stage is measured.

MEASURE.  A block of an output is held to its own scale s, evaluated at 60 digits by the generator:
    figure = max |got - ref| / (u s),   u = 2^-53,
with W_l = |Dinv_l| |Hll_l + lambda I| |Dinv_l| (entrywise) and
    Dinv_l          max W_l
    Hschur (i, j)   max (|Hpp_ij + lambda I| + sum_l |Hpl_il| W_l |Hpl_jl|')
    bschur_i        max (|b_i| + sum_l |Hpl_il| W_l |b_l|)
    x_l             max W_l (|b_l| + sum_i |Hpl_il|' |x_i|)
    x_p (solved)    per pose block of |Hs^-1| |Hs| |x_p|
No floor and no global scale.  The bound of (case, output) is 8 x the larger figure of two fp64 evaluations on the CPU that the
fixture records (the oracle; NumPy with per-tile partial sums in tile order, then the reduction)."""
import hashlib
import importlib.util
import os

import numpy as np

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "schur_blocks.npz")
# copies of two constants of the library; tests/test_schur_reference_host.py reads both definitions from the sources
TILE_BYTES = 39 * 1024                                           # BlockSolver::schur_tile_bytes (csrc/block_solver.h)
FUSE_REDUCE_MAX_PARTIALS = 6.0                                   # kFuseReduceMaxPartials (csrc/block_solver.hip)
MARGIN = 8.0
FULL_SOLVE_MAX_POSES = 60
OUTPUTS = ("Dinv", "Hschur", "bschur", "xl")                     # split interface, pinned x_p
SOLVE_OUTPUTS = ("bschur", "xp_solved", "xl_solved")             # full solve() at defaults (bschur: same reference)

# name: (p, l, G the census must give); every case carries its own lambda.  The solver family (6, 2) has Schur tiles but no
# case: no off-diagonal assembly row (d, 6, 2) exists, so no pose-landmark set of it can be built through the edge-set interface
# (build_system answers with the argument error that tests/test_gpu_parity.py holds it to).
CASES = {
    "fam_6_3": (6, 3, 4), "fam_3_2": (3, 2, 4), "fam_7_3": (7, 3, 4), "fam_3_3": (3, 3, 4),
    "group1": (6, 3, 1), "group8": (6, 3, 8),
    "graded_0": (6, 3, 1), "graded_10": (6, 3, 1), "graded_20": (6, 3, 1),
    "fixed": (6, 3, 4), "span": (6, 3, 4), "contrast": (6, 3, 4),
}
# the cases whose census must hold all three kinds of waves (all-diagonal, all-off-diagonal, mixed)
THREE_WAVE_KINDS = ("fam_6_3", "fam_3_2", "fam_7_3", "fam_3_3", "group1", "group8")
CONTRAST_SHIFT = -20                                             # Jacobian scale 2^-20 of the scaled third


def plan_module():
    """tools/probe/schur_diag_plan.py (the planner's tile tables rebuilt in NumPy)."""
    spec = importlib.util.spec_from_file_location("schur_diag_plan", os.path.join(ROOT, "tools", "probe", "schur_diag_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ================================================================================================ inputs
def _spd(rng, d):
    M = rng.randint(-1, 2, (d, d)).astype(np.float64)
    return M @ M.T + np.eye(d)


def _windows(rng, nP, nL, K):
    """Landmark j is seen by K consecutive poses from a random start (the recipe of test_gpu_schur_diag_sym._generic)."""
    return [list(range(s, s + K)) for s in rng.randint(0, nP - K, size=nL)]


def _chain_windows(nP, nL, K):
    """synthetic.make_ba_problem's lists: landmark j is seen by the K consecutive poses around j nP / nL."""
    lo = np.clip((np.arange(nL) * nP) // nL - K // 2, 0, nP - K)
    return [list(range(s, s + K)) for s in lo]


def make_case(name):
    """dict(p, l, d, nP, nL, lam, v0, v1, J0 [E][d*l], J1 [E][d*p], om [E][d*d], err [E][d], ca, cb, JA, JB, O2, e2, xp [nP*p]):
    Jacobians column-major d x dim as setEdgeData takes them."""
    p, l, _ = CASES[name]
    d = 2
    # (the three graded cases are one problem at three dampings)
    rng = np.random.RandomState(7000 + sorted(CASES).index("graded_0" if name.startswith("graded") else name))
    lam = 2.0 ** -3
    spd_landmark_info = False
    pose_scale = lm_scale = None
    if name.startswith("fam"):
        nP, nL = 40, 150
        obs = _windows(rng, nP, nL, 4)
        spd_landmark_info = name == "fam_3_3"                      # (every other landmark set has identity information)
    elif name == "group1":                                       # two poses per landmark, one from each half: at most two entries per partial
        nP, nL = 120, 240                                        # (a tile of 74 landmarks then holds more than 64 diagonal destinations)
        obs = [[int(a), int(b)] for a, b in zip(rng.randint(0, nP // 2, nL), rng.randint(nP // 2, nP, nL))]
    elif name == "group8":                                       # five consecutive poses, twelve landmarks per pose step
        nP, nL = 20, 240
        obs = _chain_windows(nP, nL, 5)
    elif name.startswith("graded"):                              # landmarks seen once, twice and five times
        # 64 poses: more than FULL_SOLVE_MAX_POSES, so the full solve is not measured here.  The scale of the solved x_p holds no
        # term for the rounding of Hschur itself, which these landmark blocks amplify: the CPU evaluations are 1.2e5 u s off at
        # lambda = 2^-20 with 40 poses (172 at 2^-10), where the generator's limit is 64; only lambda = 1 stays below it, and that
        # damping is what every other case already solves with.  The stages on pinned inputs are what the case is for; solve() on
        # ill-conditioned landmark blocks stays with the condition-based bound of tests/test_gpu_lm.py (helpers.dx_tolerance).
        nP, nL = 64, 150
        obs = [w[:(1, 2, 5)[j % 3]] for j, w in enumerate(_windows(rng, nP, nL, 5))]
        lam = 2.0 ** -int(name.split("_")[1])
    elif name == "fixed":
        nP, nL = 40, 150
        obs = _windows(rng, nP - 1, nL, 4)                        # pose nP - 1 has no landmark
        for j in range(0, nL, 5):                                # a fixed camera among the observers
            obs[j][1] = -1
        obs[77] = [-1, -1, -1]                                   # a landmark seen by fixed cameras only
    elif name == "span":
        nP, nL = 40, 150
        obs = _windows(rng, nP - 2, nL, 4)
        obs = [[q + 2 for q in w] for w in obs]                  # poses 0 and 1 share the landmarks below and nothing else
        for j in (3, 40, 75, 110, 146):
            obs[j] = [0, 1] + obs[j][:2]
    elif name == "contrast":
        nP, nL = 39, 150
        obs = _windows(rng, nP, nL, 4)
        pose_scale = np.where(np.arange(nP) >= 26, 2.0 ** CONTRAST_SHIFT, 1.0)
        lm_scale = np.array([2.0 ** CONTRAST_SHIFT if min(w) >= 26 else 1.0 for w in obs])
        lam = 2.0 ** -60                                         # below the scaled blocks (2^-40 times an integer)
    else:
        raise KeyError(name)
    v0 = np.concatenate([[nP + j] * len(w) for j, w in enumerate(obs)]).astype(np.int32)
    v1 = np.concatenate(obs).astype(np.int32)
    E = len(v0)
    J0 = rng.randint(-3, 4, (E, d * l)).astype(np.float64)
    J1 = rng.randint(-3, 4, (E, d * p)).astype(np.float64)
    om = np.array([(_spd(rng, d) if spd_landmark_info else np.eye(d)).reshape(-1) for _ in range(E)])
    err = rng.randint(-16, 17, (E, d)) / 8.0
    ca, cb = np.arange(0, nP - 1, dtype=np.int32), np.arange(1, nP, dtype=np.int32)
    n = len(ca)
    JA = rng.randint(-3, 4, (n, p * p)).astype(np.float64)
    JB = rng.randint(-3, 4, (n, p * p)).astype(np.float64)
    O2 = np.array([_spd(rng, p).reshape(-1) for _ in range(n)])
    e2 = rng.randint(-16, 17, (n, p)) / 8.0
    if pose_scale is not None:
        J0 *= lm_scale[v0 - nP][:, None]
        J1 *= np.where(v1 >= 0, pose_scale[np.maximum(v1, 0)], 1.0)[:, None]
        JA *= pose_scale[ca][:, None]
        JB *= pose_scale[cb][:, None]
    # the pinned pose solution of the back-substitution: dyadic entries of mixed magnitude
    xp = rng.randint(-7, 8, nP * p) * 2.0 ** rng.randint(-6, 4, nP * p)
    return dict(name=name, p=p, l=l, d=d, nP=nP, nL=nL, lam=lam, v0=v0, v1=v1, J0=J0, J1=J1, om=om, err=err, ca=ca, cb=cb, JA=JA,
                JB=JB, O2=O2, e2=e2, xp=xp, pose_scale=pose_scale)


INPUT_NAMES = ("v0", "v1", "J0", "J1", "om", "err", "ca", "cb", "JA", "JB", "O2", "e2", "xp")


def sha256_of(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def input_hash(c):
    return sha256_of([c[k] for k in INPUT_NAMES] + [np.float64(c["lam"])])


# ================================================================================================ exact assembly
def _mats(J, d, dim):
    """[E][d * dim] column-major -> [E][d][dim]."""
    return J.reshape(len(J), dim, d).transpose(0, 2, 1)


def _ccs(ncols, pairs):
    """Upper block CCS of a set of (row, column): colptr, rowidx (rows ascending) and {(row, column): slot}."""
    cols = [[] for _ in range(ncols)]
    for r, c in set(pairs):
        cols[c].append(r)
    cp, ri, slot = [0], [], {}
    for c in range(ncols):
        for r in sorted(cols[c]):
            slot[(r, c)] = len(ri)
            ri.append(r)
        cp.append(len(ri))
    return np.array(cp, np.int32), np.array(ri, np.int32), slot


def assemble(c):
    """The system of a case in fp64 (exact, see the head) in the library's layout:
    Hpp [nnz][p*p], Hpl [nnz][p*l], Hll [nL][l*l] (column-major blocks on upper block CCS patterns), b [nP*p + nL*l], the
    patterns pp / pl / hs as (colptr, rowidx, {(row, column): slot}), and the natural-layout blocks HppB [nnz][p][p] (row, column),
    HplB [nnz][p][l]."""
    p, l, d, nP, nL = c["p"], c["l"], c["d"], c["nP"], c["nL"]
    lmk, pose = c["v0"] - nP, c["v1"]
    free = pose >= 0
    A0, A1 = _mats(c["J0"], d, l), _mats(c["J1"], d, p)
    Om = c["om"].reshape(-1, d, d)
    we = np.einsum("eij,ej->ei", Om, c["err"])
    Hll = np.zeros((nL, l, l))
    np.add.at(Hll, lmk, np.einsum("eia,eij,ejb->eab", A0, Om, A0))
    bl = np.zeros((nL, l))
    np.add.at(bl, lmk, -np.einsum("eia,ei->ea", A0, we))
    pp = _ccs(nP, [(i, i) for i in range(nP)] + list(zip(c["ca"].tolist(), c["cb"].tolist())))
    pl = _ccs(nL, list(zip(pose[free].tolist(), lmk[free].tolist())))
    HppB = np.zeros((len(pp[1]), p, p))
    HplB = np.zeros((len(pl[1]), p, l))
    bp = np.zeros((nP, p))
    qd = np.array([pp[2][(i, i)] for i in range(nP)])
    np.add.at(HppB, qd[pose[free]], np.einsum("eia,eij,ejb->eab", A1[free], Om[free], A1[free]))
    np.add.at(bp, pose[free], -np.einsum("eia,ei->ea", A1[free], we[free]))
    ql = np.array([pl[2][(int(i), int(j))] for i, j in zip(pose[free], lmk[free])])
    np.add.at(HplB, ql, np.einsum("eia,eij,ejb->eab", A1[free], Om[free], A0[free]))
    A, B, O2 = _mats(c["JA"], p, p), _mats(c["JB"], p, p), c["O2"].reshape(-1, p, p)
    w2 = np.einsum("eij,ej->ei", O2, c["e2"])
    np.add.at(HppB, qd[c["ca"]], np.einsum("eia,eij,ejb->eab", A, O2, A))
    np.add.at(HppB, qd[c["cb"]], np.einsum("eia,eij,ejb->eab", B, O2, B))
    qo = np.array([pp[2][(int(i), int(j))] for i, j in zip(c["ca"], c["cb"])])
    np.add.at(HppB, qo, np.einsum("eia,eij,ejb->eab", A, O2, B))
    np.add.at(bp, c["ca"], -np.einsum("eia,ei->ea", A, w2))
    np.add.at(bp, c["cb"], -np.einsum("eia,ei->ea", B, w2))
    lists = pose_lists(c, pl)
    hs = _ccs(nP, [(i, j) for (i, j) in pp[2]] + [(a, b) for w in lists for k, a in enumerate(w) for b in w[k:]])
    tr = lambda X: np.ascontiguousarray(X.transpose(0, 2, 1)).reshape(len(X), -1)
    return dict(Hpp=tr(HppB), Hpl=tr(HplB), Hll=tr(Hll), b=np.concatenate([bp.reshape(-1), bl.reshape(-1)]), pp=pp, pl=pl, hs=hs,
                HppB=HppB, HplB=HplB, HllB=Hll, bp=bp, bl=bl, lists=lists)


def pose_lists(c, pl):
    """Per landmark the free poses that see it, ascending (the rows of its Hpl column)."""
    cp, ri, _ = pl
    return [ri[cp[j]:cp[j + 1]].tolist() for j in range(c["nL"])]


def assembled_hash(a):
    return sha256_of([a["Hpp"], a["Hpl"], a["Hll"], a["b"], a["pp"][0], a["pp"][1], a["pl"][0], a["pl"][1], a["hs"][0], a["hs"][1]])


# ================================================================================================ tiles
def tile_of(c, lists):
    """The planner's greedy landmark-range tiles (BlockSolver::build_structure; census() of tools/probe/schur_diag_plan.py counts
    with the same rule): tile index per landmark."""
    p, l = c["p"], c["l"]
    dpb = ((l * l + 1) & ~1) + ((l * l + l + 1) & ~1)
    bpb = (l + 1) & ~1
    out = np.zeros(c["nL"], np.int64)
    t = used = l0 = 0
    for j, w in enumerate(lists):
        k = len(w)
        add = k * p * l * 8 + dpb * 8 + bpb * 8 + k * (k + 1) // 2 * 14
        if j > l0 and used + add > TILE_BYTES:
            t, used, l0 = t + 1, 0, j
        used += add
        out[j] = t
    return out


def census_of(c, a):
    """census() of the case's observations plus the partial blocks per destination: dict(G, all_diag, all_off, mixed, n_tiles,
    n_td, partials {(row, column): tiles that hold an entry of it})."""
    cen = plan_module().census(c["v0"].astype(np.int64) - c["nP"], c["v1"], c["nP"], PD=c["p"], LD=c["l"])
    tl = tile_of(c, a["lists"])
    part = {}
    for j, w in enumerate(a["lists"]):
        for k, i1 in enumerate(w):
            for i2 in w[k:]:
                part.setdefault((i1, i2), set()).add(int(tl[j]))
    w = cen["orders"]["round"]
    n_td = sum(len(v) for v in part.values())
    assert n_td == cen["n_td"], (n_td, cen["n_td"])            # the two tile walks agree
    return dict(G=int(cen["G"]), all_diag=int(w["all_diag"]), all_off=int(w["all_off"]), mixed=int(w["mixed"]), n_tiles=int(tl.max()) + 1,
                n_td=n_td, partials={k: len(v) for k, v in part.items()}, tile=tl)


def assert_census(name, c, cen):
    """What the case is there for, from the census alone."""
    assert cen["G"] == CASES[name][2], (name, cen["G"])
    if name in THREE_WAVE_KINDS:
        assert cen["all_diag"] > 0 and cen["all_off"] > 0 and cen["mixed"] > 0, (name, cen["all_diag"], cen["all_off"], cen["mixed"])
    assert cen["n_tiles"] >= 2 and max(cen["partials"].values()) >= 2, name       # more than one block, more than one slot per destination
    if name == "span":
        assert cen["partials"][(0, 1)] >= 3 and cen["partials"][(0, 0)] >= 3 and cen["partials"][(1, 1)] >= 3, cen["partials"][(0, 1)]


def coverage(c, a):
    """Counts the host test holds: landmarks by the number of free observers, observations from fixed cameras."""
    seen = np.bincount(np.array([len(w) for w in a["lists"]]), minlength=6)
    return dict(seen=seen, fixed_obs=int((c["v1"] < 0).sum()), unseen_landmarks=int(seen[0]),
                bare_poses=int(c["nP"] - len(set(i for w in a["lists"] for i in w))))


# ================================================================================================ fixture and measure
_cache = {}


def fixture():
    if "f" not in _cache:
        with np.load(FIXTURE) as f:
            _cache["f"] = {k: f[k] for k in f.files}
    return _cache["f"]


def load_case(name):
    """The rebuilt inputs, their exact assembly and the stored references of one case (read-only, shared by every test):
    c (make_case), a (assemble), ref {output: blocks}, scale {output: per block}, cpu {output: (oracle, numpy)}, bound {output}."""
    if name in _cache:
        return _cache[name]
    f = fixture()
    c = make_case(name)
    a = assemble(c)
    g = lambda k: f[name + "/" + k]
    outs = OUTPUTS + (("xp_solved", "xl_solved") if c["nP"] <= FULL_SOLVE_MAX_POSES else ())
    k = dict(name=name, c=c, a=a, input_sha=str(g("input_sha")), assembled_sha=str(g("assembled_sha")),
             ref={o: g(o) for o in outs}, scale={o: g(o + "_s") for o in outs},
             cpu={o: (float(g(o + "_cpu")[0]), float(g(o + "_cpu")[1])) for o in outs})
    k["bound"] = {o: MARGIN * max(max(k["cpu"][o]), float(g(o + "_floor"))) for o in outs}
    for d in (k["ref"], k["scale"], c, a):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    _cache[name] = k
    return k


def figures(got, ref, scale):
    """max |got - ref| / (u s) per block: got / ref [n][...], scale [n]."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.abs(got - ref).reshape(len(ref), -1).max(axis=1) / (U * np.asarray(scale))


def hschur_blocks(values, p):
    """Library values [nnz * p * p] (column-major blocks) -> [nnz][p][p] (row, column)."""
    return np.asarray(values).reshape(-1, p, p).transpose(0, 2, 1)


# ================================================================================================ fp64 on the CPU
def numpy_evaluation(c, a, cen, with_solve):
    """The Schur stage in NumPy in the tiles' order: Dinv by np.linalg.inv (LU), per tile the partial sums of a destination in
    landmark order, then Hschur = (Hpp + lambda I) - (sum of the partials in tile order); the right-hand side alike."""
    p, l, nP, nL, lam = c["p"], c["l"], c["nP"], c["nL"], c["lam"]
    D = a["HllB"] + lam * np.eye(l)
    Dinv = np.linalg.inv(D)
    cp, ri, slot = a["pl"]
    hs = a["hs"][2]
    nt = cen["n_tiles"]
    part = [dict() for _ in range(nt)]
    prhs = np.zeros((nt, nP, p))
    for j, w in enumerate(a["lists"]):
        t = int(cen["tile"][j])
        for k, i1 in enumerate(w):
            B1 = a["HplB"][cp[j] + k]
            V = B1 @ Dinv[j]
            prhs[t, i1] += V @ a["bl"][j]
            for k2 in range(k, len(w)):
                q = hs[(i1, w[k2])]
                part[t][q] = part[t].get(q, 0.0) + V @ a["HplB"][cp[j] + k2].T
    Hs = np.zeros((len(a["hs"][1]), p, p))
    for (r, cc), q in a["pp"][2].items():
        Hs[hs[(r, cc)]] = a["HppB"][q] + (lam * np.eye(p) if r == cc else 0.0)
    red = np.zeros_like(Hs)
    for t in range(nt):
        for q, P in part[t].items():
            red[q] += P
    Hs -= red
    bs = a["bp"] - prhs.sum(axis=0)
    out = dict(Dinv=Dinv, Hschur=Hs, bschur=bs, xl=back_substitute_numpy(c, a, Dinv, c["xp"]))
    if with_solve:
        n = nP * p
        Hd = np.zeros((n, n))
        for (r, cc), q in hs.items():
            Hd[r * p:(r + 1) * p, cc * p:(cc + 1) * p] = Hs[q]
            Hd[cc * p:(cc + 1) * p, r * p:(r + 1) * p] = Hs[q].T
        Lc = np.linalg.cholesky(Hd)
        xp = np.linalg.solve(Lc.T, np.linalg.solve(Lc, bs.reshape(-1)))
        out["xp_solved"] = xp.reshape(nP, p)
        out["xl_solved"] = back_substitute_numpy(c, a, Dinv, xp)
    return out


def back_substitute_numpy(c, a, Dinv, xp):
    cp = a["pl"][0]
    xp = np.asarray(xp).reshape(c["nP"], c["p"])
    xl = np.zeros((c["nL"], c["l"]))
    for j, w in enumerate(a["lists"]):
        r = a["bl"][j].copy()
        if w:
            r -= np.einsum("kpl,kp->l", a["HplB"][cp[j]:cp[j + 1]], xp[w])
        xl[j] = Dinv[j] @ r
    return xl


def oracle_solver(O, c):
    o = O.OracleSolver(c["p"], c["l"], c["nP"], c["nL"], True)
    q0 = o.add_edge_set(c["d"], c["v0"], c["v1"]); o.set_dims(q0, c["l"], c["p"])
    q1 = o.add_edge_set(c["p"], c["ca"], c["cb"]); o.set_dims(q1, c["p"], c["p"])
    o.build_structure()
    o.set_edge_data(q0, c["J0"], c["J1"], c["om"], c["err"])
    o.set_edge_data(q1, c["JA"], c["JB"], c["O2"], c["e2"])
    o.build_system()
    return o


def oracle_evaluation(O, c, a, with_solve):
    """The same outputs from the CPU oracle (oracle/g2o_oracle.c: landmark by landmark, cofactor inverse)."""
    p, l, nP, nL = c["p"], c["l"], c["nP"], c["nL"]
    o = oracle_solver(O, c)
    assert np.array_equal(o.values("Hpp"), a["Hpp"].reshape(-1)) and np.array_equal(o.values("Hpl"), a["Hpl"].reshape(-1))
    assert np.array_equal(o.values("Hll"), a["Hll"].reshape(-1)) and np.array_equal(o.b(), a["b"])
    cp, ri = o.pattern("hs")
    assert np.array_equal(cp, a["hs"][0]) and np.array_equal(ri, a["hs"][1])
    o.set_lambda(c["lam"], True)
    o.solve_schur()
    out = dict(Dinv=o.values("Dinv").reshape(nL, l, l).transpose(0, 2, 1), Hschur=hschur_blocks(o.values("Hschur"), p),
               bschur=o.bschur().reshape(nP, p))
    x = o.view("x", o.n)
    x[:] = 0.0
    x[:nP * p] = c["xp"]
    o.solve_back_substitute()
    out["xl"] = o.x()[nP * p:].reshape(nL, l)
    if with_solve:
        assert o.solve()
        out["xp_solved"] = o.x()[:nP * p].reshape(nP, p)
        out["xl_solved"] = o.x()[nP * p:].reshape(nL, l)
    return out


# ================================================================================================ the device
def device_solver(capi, c, options=None):
    """HipBlockSolver with the case's edges, built (generic edge-data path)."""
    s = capi.HipBlockSolver(c["p"], c["l"], 0)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    k0, k1 = s.addEdgeSet(c["d"], c["v0"], c["v1"]), s.addEdgeSet(c["p"], c["ca"], c["cb"])
    s.buildStructure(c["nP"], c["nL"], True)
    s.setEdgeData(k0, c["J0"], c["J1"], c["om"], c["err"])
    s.setEdgeData(k1, c["JA"], c["JB"], c["O2"], c["e2"])
    s.buildSystem()
    return s


# ================================================================================================ the fused BA path
# EdgeProjectXYZ2UV graphs through lm.setup_device_ba / baSetEdgesClasses with ba_fused = 1: the tiles evaluate errors, Jacobians
# and robust weights from the estimates themselves, so the reference starts from the estimates too and nothing is exact.  The
# magnitudes in the scales are then the operand sums of the assembled terms (sum of |w J J'| per entry of Hpp / Hll, |t0| + |t1|
# per entry of Hpl, sum of w |J|' max(|e|, |z|) per entry of b) instead of |Hpp|, |Hll|, |Hpl|, |b|.
#   ba_prod1 / ba_prodc   the BA group of tests/golden/producer_edges.npz (12 cameras, 40 points): one class with Huber, and its
#                         class table (four classes of intrinsics and robust kernels)
#   ba_chain              synthetic.make_ba_problem(40, 400): 38 free cameras, five observations per point, Huber
# Two dampings per case: the first solve after buildSystem and a second one without a new linearisation.
FUSED_CASES = ("ba_prod1", "ba_prodc", "ba_chain")
FUSED_LAMBDAS = (2.0 ** 4, 2.0 ** -6)
CHAIN_HUBER = 20.0                                               # pixels: the median error of the chain's first estimates is 18
FUSED_FIXTURE = os.path.join(ROOT, "tests", "golden", "schur_blocks_fused.npz")
PRODUCER_FIXTURE = os.path.join(ROOT, "tests", "golden", "producer_edges.npz")


def make_fused_case(name):
    """dict(cams, pts, cam_idx, pt_idx, cam_hidx, meas, classes [n][5] = (f, cx, cy, kernel, delta), edge_class, nP, nL, v0, v1,
    xp, ...) in the form lm.setup_device_ba takes (P, L, E, f, cx, cy of class 0)."""
    if name == "ba_chain":
        from openslam_g2o_amd import synthetic as S
        pr = S.make_ba_problem(40, 400, seed=42)
        c = {k: pr[k] for k in ("cams", "pts", "cam_idx", "pt_idx", "cam_hidx", "meas")}
        classes = np.array([[pr["f"], pr["cx"], pr["cy"], 1.0, CHAIN_HUBER]])
        cls = np.zeros(pr["E"], np.int32)
    else:
        with np.load(PRODUCER_FIXTURE) as f:
            pre = "ba1" if name == "ba_prod1" else "ba"
            c = dict(cams=f["ba_cams"], pts=f["ba_pts"], cam_idx=f["ba_cam_idx"], pt_idx=f["ba_pt_idx"], cam_hidx=f["ba_cam_hidx"],
                     meas=f[pre + "_meas"])
            classes, cls = f["ba_classes"].copy(), f["ba_edge_class"].astype(np.int32)
            if name == "ba_prod1":
                classes = np.array([[classes[0, 0], classes[0, 1], classes[0, 2], 1.0, float(f["ba1_huber"])]])
                cls = np.zeros(len(cls), np.int32)
    nP, nL = int(c["cam_hidx"].max()) + 1, len(c["pts"])
    rng = np.random.RandomState(7100 + FUSED_CASES.index(name))
    xp = rng.randint(-7, 8, nP * 6) * 2.0 ** rng.randint(-12, -4, nP * 6)
    c.update(name=name, p=6, l=3, d=2, P=len(c["cams"]), L=nL, E=len(cls), nP=nP, nL=nL, classes=classes, edge_class=cls,
             f=float(classes[0, 0]), cx=float(classes[0, 1]), cy=float(classes[0, 2]), xp=xp,
             v0=(nP + c["pt_idx"]).astype(np.int32), v1=c["cam_hidx"][c["cam_idx"]].astype(np.int32))
    return c


FUSED_INPUT_NAMES = ("cams", "pts", "cam_idx", "pt_idx", "cam_hidx", "meas", "classes", "edge_class", "xp")


def fused_input_hash(c):
    return sha256_of([c[k] for k in FUSED_INPUT_NAMES] + [np.array(FUSED_LAMBDAS)])


def fused_structure(c):
    """The patterns (pp: the diagonal only), the pose lists and slots of a fused case, as assemble() gives them."""
    nP, nL = c["nP"], c["nL"]
    free = c["v1"] >= 0
    pl = _ccs(nL, list(zip(c["v1"][free].tolist(), c["pt_idx"][free].tolist())))
    pp = _ccs(nP, [(i, i) for i in range(nP)])
    lists = pose_lists(c, pl)
    hs = _ccs(nP, [(i, i) for i in range(nP)] + [(a, b) for w in lists for k, a in enumerate(w) for b in w[k:]])
    return dict(pp=pp, pl=pl, hs=hs, lists=lists)


def oracle_fused(O, c):
    """The oracle on a fused case: its fp64 producers per class (O.ba_edges), one edge set per class with that class's kernel."""
    o = O.OracleSolver(6, 3, c["nP"], c["nL"], True)
    sets = []
    for k in range(len(c["classes"])):
        sel = np.flatnonzero(c["edge_class"] == k)
        q = o.add_edge_set(2, c["v0"][sel], c["v1"][sel])
        o.set_dims(q, 3, 6)
        sets.append((q, sel))
    o.build_structure()
    for k, (q, sel) in enumerate(sets):
        f, cx, cy, kind, delta = c["classes"][k]
        J0, J1, err = O.ba_edges(c["cams"], c["pts"], c["cam_idx"][sel], c["pt_idx"][sel], c["meas"][sel], f, cx, cy)
        om = np.tile(np.eye(2).reshape(-1), (len(sel), 1))
        o.set_edge_data(q, J0, J1, om, err, float(delta) if kind > 0 else 0.0)
        if kind > 0:
            o.set_robust_kernel(q, int(kind))
    o.build_system()
    return o


def fused_cpu_evaluations(O, c, st, lam):
    """(oracle, NumPy in the tiles' order on the oracle's fp64 system) at one damping: dict(Dinv, Hschur, bschur, xl) each."""
    nP, nL = c["nP"], c["nL"]
    o = oracle_fused(O, c)
    for w, name in (("pp", "pp"), ("pl", "pl"), ("hs", "hs")):
        cp, ri = o.pattern(w)
        assert np.array_equal(cp, st[name][0]) and np.array_equal(ri, st[name][1]), w
    a = dict(st, HppB=hschur_blocks(o.values("Hpp"), 6), HplB=o.values("Hpl").reshape(-1, 3, 6).transpose(0, 2, 1),
             HllB=o.values("Hll").reshape(nL, 3, 3).transpose(0, 2, 1), bp=o.b()[:nP * 6].reshape(nP, 6), bl=o.b()[nP * 6:].reshape(nL, 3))
    cc = dict(c, lam=lam)
    cen = census_of(cc, a)
    en = numpy_evaluation(cc, a, cen, False)
    o.set_lambda(lam, True)
    o.solve_schur()
    eo = dict(Dinv=o.values("Dinv").reshape(nL, 3, 3).transpose(0, 2, 1), Hschur=hschur_blocks(o.values("Hschur"), 6),
              bschur=o.bschur().reshape(nP, 6))
    x = o.view("x", o.n)
    x[:] = 0.0
    x[:nP * 6] = c["xp"]
    o.solve_back_substitute()
    eo["xl"] = o.x()[nP * 6:].reshape(nL, 3)
    return eo, en, cen


def load_fused_case(name):
    """As load_case: c, st (fused_structure), and per damping index i the outputs under "<output>@i"."""
    key = "fused:" + name
    if key in _cache:
        return _cache[key]
    if "ff" not in _cache:
        with np.load(FUSED_FIXTURE) as z:
            _cache["ff"] = {k: z[k] for k in z.files}
    f = _cache["ff"]
    c = make_fused_case(name)
    g = lambda k: f[name + "/" + k]
    outs = ["%s@%d" % (o, i) for i in range(len(FUSED_LAMBDAS)) for o in OUTPUTS]
    k = dict(name=name, c=c, st=fused_structure(c), input_sha=str(g("input_sha")), ref={o: g(o) for o in outs},
             scale={o: g(o + "_s") for o in outs}, cpu={o: (float(g(o + "_cpu")[0]), float(g(o + "_cpu")[1])) for o in outs})
    k["bound"] = {o: MARGIN * max(max(k["cpu"][o]), float(g(o + "_floor"))) for o in outs}
    for d in (k["ref"], k["scale"]):
        for v in d.values():
            v.setflags(write=False)
    _cache[key] = k
    return k


def device_fused(capi, lm, c, options):
    """HipBlockSolver on the fused BA path, linearised and built: one class through lm.setup_device_ba (Huber), a class table
    through baSetEdgesClasses."""
    if len(c["classes"]) == 1:
        s, g = lm.setup_device_ba(c, huber_delta=float(c["classes"][0, 4]), options=options)
    else:
        s = capi.HipBlockSolver(6, 3, 0)
        for name, value in options.items():
            s.setOption(name, value)
        k = s.addEdgeSet(2, c["v0"], c["v1"])
        s.buildStructure(c["nP"], c["nL"], True)
        s.baSetEdgesClasses(k, c["cam_idx"], c["pt_idx"], c["meas"], c["classes"], c["edge_class"])
        s.baSetEstimates(c["cams"], c["cam_hidx"], c["pts"], np.arange(c["L"], dtype=np.int32))
        g = lm.DeviceBAGraph(s)
    g.linearize()
    s.buildSystem()
    return s
