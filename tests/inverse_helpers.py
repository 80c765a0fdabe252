"""Inputs, request lists and the measure of the inverse-block tests (tests/golden/make_inverse_blocks.py,
tests/test_inverse_reference_host.py, tests/test_gpu_inverse_blocks.py, tests/test_gpu_marginals.py).

MATRICES (NumPy only).  Every case is a set of generic edges: a binary edge (i < j) has J0 = a0 I, a d x d Jacobian J1 and a
symmetric information block W, a unary edge has J = a I and a symmetric W (it may be indefinite: the "diagonal remainder").
    A_ii += a0^2 W,   A_jj += J1' W J1,   A_ij += a0 W J1,        A_ii += a^2 W (unary).
Every a is a power of two and every entry of W and J1 a small integer times a power of two, so all products and sums are exact
in fp64 in any order: the narrow seam takes the assembled blocks, the wide seam assembles the same edges on the device and must
reproduce the matrix bit for bit.  (chain_decay has unsymmetric off-diagonal blocks B, so its edges are J0 = I, J1 = B, W = I
instead of J = -+I with W = -B, which would not be symmetric.)

MEASURE.  For request i with reference block Z_i and scale s_i -- the largest entry of block (r, c) of |Z| |A| |Z|, the
componentwise size of the rounding error of an inverse obtained through a Cholesky factor -- err_i = max |M_i - Z_i| / (u s_i)
in units of the fp64 unit roundoff u = 2^-53.  No floor and no global scale."""
import os

import numpy as np

U = 2.0 ** -53
BLOCK_SIZES = (3, 6, 7)
LANDMARK_DIM = {3: 2, 6: 3, 7: 3}
CASES = ("chain_flat", "chain_decay", "chain_graded", "hubs", "grid", "wide_panel")
CHAIN_NB = 40
HUB_CHAIN = 24
HUBS = {3: 22, 6: 11, 7: 10}                                     # boundary of every front below the root >= 66 / 66 / 70 rows
GRID_SIDE = {3: 8, 6: 6, 7: 6}
# wide_panel: a dense matrix of two panels of the option's 48 scalars (16 / 8 / 6 blocks each): with max_sn_scalars_lds = 48
# and exactly two fronts both hold 48 / 48 / 42 pivot scalars, so the first one (which has a boundary) runs the second k0 pass
WIDE_CAP = 48
WIDE_NB = {bs: 2 * (WIDE_CAP // bs) for bs in BLOCK_SIZES}
# wide_panel64: the same with both supernode caps at their upper limit of 64 scalars: two panels of 63 / 60 / 63 pivot scalars, the
# widest the planner makes (it caps a panel at min(max_sn_scalars, 64) / bs blocks); a third of its blocks are stored
EXTRA_CASES = ("wide_panel64",)
WIDE64_NB = {bs: 2 * (64 // bs) for bs in BLOCK_SIZES}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inverse_blocks.npz")


def key(case, bs):
    return "%s_b%d" % (case, bs)


# ================================================================================================ inputs
def _info(rng, bs):
    """A small integer SPD block: M M' + I with M in -1 .. 1."""
    M = rng.randint(-1, 2, (bs, bs)).astype(np.float64)
    return M @ M.T + np.eye(bs)


def _laplacian_edges(rng, bs, nb, pairs, scale=None):
    """Edges J = -+ d I over `pairs` with integer information blocks and one prior on block 0."""
    d = np.ones(nb) if scale is None else scale
    vi = np.array([p[0] for p in pairs], np.int32)
    vj = np.array([p[1] for p in pairs], np.int32)
    assert np.all(vi < vj)
    eye = np.eye(bs)
    return dict(nb=nb, bs=bs, vi=vi, vj=vj, a0=-d[vi], J1=np.array([d[j] * eye for j in vj]),
                W=np.array([_info(rng, bs) for _ in pairs]), ui=np.array([0], np.int32), ua=np.array([d[0]]),
                UW=np.array([_info(rng, bs)]))


def make_edges(case, bs):
    """dict(nb, bs, vi, vj, a0 [ne], J1 [ne][bs][bs], W [ne][bs][bs], ui, ua [nu], UW [nu][bs][bs])."""
    rng = np.random.RandomState(1000 * (CASES + EXTRA_CASES).index(case) + bs)
    if case in ("chain_flat", "chain_graded"):
        nb = CHAIN_NB
        scale = None
        if case == "chain_graded":                               # D A D: block scales 2^10 and 2^-10 in turn (a factor 1e6)
            scale = np.array([2.0 ** (10 if i % 2 == 0 else -10) for i in range(nb)])
        return _laplacian_edges(rng, bs, nb, [(c - 1, c) for c in range(1, nb)], scale)
    if case == "chain_decay":
        nb = CHAIN_NB
        B = np.round(rng.normal(size=(nb - 1, bs, bs)) * 1024.0) / 1024.0
        n = nb * bs
        A = np.zeros((n, n))
        for c in range(1, nb):
            A[bs * (c - 1):bs * c, bs * c:bs * (c + 1)] = B[c - 1]
        A = A + A.T
        delta = np.ceil((np.abs(A).sum(axis=1).max() + 1.0) * 1024.0) / 1024.0
        UW = np.zeros((nb, bs, bs))
        for i in range(nb):                                      # the diagonal remainder: delta I minus what the edges put there
            UW[i] = delta * np.eye(bs)
            if i < nb - 1:
                UW[i] -= np.eye(bs)
            if i > 0:
                UW[i] -= B[i - 1].T @ B[i - 1]
        return dict(nb=nb, bs=bs, vi=np.arange(nb - 1, dtype=np.int32), vj=np.arange(1, nb, dtype=np.int32), a0=np.ones(nb - 1), J1=B,
                    W=np.array([np.eye(bs)] * (nb - 1)), ui=np.arange(nb, dtype=np.int32), ua=np.ones(nb), UW=UW)
    if case == "hubs":
        nc, h = HUB_CHAIN, HUBS[bs]
        pairs = [(c - 1, c) for c in range(1, nc)] + [(c, nc + k) for c in range(nc) for k in range(h)]
        pairs += [(nc + k, nc + k2) for k in range(h) for k2 in range(k + 1, h)]
        return _laplacian_edges(rng, bs, nc + h, pairs)
    if case == "grid":
        g = GRID_SIDE[bs]
        pairs = [(y * g + x, y * g + x + 1) for y in range(g) for x in range(g - 1)]
        pairs += [(y * g + x, (y + 1) * g + x) for y in range(g - 1) for x in range(g)]
        return _laplacian_edges(rng, bs, g * g, sorted(pairs))
    if case in ("wide_panel", "wide_panel64"):
        nb = WIDE_NB[bs] if case == "wide_panel" else WIDE64_NB[bs]
        return _laplacian_edges(rng, bs, nb, [(i, j) for i in range(nb) for j in range(i + 1, nb)])
    raise KeyError(case)


def assemble(E):
    """{(r, c): bs x bs block, r <= c} of the edges, in fp64 (exact, see above)."""
    bs = E["bs"]
    blocks = {(i, i): np.zeros((bs, bs)) for i in range(E["nb"])}
    for k in range(len(E["vi"])):
        i, j = int(E["vi"][k]), int(E["vj"][k])
        a, J1, W = E["a0"][k], E["J1"][k], E["W"][k]
        blocks[(i, i)] += a * a * W
        blocks[(j, j)] += J1.T @ W @ J1
        blocks[(i, j)] = blocks.get((i, j), np.zeros((bs, bs))) + a * (W @ J1)
    for k in range(len(E["ui"])):
        i = int(E["ui"][k])
        blocks[(i, i)] += E["ua"][k] ** 2 * E["UW"][k]
    return blocks


def to_ccs(nb, blocks):
    """Upper block CCS, rows of a column increasing, column-major blocks: colptr, rowidx, values [nnzb][bs * bs]."""
    cols = [[] for _ in range(nb)]
    for (r, c) in blocks:
        assert r <= c
        cols[c].append(r)
    cp, ri, vals = [0], [], []
    for c in range(nb):
        for r in sorted(cols[c]):
            ri.append(r)
            vals.append(blocks[(r, c)].T.reshape(-1))
        cp.append(len(ri))
    return np.array(cp, np.int32), np.array(ri, np.int32), np.array(vals)


def dense_from_ccs(nb, bs, cp, ri, vals):
    A = np.zeros((nb * bs, nb * bs))
    v = np.asarray(vals).reshape(-1, bs, bs)
    for c in range(nb):
        for q in range(cp[c], cp[c + 1]):
            r = ri[q]
            A[bs * r:bs * (r + 1), bs * c:bs * (c + 1)] = v[q].T
            A[bs * c:bs * (c + 1), bs * r:bs * (r + 1)] = v[q]
    return A


def legacy_tridiagonal(bs):
    """The diagonally dominant block-tridiagonal matrix (unrounded normal entries) and the requests of
    test_inverse_blocks_inside_and_outside_the_pattern_on_both_seams in tests/test_gpu_marginals.py."""
    nb = CHAIN_NB
    rng = np.random.default_rng(400 + bs)
    n = nb * bs
    A = np.zeros((n, n))
    for c in range(1, nb):
        A[bs * (c - 1):bs * c, bs * c:bs * (c + 1)] = rng.normal(size=(bs, bs))
    A = A + A.T
    A += np.eye(n) * (np.abs(A).sum(axis=1).max() + 1.0)
    pairs = [(c, c) for c in range(nb)] + [(c, c - 1) for c in range(1, nb)] + [(0, nb - 1), (nb - 1, 0), (1, nb - 1), (0, nb - 1)]
    return A, pairs


def scales_fp64(A, Z, bs, rows, cols):
    """s_i of the measure from fp64 matrices (the tests whose matrix is no exact fixture): max entry of block (r, c) of |Z| |A| |Z|."""
    T = np.abs(Z) @ np.abs(A) @ np.abs(Z)
    return np.array([T[bs * r:bs * (r + 1), bs * c:bs * (c + 1)].max() for r, c in zip(rows, cols)])


def scale_from_columns(nb, bs, cp, ri, vals, X, r, c):
    """s of block (r, c) from the block columns r and c of the inverse alone (X: {block column: n x bs}; the inverse is
    symmetric, so rows r are column r transposed): max entry of |X_r|' |A| |X_c|, |A| applied block by block from the CCS."""
    blk = np.abs(np.asarray(vals).reshape(-1, bs, bs)).transpose(0, 2, 1)             # [q] = |block (ri[q], column)|
    cidx = np.repeat(np.arange(nb), np.diff(cp))
    ridx = np.asarray(ri)[:len(cidx)]
    Xc = np.abs(X[int(c)]).reshape(nb, bs, bs)
    T = np.zeros((nb, bs, bs))
    np.add.at(T, ridx, np.einsum("qij,qjk->qik", blk, Xc[cidx]))
    off = ridx != cidx
    np.add.at(T, cidx[off], np.einsum("qji,qjk->qik", blk[off], Xc[ridx[off]]))
    return float((np.abs(X[int(r)]).T @ T.reshape(nb * bs, bs)).max())


def legacy_margin(bs):
    """What the device may differ from NumPy's fp64 inverse (numpy_inverse) on the legacy tridiagonal matrices, in units of
    u s: 8 x the CPU's distance from the 60-digit reference (the device's margin) plus that distance once more (the fp64
    reference's own error).  The figure is measured on the narrow seam's matrix; test_gpu_marginals.py applies it to the wide
    seam's matrix of that test as well, a device-assembled random-walk chain with no 60-digit figure of its own, where it is
    a loose bound (38 / 57 u s against the 0.1 - 0.3 attained on the chain_flat cases)."""
    f = fixture()
    k = key("legacy_tridiag", bs)
    return 9.0 * max(float(f[k + "/cpu_numpy"]), float(f[k + "/cpu_oracle"]))


def far_pairs(case, bs, nb, pattern):
    """Pairs (r < c) outside the matrix's own pattern: the far corner, a block that shares its column, and a sample over at most
    12 further columns (each distinct column costs the device 2 bs triangular sweeps when the pair is outside the factor)."""
    out = [(0, nb - 1), (1, nb - 1)]
    rng = np.random.RandomState(77 + bs)
    for c in sorted(set(int(v) for v in np.linspace(2, nb - 2, 12).round())):
        r = int(rng.randint(0, max(c - 1, 1)))
        out.append((min(r, c), max(r, c)))
    seen, res = set(pattern), []
    for p in out:
        if p[0] != p[1] and p not in seen:
            seen.add(p)
            res.append(p)
    return res


def unique_pairs(case, bs, nb, blocks):
    """The pairs (r <= c) whose reference blocks the fixture stores: the matrix's own pattern (with every diagonal block), then
    far_pairs."""
    pattern = sorted(blocks.keys(), key=lambda p: (p[1], p[0]))
    if case == "wide_panel64":                                   # every diagonal block, the corner, a third of the others
        return [p for p in pattern if p[0] == p[1] or p == (0, nb - 1) or (p[0] + 2 * p[1]) % 3 == 0]
    return pattern + far_pairs(case, bs, nb, pattern)


def requests(pairs):
    """The request list of the tests from the stored pairs (r <= c): every pair in both orientations (a diagonal block once),
    in stored order -- so the far-apart pairs outside the factor's pattern sit between in-pattern ones once a test permutes
    the list -- and the far corner (0, nb - 1) once more at the end.  Returns rows, cols, idx (index of the
    stored pair) and tr (True where the request is the transpose of the stored block)."""
    rows, cols, idx, tr = [], [], [], []
    for k, (r, c) in enumerate(pairs):
        rows.append(r), cols.append(c), idx.append(k), tr.append(False)
        if r != c:
            rows.append(c), cols.append(r), idx.append(k), tr.append(True)
    corner = [k for k, (r, c) in enumerate(pairs) if r == 0 and c == max(p[1] for p in pairs)][0]
    rows.append(pairs[corner][0]), cols.append(pairs[corner][1]), idx.append(corner), tr.append(False)     # one request repeated
    return np.array(rows, np.int32), np.array(cols, np.int32), np.array(idx), np.array(tr)


# ================================================================================================ fixture and measure
_cache = {}


def fixture():
    if "f" not in _cache:
        with np.load(FIXTURE) as f:
            _cache["f"] = {k: f[k] for k in f.files}
    return _cache["f"]


def load_case(case, bs):
    """dict(nb, bs, cp, ri, vals, pairs, Z [npairs][bs][bs], s [npairs], edges..., cpu_numpy, cpu_oracle) of one stored case
    (read-only arrays shared by every test)."""
    k = key(case, bs)
    if k in _cache:
        return _cache[k]
    f = fixture()
    g = lambda name: f[k + "/" + name]
    nb = int(g("nb"))
    E = dict(nb=nb, bs=bs, vi=g("vi"), vj=g("vj"), a0=g("a0"), J1=g("J1"), W=g("W").astype(np.float64), ui=g("ui"), ua=g("ua"),
             UW=g("UW"))
    c = dict(case=case, nb=nb, bs=bs, cp=g("cp"), ri=g("ri"), vals=g("vals"), pairs=[tuple(int(v) for v in p) for p in g("pairs")],
             Z=g("Z"), s=g("s"), E=E, cpu_numpy=float(g("cpu_numpy")), cpu_oracle=float(g("cpu_oracle")))
    c["rows"], c["cols"], c["idx"], c["tr"] = requests(c["pairs"])
    c["Zreq"] = np.array([c["Z"][i].T if t else c["Z"][i] for i, t in zip(c["idx"], c["tr"])])
    c["sreq"] = c["s"][c["idx"]]
    c["bound"] = 8.0 * max(c["cpu_numpy"], c["cpu_oracle"])
    own = set((int(r), int(cc)) for cc in range(nb) for r in c["ri"][c["cp"][cc]:c["cp"][cc + 1]])
    c["own"] = np.array([p in own for p in c["pairs"]])            # stored pairs on the matrix's own pattern (inside the factor's)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[k] = c
    return c


def ratios(M, Z, s):
    """err_i = max |M_i - Z_i| / (u s_i) per request."""
    M, Z = np.asarray(M), np.asarray(Z)
    return np.abs(M - Z).reshape(len(Z), -1).max(axis=1) / (U * np.asarray(s))


def old_measure_passes(M, Z, zmax):
    """The measure this replaces: every block to 1e-9 of the largest entry of the whole inverse."""
    return bool(np.all(np.abs(np.asarray(M) - np.asarray(Z)).reshape(len(Z), -1).max(axis=1) <= 1e-9 * zmax))


def blocks_of(Zd, bs, rows, cols):
    return np.array([Zd[bs * r:bs * (r + 1), bs * c:bs * (c + 1)] for r, c in zip(rows, cols)])


# ================================================================================================ fp64 on the CPU
def numpy_inverse(A):
    """NumPy Cholesky plus two triangular solves: Z = L^-T L^-1."""
    L = np.linalg.cholesky(A)
    Li = np.linalg.solve(L, np.eye(len(A)))
    return Li.T @ Li


def oracle_inverse_columns(O, c, columns):
    """{block column: n x bs} of the inverse by the oracle's column solves (one factorisation and a pair of sweeps each)."""
    nb, bs = c["nb"], c["bs"]
    out = {}
    for col in columns:
        X = np.zeros((nb * bs, bs))
        for k in range(bs):
            e = np.zeros(nb * bs)
            e[bs * col + k] = 1.0
            ok, x, _ = O.linear_solve_blocks(nb, bs, c["cp"], c["ri"], c["vals"], e)
            assert ok
            X[:, k] = x
        out[int(col)] = X
    return out


def oracle_blocks(O, c, rows, cols):
    X = oracle_inverse_columns(O, c, sorted(set(int(v) for v in cols)))
    bs = c["bs"]
    return np.array([X[int(cc)][bs * r:bs * (r + 1)] for r, cc in zip(rows, cols)])


# ================================================================================================ the two seams
def narrow_seam(capi, c, rows, cols, options=None):
    ls = capi.HipLinearSolver(c["bs"], 0)
    for name, value in (options or {}).items():
        ls.setOption(name, value)
    M = ls.solvePattern(c["cp"], c["ri"], c["vals"], rows, cols)
    return ls, M


def bind_edges(s, E):
    """The edges of a case on a solver object with the generic interface (Jacobians [dim * d] column-major, zero errors)."""
    bs, ne, nu = E["bs"], len(E["vi"]), len(E["ui"])
    kb = s.addEdgeSet(bs, E["vi"], E["vj"])
    ku = s.addEdgeSet(bs, E["ui"])
    s.buildStructure(E["nb"], 0, False)
    eye = np.eye(bs)
    J0 = np.array([(a * eye).T.reshape(-1) for a in E["a0"]])
    J1 = np.array([J.T.reshape(-1) for J in E["J1"]])
    s.setEdgeData(kb, J0, J1, np.ascontiguousarray(E["W"].reshape(ne, -1), np.float64), np.zeros((ne, bs)))
    Ju = np.array([(a * eye).T.reshape(-1) for a in E["ua"]])
    s.setEdgeData(ku, Ju, None, np.ascontiguousarray(E["UW"].reshape(nu, -1), np.float64), np.zeros((nu, bs)))


def wide_seam(capi, c, options=None):
    """HipBlockSolver with the case's edges, built; asserts that Hpp is the fixture's matrix bit for bit."""
    bs = c["bs"]
    s = capi.HipBlockSolver(bs, LANDMARK_DIM[bs], 0)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    bind_edges(s, c["E"])
    s.buildSystem()
    hcp, hri = s.pattern(capi.HPP)
    assert np.array_equal(hcp, c["cp"]) and np.array_equal(hri, c["ri"])
    assert np.array_equal(s.values(capi.HPP).reshape(-1, bs * bs), c["vals"]), "Hpp is not the fixture's matrix bit for bit"
    return s
