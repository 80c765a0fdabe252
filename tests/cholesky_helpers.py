"""Inputs, right-hand sides, exact arithmetic, measure and fixture loader of the sparse-Cholesky solve tests
(tests/golden/make_cholesky_solve.py, tests/test_cholesky_reference_host.py, tests/test_gpu_cholesky_solve.py).

MATRICES.  The construction of tests/inverse_helpers.py: binary edges J = -+ d I with small integer SPD information blocks and
one prior on block 0, so every entry of A is an integer (times a power of two in the graded case) and exact in fp64.  The
fixture stores no matrix: generator and tests rebuild it from make_edges(), and the fixture holds the SHA-256 of what they built.
    band         257 blocks; every block couples to the next and, by a fixed rule, to some of the blocks at +2 .. +4
    band_graded  the same matrix scaled D A D, D = 2^10 / 2^-10 in turn (same seed, same information blocks)
    band_tree    the same band, BAND_TREE_NB blocks (the length at which the plan has groups for tree_backward_kernel)
    grid         12 x 12 / 10 x 10 / 10 x 10 grid Laplacian (nested dissection, several levels, LDS fronts only)
    slab512      SLAB_CHAINS chains of SLAB_CHAIN_LEN blocks, every chain block tied to each of h fully connected hub blocks:
    slab1024     fronts of 512 .. 1023 rows and of 1024 rows and more (HUBS)
    decay        the diagonally dominant tridiagonal chain of inverse_helpers ("chain_decay"), whose inverse decays by 1e-33
                 over its 40 blocks: the only case whose impulse solution has blocks far below the largest
RIGHT-HAND SIDES.  "dense": random multiples of 1/8; "impulse": blocks 0 and nb - 1 nonzero multiples of 1/8, the rest zero.

REFERENCE.  xref = hi + lo + lo2 exactly (three fp64 numbers per component, hi = fl(xref), lo = fl(xref - hi)); it comes from
iterative refinement with residuals evaluated in exact integer arithmetic (every input is dyadic) and carries the certificate
    |b - A xref| <= 2^-120 (|A| |xref| + |b|)   componentwise, evaluated exactly (certificate()).

MEASURE.  err_i = max |x_i - xref_i| / (u s_i) per block i, u = 2^-53, s_i the largest entry of block i of
|Z| d (d' |xref|) with d = sqrt(diag A) and Z the fp64 inverse: the forward form of the scaled backward error of Cholesky,
|dA| <= c u d d'.  It does not depend on the elimination order and is invariant under D A D.  No floor, no global scale other
than the one number d' |xref| the bound itself carries.  The bound per (case, block size, right-hand side) is 8 x the larger
of two fp64 figures of the CPU under the same measure (SciPy's Cholesky with two triangular solves; the oracle)."""
import hashlib
import math
import os

import numpy as np

from tests import inverse_helpers as IH

U = 2.0 ** -53
MARGIN = 8.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cholesky_solve.npz")
CASES = {"band": (6,), "band_graded": (6,), "band_tree": (6, 3), "grid": (3, 6, 7), "slab512": (3, 6, 7), "slab1024": (3, 6, 7),
         "decay": (3, 6, 7)}
PARAMS = [(case, bs) for case, sizes in CASES.items() for bs in sizes]
RHS = ("dense", "impulse")
BAND_NB = 257
# smallest of 513 / 1025 / 1537 blocks whose plan has groups of fronts for tree_backward_kernel (treeBackwardGroups > 0 at the
# defaults, both block sizes; the probe is recorded in DESIGN.md, section 5)
BAND_TREE_NB = 513
GRID_SIDE = {3: 12, 6: 10, 7: 10}
SLAB_CHAINS, SLAB_CHAIN_LEN = 3, 8
# hub blocks: chosen from maxFrontDim of one stats() probe each
HUBS = {"slab512": {3: 180, 6: 90, 7: 78}, "slab1024": {3: 350, 6: 175, 7: 150}}
GRADE = 10                                                       # D = 2^10 / 2^-10 in turn
CERT_BITS = 120
_SEED = {"band": 5000, "band_graded": 5000, "band_tree": 5100, "grid": 5200, "slab512": 5300, "slab1024": 5400}

VARIANTS = {
    "band": ({}, {"band_kernel": 0}, {"dep_levels": 0}, {"tree_backward": 0}, {"tree_backward": 2}),
    "grid": ({}, {"dep_levels": 0}, {"dep_levels": 16, "dep_backward": 0}, {"max_sn_scalars_lds": 24}),
    "slab": ({}, {"dep_levels": 0}, {"big_front_passes": 0}, {"big_group": 4, "big_group_min_rows": 64},
             {"big_group": 1, "big_group_min_rows": 64}),
    "decay": ({}, {"dep_levels": 0}),
}


def variants(case):
    return VARIANTS["band" if case.startswith("band") else "slab" if case.startswith("slab") else case]


def variant_name(opts):
    return ",".join("%s=%d" % kv for kv in sorted(opts.items())) or "default"


def key(case, bs):
    return "%s_b%d" % (case, bs)


# ================================================================================================ inputs
def band_pairs(nb):
    """(c, c + 1), (c, c + 2) and (c, c + 4) for every c, (c, c + 3) for even c.  (The planner puts a leaf chain on the band
    kernel only if nested dissection's local order keeps every row of L within four blocks of its column; of the thinned
    bands tried against the host planner this one keeps most leaf chains there, thinner ones none.)"""
    pairs = [(c, c + k) for c in range(nb) for k in (1, 2, 3, 4) if c + k < nb and (k != 3 or c % 2 == 0)]
    return sorted(pairs)


def graded_scale(nb):
    return np.array([2.0 ** (GRADE if i % 2 == 0 else -GRADE) for i in range(nb)])


def make_edges(case, bs):
    if case == "decay":
        return IH.make_edges("chain_decay", bs)
    rng = np.random.RandomState(_SEED[case] + bs)
    if case in ("band", "band_graded", "band_tree"):
        nb = BAND_TREE_NB if case == "band_tree" else BAND_NB
        return IH._laplacian_edges(rng, bs, nb, band_pairs(nb), graded_scale(nb) if case == "band_graded" else None)
    if case == "grid":
        g = GRID_SIDE[bs]
        pairs = [(y * g + x, y * g + x + 1) for y in range(g) for x in range(g - 1)]
        pairs += [(y * g + x, (y + 1) * g + x) for y in range(g - 1) for x in range(g)]
        return IH._laplacian_edges(rng, bs, g * g, sorted(pairs))
    if case in HUBS:
        nc, ln, h = SLAB_CHAINS, SLAB_CHAIN_LEN, HUBS[case][bs]
        pairs = [(q * ln + c - 1, q * ln + c) for q in range(nc) for c in range(1, ln)]
        pairs += [(c, nc * ln + k) for c in range(nc * ln) for k in range(h)]
        pairs += [(nc * ln + k, nc * ln + k2) for k in range(h) for k2 in range(k + 1, h)]
        return IH._laplacian_edges(rng, bs, nc * ln + h, sorted(pairs))
    raise KeyError(case)


def make_rhs(case, bs, nb):
    """{"dense": b, "impulse": b}; band and band_graded draw the same numbers."""
    rng = np.random.RandomState(_SEED.get(case, 5500) + 50 + bs)
    n = nb * bs
    dense = rng.randint(-64, 65, n) / 8.0
    imp = np.zeros(n)
    ends = rng.randint(1, 65, 2 * bs) * np.where(rng.randint(0, 2, 2 * bs) == 1, 1.0, -1.0) / 8.0
    imp[:bs], imp[n - bs:] = ends[:bs], ends[bs:]
    return {"dense": dense, "impulse": imp}


_cache = {}


def matrix(case, bs):
    """dict(case, bs, nb, n, cp, ri, vals, b {rhs: vector}, sha) rebuilt from the seeds (cached, read-only)."""
    k = ("m", case, bs)
    if k not in _cache:
        E = make_edges(case, bs)
        nb = E["nb"]
        cp, ri, vals = IH.to_ccs(nb, IH.assemble(E))
        b = make_rhs(case, bs, nb)
        h = hashlib.sha256()
        for a in (cp, ri, vals, b["dense"], b["impulse"]):
            h.update(np.ascontiguousarray(a).tobytes())
        for a in (cp, ri, vals, b["dense"], b["impulse"]):
            a.setflags(write=False)
        _cache[k] = dict(case=case, bs=bs, nb=nb, n=nb * bs, cp=cp, ri=ri, vals=vals, b=b, sha=h.hexdigest())
    return _cache[k]


def dense(m):
    return IH.dense_from_ccs(m["nb"], m["bs"], m["cp"], m["ri"], m["vals"])


def unscaled(m):
    """(the matrix whose entries are integers times 2^-k with a small k, D) with A = D A0 D: band_graded refines and certifies in
    the coordinates of `band` (D is a power of two, so the change of coordinates is exact); D = None elsewhere."""
    if m["case"] == "band_graded":
        return matrix("band", m["bs"]), np.repeat(graded_scale(m["nb"]), m["bs"])
    return m, None


# ================================================================================================ exact arithmetic on dyadic numbers
def lsb_exponent(v):
    """An e with v 2^-e integer for every entry of the fp64 array v."""
    ex = [math.frexp(float(x))[1] for x in np.asarray(v).reshape(-1) if x != 0.0]
    return (min(ex) if ex else 0) - 53


def to_int(v, e):
    """Object array of the integers v 2^-e (exact; asserts that they are integers)."""
    out = np.empty(len(v), object)
    for i, x in enumerate(v):
        mant, ex = math.frexp(float(x))
        mi, sh = int(mant * 9007199254740992.0), ex - 53 - e
        if sh >= 0:
            out[i] = mi << sh
        else:
            assert mi % (1 << -sh) == 0, "not an integer at this scale"
            out[i] = mi >> -sh
    return out


def from_int(X, e):
    """fl(X 2^e) per entry (float() of a Python integer rounds to nearest even)."""
    return np.array([math.ldexp(float(x), e) for x in X])


class ExactMatrix:
    """A = Aint 2^-k with integer Aint (int64, sparse): exact products with vectors of Python integers through 24-bit limbs."""

    def __init__(self, A):
        import scipy.sparse as sp
        k = 0
        while not np.array_equal(np.round(A * 2.0 ** k), A * 2.0 ** k):
            k += 1
            assert k <= 40
        self.k = k
        Ai = np.round(A * 2.0 ** k)
        assert np.abs(Ai).sum(axis=1).max() < 2.0 ** 38          # 2^38 x 2^24 < 2^63
        self.M = sp.csr_matrix(Ai.astype(np.int64))
        self.Mabs = abs(self.M)

    @staticmethod
    def _limbs(X):
        nl = max(1, (max((abs(int(x)).bit_length() for x in X), default=1) + 23) // 24)
        out = np.zeros((len(X), nl), np.int64)
        for i, x in enumerate(X):
            x = int(x)
            s, a = (-1 if x < 0 else 1), abs(x)
            for l in range(nl):
                out[i, l] = s * (a & 0xFFFFFF)
                a >>= 24
                if not a:
                    break
        return out

    @staticmethod
    def _join(P):
        out = np.empty(P.shape[0], object)
        for i in range(P.shape[0]):
            v = 0
            for l in range(P.shape[1] - 1, -1, -1):
                v = (v << 24) + int(P[i, l])
            out[i] = v
        return out

    def dot(self, X, absolute=False):
        """Aint X (or |Aint| |X|) as Python integers."""
        if absolute:
            return self._join(self.Mabs @ self._limbs([abs(int(x)) for x in X]))
        return self._join(self.M @ self._limbs(X))

    def residual(self, X, e, b):
        """(R, T, er) with b - A X 2^e = R 2^er and |A| |X| 2^e + |b| = T 2^er, all exact."""
        er = e - self.k
        B = to_int(b, er)
        R = B - self.dot(X)
        T = self.dot(X, absolute=True) + np.array([abs(int(v)) for v in B], object)
        return R, T, er


def certified(R, T, bits=CERT_BITS):
    """|R| <= 2^-bits T componentwise."""
    return all((abs(int(r)) << bits) <= int(t) for r, t in zip(R, T))


def triple_of(X, e):
    """(hi, lo, lo2): fl(x), fl(x - hi), fl(x - hi - lo) of x = X 2^e."""
    hi = from_int(X, e)
    R1 = X - to_int(hi, e)
    lo = from_int(R1, e)
    lo2 = from_int(R1 - to_int(lo, e), e)
    return hi, lo, lo2


def sum_int(terms):
    """(X, e) with sum(terms) = X 2^e exactly."""
    e = min(lsb_exponent(t) for t in terms)
    X = to_int(terms[0], e)
    for t in terms[1:]:
        X = X + to_int(t, e)
    return X, e


def certificate(m, hi, lo, lo2, b):
    """The certificate of xref = hi + lo + lo2 for the matrix of m and right-hand side b, evaluated exactly (band_graded in the
    coordinates of band: y = D x, right-hand side D^-1 b, both exact)."""
    m0, D = unscaled(m)
    if D is not None:
        hi, lo, lo2, b = hi * D, lo * D, lo2 * D, b / D
    X, e = sum_int([hi, lo, lo2])
    R, T, _ = exact_matrix(m0).residual(X, e, b)
    return certified(R, T)


def exact_matrix(m):
    k = ("x", m["case"], m["bs"])
    if k not in _cache:
        _cache[k] = ExactMatrix(dense(m))
    return _cache[k]


# ================================================================================================ measure
def block_max(v, bs):
    return np.abs(v).reshape(-1, bs).max(axis=1)


def scales(A, Z, xref, bs):
    """(s, sa): per block the largest entry of |Z| d (d' |xref|), and of |Z| |A| |xref| (recorded for information only)."""
    d = np.sqrt(np.diag(A))
    aZ, ax = np.abs(Z), np.abs(xref)
    return block_max((aZ @ d) * float(d @ ax), bs), block_max(aZ @ (np.abs(A) @ ax), bs)


def ratios(x, c, rhs, which="s"):
    """err_i per block against the stored reference (x - hi is exact or nearly so; lo is then subtracted)."""
    r = c[rhs]
    return block_max((np.asarray(x) - r["hi"]) - r["lo"], c["bs"]) / (U * r[which])


def relerr_old(x, xr):
    """The check this replaces (tests/helpers.relerr): one global figure."""
    return np.abs(x - xr).max() / np.abs(xr).max()


# ================================================================================================ fp64 on the CPU
def scipy_cholesky_solve(A, b):
    """SciPy's Cholesky factor and two triangular solves."""
    import scipy.linalg as sl
    L = sl.cholesky(A, lower=True)
    return sl.solve_triangular(L, sl.solve_triangular(L, b, lower=True), lower=True, trans="T")


def oracle_solve(m, b):
    from oracle import oracle as O
    ok, x, _ = O.linear_solve_blocks(m["nb"], m["bs"], m["cp"], m["ri"], m["vals"], b)
    assert ok
    return x


# ================================================================================================ fixture
def fixture():
    if "f" not in _cache:
        with np.load(FIXTURE) as f:
            _cache["f"] = {k: f[k] for k in f.files}
    return _cache["f"]


def load_case(case, bs):
    """The rebuilt matrix of (case, bs) with, per right-hand side, dict(b, hi, lo, lo2, s, sa, cpu_scipy, cpu_oracle, bound)
    from the fixture (and dir_hi, dir_lo for band); read-only and shared."""
    k = ("c", case, bs)
    if k in _cache:
        return _cache[k]
    f = fixture()
    c = dict(matrix(case, bs))
    p = key(case, bs) + "/"
    c["stored_sha"] = str(f[p + "sha"])
    for rhs in RHS:
        r = dict(b=c["b"][rhs])
        for name in ("hi", "lo", "lo2", "s", "sa", "dir_hi", "dir_lo"):
            if p + rhs + "/" + name in f:
                r[name] = f[p + rhs + "/" + name].astype(np.float64)       # (lo2 is stored in fp32 where that keeps the certificate)
                r[name].setflags(write=False)
        for name in ("cpu_scipy", "cpu_oracle", "cpu_scipy_sa", "cpu_oracle_sa"):
            r[name] = float(f[p + rhs + "/" + name])
        r["bound"] = MARGIN * max(r["cpu_scipy"], r["cpu_oracle"])
        c[rhs] = r
    _cache[k] = c
    return c
