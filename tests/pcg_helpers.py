"""Reference and inputs of the PCG step tests (tests/golden/make_pcg_steps.py, tests/test_pcg_reference_host.py,
tests/test_gpu_pcg_steps.py).

REFERENCE (mpmath, 60 digits as tests/reference_mp.py).  PcgMp restates LinearSolverPCG::solve
(g2o/solvers/pcg/linear_solver_pcg.hpp:79-196) statement by statement on an upper block-CCS matrix: block-Jacobi
preconditioner J_i = A_ii^-1 (inverted at 60 digits), x0 = 0, d0 = tolerance * dn0 raised to the carried residual when the
tolerance is absolute, "if (dn <= d0) break" at the head of every iteration, _residual = 0.5 * dn afterwards.  It keeps x_k
and dn_k of every iteration.  reduced_operator_mp forms S = Hpp + lam I - Hpl (Hll + lam I)^-1 Hpl' and
b_s = b_p - Hpl (Hll + lam I)^-1 b_l.  Neither shares code with block_pcg.hip or oracle/g2o_oracle.c.

INPUTS (NumPy only; the GPU tests regenerate them from the seeds stored in the fixture).  Jacobians and errors are integers in
-3 .. 3 (times powers of ten in the block-diagonal group), the information is the identity and lambda is an integer, so
sum J'J + lambda I and -sum J'e are integers far below 2^53: exact in fp64 in any summation order.  *_system build them in int64.

Layouts as in the project: a Jacobian is [d x dim] column-major per edge, a matrix block column-major, block-CCS columns hold
rows <= column in increasing order."""
import numpy as np

from tests import reference_mp as M

mp = M.mp
LAMBDA = 2                      # the damping of every stored system (an integer)


# ================================================================================================ reference (mpmath)
def _mpf_block(blk):
    return [[mp.mpf(int(v)) if isinstance(v, (int, np.integer)) else mp.mpf(v) for v in row] for row in blk]


def _inverse(blk):
    n = len(blk)
    inv = mp.matrix(_mpf_block(blk)) ** -1
    return [[inv[r, c] for c in range(n)] for r in range(n)]


def _mul_block(B, v, off, bs):
    seg = v[off:off + bs]
    return [mp.fdot(B[r], seg) for r in range(bs)]


def _dot(a, b):
    return mp.fdot(a, b)


def _transposed(B):
    return [list(c) for c in zip(*B)]


class PcgMp:
    """LinearSolverPCG::solve on the upper block-CCS matrix (colptr, row, blocks[q][r][c]); run() is the loop of :132-147."""

    def __init__(self, nb, bs, colptr, row, blocks, b):
        self.nb, self.bs, self.n = nb, bs, nb * bs
        self.diag, self.upper = [None] * nb, []                  # _diag; (_indices, _sparseMat): strictly upper blocks
        for c in range(nb):
            for q in range(int(colptr[c]), int(colptr[c + 1])):
                r = int(row[q])
                if r == c:
                    self.diag[c] = _mpf_block(blocks[q])
                    break
                a = _mpf_block(blocks[q])
                self.upper.append((r, c, a, _transposed(a)))
        assert all(d is not None for d in self.diag)
        self.J = [_inverse(d) for d in self.diag]                # _J: it->second->inverse()
        self.b = [mp.mpf(int(v)) if isinstance(v, (int, np.integer)) else mp.mpf(v) for v in b]

    def mult_diag(self, blocks, src):
        out = []
        for i in range(self.nb):
            out += _mul_block(blocks[i], src, i * self.bs, self.bs)
        return out

    def mult(self, src):
        bs = self.bs
        dest = self.mult_diag(self.diag, src)
        for r, c, a, at in self.upper:
            sc, sr = src[c * bs:(c + 1) * bs], src[r * bs:(r + 1) * bs]
            for i in range(bs):
                dest[r * bs + i] += mp.fdot(a[i], sc)            # dest_r += a src_c
                dest[c * bs + i] += mp.fdot(at[i], sr)           # dest_c += a' src_r
        return dest

    def run(self, tolerance=1e-6, absolute=True, residual=-1.0, max_iter=-1, keep=None, until=None):
        """Returns dict(x = {k: x_k} (only the iterations in `keep` when given), dn = [dn_0 .. dn_it], d0, iterations,
        residual = 0.5 dn_it).  until(dn): the recording may end once it returns True (no part of the operation)."""
        n = self.n
        x = [mp.mpf(0)] * n
        r = list(self.b)
        d = self.mult_diag(self.J, r)
        dn = _dot(r, d)
        d0 = mp.mpf(tolerance) * dn
        if absolute:
            if residual > 0 and residual > d0:
                d0 = mp.mpf(residual)
        max_iter = n if max_iter < 0 else max_iter
        xs, dns = {}, [dn]
        iteration = 0
        while iteration < max_iter:
            if dn <= d0:
                break
            q = self.mult(d)
            a = dn / _dot(d, q)
            x = [xi + a * di for xi, di in zip(x, d)]
            r = [ri - a * qi for ri, qi in zip(r, q)]
            s = self.mult_diag(self.J, r)
            dold = dn
            dn = _dot(r, s)
            ba = dn / dold
            d = [si + ba * di for si, di in zip(s, d)]
            iteration += 1
            dns.append(dn)
            if keep is None or iteration in keep:
                xs[iteration] = x
            if until is not None and until(dns):
                break
        return dict(x=xs, dn=dns, d0=d0, iterations=iteration, residual=mp.mpf("0.5") * dn, x_last=x)


def stop_iteration(dn, d0):
    """The iteration count of the loop above for the recorded sequence dn_0, dn_1, ...: the first k with dn_k <= d0 (the
    sequence must be long enough to hold it)."""
    for k, v in enumerate(dn):
        if v <= d0:
            return k
    raise AssertionError("the recorded dn sequence ends above the stopping level")


def direct_solve_mp(nb, bs, colptr, row, blocks, b):
    """Dense LU at 60 digits of the same symmetric matrix (small systems only)."""
    n = nb * bs
    A = mp.matrix(n, n)
    for c in range(nb):
        for q in range(int(colptr[c]), int(colptr[c + 1])):
            r = int(row[q])
            for i in range(bs):
                for j in range(bs):
                    A[r * bs + i, c * bs + j] = mp.mpf(blocks[q][i][j])
                    A[c * bs + j, r * bs + i] = mp.mpf(blocks[q][i][j])
    x = mp.lu_solve(A, mp.matrix([mp.mpf(int(v)) if isinstance(v, (int, np.integer)) else mp.mpf(v) for v in b]))
    return [x[i] for i in range(n)]


def reduced_operator_mp(nP, p, l, pp, obs, Hll, lam, b):
    """S = Hpp + lam I - Hpl (Hll + lam I)^-1 Hpl' as upper blocks {(r, c): [p][p]} and b_s = b_p - Hpl (Hll + lam I)^-1 b_l.
    pp: {(r, c): p x p} upper blocks of Hpp (r <= c); obs: per landmark a list of (pose, p x l block of Hpl); Hll: per
    landmark l x l; b: poses then landmarks."""
    lam = mp.mpf(lam)
    S = {k: _mpf_block(v) for k, v in pp.items()}
    for i in range(nP):
        for k in range(p):
            S[(i, i)][k][k] += lam
    bs = [mp.mpf(int(v)) for v in b[:nP * p]]
    for j, ob in enumerate(obs):
        D = _mpf_block(Hll[j])
        for k in range(l):
            D[k][k] += lam
        Dinv = _inverse(D)
        bl = [mp.mpf(int(v)) for v in b[nP * p + j * l:nP * p + (j + 1) * l]]
        T = {}                                                   # B Dinv per observing pose
        for i, B in ob:
            Bm = _mpf_block(B)
            T[i] = [[mp.fdot(Bm[r], Dinv[c]) for c in range(l)] for r in range(p)]       # (Dinv is symmetric)
            for r in range(p):
                bs[i * p + r] -= mp.fdot(T[i][r], bl)
        for i, _ in ob:
            for i2, B2 in ob:
                if i > i2:
                    continue
                blk = S.setdefault((i, i2), [[mp.mpf(0)] * p for _ in range(p)])
                B2m = _mpf_block(B2)
                for r in range(p):
                    for c in range(p):
                        blk[r][c] -= mp.fdot(T[i][r], B2m[c])
    return S, bs


def blocks_to_ccs(nb, blocks):
    """{(r, c): block} (r <= c) -> colptr, row, [block] with the rows of a column increasing."""
    cols = [[] for _ in range(nb)]
    for (r, c) in blocks:
        assert r <= c
        cols[c].append(r)
    colptr, row, out = [0], [], []
    for c in range(nb):
        for r in sorted(cols[c]):
            row.append(r)
            out.append(blocks[(r, c)])
        colptr.append(len(row))
    return np.array(colptr, np.int32), np.array(row, np.int32), out


def f64(v):
    return np.array([float(t) for t in v], np.float64)


def ccs_values(blocks):
    """[q][r][c] -> [q][bs * bs] column-major fp64."""
    return np.array([[float(blk[r][c]) for c in range(len(blk)) for r in range(len(blk))] for blk in blocks], np.float64)


def figure(got, ref):
    """max |got - ref| / max |ref| (1 where the reference is all zero and the result is not)."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    m = float(np.abs(ref).max())
    e = float(np.abs(got - ref).max())
    return e / m if m > 0 else (0.0 if e == 0 else 1.0)


def figure_per_block(got, ref, bs):
    got, ref = np.asarray(got, np.float64).reshape(-1, bs), np.asarray(ref, np.float64).reshape(-1, bs)
    return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


# ================================================================================================ inputs (NumPy)
CHAIN_NB = (1, 255, 256, 257, 513)
CHAIN_BS = {3: CHAIN_NB, 6: CHAIN_NB, 7: (1, 257)}               # block size 7 at the two sizes that bound the mp time
LANDMARK_DIM = {3: 2, 6: 3, 7: 3}
STEPS = (1, 2, 3, 8)
DIAG_BLOCKS = 300
RED_POSES, RED_LANDMARKS = 257, 600


def chain_case_name(bs, nb):
    return "chain_b%d_n%d" % (bs, nb)


def _jac(J, dim, d):
    """[dim * d] column-major -> d x dim."""
    return J.reshape(dim, d).T


def chain_inputs(seed, nb, bs):
    """A chain 0-1-...-(nb-1) with about 10 % random closures (binary edges, error dimension bs) and one unary edge per
    vertex.  Returns dict(vi, vj, J0, J1, e, Ju, eu) with int64 entries in -3 .. 3."""
    rng = np.random.RandomState(seed)
    vi, vj = list(range(nb - 1)), list(range(1, nb))
    nc = int(round(0.1 * nb)) if nb >= 3 else 0
    for _ in range(nc):
        a = int(rng.randint(0, nb - 2))
        b = int(rng.randint(a + 2, nb))
        if rng.rand() < 0.5:
            a, b = b, a                                          # (either vertex order: blocks above and "below" the diagonal)
        vi.append(a)
        vj.append(b)
    ne = len(vi)
    r = lambda *shape: rng.randint(-3, 4, shape).astype(np.int64)
    return dict(vi=np.array(vi, np.int32), vj=np.array(vj, np.int32), J0=r(ne, bs * bs), J1=r(ne, bs * bs), e=r(ne, bs),
                Ju=r(nb, bs * bs), eu=r(nb, bs))


def chain_system(inp, nb, bs, lam=LAMBDA):
    """sum J'J + lam I (upper blocks {(r, c): int64 bs x bs}) and b = -sum J'e of chain_inputs, exactly."""
    blocks = {(i, i): lam * np.eye(bs, dtype=np.int64) for i in range(nb)}
    b = np.zeros(nb * bs, np.int64)
    for i in range(nb):
        J = _jac(inp["Ju"][i], bs, bs)
        blocks[(i, i)] += J.T @ J
        b[i * bs:(i + 1) * bs] -= J.T @ inp["eu"][i]
    for k in range(len(inp["vi"])):
        i, j = int(inp["vi"][k]), int(inp["vj"][k])
        A, B, e = _jac(inp["J0"][k], bs, bs), _jac(inp["J1"][k], bs, bs), inp["e"][k]
        blocks[(i, i)] += A.T @ A
        blocks[(j, j)] += B.T @ B
        b[i * bs:(i + 1) * bs] -= A.T @ e
        b[j * bs:(j + 1) * bs] -= B.T @ e
        key, blk = ((i, j), A.T @ B) if i < j else ((j, i), B.T @ A)
        blocks[key] = blocks.get(key, np.zeros((bs, bs), np.int64)) + blk
    return blocks, b


def diag_inputs(seed, bs, n=DIAG_BLOCKS):
    """Unary edges only, one per vertex: J = M diag(10^k) with M integer in -3 .. 3 (diagonal 4 .. 6: well conditioned) and
    k in 0 .. 4 per column, so the blocks J'J + lam I have condition numbers from 1 to 1e8 that come from their scaling;
    block 0 has J = 4 I (condition 1)."""
    rng = np.random.RandomState(seed)
    Ju = np.zeros((n, bs * bs), np.int64)
    Ju[0] = (4 * np.eye(bs, dtype=np.int64)).reshape(-1)
    for i in range(1, n):
        Mi = rng.randint(-1, 2, (bs, bs)).astype(np.int64)
        Mi[np.arange(bs), np.arange(bs)] = rng.randint(4, 7, bs)
        top = (i * 5) // n                                       # largest exponent 0 .. 4 across the group
        k = rng.randint(0, top + 1, bs)
        a = int(rng.randint(0, bs))
        k[a], k[(a + 1) % bs] = top, 0                           # (both ends of the range in every block)
        Ju[i] = (Mi * (10 ** k)[None, :]).T.reshape(-1)
    eu = rng.randint(-3, 4, (n, bs)).astype(np.int64)
    eu[eu == 0] = 1
    return dict(Ju=Ju, eu=eu)


def diag_system(inp, bs, lam=LAMBDA):
    n = len(inp["Ju"])
    blocks, b = {}, np.zeros(n * bs, np.int64)
    for i in range(n):
        J = _jac(inp["Ju"][i], bs, bs)
        blocks[(i, i)] = J.T @ J + lam * np.eye(bs, dtype=np.int64)
        b[i * bs:(i + 1) * bs] = -(J.T @ inp["eu"][i])
    return blocks, b


def reduced_inputs(seed, p, l, nP=RED_POSES, nL=RED_LANDMARKS):
    """nP poses on a chain (binary pose-pose edges, error dimension p), nL landmarks seen from 2 - 4 poses each (error
    dimension l), poses 5 and nP - 2 seen by no landmark; one unary edge on each of those two.  Integer v for S v."""
    rng = np.random.RandomState(seed)
    blind = (5, nP - 2)
    seeing = np.array([i for i in range(nP) if i not in blind])
    lp, ll = [], []
    for j in range(nL):
        k = int(rng.randint(2, 5))
        c = j % len(seeing)                                      # (every seeing pose is some landmark's first observer)
        lo = min(max(c - 6, 0), len(seeing) - 13)
        near = np.array([i for i in seeing[lo:lo + 13] if i != seeing[c]])
        for i in sorted([int(seeing[c])] + rng.choice(near, k - 1, replace=False).tolist()):
            lp.append(i)
            ll.append(j)
    ne = len(lp)
    r = lambda *shape: rng.randint(-3, 4, shape).astype(np.int64)
    return dict(vi=np.arange(nP - 1, dtype=np.int32), vj=np.arange(1, nP, dtype=np.int32), J0=r(nP - 1, p * p), J1=r(nP - 1, p * p),
                e=r(nP - 1, p), lp=np.array(lp, np.int32), ll=np.array(ll, np.int32), Jl=r(ne, l * l), Jp=r(ne, l * p), el=r(ne, l),
                blind=np.array(blind, np.int32), Ju=r(2, p * p), eu=r(2, p), v=r(nP * p), vfull=r(nP * p + nL * l))


def reduced_system(inp, p, l, nP=RED_POSES, nL=RED_LANDMARKS):
    """Undamped Hpp (upper blocks), per landmark [(pose, Hpl block p x l)], Hll blocks and b, exactly (int64)."""
    pp = {(i, i): np.zeros((p, p), np.int64) for i in range(nP)}
    b = np.zeros(nP * p + nL * l, np.int64)
    for k in range(nP - 1):
        i, j = int(inp["vi"][k]), int(inp["vj"][k])
        A, B, e = _jac(inp["J0"][k], p, p), _jac(inp["J1"][k], p, p), inp["e"][k]
        pp[(i, i)] += A.T @ A
        pp[(j, j)] += B.T @ B
        pp[(i, j)] = pp.get((i, j), np.zeros((p, p), np.int64)) + A.T @ B
        b[i * p:(i + 1) * p] -= A.T @ e
        b[j * p:(j + 1) * p] -= B.T @ e
    for k, i in enumerate(inp["blind"]):
        J = _jac(inp["Ju"][k], p, p)
        pp[(int(i), int(i))] += J.T @ J
        b[i * p:(i + 1) * p] -= J.T @ inp["eu"][k]
    obs = [[] for _ in range(nL)]
    Hll = [np.zeros((l, l), np.int64) for _ in range(nL)]
    for k in range(len(inp["lp"])):
        i, j = int(inp["lp"][k]), int(inp["ll"][k])
        A, B, e = _jac(inp["Jl"][k], l, l), _jac(inp["Jp"][k], p, l), inp["el"][k]   # landmark (l x l), pose (l x p)
        Hll[j] += A.T @ A
        pp[(i, i)] += B.T @ B
        obs[j].append((i, B.T @ A))
        b[i * p:(i + 1) * p] -= B.T @ e
        b[nP * p + j * l:nP * p + (j + 1) * l] -= A.T @ e
    return pp, obs, Hll, b


def full_product(pp, obs, Hll, p, l, nP, nL, lam, v):
    """[Hpp + lam I, Hpl; Hpl', Hll + lam I] v in int64."""
    v = np.asarray(v, np.int64)
    out = lam * v.copy()
    for (r, c), blk in pp.items():
        out[r * p:(r + 1) * p] += blk @ v[c * p:(c + 1) * p]
        if r != c:
            out[c * p:(c + 1) * p] += blk.T @ v[r * p:(r + 1) * p]
    o = nP * p
    for j in range(nL):
        out[o + j * l:o + (j + 1) * l] += Hll[j] @ v[o + j * l:o + (j + 1) * l]
        for i, B in obs[j]:
            out[i * p:(i + 1) * p] += B @ v[o + j * l:o + (j + 1) * l]
            out[o + j * l:o + (j + 1) * l] += B.T @ v[i * p:(i + 1) * p]
    return out


def col(J):
    return np.ascontiguousarray(J, np.float64)


def eye_info(n, d):
    return np.tile(np.eye(d).reshape(-1), (n, 1))


# ---- the same inputs through the generic path of a solver object (device: capi.HipBlockSolver; oracle: O.OracleSolver) -------
def device_chain(capi, inp, nb, bs, lam=LAMBDA, options=None):
    s = capi.HipBlockSolver(bs, LANDMARK_DIM[bs], 0)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    bind_chain(s, inp, nb, bs)
    s.buildSystem()
    s.setLambda(float(lam), True)
    return s


def bind_chain(s, inp, nb, bs):
    ku = s.addEdgeSet(bs, np.arange(nb, dtype=np.int32))
    kb = s.addEdgeSet(bs, inp["vi"], inp["vj"]) if len(inp["vi"]) else None
    s.buildStructure(nb, 0, False)
    s.setEdgeData(ku, col(inp["Ju"]), None, eye_info(nb, bs), col(inp["eu"]))
    if kb is not None:
        s.setEdgeData(kb, col(inp["J0"]), col(inp["J1"]), eye_info(len(inp["vi"]), bs), col(inp["e"]))


def device_diag(capi, inp, bs, lam=LAMBDA, options=None):
    n = len(inp["Ju"])
    s = capi.HipBlockSolver(bs, LANDMARK_DIM[bs], 0)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    ku = s.addEdgeSet(bs, np.arange(n, dtype=np.int32))
    s.buildStructure(n, 0, False)
    s.setEdgeData(ku, col(inp["Ju"]), None, eye_info(n, bs), col(inp["eu"]))
    s.buildSystem()
    s.setLambda(float(lam), True)
    return s


def device_reduced(capi, inp, p, l, lam=LAMBDA, options=None, nP=RED_POSES, nL=RED_LANDMARKS, schur=True):
    s = capi.HipBlockSolver(p, l, 0)
    for name, value in (options or {}).items():
        s.setOption(name, value)
    kb = s.addEdgeSet(p, inp["vi"], inp["vj"])
    ku = s.addEdgeSet(p, inp["blind"])
    kl = s.addEdgeSet(l, nP + inp["ll"], inp["lp"])                  # vertex 0 = landmark, vertex 1 = pose
    s.buildStructure(nP, nL, schur)
    s.setEdgeData(kb, col(inp["J0"]), col(inp["J1"]), eye_info(nP - 1, p), col(inp["e"]))
    s.setEdgeData(ku, col(inp["Ju"]), None, eye_info(2, p), col(inp["eu"]))
    s.setEdgeData(kl, col(inp["Jl"]), col(inp["Jp"]), eye_info(len(inp["lp"]), l), col(inp["el"]))
    s.buildSystem()
    s.setLambda(float(lam), True)
    return s
