"""GPU: the device PCG (block_pcg.hip) and the matrix-free reduced operator (mf_pose_kernel, mf_diag_kernel, schur_operator_*)
step by step against tests/golden/pcg_steps.npz: the extended-precision iterates of LinearSolverPCG::solve and the iteration
counts of its stopping rule on integer systems (tests/golden/make_pcg_steps.py; inputs regenerated here from the stored seeds).
Nothing here evaluates a reference, except the ring test, whose x_1 is predictable bit for bit from int64 arithmetic.

Bound of every comparison: 8 x the CPU oracle's own figure max |x - ref| / max |ref| against the same reference
(tests/producer_metric.py: MARGIN, CEILING).  Iteration counts are exact: the generator keeps every dn_k a relative 1e-6 away
from the stopping levels.  Every comparison prints a PCG_FIGURE line."""
import json
import os

import numpy as np
import pytest

from tests import pcg_helpers as H
from tests import producer_metric as PM

pytestmark = pytest.mark.gpu

FX = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcg_steps.npz")))
CHAINS = [(bs, nb) for bs in sorted(H.CHAIN_BS) for nb in H.CHAIN_BS[bs]]
SHAPES = [(p, H.LANDMARK_DIM[p]) for p in sorted(H.LANDMARK_DIM)]
LAM = int(FX["lambda"])


def _capi():
    from openslam_g2o_amd import capi
    return capi


def check(key, got, ref, what="", per_block=0):
    fig = float(H.figure_per_block(got, ref, per_block).max()) if per_block else H.figure(got, ref)
    bound = PM.bound(FX, key)
    print("PCG_FIGURE " + json.dumps(dict(output=key, who="device", what=what, figure=fig, bound=bound)))
    assert fig <= bound, (key, what, fig, bound)


def chain(bs, nb, options=None, zero_b=False):
    name = H.chain_case_name(bs, nb)
    inp = H.chain_inputs(int(FX[name + "_seed"]), nb, bs)
    if zero_b:
        inp["e"], inp["eu"] = 0 * inp["e"], 0 * inp["eu"]
    opts = dict(linear_solver=1)
    opts.update(options or {})
    return name, inp, H.device_chain(_capi(), inp, nb, bs, LAM, opts)


def solve(s, **options):
    for k, v in options.items():
        s.setOption(k, v)
    assert s.solve()
    return s.stats()["iterationsLinearSolver"]


# ================================================================================================ step by step
@pytest.mark.parametrize("bs,nb", CHAINS)
def test_iterates_follow_the_reference_step_by_step(bs, nb):
    name, inp, s = chain(bs, nb, dict(pcg_tolerance=1e-300, pcg_absolute_tolerance=0))
    for k, want in zip(H.STEPS, FX[name + "_it_steps"]):
        it = solve(s, pcg_max_iterations=k)
        check("%s_x%d" % (name, k), s.x(), FX["%s_x%d" % (name, k)], "max_iter %d" % k)
        if want >= 0:
            assert it == k, (name, k, it)
        else:       # the reference reached 1e-20 dn_0 before iteration k: fp64 iterates on rounding residue (or stops at dn == 0)
            assert 1 <= it <= k, (name, k, it)


# ================================================================================================ stopping rule
def _expect(it, want, floor):
    if want >= 0:
        assert it == want, (it, want)
    else:           # a stopping level below the fp64 floor of dn (one-block systems): not defined by the reference
        assert it >= floor, (it, floor)


@pytest.mark.parametrize("bs,nb", CHAINS)
def test_stopping_rule_relative_and_carried_residual(bs, nb):
    name, inp, s = chain(bs, nb, dict(pcg_tolerance=1e-6, pcg_absolute_tolerance=0))
    want = FX[name + "_it_carried"]
    it = solve(s)
    assert it == int(FX[name + "_it_rel"]) == want[0], (name, it)
    # the residual of that solve is the stopping level of the next (pcg_tolerance 1e-20 is far below it), and so on
    it2 = solve(s, pcg_absolute_tolerance=1, pcg_tolerance=1e-20)
    _expect(it2, want[1], it)
    it3 = solve(s)
    _expect(it3, want[2], it2)
    print("PCG_FIGURE " + json.dumps(dict(output=name + "_it_carried", who="device", iterations=[it, it2, it3], reference=want.tolist())))


@pytest.mark.parametrize("bs,nb", CHAINS)
def test_library_default_configuration(bs, nb):
    """No PCG option but linear_solver: tolerance 1e-6, absolute, the residual carried from solve to solve."""
    name, inp, s = chain(bs, nb)
    its = [solve(s) for _ in range(3)]
    assert its == FX[name + "_it_default"].tolist(), (name, its)


@pytest.mark.parametrize("rebuild", [False, True])
@pytest.mark.parametrize("bs,nb", [(3, 257), (6, 255), (7, 257)])
def test_init_forgets_the_carried_residual(bs, nb, rebuild):
    """LinearSolverPCG::init() sets _residual = -1 (linear_solver_pcg.h:64-70).  A loose solve leaves 0.5 dn ~ 1e-3 dn_0 behind; the
    next solve at tolerance 1e-6 (absolute) stops there, and after init() -- with or without a rebuilt structure -- it does not."""
    name, inp, s = chain(bs, nb, dict(pcg_tolerance=1e-2))
    loose = FX[name + "_it_loose"]
    assert solve(s) == loose[0]
    assert solve(s, pcg_tolerance=1e-6) == loose[1] < int(FX[name + "_it_rel"])
    assert solve(s, pcg_tolerance=1e-2) == loose[0]
    s.init()
    if rebuild:
        s.clearEdgeSets()
        H.bind_chain(s, inp, nb, bs)
    s.buildSystem()
    s.setLambda(float(LAM), True)
    assert solve(s, pcg_tolerance=1e-6) == int(FX[name + "_it_rel"])


@pytest.mark.parametrize("bs,nb", CHAINS)
def test_check_every_changes_nothing(bs, nb):
    name, inp, s = chain(bs, nb, dict(pcg_tolerance=1e-6, pcg_absolute_tolerance=0))
    for max_iter, want in ((-1, int(FX[name + "_it_rel"])), (5, min(5, int(FX[name + "_it_rel"])))):
        xs = []
        for every in (1, 3, 16):
            assert solve(s, pcg_check_every=every, pcg_max_iterations=max_iter) == want, (name, every, max_iter)
            xs.append(s.x())
        assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[0], xs[2]), (name, max_iter)


# ================================================================================================ block-diagonal matrices
@pytest.mark.parametrize("bs", sorted(H.CHAIN_BS))
def test_block_diagonal_matrix_is_solved_by_one_iteration(bs):
    """spd_inverse<BS> on 300 blocks with condition numbers 1 .. 1e8, and the empty entry list of BlockPCG::analyze."""
    name = "diag_b%d" % bs
    inp = H.diag_inputs(int(FX[name + "_seed"]), bs)
    s = H.device_diag(_capi(), inp, bs, LAM, dict(linear_solver=1, pcg_tolerance=1e-6, pcg_absolute_tolerance=0))
    assert solve(s) == 1
    check(name + "_x", s.x(), FX[name + "_x"], "per block", per_block=bs)


# ================================================================================================ edges
@pytest.mark.parametrize("bs,nb", [(3, 257), (6, 1), (7, 257)])
def test_zero_right_hand_side_is_done_at_once(bs, nb):
    name, inp, s = chain(bs, nb, dict(pcg_tolerance=1e-6, pcg_absolute_tolerance=0), zero_b=True)
    assert not s.b().any()
    s.setX(np.ones(nb * bs))
    assert solve(s) == 0
    assert not s.x().any()
    assert solve(s, pcg_absolute_tolerance=1) == 0 and not s.x().any()      # (a carried residual of 0 is no stopping level)


@pytest.mark.parametrize("bs", sorted(H.CHAIN_BS))
def test_non_positive_diagonal_block_is_reported(bs):
    name, inp, s = chain(bs, 257, dict(pcg_tolerance=1e-6, pcg_absolute_tolerance=0))
    s.restoreDiagonal()
    s.setLambda(-1e12, True)
    assert not s.solve()
    s.restoreDiagonal()
    s.setLambda(float(LAM), True)
    assert solve(s) == int(FX[name + "_it_rel"])


# ================================================================================================ more than 256 partial sums
def _ring(n, seed):
    rng = np.random.RandomState(seed)
    vi, vj = np.arange(n, dtype=np.int32), ((np.arange(n) + 1) % n).astype(np.int32)
    perm = np.array([rng.permutation(3) for _ in range(n)])
    sign = rng.choice([-1, 1], (n, 3))
    P = np.zeros((n, 3, 3), np.int64)                            # [edge][row][col]: one signed unit entry per row and column
    P[np.arange(n)[:, None], np.arange(3)[None, :], perm] = sign
    e = rng.randint(-3, 4, (n, 3)).astype(np.int64)
    return vi, vj, P, e


def _ring_product(n, vi, vj, P, lam, v):
    """(sum J'J + lam I) v with J0 = I, J1 = P, in int64."""
    v = v.reshape(n, 3)
    w = v[vi] + np.einsum("erc,ec->er", P, v[vj])                # J0 v_i + J1 v_j per edge
    out = lam * v.copy()
    np.add.at(out, vi, w)
    np.add.at(out, vj, np.einsum("erc,er->ec", P, w))
    return out.reshape(-1)


def test_second_trip_of_the_final_reduction_is_exact_on_a_ring():
    """65 600 block rows = 257 partial sums: pcg_reduce_kernel's loop makes a second trip.  Every diagonal block is I + P'P + 2 I =
    4 I, so J_i = I / 4, d = b / 4, q = A d, dn = b'b / 4 and d'q are exact in fp64 in any order, and x_1 = fl(fl(dn / dq) d)."""
    capi = _capi()
    n, lam = 65600, 2
    vi, vj, P, e = _ring(n, 77)
    s = capi.HipBlockSolver(3, 2, 0)
    for k, v in dict(linear_solver=1, pcg_tolerance=1e-300, pcg_absolute_tolerance=0, pcg_max_iterations=1).items():
        s.setOption(k, v)
    kb = s.addEdgeSet(3, vi, vj)
    s.buildStructure(n, 0, False)
    J0 = np.tile(np.eye(3).reshape(-1), (n, 1))
    s.setEdgeData(kb, J0, H.col(P.transpose(0, 2, 1).reshape(n, 9)), H.eye_info(n, 3), H.col(e))
    s.buildSystem()
    s.setLambda(float(lam), True)
    b = np.zeros((n, 3), np.int64)
    np.add.at(b, vi, -e)
    np.add.at(b, vj, -np.einsum("erc,er->ec", P, e))
    b = b.reshape(-1)
    assert np.array_equal(s.b(), b.astype(np.float64))
    v = np.random.RandomState(5).randint(-3, 4, 3 * n).astype(np.int64)
    assert np.array_equal(s.multiplyHessian(v.astype(np.float64)), _ring_product(n, vi, vj, P, lam, v).astype(np.float64))
    assert s.solve() and s.stats()["iterationsLinearSolver"] == 1
    q4 = _ring_product(n, vi, vj, P, lam, b)                     # 4 q
    dn, dq = float(int(b @ b)) / 4.0, float(int(b @ q4)) / 16.0   # (both far below 2^53: exact)
    x1 = (dn / dq) * (b.astype(np.float64) / 4.0)
    assert np.array_equal(s.x(), x1)


# ================================================================================================ reduced operator
def _reduced(p, l, options=None, schur=True):
    name = "red_b%d" % p
    inp = H.reduced_inputs(int(FX[name + "_seed"]), p, l)
    return name, inp, H.device_reduced(_capi(), inp, p, l, LAM, options, schur=schur)


def _device_copy(s, which):
    import torch
    from openslam_g2o_amd.distributed import tensor_from_device_ptr
    ptr, n = s.deviceArray(which)
    s.sync()
    return tensor_from_device_ptr(ptr, n, torch.device("cuda:0")).cpu().numpy().copy()


@pytest.mark.parametrize("p,l", SHAPES)
def test_reduced_operator_blocks_right_hand_side_and_product(p, l):
    import torch
    capi = _capi()
    name, inp, s = _reduced(p, l)
    nP = H.RED_POSES
    s.schurOperatorPrepare()
    check(name + "_Sdiag", _device_copy(s, capi.ARR_SCHUR_DIAG).reshape(nP, p * p), FX[name + "_Sdiag"], "mf_diag_kernel")
    check(name + "_bs", _device_copy(s, capi.ARR_BSCHUR), FX[name + "_bs"], "b_s")
    assert np.array_equal(inp["v"], FX[name + "_v"])
    v = torch.tensor(inp["v"].astype(np.float64), device="cuda:0")
    out = torch.empty_like(v)
    torch.cuda.synchronize()
    s.schurOperatorApply(v.data_ptr(), out.data_ptr())
    s.sync()
    check(name + "_Sv", out.cpu().numpy(), FX[name + "_Sv"], "schur_operator_apply")
    with pytest.raises(capi.G2oHipError):                        # in place is refused (g2ohip.h), the vector stays as it was
        s.schurOperatorApply(v.data_ptr(), v.data_ptr())
    s.sync()
    assert np.array_equal(v.cpu().numpy(), inp["v"].astype(np.float64))


@pytest.mark.parametrize("p,l", SHAPES)
def test_matrix_free_pcg_step_by_step_and_its_iteration_count(p, l):
    name, inp, s = _reduced(p, l, dict(linear_solver=2, pcg_tolerance=1e-300, pcg_absolute_tolerance=0))
    n = H.RED_POSES * p
    for k in (1, 2, 3):
        assert solve(s, pcg_max_iterations=k) == k
        check("%s_x%d" % (name, k), s.x()[:n], FX["%s_x%d" % (name, k)], "linear_solver 2, max_iter %d" % k)
    want = int(FX[name + "_it_rel"])
    assert solve(s, pcg_max_iterations=-1, pcg_tolerance=1e-6) == want
    name, inp, s1 = _reduced(p, l, dict(linear_solver=1, pcg_tolerance=1e-300, pcg_absolute_tolerance=0))
    for k in (1, 2, 3):                                           # (the same iterates on the formed Hschur)
        assert solve(s1, pcg_max_iterations=k) == k
        check("%s_x%d" % (name, k), s1.x()[:n], FX["%s_x%d" % (name, k)], "linear_solver 1, max_iter %d" % k)
    assert solve(s1, pcg_max_iterations=-1, pcg_tolerance=1e-6) == want


@pytest.mark.parametrize("schur", [True, False])
@pytest.mark.parametrize("p,l", SHAPES)
def test_multiply_hessian_with_landmarks_is_exact_on_integers(p, l, schur):
    """dest += H src (the wrapper passes dest = 0) with the damping included: virtual with the Schur complement (added on the
    host), written into the diagonals without it."""
    name, inp, s = _reduced(p, l, schur=schur)
    nP, nL = H.RED_POSES, H.RED_LANDMARKS
    pp, obs, Hll, b = H.reduced_system(inp, p, l)
    assert np.array_equal(s.b(), b.astype(np.float64))
    want = H.full_product(pp, obs, Hll, p, l, nP, nL, LAM, inp["vfull"])
    assert np.array_equal(s.multiplyHessian(inp["vfull"].astype(np.float64)), want.astype(np.float64))
