"""GPU: BASELINE.json's configs at their stated sizes (config 3: 50 000 poses / 500 000 points; configs 4-5: 100 000 poses /
1 000 000 landmarks / 5 000 000 observations, plain and with Huber + outliers): against the CPU oracle on the same inputs
(one oracle iteration costs 1.5-2 s at 100 000 poses: b, chi2, Hschur, Dinv and the step are compared directly) and through
size-independent properties:
  * residual of the damped system |H x - b|_inf <= 1e-10 |b|_inf (H applied by the device: multiplyHessian),
  * chi2 of the device-side linearisation against a host evaluation of the same estimates (numpy),
  * exact linearity: the same system with every measurement residual doubled ... is replaced, for the device-resident
    front end, by repeatability: two solves of the same trial are bit-identical (dependency-driven launches, extend-add
    order, no atomics with data-dependent order),
  * an accepted LM step decreases chi2,
  * fill: choleskyNNZ against the reference's cs_amd block ordering (tests/golden/lnz_amd.json, generated from
    oracle/_ref by tests/golden/make_golden.py): nested dissection pays a bounded factor for a shallow tree."""
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import capi, lm, synthetic as S
from oracle import oracle as O
from tests.helpers import GOLD, relerr

pytestmark = pytest.mark.gpu

LNZ = json.load(open(os.path.join(GOLD, "lnz_amd.json")))
# nested dissection with 24-scalar supernodes against AMD's pure band order: every column carries one separator
# (24 rows) on top of the band: 2.19 measured at the metric configuration (2.14-2.18 at the smaller sizes)
FILL_BOUND = 2.25


def _host_chi2(pr, huber=0.0):
    e = S.ba_linearize(pr, jac=False)
    e2 = np.sum(e * e, axis=1)
    if huber > 0:
        big = e2 > huber * huber
        e2 = np.where(big, 2.0 * huber * np.sqrt(np.maximum(e2, 1e-300)) - huber * huber, e2)   # robust_kernel_impl.cpp:65-78
    return float(np.sum(e2))


def _report(meas):
    """Measured errors of a full-size comparison: printed (pytest -s) and appended to gpurun_out/r5_fullsize_errors.jsonl."""
    print("full-size parity, measured:", json.dumps(meas))
    out = os.path.join(os.path.dirname(GOLD), "..", "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "r5_fullsize_errors.jsonl"), "a") as fp:
            fp.write(json.dumps(meas) + "\n")


def _compare_with_the_oracle(pr, s, huber, lam, chi0, x, b):
    """The oracle (oracle/g2o_oracle.c: block_solver.hpp:367-483, base_binary_edge.hpp:54-120, robust_kernel_impl.cpp:65-78,
    csparse_helper.cpp:88-143) on the same estimates, measurements, kernel and damping: b and the assembled reduced system to
    max(1e-12, 16 eps kappa) (64 with the robust kernel), chi2 to 1e-9, the step to 1e-8 (north_star's fp64 bar; measured 3e-10: the summation order of the
    Schur products and the elimination order differ).  kappa: the camera-frame point R X + t cancels world coordinates of
    magnitude |X| ~ P (the trajectory runs along x, one unit per pose) against a depth of >= 3, so ANY evaluation of the
    projection carries a relative rounding error of eps |X| / 3 into the error and the Jacobians -- the device contracts the
    products to FMAs, gcc on x86-64 does not; at the 300-pose sizes of tests/test_gpu_parity.py the same comparison holds 1e-12."""
    kappa = float(np.abs(pr["pts"]).max()) / 3.0
    # (with the robust kernel the weight rho'(e'Oe) carries the same relative error once more, on outliers of hundreds of pixels)
    tol_mat = max(1e-12, (64.0 if huber > 0 else 16.0) * np.finfo(float).eps * kappa)
    Jp, Jc, err = O.ba_edges(pr["cams"], pr["pts"], pr["cam_idx"], pr["pt_idx"], pr["meas"], pr["f"], pr["cx"], pr["cy"])
    o = O.OracleSolver(6, 3, pr["nP"], pr["nL"], True)
    k = o.add_edge_set(2, pr["v0"], pr["v1"])
    o.set_dims(k, 3, 6)
    o.build_structure()
    o.set_edge_data(k, Jp, Jc, S.ba_omega(pr), err, huber)
    del Jp, Jc
    o.build_system()
    assert abs(o.chi2() - chi0) <= 1e-9 * chi0
    meas = {"P": pr["nP"], "huber": huber, "eps_kappa": float(np.finfo(float).eps * kappa), "tol_mat": tol_mat, "chi2": abs(o.chi2() - chi0) / chi0,
            "b": relerr(b, o.b())}
    assert relerr(b, o.b()) < tol_mat, (relerr(b, o.b()), tol_mat)
    assert abs(lam - 1e-5 * o.max_diagonal()) <= tol_mat * lam
    o.set_lambda(lam, True)
    assert o.solve()
    xo = o.x()
    assert relerr(x, xo) < 1e-8, relerr(x, xo)
    sizeP = 6 * pr["nP"]
    assert relerr(x[:sizeP], xo[:sizeP]) < 1e-8 and relerr(x[sizeP:], xo[sizeP:]) < 1e-8
    # the reduced system and the landmark inverses, block by block (a strided sample would do; the whole arrays cost 0.3 s)
    cp, ri = s.pattern(capi.HSCHUR)
    ocp, ori = o.pattern("hs")
    assert np.array_equal(cp, ocp) and np.array_equal(ri, ori)
    meas.update(dx=relerr(x, xo), Hschur=relerr(s.values(capi.HSCHUR), o.values("Hschur")), Dinv=relerr(s.values(capi.DINV), o.values("Dinv")))
    _report(meas)
    assert meas["Hschur"] < tol_mat and meas["Dinv"] < tol_mat, meas
    # ... and the MEASURED errors are what the argument predicts, not merely below a generous bound: 8 eps kappa plain (measured
    # at configs 3 / 4: b 5.1 / 6.4, Dinv 3.9, Hschur 0.24 eps kappa), 48 with the robust kernel (config 5: Hschur 38, b 30, Dinv 14):
    # profiles/r5_fullsize_errors.jsonl
    tight = (48.0 if huber > 0 else 8.0) * np.finfo(float).eps * kappa
    assert max(meas["b"], meas["Hschur"], meas["Dinv"]) <= max(1e-12, tight), meas


@pytest.mark.parametrize("P,L,huber,outliers", [(50000, 500000, 0.0, 0.0), (100000, 1000000, 0.0, 0.0), (100000, 1000000, 1.0, 0.05)])
def test_full_size_properties(P, L, huber, outliers):
    pr = S.make_ba_problem(P, L, outlier_frac=outliers)
    s, g = lm.setup_device_ba(pr, huber_delta=huber)
    g.linearize()
    chi0 = g.chi2()
    assert abs(chi0 - _host_chi2(pr, huber)) <= 1e-9 * chi0
    s.buildSystem()
    lam = 1e-5 * s.maxDiagonal()                     # computeLambdaInit, tau = 1e-5
    s.setLambda(lam, True)
    assert s.solve()
    x, b = s.x(), s.b()
    r = s.multiplyHessian(x) - b
    assert np.abs(r).max() <= 1e-10 * np.abs(b).max()
    assert s.solve() and np.array_equal(s.x(), x)    # bit-repeatable
    _compare_with_the_oracle(pr, s, huber, lam, chi0, x, b)
    st = s.stats()
    assert st["hessianPoseDimension"] == 6 * pr["nP"] and st["hessianLandmarkDimension"] == 3 * pr["nL"]
    ref = LNZ[str(P)]
    assert ref["block_columns"] == pr["nP"]
    assert ref["lnz_block_amd"] <= st["choleskyNNZ"] <= FILL_BOUND * ref["lnz_block_amd"]
    # one LM trial: the update is applied on the device, chi2 decreases, the linear model predicts it
    # (optimization_algorithm_levenberg.cpp:108-124: rho = (chi2_old - chi2_new) / computeScale > 0)
    g.push()
    g.update()
    s.restoreDiagonal()
    g.compute_active_errors()
    chi1 = g.chi2()
    scale = s.computeScale(lam)
    assert chi1 < chi0 and scale > 0 and (chi0 - chi1) / scale > 0.25
    # ... and it is the chi2 a host evaluation of the updated estimates gives
    cams, pts = s.baGetEstimates()
    pr2 = dict(pr)
    pr2["cams"], pr2["pts"] = cams, pts
    assert abs(chi1 - _host_chi2(pr2, huber)) <= 1e-9 * chi1
    g.pop()
    g.compute_active_errors()
    assert g.chi2() == chi0


def test_fill_against_reference_amd_at_test_sizes():
    """The same fill check at the sizes the oracle parity tests run (the fixture holds the reference's lnz for them)."""
    for P, L in ((300, 3000), (2000, 20000), (20000, 200000)):
        pr = S.make_ba_problem(P, L)
        s, g = lm.setup_device_ba(pr)
        g.linearize()
        s.buildSystem()
        s.setLambda(1.0, True)
        assert s.solve()
        ref = LNZ[str(P)]
        assert ref["block_columns"] == pr["nP"]
        nnz = s.stats()["choleskyNNZ"]
        assert ref["lnz_block_amd"] <= nnz <= FILL_BOUND * ref["lnz_block_amd"], (P, nnz, ref)


def test_dense_reduced_system_with_a_front_beyond_the_lds_limit():
    """A hub point seen by 1 200 poses couples them all: the reduced system has a dense 7 200-row frontal matrix -- beyond
    what the triangular sweeps hold in LDS (their vectors go to HBM) and far beyond one Schur tile (the hub is split into
    chunk-pair tiles).  Size-independent properties: residual of the damped system, repeatability, an LM step."""
    pr = S.make_ba_loops(3600, 9000, laps=4, hubs=1)
    s, g = lm.setup_device_ba(pr, huber_delta=1.0)
    g.linearize()
    chi0 = g.chi2()
    s.buildSystem()
    lam = 1e-4 * s.maxDiagonal()
    s.setLambda(lam, True)
    assert s.solve()
    x, b = s.x(), s.b()
    r = s.multiplyHessian(x) - b
    assert np.abs(r).max() <= 1e-10 * np.abs(b).max()
    assert s.stats()["maxFrontDim"] > 6600
    assert s.solve() and np.array_equal(s.x(), x)
    g.push()
    g.update()
    s.restoreDiagonal()
    g.compute_active_errors()
    assert g.chi2() < chi0


def test_grid_graph_with_visibility_by_distance_against_the_oracle_and_at_size():
    """The bundle-adjustment graph that is NOT a camera trajectory (synthetic.make_ba_grid: cameras on a square lattice, every point
    observed by all cameras within a radius -- 4 .. 12 observations per point, every camera coupled to ~40 others; the workload of
    `bench.py --workload grid`).  At 400 cameras against the CPU oracle (b, Hschur, Dinv to 1e-12, the step to the condition-aware
    tolerance); at 10 000 cameras (60 000 x 60 000 reduced system, frontal matrices of 3 500 rows, nnz(L) 60 M) through the
    size-independent properties: residual of the damped system, bit-repeatability, fill against the oracle's block-AMD count at the
    small size, and an accepted Levenberg-Marquardt trial."""
    from tests.helpers import dx_tolerance
    pr = S.make_ba_grid(400)
    K = np.bincount(pr["pt_idx"])
    assert K.min() >= 2 and K.max() > 8 and K.min() < K.max()          # ragged observation lists
    s, g = lm.setup_device_ba(pr)
    g.linearize()
    chi0 = g.chi2()
    assert abs(chi0 - _host_chi2(pr)) <= 1e-9 * chi0
    s.buildSystem()
    lam = 1e-5 * s.maxDiagonal()
    s.setLambda(lam, True)
    assert s.solve()
    x, b = s.x(), s.b()
    Jp, Jc, err = O.ba_edges(pr["cams"], pr["pts"], pr["cam_idx"], pr["pt_idx"], pr["meas"], pr["f"], pr["cx"], pr["cy"])
    o = O.OracleSolver(6, 3, pr["nP"], pr["nL"], True)
    k = o.add_edge_set(2, pr["v0"], pr["v1"])
    o.set_dims(k, 3, 6)
    o.build_structure()
    o.set_edge_data(k, Jp, Jc, S.ba_omega(pr), err)
    o.build_system()
    assert abs(o.chi2() - chi0) <= 1e-9 * chi0
    assert relerr(b, o.b()) < 1e-12
    o.set_lambda(lam, True)
    assert o.solve()
    cp, ri = s.pattern(capi.HSCHUR)
    ocp, ori = o.pattern("hs")
    assert np.array_equal(cp, ocp) and np.array_equal(ri, ori)
    assert relerr(s.values(capi.HSCHUR), o.values("Hschur")) < 1e-12 and relerr(s.values(capi.DINV), o.values("Dinv")) < 1e-12
    assert relerr(x, o.x()) < dx_tolerance(o)[0]
    assert s.stats()["choleskyNNZ"] <= 1.25 * o.lnz()                   # nested dissection against the oracle's block-AMD on a mesh (measured 0.84 at 10 000)
    assert s.stats()["bandChains"] == 0                                 # (nothing here is a band)
    # ---- at size
    pr = S.make_ba_grid(10000)
    s, g = lm.setup_device_ba(pr, huber_delta=1.0)
    g.linearize()
    chi0 = g.chi2()
    s.buildSystem()
    lam = 1e-5 * s.maxDiagonal()
    s.setLambda(lam, True)
    assert s.solve()
    x, b = s.x(), s.b()
    r = s.multiplyHessian(x) - b
    assert np.abs(r).max() <= 1e-10 * np.abs(b).max()
    st = s.stats()
    assert st["maxFrontDim"] > 2000 and st["hessianPoseDimension"] == 6 * pr["nP"]
    assert s.solve() and np.array_equal(s.x(), x)
    g.push()
    g.update()
    s.restoreDiagonal()
    g.compute_active_errors()
    assert g.chi2() < chi0


def test_grid_graph_whole_gpu_passes_against_one_workgroup_per_front():
    """2 500 cameras on the lattice (frontal matrices of 1 700 rows, levels of more than 256 tiles, grouped in-place chains): the
    scratch-slab path as it runs by default -- pivot block + panel rows in one launch with the rows on the matrix cores
    (big_panel_solve_kernel), the extend-add of a level as ONE launch that writes its fronts' regions (big_extend_gather_kernel), the
    grouped rank-480 updates reading solved rows from the L panels -- against the independent form of the same factorisation, one
    workgroup per front with everything in one kernel (big_front_passes = 0): the same step to rounding, both with a clean residual."""
    pr = S.make_ba_grid(2500)
    xs = {}
    for name, opts in (("whole-GPU passes", {}), ("one workgroup per front", {"big_front_passes": 0})):
        s, g = lm.setup_device_ba(pr, huber_delta=1.0, options=opts)
        g.linearize()
        s.buildSystem()
        s.setLambda(1e-5 * s.maxDiagonal(), True)
        assert s.solve(), name
        x, b = s.x(), s.b()
        r = s.multiplyHessian(x) - b
        assert np.abs(r).max() <= 1e-10 * np.abs(b).max(), name
        assert s.stats()["maxFrontDim"] >= 1024
        xs[name] = x
    assert relerr(xs["whole-GPU passes"], xs["one workgroup per front"]) < 1e-9


def test_bench_line_contract_on_both_workloads(tmp_path):
    """bench.py --full prints ONE JSON line with the contract's keys; `roofline` carries frac_traffic / traffic_commit / the matrix-core block
    on the chain workload at the metric configuration only (the PMC file is for that size) and switches to the MFMA bound with the
    factorisation's flop count where the factorisation dominates (--workload grid); `cpu_baseline` (the oracle, one repetition on the
    grid) sits beside it with dx / chi2 against it."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for args, bound in ((["--workload", "grid", "--poses", "900"], "mfma"), (["--poses", "3000", "--landmarks", "30000"], "hbm")):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "3", "--warmup", "2"] + args, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stderr[-1500:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                  "roofline", "cpu_baseline"):
            assert k in d, k
        assert d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["dtype"] == "f64" and d["higher_is_better"] is False
        assert d["roofline"]["bound"] == bound and 0 < d["roofline"]["frac"] < 1
        assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["value"] > 0
        assert d["dx_rel_err"] < 1e-8 and d["chi2_rel_err"] < 1e-9 and d["residual_rel"] < 1e-11
        if bound == "mfma":
            assert d["roofline"]["unit"] == "TFLOP/s" and d["solver_stats"]["choleskyFlops"] > 0 and "visibility by distance" in d["config"]["workload"]


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    """A plain bench.py run (no --full) prints the headline keys only -- no second pass, no residual check, no CPU oracle -- and
    --dump-outputs writes the increment x of its last timed step (float64).  The --full run on the same arguments dumps the same x,
    and there x solves the damped system (residual_rel) and equals the CPU oracle's (dx_rel_err)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {}
    for mode, extra in (("plain", []), ("full", ["--full"])):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "2", "--poses", "3000", "--landmarks", "30000",
                            "--dump-outputs", str(tmp_path / mode)] + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-1500:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        runs[mode] = (json.loads(lines[0]), np.load(tmp_path / mode / "x.npy"))
    d, x = runs["plain"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "solve_ok"):
        assert k in d, k
    for k in ("roofline", "kernels", "solver_stats", "residual_rel", "cpu_baseline", "dx_rel_err"):
        assert k not in d, k
    assert d["steps"] == 3 and d["warmup"] == 2 and d["solve_ok"] and d["value"] == d["ms_per_step"] > 0 and d["dtype"] == "f64"
    assert x.dtype == np.float64 and x.ndim == 1 and x.size >= 3 * 30000 and np.isfinite(x).all()
    full, xf = runs["full"]
    assert full["dx_rel_err"] < 1e-8 and full["residual_rel"] < 1e-11
    assert xf.shape == x.shape and relerr(x, xf) < 1e-12
