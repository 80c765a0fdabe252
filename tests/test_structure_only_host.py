"""Host side of the structure-only bundle adjustment: the fp64 restatement (openslam_g2o_amd/structure_only.py) against the
60-digit run recorded in tests/golden/structure_only.npz, the decision margins of that run, one hand-checked point, the wrappers.
The traced runs take structure_only_helpers.TRACE_ITERS outer iterations (that file says why); the ten-iteration run of every
graph is held through its points and chi2."""
import numpy as np
import pytest

import structure_only_helpers as H
from openslam_g2o_amd import capi, lm, structure_only as SO


@pytest.fixture(scope="module")
def golden():
    return H.load_golden()


@pytest.mark.parametrize("name", list(H.SPECS))
def test_fp64_restatement_against_60_digits(golden, name):
    g, ref = golden[name]
    pts, tr, chi = H.run(H.FP64, g, name)
    assert np.array_equal(tr, ref["trace"])                         # every point
    # (the 60-digit values are stored rounded to fp64: one spacing of the largest of them on top of the recorded drift)
    assert np.abs(SO.to_f64(pts) - ref["pts"]).max() <= ref["drift"][0] + np.spacing(np.abs(ref["pts"]).max())
    assert np.abs(SO.to_f64(chi) - ref["chi2"]).max() <= ref["drift"][1] + np.spacing(np.abs(ref["chi2"]).max())
    _, tr1, _ = H.run(H.FP64, g, name, H.TRACE_ITERS, 1)
    assert np.array_equal(tr1, ref["trace1"])
    _, i_empty, i_fixedcam, i_conv = H.special(g)
    assert tuple(tr[i_empty]) == (0, 0, 0, SO.REASON_SKIPPED) and tuple(tr[i_conv]) == (1, 0, 0, SO.REASON_GRADIENT)
    assert tr[0, 3] != SO.REASON_SKIPPED and tr[i_fixedcam, 3] != SO.REASON_SKIPPED
    if H.SPECS[name]["specials"]:      # a point whose first trial is rejected: with one trial allowed it stops there
        assert ((tr1[:, 0] == 1) & (tr1[:, 2] == 1) & (tr1[:, 3] == SO.REASON_TRIALS)).any()
    p10, t10, c10 = H.run(H.FP64, g, name, 10, 10)
    assert np.array_equal(t10, ref["trace10"])                      # every point, all ten iterations
    assert H.each_ok(ref["each10"])                                 # ... every decision 1000 x its own difference from its threshold
    assert np.abs(SO.to_f64(p10) - ref["pts10"]).max() <= ref["drift10"][0] + np.spacing(np.abs(ref["pts10"]).max())
    assert np.abs(SO.to_f64(c10) - ref["chi210"]).max() <= ref["drift10"][1] + np.spacing(np.abs(ref["chi210"]).max())


@pytest.mark.parametrize("name", list(H.SPECS))
def test_decision_margins(golden, name):
    """Every decision of the 60-digit run is at least 1000 x the largest fp64-vs-60-digit difference of that quantity on the
    graph away from its threshold (asserted again from the recorded decisions)."""
    g, ref = golden[name]
    dec = ref["decisions"]
    kinds = list(H.THRESHOLD)
    for i, k in enumerate(kinds):
        vals = dec[dec[:, 1] == i, 2]
        margin = np.abs(vals - H.THRESHOLD[k]).min() if len(vals) else np.inf
        print(name, k, "margin", margin, "largest difference", ref["diff"][i])
        assert margin >= H.MARGIN_FACTOR * ref["diff"][i], (name, k, margin, ref["diff"][i])


def test_60_digit_run_reproduces_the_golden(golden):
    g, ref = golden["stereo_identity"]
    few = dict(g)
    keep = g["pt_idx"] < 12
    for key in ("cam_idx", "pt_idx", "meas"):
        few[key] = g[key][keep]
    few["pts"], few["pt_hidx"] = g["pts"][:12], g["pt_hidx"][:12]
    pts, tr, chi = H.run(H.MP, few, "stereo_identity")
    assert np.array_equal(tr, ref["trace"][:12])
    assert np.array_equal(SO.to_f64(pts), ref["pts"][:12]) and np.array_equal(SO.to_f64(chi), ref["chi2"][:12])


def test_one_iteration_is_a_damped_normal_equation():
    """One point of ba_demo-like geometry: cameras at x = 0, 0.5, 1 looking down z, f = 1000, the point near (0.4, 0.1, 3.5).
    One iteration equals the dense solve of (H + 0.01 I) delta = b with H, b from the closed-form Jacobian of the pinhole."""
    cams = np.zeros((3, 12))
    cams[:, [0, 4, 8]] = 1.0
    cams[:, 9] = [0.0, -0.5, -1.0]
    true, X = np.array([0.4, 0.1, 3.5]), np.array([0.45, 0.05, 3.7])
    meas = np.array([[(true[0] + c[9]) / true[2] * 1000 + 320, true[1] / true[2] * 1000 + 240] for c in cams])
    prob = dict(cams=cams, pts=X[None], meas=meas, cam_idx=np.arange(3), pt_idx=np.zeros(3, int), f=1000.0, cx=320.0, cy=240.0)
    pts, tr, chi = SO.structure_only(prob, 1, 10)
    Hm, b, c0 = np.zeros((3, 3)), np.zeros(3), 0.0
    for c, z in zip(cams, meas):
        x, y, zc = X + c[9:12]
        e = z - np.array([x / zc * 1000 + 320, y / zc * 1000 + 240])
        J = -np.array([[1000 / zc, 0, -1000 * x / zc ** 2], [0, 1000 / zc, -1000 * y / zc ** 2]])
        Hm += J.T @ J
        b -= J.T @ e
        c0 += e @ e
    delta = np.linalg.solve(Hm + 0.01 * np.eye(3), b)
    assert tr[0] == (1, 1, 0, SO.REASON_ITERS)
    assert np.allclose(SO.to_f64(pts)[0], X + delta, rtol=0, atol=1e-11)
    assert abs(float(chi[0][0]) - c0) <= 1e-12 * c0 and float(chi[0][1]) < c0
    assert np.abs(SO.to_f64(pts)[0] - true).max() < np.abs(X - true).max()


def test_several_iterations_against_an_independent_loop():
    """One point with an outlier under a Huber kernel, started where the weighted step raises the raw chi2: several outer
    iterations with rejected trials, against a loop written apart from the restatement (NumPy matrices, numpy.linalg.solve,
    eigenvalues for positivity): the same trace, the same damping history and the same point."""
    cams = np.zeros((4, 12))
    cams[:, [0, 4, 8]] = 1.0
    cams[:, 9] = [0.0, -0.5, -1.0, -1.5]
    true = np.array([0.7, -0.2, 3.2])
    meas = np.array([[(true[0] + c[9]) / true[2] * 1000 + 320, true[1] / true[2] * 1000 + 240] for c in cams])
    meas[0, 0] += 60.0
    base = dict(cams=cams, pts=true[None], meas=meas, cam_idx=np.arange(4), pt_idx=np.zeros(4, int), f=1000.0, cx=320.0, cy=240.0)
    ls = SO.to_f64(SO.structure_only(base, 10, 10)[0])[0]                     # the optimum of the raw least squares
    X0 = true + np.array([0.03, 0.0, -0.08])
    prob = dict(cams=cams, pts=X0[None], meas=meas, cam_idx=np.arange(4), pt_idx=np.zeros(4, int), f=1000.0, cx=320.0, cy=240.0)
    delta_h = 2.0

    def terms(X):
        chi, Hm, b = 0.0, np.zeros((3, 3)), np.zeros(3)
        for c, z in zip(cams, meas):
            x, y, zc = X + c[9:12]
            e = z - np.array([x / zc * 1000 + 320, y / zc * 1000 + 240])
            J = -np.array([[1000 / zc, 0, -1000 * x / zc ** 2], [0, 1000 / zc, -1000 * y / zc ** 2]])
            e2 = e @ e
            w = 1.0 if e2 <= delta_h ** 2 else delta_h / np.sqrt(e2)
            chi, Hm, b = chi + e2, Hm + w * J.T @ J, b - w * J.T @ e
        return chi, Hm, b

    # (start, num_iters, num_max_trials): from beside the truth, several accepted steps; half way to the raw optimum the weighted
    # step raises the raw chi2 and the trials run out
    seen = []
    for start, iters, trials in ((X0, 4, 10), (X0, 2, 1), (0.5 * (true + ls), 3, 4), (0.5 * (true + ls), 3, 1), (ls, 3, 4)):
        prob["pts"] = start[None]
        X, mu, nu, log = start.copy(), 0.01, 2.0, [0, 0, 0, 0]
        chi = terms(X)[0]
        for _ in range(iters):
            log[0] += 1
            _, Hm, b = terms(X)
            if np.linalg.norm(b) < 0.001:
                log[3] = 1
                break
            trial, stop = 0, False
            while True:
                A = Hm + mu * np.eye(3)
                good = False
                if np.linalg.eigvalsh(A).min() > 0:
                    Xn = X + np.linalg.solve(A, b)
                    new = terms(Xn)[0]
                    if chi - new > 0 and np.isfinite(new):
                        good, chi, X = True, new, Xn
                if good:
                    mu, nu = mu / 3.0, 2.0
                    log[1] += 1
                    break
                mu, nu, trial = mu * nu, nu * 2.0, trial + 1
                log[2] += 1
                if trial >= trials:
                    stop = True
                    break
            if stop:
                log[3] = 2
                break
        pts, tr, c = SO.structure_only(prob, iters, trials, (1, delta_h))
        assert tuple(tr[0]) == tuple(log), (iters, trials, tr[0], log)
        assert np.allclose(SO.to_f64(pts)[0], X, rtol=0, atol=1e-9) and abs(float(c[0][1]) - chi) <= 1e-9 * chi
        if start is X0 and iters == 4:
            assert log[1] > 1                     # more than one accepted step: mu was carried over
        seen.append(tuple(log))


    assert len(set(seen)) > 1


def test_entry_is_declared_everywhere():
    assert "g2ohip_ba_structure_only" in capi.EXPORTS
    assert callable(capi.HipBlockSolver.baStructureOnly) and callable(lm.structure_only)
    with pytest.raises(ValueError):
        SO.structure_only(dict(pts=np.zeros((0, 3)), cams=np.zeros((0, 12)), meas=np.zeros((0, 2)), cam_idx=[], pt_idx=[], f=1, cx=0, cy=0), -1)
