"""g2ohip_ba_structure_only on the device against the fp64 restatement and the 60-digit goldens
(tests/golden/structure_only.npz): parity of traces / points / chi2 on every binding, num_max_trials = 1, num_iters = 0, the
state of the handle afterwards, and the ba_demo sequence end to end.  No point is left out of any trace comparison.

G2OHIP_SO_RECORD=1 appends the device's own figures to profiles/structure_only.jsonl."""
import os

import numpy as np
import pytest

import structure_only_helpers as H
from openslam_g2o_amd import capi, lm, structure_only as SO, synthetic

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.fixture(scope="module")
def golden():
    return H.load_golden()


@pytest.mark.parametrize("name", list(H.SPECS))
def test_parity_with_restatement_and_golden(golden, name):
    """Traces, points and chi2 of the margin-qualified run (H.TRACE_ITERS outer iterations) on every point; points and chi2 of the
    ten-iteration run: both within 8 x the fp64-vs-60-digit drift recorded for that run."""
    g, ref = golden[name]
    s, _ = H.setup_device(g, name)
    tr, chi = s.baStructureOnly(H.TRACE_ITERS, 10, trace=True)
    pts = s.baGetEstimates()[1]
    _, t64, _ = H.run(H.FP64, g, name)
    d_pts, d_chi = float(np.abs(pts - ref["pts"]).max()), float(np.abs(chi - ref["chi2"]).max())
    s10, _ = H.setup_device(g, name)
    tr10, chi10 = s10.baStructureOnly(10, 10, trace=True)
    pts10 = s10.baGetEstimates()[1]
    d_pts10, d_chi10 = float(np.abs(pts10 - ref["pts10"]).max()), float(np.abs(chi10 - ref["chi210"]).max())
    print(name, "device vs 60 digits: points", d_pts, "chi2", d_chi, "recorded drift", ref["drift"].tolist(), "mismatching traces",
          int((tr != t64).any(axis=1).sum()), "; ten iterations: points", d_pts10, "chi2", d_chi10, "recorded drift", ref["drift10"].tolist())
    if os.environ.get("G2OHIP_SO_RECORD"):
        H.append_profile(dict(what="device vs 60-digit run", graph=name, outer_iterations=H.TRACE_ITERS, difference_points=d_pts,
                              difference_chi2=d_chi, trace_mismatches=int((tr != ref["trace"]).any(axis=1).sum()),
                              difference_points_10_iterations=d_pts10, difference_chi2_10_iterations=d_chi10,
                              stop_reasons_10_iterations=np.bincount(tr10[:, 3], minlength=4).tolist()))
    assert np.array_equal(tr, t64) and np.array_equal(tr, ref["trace"])      # every point
    _, t64_10, _ = H.run(H.FP64, g, name, 10, 10)
    print(name, "ten iterations: traces that differ from the fp64 restatement's", np.flatnonzero((tr10 != t64_10).any(axis=1)).tolist(),
          "from the 60-digit run's", np.flatnonzero((tr10 != ref["trace10"]).any(axis=1)).tolist())
    assert np.array_equal(tr10, t64_10) and np.array_equal(tr10, ref["trace10"])      # every point, all ten iterations
    assert d_pts <= 8 * ref["drift"][0] and d_chi <= 8 * ref["drift"][1]
    assert d_pts10 <= 8 * ref["drift10"][0] and d_chi10 <= 8 * ref["drift10"][1]
    skipped = tr[:, 3] == SO.REASON_SKIPPED
    _, i_empty, i_fixedcam, _ = H.special(g)
    assert skipped[i_empty] and np.array_equal(pts[skipped], g["pts"][skipped])   # the empty track (and a fixed point) stay
    assert not skipped[i_fixedcam] and not skipped[0]                            # fixed cameras only; the long track


@pytest.mark.parametrize("name", ["mono_general", "stereo_general"])
def test_one_trial_rejections_leave_the_point(golden, name):
    g, ref = golden[name]
    s, _ = H.setup_device(g, name)
    tr, _ = s.baStructureOnly(H.TRACE_ITERS, 1, trace=True)
    pts = s.baGetEstimates()[1]
    assert np.array_equal(tr, ref["trace1"])
    first = (tr[:, 3] == SO.REASON_TRIALS) & (tr[:, 0] == 1)
    assert first.any()                                          # a point whose first trial is rejected ...
    assert np.array_equal(pts[first], g["pts"][first])          # ... is unchanged bit for bit
    assert tuple(tr[H.special(g)[3]]) == (1, 0, 0, SO.REASON_GRADIENT)      # a converged start stops at iteration 0


@pytest.mark.parametrize("name", ["mono_general", "stereo_general"])
def test_zero_iterations_is_chi2_only(golden, name):
    g, _ = golden[name]
    s, k = H.setup_device(g, name)
    s.setRobustKernel(k, capi.KERNEL_NONE, 0.0)
    tr, chi = s.baStructureOnly(0, 10, trace=True)
    assert np.array_equal(s.baGetEstimates()[1], g["pts"])
    assert (tr[:, :3] == 0).all()
    free = g["pt_hidx"] >= 0
    fixed_edges = dict(g)
    keep = ~free[g["pt_idx"]]
    for key in ("cam_idx", "pt_idx", "meas", "info", "edge_class"):
        if key in g:
            fixed_edges[key] = g[key][keep]
    total = chi[free, 0].sum() + SO.total_chi2(fixed_edges)
    s.baLinearize(False)
    ref_total = s.chi2()
    assert abs(total - ref_total) <= 1e-12 * ref_total


@pytest.mark.parametrize("name,fused", [("mono_fused", 1), ("mono_fused", 0), ("mono_general", 1), ("stereo_general", 1)])
def test_state_after_the_call(golden, name, fused):
    g, _ = golden[name]

    def solve(s):
        s.baLinearize(True)
        s.buildSystem()
        s.setLambda(5.0, True)
        assert s.solve()
        x = s.x()
        s.restoreDiagonal()
        return x

    s, _ = H.setup_device(g, name, fused=bool(fused))
    solve(s)                                   # a system built from the OLD estimates must not survive the call
    s.baStructureOnly(10, 10)
    x = solve(s)
    cams, pts = s.baGetEstimates()
    g2 = dict(g, pts=pts)
    s2, _ = H.setup_device(g2, name, fused=bool(fused))
    assert relerr(x, solve(s2)) < 1e-8         # (the x bound of tests/test_gpu_lm.py)
    # push / call / pop on a handle at the displaced start: the points move, and pop brings the pushed ones back bit for bit
    s3, _ = H.setup_device(g, name, fused=bool(fused))
    s3.baPush()
    s3.baStructureOnly(3, 10)
    assert not np.array_equal(s3.baGetEstimates()[1], g["pts"])
    s3.baPop()
    assert np.array_equal(s3.baGetEstimates()[1], g["pts"]) and np.array_equal(s3.baGetEstimates()[0], g["cams"])


def test_error_codes(golden):
    g, _ = golden["mono_fused"]
    s = capi.HipBlockSolver(6, 3, 0)
    with pytest.raises(capi.G2oHipError, match=r"failed \(-3\)"):          # G2OHIP_ERR_STATE: nothing bound
        s.baStructureOnly()
    s, _ = H.setup_device(g, "mono_fused")
    for bad in ((-1, 10), (10, 0)):
        with pytest.raises(capi.G2oHipError, match=r"failed \(-1\)"):      # G2OHIP_ERR_ARG
            s.baStructureOnly(*bad)
    sp, _ = lm.setup_device_ba(synthetic.make_ba_inverse_depth(8, 40))
    with pytest.raises(capi.G2oHipError, match=r"failed \(-3\).*PSI2UV"):  # G2OHIP_ERR_STATE: an inverse-depth binding
        sp.baStructureOnly()


def test_end_to_end_as_ba_demo(golden):
    g, _ = golden["mono_fused"]               # cameras exact (the observations were generated from them), points displaced

    def chi2_of(s):
        s.baLinearize(False)
        return s.chi2()

    s, _ = H.setup_device(g, "mono_fused")
    graph = lm.DeviceBAGraph(s)
    chi_before = chi2_of(s)
    tr, _ = lm.structure_only(s, 10, trace=True)
    chi_after = chi2_of(s)
    pts = s.baGetEstimates()[1]
    moved = tr[:, 3] != SO.REASON_SKIPPED
    rms = lambda p: float(np.sqrt(((p[moved] - g["pts_true"][moved]) ** 2).sum(axis=1).mean()))   # noqa: E731
    print("chi2", chi_before, "->", chi_after, "rms", rms(g["pts"]), "->", rms(pts))
    assert chi_after < chi_before and rms(pts) < rms(g["pts"])
    _, chis_with, _, _ = lm.optimize(graph, s, 3)
    s0, _ = H.setup_device(g, "mono_fused")
    _, chis_without, _, _ = lm.optimize(lm.DeviceBAGraph(s0), s0, 3)
    print("after 3 LM iterations: with the pre-step", chis_with[-1], "without", chis_without[-1])
    assert chis_with[-1] <= chis_without[-1]
