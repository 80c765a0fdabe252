"""GPU: the unary prior kernels (pg_se2_prior_linearize_kernel<7/8>, pg_se3_prior_linearize_kernel), the depth / disparity
camera kernel (pg_se3_point_linearize_kernel<5/6>) and the stereo kernel (ba_stereo_linearize_kernel, with the chi2 that rides
along) on the branch-covering inputs of tests/golden/sensor_edges.npz, against the 60-digit reference stored there
(tests/golden/make_sensor_edges.py; nothing here evaluates a reference).

Metric of J and err (tests/producer_metric.per_row): per edge AND per output row, max |got - ref| over the row divided by
max(max |ref row|, ops_rows[edge, row]) -- no floor of 1, the rows of a block carry different units.  H, b and chi2 keep the
block metric (producer_metric.per_edge) with their term-magnitude scales.  Bound per output: producer_metric.bound, 8 x the
fp64 restatement's own figure against the same reference, never above 1e-12; EdgeSE2XYPrior is compared bit for bit.  Every
comparison prints a PRODUCER_FIGURE line before it asserts."""
import json
import os

import numpy as np
import pytest

from openslam_g2o_amd import lm
from tests import producer_metric as PM

pytestmark = pytest.mark.gpu

FX = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sensor_edges.npz")))
TAILS = (1, 255, 256, 257, 513)
CONFIGS = ("none", "set1", "set2", "set3", "set4", "set5", "edge")
CHI_N = (257, 513)
PRIOR = {7: ("prior2", 3, 3), 8: ("prior2xy", 2, 3), 9: ("prior3", 6, 6)}     # type -> (fixture group, error dim, pose dim)


def _capi():
    from openslam_g2o_amd import capi
    return capi


def check_rows(key, got, ref, ops, d, what, tag=None):
    fig, k, r = PM.worst_row(got, ref, ops, d)
    b = PM.bound(FX, key)
    rec = dict(output=key, who="device", case=what, worst=fig, edge=k, row=r, branch=None if tag is None else tag(k), bound=b)
    print("PRODUCER_FIGURE", json.dumps(rec))
    assert fig <= b, rec
    return fig


def check_block(key, got, what, ref=None, ops=None):
    ref = FX[key] if ref is None else ref
    ops = FX[key + "_ops"] if ops is None else ops
    fig, k = PM.worst(got, ref, ops)
    b = PM.bound(FX, key)
    rec = dict(output=key, who="device", case=what, worst=fig, edge=k, row=None, branch=None, bound=b)
    print("PRODUCER_FIGURE", json.dumps(rec))
    assert fig <= b, rec
    return fig


def _eye(n, d):
    return np.tile(np.eye(d).reshape(1, d * d), (n, 1))


def _diag_blocks(s, which, n, bs):
    cp, ri = s.pattern(which)
    V = s.values(which).reshape(-1, bs)
    return np.array([V[[q for q in range(cp[c], cp[c + 1]) if ri[q] == c][0]] for c in range(n)])


# ================================================================================================ priors
def _prior_solver(ptype, group, n, staged, info=None, odometry_info=None):
    """setup_device_pose_graph(priors=...): the odometry chain of the fixture as the pose-pose set, the first n priors."""
    pose_group = "prior3" if ptype == 9 else "prior2"
    _, d, p = PRIOR[ptype]
    poses, hidx = FX[group + "_poses"], FX[(group if group == "prior3n" else pose_group) + "_hidx"]
    vi, vj = FX[pose_group + "_vi"], FX[pose_group + "_vj"]
    Zodo = FX[("prior3" if ptype == 9 else group) + "_Zodo"]
    vq = FX[(group if ptype == 9 else "prior2") + "_vq"][:n]
    offset = FX["prior3_offset"] if group == "prior3" else None
    info = _eye(n, d) if info is None else info[:n]
    odo = _eye(len(vi), p) if odometry_info is None else odometry_info
    s, graph = lm.setup_device_pose_graph(2 if ptype == 9 else 1, poses, hidx, int(hidx.max()) + 1, vi, vj, Zodo, odo,
                                          priors=(ptype, vq, FX[group + "_Z"][:n], info, offset))
    s.setOption("pg_landmark_staged", staged)
    return s


def _prior3_tag(group):
    return lambda e: "case%d/qw%s" % (FX[group + "_case"][e], "+" if FX[group + "_sign"][e] > 0 else "-")


def _prior2_tag(e):
    return "exactly M_PI" if FX["prior2_exact"][e] else ("far angle" if FX["prior2_far"][e] else "in range")


def _check_prior(ptype, group, staged, n):
    _, d, p = PRIOR[ptype]
    s = _prior_solver(ptype, group, n, staged)
    s.pgLinearize(True)
    J0, _, err = s.edgeData(s.prior_set, n, d, p, 0)
    what = "type=%d staged=%d n=%d" % (ptype, staged, n)
    rJ, re = FX[group + "_J0"][:n], FX[group + "_err"][:n]
    if ptype == 8:       # J is the constants 1 and 0, err one IEEE subtraction: the reference bit for bit, no bound
        print("PRODUCER_FIGURE", json.dumps(dict(output=group, who="device", case=what, worst=float(np.abs(err - re).max()), edge=0, row=None,
                                                 branch="bitwise", bound=0.0)))
        assert np.array_equal(J0, rJ) and np.array_equal(err, re)
    else:
        tag = _prior3_tag(group) if ptype == 9 else _prior2_tag
        check_rows(group + "_err", err, re, FX[group + "_err_ops"][:n], d, what, tag)
        check_rows(group + "_J0", J0, rJ, FX[group + "_J0_ops"][:n], d, what, tag)
    # pgLinearize(False) at moved estimates leaves J0 bit-identical and changes err; back at the old ones err returns
    before = s.pgGetEstimates()
    s.setX(0.01 * np.random.RandomState(7).normal(size=s.vectorSize()))
    s.pgPush()
    s.pgUpdate()
    assert not np.array_equal(s.pgGetEstimates(), before)
    s.pgLinearize(False)
    xJ0, _, xerr = s.edgeData(s.prior_set, n, d, p, 0)
    assert np.array_equal(xJ0, J0)
    moved = FX[group + "_hidx" if group != "prior2xy" else "prior2_hidx"][FX[(group if ptype == 9 else "prior2") + "_vq"][:n]] >= 0
    assert not np.array_equal(xerr[moved], err[moved]) and np.array_equal(xerr[~moved], err[~moved])
    s.pgPop()
    s.pgLinearize(False)
    xJ0, _, xerr = s.edgeData(s.prior_set, n, d, p, 0)
    assert np.array_equal(xJ0, J0) and np.array_equal(xerr, err)
    # the other store form: bit-identical
    s.setOption("pg_landmark_staged", 1 - staged)
    s.pgLinearize(True)
    xJ0, _, xerr = s.edgeData(s.prior_set, n, d, p, 0)
    assert np.array_equal(xJ0, J0) and np.array_equal(xerr, err)
    return s, J0, err


@pytest.mark.parametrize("ptype", [7, 8, 9])
@pytest.mark.parametrize("staged", [1, 0])
@pytest.mark.parametrize("n", TAILS)
def test_prior_producers_tails_and_store_forms(ptype, staged, n):
    group = PRIOR[ptype][0]
    s, J0, err = _check_prior(ptype, group, staged, n)
    if ptype == 9 and n == TAILS[-1]:      # every (case, sign) group on its own: the printed worst edges name all seven
        case, sign = FX["prior3_case"], FX["prior3_sign"]
        for c in range(4):
            for sg in (1, -1):
                sel = np.nonzero((case == c) & (sign == sg))[0]
                assert len(sel) >= 12 or (c == 0 and sg == -1 and len(sel) == 0)
                if len(sel):
                    what = "case%d/qw%s staged=%d" % (c, "+" if sg > 0 else "-", staged)
                    tag = lambda e: "edge %d%s" % (sel[e], " boundary" if FX["prior3_boundary"][sel[e]] else "")
                    check_rows("prior3_J0", J0[sel], FX["prior3_J0"][sel], FX["prior3_J0_ops"][sel], 6, what, tag)
                    check_rows("prior3_err", err[sel], FX["prior3_err"][sel], FX["prior3_err_ops"][sel], 6, what, tag)


@pytest.mark.parametrize("staged", [1, 0])
def test_se3_prior_without_an_offset(staged):
    n = len(FX["prior3n_vq"])
    _check_prior(9, "prior3n", staged, n)
    k = n - 1                               # the identity error, exactly: err = 0 and the translation block of J is I, bit for bit
    s = _prior_solver(9, "prior3n", n, staged)
    s.pgLinearize(True)
    J0, _, err = s.edgeData(s.prior_set, n, 6, 6, 0)
    assert np.array_equal(err[k], np.zeros(6)) and np.array_equal(J0[k].reshape(6, 6).T[:3, :3], np.eye(3))


def test_se3_prior_assembled_system():
    """The unary path of the generic assembly: Hpp diagonal and b from 513 priors with full SPD 6 x 6 information (the
    odometry set carries zero information and adds nothing)."""
    capi = _capi()
    n = TAILS[-1]
    nv = len(FX["prior3_vi"])
    s = _prior_solver(9, "prior3", n, 1, info=FX["prior3_omega"], odometry_info=np.zeros((nv, 36)))
    s.pgLinearize(True)
    s.buildSystem()
    nP = int(FX["prior3_hidx"].max()) + 1
    check_block("prior3_Hpp", _diag_blocks(s, capi.HPP, nP, 36), "assembled")
    check_block("prior3_b", s.b().reshape(-1, 1), "assembled", FX["prior3_b"].reshape(-1, 1))


# ================================================================================================ depth / disparity
CAMERA_TAG = ("front, inside the image", "front, outside the image", "behind the sensor")


def _camera_solver(group, n, staged, info=None, odometry_info=None):
    capi = _capi()
    hidx, pt_hidx = FX["cam_hidx"], FX["cam_pt_hidx"]
    vi, vj, vp, vl = FX["cam_vi"], FX["cam_vj"], FX["cam_vp"][:n], FX["cam_vl"][:n]
    nP = int(hidx.max()) + 1
    nL = int(pt_hidx.max()) + 1 - nP
    s = capi.HipBlockSolver(6, 3, 0)
    k0 = s.addEdgeSet(6, hidx[vi], hidx[vj])
    k1 = s.addEdgeSet(3, hidx[vp], pt_hidx[vl])
    s.buildStructure(nP, nL, True)
    s.pgSetEdges(k0, 2, vi, vj, FX["cam_Zodo"], _eye(len(vi), 6) if odometry_info is None else odometry_info)
    s.pgSetEstimates(FX["cam_poses"], hidx)
    s.pgSetLandmarkCameraEdges(k1, 5 if group == "depth" else 6, vp, vl, FX[group + "_zl"][:n], _eye(n, 3) if info is None else info[:n],
                               FX["cam_offset"], FX["cam_kcam"])
    s.pgSetLandmarkEstimates(FX["cam_points"], pt_hidx)
    s.setOption("pg_landmark_staged", staged)
    return s, k1, nP, nL


@pytest.mark.parametrize("group", ["depth", "disparity"])
@pytest.mark.parametrize("staged", [1, 0])
@pytest.mark.parametrize("n", TAILS)
def test_camera_producers_tails_and_store_forms(group, staged, n):
    s, k1, _, _ = _camera_solver(group, n, staged)
    s.pgLinearize(True)
    J0, J1, err = s.edgeData(k1, n, 3, 6, 3)
    what = "staged=%d n=%d" % (staged, n)
    tag = lambda e: CAMERA_TAG[FX[group + "_tag"][e]]
    for name, got in (("err", err), ("J0", J0), ("J1", J1)):
        key = group + "_" + name
        check_rows(key, got, FX[key][:n], FX[key + "_ops"][:n], 3, what, tag)
    if n == TAILS[-1]:                      # front, outside and behind each on its own
        for t in range(3):
            sel = np.nonzero(FX[group + "_tag"] == t)[0]
            assert len(sel) >= 20
            for name, got in (("err", err), ("J0", J0), ("J1", J1)):
                key = group + "_" + name
                check_rows(key, got[sel], FX[key][sel], FX[key + "_ops"][sel], 3, "%s staged=%d" % (CAMERA_TAG[t], staged),
                           lambda e: "edge %d" % sel[e])
    s.setOption("pg_landmark_staged", 1 - staged)
    s.pgLinearize(True)
    xJ0, xJ1, xerr = s.edgeData(k1, n, 3, 6, 3)
    assert np.array_equal(xJ0, J0) and np.array_equal(xJ1, J1) and np.array_equal(xerr, err)


def test_disparity_assembled_system():
    """The landmark path of the generic assembly: Hpp diagonal, Hll and b from 513 disparity edges with full SPD 3 x 3
    information (the odometry set carries zero information and adds nothing)."""
    capi = _capi()
    n = TAILS[-1]
    s, k1, nP, nL = _camera_solver("disparity", n, 1, info=FX["cam_omega"], odometry_info=np.zeros((len(FX["cam_vi"]), 36)))
    s.pgLinearize(True)
    s.buildSystem()
    check_block("disparity_Hpp", _diag_blocks(s, capi.HPP, nP, 36), "assembled")
    check_block("disparity_Hll", s.values(capi.HLL).reshape(nL, 9), "assembled")
    check_block("disparity_b", s.b().reshape(-1, 1), "assembled", FX["disparity_b"].reshape(-1, 1))


# ================================================================================================ stereo
def _stereo_solver(si, n, staged, info=None, config="none"):
    """The first n observations of intrinsics set si bound by hand.  Points that lose all their observations leave the
    structure (as tests/stereo_helpers.truncated); at n = 513 the landmark numbering is the fixture's."""
    capi = _capi()
    cam_idx, pt_idx = FX["st_cam_idx"][:n], FX["st_pt_idx"][:n]
    cam_hidx = FX["st_cam_hidx"]
    free = (np.bincount(pt_idx, minlength=len(FX["st_pts"])) > 0) & (FX["st_pt_hidx"] >= 0)
    pt_h = np.where(free, np.cumsum(free) - 1, -1).astype(np.int32)
    nP, nL = int(cam_hidx.max()) + 1, int(free.sum())
    if n == TAILS[-1]:
        assert np.array_equal(pt_h, FX["st_pt_hidx"])
    v0 = np.where(pt_h[pt_idx] >= 0, nP + pt_h[pt_idx], -1).astype(np.int32)
    v1 = cam_hidx[cam_idx].astype(np.int32)
    f, cx, cy, b = (float(v) for v in FX["st_sets"][si])
    s = capi.HipBlockSolver(6, 3, 0)
    s.setOption("ba_stereo_staged", staged)
    k = s.addEdgeSet(3, v0, v1)
    s.buildStructure(nP, nL, True)
    s.baSetStereoEdges(k, cam_idx, pt_idx, FX["st%d_meas" % si][:n], None if info is None else info[:n], f, cx, cy, b)
    s.baSetEstimates(FX["st_cams"], cam_hidx, FX["st_pts"], pt_h)
    if config == "edge":
        s.setRobustKernelPerEdge(k, FX["st_rk_kinds"][:n], FX["st_rk_deltas"][:n])
    elif config != "none":
        kind = int(config[3:])
        s.setRobustKernel(k, kind, float(FX["st_set_deltas"][kind - 1]))
    return s, k, v1, pt_h, nP, nL


def _stereo_tag(e):
    return "far cluster" if FX["st_cam_idx"][e] >= 12 else "near cluster"


@pytest.mark.parametrize("si", [0, 1])
@pytest.mark.parametrize("staged", [1, 0])
@pytest.mark.parametrize("n", TAILS)
def test_stereo_producers_tails_and_store_forms(si, staged, n):
    s, k, _, _, _, _ = _stereo_solver(si, n, staged)
    s.baLinearize(True)
    J0, J1, err = s.edgeData(k, n, 3, 3, 6)
    what = "set=%d staged=%d n=%d" % (si, staged, n)
    for name, got in (("err", err), ("J0", J0), ("J1", J1)):
        key = "st%d_%s" % (si, name)
        check_rows(key, got, FX[key][:n], FX[key + "_ops"][:n], 3, what, _stereo_tag)
    s.setOption("ba_stereo_staged", 1 - staged)
    s.baLinearize(True)
    xJ0, xJ1, xerr = s.edgeData(k, n, 3, 3, 6)
    assert np.array_equal(xJ0, J0) and np.array_equal(xJ1, J1) and np.array_equal(xerr, err)


@pytest.mark.parametrize("si", [0, 1])
@pytest.mark.parametrize("n", CHI_N)
def test_stereo_chi2_rides_along(si, n):
    """s.chi2() straight after baLinearize (the partial sums of ba_stereo_linearize_kernel) against the reference rho-sum: no
    kernel, each kind as the set's kernel, the per-edge table; identity and full information; 257 edges end in a one-lane
    block, 513 in a full one and a one-lane one."""
    key = "st%d_chi2" % si
    for wi, info in enumerate((None, FX["st_omega"])):
        for ci, config in enumerate(CONFIGS):
            s, k, _, _, _, _ = _stereo_solver(si, n, 1, info=info, config=config)
            s.baLinearize(True)
            ni = CHI_N.index(n)
            check_block(key, np.array([[s.chi2()]]), "n=%d %s %s" % (n, "identity" if info is None else "full information", config),
                        np.array([[FX[key][wi, ci, ni]]]), np.array([FX[key + "_ops"][wi, ci, ni]]))


def test_stereo_assembled_system():
    """Hpl per edge, Hll, Hpp diagonal and b of intrinsics set 1 with per-edge robust kernels and full SPD information."""
    capi = _capi()
    n = TAILS[-1]
    s, k, v1, pt_h, nP, nL = _stereo_solver(1, n, 1, info=FX["st_omega"], config="edge")
    s.baLinearize(True)
    s.buildSystem()
    hl = pt_h[FX["st_pt_idx"]]
    edge_of = {(int(v1[e]), int(hl[e])): e for e in range(n) if v1[e] >= 0 and hl[e] >= 0}
    assert len(edge_of) == int(((v1 >= 0) & (hl >= 0)).sum())       # one edge per (camera, point) pair
    cp, ri = s.pattern(capi.HPL)
    V = s.values(capi.HPL).reshape(-1, 18)
    assert len(V) == len(edge_of)
    got = np.zeros((n, 18))
    for c in range(nL):
        for q in range(cp[c], cp[c + 1]):
            got[edge_of[(int(ri[q]), c)]] = V[q]
    check_block("st1_Hpl", got, "assembled")
    check_block("st1_Hll", s.values(capi.HLL).reshape(nL, 9), "assembled")
    check_block("st1_Hpp", _diag_blocks(s, capi.HPP, nP, 36), "assembled")
    check_block("st1_b", s.b().reshape(-1, 1), "assembled", FX["st1_b"].reshape(-1, 1))
    wi, ci, ni = 1, CONFIGS.index("edge"), CHI_N.index(n)
    check_block("st1_chi2", np.array([[s.chi2()]]), "assembled", np.array([[FX["st1_chi2"][wi, ci, ni]]]), np.array([FX["st1_chi2_ops"][wi, ci, ni]]))
