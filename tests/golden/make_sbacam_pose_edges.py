"""Generator of tests/golden/sbacam_pose_edges.npz and of the oracle-drift lines of profiles/sba_cam_edges.jsonl (CPU only; run
from the repository root: python tests/golden/make_sbacam_pose_edges.py).  Needs the built CPU oracle (make -C oracle).

Per test graph of the device EdgeSBACam / EdgeSBAScale sets: the inputs, the producers of openslam_g2o_amd/sbacam.py evaluated
with mpmath at 60 digits (rounded to fp64; for EdgeSBACam the inverse measurements too) and the drift of the SAME formulas
evaluated in fp64 against them -- max abs over err, over J0 | J1, over the inverse measurements.  The drift of J is ~1e-7 on
entries of order 1: the reference defines these Jacobians as central differences with delta = 1e-9, and 1 / (2 delta) = 5e8
multiplies every rounding of the error.  The GPU tests bound the device against the mpmath figures by 8 x the drift recorded here
for the same graph and output -- the oracle's own figure, never the device's.

  branch       sbacam_pose_helpers.branch_graph: normalizeRotation's flip in the first product, in the second, at binding, and no
               flip; fixed vertex on side 0 / side 1 / none; a pair twice and in both orders; e = 0; translations of 1e3
  c1 ... c300  random EdgeSBACam graphs; 12 lanes per edge and 256 threads per block: 21 edges fill a block of the Jacobian
               kernel, the 22nd straddles it; 257 is one past a block of the error kernel; 300 leaves partial last blocks
  s1 ... s300  the same sizes for EdgeSBAScale;  coincident: one scale edge between two cameras at one position
  lm           synthetic.make_sbacam_ba(12 cameras, 60 points, cam_edges=4, scale_edges=2): ten LM iterations of lm.optimize
               (from user_lambda_init = sbacam_pose_helpers.LM_LAMBDA, see there) over the CPU oracle solver, fed by the fp64 and by the mpmath producers -- "ba" (with the projection set), "pose" (the
               same cameras and constraints without points), "huber" (with the projection set, Huber on the EdgeSBACam set):
               chi2 per iteration, their relative difference, the trials, the gap of the final estimates
  default_hash sha256 over the arrays of make_sbacam_ba with default arguments (mono and stereo): the generator's output without
               cam_edges / scale_edges is the one of the commit before these arguments existed"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import lm, synthetic  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import sbacam_helpers as HB  # noqa: E402
from tests import sbacam_pose_helpers as H  # noqa: E402


def default_hash():
    h = hashlib.sha256()
    for stereo in (False, True):
        g = synthetic.make_sbacam_ba(stereo=stereo, **HB.BA_ARGS)
        for k in sorted(g):
            h.update(k.encode())
            h.update(np.ascontiguousarray(np.asarray(g[k])).tobytes())
    return h.hexdigest()


class OracleSolver:
    def __init__(self, g, huber):
        self.g = g
        with_points = len(g["vp"]) > 0
        self.o = O.OracleSolver(6, 3, g["nP"], g["nL"] if with_points else 0, with_points)
        self.k, self.info, self.huber = {}, {}, {}
        if with_points:
            self.k["obs"] = self.o.add_edge_set(g["zl"].shape[1], g["hidx"][g["vp"]], g["pt_hidx"][g["vl"]])
            self.o.set_dims(self.k["obs"], 6, 3)
            self.info["obs"], self.huber["obs"] = g["omega_l"], 0.0
        for name, key, d in (("cam", "cam_edges", 6), ("scale", "scale_edges", 1)):
            e = g[key]
            self.k[name] = self.o.add_edge_set(d, g["hidx"][e["vi"]], g["hidx"][e["vj"]])
            self.o.set_dims(self.k[name], 6, 6)
            self.info[name], self.huber[name] = e["info"], huber if name == "cam" else 0.0
        self.o.build_structure()

    def feed(self, name, J0, J1, err):
        self.o.set_edge_data(self.k[name], J0, J1, self.info[name], err, self.huber[name])

    buildSystem = lambda self: self.o.build_system()
    setLambda = lambda self, lam, backup=False: self.o.set_lambda(lam, backup)
    restoreDiagonal = lambda self: self.o.restore_diagonal()
    solve = lambda self: self.o.solve()
    maxDiagonal = lambda self: self.o.max_diagonal()
    computeScale = lambda self, lam: self.o.compute_scale(lam)
    x = lambda self: self.o.x()


def oracle_run(F, g, huber):
    s = OracleSolver(g, huber)
    graph = H.HostSbacamPoseGraph(F, g, s.feed, s.x, s.o.chi2)
    graph.linearize()
    chi0 = graph.chi2()
    done, chis, lams, trials = lm.optimize(graph, s, H.ITERATIONS, "lm", user_lambda_init=H.LM_LAMBDA)
    return dict(chi0=chi0, chis=np.array(chis), trials=list(trials), est=graph.est.copy(), points=graph.points.copy(), done=done)


def main():
    out, lines = {"default_hash": np.array(default_hash())}, []
    for scale, graphs in ((False, H.cam_graphs()), (True, H.scale_graphs())):
        for name, g in graphs.items():
            t64, tmp = [], []
            J0, J1, e = H.producers(H.FP64, g, scale, trace=t64)
            M0, M1, me = H.producers(H.MP, g, scale, trace=tmp)
            assert t64 == tmp, "fp64 and mpmath took different branches"
            fig = dict(err=float(np.abs(e - me).max()), J=float(max(np.abs(J0 - M0).max(), np.abs(J1 - M1).max())))
            for k in H.CAM_KEYS:
                out["%s_%s" % (name, k)] = g[k]
            out.update({name + "_J0": M0, name + "_J1": M1, name + "_err": me})
            # per output and side: the fp64 restatement's own distance from the 60-digit values
            drift = [fig["err"], float(np.abs(J0 - M0).max()), float(np.abs(J1 - M1).max())]
            if not scale:
                zi64, zimp = H.inverse_measurements(H.FP64, g["meas"]), H.inverse_measurements(H.MP, g["meas"])
                out[name + "_zinv"] = zimp
                fig["zinv"] = float(np.abs(zi64 - zimp).max())
                drift.append(fig["zinv"])
            out[name + "_drift"] = np.array(drift)
            if name == "branch":
                out["branch_trace"] = np.array(edge_trace(g), np.int8)
            lines.append(dict(kind="oracle_drift", type="EdgeSBAScale" if scale else "EdgeSBACam", graph=name, edges=int(len(g["vi"])), **fig))
            print(lines[-1], flush=True)
    tr = edge_trace(H.branch_graph())
    for k, want in H.BRANCH_TRACE.items():
        assert tuple(bool(v) for v in tr[k]) == want, (k, tr[k], want)
    assert any(not any(t) for t in tr)

    for tag, points, huber in (("ba", True, 0.0), ("pose", False, 0.0), ("huber", True, H.HUBER)):
        g = H.lm_problem(points)
        a, b = oracle_run(H.FP64, g, huber), oracle_run(H.MP, g, huber)
        assert a["trials"] == b["trials"], (a["trials"], b["trials"])
        assert a["done"] == b["done"] == H.ITERATIONS
        rel = np.abs(a["chis"] - b["chis"]) / np.abs(b["chis"])
        dest = H.transform_gap(a["est"], b["est"])
        dpts = float(np.abs(a["points"] - b["points"]).max()) if points else 0.0
        out.update({"lm_%s_chis" % tag: b["chis"], "lm_%s_rel" % tag: rel, "lm_%s_trials" % tag: np.array(b["trials"]),
                    "lm_%s_chi0" % tag: np.array([b["chi0"]]), "lm_%s_est_drift" % tag: np.array([dest]),
                    "lm_%s_points_drift" % tag: np.array([dpts])})
        lines.append(dict(kind="oracle_drift", graph="lm " + tag, args=H.LM_ARGS, points=points, cam_huber=huber, chi2_initial=b["chi0"],
                          chi2_mp=[float(v) for v in b["chis"]], chi2_rel_fp64_vs_mp=[float(v) for v in rel],
                          trials=[int(t) for t in b["trials"]], final_cameras_max_abs=dest, final_points_max_abs=dpts))
        print(lines[-1], flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sbacam_pose_edges.npz"), **out)
    path = os.path.join(ROOT, "profiles", "sba_cam_edges.jsonl")
    keep = []
    if os.path.exists(path):
        keep = [l for l in open(path).read().splitlines() if l.strip() and json.loads(l).get("kind") != "oracle_drift"]
    with open(path, "w") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")
        for l in keep:
            f.write(l + "\n")


def edge_trace(g):
    """(flip at binding, flip in product 1, flip in product 2) of the error evaluation of every edge, fp64."""
    from openslam_g2o_amd import sbacam as SB
    rows = []
    for k in range(len(g["vi"])):
        t = []
        zinv = SB.inverse_measurement(SB.FP64, g["meas"][k], t)
        SB.cam_edge_error(SB.FP64, g["est"][g["vi"][k]], g["est"][g["vj"][k]], zinv, t)
        rows.append([int(f) for _, f in t])
    return rows


if __name__ == "__main__":
    main()
