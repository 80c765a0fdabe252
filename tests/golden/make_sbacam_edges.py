"""Generator of tests/golden/sbacam_edges.npz and of the oracle-drift lines of profiles/sba_cam.jsonl (CPU only; run from the
repository root: python tests/golden/make_sbacam_edges.py).  Needs the built CPU oracle (make -C oracle).

Per test graph of the device SBA-format front end (EdgeProjectP2MC "m", EdgeProjectP2SC "s"): the inputs,
sbacam.project_edges evaluated with mpmath at 60 digits (rounded to fp64) and the drift of the SAME formulas evaluated in fp64
against them -- max abs over err, max abs over J0 | J1.  The Jacobians are analytic: their drift is the rounding of a few dozen
operations on entries of 1e2 ... 1e3 pixels per unit (~1e-13), far below the 1e-4 of the numeric Sim3 ones.  The GPU tests bound
the device against the mpmath figures by 8 x the drift recorded here for the same graph -- the oracle's own figure, never the
device's.

  m1, m65, m256, m257, m300, s1 ... s300   sbacam_helpers.random_graph: few cameras and points shared by many edges, a fixed
           camera, a fixed point, one pair observed twice, intrinsics and baselines that differ per camera, every pz > 1.5
           (asserted there); one lane per edge and 256 threads per block: 65 crosses a wave boundary, 256 fills a block
           exactly, 257 is one edge more, 300 leaves a partial last block in the staged form
  update   a step x (|x[3:6]| well below 1) over the cameras and points of m65, the cameras' oplus in mpmath and the drift of
           the fp64 oplus as transformations (max abs over R, t); the points move by one fp64 addition per coordinate,
           compared exactly
  lm       synthetic.make_sbacam_ba(12 cameras, 60 points, 4 observations per point, seed 7), mono and stereo, plain and with
           Huber (delta 3): five LM iterations of lm.optimize over the CPU oracle solver (Schur on), fed by the fp64 producers
           and by the mpmath producers (rounded to fp64): chi2 per iteration of both, the max abs difference of the final
           cameras and of the final points."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import lm, synthetic  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import sbacam_helpers as H  # noqa: E402

GRAPH_KEYS = ("est", "points", "hidx", "pt_hidx", "vp", "vl", "zl", "omega_l", "intrinsics")


class OracleSbacamBASolver:
    """The CPU oracle solver over the observation set of a make_sbacam_ba graph."""

    def __init__(self, g, huber):
        self.g, self.huber = g, huber
        d = g["zl"].shape[1]
        self.o = O.OracleSolver(6, 3, g["nP"], g["nL"], True)
        self.k = self.o.add_edge_set(d, g["hidx"][g["vp"]], g["pt_hidx"][g["vl"]])
        self.o.set_dims(self.k, 6, 3)
        self.o.build_structure()

    def feed(self, J0, J1, err):
        self.o.set_edge_data(self.k, J0, J1, self.g["omega_l"], err, self.huber)

    buildSystem = lambda self: self.o.build_system()
    setLambda = lambda self, lam, backup=False: self.o.set_lambda(lam, backup)
    restoreDiagonal = lambda self: self.o.restore_diagonal()
    solve = lambda self: self.o.solve()
    maxDiagonal = lambda self: self.o.max_diagonal()
    computeScale = lambda self, lam: self.o.compute_scale(lam)
    x = lambda self: self.o.x()


def oracle_run(F, g, huber):
    s = OracleSbacamBASolver(g, huber)
    graph = H.HostSbacamBAGraph(F, g, s.feed, s.x, s.o.chi2)
    graph.linearize()
    chi0 = graph.chi2()
    done, chis, lams, trials = lm.optimize(graph, s, H.ITERATIONS, "lm")
    return dict(chi0=chi0, chis=np.array(chis), trials=trials, est=graph.est.copy(), points=graph.points.copy(), done=done)


def producer_figures(g):
    J0, J1, e = H.producers(H.FP64, g)
    M0, M1, me = H.producers(H.MP, g)
    return (M0, M1, me), dict(err=float(np.abs(e - me).max()), J=float(max(np.abs(J0 - M0).max(), np.abs(J1 - M1).max())))


def main():
    out, lines = {}, []
    graphs = {}
    for stereo in (False, True):
        for n in H.EDGE_COUNTS:
            graphs[H.graph_name(n, stereo)] = H.random_graph(n, 100 + n + (1000 if stereo else 0), stereo)
    for name, g in graphs.items():
        (M0, M1, me), fig = producer_figures(g)
        for k in GRAPH_KEYS:
            out["%s_%s" % (name, k)] = g[k]
        out.update({name + "_J0": M0, name + "_J1": M1, name + "_err": me, name + "_drift": np.array([fig["err"], fig["J"]])})
        lines.append(dict(kind="oracle_drift", graph=name, edges=int(len(g["vp"])), err_max_abs=float(np.abs(me).max()),
                          J_max_abs=float(max(np.abs(M0).max(), np.abs(M1).max())), **fig))
        print(lines[-1], flush=True)

    g = graphs["m65"]
    x = H.update_step(g, 21)
    up64, upmp = H.update(H.FP64, g["est"], g["hidx"], x), H.update(H.MP, g["est"], g["hidx"], x)
    d = H.transform_gap(up64, upmp)
    out.update(update_x=x, update_est=upmp, update_points=H.moved_points(g["points"], g["pt_hidx"], g["nP"], x),
               update_drift=np.array([d]))
    lines.append(dict(kind="oracle_drift", graph="update (oplus over the cameras of m65)", transform=d))
    print(lines[-1], flush=True)

    for tag, stereo, huber in H.RUNS:
        g = synthetic.make_sbacam_ba(stereo=stereo, **H.BA_ARGS)
        a, b = oracle_run(H.FP64, g, huber), oracle_run(H.MP, g, huber)
        # (no assertion on equal trial counts: once converged the sign of LM's gain ratio is rounding noise, and what such a
        # trial changes in the estimates is part of the recorded difference)
        rel = np.abs(a["chis"] - b["chis"]) / np.abs(b["chis"])
        dest, dpts = H.transform_gap(a["est"], b["est"]), float(np.abs(a["points"] - b["points"]).max())
        out.update({"lm_%s_chis" % tag: b["chis"], "lm_%s_rel" % tag: rel, "lm_%s_est_drift" % tag: np.array([dest]),
                    "lm_%s_points_drift" % tag: np.array([dpts]), "lm_%s_trials" % tag: np.array(b["trials"]),
                    "lm_%s_chi0" % tag: np.array([b["chi0"]])})
        lines.append(dict(kind="oracle_drift", graph="lm " + tag, args=H.BA_ARGS, stereo=stereo, huber=huber, edges=int(len(g["vp"])),
                          chi2_initial=b["chi0"], chi2_mp=[float(v) for v in b["chis"]], chi2_rel_fp64_vs_mp=[float(v) for v in rel],
                          trials=[int(t) for t in b["trials"]], trials_fp64=[int(t) for t in a["trials"]],
                          final_cameras_max_abs=dest, final_points_max_abs=dpts))
        print(lines[-1], flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sbacam_edges.npz"), **out)
    path = os.path.join(ROOT, "profiles", "sba_cam.jsonl")
    keep = []
    if os.path.exists(path):
        keep = [l for l in open(path).read().splitlines() if l.strip() and json.loads(l).get("kind") != "oracle_drift"]
    with open(path, "w") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")
        for l in keep:
            f.write(l + "\n")


if __name__ == "__main__":
    main()
