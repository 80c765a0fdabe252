"""Generator of tests/golden/sim3_edges.npz and of the oracle-drift lines of profiles/sim3_edges.jsonl (CPU only; run from the
repository root: python tests/golden/make_sim3_edges.py).  Needs the built CPU oracle (make -C oracle).

Per test graph of the device Sim3 front end: the inputs, the producers of tests/sim3_helpers.py evaluated with mpmath at 60
digits (rounded to fp64) and the drift of the SAME formulas evaluated in fp64 against them -- max abs over err, max abs over
J0 | J1.  The drift of J is ~1e-7: the reference defines this Jacobian as a central difference with delta = 1e-9, and 1 /
(2 delta) = 5e8 multiplies every rounding of the error.  The GPU tests bound the device against the mpmath figures by 8 x the
drift recorded here for the same graph -- the oracle's own figure, never the device's.

  branch   tests/sim3_helpers.branch_class_graph: every log branch class of the error x (fixed vertex on side 0, on side 1,
           free / free twice) and one edge with e = 0 exactly; 17 edges
  n1, n18, n19, n300   sim3_helpers.random_graph: few vertices shared by many edges; 14 lanes per edge and 256 threads per block put
           18 edges (252 lanes) inside one block of the Jacobian kernel and let the 19th straddle it; 257 edges (the first
           257 of n300, drift recorded on its own) are one more than a block of the error kernel; 300 leave partial last blocks
  update   a step x over the vertices of `branch` that takes every exp branch, its oplus in mpmath, and the drift of the fp64
           oplus as transformations (max abs over R, t, s)
  lm       synthetic.make_sim3_graph(40, loop_every=10, scale_drift=0.01, seed=7): ten LM iterations of lm.optimize over the CPU
           oracle solver, fed by the fp64 producers and by the mpmath producers (rounded to fp64), plain and with Huber (delta
           5) on the set: chi2 per iteration of both, their relative difference, the max abs difference of the final estimates,
           the relative difference of the first Gauss-Newton step dx."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import lm, synthetic  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import sim3_helpers as H  # noqa: E402

LM_ARGS = dict(n=40, loop_every=10, scale_drift=0.01, seed=7)
HUBER = 5.0
ITERATIONS = 10


class OracleSim3Solver:
    def __init__(self, g):
        self.o = O.OracleSolver(7, 3, g["num_free"], 0, False)
        k = self.o.add_edge_set(7, g["hidx"][g["vi"]], g["hidx"][g["vj"]])
        self.o.set_dims(k, 7, 7)
        self.o.build_structure()

    buildSystem = lambda self: self.o.build_system()
    setLambda = lambda self, lam, backup=False: self.o.set_lambda(lam, backup)
    restoreDiagonal = lambda self: self.o.restore_diagonal()
    solve = lambda self: self.o.solve()
    maxDiagonal = lambda self: self.o.max_diagonal()
    computeScale = lambda self, lam: self.o.compute_scale(lam)
    x = lambda self: self.o.x()


def oracle_run(F, g, huber):
    s = OracleSim3Solver(g)
    graph = H.HostSim3Graph(F, g, lambda J0, J1, err: s.o.set_edge_data(0, J0, J1, g["info"], err, huber), s.x, s.o.chi2)
    graph.linearize()
    chi0 = graph.chi2()
    s.buildSystem()
    assert s.solve()
    dx0 = s.x().copy()
    done, chis, lams, trials = lm.optimize(graph, s, ITERATIONS, "lm")
    return dict(chi0=chi0, dx0=dx0, chis=np.array(chis), trials=trials, est=graph.est.copy(), done=done)


def producer_figures(g, n=None):
    sl = slice(0, n)
    args = (g["est"], g["vi"][sl], g["vj"][sl], g["meas"][sl], g["hidx"])
    t64, tmp = [], []
    J0, J1, e = H.edges(H.FP64, *args, trace=t64)
    M0, M1, me = H.edges(H.MP, *args, trace=tmp)
    assert t64 == tmp, "fp64 and mpmath took different branches"
    return (M0, M1, me), dict(err=float(np.abs(e - me).max()), J=float(max(np.abs(J0 - M0).max(), np.abs(J1 - M1).max())))


def main():
    out, lines = {}, []
    graphs = dict(branch=H.branch_class_graph(), n1=H.random_graph(1, 11), n18=H.random_graph(18, 12), n19=H.random_graph(19, 13),
                  n300=H.random_graph(300, 14))
    for name, g in graphs.items():
        (M0, M1, me), fig = producer_figures(g)
        for k in ("est", "hidx", "vi", "vj", "meas"):
            out["%s_%s" % (name, k)] = g[k]
        out.update({name + "_J0": M0, name + "_J1": M1, name + "_err": me, name + "_drift": np.array([fig["err"], fig["J"]])})
        lines.append(dict(kind="oracle_drift", graph=name, edges=int(len(g["vi"])), **fig))
        print(lines[-1], flush=True)
    _, fig = producer_figures(graphs["n300"], 257)
    out["n257_drift"] = np.array([fig["err"], fig["J"]])
    lines.append(dict(kind="oracle_drift", graph="n257 (first 257 edges of n300)", edges=257, **fig))

    g = graphs["branch"]
    rng = np.random.default_rng(21)
    x = np.concatenate([H.branch_vector(h % 4, rng) for h in range(g["num_free"])])
    up64, upmp = H.update(H.FP64, g["est"], g["hidx"], x), H.update(H.MP, g["est"], g["hidx"], x)
    d = 0.0
    for a, b in zip(up64, upmp):
        (Ra, ta, sa), (Rb, tb, sb) = H.transform(a), H.transform(b)
        d = max(d, np.abs(Ra - Rb).max(), np.abs(ta - tb).max(), abs(sa - sb))
    out.update(update_x=x, update_est=upmp, update_drift=np.array([d]))
    lines.append(dict(kind="oracle_drift", graph="update (oplus over branch, all exp branches)", transform=float(d)))

    g = synthetic.make_sim3_graph(**LM_ARGS)
    for tag, huber in (("plain", 0.0), ("huber", HUBER)):
        a, b = oracle_run(H.FP64, g, huber), oracle_run(H.MP, g, huber)
        assert a["trials"] == b["trials"], (a["trials"], b["trials"])
        rel = np.abs(a["chis"] - b["chis"]) / np.abs(b["chis"])
        dest = float(np.abs(a["est"] - b["est"]).max())
        dx = float(np.abs(a["dx0"] - b["dx0"]).max() / np.abs(b["dx0"]).max())
        out.update({"lm_%s_chis" % tag: b["chis"], "lm_%s_rel" % tag: rel, "lm_%s_est" % tag: b["est"],
                    "lm_%s_est_drift" % tag: np.array([dest]), "lm_%s_trials" % tag: np.array(b["trials"]),
                    "lm_%s_chi0" % tag: np.array([b["chi0"]]), "lm_%s_dx_drift" % tag: np.array([dx])})
        lines.append(dict(kind="oracle_drift", graph="lm " + tag, args=LM_ARGS, huber=huber, edges=int(len(g["vi"])), chi2_initial=b["chi0"],
                          chi2_mp=[float(v) for v in b["chis"]], chi2_rel_fp64_vs_mp=[float(v) for v in rel], trials=[int(t) for t in b["trials"]],
                          final_estimates_max_abs=dest, dx_first_solve_rel=dx))
        print(lines[-1], flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sim3_edges.npz"), **out)
    path = os.path.join(ROOT, "profiles", "sim3_edges.jsonl")
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
