"""Writes tests/golden/structure_only.npz: the graphs of tests/structure_only_helpers.py with the 60-digit run of the
structure-only restatement on each (traces, points, chi2, every decision's value), the fp64-vs-60-digit drift and the decision
margins; the drift also goes to profiles/structure_only.jsonl.

For every graph seeds are drawn until (a) the fp64 and the 60-digit run take the same path, (b) every decision of the 60-digit
run is at least 1000 x the largest fp64-vs-60-digit difference of that quantity on the graph away from its threshold, and (c), on
the graphs with the special tracks, at least one point's first trial is rejected.  If no seed of a graph qualifies the noise
shrinks (never the factor).  That condition is held by runs of H.TRACE_ITERS outer iterations (structure_only_helpers.py says
why); the ten-iteration run of the same graph must (d) take the same path in both arithmetics with every decision at least 1000 x
ITS OWN fp64-vs-60-digit difference away from its threshold, and is recorded with its traces, decisions and drift.

    python tests/golden/make_structure_only.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import structure_only_helpers as H  # noqa: E402


def main():
    out = {}
    for gi, name in enumerate(H.SPECS):
        found = None
        for noise in (1.0, 0.01, 0.001):
            for seed in range(100 * gi, 100 * gi + (2 if noise == 1.0 else 14)):
                g = H.make_graph(name, seed, noise=noise)
                c = H.compare(g, name)
                _, t1, _ = H.run(H.MP, g, name, H.TRACE_ITERS, 1)
                rejected_first = bool(((t1[:, 3] == 2) & (t1[:, 0] == 1)).any())
                print(name, "seed", seed, "noise", noise, "trace_equal", c["trace_equal"], "margins_ok", c["margins_ok"], "first trial rejected",
                      rejected_first, c["margin"], c["diff"], flush=True)
                if c["trace_equal"] and c["margins_ok"] and (rejected_first or not H.SPECS[name]["specials"]):
                    c10 = H.compare(g, name, 10, 10)
                    print("   ten iterations: trace_equal", c10["trace_equal"], "every decision 1000 x its own difference:", c10["each_ok"], flush=True)
                    if c10["trace_equal"] and c10["each_ok"]:
                        found = (g, c, seed, noise, c10)
                        break
            if found:
                break
        if not found:
            raise SystemExit("no seed of %s meets the margin condition" % name)
        g, c, seed, noise, c10 = found
        p1, t1, _ = H.run(H.MP, g, name, H.TRACE_ITERS, 1)
        for k in H.GRAPH_KEYS:
            if k in g:
                out["%s/%s" % (name, k)] = g[k]
        kinds = list(H.THRESHOLD)
        out["%s/ref_trace" % name] = c["trace"]
        out["%s/ref_pts" % name] = c["pts"]
        out["%s/ref_chi2" % name] = c["chi2"]
        out["%s/ref_drift" % name] = np.array([c["drift_pts"], c["drift_chi2"]])
        out["%s/ref_decisions" % name] = c["decisions"]
        out["%s/ref_margin" % name] = np.array([c["margin"][k] for k in kinds])
        out["%s/ref_diff" % name] = np.array([c["diff"][k] for k in kinds])
        out["%s/ref_pts10" % name] = c10["pts"]
        out["%s/ref_chi210" % name] = c10["chi2"]
        out["%s/ref_drift10" % name] = np.array([c10["drift_pts"], c10["drift_chi2"]])
        out["%s/ref_trace10" % name] = c10["trace"]
        out["%s/ref_each10" % name] = c10["each"]
        out["%s/ref_trace1" % name] = t1
        out["%s/ref_pts1" % name] = H.SO.to_f64(p1)
        H.append_profile(dict(what="fp64 restatement vs 60-digit run", graph=name, outer_iterations=H.TRACE_ITERS,
                              drift_points_10_iterations=c10["drift_pts"], drift_chi2_10_iterations=c10["drift_chi2"], seed=seed, noise_px=noise, drift_points=c["drift_pts"],
                              drift_chi2=c["drift_chi2"], margin=c["margin"], largest_difference=c["diff"],
                              stop_reasons=np.bincount(c["trace"][:, 3], minlength=4).tolist(),
                              stop_reasons_10_iterations=np.bincount(c10["trace"][:, 3], minlength=4).tolist(),
                              outer_iterations_10_iterations=np.bincount(c10["trace"][:, 0], minlength=11).tolist()))
    np.savez_compressed(H.GOLDEN, **out)
    print("wrote", H.GOLDEN, os.path.getsize(H.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
