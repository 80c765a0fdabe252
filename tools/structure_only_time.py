"""Times g2ohip_ba_structure_only at scale and appends the figures to profiles/structure_only.jsonl:

  - the time per call (num_iters = 10), min .. max over ten calls from the same perturbed start, mono and stereo;
  - the distribution of outer iterations and of stop reasons;
  - for context, one error-only g2ohip_ba_linearize and one device-resident LM iteration on the same graph;
  - the fp64 restatement (openslam_g2o_amd/structure_only.py) on the first 2 000 points -- a pure Python evaluation, edge by
    edge, not a C++ host implementation: it says what the check costs, not what a CPU can do.

    python tools/structure_only_time.py [--cams 20000 --points 200000 --obs 5 --calls 10]

There is no pass / fail threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openslam_g2o_amd import lm, structure_only as SO, synthetic  # noqa: E402


def measure(prob, calls, host_points):
    L = prob["L"]
    hidx = np.arange(L, dtype=np.int32)
    s, graph = lm.setup_device_ba(prob)
    s.baStructureOnly(1, 10)                          # first launch: code object load
    times, tr = [], None
    for _ in range(calls):
        s.baSetEstimates(prob["cams"], prob["cam_hidx"], prob["pts"], hidx)
        s.sync()
        t = time.perf_counter()
        s.baStructureOnly(10, 10)
        s.sync()
        times.append(time.perf_counter() - t)
    s.baSetEstimates(prob["cams"], prob["cam_hidx"], prob["pts"], hidx)
    tr, chi = s.baStructureOnly(10, 10, trace=True)
    s.baSetEstimates(prob["cams"], prob["cam_hidx"], prob["pts"], hidx)
    graph.compute_active_errors()
    s.sync()
    lin = []
    for _ in range(5):
        s.baSetEstimates(prob["cams"], prob["cam_hidx"], prob["pts"], hidx)
        s.sync()
        t = time.perf_counter()
        graph.compute_active_errors()
        s.sync()
        lin.append(time.perf_counter() - t)
    it_times = []
    lm.optimize(graph, s, 3, times=it_times)
    few = dict(prob)
    keep = prob["pt_idx"] < host_points
    for k in ("cam_idx", "pt_idx", "meas"):
        few[k] = prob[k][keep]
    few["pts"] = prob["pts"][:host_points]
    t = time.perf_counter()
    SO.structure_only(few, 10, 10)
    host = time.perf_counter() - t
    return dict(seconds_per_call_min=min(times), seconds_per_call_max=max(times), calls=calls,
                outer_iterations=np.bincount(tr[:, 0], minlength=11).tolist(), stop_reasons=np.bincount(tr[:, 3], minlength=4).tolist(),
                chi2_before=float(chi[:, 0].sum()), chi2_after=float(chi[:, 1].sum()),
                seconds_error_only_linearize_min=min(lin), seconds_lm_iteration_min=min(it_times[1:] or it_times),
                python_restatement_points=host_points, python_restatement_seconds=host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=20000)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--obs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-points", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_only.jsonl"))
    a = ap.parse_args()
    for stereo in (False, True):
        prob = synthetic.make_ba_problem(a.cams, a.points, obs_per_landmark=a.obs, stereo_baseline=0.3 if stereo else None)
        rng = np.random.default_rng(1)
        prob["pts"] = prob["pts"] + rng.uniform(-0.5, 0.5, prob["pts"].shape)      # the perturbed start of every call
        rec = dict(what="g2ohip_ba_structure_only at scale", binding="EdgeProjectXYZ2UVU" if stereo else "EdgeProjectXYZ2UV", cameras=a.cams,
                   points=a.points, observations=int(prob["E"]), num_iters=10, num_max_trials=10)
        rec.update(measure(prob, a.calls, a.host_points))
        print(json.dumps(rec, sort_keys=True), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
