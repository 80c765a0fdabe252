"""Generator of tests/golden/scam_edges.npz (CPU only; run from the repository root: python tests/golden/make_scam_edges.py).  Needs
mpmath and the built CPU oracle (make -C oracle; its VertexSE3 oplus moves the cameras).

ONE graph of 300 stereo observations Edge_XYZ_VSC (scam_helpers.base_graph: 4 VertexSCam cameras whose rotations are far from the
identity and from each other, camera 0 fixed, 3 EdgeSE3 odometry edges, 12 points of which one is fixed; the observations cycle
over the 48 camera / point pairs, so pairs repeat); the graphs of the edge counts 1, 63, 64, 65, 255, 256, 257, 300 are its first n
observations (one lane per edge, 64 lanes per wave, 256 threads per block: either side of a wave and of a block, and a partial last
block), so one set of arrays serves them all:

  graph_*                    the graph
  err, J0, J1                scam.py evaluated with mpmath at 60 digits, rounded to fp64
  drift [8][2]               per edge count: max abs of the SAME formulas evaluated in fp64 against them, over err and over J0 | J1.
                             The GPU tests bound the device against the fp64 restatement by 8 x this figure -- the restatement's
                             own, never the device's
  moved_x, moved_poses, moved_points, moved_err, moved_drift [8]   a step over the free cameras (the oracle's oplus) and the free
                             points (plain addition), the moved estimates, the errors there at 60 digits and the drift of the fp64
                             errors there (the error-only evaluation)
  numeric_noise              max abs of the reference's central difference through the VertexSE3 oplus (delta = 1e-9) evaluated at
                             60 digits against the exact Jacobian at 60 digits -- only the truncation error of the difference remains
  J_max_abs                  max |J| at 60 digits

Asserted here (the seed is chosen so that they hold; no edge needs excluding anywhere):
  - every depth q2 is at least 1, before and after the move
  - the drift of the errors of the first edge is not zero, before or after the move: 8 x 0 would ask for bit equality
  - numeric_noise < 1e-9 max|J|: the truncation of the central difference is of order delta^2 = 1e-18 relative, a wrong column
    of order 1"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from openslam_g2o_amd import scam as SC  # noqa: E402
from tests import scam_helpers as H  # noqa: E402

MOVE_SEED = 21


def first_edge_drift(g, moved):
    one = H.take_edges(g, slice(0, 1))
    a = np.abs(H.producers(H.FP64, one, jac=False) - H.producers(H.MP(), one, jac=False)).max()
    b = np.abs(H.producers(H.FP64, one, moved[0], moved[1], jac=False) - H.producers(H.MP(), one, moved[0], moved[1], jac=False)).max()
    return a, b


def check_inputs(g, moved):
    assert H.depths(g).min() >= H.MIN_DEPTH and H.depths(g, moved[0], moved[1]).min() >= H.MIN_DEPTH
    a, b = first_edge_drift(g, moved)
    assert a > 0 and b > 0, (a, b)


def find_seed(limit=200):
    for seed in range(limit):
        g = H.base_graph(seed=seed)
        try:
            check_inputs(g, H.oplus(g, g["poses"], g["points"], H.update_step(g, MOVE_SEED)))
        except AssertionError:
            continue
        return seed
    raise SystemExit("no seed below %d meets the assertions" % limit)


def main():
    if "--find-seed" in sys.argv:
        print("seed", find_seed())
        return
    MP = H.MP()
    out = {}
    g = H.base_graph()
    x = H.update_step(g, MOVE_SEED)
    moved = H.oplus(g, g["poses"], g["points"], x)
    check_inputs(g, moved)
    print("depths", H.depths(g).min(), H.depths(g).max(), "moved", H.depths(g, *moved).min(), flush=True)
    for k in H.GRAPH_KEYS:
        out["graph_" + k] = np.asarray(g[k])
    a, b = H.producers(H.FP64, g), H.producers(MP, g)
    de = np.abs(a[2] - b[2]).max(axis=1)
    dJ = np.maximum(np.abs(a[0] - b[0]).max(axis=1), np.abs(a[1] - b[1]).max(axis=1))
    out.update(J0=b[0], J1=b[1], err=b[2])
    e64, emp = (H.producers(F, g, moved[0], moved[1], jac=False) for F in (H.FP64, MP))
    dm = np.abs(e64 - emp).max(axis=1)
    assert de[0] > 0 and dm[0] > 0, (de[0], dm[0])
    out.update(moved_x=x, moved_poses=moved[0], moved_points=moved[1], moved_err=emp,
               drift=np.array([[de[:n].max(), dJ[:n].max()] for n in H.EDGE_COUNTS]),
               moved_drift=np.array([dm[:n].max() for n in H.EDGE_COUNTS]))
    for n, row, mv in zip(H.EDGE_COUNTS, out["drift"], out["moved_drift"]):
        print(dict(edges=int(n), err=float(row[0]), J=float(row[1]), moved_err=float(mv)), flush=True)
    N0, N1 = SC.numeric_edges(MP, g["poses"], g["points"], g["vp"], g["vl"], g["zl"], g["kcam"])
    noise, jmax = 0.0, 0.0   # (against the exact Jacobian at 60 digits, unrounded)
    for k in range(len(g["vp"])):
        A, B = SC.scam_jacobians(MP, g["poses"][g["vp"][k]], g["points"][g["vl"][k]], g["kcam"])
        noise = max(noise, max(abs(float(n_ - a_)) for n_, a_ in zip(list(N0[k]) + list(N1[k]), A + B)))
        jmax = max(jmax, max(abs(float(a_)) for a_ in A + B))
    print(dict(numeric_noise=noise, J_max_abs=jmax), flush=True)
    assert noise < 1e-9 * jmax, (noise, jmax)
    out.update(numeric_noise=np.array(noise), J_max_abs=np.array(jmax))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "scam_edges.npz"), **out)


if __name__ == "__main__":
    main()
