"""Writes tests/golden/assembly_blocks.npz and the CPU rows of profiles/assembly_blocks.jsonl: per case of tests/assembly_helpers.py
the SHA-256 of the rebuilt inputs, the 60-digit references of Hpp, Hpl, Hll, b, chi2 (computeScale, H x) rounded to fp64, the
per-block scales and the figures of the two fp64 evaluations on the CPU (oracle.OracleSolver; NumPy in the kernels' order).

    python tests/golden/make_assembly_blocks.py            (about two minutes; byte-stable)"""
import io
import json
import multiprocessing
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import assembly_helpers as H  # noqa: E402

F64 = np.vectorize(float, otypes=[np.float64])


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates (byte-stable)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def _block_scales(a):
    return np.array([float(max(np.asarray(v).reshape(-1))) for v in a]) if len(a) else np.zeros(0)


def references(name):
    """{key: array} of one case and its profile records."""
    import mpmath as mp
    from oracle import oracle as O
    from tests import reference_mp  # noqa: F401
    c = H.make_case(name)
    st = H.structure(c)
    out = {"input_sha": np.array(H.input_hash(c))}
    n_rob, n_on, n_bad = H.threshold_census(c)
    assert n_bad == 0, (name, n_bad)
    out["threshold"] = np.array([n_rob, n_on, n_bad])
    ref, scale, cpu = {}, {}, {}
    MP = np.vectorize(lambda v: mp.mpf(float(v)), otypes=[object])
    if c["kind"] == "exact":
        K = np.rint(c["sets"][0]["err"][:, 0] * 8).astype(np.int64)
        total = int((K * K).sum())
        assert total < 2 ** 53 and np.array_equal(K / 8.0, c["sets"][0]["err"][:, 0])
        out["exact_chi2"] = np.array(total / 64.0)
    elif c["kind"] == "chi2":
        m, e = H.evaluate(c, st, "mp", False), H.evaluate(c, st, "np", False)
        o = H.oracle_solver(O, c)
        ref["chi2"], scale["chi2"] = [m["chi2"]], [m["chi2_s"]]
        cpu["chi2"] = ([o.chi2()], [e["chi2"]])
    elif c["kind"] == "scale":
        m, e = H.evaluate(c, st, "mp"), H.evaluate(c, st, "np")
        b = np.concatenate([e["bp"].reshape(-1), e["bl"].reshape(-1)])
        bm = np.concatenate([m["bp"].reshape(-1), m["bl"].reshape(-1)])
        assert all(mp.mpf(float(v)) == w for v, w in zip(b, bm)) and np.array_equal(b, c["b_exact"])        # b is exact
        x, lam = MP(c["x"]), mp.mpf(c["lam"])
        ref["scale"] = [sum(xi * (lam * xi + bi) for xi, bi in zip(x, bm))]
        scale["scale"] = [sum(abs(xi) * (abs(lam * xi) + abs(bi)) for xi, bi in zip(x, bm))]
        o = H.oracle_solver(O, c)
        assert np.array_equal(o.b(), b)
        o.view("x", o.n)[:] = c["x"]
        cpu["scale"] = ([o.compute_scale(c["lam"])], [H.scale_numpy(c, b)])
    else:
        m, e = H.evaluate(c, st, "mp"), H.evaluate(c, st, "np")
        ov = H.oracle_evaluation(O, c, st)
        nv = H.numpy_outputs(c, st, e)
        rb = H.blocks_of(c, m)
        sb = H.blocks_of(c, {k[:-2]: v for k, v in m.items() if k.endswith("_s") and k != "chi2_s"})
        for k in rb:
            ref[k], scale[k], cpu[k] = rb[k], _block_scales(sb[k]), (ov[k], nv[k])
        ref["chi2"], scale["chi2"], cpu["chi2"] = [m["chi2"]], [m["chi2_s"]], (ov["chi2"], nv["chi2"])
        if c["kind"] == "single":
            s0 = c["sets"][0]
            n, d = s0["n"], s0["d"]
            Om = MP(s0["om"]).reshape(n, d, d)
            A = [MP(s0["J0"]).reshape(n, s0["d0"], d).transpose(0, 2, 1), MP(s0["J1"]).reshape(n, s0["d1"], d).transpose(0, 2, 1)]
            idx, M, sw = np.zeros((3, n, 2), np.int64), np.zeros((3, n)), np.zeros((3, n))
            for k, (qd, qo, tr, q1) in enumerate(H.single_blocks(c, st)):
                L, Rm = (A[1][k], A[0][k]) if tr else (A[0][k], A[1][k])
                for row, (X, Y, blk) in enumerate(((A[0][k], A[0][k], qd), (L, Rm, qo), (A[1][k], A[1][k], q1))):
                    Mx, aM = X.T @ Om[k] @ Y, np.abs(X).T @ np.abs(Om[k]) @ np.abs(Y)
                    i = np.unravel_index(np.argmax(F64(np.abs(Mx) / aM)), Mx.shape)
                    idx[row, k], M[row, k] = i, float(Mx[i])
                    sw[row, k] = float(max(m["Hpp_s"][blk].reshape(-1)) / abs(Mx[i]))
            out["single_idx"], out["single_M"] = idx, M
            wo, wn = (H.weights_from_blocks(c, st, v["Hpp"], idx, M) for v in (ov, nv))
            both = lambda a: np.concatenate([a[0], a[2]])           # w_diag: vertex 0 of every edge, then vertex 1
            ref["w_diag"], scale["w_diag"], cpu["w_diag"] = list(m["w"][0]) * 2, both(sw), (both(wo), both(wn))
            ref["w_off"], scale["w_off"], cpu["w_off"] = list(m["w"][0]), sw[1], (wo[1], wn[1])
        if name in H.HX_CASES:
            o = ov["_o"]
            for i, lam in enumerate(c["lams"]):
                k = "Hx%d" % i
                lm = (mp.mpf(lam[0]), mp.mpf(lam[1]))
                ref[k] = H.split_b(c, H.multiply(c, st, m, MP(c["x"]), lm, dt=object))
                scale[k] = _block_scales(H.split_b(c, H.multiply(c, st, m, MP(c["x"]), lm, dt=object, absolute=True)))
                o.build_system()
                o.set_lambda_split(lam[0], lam[1], False)
                cpu[k] = (H.split_b(c, o.multiply_full(c["x"])), H.split_b(c, H.multiply(c, st, e, c["x"], lam)))
    recs = []
    for k in ref:
        r64 = [F64(np.asarray(v, dtype=object)) for v in ref[k]]
        s64 = np.array([float(v) for v in scale[k]])
        figs = [float(H.figures(g, r64, s64).max()) for g in cpu[k]]
        out[k] = np.concatenate([np.asarray(v).reshape(-1) for v in r64]) if k in ("b", "Hx0", "Hx1") else np.array(r64)
        out[k + "_s"], out[k + "_cpu"] = s64, np.array(figs)
        # 0 unless both CPU figures are 0: then 0.5, the figure of a result rounded once (as tests/golden/make_schur_blocks.py)
        out[k + "_floor"] = np.float64(0.5 if max(figs) == 0.0 else 0.0)
        assert np.all(np.isfinite(figs)), (name, k, figs)
        recs.append(dict(path="cpu", case=name, output=k, cpu_oracle=figs[0], cpu_numpy=figs[1], bound=H.MARGIN * max(max(figs), float(out[k + "_floor"]))))
    return name, out, recs


def main():
    names = sys.argv[1:] or sorted(H.NAMES, key=lambda n: -sum(s["n"] * s["d"] ** 2 for s in H.make_case(n)["sets"]))
    with multiprocessing.Pool(min(8, len(names))) as pool:
        results = pool.map(references, names, chunksize=1)
    arrays, recs = {}, []
    for name, out, rec in sorted(results, key=lambda r: r[0]):
        for k, v in out.items():
            arrays[name + "/" + k] = v
        recs += rec
    if sys.argv[1:]:
        for r in recs:
            print(json.dumps(r))
        return
    write_npz(H.FIXTURE, arrays)
    # profiles/assembly_blocks.jsonl: the CPU rows are rewritten, the device rows (the ASMBLK lines of the GPU test) kept
    prof = os.path.join(ROOT, "profiles", "assembly_blocks.jsonl")
    kept = []
    if os.path.exists(prof):
        with open(prof) as f:
            kept = [line for line in f if line.strip() and json.loads(line).get("path") != "cpu"]
    with open(prof, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
        f.writelines(kept)
    print("wrote", H.FIXTURE, os.path.getsize(H.FIXTURE), "bytes,", len(recs), "CPU rows")


if __name__ == "__main__":
    main()
