#!/usr/bin/env python3
"""Times Predictor.overlap (host/score.py, csrc/overlap.hip) at the two shapes DESIGN section 20 quotes, and prints one JSON line.

  N = 1e6, D = 64, a Float32 device tensor (the `.T` view of (N, D) memory), K = 32 and K = 256

On the same data, in the same process:
  floor         Predictor.predict_labels alone: the overlap cannot avoid evaluating that table
  composition   what could be done before: Predictor.predict, then P.double().T @ P.double() in torch, in chunks of 262144 rows
  overlap       Predictor.overlap
and the matrices of the two routes compared: the largest relative difference, in units of the bound n * 2^-52.
`contraction` is overlap - floor; its rate counts the N K (K + 1) flops of the lower triangle against the Float64 matrix peak of the
MI355X data sheet, 78.6 TFLOP/s.  The data are drawn by Predictor.sample from the model they are scored with.  Every figure is the median
(and the minimum) of --reps calls after one warm-up call, timed from the host around the call; every call ends synchronised (the results
are read or torch.cuda.synchronize is called).  --scale shrinks N (a quick check of the script itself)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F64_MATRIX_PEAK = 78.6e12
CHUNK = 262144


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--K", default="32,256")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale}

    def note(msg):
        print("[bench_overlap] " + msg, file=sys.stderr, flush=True)

    def median_ms(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": float(np.median(ts)), "best_ms": float(min(ts))}

    def composition(p, data):
        _, P = p.predict(data)
        K = P.shape[1]
        O = torch.zeros((K, K), dtype=torch.float64, device=P.device)
        for lo in range(0, P.shape[0], CHUNK):
            Q = P[lo:lo + CHUNK].double()
            O += Q.T @ Q
        return O.cpu().numpy()

    N, D = int(1e6 * a.scale), 64
    for K in (int(k) for k in a.K.split(",")):
        post, _, _, _ = R.niw_model(D, K, 60.0, 1)
        with score.Predictor.load(R.predictor_file(0, D, 1.0, np.full(K, 100.0), post), capacity=N) as p:
            note(f"K = {K}: drawing the data")
            x, _ = p.sample(N, seed=1)
            xs = x.T[torch.randperm(N, device=x.device)].contiguous()          # (N, D) float32, the clusters mixed
            del x
            torch.cuda.empty_cache()
            data = xs.T
            r = {"N": N, "D": D, "K": K}
            note(f"K = {K}: floor")
            r["floor"] = median_ms(lambda: p.predict_labels(data))
            note(f"K = {K}: composition")
            r["composition"] = median_ms(lambda: composition(p, data))
            note(f"K = {K}: overlap")
            r["overlap"] = median_ms(lambda: p.overlap(data))
            ov, ref = p.overlap(data), composition(p, data)
            rel = np.abs(ov.matrix - ref) / np.maximum(np.maximum(ov.matrix, ref), 1e-300)
            r["max_rel_diff_in_bounds"] = float(rel.max() / (N * 2.0 ** -52))
            r["skipped"] = ov.skipped
            r["overlap"]["over_floor"] = r["overlap"]["ms"] / r["floor"]["ms"]
            r["overlap"]["over_composition"] = r["overlap"]["ms"] / r["composition"]["ms"]
            ms = max(r["overlap"]["ms"] - r["floor"]["ms"], 1e-6)
            r["contraction"] = {"ms": ms, "tflops": N * K * (K + 1) / ms / 1e9, "share_of_f64_matrix_peak": N * K * (K + 1) / (ms * 1e-3) / F64_MATRIX_PEAK}
            out[f"K{K}"] = r
            del xs, data
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
