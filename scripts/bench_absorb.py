#!/usr/bin/env python3
"""Times Predictor.statistics (host/score.py, csrc/batchstats.hip) at the two shapes DESIGN section 22 quotes, and prints one JSON line.

  N = 1e6, K = 32, a Float32 device tensor (the `.T` view of (N, D) memory), D = 64 and D = 256

On the same data, in the same process:
  floor              Predictor.predict_labels alone: the statistics cannot avoid evaluating that table
  composition_soft   what could be done before: Predictor.predict, then torch.einsum('ik,id,ie->kde', P.double(), X.double(), X.double()),
                     in chunks of rows sized so that a (rows, K, D) Float64 intermediate stays within 256 MB
  composition_hard   Predictor.predict_labels, an index sort of the labels, then X_k.double().T @ X_k.double() per cluster
  hard, soft         Predictor.statistics(assign=...)
and S of the two routes compared: the largest difference in units of 2 gamma(n + 2) T (T from the torch route's |x| products).
`added` is statistics - floor; its rate counts the D (D + 1) flops of the lower triangle per non-zero weight (hard: one per point; soft:
the entries of P above 0) against the Float64 matrix peak of the MI355X data sheet, 78.6 TFLOP/s.  The data are drawn by Predictor.sample
from the model they are scored with.  Every figure is the median (and the minimum) of --reps calls after one warm-up call, timed from
the host around the call; every call ends synchronised.  --scale shrinks N (a quick check of the script itself)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--D", default="64,256")
    ap.add_argument("--K", type=int, default=32)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale}

    def note(msg):
        print("[bench_absorb] " + msg, file=sys.stderr, flush=True)

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

    def composition_soft(p, data, absolute=False):
        _, P = p.predict(data)
        X = data.T                                                             # (N, D)
        K, D = P.shape[1], X.shape[1]
        S = torch.zeros((K, D, D), dtype=torch.float64, device=P.device)
        rows = max(1, (1 << 28) // (8 * K * D))
        for lo in range(0, P.shape[0], rows):
            x = X[lo:lo + rows].double()
            if absolute:
                x = x.abs()
            S += torch.einsum("ik,id,ie->kde", P[lo:lo + rows].double(), x, x)
        return S.cpu().numpy()

    def composition_hard(p, data):
        lab = p.predict_labels(data)
        X = data.T
        K, D = p.K, X.shape[1]
        order = torch.argsort(lab)
        ends = torch.searchsorted(lab[order], torch.arange(1, K + 2, device=lab.device)).tolist()
        S = torch.zeros((K, D, D), dtype=torch.float64, device=lab.device)
        for k in range(K):
            x = X[order[ends[k]:ends[k + 1]]].double()
            S[k] = x.T @ x
        return S.cpu().numpy()

    N, K = int(1e6 * a.scale), a.K
    for D in (int(d) for d in a.D.split(",")):
        post, _, _, _ = R.niw_model(D, K, 60.0, 1)
        with score.Predictor.load(R.predictor_file(0, D, 1.0, np.full(K, 100.0), post), capacity=N) as p:
            note(f"D = {D}: drawing the data")
            x, _ = p.sample(N, seed=1)
            xs = x.T[torch.randperm(N, device=x.device)].contiguous()          # (N, D) float32, the clusters mixed
            del x
            torch.cuda.empty_cache()
            data = xs.T
            r = {"N": N, "D": D, "K": K}
            for name, fn in (("floor", lambda: p.predict_labels(data)), ("composition_soft", lambda: composition_soft(p, data)),
                             ("composition_hard", lambda: composition_hard(p, data)), ("hard", lambda: p.statistics(data, assign="hard")),
                             ("soft", lambda: p.statistics(data, assign="soft"))):
                note(f"D = {D}: {name}")
                r[name] = median_ms(fn)
            soft, hard = p.statistics(data, assign="soft"), p.statistics(data, assign="hard")
            bound = 2 * (N + 2) * 2.0 ** -53
            T = composition_soft(p, data, absolute=True)
            r["soft_max_diff_in_bounds"] = float((np.abs(soft.S - composition_soft(p, data)) / (bound * np.maximum(T, 1e-300))).max())
            r["hard_max_rel_diff"] = float(np.abs(hard.S - composition_hard(p, data)).max() / np.abs(hard.S).max())
            r["skipped"] = hard.skipped
            nnz = {"hard": float(hard.count.sum()), "soft": float((p.predict(data)[1] > 0).sum().item())}
            for mode in ("hard", "soft"):
                r[mode]["over_floor"] = r[mode]["ms"] / r["floor"]["ms"]
                r[mode]["over_composition"] = r[mode]["ms"] / r["composition_" + mode]["ms"]
                ms = max(r[mode]["ms"] - r["floor"]["ms"], 1e-6)
                flops = nnz[mode] * D * (D + 1)
                r[mode]["added"] = {"ms": ms, "nonzero_weights": nnz[mode], "tflops": flops / ms / 1e9, "share_of_f64_matrix_peak": flops / (ms * 1e-3) / F64_MATRIX_PEAK}
            out[f"D{D}"] = r
            del xs, data
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
