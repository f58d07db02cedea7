#!/usr/bin/env python3
"""Times Predictor.impute(data, draws=m) (host/score.py, miss_draw_kernel of csrc/missing.hip) at the shape DESIGN section 21 quotes, and
prints one JSON line.

  N = 1e6, D = 64, K = 32, a Float32 device tensor (the `.T` view of (N, D) memory), drawn by Predictor.sample from the model it is imputed with

  share 0 %, 1 %, 10 %   of the points get 1 - 4 NaN features at random places
  impute                 Predictor.impute(data): the mean imputation, the floor for the table and the copy (K systems per gapped point)
  draws m = 1, 5, 20     Predictor.impute(data, draws=m): one table, m copies, one system per (gapped point, draw)
  m x impute             m separate impute calls: what m completed copies cost without the draws
The impute of the 0 % data is timed `--rounds` times over (a median of --reps calls each, after one warm-up call): the spread of those
medians is the run-to-run noise that the other figures have to be read against.  Every call ends synchronised.  --scale shrinks N."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    N, D, K = int(1e6 * a.scale), 64, 32
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "N": N, "D": D, "K": K}

    def note(msg):
        print("[bench_impute_draws] " + msg, file=sys.stderr, flush=True)

    def median_ms(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    post, _, _, _ = R.niw_model(D, K, 60.0, 1)
    path = R.predictor_file(0, D, 1.0, np.full(K, 100.0), post)
    with score.Predictor.load(path, capacity=max(1, N // 4)) as p:                    # four full slabs: results are written where they stay
        note("drawing the data")
        x, _ = p.sample(N, seed=1)
        x = x.T[torch.randperm(N, device=x.device)].contiguous()                   # (N, D) Float32, the clusters mixed
        g = torch.Generator(device=x.device).manual_seed(7)
        for share in (0.0, 0.01, 0.10):
            xs = x.clone()
            pts = torch.nonzero(torch.rand(N, device=x.device, generator=g) < share)[:, 0]
            r = torch.randint(1, 5, (pts.numel(),), device=x.device, generator=g)
            for j in range(4):                                                     # up to four places per point (a repeated place: one gap fewer)
                sel = pts[r > j]
                xs[sel, torch.randint(0, D, (sel.numel(),), device=x.device, generator=g)] = float("nan")
            data = xs.T
            torch.cuda.synchronize()
            key = "%g%%" % (100 * share)
            note(key)
            res = {}
            rounds = [median_ms(lambda: p.impute(data)) for _ in range(a.rounds if share == 0.0 else 1)]
            res["impute_ms"] = float(np.median(rounds))
            if share == 0.0:
                res["impute_rounds_ms"], res["impute_spread_ms"] = rounds, float(max(rounds) - min(rounds))
            res["missing_counts"] = list(p.missing_counts)
            for m in (1, 5, 20):
                res[f"draws_{m}_ms"] = median_ms(lambda: p.impute(data, draws=m, seed=3))
                res[f"{m}_x_impute_ms"] = res["impute_ms"] if m == 1 else median_ms(lambda: [p.impute(data) for _ in range(m)])
            out[key] = res
            del xs, data
    print(json.dumps(out))


if __name__ == "__main__":
    main()
