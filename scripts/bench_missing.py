#!/usr/bin/env python3
"""Times Predictor.score_samples with missing="marginalize" (host/score.py, csrc/missing.hip) at the shape DESIGN section 18 quotes, and
prints one JSON line.

  N = 1e6, D = 64, K = 32, a Float32 device tensor (the `.T` view of (N, D) memory), drawn by Predictor.sample from the model it is scored with

  share 0 %, 1 %, 10 %   of the points get 1 - 4 NaN features at random places
  propagate              score_samples on the same data with missing="propagate": the floor (NaN rows cost what complete rows cost)
  marginalize            score_samples with missing="marginalize"; at 0 % this is the price of the option on complete data
  impute                 Predictor.impute on the same data
The floor of the 0 % data is timed `--rounds` times over (a median of --reps calls each, after one warm-up call): the spread of those
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
        print("[bench_missing] " + msg, file=sys.stderr, flush=True)

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
    with score.Predictor.load(path, capacity=1 << 20) as prop, score.Predictor.load(path, capacity=1 << 20, missing="marginalize") as marg:
        note("drawing the data")
        x, _ = prop.sample(N, seed=1)
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
            if share == 0.0:
                floors = [median_ms(lambda: prop.score_samples(data)) for _ in range(a.rounds)]
                margs = [median_ms(lambda: marg.score_samples(data)) for _ in range(a.rounds)]
                res["propagate_rounds_ms"], res["marginalize_rounds_ms"] = floors, margs
                res["propagate_ms"], res["marginalize_ms"] = float(np.median(floors)), float(np.median(margs))
                res["propagate_spread_ms"] = float(max(floors) - min(floors))
            else:
                res["propagate_ms"] = median_ms(lambda: prop.score_samples(data))
                res["marginalize_ms"] = median_ms(lambda: marg.score_samples(data))
            res["missing_counts"] = list(marg.missing_counts)
            res["impute_ms"] = median_ms(lambda: marg.impute(data))
            res["marginalize_over_propagate"] = res["marginalize_ms"] / res["propagate_ms"]
            out[key] = res
            del xs, data
    print(json.dumps(out))


if __name__ == "__main__":
    main()
