#!/usr/bin/env python3
"""Times Regressor.predict (host/score.py, csrc/regress.hip) at the shapes DESIGN section 29 quotes, and prints one JSON line.

  N = 1e6, K = 32, a Float32 device tensor (the `.T` view of (N, D_o) memory) drawn by the marginal Predictor's own sampler;
  (D_o, D_t) = (32, 32) and (128, 128), and (48, 16) for the comparison with `impute`

  labels        marginal.predict_labels alone: the floor that shares the table walk
  regress       Regressor.predict(data), and with return_std=True
  torch         the composition a user needed before: marginal.predict (the (n, K) probabilities) plus a chunked einsum over Float32 B,
                with its peak extra memory (torch.cuda.max_memory_allocated above the resting level)
  impute        D_t <= 16: Predictor.impute on the same points with the targets set to NaN
Medians of --reps calls after one warm-up call each, the calls interleaved round by round.  Every call ends synchronised.  --scale shrinks N."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    N, K = int(1e6 * a.scale), 32
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "N": N, "K": K}

    def note(msg):
        print("[bench_regress] " + msg, file=sys.stderr, flush=True)

    def interleaved_ms(fns):
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        return {k + "_ms": float(np.median(v)) for k, v in ts.items()}

    for Do, Dt in ((32, 32), (128, 128), (48, 16)):
        D = Do + Dt
        note(f"D_o = {Do}, D_t = {Dt}")
        post, _, _, _ = R.niw_model(D, K, 60.0, 1)
        path = R.predictor_file(0, D, 1.0, np.full(K, 100.0), post)
        given, targets = list(range(Do)), list(range(Do, D))
        with score.Predictor.load(path, capacity=1 << 20) as parent, parent.regressor(given, targets) as reg:
            mg = reg.marginal
            x, _ = mg.sample(N, seed=1)
            x = x.T[torch.randperm(N, device=x.device)].contiguous()               # (N, D_o) Float32, the clusters mixed
            data = x.T
            B, c, _, _, _ = reg.tables()
            Bf = torch.as_tensor(B, dtype=torch.float32, device=x.device)
            cf = torch.as_tensor(c, dtype=torch.float32, device=x.device)
            chunk = 1 << 16

            def composed():
                _, p = mg.predict(data)
                mean = torch.empty((N, Dt), dtype=torch.float32, device=x.device)
                for lo in range(0, N, chunk):
                    mu = torch.einsum("kde,ne->nkd", Bf, x[lo:lo + chunk]) + cf[None]
                    mean[lo:lo + chunk] = torch.einsum("nk,nkd->nd", p[lo:lo + chunk], mu)
                return mean

            fns = {"labels": lambda: mg.predict_labels(data), "regress": lambda: reg.predict(data),
                   "regress_std": lambda: reg.predict(data, return_std=True), "torch": composed}
            if Dt <= 16:
                full = torch.full((N, D), float("nan"), dtype=torch.float32, device=x.device)
                full[:, :Do] = x
                fns["impute"] = lambda: parent.impute(full.T)
            res = interleaved_ms(fns)
            torch.cuda.synchronize()
            rest = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ref = composed()
            torch.cuda.synchronize()
            res["torch_peak_extra_mb"] = (torch.cuda.max_memory_allocated() - rest) / 2 ** 20
            got = reg.predict(data).mean.T
            res["max_abs_diff_to_torch"] = float((got - ref).abs().max())
            res["regress_over_labels"] = res["regress_ms"] / res["labels_ms"]
            res["torch_over_regress"] = res["torch_ms"] / res["regress_ms"]
            out[f"{Do}x{Dt}"] = res
            del x, data, ref, got
    print(json.dumps(out))


if __name__ == "__main__":
    main()
