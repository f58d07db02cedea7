#!/usr/bin/env python3
"""Times Predictor.sample (host/score.py, csrc/sample.hip) at the three shapes DESIGN section 15 quotes, and prints one JSON line.

  niw           N = 1e7, D = 64, K = 32       time, write rate on 4 D N bytes, and the same bytes written by a plain fill of the output
                                              (torch's fill_ kernel, timed in the same run): the yardstick of "write-bound"
  mult_dense    N = 1e6, D = 1000, trials = 1000
  mult_sparse   N = 1e6, D = 20000, trials = 100
  --host        also the cost of what a user had to do before: generate_gaussian_data / generate_mnmm_data on the host plus the upload
                (another law -- a random mixture, not a fitted one: a comparison of cost only)

Every figure is the median of --reps calls after one warm-up call; a call is timed from the host around p.sample (which returns after the
library has synchronised its stream), the fill with torch events.  --scale shrinks every N (a quick check of the script itself)."""
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


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--only", default="niw,mult_dense,mult_sparse")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    host = importlib.import_module(pkg.__name__ + ".host")
    from tools import sample_ref as R
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale}
    only = a.only.split(",")

    def note(msg):
        print("[bench_sample] " + msg, file=sys.stderr, flush=True)

    if "niw" in only:
        note("niw")
        N, D, K = int(1e7 * a.scale), 64, 32
        post, _, _, _ = R.niw_model(D, K, 60.0, 1)
        with score.Predictor.load(R.predictor_file(0, D, 1.0, np.full(K, 100.0), post), capacity=1 << 20) as p:
            med, best = median_ms(lambda: p.sample(N, seed=1), a.reps)
            x, _ = p.sample(N, seed=1)
        buf = x.T                                                     # the (N, D) memory the kernel wrote
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        fills = []
        for _ in range(a.reps + 1):
            ev[0].record(); buf.fill_(1.0); ev[1].record(); torch.cuda.synchronize()
            fills.append(ev[0].elapsed_time(ev[1]))
        fill = float(np.median(fills[1:]))
        nbytes = 4.0 * D * N
        out["niw"] = {"N": N, "D": D, "K": K, "ms": med, "best_ms": best, "write_GBps": nbytes / med / 1e6, "fill_ms": fill,
                      "fill_GBps": nbytes / fill / 1e6, "fraction_of_fill_rate": fill / med}
        del x, buf
        if a.host:
            note("niw: host generator + upload")
            t0 = time.perf_counter()
            hx = host.generate_gaussian_data(N, D, K, 80.0, seed=1)[0]
            t1 = time.perf_counter()
            torch.as_tensor(hx).to("cuda:0"); torch.cuda.synchronize()
            out["niw"]["host_generate_ms"], out["niw"]["host_upload_ms"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
            del hx
    for name, N, D, trials, sparse in (("mult_dense", 1e6, 1000, 1000, False), ("mult_sparse", 1e6, 20000, 100, True)):
        if name not in only:
            continue
        note(name)
        N, K = int(N * a.scale), 8
        alpha = np.random.default_rng(2).dirichlet(np.full(D, 0.1), K) * 1e4 + 1e-3
        with score.Predictor.load(R.predictor_file(1, D, 1.0, np.full(K, 100.0), dict(alpha=alpha)), capacity=1 << 18) as p:
            med, best = median_ms(lambda: p.sample(N, seed=1, trials=trials, sparse=sparse), a.reps)
            x, _ = p.sample(N, seed=1, trials=trials, sparse=sparse)
        out[name] = {"N": N, "D": D, "K": K, "trials": trials, "ms": med, "best_ms": best}
        if sparse:
            out[name]["nnz"] = int(x.values().numel())
        del x
        torch.cuda.empty_cache()
        if a.host:
            note(name + ": host generator + upload")
            t0 = time.perf_counter()
            hx = host.generate_mnmm_data(N, D, K, trials, seed=1, sparse=sparse)[0]
            t1 = time.perf_counter()
            for part in (hx[:3] if sparse else (hx,)):
                torch.as_tensor(part).to("cuda:0")
            torch.cuda.synchronize()
            out[name]["host_generate_ms"], out[name]["host_upload_ms"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
            del hx
    print(json.dumps(out))


if __name__ == "__main__":
    main()
