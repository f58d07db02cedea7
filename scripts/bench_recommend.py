#!/usr/bin/env python3
"""Times Predictor.recommend (host/score.py, csrc/recommend.hip) at the two shapes DESIGN quotes, and prints one JSON line.

  dense    D = 1000, N = 1e6 small integer counts, a Float32 device tensor that the worker keeps as bytes, K = 32, m = 10
  sparse   D = 20000, N = 1e6, 100 entries per point (1e8 in all), a torch.sparse_csc tensor on the device, K = 32, m = 10

On the same data, in the same process, the calls interleaved (floor, composition, recommend, floor, ...):
  floor          Predictor.predict_labels alone: recommend cannot avoid evaluating that table
  composition    what a user of torch has to do today: predict, then in chunks of points whose (rows, D) Float32 block stays within
                 --chunk-mb: P @ theta, the features the point holds set to -inf (dense: from the rows; sparse: an index_put_ of the
                 chunk's entries), topk.  Its peak extra memory (torch.cuda.max_memory_allocated over the call) is reported.
  recommend      Predictor.recommend(data, m)
Every figure is the median (and the minimum) of --reps calls after one warm-up call, timed from the host around the call; every call ends
synchronised.  added_ms = recommend - floor, and the share of the FP32 matrix peak (--peak-tflops, 157.3 for the MI355X) that 2 N D K flop
in added_ms amount to.  --scale shrinks N (a quick check of the script itself)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--chunk-mb", type=int, default=512)
    ap.add_argument("--peak-tflops", type=float, default=157.3)
    ap.add_argument("--shapes", default="dense,sparse")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale, "m": a.m}

    def note(msg):
        print("[bench_recommend] " + msg, file=sys.stderr, flush=True)

    def predictor(D, K, N, seed):
        rng = np.random.default_rng(seed)
        alpha = rng.gamma(0.3, 1.0, (K, D)).astype(np.float32) + np.float32(0.05)
        p = score.Predictor.__new__(score.Predictor)
        p._setup(1, D, 10.0, np.full(K, 100.0), dict(alpha=alpha), N, 0, None)
        return p

    N, K, m = int(1e6 * a.scale), a.K, a.m
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for shape in a.shapes.split(","):
        if shape == "dense":
            D = 1000
            p = predictor(D, K, N, 2)
            xs = torch.poisson(torch.full((N, D), 0.3, device=dev), generator=g)          # (N, D) float32 counts
            data = xs.T
        else:
            D, per = 20000, 100
            p = predictor(D, K, N, 3)
            step = D // per
            rowval = ((torch.arange(per, device=dev) * step)[None, :] + torch.randint(0, step, (N, per), device=dev, generator=g)).reshape(-1)      # sorted, distinct
            nzval = torch.randint(1, 5, (N * per,), device=dev, generator=g).float()
            colptr = torch.arange(N + 1, device=dev, dtype=torch.int64) * per
            data = torch.sparse_csc_tensor(colptr, rowval, nzval, size=(D, N))
        a64 = np.asarray(p.post["alpha"], np.float64)
        theta = torch.from_numpy((a64 / a64.sum(1, keepdims=True)).astype(np.float32)).to(dev)
        rows = max(1, (a.chunk_mb << 20) // (4 * D))

        def composition():
            _, P = p.predict(data)
            feats = torch.empty((N, m), dtype=torch.int64, device=dev)
            prob = torch.empty((N, m), dtype=torch.float32, device=dev)
            for lo in range(0, N, rows):
                hi = min(N, lo + rows)
                r = P[lo:hi] @ theta
                if shape == "dense":
                    r.masked_fill_(xs[lo:hi] != 0, float("-inf"))
                else:
                    e0, e1 = lo * per, hi * per
                    col = torch.arange(lo, hi, device=dev).repeat_interleave(per) - lo
                    r.index_put_((col, rowval[e0:e1]), torch.tensor(float("-inf"), device=dev))
                prob[lo:hi], feats[lo:hi] = torch.topk(r, m, dim=1)
            return feats, prob

        calls = {"floor": lambda: p.predict_labels(data), "composition": composition, "recommend": lambda: p.recommend(data, m)}
        torch.cuda.synchronize()
        r = {"N": N, "D": D, "K": K, "composition_chunk_rows": rows}
        times = {name: [] for name in calls}
        for name, fn in calls.items():                      # the warm-up, and the composition's peak memory
            note(f"{shape}: warm-up {name}")
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            r.setdefault("peak_extra_mb", {})[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        for rep in range(a.reps):
            for name, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name, ts in times.items():
            r[name] = {"ms": float(np.median(ts)), "best_ms": float(min(ts))}
        got = p.recommend(data, m)
        ref_f, ref_p = composition()
        r["recommend"]["over_floor"] = r["recommend"]["ms"] / r["floor"]["ms"]
        r["recommend"]["over_composition"] = r["recommend"]["ms"] / r["composition"]["ms"]
        added = r["recommend"]["ms"] - r["floor"]["ms"]
        r["recommend"]["added_ms"] = added
        r["recommend"]["share_of_fp32_matrix_peak"] = (2.0 * N * D * K / (added * 1e-3)) / (a.peak_tflops * 1e12) if added > 0 else None
        r["recommend"]["first_feature_agrees_with_composition"] = float((got.features[:, 0].long() == ref_f[:, 0]).float().mean())
        r["recommend"]["max_rel_diff_of_first_prob"] = float(((got.prob[:, 0] - ref_p[:, 0]).abs() / ref_p[:, 0]).max())
        r["recommend"]["skipped"] = got.skipped
        out[shape] = r
        p.close()
        del data, got, ref_f, ref_p
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
