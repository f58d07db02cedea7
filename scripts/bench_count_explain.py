#!/usr/bin/env python3
"""Times Predictor.explain_counts (host/score.py, csrc/count_explain.hip) at the two shapes DESIGN quotes, and prints one JSON line.

  dense    D = 1000, N = 1e6 small integer counts, a Float32 device tensor that the worker keeps as bytes, K = 32, top = 10
  sparse   D = 20000, N = 1e6, 100 entries per point (1e8 in all), a torch.sparse_csc tensor on the device, K = 32, top = 10

On the same data, in the same process, the calls interleaved (floor, recommend, composition, explain_counts, floor, ...):
  floor          Predictor.predict_labels alone: explain_counts cannot avoid evaluating that table
  recommend      Predictor.recommend(data, top): the same walk with a matrix chain in place of the deviances
  composition    what a user of torch has to do today: predict_labels, then in chunks of points whose (rows, D) Float64 block stays within
                 --chunk-mb: the dense deviance from theta[labels] (sparse data: the chunk densified by index_put_), topk of |residual|,
                 and the tails of the N top winners by scipy.special.betainc / betaincc on the host.  Its peak extra device memory
                 (torch.cuda.max_memory_allocated over the call) is reported.
  explain        Predictor.explain_counts(data, top)
Every figure is the median (and the minimum) of --reps calls after one warm-up call, timed from the host around the call; every call ends
synchronised.  The spread of the floor within the run (max / min) says how far to trust a ratio.  --scale shrinks N (a quick check of the
script itself)."""
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
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--chunk-mb", type=int, default=512)
    ap.add_argument("--shapes", default="dense,sparse")
    a = ap.parse_args()
    import scipy.special as ss
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale, "top": a.top}

    def note(msg):
        print("[bench_count_explain] " + msg, file=sys.stderr, flush=True)

    def predictor(D, K, N, seed):
        rng = np.random.default_rng(seed)
        alpha = rng.gamma(0.3, 1.0, (K, D)).astype(np.float32) + np.float32(0.05)
        p = score.Predictor.__new__(score.Predictor)
        p._setup(1, D, 10.0, np.full(K, 100.0), dict(alpha=alpha), N, 0, None)
        return p

    N, K, top = int(1e6 * a.scale), a.K, a.top
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
        th64 = a64 / a64.sum(1, keepdims=True)
        lth, l1m = torch.from_numpy(np.log(th64)).to(dev), torch.from_numpy(np.log1p(-th64)).to(dev)
        rows = max(1, (a.chunk_mb << 20) // (8 * D))

        def composition():
            lab = p.predict_labels(data) - 1
            feats = torch.empty((N, top), dtype=torch.int64, device=dev)
            res = torch.empty((N, top), dtype=torch.float32, device=dev)
            cnt = torch.empty((N, top), dtype=torch.float64, device=dev)
            tot = torch.empty(N, dtype=torch.float64, device=dev)
            for lo in range(0, N, rows):
                hi = min(N, lo + rows)
                if shape == "dense":
                    x = xs[lo:hi].double()
                else:
                    e0, e1 = lo * per, hi * per
                    x = torch.zeros((hi - lo, D), dtype=torch.float64, device=dev)
                    x.index_put_((torch.arange(lo, hi, device=dev).repeat_interleave(per) - lo, rowval[e0:e1]), nzval[e0:e1].double())
                t = x.sum(1, keepdim=True)
                y = t - x
                gdev = 2 * (torch.xlogy(x, x / t) - x * lth[lab[lo:hi]] + torch.xlogy(y, y / t) - y * l1m[lab[lo:hi]])
                r = torch.sqrt(gdev.clamp_(min=0))
                v, f = torch.topk(r, top, dim=1)
                feats[lo:hi], cnt[lo:hi], tot[lo:hi] = f, torch.gather(x, 1, f), t[:, 0]
                res[lo:hi] = v.float()
            f, c, t, k = feats.cpu().numpy(), cnt.cpu().numpy(), tot.cpu().numpy()[:, None], lab.cpu().numpy()[:, None]
            th = th64[k, f]
            with np.errstate(all="ignore"):
                tail = np.where(c > t * th, ss.betainc(np.maximum(c, 1e-300), t - c + 1, th), ss.betaincc(c + 1, np.maximum(t - c, 1e-300), th))
            return feats, res, tail

        calls = {"floor": lambda: p.predict_labels(data), "recommend": lambda: p.recommend(data, top), "composition": composition,
                 "explain": lambda: p.explain_counts(data, top)}
        torch.cuda.synchronize()
        r = {"N": N, "D": D, "K": K, "composition_chunk_rows": rows}
        times = {name: [] for name in calls}
        for name, fn in calls.items():                      # the warm-up, and the peak memory
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
            r[name] = {"ms": float(np.median(ts)), "best_ms": float(min(ts)), "worst_ms": float(max(ts))}
        r["floor"]["spread"] = r["floor"]["worst_ms"] / r["floor"]["best_ms"]
        got = p.explain_counts(data, top)
        ref_f, ref_r, ref_t = composition()
        for other in ("floor", "recommend", "composition"):
            r["explain"]["over_" + other] = r["explain"]["ms"] / r[other]["ms"]
        r["explain"]["first_feature_agrees_with_composition"] = float((got.features[:, 0].long() == ref_f[:, 0]).float().mean())
        r["explain"]["max_rel_diff_of_first_tail"] = float(np.nanmax(np.abs(got.feature_tail[:, 0].cpu().numpy() - ref_t[:, 0]) / np.maximum(ref_t[:, 0], 1e-30)))
        r["explain"]["skipped"], r["explain"]["incomplete"] = got.skipped, got.incomplete
        out[shape] = r
        p.close()
        del data, got, ref_f, ref_r, ref_t
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
