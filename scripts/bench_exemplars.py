#!/usr/bin/env python3
"""Times Predictor.exemplars (host/score.py, csrc/rank.hip) with m = 16 at the two shapes DESIGN section 16 quotes, and prints one JSON line.

  niw      N = 1e7, D = 64, K = 32, a bfloat16 device tensor (the `.T` view of (N, D) memory)
  sparse   the sparse Multinomial shape of DESIGN section 14: D = 20000, N = 1e6, about 100 entries per point, a torch.sparse_csc tensor

On the same data, in the same process:
  floor         Predictor.predict_labels alone: the ranking cannot avoid evaluating that table
  composition   what could be done before: predict_labels + score_samples, then a torch sort by (label, score) and a gather of the first
                m of every cluster -- two n-sized results, an n-sized sort, and the mixture density where the cluster's own is meant
  exemplars     both lists
  adversarial   exemplars on the data permuted by ascending score (score_samples): nearly every point beats the running threshold of
                its typical list
The data are drawn by Predictor.sample from the model they are scored with.  Every figure is the median (and the minimum) of --reps calls
after one warm-up call, timed from the host around the call; every call ends synchronised (the results are read or torch.cuda.synchronize
is called).  --scale shrinks every N (a quick check of the script itself)."""
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

M = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="niw,sparse")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale, "m": M}

    def note(msg):
        print("[bench_exemplars] " + msg, file=sys.stderr, flush=True)

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

    def composition(p, data, K):
        lab = p.predict_labels(data)
        s = p.score_samples(data)
        res = []
        for sign in (-1.0, 1.0):                                   # typical, fringe: a stable sort by score, then by label
            o1 = torch.sort(sign * s, stable=True).indices
            o2 = torch.sort(lab[o1], stable=True)
            order = o1[o2.indices]
            start = torch.searchsorted(o2.values, torch.arange(1, K + 1, device=lab.device))
            pos = torch.clamp(start[:, None] + torch.arange(M, device=lab.device)[None, :], max=lab.numel() - 1)
            res.append(order[pos])
        return res

    def measure(name, p, data, K, permute):
        r = {}
        note(name + ": floor")
        r["floor"] = median_ms(lambda: p.predict_labels(data))
        note(name + ": composition")
        r["composition"] = median_ms(lambda: composition(p, data, K))
        note(name + ": exemplars")
        r["exemplars"] = median_ms(lambda: p.exemplars(data, M))
        ex = p.exemplars(data, M)
        r["count_min"], r["skipped"] = int(ex.count.min()), ex.skipped
        note(name + ": adversarial order")
        # (the order is that of score_samples, the mixture's log-density: the n-sized score there is; it differs from the own cluster's
        # score by the other clusters' share, which between separated clusters is small, so nearly every point beats its threshold)
        s = p.score_samples(data)
        data_up = permute(data, torch.sort(s, stable=True).indices)
        del s
        torch.cuda.synchronize()
        r["adversarial"] = median_ms(lambda: p.exemplars(data_up, M))
        for k in ("composition", "exemplars", "adversarial"):
            r[k]["over_floor"] = r[k]["ms"] / r["floor"]["ms"]
        r["exemplars"]["over_composition"] = r["exemplars"]["ms"] / r["composition"]["ms"]
        r["adversarial"]["over_composition"] = r["adversarial"]["ms"] / r["composition"]["ms"]
        return r

    only = a.only.split(",")
    if "niw" in only:
        N, D, K = int(1e7 * a.scale), 64, 32
        post, _, _, _ = R.niw_model(D, K, 60.0, 1)
        with score.Predictor.load(R.predictor_file(0, D, 1.0, np.full(K, 100.0), post), capacity=1 << 20) as p:
            note("niw: drawing the data")
            x, _ = p.sample(N, seed=1)
            xb = x.T.to(torch.bfloat16)[torch.randperm(N, device=x.device)]          # (N, D) bfloat16, the clusters mixed
            del x
            torch.cuda.empty_cache()
            out["niw"] = dict(N=N, D=D, K=K, **measure("niw", p, xb.T, K, lambda d, o: d.T[o].T))
            del xb
        torch.cuda.empty_cache()
    if "sparse" in only:
        N, D, K, trials = int(1e6 * a.scale), 20000, 8, 100
        alpha = np.random.default_rng(2).dirichlet(np.full(D, 0.1), K) * 1e4 + 1e-3
        with score.Predictor.load(R.predictor_file(1, D, 1.0, np.full(K, 100.0), dict(alpha=alpha)), capacity=1 << 18) as p:
            note("sparse: drawing the data")
            x, _ = p.sample(N, seed=1, trials=trials, sparse=True)

            def permute(d, o):                                     # the columns of a sparse_csc tensor in another order
                cp, ri, v = d.ccol_indices(), d.row_indices(), d.values()
                cnt = (cp[1:] - cp[:-1])[o]
                ncp = torch.zeros_like(cp)
                ncp[1:] = torch.cumsum(cnt, 0)
                src = torch.repeat_interleave(cp[:-1][o] - ncp[:-1], cnt) + torch.arange(ri.numel(), device=ri.device)
                return torch.sparse_csc_tensor(ncp, ri[src], v[src], size=d.shape)

            x = permute(x, torch.randperm(N, device=x.device))     # the clusters mixed
            out["sparse"] = dict(N=N, D=D, K=K, nnz=int(x.values().numel()), **measure("sparse", p, x, K, permute))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
