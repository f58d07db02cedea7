#!/usr/bin/env python3
"""Times Predictor.held_out_counts (host/score.py, csrc/holdout.hip) and prints one JSON line.

  N = 1e6, K = 32, 0.1 %, 1 % and 10 % of the documents novel (all their counts on features every cluster gives little mass):
    dense    D = 1000, small integer counts on the device as Float32: the worker keeps its lossless byte copy
    sparse   D = 20000, about 100 stored entries per document, a torch.sparse_csc tensor on the device

On the same data, in the same process, with the same floor per count:
  floor          Predictor.count_statistics(min_logdens_per_count=f): the same walk over the table and the same totals, plus the sums
  held_out       Predictor.held_out_counts(min_logdens_per_count=f)
  composition    what a user could write before: Predictor.score_samples -> column totals -> a mask -> nonzero -> index_select of the rows
                 (dense) or offset arithmetic and a gather of the entries (sparse), all in torch on the device
Every figure is the median, the minimum and the maximum of --reps calls after one warm-up call, timed from the host around the call; every
call ends synchronised.  --scale shrinks N (a quick check of the script itself)."""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--fractions", default="0.001,0.01,0.1")
    ap.add_argument("--cases", default="dense,sparse")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale}

    def note(msg):
        print("[bench_count_holdout] " + msg, file=sys.stderr, flush=True)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": float(np.median(ts)), "best_ms": float(min(ts)), "worst_ms": float(max(ts))}

    def model(D, K, novel):
        """K topics of 16 preferred features each; the last `novel` features get the least mass from every topic."""
        rng = np.random.default_rng(1)
        alpha = np.full((K, D), 0.25)
        for k in range(K):
            alpha[k, rng.choice(D - novel, 16, replace=False)] = 8.0
        p = score.Predictor.__new__(score.Predictor)
        p._setup(1, D, 10.0, np.full(K, 100.0), dict(alpha=alpha.astype(np.float32)), N, 0, None)
        # a novel document lies at log(0.25 / sum alpha) per count or below; an ordinary one far above
        return p, float(np.log(0.25 / alpha.sum(1)).max() + 0.5)

    def dense_composition(p, data, f):
        ld = p.score_samples(data)
        t = data.sum(0, dtype=torch.float64)
        idx = torch.nonzero((t > 0) & (ld.double() < f * t)).squeeze(1)
        return torch.index_select(data.T, 0, idx), idx

    def sparse_composition(p, data, f):
        ld = p.score_samples(data)
        cp, rows, vals = data.ccol_indices(), data.row_indices(), data.values()
        lens = cp[1:] - cp[:-1]
        col = torch.repeat_interleave(torch.arange(lens.numel(), device=dev), lens)
        t = torch.zeros(lens.numel(), dtype=torch.float64, device=dev).index_add_(0, col, vals.double())
        idx = torch.nonzero((t > 0) & (ld.double() < f * t)).squeeze(1)
        hl = lens[idx]
        ncp = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(hl, 0)])
        src = torch.repeat_interleave(cp[:-1][idx] - ncp[:-1], hl) + torch.arange(int(ncp[-1]), device=dev)
        return ncp, rows[src], vals[src], idx

    N, K = int(1e6 * a.scale), a.K
    for case in a.cases.split(","):
        D, trials, novel = (1000, 200, 8) if case == "dense" else (20000, 100, 64)
        p, f = model(D, K, novel)
        with p:
            note(f"{case}: drawing the data")
            x, _ = p.sample(N, seed=1, trials=trials, sparse=case == "sparse")
            perm = torch.randperm(N, device=dev)
            out[case] = r = {"N": N, "D": D, "K": K, "floor_per_count": f}
            for frac in (float(v) for v in a.fractions.split(",")):
                m = int(round(frac * N))
                g = torch.Generator(device=dev).manual_seed(int(frac * 1e6))
                if case == "dense":
                    ys = x.T[perm].contiguous()
                    moved = torch.randperm(N, device=dev, generator=g)[:m]
                    ys[moved] = 0
                    ys[moved, D - novel:] = float(trials // novel)
                    data = ys.T
                    comp = lambda: dense_composition(p, data, f)      # noqa: E731
                else:                                                 # the novel documents replace the last m columns, then nothing is permuted:
                    cp, rows, vals = x.ccol_indices(), x.row_indices(), x.values()      # a CSC permutation is itself a gather of entries
                    keep = int(cp[N - m])
                    nrows = (D - novel + torch.arange(novel, device=dev)).repeat(m)
                    ncp = torch.cat([cp[:N - m + 1], keep + novel * torch.arange(1, m + 1, device=dev)])
                    data = torch.sparse_csc_tensor(ncp, torch.cat([rows[:keep], nrows]), torch.cat([vals[:keep], torch.full((m * novel,), 2.0, device=dev)]),
                                                   size=(D, N))
                    comp = lambda: sparse_composition(p, data, f)     # noqa: E731
                c = {}
                for name, fn in (("floor", lambda: p.count_statistics(data, min_logdens_per_count=f)),
                                 ("held_out", lambda: p.held_out_counts(data, min_logdens_per_count=f, max_points=N, max_entries=1 << 30)),
                                 ("composition", comp)):
                    note(f"{case} {frac:g}: {name}")
                    c[name] = timed(fn)
                h = p.held_out_counts(data, min_logdens_per_count=f, max_points=N, max_entries=1 << 30)
                ref = comp()
                c["total"], c["novel"], c["total_entries"] = h.total, m, h.total_entries
                if case == "dense":
                    c["same_as_composition"] = bool(torch.equal(h.index, ref[1]) and torch.equal(h.points.T, ref[0]))
                else:
                    c["same_as_composition"] = bool(torch.equal(h.index, ref[3]) and torch.equal(h.points.ccol_indices().long(), ref[0])
                                                    and torch.equal(h.points.row_indices().long(), ref[1].long()) and torch.equal(h.points.values(), ref[2]))
                c["held_out"]["over_floor"] = c["held_out"]["ms"] / c["floor"]["ms"]
                c["held_out"]["over_composition"] = c["held_out"]["ms"] / c["composition"]["ms"]
                c["floor"]["spread"] = (c["floor"]["worst_ms"] - c["floor"]["best_ms"]) / c["floor"]["ms"]
                r[f"{frac:g}"] = c
                del data, ref, h
                torch.cuda.empty_cache()
            del x
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
