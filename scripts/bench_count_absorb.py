#!/usr/bin/env python3
"""Times Predictor.count_statistics (host/score.py, csrc/countstats.hip) at the two shapes DESIGN quotes, and prints one JSON line.

  sparse   D = 20000, N = 1e6, 100 entries per point (1e8 in all), a torch.sparse_csc tensor on the device, K = 32
  dense    D = 1000, N = 1e6 small integer counts, a Float32 device tensor that the worker keeps as bytes, K = 32

On the same data, in the same process:
  floor          Predictor.predict_labels alone: the statistics cannot avoid evaluating that table
  composition    what a user of torch could do before, in Float64:
                 dense   hard: predict_labels, then index_add_ of the rows, in chunks whose Float64 copy stays within 512 MB;
                         soft: predict, then P' X by matmul over the same chunks
                 sparse  hard: predict_labels, then one index_add_ over the stored entries into the flat (K D) result -- the entries'
                         point indices come from repeat_interleave over the column lengths; nothing is densified;
                         soft: predict, then torch.sparse.mm of the CSC tensor with P in Float64 -- reported as unsupported, with the
                         error, if this torch build cannot do it
  hard, soft     Predictor.count_statistics(assign=...)
and the sums of the two routes compared.  Every figure is the median (and the minimum) of --reps calls after one warm-up call, timed
from the host around the call; every call ends synchronised.  --scale shrinks N (a quick check of the script itself)."""
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
    ap.add_argument("--shapes", default="sparse,dense")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale}

    def note(msg):
        print("[bench_count_absorb] " + msg, file=sys.stderr, flush=True)

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

    def predictor(D, K, N, seed):
        rng = np.random.default_rng(seed)
        alpha = rng.gamma(0.3, 1.0, (K, D)).astype(np.float32) + np.float32(0.05)
        p = score.Predictor.__new__(score.Predictor)
        p._setup(1, D, 10.0, np.full(K, 100.0), dict(alpha=alpha), N, 0, None)
        return p

    N, K = int(1e6 * a.scale), a.K
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for shape in a.shapes.split(","):
        if shape == "dense":
            D = 1000
            p = predictor(D, K, N, 2)
            xs = torch.poisson(torch.full((N, D), 0.3, device=dev), generator=g)          # (N, D) float32 counts
            data = xs.T
            rows = max(1, (1 << 29) // (8 * D))

            def comp_hard():
                lab = p.predict_labels(data)
                S = torch.zeros((K, D), dtype=torch.float64, device=dev)
                for lo in range(0, N, rows):
                    S.index_add_(0, lab[lo:lo + rows] - 1, xs[lo:lo + rows].double())
                return S.cpu().numpy()

            def comp_soft():
                _, P = p.predict(data)
                S = torch.zeros((K, D), dtype=torch.float64, device=dev)
                for lo in range(0, N, rows):
                    S += P[lo:lo + rows].double().T @ xs[lo:lo + rows].double()
                return S.cpu().numpy()
            routes = {"hard": "predict_labels + index_add_ (Float64, chunked)", "soft": "predict + matmul (Float64, chunked)"}
        else:
            D, per = 20000, 100
            p = predictor(D, K, N, 3)
            step = D // per
            rowval = (torch.arange(per, device=dev) * step)[None, :] + torch.randint(0, step, (N, per), device=dev, generator=g)      # sorted, distinct
            rowval = rowval.reshape(-1)
            nzval = torch.randint(1, 5, (N * per,), device=dev, generator=g).float()
            colptr = torch.arange(N + 1, device=dev, dtype=torch.int64) * per
            data = torch.sparse_csc_tensor(colptr, rowval, nzval, size=(D, N))

            def comp_hard():
                lab = p.predict_labels(data)
                col = torch.repeat_interleave(torch.arange(N, device=dev), colptr[1:] - colptr[:-1], output_size=N * per)
                S = torch.zeros(K * D, dtype=torch.float64, device=dev)
                S.index_add_(0, (lab[col] - 1) * D + rowval, nzval.double())
                return S.view(K, D).cpu().numpy()

            def comp_soft():
                _, P = p.predict(data)
                x64 = torch.sparse_csc_tensor(colptr, rowval, nzval.double(), size=(D, N))
                return torch.sparse.mm(x64, P.double()).T.contiguous().cpu().numpy()
            routes = {"hard": "predict_labels + index_add_ over the entries (Float64)", "soft": "predict + torch.sparse.mm(CSC, P) (Float64)"}
        torch.cuda.synchronize()
        r = {"N": N, "D": D, "K": K, "composition_routes": routes}
        comps = {"hard": comp_hard, "soft": comp_soft}
        for name, fn in (("floor", lambda: p.predict_labels(data)), ("composition_hard", comp_hard), ("composition_soft", comp_soft),
                         ("hard", lambda: p.count_statistics(data, assign="hard")), ("soft", lambda: p.count_statistics(data, assign="soft"))):
            note(f"{shape}: {name}")
            try:
                r[name] = median_ms(fn)
            except Exception as e:      # (a composition this torch build cannot run)
                r[name] = {"unsupported": f"{type(e).__name__}: {str(e)[:200]}"}
                torch.cuda.synchronize()
        for mode in ("hard", "soft"):
            got = p.count_statistics(data, assign=mode)
            r[mode]["over_floor"] = r[mode]["ms"] / r["floor"]["ms"]
            r[mode]["added_ms"] = r[mode]["ms"] - r["floor"]["ms"]
            if "ms" in r["composition_" + mode]:
                r[mode]["over_composition"] = r[mode]["ms"] / r["composition_" + mode]["ms"]
                ref = comps[mode]()
                r[mode]["max_rel_diff_to_composition"] = float(np.abs(got.sums - ref).max() / np.abs(ref).max())
            r[mode]["taking_part"] = int(got.count.sum())
        out[shape] = r
        p.close()
        del data
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
