#!/usr/bin/env python3
"""Times Predictor.typicality / Predictor.explain(top=4) with gaps="marginalize" (host/score.py, typ_gap_kernel of csrc/typicality.hip,
csrc/explain_gap.hip) and prints one JSON line.

  N = 1e6, K = 32, a Float32 device tensor (the `.T` view of (N, D) memory), D = 64 and D = 256, and 0 % / 1 % / 10 % of the points lacking
  1 .. 4 features (NaN), on a Predictor made with missing="marginalize"

On the same data, in the same process:
  typicality_gaps, explain_gaps   the calls with gaps="marginalize"
  typicality, explain             the same calls with the default: the floor, which shares everything but the list-driven kernels
and the cost per point with gaps the difference implies (ns).  The four calls are interleaved -- every repetition runs each of them once -- so
that a drift of the machine meets all four alike, and the cost is the median of the --reps paired differences (gaps call minus default call
of the same repetition), printed with the smallest and the largest of them: where that span holds 0 the cost is not resolved.  At 0 % the
default call is also what the parent commit runs -- it launches nothing new -- so its median, repeated --floor-reps times, is printed as
`default_medians`.  --default-only times nothing else and uses no keyword the parent commit lacks: copied into a checkout of the parent
commit and run there in the same session, it gives the parent's five medians to compare with.  The data are drawn by Predictor.sample from the
model they are scored with.  Every figure is the median (and the minimum) of --reps calls after one warm-up call, timed from the host around
the call; every call ends synchronised.  --scale shrinks N (a quick check of the script itself)."""
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
    ap.add_argument("--floor-reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--D", default="64,256")
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--gaps", default="0,0.01,0.1")
    ap.add_argument("--default-only", action="store_true")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale}

    def note(msg):
        print("[bench_gap_typicality] " + msg, file=sys.stderr, flush=True)

    def times_ms(fns):
        """(len(fns), reps) times: one warm-up call of each, then --reps rounds that run each of them once"""
        ts = np.empty((len(fns), a.reps))
        for rep in range(-1, a.reps):
            for j, fn in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep >= 0:
                    ts[j, rep] = (time.perf_counter() - t0) * 1e3
        return ts

    def median_ms(fn):
        ts = times_ms([fn])[0]
        return {"ms": float(np.median(ts)), "best_ms": float(ts.min())}

    def paired_ns(ts_gaps, ts_default, ng):
        d = (ts_gaps - ts_default) * 1e6 / ng
        return {"ns": float(np.median(d)), "min_ns": float(d.min()), "max_ns": float(d.max()), "resolved": bool(d.min() > 0 or d.max() < 0)}

    N, K = int(1e6 * a.scale), a.K
    for D in (int(d) for d in a.D.split(",")):
        post, _, _, _ = R.niw_model(D, K, 60.0, 1)
        with score.Predictor.load(R.predictor_file(0, D, 1.0, np.full(K, 100.0), post), capacity=N, missing="marginalize") as p:
            note(f"D = {D}: drawing the data")
            x, _ = p.sample(N, seed=1)
            xs = x.T[torch.randperm(N, device=x.device)].contiguous()          # (N, D) float32, the clusters mixed
            del x
            torch.cuda.empty_cache()
            for frac in ((0.0,) if a.default_only else (float(f) for f in a.gaps.split(","))):
                xg = xs.clone()
                g = torch.Generator(device=xs.device).manual_seed(7)
                ng = int(round(frac * N))
                if ng:
                    rows = torch.randperm(N, device=xs.device, generator=g)[:ng]
                    cols = torch.rand((ng, D), device=xs.device, generator=g).argsort(1)[:, :4]
                    keep = torch.arange(4, device=xs.device)[None, :] < torch.randint(1, 5, (ng, 1), device=xs.device, generator=g)
                    xg[rows[:, None].expand(-1, 4)[keep], cols[keep]] = float("nan")
                data = xg.T
                r = {"N": N, "D": D, "K": K, "gappy": ng}
                floor = lambda: {"typicality": [median_ms(lambda: p.typicality(data))["ms"] for _ in range(a.floor_reps)],
                                 "explain": [median_ms(lambda: p.explain(data, top=4))["ms"] for _ in range(a.floor_reps)]}
                if a.default_only:
                    note(f"D = {D}: the default calls alone")
                    r["default_medians"] = floor()
                    out[f"D{D}_gaps0"] = r
                    continue
                names = ("typicality", "typicality_gaps", "explain", "explain_gaps")
                note(f"D = {D}, {frac:g} of the points with gaps")
                ts = times_ms([lambda: p.typicality(data), lambda: p.typicality(data, gaps="marginalize"), lambda: p.explain(data, top=4),
                               lambda: p.explain(data, top=4, gaps="marginalize")])
                for j, name in enumerate(names):
                    r[name] = {"ms": float(np.median(ts[j])), "best_ms": float(ts[j].min())}
                got = p.typicality(data, gaps="marginalize")
                r["skipped"], r["incomplete"] = got.skipped, got.incomplete
                if ng:
                    r["typicality_per_gappy_point"] = paired_ns(ts[1], ts[0], ng)
                    r["explain_per_gappy_point"] = paired_ns(ts[3], ts[2], ng)
                else:
                    r["default_medians"] = floor()
                out[f"D{D}_gaps{frac:g}"] = r
                del xg, data
            del xs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
