#!/usr/bin/env python3
"""Times Predictor.held_out (host/score.py, csrc/holdout.hip) and one Predictor.grow, and prints one JSON line.

  N = 1e6, K = 32, a Float32 device tensor (the `.T` view of (N, D) memory), D = 64 and D = 256; 0.1 %, 1 % and 10 % of the points moved
  far from every cluster, so that they lie beyond min_tail = 1e-6 (of the points left where they were drawn, about N * 1e-6 do as well)

On the same data, in the same process:
  floor          Predictor.statistics(min_tail=t): the same walk over the table and the same tail pass, plus the moments
  held_out       Predictor.held_out(min_tail=t)
  composition    what a user needed before: Predictor.typicality -> tail < t -> nonzero -> index_select of the rows, all in torch on the device
and, at 1 %, one Predictor.grow end to end on a freshly loaded model, split into capture (the held_out part), fit (the sub-fit) and
reload (the rest: the graft, the predictive parameters into the worker).  The data are drawn by Predictor.sample from the model they are
scored with.  Every figure is the median, the minimum and the maximum of --reps calls after one warm-up call, timed from the host around
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

T = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--D", default="64,256")
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--fractions", default="0.001,0.01,0.1")
    ap.add_argument("--grow-iters", type=int, default=100)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    api = importlib.import_module(pkg.__name__ + ".host.api")
    priors = importlib.import_module(pkg.__name__ + ".host.priors")
    from tools import sample_ref as R
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale, "min_tail": T}

    def note(msg):
        print("[bench_holdout] " + msg, file=sys.stderr, flush=True)

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

    def composition(p, data):
        t = p.typicality(data)
        idx = torch.nonzero(t.tail < T).squeeze(1)
        return torch.index_select(data.T, 0, idx), idx

    N, K = int(1e6 * a.scale), a.K
    for D in (int(d) for d in a.D.split(",")):
        post, _, _, _ = R.niw_model(D, K, 60.0, 1)
        model = lambda: R.predictor_file(0, D, 1.0, np.full(K, 100.0), post)      # noqa: E731  (an in-memory .npz, without the prior)
        prior = priors.niw_hyperparams(1.0, np.zeros(D), D + 3.0, np.eye(D))
        with score.Predictor.load(model(), capacity=N) as p:
            note(f"D = {D}: drawing the data")
            x, _ = p.sample(N, seed=1)
            xs = x.T[torch.randperm(N, device=x.device)].contiguous()          # (N, D) float32, the clusters mixed
            del x
            torch.cuda.empty_cache()
            out[f"D{D}"] = r = {"N": N, "D": D, "K": K}
            for frac in (float(f) for f in a.fractions.split(",")):
                g = torch.Generator(device=xs.device).manual_seed(int(frac * 1e6))
                moved = torch.randperm(N, device=xs.device, generator=g)[:int(round(frac * N))]
                ys = xs.clone()
                ys[moved] += 1000.0
                data = ys.T
                c = {}
                for name, fn in (("floor", lambda: p.statistics(data, min_tail=T)), ("held_out", lambda: p.held_out(data, min_tail=T)),
                                 ("composition", lambda: composition(p, data))):
                    note(f"D = {D} {frac:g}: {name}")
                    c[name] = timed(fn)
                h = p.held_out(data, min_tail=T)
                rows, idx = composition(p, data)
                c["total"], c["moved"] = h.total, int(moved.numel())
                c["same_as_composition"] = bool(torch.equal(h.index, idx) and torch.equal(h.points.T, rows))
                c["held_out"]["over_floor"] = c["held_out"]["ms"] / c["floor"]["ms"]
                c["held_out"]["over_composition"] = c["held_out"]["ms"] / c["composition"]["ms"]
                c["floor"]["spread"] = (c["floor"]["worst_ms"] - c["floor"]["best_ms"]) / c["floor"]["ms"]
                # beyond the floor's traffic: ballots and workgroup words written and read once each, the held rows read and written, their indices
                c["bytes_over_floor"] = int(2 * (N // 8 + (N // 256 + 1) * 24) + h.total * (8 * D + 8))
                r[f"{frac:g}"] = c
                if abs(frac - 0.01) < 1e-9:
                    note(f"D = {D} {frac:g}: grow")
                    parts = {}
                    fit = api.fit

                    def timed_fit(*args, **kw):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        try:
                            return fit(*args, **kw)
                        finally:
                            torch.cuda.synchronize()
                            parts["fit_ms"] = (time.perf_counter() - t0) * 1e3
                    with score.Predictor.load(model(), capacity=N) as q:
                        q.held_out(data, min_tail=T)                           # warm-up of the worker's buffers
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        q.held_out(data, min_tail=T)
                        torch.cuda.synchronize()
                        parts["capture_ms"] = (time.perf_counter() - t0) * 1e3
                        api.fit = timed_fit
                        try:
                            t0 = time.perf_counter()
                            gr = q.grow(data, min_tail=T, prior=prior, iters=a.grow_iters)
                            torch.cuda.synchronize()
                            parts["total_ms"] = (time.perf_counter() - t0) * 1e3
                        finally:
                            api.fit = fit
                        parts["reload_ms"] = parts["total_ms"] - parts["capture_ms"] - parts.get("fit_ms", 0.0)
                        parts.update(added=gr.added, sizes=[int(v) for v in gr.sizes], dropped=gr.dropped, K_after=q.K, iters=a.grow_iters)
                    c["grow"] = parts
                del ys, data, rows, idx, h
                torch.cuda.empty_cache()
            del xs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
