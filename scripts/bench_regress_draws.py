#!/usr/bin/env python3
"""Times Regressor.sample (host/score.py, csrc/regress_draw.hip) at the shapes DESIGN section 30 quotes, and prints one JSON line.

  N = 1e6, K = 32, a Float32 device tensor (the `.T` view of (N, D_o) memory) drawn by the marginal Predictor's own sampler;
  (D_o, D_t) = (32, 32), (128, 128) and (48, 16); draws m in {1, 5, 20}; three layouts: "overlap", the model of
  scripts/bench_regress.py (means ~ N(0, I): a tile of 32 points draws many components), "separated" (the same means times 50: a tile
  holds as many clusters as before, because the points are shuffled: each gets probability 1 for its own) and "grouped" (the separated
  model with the points in the sampler's order, cluster by cluster: a tile draws one component)

  predict_std   Regressor.predict(data, return_std=True): the floor that shares the table walk
  sample_m      Regressor.sample(data, draws=m)
  single_m      m calls of Regressor.sample(data, draws=1), m > 1: what evaluating the table once per range saves
  torch_m       the composition a user needs today: marginal.predict (the (n, K) probabilities), torch.multinomial, and per draw a chunked
                gather of B[k] and W[k], two torch.bmm and a chi-square from torch.distributions -- with q = 0 in the scale (the composition
                has no cheap route to q; this flatters it) -- with its peak extra memory (torch.cuda.max_memory_allocated above rest)
  impute_m      (48, 16) only: Predictor.impute(draws=m) on the same points with the targets set to NaN
Medians of --reps calls after one warm-up call each, the calls interleaved round by round.  Every call ends synchronised.  --scale shrinks
N; --layouts, --shapes and --draws select."""
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

SHAPES = {"32x32": (32, 32), "128x128": (128, 128), "48x16": (48, 16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--layouts", default="overlap,separated,grouped")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--draws", default="1,5,20")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    N, K = int(1e6 * a.scale), 32
    ms = [int(m) for m in a.draws.split(",")]
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "N": N, "K": K, "draws": ms}

    def note(msg):
        print("[bench_regress_draws] " + msg, file=sys.stderr, flush=True)

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

    for layout in a.layouts.split(","):
        for name in a.shapes.split(","):
            Do, Dt = SHAPES[name]
            D = Do + Dt
            note(f"{layout}: D_o = {Do}, D_t = {Dt}")
            post, _, _, _ = R.niw_model(D, K, 60.0, 1)
            if layout in ("separated", "grouped"):
                post["m"] = post["m"] * 50.0
            path = R.predictor_file(0, D, 1.0, np.full(K, 100.0), post)
            given, targets = list(range(Do)), list(range(Do, D))
            with score.Predictor.load(path, capacity=1 << 20) as parent, parent.regressor(given, targets) as reg:
                mg = reg.marginal
                x, _ = mg.sample(N, seed=1)
                x = x.T.contiguous() if layout == "grouped" else x.T[torch.randperm(N, device=x.device)].contiguous()      # (N, D_o) Float32
                data = x.T
                B, c, _, _, df, W = reg.tables(factor=True)
                dev = x.device
                Bf, cf, Wf = (torch.as_tensor(t, dtype=torch.float32, device=dev) for t in (B, c, W))
                dfo = torch.as_tensor(df + Do, dtype=torch.float32, device=dev)
                dff = torch.as_tensor(df, dtype=torch.float32, device=dev)
                chunk = 1 << 14

                def composed(m):
                    _, p = mg.predict(data)
                    ks = torch.multinomial(p.clamp_min(0), m, replacement=True)          # (N, m)
                    vals = torch.empty((m, N, Dt), dtype=torch.float32, device=dev)
                    for j in range(m):
                        k = ks[:, j]
                        g = torch.distributions.Chi2(dfo[k]).sample()
                        s = torch.sqrt(dff[k] / g)
                        for lo in range(0, N, chunk):
                            kk = k[lo:lo + chunk]
                            mu = torch.bmm(Bf[kk], x[lo:lo + chunk, :, None])[:, :, 0] + cf[kk]
                            nz = torch.randn((len(kk), Dt, 1), dtype=torch.float32, device=dev)
                            vals[j, lo:lo + chunk] = mu + s[lo:lo + chunk, None] * torch.bmm(Wf[kk], nz)[:, :, 0]
                    return vals

                fns = {"predict_std": lambda: reg.predict(data, return_std=True)}
                for m in ms:
                    fns[f"sample_{m}"] = lambda m=m: reg.sample(data, draws=m)
                    if m > 1:
                        fns[f"single_{m}"] = lambda m=m: [reg.sample(data, draws=1, seed=j) for j in range(m)]
                    fns[f"torch_{m}"] = lambda m=m: composed(m)
                if name == "48x16":
                    full = torch.full((N, D), float("nan"), dtype=torch.float32, device=dev)
                    full[:, :Do] = x
                    for m in ms:
                        fns[f"impute_{m}"] = lambda m=m: parent.impute(full.T, draws=m)
                res = interleaved_ms(fns)
                torch.cuda.synchronize()
                for m in ms:
                    rest = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    v = composed(m)
                    torch.cuda.synchronize()
                    res[f"torch_{m}_peak_extra_mb"] = (torch.cuda.max_memory_allocated() - rest - v.numel() * 4) / 2 ** 20
                    del v
                    res[f"sample_{m}_over_predict_std"] = res[f"sample_{m}_ms"] / res["predict_std_ms"]
                    res[f"torch_{m}_over_sample"] = res[f"torch_{m}_ms"] / res[f"sample_{m}_ms"]
                    if m > 1:
                        res[f"single_{m}_over_sample"] = res[f"single_{m}_ms"] / res[f"sample_{m}_ms"]
                    if name == "48x16":
                        res[f"impute_{m}_over_sample"] = res[f"impute_{m}_ms"] / res[f"sample_{m}_ms"]
                comp = reg.sample(data, draws=1, return_components=True).components
                tiles = comp[0, :(N // 32) * 32].reshape(-1, 32)
                srt = tiles.sort(dim=1).values
                res["components_per_tile"] = float(((srt[:, 1:] != srt[:, :-1]).sum(1) + 1).float().mean())
                out[f"{layout}_{name}"] = res
                note(json.dumps(res))
                del x, data
    print(json.dumps(out))


if __name__ == "__main__":
    main()
