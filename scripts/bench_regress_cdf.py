#!/usr/bin/env python3
"""Times Regressor.cdf and Regressor.quantile (host/score.py, csrc/regress_cdf.hip) at the shapes DESIGN section 31 quotes, and prints one JSON line.

  N = 1e6, K = 32, a Float32 device tensor drawn by the joint Predictor's own sampler, the points shuffled; (D_o, D_t) = (32, 32), (128, 128)
  and (48, 16); two models per shape: "separated" (cluster means 10 times further apart) and "overlapping" (0.3 times)

  cdf           Regressor.cdf(data, y) at the drawn targets
  q1, q3, q9    Regressor.quantile at 1, 3 and 9 levels
  std           Regressor.predict(data, return_std=True): the floor that shares tile and chain
  host          the composition a user needed before: marginal.predict (the (n, K) probabilities), torch for mu, the quadratic forms and
                sigma, then scipy.stats.t.cdf on the host -- timed on N / 64 points and scaled by 64 (it is linear in N)
  draws         empirical quantiles from Regressor.sample: m = p (1 - p) (1.96 / 0.005)^2 = 7299 draws give a 5 % quantile to +-0.005 in
                probability (95 %) -- the accuracy the issue of this feature names; the contract of `quantile` is seven orders tighter and out
                of reach of any m.  Timed at 20 draws and scaled by m / 20 (the draws of a point are independent work).
  one_cluster_tiles   the share of 32-point tiles whose points all have one cluster with p != 0: those run no solve
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

LEVELS = {1: (0.5,), 3: (0.05, 0.5, 0.95), 9: (0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99)}
M_DRAWS = int(np.ceil(0.05 * 0.95 * (1.96 / 0.005) ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    from scipy import stats
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    N, K = int(1e6 * a.scale), 32
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "N": N, "K": K, "m_draws": M_DRAWS}

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
        for name, spread in (("separated", 10.0), ("overlapping", 0.3)):
            print(f"[bench_regress_cdf] D_o = {Do}, D_t = {Dt}, {name}", file=sys.stderr, flush=True)
            post, _, _, _ = R.niw_model(D, K, 60.0, 1)
            post["m"] = (post["m"] * spread).astype(np.float32).astype(np.float64)
            path = R.predictor_file(0, D, 1.0, np.full(K, 100.0), post)
            given, targets = list(range(Do)), list(range(Do, D))
            with score.Predictor.load(path, capacity=1 << 20) as parent, parent.regressor(given, targets) as reg:
                mg = reg.marginal
                full, _ = parent.sample(N, seed=1)
                full = full.T[torch.randperm(N, device=full.device)].contiguous()       # (N, D) Float32, the clusters mixed
                x, yt = full[:, :Do].contiguous(), full[:, Do:].contiguous()
                data, y = x.T, yt.T
                B, c, V, h, df = reg.tables()
                Bf, cf = (torch.as_tensor(t, dtype=torch.float32, device=x.device) for t in (B, c))
                sub = max(1, N // 64)

                mm = torch.as_tensor(np.asarray(mg._predictive_args()[1][0], np.float32), device=x.device)
                RR = torch.as_tensor(np.asarray(mg._predictive_args()[1][1], np.float32).reshape(K, Do, Do), device=x.device)
                dff, Vf = (torch.as_tensor(t, dtype=torch.float64, device=x.device) for t in (df, V))

                def host():
                    _, p = mg.predict(x[:sub].contiguous().T)
                    mu = torch.einsum("kde,ne->nkd", Bf, x[:sub]) + cf[None]
                    q = (torch.einsum("kij,nkj->nki", RR, x[:sub, None, :] - mm[None]) ** 2).sum(-1).double()
                    sig = torch.sqrt(((dff[None] + q) / (dff[None] + Do))[:, :, None] * Vf[None])
                    t = ((yt[:sub, None, :].double() - mu.double()) / sig).cpu().numpy()
                    return (p.cpu().numpy()[:, :, None] * stats.t.cdf(t, (df + Do)[None, :, None])).sum(1)

                fns = {"cdf": lambda: reg.cdf(data, y), "std": lambda: reg.predict(data, return_std=True), "draws20": lambda: reg.sample(data, draws=20, seed=1)}
                for L, lv in LEVELS.items():
                    fns[f"q{L}"] = (lambda lv=lv: reg.quantile(data, lv))
                res = interleaved_ms(fns)
                t0 = time.perf_counter()
                host()
                res["host_ms"] = (time.perf_counter() - t0) * 1e3 * (N / sub)
                res["draws_ms"] = res.pop("draws20_ms") * M_DRAWS / 20
                _, p = mg.predict(data)
                one = ((p != 0).sum(1) <= 1)
                tiles = one[:N - N % 32].reshape(-1, 32).all(1)
                res["one_cluster_tiles"] = float(tiles.float().mean())
                res["one_cluster_points"] = float(one.float().mean())
                out[f"{Do}x{Dt}_{name}"] = res
                del full, x, yt, data, y, p
    print(json.dumps(out))


if __name__ == "__main__":
    main()
