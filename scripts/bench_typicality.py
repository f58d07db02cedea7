#!/usr/bin/env python3
"""Times Predictor.typicality (host/score.py, csrc/typicality.hip) at the two shapes DESIGN quotes, and prints one JSON line.

  N = 1e6, K = 32, a Float32 device tensor (the `.T` view of (N, D) memory), D = 64 and D = 256

On the same data, in the same process:
  floor              Predictor.predict_labels alone: typicality cannot avoid evaluating that table
  composition        what a user needed before: Predictor.predict_labels, a gather of R[label] and torch.bmm in chunks of rows sized so
                     that the gathered (rows, D, D) Float32 factors stay within 256 MB, then scipy.special.betainc on the host
  typicality         Predictor.typicality
  statistics         Predictor.statistics() and Predictor.statistics(min_tail=1e-3)
and the two routes compared: the largest relative difference of q and the largest absolute difference of the tails.  The data are drawn
by Predictor.sample from the model they are scored with.  Every figure is the median (and the minimum) of --reps calls after one warm-up
call, timed from the host around the call; every call ends synchronised.  --scale shrinks N (a quick check of the script itself)."""
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
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--D", default="64,256")
    ap.add_argument("--K", type=int, default=32)
    a = ap.parse_args()
    import torch
    from scipy.special import betainc
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale}

    def note(msg):
        print("[bench_typicality] " + msg, file=sys.stderr, flush=True)

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

    def composition(p, data, m, Rf, df):
        lab = p.predict_labels(data) - 1
        X = data.T                                                             # (N, D)
        D = X.shape[1]
        q = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
        rows = max(1, (1 << 28) // (4 * D * D))
        for lo in range(0, X.shape[0], rows):
            k = lab[lo:lo + rows]
            y = torch.bmm(Rf[k], (X[lo:lo + rows] - m[k]).unsqueeze(2)).squeeze(2)
            q[lo:lo + rows] = (y * y).sum(1)
        qh, dfh = q.cpu().numpy().astype(np.float64), df[lab.cpu().numpy()]
        return q, betainc(0.5 * dfh, 0.5 * D, dfh / (dfh + qh))

    N, K = int(1e6 * a.scale), a.K
    for D in (int(d) for d in a.D.split(",")):
        post, _, _, _ = R.niw_model(D, K, 60.0, 1)
        with score.Predictor.load(R.predictor_file(0, D, 1.0, np.full(K, 100.0), post), capacity=N) as p:
            note(f"D = {D}: drawing the data")
            x, _ = p.sample(N, seed=1)
            xs = x.T[torch.randperm(N, device=x.device)].contiguous()          # (N, D) float32, the clusters mixed
            del x
            torch.cuda.empty_cache()
            data = xs.T
            _, (m, Rw, _, df, _) = p._predictive_args()
            m_d = torch.as_tensor(np.asarray(m, np.float32), device=xs.device)
            R_d = torch.as_tensor(np.triu(np.asarray(Rw, np.float32).reshape(K, D, D)), device=xs.device)
            df64 = np.asarray(df, np.float32).astype(np.float64)
            r = {"N": N, "D": D, "K": K}
            for name, fn in (("floor", lambda: p.predict_labels(data)), ("composition", lambda: composition(p, data, m_d, R_d, df64)),
                             ("typicality", lambda: p.typicality(data)), ("statistics", lambda: p.statistics(data)),
                             ("statistics_min_tail", lambda: p.statistics(data, min_tail=1e-3))):
                note(f"D = {D}: {name}")
                r[name] = median_ms(fn)
            got = p.typicality(data)
            qc, tc = composition(p, data, m_d, R_d, df64)
            r["q_max_rel_diff"] = float(((got.mahalanobis - qc).abs() / qc.clamp_min(1e-30)).max().item())
            r["tail_max_abs_diff"] = float(np.abs(got.tail.cpu().numpy().astype(np.float64) - tc).max())
            r["skipped"], r["incomplete"] = got.skipped, got.incomplete
            r["held_out_at_1e-3"] = p.statistics(data, min_tail=1e-3).held_out
            r["typicality"]["over_floor"] = r["typicality"]["ms"] / r["floor"]["ms"]
            r["typicality"]["over_composition"] = r["typicality"]["ms"] / r["composition"]["ms"]
            r["statistics_min_tail"]["over_statistics"] = r["statistics_min_tail"]["ms"] / r["statistics"]["ms"]
            out[f"D{D}"] = r
            del xs, data
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
