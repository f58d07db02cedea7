#!/usr/bin/env python3
"""Times Predictor.explain (host/score.py, csrc/explain.hip) at the two shapes DESIGN quotes, and prints one JSON line.

  N = 1e6, K = 32, a Float32 device tensor (the `.T` view of (N, D) memory), D = 64 and D = 256

On the same data, in the same process:
  typicality         Predictor.typicality alone: the floor, explain cannot avoid that pass
  explain_top4       Predictor.explain(top=4)
  explain            Predictor.explain(): all D features of every point
  composition        what a user needed before: Predictor.predict_labels, a gather of R[label] and two torch.bmm (y = R z, g = R' y) in chunks of
                     rows sized so that the gathered (rows, D, D) Float32 factors stay within 256 MB, the z-scores on the GPU, then
                     scipy.stats.t.sf on the host
and the two routes compared: the largest difference of the z-scores relative to 1 + |t|.  The data are drawn by Predictor.sample from the
model they are scored with.  Every figure is the median (and the minimum) of --reps calls after one warm-up call, timed from the host
around the call; every call ends synchronised.  The composition is timed ONCE, behind the library's calls (so the device is warm): its host
part alone takes tens of seconds at D = 256.  --scale shrinks N (a quick check of the script itself)."""
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
    ap.add_argument("--calls", default="typicality,explain_top4,explain,composition",
                    help="which of typicality, explain_top4, explain, composition to run (a profiler's kernel statistics then speak of those alone)")
    a = ap.parse_args()
    import torch
    from scipy.stats import t as student
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale}

    def note(msg):
        print("[bench_explain] " + msg, file=sys.stderr, flush=True)

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

    def composition(p, data, m, Rf, df_d, df64):
        lab = p.predict_labels(data) - 1
        X = data.T                                                             # (N, D)
        D = X.shape[1]
        t = torch.empty(X.shape, dtype=torch.float32, device=X.device)
        rows = max(1, (1 << 28) // (4 * D * D))
        for lo in range(0, X.shape[0], rows):
            k = lab[lo:lo + rows]
            Rk = Rf[k]
            y = torch.bmm(Rk, (X[lo:lo + rows] - m[k]).unsqueeze(2))
            g = torch.bmm(Rk.transpose(1, 2), y).squeeze(2)
            q = (y * y).sum(1)
            ad = (Rk * Rk).sum(1)
            dfk = df_d[k].unsqueeze(1)
            t[lo:lo + rows] = g * torch.sqrt((dfk + (D - 1)) / (ad * (dfk + (q - g * g / ad).clamp_min(0))))
        th = t.cpu().numpy().astype(np.float64)
        return t, 2.0 * student.sf(np.abs(th), (df64[lab.cpu().numpy()] + D - 1)[:, None])

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
            df_d = torch.as_tensor(np.asarray(df, np.float32), device=xs.device)
            df64 = np.asarray(df, np.float32).astype(np.float64)
            r = {"N": N, "D": D, "K": K}
            calls = a.calls.split(",")
            for name, fn in (("typicality", lambda: p.typicality(data)), ("explain_top4", lambda: p.explain(data, top=4)),
                             ("explain", lambda: p.explain(data))):
                if name in calls:
                    note(f"D = {D}: {name}")
                    r[name] = median_ms(fn)
            if "composition" in calls:
                note(f"D = {D}: composition (once: the host part takes tens of seconds at D = 256)")
                t0 = time.perf_counter()
                tc, _ = composition(p, data, m_d, R_d, df_d, df64)
                torch.cuda.synchronize()
                r["composition"] = {"ms": (time.perf_counter() - t0) * 1e3, "calls": 1}
                got = p.explain(data)
                r["zscore_max_diff_rel_1_plus_t"] = float(((got.zscore.T - tc).abs() / (1 + tc.abs())).max().item())
                r["skipped"], r["incomplete"] = got.skipped, got.incomplete
                del got, tc
            for name in ("explain_top4", "explain"):
                if name in r and "typicality" in r:
                    r[name]["added_ms"] = r[name]["ms"] - r["typicality"]["ms"]
                if name in r and "composition" in r:
                    r[name]["over_composition"] = r[name]["ms"] / r["composition"]["ms"]
            out[f"D{D}"] = r
            del xs, data
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
