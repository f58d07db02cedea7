#!/usr/bin/env python3
"""Times Predictor.explain_groups (host/score.py, csrc/explain_group.hip) at the shapes DESIGN §33 quotes, and prints one JSON line.

  N = 1e6, K = 32, a Float32 device tensor (the `.T` view of (N, D) memory); D = 64 with 4 x 16 and 8 x 8 groups, D = 256 with 4 x 64 and
  16 x 16 groups

On the same data, in the same process, the calls INTERLEAVED (one round calls each once; --reps rounds after one warm-up round; medians):
  typicality         Predictor.typicality alone: the floor, it shares the table and the q pass
  explain_top4       Predictor.explain(top=4): it shares both passes over R
  groups_<a>x<s>     Predictor.explain_groups with a blocks of s consecutive features (the tables are uploaded by the warm-up round and
                     again whenever the groups change: the two groupings of a D are timed in rounds of their own)
  composition        what a user needed before, ONCE per grouping: Predictor.predict_labels, a gather of R[label] and two torch.bmm
                     (y = R z, g = R' y) in chunks of rows, a gather of the clusters' block factors, a batched triangular solve per group,
                     then scipy.special.betainc on the host
and the two routes compared: the largest difference of q_G relative to 1 + q_G.  `floor_spread` is (max - min) / median of the floor's
calls.  --scale shrinks N (a quick check of the script itself)."""
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

SHAPES = {64: (16, 8), 256: (64, 16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--D", default="64,256")
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--no-composition", action="store_true")
    a = ap.parse_args()
    import torch
    from scipy.special import betainc
    from __graft_entry__ import load_package
    pkg = load_package()
    score = importlib.import_module(pkg.__name__ + ".host.score")
    from tools import sample_ref as R
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "scale": a.scale}

    def note(msg):
        print("[bench_explain_groups] " + msg, file=sys.stderr, flush=True)

    def rounds(calls):
        """Every call once per round, a warm-up round first: name -> list of ms."""
        ts = {name: [] for name, _ in calls}
        for rep in range(a.reps + 1):
            for name, fn in calls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep:
                    ts[name].append((time.perf_counter() - t0) * 1e3)
        return ts

    def composition(p, data, m, Rf, df_d, df64, groups):
        lab = p.predict_labels(data) - 1
        X = data.T                                                             # (N, D)
        D = X.shape[1]
        A = torch.bmm(Rf.transpose(1, 2), Rf)
        Ls = [torch.linalg.cholesky(A[:, g][:, :, g]) for g in (torch.as_tensor(g, device=X.device) for g in groups)]
        qg = torch.empty((X.shape[0], len(groups)), dtype=torch.float32, device=X.device)
        q = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
        rows = max(1, (1 << 28) // (4 * D * D))
        for lo in range(0, X.shape[0], rows):
            k = lab[lo:lo + rows]
            Rk = Rf[k]
            y = torch.bmm(Rk, (X[lo:lo + rows] - m[k]).unsqueeze(2))
            g = torch.bmm(Rk.transpose(1, 2), y).squeeze(2)
            q[lo:lo + rows] = (y * y).sum(1).squeeze(1)
            for j, grp in enumerate(groups):
                v = torch.linalg.solve_triangular(Ls[j][k], g[:, grp].unsqueeze(2), upper=False)
                qg[lo:lo + rows, j] = (v * v).sum(1).squeeze(1)
        s = np.array([len(g) for g in groups], np.float64)
        dfh = df64[lab.cpu().numpy()][:, None]
        qh, qgh = q.cpu().numpy().astype(np.float64)[:, None], qg.cpu().numpy().astype(np.float64)
        f = qgh * (dfh + D - s) / (dfh + np.maximum(qh - qgh, 0))
        nu = dfh + D - s
        return qg, betainc(0.5 * nu, 0.5 * s, nu / (nu + f))

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
            floor = []
            for s in SHAPES.get(D, (max(1, D // 4),)):
                groups = [list(range(lo, lo + s)) for lo in range(0, D - s + 1, s)]
                name = f"groups_{len(groups)}x{s}"
                note(f"D = {D}: {name}, interleaved with typicality and explain(top=4)")
                ts = rounds([("typicality", lambda: p.typicality(data)), ("explain_top4", lambda: p.explain(data, top=min(4, D))),
                             (name, lambda: p.explain_groups(data, groups))])
                floor += ts["typicality"]
                med = {k: float(np.median(v)) for k, v in ts.items()}
                r[name] = {"ms": med[name], "best_ms": float(min(ts[name])), "typicality_ms": med["typicality"], "explain_top4_ms": med["explain_top4"],
                           "over_typicality_ms": med[name] - med["typicality"], "over_explain_top4_ms": med[name] - med["explain_top4"]}
                if not a.no_composition:
                    note(f"D = {D}: {name}: the composition, once")
                    t0 = time.perf_counter()
                    qc, _ = composition(p, data, m_d, R_d, df_d, df64, groups)
                    torch.cuda.synchronize()
                    r[name]["composition_ms"] = (time.perf_counter() - t0) * 1e3
                    got = p.explain_groups(data, groups)
                    r[name]["qg_max_diff_rel_1_plus_qg"] = float(((got.group_mahalanobis.T - qc).abs() / (1 + qc.abs())).max().item())
                    r[name]["over_composition"] = r[name]["ms"] / r[name]["composition_ms"]
                    del got, qc
            r["floor_spread"] = float((max(floor) - min(floor)) / np.median(floor))
            out[f"D{D}"] = r
            del xs, data
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
