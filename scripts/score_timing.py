"""Timing of the scoring surface (include/dpmm_hip_score.h, host/score.py) against `predict`, in one process -> profiles/score_timing.txt.

    python scripts/score_timing.py [--n 10000000] [--out profiles/score_timing.txt] [--quick]

Large case: N points, D = 64, K = 32, a bf16 device tensor in (N, D).T layout.  `predict` (labels + probs) against a Predictor with
capacity = N for labels only, score_samples, top-4 and labels + probs: median of 10 runs after 3 warm-up runs, and the largest drop of
free device memory (hipMemGetInfo) seen during a run.  Budget sweep: DPMM_OPT_SCORE_TABLE_MB = 32 / 128 / 512 on labels + probs.
Serving case: 1000 batches of 4096 points through one Predictor against 1000 calls of `predict`, per-batch median."""
import argparse
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def synthetic_model(host, D, K, seed=3):
    """What `predict` and a Predictor read of a fitted model, with exactly K clusters: posteriors of K well-separated Gaussian clusters
    (means ~ N(0, 100 I) as the reference's generator draws them, unit covariance, 1000 to 2000 points each).  No fit: the shape is fixed."""
    import types
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1000, 2000, K)
    N3 = np.repeat(cnt, 3).astype(np.float64)
    nu = D + 3 + N3
    post = dict(kappa=1 + N3, nu=nu, m=np.repeat(rng.standard_normal((K, D)) * 10, 3, axis=0),
                U=np.sqrt(nu)[:, None, None] * np.eye(D)[None], logdet_psi=np.zeros(3 * K))      # nu' psi' = U U', psi' = I
    prior = host.niw_hyperparams(1.0, np.zeros(D), D + 3, np.eye(D))
    s = types.SimpleNamespace(K=K, prior=prior, post=post, alpha=10.0, points_count=cnt, wk=types.SimpleNamespace(device=0))
    return types.SimpleNamespace(sampler=s)


def points(model, n, g):
    """(n, D) bf16 points around the model's cluster means."""
    means = torch.from_numpy(model.sampler.post["m"][::3].astype(np.float32)).to("cuda:0")
    z = torch.randint(0, means.shape[0], (n,), device="cuda:0", generator=g)
    return (means[z] + torch.randn((n, means.shape[1]), device="cuda:0", generator=g)).to(torch.bfloat16)


class FreeWatch:
    """Smallest free device memory seen while a block runs, sampled from a thread."""

    def __enter__(self):
        torch.cuda.synchronize()
        self.start = torch.cuda.mem_get_info(0)[0]
        self.low = self.start
        self.stop = False
        self.t = threading.Thread(target=self._poll)
        self.t.start()
        return self

    def _poll(self):
        while not self.stop:
            self.low = min(self.low, torch.cuda.mem_get_info(0)[0])
            time.sleep(0.0005)

    def __exit__(self, *exc):
        self.stop = True
        self.t.join()
        self.drop_mb = (self.start - self.low) / 2.0 ** 20


def timed(fn, runs, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    with FreeWatch() as fw:
        for _ in range(runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), fw.drop_mb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10 ** 7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_timing.txt"))
    ap.add_argument("--quick", action="store_true", help="3 runs, 100 serving batches")
    ap.add_argument("--only", default="", help="comma list of parts: large, sweep, serving")
    a = ap.parse_args()
    parts = set(a.only.split(",")) if a.only else {"large", "sweep", "serving"}
    runs, warm, batches = (3, 1, 100) if a.quick else (10, 3, 1000)
    pkg = load_package()
    import importlib
    host = importlib.import_module(pkg.__name__ + ".host")
    binding = importlib.import_module(pkg.__name__ + ".binding")
    D, K = 64, 32
    model = synthetic_model(host, D, K)
    lines = [f"score_timing: N = {a.n}, D = {D}, K = {model.sampler.K}, bf16 device tensor (N, D).T; median of {runs} after {warm} warm-up; ms",
             "device: " + torch.cuda.get_device_name(0)]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda:0").manual_seed(1)
    if parts & {"large", "sweep"}:
        X = points(model, a.n, g)
        data = X.T
        if "large" in parts:
            t, d = timed(lambda: host.predict(model, data), runs, warm)
            emit(f"large  predict (labels + probs)              {t:9.2f} ms   peak free-memory drop {d:9.1f} MB")
            with host.Predictor(model, capacity=a.n) as p:
                for name, fn in (("labels only", lambda: p.predict_labels(data)), ("score_samples", lambda: p.score_samples(data)),
                                 ("top-4", lambda: p.predict_topk(data, 4)), ("labels + probs", lambda: p.predict(data))):
                    t, d = timed(fn, runs, warm)
                    emit(f"large  Predictor {name:<28s}{t:9.2f} ms   peak free-memory drop {d:9.1f} MB")
        if "sweep" in parts:
            for mb in (32, 128, 512):
                with host.Predictor(model, capacity=a.n) as p:
                    p._wk.set_option(binding.OPT_SCORE_TABLE_MB, float(mb))
                    t, d = timed(lambda: p.predict(data), runs, warm)
                    t2, _ = timed(lambda: p.predict_labels(data), runs, warm)
                    emit(f"sweep  budget {mb:4d} MB: labels + probs {t:9.2f} ms   labels only {t2:9.2f} ms   peak free-memory drop {d:9.1f} MB")
        del X, data
        torch.cuda.empty_cache()
    if "serving" in parts:
        B = 4096
        Xs = points(model, batches * B, g).reshape(batches, B, D)
        torch.cuda.synchronize()
        ts = []
        for i in range(batches):
            t0 = time.perf_counter()
            host.predict(model, Xs[i].T)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        emit(f"serve  predict, {batches} batches of {B}:     per-batch median {np.median(ts):8.3f} ms")
        with host.Predictor(model, capacity=B) as p:
            for name, fn in (("labels + probs", p.predict), ("labels only", p.predict_labels), ("score_samples", p.score_samples)):
                ts = []
                for i in range(batches):
                    t0 = time.perf_counter()
                    fn(Xs[i].T)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                emit(f"serve  Predictor {name:<16s} per-batch median {np.median(ts):8.3f} ms")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
