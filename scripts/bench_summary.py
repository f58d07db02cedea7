#!/usr/bin/env python3
"""Times the label trace (include/dpmm_hip_trace.h, csrc/trace.hip) at the shape DESIGN section 19 quotes, and prints one JSON line.

  N = 1e7 points, T = 32 samples + the final labelling, random labellings of K = 32 clusters (and of K = 4: every wave on 16 counters)

  (a) record        dpmm_trace_record: 4 N bytes read, 2 N bytes written.  `--reps` records are queued and the stream synchronised once.
      copy floor    a device-to-device copy that moves the same 6 N bytes (3 N read, 3 N written), timed with events on torch's stream;
                    the library's own copy kernel is not reachable through the C ABI
      --step-ms     the step time `bench.py` printed for the same N: the record is reported as a share of it
  (b) tables        all T (T + 1) / 2 = 528 tables of a candidate against an earlier sample plus the T + 1 diagonals in ONE
                    dpmm_trace_tables call, the T ratio tables on the host and dpmm_trace_confidence: what a PosteriorSummary costs
      torch         what a user could do before on the same device: per pair torch.bincount(a.long() * Kt + b.long(), minlength=Ks * Kt)
                    on the same 16-bit ids (528 pairs; the confidence is not included: it only makes this side slower)
      one by one    528 dpmm_trace_tables calls of one pair each: one launch, one table in LDS and one synchronisation per pair, as
                    dpmm_contingency works
Every figure is a median over --reps calls after one warm-up call; every call ends synchronised.  --scale shrinks N."""
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
    ap.add_argument("--step-ms", type=float, default=0.0)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    binding = importlib.import_module(pkg.__name__ + ".binding")
    summary = importlib.import_module(pkg.__name__ + ".host.summary")
    N, T = int(1e7 * a.scale), 32
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "N": N, "T": T}

    def note(msg):
        print("[bench_summary] " + msg, file=sys.stderr, flush=True)

    def wall_ms(fn, reps=a.reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def event_ms(fn, reps=a.reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    wk = binding.Worker(binding.PRIOR_NIW, 2, N, device=0, seed=1, timing=False)
    pairs = summary.pair_list(T)
    off_diagonal = [p for p in pairs if p[0] != p[1]]
    assert len(off_diagonal) == T * (T + 1) // 2
    g = torch.Generator(device=dev).manual_seed(3)
    sub = torch.ones(N, dtype=torch.int64, device=dev)
    for K in (32, 4):
        note(f"K = {K}: recording {T + 1} labellings")
        wk.trace_open(T + 1)
        ids = []
        for j in range(T + 1):
            lab = torch.randint(1, K + 1, (N,), device=dev, generator=g)
            torch.cuda.synchronize()
            wk.set_labels_device(lab.data_ptr(), sub.data_ptr())
            wk.trace_record(j, K)
            ids.append((lab - 1).to(torch.int16))
        wk.sync()
        res = {}
        if K == 32:
            def records():
                for _ in range(a.reps):
                    wk.trace_record(T, K)
                wk.sync()
            res["record_ms"] = wall_ms(records, reps=3) / a.reps
            src, dst = torch.empty(3 * N, dtype=torch.uint8, device=dev), torch.empty(3 * N, dtype=torch.uint8, device=dev)
            res["copy_same_bytes_ms"] = event_ms(lambda: dst.copy_(src))
            res["record_over_copy"] = res["record_ms"] / res["copy_same_bytes_ms"]
            res["record_GBps"] = 6 * N / res["record_ms"] / 1e6
            if a.step_ms > 0:
                res["record_share_of_step"] = res["record_ms"] / a.step_ms
            del src, dst

        def kernel_route():
            tables = dict(zip(pairs, wk.trace_tables(pairs)))
            return wk.trace_confidence(T, list(range(T)), summary.ratio_tables(tables, T, T), device=dev)

        def tables_only():
            return wk.trace_tables(pairs)

        def torch_route():
            return [torch.bincount(ids[s].long() * K + ids[t].long(), minlength=K * K) for s, t in off_diagonal]

        def one_by_one():
            return [wk.trace_tables([p])[0] for p in off_diagonal]

        note("the kernel route")
        res["tables_and_confidence_ms"] = wall_ms(kernel_route)
        res["tables_ms"] = wall_ms(tables_only)
        note("the torch composition")
        res["torch_bincount_ms"] = event_ms(torch_route, reps=3)
        note("one call per pair")
        res["one_call_per_pair_ms"] = wall_ms(one_by_one, reps=3)
        got = tables_only()
        ref = torch_route()
        res["equal"] = all(np.array_equal(t.ravel(), r.cpu().numpy()) for (p, t), r in zip(((p, t) for p, t in zip(pairs, got) if p[0] != p[1]), ref))
        res["torch_over_kernel"] = res["torch_bincount_ms"] / res["tables_and_confidence_ms"]
        res["one_call_per_pair_over_kernel"] = res["one_call_per_pair_ms"] / res["tables_ms"]
        res["LDS_adds_per_ns"] = N * len(pairs) / res["tables_ms"] / 1e6
        out[f"K{K}"] = res
        del ids
    wk.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
