"""The projected upload against the composition a user needs without it, on one MI355X.

For N = 1e6 and (D_in, dtype) -> d in (768, bfloat16) -> 64 and (1024, float32) -> 256, in one process:
  projected    dpmm_upload_points_projected_device from the (N, D_in) tensor (host clock around the call, which returns synchronised);
  composition  a loop over 65536-point chunks of `x.float() @ W32 - b` into an (N, d) tensor, then dpmm_upload_points_strided_device.
Both are warmed up, then timed alternately `--repeats` times; medians and the spread are printed, and one JSON line at the end.  The
share of HBM peak is the SOURCE bytes of the projected upload over its time, against 8 TB/s.

    python scripts/bench_project.py [--n 1000000] [--repeats 10] [--warmup 3]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from __graft_entry__ import load_package  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    binding = importlib.import_module(pkg.__name__ + ".binding")
    project = importlib.import_module(pkg.__name__ + ".host.project")
    dev = torch.device("cuda", 0)
    n, results = args.n, []
    for D_in, dtype, code, d in ((768, torch.bfloat16, binding.DT_BF16, 64), (1024, torch.float32, binding.DT_F32, 256)):
        x = torch.empty((n, D_in), dtype=dtype, device=dev)
        for lo in range(0, n, 65536):
            x[lo:lo + 65536] = torch.randn((min(65536, n - lo), D_in), device=dev).to(dtype)
        P = project.random_projection(D_in, d, seed=1, mean=np.linspace(-0.5, 0.5, D_in))
        W32 = torch.from_numpy(P.basis.astype(np.float32)).to(dev)
        b32 = torch.from_numpy((P.mean @ P.basis).astype(np.float32)).to(dev)
        wk = binding.Worker(binding.PRIOR_NIW, d, n, timing=False)
        wk.set_projection(P.basis, P.mean)
        y = torch.empty((n, d), dtype=torch.float32, device=dev)

        def projected():
            torch.cuda.synchronize()
            t = time.perf_counter()
            wk.upload_points_projected_strided_device(x.data_ptr(), code, D_in, 1)
            return time.perf_counter() - t

        def composition():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for lo in range(0, n, 65536):
                torch.sub(x[lo:lo + 65536].float() @ W32, b32, out=y[lo:lo + 65536])
            torch.cuda.synchronize()
            wk.upload_points_strided_device(y.data_ptr(), binding.DT_F32, d, 1)
            return time.perf_counter() - t

        for _ in range(args.warmup):
            projected(); composition()
        tp, tc = [], []
        for _ in range(args.repeats):
            tp.append(projected()); tc.append(composition())
        # the two agree to the Float32 rounding of the composition
        out = torch.empty((n, d), dtype=torch.float32, device=dev)
        projected()
        wk.get_points_device(out.data_ptr(), d)
        diff = float((out[:65536] - y[:65536]).abs().max())
        mp, mc = statistics.median(tp), statistics.median(tc)
        src_bytes = n * D_in * x.element_size()
        r = dict(D_in=D_in, dtype=str(dtype).split(".")[1], d=d, n=n, projected_ms=1e3 * mp, projected_min_ms=1e3 * min(tp), projected_max_ms=1e3 * max(tp),
                 composition_ms=1e3 * mc, composition_min_ms=1e3 * min(tc), composition_max_ms=1e3 * max(tc), source_GBps=src_bytes / mp / 1e9,
                 hbm_share=src_bytes / mp / HBM_PEAK, speedup=mc / mp, not_slower=bool(mp <= mc), max_abs_diff_first_chunk=diff)
        print(f"({D_in}, {r['dtype']}) -> {d}, N = {n}: projected {r['projected_ms']:.3f} ms [{r['projected_min_ms']:.3f}, {r['projected_max_ms']:.3f}]"
              f" = {r['source_GBps']:.0f} GB/s of source, {100 * r['hbm_share']:.1f} % of HBM peak | composition {r['composition_ms']:.3f} ms"
              f" [{r['composition_min_ms']:.3f}, {r['composition_max_ms']:.3f}] | x{r['speedup']:.2f}", flush=True)
        results.append(r)
        wk.close()
        del x, y, out
        torch.cuda.empty_cache()
    print(json.dumps(dict(bench="project", results=results)))
    return 0 if all(r["not_slower"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
