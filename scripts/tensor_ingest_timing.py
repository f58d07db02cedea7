"""Lab script: what it costs to take the points from a device tensor (dpmm_upload_points_strided_device, csrc/tensor_io.hip).

   python3 scripts/tensor_ingest_timing.py [N D] ...      default: 10000000 64  1250000 256 (the headline shape and C5's shard)

The yardstick is not the code under test: dpmm_upload_points_device on a Float32 point-major source of the same shape -- a
hipMemcpy2DAsync device to device, n D 4 bytes read and as many written -- timed in the same process and the same run.  For every
element type x {point-major, feature-major} and for one general-stride source: time, bytes read + written, achieved bytes / s and the
ratio of that rate to the yardstick's.  HIP events on the ctx stream around the call (the call ends with a synchronise of that stream, so
the interval is the queueing of the call plus its kernels; the yardstick is timed the same way), 3 warm-up + 20 timed repetitions,
median (min - max).  The bar: both main modes, for Float32 and bfloat16, reach at least half the yardstick's rate.
(As committed -- profiles/tensor_ingest_timing.txt -- the script prints MISSED for N = 1e7, D = 64: bfloat16 feature-major 0.499 x, 3.06
against 6.12 TB/s, the other three cases 0.75 - 0.81 x; MET for N = 1.25e6, D = 256, lowest 0.60 x.)
Then, end to end, the wall time from "tensor on the device" to "points in the context" through the new path and through the only
route there was before (x.float().cpu().numpy() and the host upload).  Run under its own `timeout`."""
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
WARM, REPS = 3, 20
DEV = torch.device("cuda", 0)
DTYPES = [("float16", torch.float16), ("bfloat16", torch.bfloat16), ("float32", torch.float32), ("float64", torch.float64),
          ("uint8", torch.uint8), ("int16", torch.int16), ("int32", torch.int32), ("int64", torch.int64)]      # DPMM_DT_* order


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "?"
    except Exception:  # noqa: BLE001
        return "?"


def timed(wk, call):
    """Milliseconds of WARM + REPS calls, HIP events on the ctx stream around each."""
    stream = torch.cuda.ExternalStream(wk.stream, device=DEV)
    ms = []
    for _ in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.array(ms[WARM:])


def line(name, ms, nbytes, yard_rate=None):
    med = float(np.median(ms))
    rate = nbytes / (med * 1e-3)
    txt = f"  {name:34s} {med:8.3f} ms ({ms.min():.3f} - {ms.max():.3f})   {nbytes / 1e9:6.3f} GB   {rate / 1e12:6.3f} TB/s"
    if yard_rate:
        txt += f"   {rate / yard_rate:5.2f} x yardstick"
    print(txt, flush=True)
    return rate


def shape(N, D):
    print(f"\nN = {N}, D = {D}: the ctx image is {N * D * 4 / 1e9:.3f} GB", flush=True)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, N, device=0, seed=1)
    g = torch.Generator(device=DEV).manual_seed(1)
    base = torch.randn(N, D, generator=g, device=DEV)                       # (N, D) Float32, point-major
    torch.cuda.synchronize()
    yard = line("yardstick: hipMemcpy2D d2d float32", timed(wk, lambda: wk.upload_points_device(base.data_ptr(), D)), 2 * N * D * 4)
    results = {}
    for code, (name, dt) in enumerate(DTYPES):
        src = (base * 20).to(dt) if not dt.is_floating_point else base.to(dt)
        es = src.element_size()
        for mode, v in (("point-major", src.T), ("feature-major", src.T.contiguous())):
            torch.cuda.synchronize()
            ms = timed(wk, lambda: wk.upload_points_strided_device(v.data_ptr(), code, v.stride(1), v.stride(0)))
            results[(name, mode)] = line(f"{name} {mode}", ms, N * D * (es + 4), yard) / yard
    wide = torch.randn(2 * D, 3 * (N // 8), generator=g, device=DEV)
    v = wide[::2, ::3]                                                      # general strides, an eighth of the points
    sub = pkg.Worker(pkg.PRIOR_NIW, D, v.shape[1], device=0, seed=1)
    torch.cuda.synchronize()
    ms = timed(sub, lambda: sub.upload_points_strided_device(v.data_ptr(), 2, v.stride(1), v.stride(0)))
    line(f"float32 general x[::2, ::3], n = {v.shape[1]}", ms, v.shape[1] * D * 8, yard)
    sub.close()

    ok = all(results[(t, m)] >= 0.5 for t in ("float32", "bfloat16") for m in ("point-major", "feature-major"))
    worst = min(results[(t, m)] for t in ("float32", "bfloat16") for m in ("point-major", "feature-major"))
    print(f"  bar (float32 and bfloat16, both main modes >= 0.5 x yardstick): {'MET' if ok else 'MISSED'} (lowest {worst:.2f})", flush=True)

    # end to end: tensor on the device -> points in the context
    emb = base.to(torch.bfloat16)                                           # (N, D) bfloat16 embeddings; the caller passes emb.T
    tensors = importlib_tensors()
    new, old = [], []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        desc = tensors.as_device_points(emb.T)
        desc.synchronize()
        wk.upload_points_tensor(desc, 0, N)
        new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        X = emb.T.float().cpu().numpy()                                     # the only way in before: (D, N) on the host ...
        wk.upload_points(np.ascontiguousarray(X.T, dtype=np.float32))       # ... and fit's host-side transpose and upload
        old.append(time.perf_counter() - t0)
    print(f"  end to end, bfloat16 (N, D) embeddings passed as .T: device tensor path {min(new) * 1e3:.2f} ms; through the host "
          f"{min(old) * 1e3:.1f} ms (best of 3 each; {N * D * 4 / 1e9:.2f} GB down and up the host link)", flush=True)
    wk.close()


def importlib_tensors():
    import importlib
    importlib.import_module(pkg.__name__ + ".host")
    return importlib.import_module(pkg.__name__ + ".host.tensors")


if __name__ == "__main__":
    print(f"build: commit {commit()}; {torch.cuda.get_device_name(0)}", flush=True)
    args = [int(float(a)) for a in sys.argv[1:]] or [10 ** 7, 64, 1250000, 256]
    for N, D in zip(args[0::2], args[1::2]):
        shape(N, D)
