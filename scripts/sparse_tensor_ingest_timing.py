"""Lab script: what it costs to take sparse points from a torch.sparse_csc tensor on the GPU (dpmm_upload_points_csc_device, csrc/csc_io.hip).

   python3 scripts/sparse_tensor_ingest_timing.py [N [D [PER_POINT]]]      default: 1000000 20000 100

A synthetic canonical matrix (D x N, 50 .. 150 entries per point, Int64 indices, Float32 counts) is built on the device.  Timed, wall clock
around the call with the device idle before and after, 2 warm-up + 10 timed repetitions, median (min - max):
  (a) what a user of the host call does with such a tensor: the three .cpu() copies, the numpy conversions, upload_points_csc;
  (b) upload_points_csc alone from ready host arrays (Int64 / Int64 / Float32);
  (c) upload_points_csc_device from the tensor where it is.
For (c): achieved bytes / s on its algorithmic bytes -- the inputs read twice (check, compaction), 6 bytes written per kept entry, 12 per
point (cnt written and read, the offset written) -- against the 8 TB/s HBM peak of the MI355X.  The requirement: (c) is
faster than (b); as committed, profiles/sparse_tensor_ingest_timing.txt: 1.58 against 34.4 ms.  Run under its own `timeout`."""
import importlib
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
binding = importlib.import_module(pkg.__name__ + ".binding")
WARM, REPS = 2, 10
DEV = torch.device("cuda", 0)
HBM_PEAK = 8.0e12


def build(N, D, per):
    g = torch.Generator(device=DEV); g.manual_seed(1)
    slots = per + per // 2
    width = D // slots
    assert width >= 1
    length = torch.randint(per // 2, slots + 1, (N,), device=DEV, generator=g)
    colptr = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(length, 0, out=colptr[1:])
    rowval = torch.empty(int(colptr[-1]), dtype=torch.int64, device=DEV)
    for lo in range(0, N, 100000):                     # (slot k of a point holds one row of [k width, (k + 1) width): increasing by construction)
        hi = min(N, lo + 100000)
        cand = torch.arange(slots, device=DEV)[None, :] * width + torch.randint(0, width, (hi - lo, slots), device=DEV, generator=g)
        keep = torch.arange(slots, device=DEV)[None, :] < length[lo:hi, None]
        rowval[int(colptr[lo]):int(colptr[hi])] = cand[keep]
    nzval = torch.randint(1, 5, (rowval.numel(),), device=DEV, generator=g).float()
    return torch.sparse_csc_tensor(colptr, rowval, nzval, size=(D, N))


def timed(call):
    ms = []
    for _ in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return np.array(ms[WARM:])


def show(name, ms):
    print(f"  {name:<58s} {np.median(ms):10.2f} ms  ({ms.min():.2f} - {ms.max():.2f})", flush=True)
    return float(np.median(ms))


def main():
    a = [int(v) for v in sys.argv[1:]]
    N, D, per = (a + [1000000, 20000, 100][len(a):])[:3]
    t = build(N, D, per)
    cp, rv, nz = t.ccol_indices(), t.row_indices(), t.values()
    nnz = rv.numel()
    print(f"D = {D}, N = {N}, {nnz} entries ({nnz / N:.1f} per point), Int64 indices, Float32 values", flush=True)
    wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=1, timing=False)

    def user_route():
        wk.upload_points_csc(cp.cpu().numpy(), rv.cpu().numpy(), nz.cpu().numpy())

    h = (cp.cpu().numpy(), rv.cpu().numpy(), nz.cpu().numpy())
    ta = show("(a) .cpu() x 3 + numpy + upload_points_csc", timed(user_route))
    tb = show("(b) upload_points_csc from ready host arrays", timed(lambda: wk.upload_points_csc(*h)))
    tc = show("(c) upload_points_csc_device from the tensor", timed(lambda: wk.upload_points_csc_device(cp.data_ptr(), binding.DT_I64, rv.data_ptr(), nz.data_ptr(), binding.DT_F32, nnz, 0)))
    alg = 2 * (nnz * 12 + (N + 1) * 8) + 6 * nnz + 12 * N
    rate = alg / (tc * 1e-3)
    print(f"  (c): {alg / 1e9:.2f} GB algorithmic -> {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    print(f"  (b) / (c) = {tb / tc:.1f} x, (a) / (c) = {ta / tc:.1f} x   -- requirement (c) < (b): {'MET' if tc < tb else 'MISSED'}")
    tmp = 4 * N + 8 * ((N + 2047) // 2048 + 2)         # cnt [N] Int32 + the scan's tile totals and the two words the host reads
    print(f"  temporary device memory of (c), computed from its two allocations (not measured): {tmp} bytes ({tmp / N:.3f} per point)")
    wk.close()


if __name__ == "__main__":
    main()
