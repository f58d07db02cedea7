"""The data argument of `fit` / `dp_parallel` / `resume_from_checkpoint` / `predict` / `Predictor` / `Projection.transform`, described once:
`describe` recognises it (host/tensors.py, host/sparse.py) and returns a `Points` -- what it is, how large, where it lives, and how the
points [lo, hi) get into a worker.  Five kinds: a host array (a CPU tensor becomes one), a dense tensor in device memory and a
torch.sparse_csc tensor in device memory (both read in place), host CSC, and the Samples x Dimensions rows of a .npy file.  Every fall-back
for a worker that lacks an entry point (test stand-ins, third-party worker factories) is here, chosen by `hasattr` on the worker: device
data goes through the host, sparse data is made dense, .npy rows are cleaned on the host.  torch is imported only where a tensor exists.
"""
import copy

import numpy as np

from . import sparse as _sparse
from . import tensors as _tensors


class Points:
    """What every kind offers (the defaults below are those of host data):
      D, N, is_sparse, torch_device (None for host data);
      device_index(device): the index a worker for these points is created on -- the tensor's (an explicit `device` must agree), else `device`;
      synchronize(): device data is complete before the library reads it on its own stream; once before a run of uploads;
      served(target, ...): these points as `target`, a worker or a worker factory, can take them -- `self`, or, for device data and a target
        without the entry point that reads it in place, the same points as host data (the results are then numpy arrays);
      upload(wk, lo, hi, projected=False, results=False): the worker's n = hi - lo points become the points [lo, hi).  projected: D_in-wide,
        through the worker's projection; results: labels and predictions follow device data (the worker's `*_tensor` entry points);
      padded(lo, hi, cap, stages): a Predictor's short last slab -- a Points of exactly `cap` points, [lo, hi) and then zero points (empty
        columns for sparse data), built in storage that `stages.get("host" | "dev" | "csc", make, fits)` keeps for the next call."""
    is_sparse = False
    torch_device = None

    def device_index(self, device):
        return device

    def synchronize(self):
        pass

    def served(self, target, projected=False, results=False):
        return self


class _HostDense(Points):
    def __init__(self, X):
        self.X = np.asarray(X)
        if self.X.ndim != 2:
            raise ValueError("data must be 2-D, Dimensions x Samples")
        self.D, self.N = self.X.shape

    def upload(self, wk, lo, hi, projected=False, results=False):
        X = np.ascontiguousarray(self.X[:, lo:hi].T, dtype=np.float32)      # (n, D): row = point
        (wk.upload_points_projected if projected else wk.upload_points)(X)

    def padded(self, lo, hi, cap, stages):
        st = stages.get("host", lambda: np.zeros((cap, self.D), np.float32))
        st[:hi - lo] = self.X[:, lo:hi].T
        st[hi - lo:] = 0
        return _HostDense(st.T)


class _NpyRows(Points):                   # Samples x Dimensions, as stored; cleaned (NaN -> 0) and converted on the GPU by dpmm_upload_points_npy
    def __init__(self, rows):
        self.rows = rows
        self.N, self.D = rows.shape

    def upload(self, wk, lo, hi, projected=False, results=False):
        if hasattr(wk, "upload_points_npy"):
            wk.upload_points_npy(self.rows[lo:hi])
        else:
            wk.upload_points(np.nan_to_num(np.asarray(self.rows[lo:hi], dtype=np.float32), nan=0.0, posinf=np.inf, neginf=-np.inf))


class _HostCSC(Points):
    is_sparse = True

    def __init__(self, csc):
        self.csc = csc
        self.D, self.N = csc.shape

    def upload(self, wk, lo, hi, projected=False, results=False):
        if hasattr(wk, "upload_points_csc"):
            cp, rv, nz = self.csc.columns(lo, hi, check=False)     # (the device checks what it is given and names the point)
            wk.upload_points_csc(cp, rv, nz, index_base=0)         # columns [lo, hi): no rank touches another rank's entries
        else:
            wk.upload_points(self.csc.dense_rows(lo, hi))

    def padded(self, lo, hi, cap, stages):                         # empty columns behind the last point, over the same entries
        cp = self.csc.indptr
        return _HostCSC(_sparse.CSC(np.concatenate([cp[lo:hi + 1], np.full(cap - (hi - lo), cp[hi], np.int64)]), self.csc.indices,
                                    self.csc.data, (self.D, cap)))


class _OnDevice(Points):                  # over a description of host/tensors.py / host/sparse.py, whose attributes are read when asked for
    def __init__(self, desc):
        self.desc = desc

    D = property(lambda self: self.desc.shape[0])
    N = property(lambda self: self.desc.shape[1])
    torch_device = property(lambda self: self.desc.torch_device)

    def device_index(self, device):
        return _tensors.resolve_device(self.desc, device)

    def synchronize(self):
        self.desc.synchronize()

    def served(self, target, projected=False, results=False):
        return self if hasattr(target, self._entry(projected, results)) else self._on_host()


class _DeviceDense(_OnDevice):
    def _entry(self, projected, results):
        return "upload_points" + ("_projected" if projected else "") + ("_tensor" if results else "_strided_device")

    def _on_host(self, lo=0, hi=None):
        return _HostDense(self.desc.tensor[:, lo:hi].float().cpu().numpy())

    def upload(self, wk, lo, hi, projected=False, results=False):
        d = self.desc
        if not hasattr(wk, self._entry(projected, results)):
            self._on_host(lo, hi).upload(wk, 0, hi - lo, projected)
        elif results:              # points [lo, hi) where they are: an address, no copy and no slicing on the host
            (wk.upload_points_projected_tensor if projected else wk.upload_points_tensor)(d, lo, hi)
        elif projected:
            wk.upload_points_projected_strided_device(d.shard_ptr(lo), d.dtype, d.stride_point, d.stride_feature)
        else:
            wk.upload_points_strided_device(d.shard_ptr(lo), d.dtype, d.stride_point, d.stride_feature, False)

    def padded(self, lo, hi, cap, stages):
        import torch
        dev = self.torch_device
        st = stages.get("dev", lambda: torch.zeros((cap, self.D), dtype=torch.float32, device=dev), lambda st: st.device == dev)
        st[:hi - lo].copy_(self.desc.tensor[:, lo:hi].T)           # (rounds to Float32 to nearest even, as the library's own read does)
        st[hi - lo:].zero_()
        torch.cuda.current_stream(dev).synchronize()
        return _DeviceDense(_tensors.DeviceTensor(st.T, _tensors.DT_F32))


class _DeviceCSC(_OnDevice):
    is_sparse = True

    def _entry(self, projected, results):
        return "upload_points_csc_tensor" if results else "upload_points_csc_device"

    def _on_host(self):
        return _HostCSC(self.desc.to_host())

    def upload(self, wk, lo, hi, projected=False, results=False):
        d = self.desc
        if not hasattr(wk, self._entry(projected, results)):
            self._on_host().upload(wk, lo, hi)
        elif results:              # the offsets from `lo` on: an address, no copy and no slicing on the host
            wk.upload_points_csc_tensor(d, lo, hi)
        else:                      # the slab's offsets where they are, the same entry arrays
            wk.upload_points_csc_device(d.colptr_ptr(lo), d.index_dtype, d.rowval_ptr, d.nzval_ptr, d.value_dtype, d.nnz_extent, 0)

    def padded(self, lo, hi, cap, stages):                         # the slice of the offsets, then empty columns behind the last point
        import torch
        d, dev = self.desc, self.torch_device
        st = stages.get("csc", lambda: torch.empty(cap + 1, dtype=d.colptr.dtype, device=dev),
                        lambda st: st.device == dev and st.dtype == d.colptr.dtype)
        st[:hi - lo + 1].copy_(d.colptr[lo:hi + 1])
        st[hi - lo + 1:].copy_(d.colptr[hi:hi + 1].expand(cap - (hi - lo)))
        torch.cuda.current_stream(dev).synchronize()
        slab = copy.copy(d)
        slab.colptr, slab.N, slab.shape = st, cap, (d.D, cap)
        return _DeviceCSC(slab)


def describe(data, rows=None):
    """The Points of `data` (Dimensions x Samples, anything `fit` takes) -- or of `rows`, Samples x Dimensions as a .npy file holds them."""
    if rows is not None:
        return _NpyRows(rows)
    csc = _sparse.as_csc(data)
    if csc is not None:
        return _DeviceCSC(csc) if isinstance(csc, _sparse.DeviceCSC) else _HostCSC(csc)
    desc = _tensors.as_device_points(data)
    if desc is not None:
        return _DeviceDense(desc)
    return _HostDense(_tensors.as_host_array(data))
