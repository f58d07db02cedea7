"""Sparse count data for the Multinomial prior: compressed sparse columns, one column per point -- the D x N convention of the
reference as Julia's SparseMatrixCSC / scipy.sparse.csc_matrix of shape (D, N) hold it.  Duck typing only: nothing here imports scipy.

Accepted wherever `fit` / `dp_parallel` / `resume_from_checkpoint` / `predict` take the data array:
  * an object with `indptr`, `indices`, `data` and `shape == (D, N)` (csc_matrix / csc_array; a CSR matrix of shape (N, D) is the
    same memory and comes in through `.T`).  Made canonical on a copy when it offers `sum_duplicates()` / `sort_indices()`;
  * a tuple `(colptr, rowval, nzval, (D, N))`, 0-based, which must be canonical already (rows strictly increasing inside a column);
  * a torch tensor of layout `torch.sparse_csc` and shape (D, N): int32 or int64 indices, values of one of the eight element types of
    host/tensors.py, 2-D, no batch or dense dimensions, not requiring grad.  A bag-of-words matrix held as `torch.sparse_csr` of shape
    (N, D) is the same memory and comes in through `.t()` (`.T` is not implemented for that layout).  Canonical already, as a tuple: a
    tensor that is not is refused by the upload, which names the point.  On a ROCm device it is described by a `DeviceCSC` and read in
    place (include/dpmm_hip_csc.h: checked, counted and compacted on the device), labels / predictions come back as tensors on that
    device; on the CPU it is the `CSC` over numpy views of its three arrays.  Other sparse layouts (COO, CSR, BSR, BSC) raise TypeError:
    `.to_sparse_csc()` converts them.  torch is never imported here: a tensor cannot exist unless the caller has done so.
"""
import sys

import numpy as np

from . import tensors as _tensors


class CSC:
    """Canonical 0-based CSC arrays of a D x N matrix."""

    def __init__(self, indptr, indices, data, shape):
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.indices = indices
        self.data = data
        self.shape = (int(shape[0]), int(shape[1]))
        D, N = self.shape
        if self.indptr.ndim != 1 or self.indptr.size != N + 1:
            raise ValueError(f"sparse data: colptr has {self.indptr.size} entries, shape {self.shape} needs {N + 1}")
        if len(self.indices) != len(self.data):
            raise ValueError("sparse data: rowval and nzval differ in length")
        dec = np.nonzero(np.diff(self.indptr) < 0)[0]
        if dec.size:
            raise ValueError(f"sparse data: colptr decreases at point {int(dec[0])}")
        if self.indptr[0] < 0 or self.indptr[-1] > len(self.indices):
            raise ValueError("sparse data: colptr points outside rowval / nzval")

    def columns(self, lo, hi, check=True):
        """(colptr, rowval Int64, nzval Float32) of the columns [lo, hi): a slice of colptr with the slice of the entries it spans
        (colptr keeps its offsets: entry e of the slice is colptr[i] - colptr[0]).  Only these entries are touched."""
        cp = self.indptr[lo:hi + 1]
        a, b = (int(cp[0]), int(cp[-1])) if cp.size else (0, 0)
        rv = np.ascontiguousarray(self.indices[a:b], dtype=np.int64)
        nz = np.ascontiguousarray(self.data[a:b], dtype=np.float32)
        if check and rv.size:
            D = self.shape[0]
            col = np.repeat(np.arange(hi - lo), np.diff(cp))             # point of every entry
            oob = np.nonzero((rv < 0) | (rv >= D))[0]
            if oob.size:
                raise ValueError(f"sparse data: point {lo + int(col[oob[0]])}: row index out of range")
            bad = np.nonzero((np.diff(rv) <= 0) & (col[1:] == col[:-1]))[0]
            if bad.size:
                raise ValueError(f"sparse data: point {lo + int(col[bad[0] + 1])}: row indices are not strictly increasing "
                                 "(unsorted or duplicate)")
        return cp, rv, nz

    def dense_rows(self, lo, hi):
        """The columns [lo, hi) as the (n, D) Float32 rows `upload_points` takes (workers without a sparse upload)."""
        cp, rv, nz = self.columns(lo, hi)
        X = np.zeros((hi - lo, self.shape[0]), np.float32)
        X[np.repeat(np.arange(hi - lo), np.diff(cp)), rv] = nz
        return X


class DeviceCSC:
    """A (D, N) torch.sparse_csc tensor in device memory: the addresses of its three arrays, their element types and how many entries lie
    behind rowval / nzval.  The offsets are absolute into the entries, so the columns [lo, hi) are `colptr_ptr(lo)` with the same two
    entry addresses."""

    def __init__(self, tensor, index_dtype, value_dtype):
        self.tensor = tensor                       # keeps the memory alive for as long as the description is
        self.shape = (int(tensor.shape[0]), int(tensor.shape[1]))
        self.D, self.N = self.shape
        self.colptr, self.rowval, self.nzval = tensor.ccol_indices(), tensor.row_indices(), tensor.values()
        if not (self.colptr.is_contiguous() and self.rowval.is_contiguous() and self.nzval.is_contiguous()):
            raise TypeError("sparse tensor data: the index and value arrays must be contiguous")
        self.index_dtype, self.value_dtype = index_dtype, value_dtype
        self.index_itemsize = _tensors.ITEMSIZE[index_dtype]
        self.nnz_extent = int(self.rowval.numel())
        self.rowval_ptr = int(self.rowval.data_ptr()) if self.nnz_extent else 0
        self.nzval_ptr = int(self.nzval.data_ptr()) if self.nnz_extent else 0
        self.torch_device = tensor.device
        self.device_index = tensor.device.index if tensor.device.index is not None else 0

    def colptr_ptr(self, lo):
        """Address of point `lo`'s offset: the first of hi - lo + 1 offsets of the columns [lo, hi)."""
        return int(self.colptr.data_ptr()) + int(lo) * self.index_itemsize

    def synchronize(self):
        """The tensor's arrays must be complete before the library reads them on its own stream."""
        import torch
        torch.cuda.current_stream(self.torch_device).synchronize()

    def to_host(self):
        """The same matrix as a host `CSC` (workers without the device entry point)."""
        return _torch_csc_host(self.tensor.cpu(), self.value_dtype)


def _torch_csc_host(t, value_dtype):
    vals = t.values()
    return CSC(t.ccol_indices().numpy(), t.row_indices().numpy(), (vals.float() if value_dtype == _tensors.DT_BF16 else vals).numpy(), t.shape)


def _torch_sparse(data):
    """`data` as CSC / DeviceCSC when it is a torch tensor of a sparse layout (TypeError where it cannot be taken); None otherwise."""
    torch = sys.modules.get("torch")
    if torch is None or not isinstance(data, torch.Tensor) or data.layout == torch.strided:
        return None
    if data.layout != torch.sparse_csc:
        raise TypeError(f"sparse tensor data must be of layout torch.sparse_csc and shape (D, N); got {data.layout} -- "
                        "tensor.to_sparse_csc() converts it (a sparse_csr tensor of shape (N, D) comes in as tensor.t())")
    if data.requires_grad:
        raise TypeError("tensor data requires grad: pass tensor.detach()")
    vals = data.values()
    if data.ndim != 2 or vals.ndim != 1 or data.ccol_indices().ndim != 1:
        raise TypeError("sparse tensor data must be 2-D, Dimensions x Samples, without batch or dense dimensions")
    value_dtype = _tensors._dtype_code(torch, vals.dtype)
    index_dtype = _tensors._dtype_code(torch, data.ccol_indices().dtype)
    if index_dtype not in (_tensors.DT_I32, _tensors.DT_I64):
        raise TypeError("sparse tensor data: indices must be int32 or int64")
    if data.device.type == "cpu":
        return _torch_csc_host(data, value_dtype)
    if data.device.type != "cuda":
        raise TypeError(f"tensor data lives on device {data.device}: a ROCm device or the CPU is needed")
    return DeviceCSC(data, index_dtype, value_dtype)


def as_csc(data):
    """CSC view of `data` (a DeviceCSC for a sparse_csc tensor in device memory), or None when it is not sparse input (an array goes the
    dense way)."""
    t = _torch_sparse(data)
    if t is not None:
        return t
    if isinstance(data, tuple) and len(data) == 4 and isinstance(data[3], (tuple, list)) and len(data[3]) == 2:
        return CSC(data[0], data[1], data[2], data[3])
    if all(hasattr(data, a) for a in ("indptr", "indices", "data", "shape")) and not isinstance(data, np.ndarray):
        if getattr(data, "format", "csc") != "csc":
            if not hasattr(data, "tocsc"):
                raise TypeError("sparse data must be compressed sparse columns of shape (D, N)")
            data = data.tocsc()
        canonical = getattr(data, "has_canonical_format", None)
        if canonical is False or (canonical is None and getattr(data, "has_sorted_indices", True) is False):
            if hasattr(data, "copy") and (hasattr(data, "sum_duplicates") or hasattr(data, "sort_indices")):
                data = data.copy()
                if hasattr(data, "sum_duplicates"):
                    data.sum_duplicates()            # (sorts as well)
                else:
                    data.sort_indices()
        return CSC(data.indptr, data.indices, data.data, data.shape)
    return None
