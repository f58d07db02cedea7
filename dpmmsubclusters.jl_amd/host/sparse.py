"""Sparse count data for the Multinomial prior: compressed sparse columns, one column per point -- the D x N convention of the
reference as Julia's SparseMatrixCSC / scipy.sparse.csc_matrix of shape (D, N) hold it.  Duck typing only: nothing here imports scipy.

Accepted wherever `fit` / `dp_parallel` / `resume_from_checkpoint` / `predict` take the data array:
  * an object with `indptr`, `indices`, `data` and `shape == (D, N)` (csc_matrix / csc_array; a CSR matrix of shape (N, D) is the
    same memory and comes in through `.T`).  Made canonical on a copy when it offers `sum_duplicates()` / `sort_indices()`;
  * a tuple `(colptr, rowval, nzval, (D, N))`, 0-based, which must be canonical already (rows strictly increasing inside a column).
"""
import numpy as np


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


def as_csc(data):
    """CSC view of `data`, or None when it is not sparse input (an array goes the dense way)."""
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


def upload_columns(wk, csc, lo, hi):
    """The shard [lo, hi) into a worker: sparse where the worker can take it, else made dense on the host (test stand-ins, third-party
    worker factories) -- as the .npy path falls back."""
    if hasattr(wk, "upload_points_csc"):
        cp, rv, nz = csc.columns(lo, hi, check=False)          # (the device checks what it is given and names the point)
        wk.upload_points_csc(cp, rv, nz, index_base=0)
    else:
        wk.upload_points(csc.dense_rows(lo, hi))
