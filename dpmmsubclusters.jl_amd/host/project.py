"""Embeddings wider than the worker's 256 features: a linear projection that the model carries (include/dpmm_hip_project.h).

    P = fit_projection(X, 64)                  # PCA from a bounded subsample; X is Dimensions x Samples, any of the forms `fit` takes
    labels, *_, model = fit(X, alpha, project=P)          # the GPU reads the wide points and keeps only their 64 coordinates
    predict(model, X_new)                      # D_in-row data is projected on the way in; d-row data is taken as already projected

The basis comes from at most `sample` points through torch and numpy; the one path that scales with N -- reading the wide points and
writing the worker's own image -- is the library's kernel (csrc/project.hip).  `Projection.transform` returns those coordinates.
"""
import warnings

import numpy as np

from .. import binding
from . import points as _points
from . import priors as _priors
from . import tensors as _tensors

MAX_D_IN = binding.MAX_DIM_PROJECT_IN
MAX_D = 256


def _fix_signs(B):
    """Every column with its largest-magnitude entry (the first of equals) positive."""
    i = np.abs(B).argmax(0)
    s = np.sign(B[i, np.arange(B.shape[1])])
    s[s == 0] = 1.0
    return B * s


def _check_dims(D_in, d):
    if not (isinstance(d, (int, np.integer)) and not isinstance(d, bool)):
        raise TypeError("d must be an int")
    if D_in > MAX_D_IN:
        raise ValueError(f"D_in = {D_in} exceeds {MAX_D_IN} (DPMM_MAX_DIM_PROJECT_IN)")
    if not 1 <= d <= min(MAX_D, D_in):
        raise ValueError(f"d = {d} must be in 1..min({MAX_D}, D_in = {D_in})")


class Projection:
    """Projection(mean (D_in,), basis (D_in, d), explained_variance=None): y = basis' (x - mean).  Immutable, Float64."""

    __slots__ = ("mean", "basis", "explained_variance")

    def __init__(self, mean, basis, explained_variance=None):
        basis = np.array(basis, dtype=np.float64, order="C")
        mean = np.array(mean, dtype=np.float64).reshape(-1)
        if basis.ndim != 2 or mean.shape != (basis.shape[0],):
            raise ValueError("mean must be (D_in,) and basis (D_in, d)")
        _check_dims(basis.shape[0], basis.shape[1])
        if not (np.isfinite(basis).all() and np.isfinite(mean).all()):
            raise ValueError("mean and basis must be finite")
        ev = None if explained_variance is None else np.array(explained_variance, dtype=np.float64).reshape(-1)
        for a in (mean, basis, ev):
            if a is not None:
                a.setflags(write=False)
        object.__setattr__(self, "mean", mean)
        object.__setattr__(self, "basis", basis)
        object.__setattr__(self, "explained_variance", ev)

    def __setattr__(self, *a):
        raise AttributeError("Projection is immutable")

    __delattr__ = __setattr__

    @property
    def D_in(self):
        return self.basis.shape[0]

    @property
    def d(self):
        return self.basis.shape[1]

    def arrays(self, prefix=""):
        out = {prefix + "mean": self.mean, prefix + "basis": self.basis}
        if self.explained_variance is not None:
            out[prefix + "explained_variance"] = self.explained_variance
        return out

    @classmethod
    def from_arrays(cls, z, prefix=""):
        """The Projection stored under `prefix` in a mapping of arrays (an open .npz), or None when there is none."""
        names = z.files if hasattr(z, "files") else z
        if prefix + "basis" not in names:
            return None
        return cls(z[prefix + "mean"], z[prefix + "basis"], z[prefix + "explained_variance"] if prefix + "explained_variance" in names else None)

    def save(self, path):
        np.savez(path, **self.arrays())

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls.from_arrays(z)

    def apply(self, wk):
        """Give the worker this projection (set_projection)."""
        wk.set_projection(self.basis, self.mean)

    def transform(self, data, device=None, capacity=65536, worker_factory=None):
        """(d, n) Float32 coordinates of `data` (D_in, n), computed on the GPU in slabs of `capacity` points: projected upload, then the
        points read back.  For a tensor in device memory the result is a tensor on that device whose memory is point-major (the `.T` of
        an (n, d) tensor: what `fit` reads in place); otherwise a numpy array."""
        pts = _points.describe(data)
        cap = int(capacity)
        if cap < 1:
            raise ValueError("capacity must be at least 1")
        if pts.is_sparse:
            raise TypeError("a projection takes dense data (an array or a tensor), Dimensions x Samples")
        factory = worker_factory or binding.Worker
        pts = pts.served(factory, projected=True)      # (a stand-in worker without the device entry points: host data)
        D_in, n = pts.D, pts.N
        if D_in != self.D_in:
            raise ValueError(f"data has {D_in} rows, the projection reads {self.D_in}")
        dev = pts.device_index(device)
        dev = 0 if dev is None else dev
        d = self.d
        on_device = pts.torch_device is not None
        if on_device:
            import torch
        out = torch.empty((n, d), dtype=torch.float32, device=pts.torch_device) if on_device else np.empty((n, d), np.float32)
        pts.synchronize()
        workers = {}
        try:
            for lo in range(0, n, cap):
                m = min(cap, n - lo)
                wk = workers.get(m)
                if wk is None:
                    wk = workers[m] = factory(_priors.PRIOR_NIW, d, m, first_index=0, device=dev, seed=0)
                    self.apply(wk)
                pts.upload(wk, lo, lo + m, projected=True)
                if on_device:
                    wk.get_points_device(out.data_ptr() + 4 * lo * d, d)
                elif hasattr(wk, "get_points"):
                    out[lo:lo + m] = wk.get_points()
                else:
                    import torch
                    t = torch.empty((m, d), dtype=torch.float32, device=torch.device("cuda", int(dev or 0)))
                    torch.cuda.current_stream(t.device).synchronize()
                    wk.get_points_device(t.data_ptr(), d)
                    out[lo:lo + m] = t.cpu().numpy()
        finally:
            for wk in workers.values():
                wk.close()
        return out.T


def _as_torch(data):
    """`data` (D_in, n) as a torch tensor where it lives (a numpy array is shared, not copied)."""
    import torch
    t = _tensors.as_tensor(data)
    if t is None:
        a = np.asarray(data)
        if a.ndim != 2:
            raise ValueError("data must be 2-D, Dimensions x Samples")
        if a.dtype.name not in _tensors._DTYPE_NAMES:
            a = a.astype(np.float64)
        with warnings.catch_warnings():          # (a read-only array is only read here: no copy for the sake of torch's warning)
            warnings.simplefilter("ignore", UserWarning)
            t = torch.from_numpy(a)
    _tensors.describe(t)       # element type, layout, ndim
    return t


def fit_projection(data, d, sample=65536, seed=0, whiten=False, chunk=8192):
    """PCA of `data` (D_in, n: numpy or a torch tensor on the CPU or a GPU, any of the eight element types, any strides) to d dimensions.

    min(n, sample) points at sorted indices drawn without replacement from np.random.Generator(Philox(seed)); their mean and their
    centred Gram matrix are accumulated in Float64 with torch on the device the data lives on, in chunks of `chunk` points; the
    D_in x D_in covariance (divided by m - 1) goes through numpy.linalg.eigh on the host.  The basis is the top d eigenvectors, each with
    its largest-magnitude entry positive; whiten=True divides column j by sqrt(eigenvalue j) (ValueError if one kept is <= 0)."""
    import torch
    t = _as_torch(data)
    D_in, n = int(t.shape[0]), int(t.shape[1])
    _check_dims(D_in, d)
    if n < 1:
        raise ValueError("data has no points")
    m = min(n, int(sample))
    if m < 1:
        raise ValueError("sample must be at least 1")
    rng = np.random.Generator(np.random.Philox(int(seed)))
    idx = np.arange(n) if m == n else np.sort(rng.choice(n, size=m, replace=False))
    tidx = torch.from_numpy(idx.astype(np.int64)).to(t.device)
    total = torch.zeros(D_in, dtype=torch.float64, device=t.device)
    for lo in range(0, m, chunk):
        total += t.index_select(1, tidx[lo:lo + chunk]).to(torch.float64).sum(1)
    mean = total / m
    gram = torch.zeros((D_in, D_in), dtype=torch.float64, device=t.device)
    for lo in range(0, m, chunk):
        c = t.index_select(1, tidx[lo:lo + chunk]).to(torch.float64) - mean[:, None]
        gram += c @ c.T
    cov = (gram / max(m - 1, 1)).cpu().numpy()
    cov = (cov + cov.T) / 2
    vals, vecs = np.linalg.eigh(cov)
    vals, vecs = vals[::-1][:d].copy(), vecs[:, ::-1][:, :d].copy()
    basis = _fix_signs(vecs)
    if whiten:
        if not (vals > 0).all():
            raise ValueError("whiten=True: an eigenvalue kept is <= 0 (fewer independent directions than d)")
        basis = basis / np.sqrt(vals)
    return Projection(mean.cpu().numpy(), basis, vals)


def random_projection(D_in, d, seed=0, mean=None):
    """An orthonormal basis (D_in, d): the Q of the QR of a Gaussian matrix drawn from Philox(seed), signs fixed as fit_projection's."""
    D_in, d = int(D_in), int(d)
    _check_dims(D_in, d)
    G = np.random.Generator(np.random.Philox(int(seed))).standard_normal((D_in, d))
    Q, _ = np.linalg.qr(G)
    return Projection(np.zeros(D_in) if mean is None else mean, _fix_signs(Q))


def resolve(project, all_data, seed, comm):
    """The `project` keyword of fit / dp_parallel / resume_from_checkpoint as a Projection (None stays None)."""
    if project is None or isinstance(project, Projection):
        return project
    if isinstance(project, (int, np.integer)) and not isinstance(project, bool):
        if getattr(comm, "world", 1) > 1:
            raise ValueError("project=<int> fits a basis on this rank only: with more than one rank pass the same Projection on every rank")
        return fit_projection(all_data, int(project), seed=seed or 0)
    raise TypeError("project must be a Projection or an int (the number of dimensions to keep)")
