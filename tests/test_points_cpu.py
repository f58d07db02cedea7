"""host/points.py: what a worker is asked when data of every kind goes through `fit`, `predict`, a `Predictor` and `Projection.transform`.

A recording stand-in worker logs every call (method, the shapes and element types of its array arguments, its scalars).  The logs of
the whole product -- entry point x kind of input x model x what the worker can take x n -- are kept in tests/golden/points_calls.json,
written by `python tests/test_points_cpu.py` from the code before the input's description moved into one module; the test asserts that
the calls are still those.  A combination that is refused is recorded as the exception's type and text, after the calls made so far.

Sizes: D = 3 (or D_in = 5 projected to d = 3), capacity 4, n in {0, 1, 4, 5, 9}: no point, one short slab, one full slab, full + short,
two full + short.  A tensor in device memory is a stub description (`Stub`) handed out by a patched `tensors.as_device_points`, the idiom
of tests/test_score_cpu.py; its "device" is the CPU, so the full-capability worker sees the in-place calls and the staging of a short
slab, and the others the fall-back through the host."""
import importlib
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fake_worker import FakeWorker      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "points_calls.json")
D, D_IN, CAP, K = 3, 5, 4, 2
SIZES = (0, 1, 4, 5, 9)
STUB_BASE = 1 << 48                     # the stub's "addresses": above anything a process maps, so the log tells them from real ones


def _host():
    from __graft_entry__ import load_package
    load_package()
    return importlib.import_module("dpmmsubclusters_jl_amd.host")


# ---------------------------------------------------------------------------------------------- the log
LOG = []


def _d(x):
    """What the log keeps of an argument: shapes and element types of arrays, scalars as they are, addresses by their origin."""
    if isinstance(x, np.ndarray):
        return f"{x.dtype}{list(x.shape)}"
    if isinstance(x, torch.Tensor):
        return f"{x.dtype}{list(x.shape)}"
    if isinstance(x, (bool, str)) or x is None:
        return x
    if isinstance(x, (int, np.integer)):
        x = int(x)
        return f"stub+{x - STUB_BASE}" if x >= STUB_BASE else "address" if x >= 1 << 32 else x
    if isinstance(x, (float, np.floating)):
        return float(x)
    if isinstance(x, dict):
        return {str(k): _d(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_d(v) for v in x]
    if isinstance(x, torch.device):
        return str(x)
    return type(x).__name__


def _logged(name, fn):
    def call(self, *a, **k):
        LOG.append([name] + [_d(v) for v in a] + ([_d(k)] if k else []))
        return fn(self, *a, **k)
    call.__name__ = name
    return call


# ---------------------------------------------------------------------------------------------- the recording worker
class _Base(FakeWorker):
    """The oracle-backed stand-in (so that `fit` runs a sweep) with the calls of predict / Predictor / transform answered by zeros."""

    def __init__(self, prior, D, n_local, first_index=0, device=0, seed=0):
        super().__init__(prior, D, n_local, first_index=first_index, device=device, seed=seed)
        self.W = self.mu = None

    def close(self):
        pass

    def set_option(self, option, value):
        pass

    def set_projection(self, W, mu=None):
        self.W = np.asarray(W, np.float64)
        self.mu = np.zeros(self.W.shape[0]) if mu is None else np.asarray(mu, np.float64)

    def set_predictive_niw(self, m, R, logdet, df, weights):
        self.K = len(weights)

    def set_predictive_mult(self, logp, weights):
        self.K = len(weights)

    def predict_table_niw(self, m, R, logdet, df, weights, points=False):
        return np.zeros((len(weights), self.n), np.float32)

    def predict_table_mult(self, logp, weights, points=False):
        return np.zeros((len(weights), self.n), np.float32)

    def score_points_into(self, outs, m=0):
        for name, arr in outs.items():
            assert arr.shape[0] == self.n, (name, arr.shape)
            arr[...] = 0

    def score_missing_counts(self):
        return (0, 0)

    def impute_points_into(self, out):
        assert tuple(out.shape) == (self.n, self.D)
        out[...] = 0

    def rank_begin(self, m, which):
        self.m = int(m)

    def rank_accumulate(self, index_base, n_valid):
        assert 0 <= n_valid <= self.n

    def rank_read(self, device=None):
        r = {k: np.zeros((self.K, self.m), dt) for k, dt in (("typ_idx", np.int64), ("typ_score", np.float32), ("fringe_idx", np.int64),
                                                             ("fringe_score", np.float32))}
        r["count"], r["skipped"] = np.zeros(self.K, np.int64), np.zeros(1, np.int64)
        return r

    def get_points(self):
        return np.zeros((self.n, self.D), np.float32)

    def get_points_device(self, ptr, ld_out):
        pass


for _name in sorted({n for c in (FakeWorker, _Base) for n, f in vars(c).items() if callable(f) and (not n.startswith("_") or n == "__init__")}):
    setattr(_Base, _name, _logged(_name, getattr(_Base, _name)))


class _Uploads:
    """Every upload entry point of binding.Worker; each leaves the (n, D) Float32 points in self.X, as `upload_points` does."""

    def upload_points(self, X):
        X = np.asarray(X)
        assert X.shape == (self.n, self.D) and X.dtype == np.float32, (X.shape, X.dtype)      # never a short upload
        self.X = np.ascontiguousarray(X)

    def upload_points_npy(self, rows, nan_to_zero=True):
        assert rows.shape[0] == self.n and rows.shape[1] >= self.D
        self.X = np.ascontiguousarray(np.nan_to_num(np.asarray(rows, np.float32), nan=0.0, posinf=np.inf, neginf=-np.inf))

    def upload_points_csc(self, colptr, rowval, nzval, index_base=0):
        assert len(colptr) == self.n + 1 and len(rowval) == len(nzval)
        cp = np.asarray(colptr, np.int64) - int(colptr[0])
        self.X = np.zeros((self.n, self.D), np.float32)
        self.X[np.repeat(np.arange(self.n), np.diff(cp)), np.asarray(rowval, np.int64)[:cp[-1]]] = np.asarray(nzval, np.float32)[:cp[-1]]

    def upload_points_strided_device(self, ptr, dtype, stride_point, stride_feature, nan_to_zero=False):
        self.X = np.zeros((self.n, self.D), np.float32)

    def upload_points_tensor(self, desc, lo, hi):
        assert hi - lo == self.n and desc.D == self.D
        self.X = np.ascontiguousarray(desc.tensor[:, lo:hi].T.float().numpy())

    def upload_points_csc_device(self, colptr_ptr, index_dtype, rowval_ptr, nzval_ptr, value_dtype, nnz_extent, index_base=0):
        self.X = np.zeros((self.n, self.D), np.float32)

    def upload_points_csc_tensor(self, desc, lo, hi):
        assert hi - lo == self.n and desc.D == self.D
        self.X = np.zeros((self.n, self.D), np.float32)

    def _project(self, X):
        assert self.W is not None and X.shape == (self.n, self.W.shape[0]), X.shape
        self.X = (X.astype(np.float64) @ self.W - self.mu @ self.W).astype(np.float32)

    def upload_points_projected(self, X):
        X = np.asarray(X)
        assert X.dtype == np.float32, X.dtype
        self._project(X)

    def upload_points_projected_strided_device(self, ptr, dtype, stride_point, stride_feature):
        self._project(np.zeros((self.n, self.W.shape[0]), np.float32))

    def upload_points_projected_tensor(self, desc, lo, hi):
        assert hi - lo == self.n
        self._project(desc.tensor[:, lo:hi].T.float().numpy())


CAPABILITY = {
    "all": [n for n in vars(_Uploads) if n.startswith("upload_")],
    "plain": ["upload_points"],
    "plain+projected": ["upload_points", "upload_points_projected"],
}
WORKERS = {cap: type("Recorder_" + cap.replace("+", "_"), (_Base,),
                     dict({n: _logged(n, vars(_Uploads)[n]) for n in names}, _project=_Uploads._project))
           for cap, names in CAPABILITY.items()}


# ---------------------------------------------------------------------------------------------- the inputs
class Stub:
    """What the package reads of a tensors.DeviceTensor, over a Float32 tensor on the CPU whose memory is point-major."""
    dtype, itemsize, device_index, data_ptr = 2, 4, 0, STUB_BASE

    def __init__(self, X):
        self.tensor = torch.from_numpy(np.ascontiguousarray(X.T)).T
        self.shape = (self.D, self.N) = tuple(int(v) for v in X.shape)
        self.stride_feature, self.stride_point = (int(v) for v in self.tensor.stride())
        self.torch_device = torch.device("cpu")

    def shard_ptr(self, lo):
        return self.data_ptr + int(lo) * self.stride_point * self.itemsize

    def synchronize(self):
        pass


class OnTheStub:
    """The object that stands for a tensor in device memory: the patched `as_device_points` answers it with its Stub."""

    def __init__(self, X):
        self.stub = Stub(X)


DENSE = ("numpy", "f32", "bf16", "stub")
SPARSE = ("csc", "torch_csc")
INPUTS = DENSE + SPARSE


def values(rows, n):
    """(rows, n) Float32 small counts: exact in bfloat16, valid for both priors."""
    return np.random.default_rng(100 * rows + n).integers(0, 4, (rows, n)).astype(np.float32)


def make_input(kind, X):
    if kind == "numpy":
        return X.astype(np.float64)
    if kind == "f32":
        return torch.from_numpy(X.copy())
    if kind == "bf16":
        return torch.from_numpy(X.copy()).to(torch.bfloat16)
    if kind == "stub":
        return OnTheStub(X)
    n = X.shape[1]
    cp = np.concatenate([[0], np.cumsum((X != 0).sum(0))]).astype(np.int64)
    rv = np.concatenate([np.flatnonzero(X[:, i]) for i in range(n)] + [np.zeros(0, np.int64)]).astype(np.int64)
    nz = np.concatenate([X[X[:, i] != 0, i] for i in range(n)] + [np.zeros(0, np.float32)]).astype(np.float32)
    if kind == "csc":
        return (cp, rv, nz, X.shape)
    return torch.sparse_csc_tensor(torch.from_numpy(cp), torch.from_numpy(rv), torch.from_numpy(nz), size=X.shape)


# ---------------------------------------------------------------------------------------------- the models
def projection(host):
    return host.project.random_projection(D_IN, D, seed=1, mean=np.linspace(-1, 1, D_IN))


def hyper(host, model):
    return host.multinomial_hyper(np.ones(D)) if model == "mult" else host.niw_hyperparams(1.0, np.zeros(D), D + 3, np.eye(D))


def fitted(host, model):
    """What predict and a Predictor read of a fitted model."""
    rng = np.random.default_rng(7)
    if model == "mult":
        post = dict(alpha=(1 + rng.random((3 * K, D))).astype(np.float32))
    else:
        A = rng.standard_normal((3 * K, D, D)) * 0.1 + np.eye(D)
        post = dict(kappa=1 + rng.random(3 * K), nu=D + 3 + rng.random(3 * K), m=rng.standard_normal((3 * K, D)), U=np.triu(A) + 2 * np.eye(D),
                    logdet_psi=np.zeros(3 * K))
    s = types.SimpleNamespace(K=K, prior=hyper(host, model), post=post, alpha=10.0, points_count=np.array([5, 7]), wk=types.SimpleNamespace(device=0))
    return types.SimpleNamespace(sampler=s, projection=projection(host) if model == "niw+proj" else None)


def models_of(kind):
    return ("niw", "niw+proj") if kind in DENSE else ("mult", "niw", "niw+proj")


PARAMS = """
data_path = {path!r}
data_prefix = "pts"
iterations = 1
initial_clusters = 1
random_seed = 3
burnout_period = 1
α = 10.0
hyper_params = DPMMSubClusters.niw_hyperparams(1.0, zeros(3), 6, eye(3))
enable_saving = false
"""


# ---------------------------------------------------------------------------------------------- one case
def run(host, entry, kind, model, cap, n, tmp):
    """The log of one combination, ending with what came back or what was raised."""
    factory = WORKERS[cap]
    rows = D_IN if model == "niw+proj" or entry == "transform" else D
    data = None if kind == "npy" else make_input(kind, values(rows, n))
    del LOG[:]
    try:
        if entry == "fit" and kind == "npy":
            rowsfile = values(D, n).T.astype(np.float64)
            rowsfile[:1, 0] = np.nan
            os.makedirs(tmp, exist_ok=True)
            np.save(os.path.join(tmp, "pts.npy"), rowsfile)
            with open(os.path.join(tmp, "params.py"), "w") as f:
                f.write(PARAMS.format(path=tmp + "/"))
            out = host.dp_parallel(os.path.join(tmp, "params.py"), verbose=False, worker_factory=factory, nthreads=1)[0].labels
        elif entry == "fit":
            kw = dict(project=projection(host)) if model == "niw+proj" else {}
            out = host.fit(data, hyper(host, model), 10.0, iters=1, seed=3, burnout=1, verbose=False, worker_factory=factory, nthreads=1, **kw)[0]
        elif entry == "predict":
            out = host.predict(fitted(host, model), data, worker_factory=factory)
        elif entry == "transform":
            out = projection(host).transform(data, capacity=CAP, worker_factory=factory)
        else:
            with host.Predictor(fitted(host, model), capacity=CAP, worker_factory=factory) as p:
                out = p.predict(data) if entry == "Predictor.predict" else p.impute(data) if entry == "Predictor.impute" else p.exemplars(data, 2)
                LOG.append(["missing_counts", _d(p.missing_counts)])
        LOG.append(["returns", _d(out)])
    except Exception as e:  # noqa: BLE001
        LOG.append(["raises", type(e).__name__, str(e)])
    return list(LOG)


ENTRIES = ("fit", "predict", "Predictor.predict", "Predictor.impute", "Predictor.exemplars", "transform")
GROUPS = [(e, k) for e in ENTRIES for k in (DENSE if e == "transform" else INPUTS)] + [("fit", "npy")]


def models_for(entry, kind):
    return ("niw",) if kind == "npy" else ("niw+proj",) if entry == "transform" else models_of(kind)


def group(host, entry, kind, tmp, monkeypatch):
    """{"model capability": [the log for every n of SIZES]} of one entry point and one kind of input."""
    T = host.tensors
    real = T.as_device_points
    monkeypatch.setattr(T, "as_device_points", lambda data: data.stub if isinstance(data, OnTheStub) else real(data))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(synchronize=lambda: None))
    return {f"{model} {cap}": [run(host, entry, kind, model, cap, n, tmp) for n in SIZES] for model in models_for(entry, kind) for cap in CAPABILITY}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("entry,kind", GROUPS)
def test_the_worker_sees_the_calls_it_saw(entry, kind, golden, tmp_path, monkeypatch):
    want = golden["cases"][f"{entry} {kind}"]
    got = group(_host(), entry, kind, str(tmp_path), monkeypatch)
    assert sorted(got) == sorted(want) == sorted(f"{m} {c}" for m in models_for(entry, kind) for c in CAPABILITY)
    for key, logs in got.items():
        for n, log, i in zip(SIZES, logs, want[key]):
            assert json.loads(json.dumps(log)) == golden["logs"][i], (entry, kind, key, n)


def test_the_fixture_holds_exactly_these_groups(golden):
    assert sorted(golden["cases"]) == sorted(f"{e} {k}" for e, k in GROUPS)
    assert all(len(v) == len(SIZES) for g in golden["cases"].values() for v in g.values())


def test_the_description_imports_without_torch():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; load_package(); import importlib; "
            "importlib.import_module('dpmmsubclusters_jl_amd.host.points'); assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


if __name__ == "__main__":              # writes the fixture: run on the code whose calls are the reference
    import tempfile
    host = _host()
    mp = pytest.MonkeyPatch()
    logs, index, cases = [], {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for entry, kind in GROUPS:
            got = group(host, entry, kind, tmp, mp)
            mp.undo()
            for key, per_n in got.items():
                for j, log in enumerate(per_n):
                    text = json.dumps(log, separators=(",", ":"))
                    if text not in index:
                        index[text] = len(logs)
                        logs.append(text)
                    per_n[j] = index[text]
            cases[f"{entry} {kind}"] = got
    with open(GOLDEN, "w") as f:
        f.write('{"logs": [\n' + ",\n".join(logs) + '\n],\n"cases": {\n'
                + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in cases.items()) + "\n}}\n")
    print(sum(len(v) for g in cases.values() for v in g.values()), "cases,", len(logs), "distinct logs,", os.path.getsize(GOLDEN), "bytes")
