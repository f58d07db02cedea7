"""GPU test of the short-slab rule of the Python point calls (host/score.py, `Predictor._walk`): a short last slab is zero padded to
`capacity` and scored whole, and neither the results nor the counters may show it.  n = 130 points, three of them with a NaN -- in the
first, a middle and the last slab of capacity 64 (two full slabs and a short one of 2 points).  Every call with a closure of its own in
host/score.py is run at capacity 64, at 130 (no padding) and at 256 (one short slab only), from a numpy array and from a device tensor:
every output array and every counter equals that of capacity 130 from numpy, byte for byte.  No capacity rule of the worker stands in the
way of 64 / 130 / 256.  NIW: D = 4, K = 3, the regressor from features 0..2 to feature 3; Multinomial: D = 12, K = 3.  Fixed seeds."""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_countstats as G
from tools import regress_ref as rr

pytestmark = pytest.mark.gpu

DEV = G.DEV
N = 130
CAPS = (130, 64, 256)
HOLES = ((1, 5), (0, 70), (2, 129))      # (feature, point): slabs 0, 1 and the short one of capacity 64
SEED = 2024
LEVELS = (0.1, 0.5, 0.9)


@pytest.fixture(scope="module")
def host():
    from __graft_entry__ import load_package
    return importlib.import_module(load_package().__name__ + ".host")


def flat(result):
    """The fields of a result tuple (or one array, or a pair): arrays as (dtype, shape, bytes), counters as they are, None left out."""
    fields = result if isinstance(result, tuple) else (result,)
    out = []
    for f in fields:
        if f is None:
            continue
        if isinstance(f, (int, float)) or (isinstance(f, tuple) and all(isinstance(v, float) for v in f)):
            out.append(f)
            continue
        a = np.ascontiguousarray(G.as_np(f))
        out.append((str(a.dtype), a.shape, a.tobytes()))
    return out


def on(X, device):
    return torch.as_tensor(X, device=DEV) if device else X


def check_all(runs, counters):
    """runs: {(capacity, device): {call: flat result}}; every one equals that of (130, numpy)."""
    base = runs[(CAPS[0], False)]
    arrays = 0
    for key, got in runs.items():
        assert got.keys() == base.keys()
        for call in base:
            assert len(got[call]) == len(base[call]), (key, call)
            for j, (a, b) in enumerate(zip(got[call], base[call])):
                assert a == b, (key, call, j)
                arrays += isinstance(a, tuple) and isinstance(a[-1], bytes)
    for call, want in counters.items():
        assert want(base[call]), (call, [f for f in base[call] if not isinstance(f, tuple)])
    print("arrays compared:", arrays)


def test_niw_calls(host):
    post, s = rr.make_posterior(4, 3, 7)
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 3, N)
    X = (post["m"][lab] + s[lab][:, None] * rng.standard_normal((N, 4))).astype(np.float32).T.copy()      # (D, n)
    for f, i in HOLES:
        X[f, i] = np.nan
    given, y = np.ascontiguousarray(X[:3]), np.ascontiguousarray(X[3:])
    runs = {}
    for cap in CAPS:
        with host.Predictor(rr.dummy_model(post, 3, 4), capacity=cap) as p, p.regressor([0, 1, 2], [3]) as reg:
            for device in (False, True):
                r = runs[(cap, device)] = {}
                r["typicality"] = flat(p.typicality(on(X, device)))
                r["explain"] = flat(p.explain(on(X, device)))
                r["explain top"] = flat(p.explain(on(X, device), top=2))
                r["impute draws"] = flat(p.impute(on(X, device), draws=2, seed=SEED, return_components=True))
                r["predict"] = flat(reg.predict(on(given, device), return_std=True))
                r["sample"] = flat(reg.sample(on(given, device), draws=2, seed=SEED, return_components=True))
                r["cdf"] = flat(reg.cdf(on(given, device), on(y, device)))
                r["quantile"] = flat(reg.quantile(on(given, device), LEVELS))
    took_no_part = lambda fields: fields[-1] == len(HOLES)                   # noqa: E731  (skipped is the last field)
    check_all(runs, {"typicality": lambda fields: fields[-2] + fields[-1] == len(HOLES), "explain": lambda fields: fields[-2] + fields[-1] == len(HOLES),
                     "predict": took_no_part, "sample": took_no_part, "cdf": took_no_part, "quantile": lambda fields: fields[-1] == len(HOLES)})


def test_recommend(host):
    rng = np.random.default_rng(3)
    post = G.posterior(12, 3, rng)
    X = G.counts_data(post, N, rng)
    for f, i in ((4, 5), (0, 70), (11, 129)):
        X[f, i] = np.nan
    runs = {}
    for cap in CAPS:
        with G.open_predictor(host, post, cap) as p:
            for device in (False, True):
                runs[(cap, device)] = {"recommend": flat(p.recommend(on(X, device), 3)), "recommend all": flat(p.recommend(on(X, device), 3, exclude_seen=False))}
    check_all(runs, {"recommend": lambda fields: fields[-1] == 3, "recommend all": lambda fields: fields[-1] == 3})
