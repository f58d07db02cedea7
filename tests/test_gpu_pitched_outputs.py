"""GPU tests of the pitched outputs of the table calls: every call whose rows the caller may pitch wider than their payload -- regress_points,
regress_cdf_points, regress_quantile_points, recommend_points, count_explain_points, impute_points, explain_points, explain_groups_points,
regress_draw_points, impute_draws -- through its `_into` binding, into storage whose rows are PAD words wider than the payload and
prefilled with a sentinel, host variant (numpy) and device variant (tensor).

Asserted: the two variants agree byte for byte over the whole array, the padding is zero -- explain_points and explain_groups_points leave
it alone instead: there it still holds the sentinel --, the payload has the bits of the unpadded call, `skipped` and labels / components
agree.  No reference beyond the library's own unpadded call is needed: what that call computes is the subject of the tests of each
feature.  Shapes: NIW (D_o, D_t, K) = (5, 33, 3) -- a second block of targets that holds one target -- and NIW D = 5, K = 3 for the
explanations and the imputation; count data D = 40, K = 3; n = two ranges of the smallest table budget plus 33 points, so that the last
range is ragged and its last 32-point tile too; one point with a NaN feature (it takes no part), a few for the imputation.  The stacked layout of the draws (draw_stride >= n ld), which the bindings do
not reach, goes through the C entry points once each and must equal the interleaved result transposed."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import test_gpu_countstats as G
import test_gpu_score as S
from tools import regress_cdf_ref as rc
from tools import regress_ref as rr

pytestmark = pytest.mark.gpu

PAD = 3
N = 2 * 256 + 33                          # the smallest range of an NIW table with D <= 64 is 256 points
SENTINEL = 0x7FA5A5A5                     # a NaN pattern no kernel writes; as int32 no feature index either
LEVELS = (0.1, 0.5, 0.9)
DRAWS = 3
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def binding(pkg):
    return importlib.import_module(pkg.__name__ + ".binding")


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


def fresh(shape, dtype, device):
    """Storage prefilled with the sentinel: a numpy array, or a tensor on the GPU."""
    a = np.full(shape, SENTINEL, np.int32).view(np.float32 if dtype == "float32" else np.int32)
    if dtype in ("int64", "float64"):
        a = np.full(shape, -7, dtype)
    return torch.as_tensor(a, device=DEV) if device else a


def raw(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype.itemsize == 8 else np.uint32)


def both(call, shapes, keep=False):
    """call(outs) -> skipped with outs made by `shapes` = [(name, shape without the last axis, payload width of a row or None, dtype)], three
    times: unpadded on the host, padded on the host, padded on the device.  Checks what the module's docstring lists; returns the unpadded
    outputs.  keep: the call leaves the words behind the payload alone, in both variants."""
    runs = []
    for pad, device in ((0, False), (PAD, False), (PAD, True)):
        outs = {name: fresh(lead + ((w + pad,) if w else ()), dt, device) for name, lead, w, dt in shapes}
        runs.append((outs, call(outs)))
    (plain, sk), (hostp, sk_h), (devp, sk_d) = runs
    assert sk == sk_h == sk_d
    for name, lead, w, dt in shapes:
        assert np.array_equal(raw(hostp[name]), raw(devp[name])), name
        if w:
            assert np.array_equal(raw(hostp[name][..., :w]), raw(plain[name])), name
            if keep:
                assert (raw(hostp[name][..., w:]) == SENTINEL).all() and (raw(devp[name][..., w:]) == SENTINEL).all(), name
                assert np.array_equal(raw(devp[name][..., :w]), raw(hostp[name][..., :w])), name
            else:
                assert not raw(hostp[name][..., w:]).any(), name
        else:
            assert np.array_equal(raw(hostp[name]), raw(plain[name])), name
    return plain, sk


def stacked(wk, fn, n, w, seed, extra):
    """The C entry point `fn` (host variant) with the draws stacked: out (DRAWS, n, w + PAD), ld = w + PAD, draw_stride = n ld."""
    out, comp = fresh((DRAWS, n, w + PAD), "float32", False), fresh((DRAWS, n), "int32", False)
    wk._chk(fn(wk._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), w + PAD, n * (w + PAD), ctypes.c_void_p(comp.ctypes.data), ctypes.c_uint64(seed), 0, 1, DRAWS,
               *extra))
    return out, comp


def test_niw_calls(pkg, binding, host):
    score = importlib.import_module(pkg.__name__ + ".host.score")
    c = rc.make_case(5, 33, 3, N)
    Dt, n = 33, N
    X, Y = c["X"].copy(), c["Y"].copy()
    X[N - 2, 1] = np.nan                                   # in the last, ragged tile: takes no part
    data, y = np.ascontiguousarray(X.T), np.ascontiguousarray(Y)
    parent = score.Predictor(rr.dummy_model(c["post"], c["K"], c["D"]), capacity=n)
    reg = parent.regressor(c["given"], c["targets"])
    with parent, reg:
        wk = reg.marginal._wk
        wk.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)   # a range is one tile of the sweep
        pred, qs = reg.predict(data, return_std=True), reg.quantile(data, LEVELS)      # tables and levels in force, the points uploaded
        assert pred.skipped == 1 and wk.n == n

        plain, sk = both(lambda o: wk.regress_points_into(o["mean"], o["std"], o["labels"]),
                         [("mean", (n,), Dt, "float32"), ("std", (n,), Dt, "float32"), ("labels", (n,), None, "int64")])
        assert sk == 1 and np.array_equal(raw(plain["mean"].T), raw(pred.mean)) and np.array_equal(plain["labels"], pred.labels)

        def cdf(o):
            yy = o["cdf"].new_zeros(o["cdf"].shape) if hasattr(o["cdf"], "new_zeros") else np.zeros_like(o["cdf"])
            yy[:, :Dt] = torch.as_tensor(y, device=DEV) if hasattr(yy, "cpu") else y      # y pitched like the outputs
            return wk.regress_cdf_points_into(yy, o["cdf"], o["sf"], o["labels"])
        plain, sk = both(cdf, [("cdf", (n,), Dt, "float32"), ("sf", (n,), Dt, "float32"), ("labels", (n,), None, "int64")])
        assert sk == 1 and np.array_equal(plain["labels"], pred.labels) and np.isnan(plain["cdf"][N - 2]).all()

        plain, sk = both(lambda o: wk.regress_quantile_points_into(o["out"], o["labels"]),
                         [("out", (n, len(LEVELS)), Dt, "float32"), ("labels", (n,), None, "int64")])
        assert sk == 1 and np.array_equal(raw(plain["out"].transpose(1, 2, 0)), raw(qs.values))

        plain, sk = both(lambda o: wk.regress_draw_points_into(o["out"], 11, 0, draw0=1, comp=o["comp"]),
                         [("out", (n, DRAWS), Dt, "float32"), ("comp", (DRAWS, n), None, "int32")])
        assert sk == 1 and (plain["comp"][:, N - 2] == -1).all()
        skipped = np.zeros(1, np.int64)
        out, comp = stacked(wk, wk._lib.dpmm_regress_draw_points, n, Dt, 11, (skipped.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),))
        assert skipped[0] == 1 and np.array_equal(comp, plain["comp"])
        assert np.array_equal(raw(out[..., :Dt].transpose(1, 0, 2)), raw(plain["out"])) and not raw(out[..., Dt:]).any()

        # ---- imputation draws of the full table (D = 38) with gaps, on the parent Predictor
        D = c["D"]
        full = np.empty((D, n), np.float32)
        full[c["given"]], full[c["targets"]] = c["X"].T, c["Y"].T
        full[3, 5] = full[0, 300] = full[7, 300] = full[2, N - 1] = np.nan
        pw = parent._wk
        pw.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)
        drawn = parent.impute(full, draws=DRAWS, seed=5, return_components=True)       # uploads the points
        plain, _ = both(lambda o: pw.impute_draws_into(o["out"], 5, 0, draw0=1, comp=o["comp"]),
                        [("out", (n, DRAWS), D, "float32"), ("comp", (DRAWS, n), None, "int32")])
        assert np.array_equal(raw(plain["out"][:, 0, :].T), raw(drawn[0][1])) and (plain["comp"][:, 300] >= 0).all() and (plain["comp"][:, 6] == -1).all()
        out, comp = stacked(pw, pw._lib.dpmm_impute_draw_points, n, D, 5, ())
        assert np.array_equal(comp, plain["comp"])
        assert np.array_equal(raw(out[..., :D].transpose(1, 0, 2)), raw(plain["out"])) and not raw(out[..., D:]).any()


def test_recommend(binding, host):
    rng = np.random.default_rng(40)
    post = G.posterior(40, 3, rng)
    X = G.counts_data(post, N, rng).astype(np.float32)
    X[4, N - 2] = np.nan                                   # (D, n): a feature of a point of the last tile
    m = 3
    with G.open_predictor(host, post, N, binding=binding) as p:
        p._wk.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)
        got = p.recommend(X, m)                           # the table of set_recommend in force, the points uploaded
        wk = p._wk
        plain, sk = both(lambda o: wk.recommend_points_into(o, m),
                         [("features", (N,), m, "int32"), ("prob", (N,), m, "float32"), ("labels", (N,), None, "int64")])
    assert sk == got.skipped == 1
    assert np.array_equal(plain["features"], got.features) and np.array_equal(raw(plain["prob"]), raw(got.prob)) and np.array_equal(plain["labels"], got.labels)


@pytest.fixture(scope="module")
def niw5(pkg, binding):
    """(worker, its predictive parameters, the points (n, D)): NIW D = 5, K = 3, N points in three ranges, four of them with gaps."""
    D, K = 5, 3
    rng = np.random.default_rng(77)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X[5, 3] = X[300, 0] = X[300, 2] = X[N - 2, 1] = X[N - 1, 2] = np.nan
    wk = pkg.Worker(pkg.PRIOR_NIW, D, N, device=0, seed=1)
    wk.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)       # a range is one tile of the sweep
    wk.upload_points(X)
    pars = S.niw_params(rng, D, K)
    wk.set_predictive_niw(*pars)
    yield wk, pars, X
    wk.close()


VECTORS = [("labels", (N,), None, "int64"), ("mahalanobis", (N,), None, "float32"), ("tail", (N,), None, "float32")]


@pytest.mark.parametrize("top", [2, 0])
def test_explain_rows_keep_the_words_behind(niw5, top):
    """explain_points, top = 2 and top = 0 (rows of D entries).  Host variant: the words behind the payload are not written.  Device variant:
    the kernels write the payload only, so the sentinel stays there too (what the library did before the rows went through the shared
    staging, recorded on that commit) and the two variants agree over the whole array."""
    wk, _, X = niw5
    w = top or X.shape[1]
    rows = [(name, (N,), w, "float32") for name in ("residual", "zscore", "feature_tail")] + ([("features", (N,), w, "int32")] if top else [])
    plain, cnt = both(lambda o: wk.explain_points_into(o, top=top), VECTORS + rows, keep=True)
    assert cnt == (int(np.isnan(X).any(1).sum()), 0)      # (no marginalising asked for: the points with gaps take no part)
    assert np.isfinite(plain["residual"][0]).all()


def test_explain_groups_rows_keep_the_words_behind(pkg, niw5):
    """explain_groups_points with two groups: as explain_points, the words behind the G entries of a row keep the sentinel in both variants
    (recorded on the commit before the rows went through the shared staging)."""
    wk, pars, X = niw5
    groups = [[0, 3], [1]]
    cond = importlib.import_module(pkg.__name__ + ".host.condition")
    wk.set_explain_groups(groups, cond.group_factors(pars[1], groups))
    rows = [(name, (N,), len(groups), "float32") for name in ("group_mahalanobis", "group_tail")]
    plain, cnt = both(lambda o: wk.explain_groups_points_into(o), VECTORS + rows, keep=True)
    assert cnt == (int(np.isnan(X).any(1).sum()), 0)
    assert np.isfinite(plain["group_tail"][0]).all()


def test_impute(niw5):
    wk, _, X = niw5
    plain, _ = both(lambda o: wk.impute_points_into(o["out"]), [("out", (N,), X.shape[1], "float32")])
    gaps = np.isnan(X)
    assert np.array_equal(raw(plain["out"])[~gaps], raw(X)[~gaps]) and np.isfinite(plain["out"][gaps]).all()


def test_count_explain(binding, host):
    rng = np.random.default_rng(41)
    post = G.posterior(40, 3, rng)
    X = G.counts_data(post, N, rng).astype(np.float32)
    X[4, N - 2] = np.nan                                   # (D, n): a feature of a point of the last tile
    top = 3
    rows = [("features", (N,), top, "int32")] + [(name, (N,), top, "float32") for name in ("count", "expected", "residual", "feature_tail")]
    with G.open_predictor(host, post, N, binding=binding) as p:
        p._wk.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)
        got = p.explain_counts(X, top)                    # the tables of set_count_explain in force, the points uploaded
        wk = p._wk
        plain, cnt = both(lambda o: wk.count_explain_points_into(o, top), rows + [("labels", (N,), None, "int64"), ("total", (N,), None, "float64")])
    assert cnt == (got.skipped, got.incomplete) and cnt[0] == 1
    for name in plain:
        assert np.array_equal(raw(plain[name]), raw(getattr(got, name))), name
