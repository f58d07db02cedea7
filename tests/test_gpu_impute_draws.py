"""GPU tests of the imputation draws (include/dpmm_hip_impute.h, miss_draw_kernel of csrc/missing.hip) through host/score.py's
Predictor.impute(draws=m).

The reference is tests/tools/impute_draw_ref.py (Float64 from the same random words; tests/test_impute_draws_cpu.py checks it on the CPU:
two independent routes agree, the law checks accept it and reject six planted mistakes at the sizes used here, the seeds used here excuse
at most 1 % of the components).

Values.  Given the component the GPU drew, a drawn value x_a = c_a + s w_a (c = m_M - t, s = sqrt((df + q_o) / g), w = L'^-1 n) lies within
    bound_a = dcm_a + s (2e-3 sum_b |(L'^-1)_ab| (1 + |n_b|) + |w_a| dq / (2 (df + q_o)) + 2^-36 sum_b |(L'^-1)_ab| |n_b|) + 2^-23 |x_a|
of the reference, DERIVED term by term in impute_draw_ref's docstring: the Float32 error of y through the solve (missing_ref.point_bounds'
dcm and dq), the Float32 Box-Muller normals (|dn| < 1e-3 with room, tests/test_gpu_sample.py's derivation) through the back-substitution,
the Float64 steps, the one rounding to Float32.  Nothing in it is fitted to what the kernel gives.
Components.  The GPU's table is Float32: its cumulative edges lie within rel c_k (rel = expm1(2 max_k bound_k) + 2^-23 (K + 16), the
relative tolerance of the probabilities in missing_ref.derived) of the reference's.  The GPU's component must equal the reference's unless
u lies that close to an edge, and at most 1 % of the (marginalised point, draw) pairs may be excused this way.
Law.  2 000 points x 10 draws per case, standardised with the reference's L, t, q_o of the cluster the GPU drew:
sample_ref.check_whitened per cluster, independence between the draws of a point, and the component frequencies against the reference's
p_k with a chi-square bound of error probability 1e-9 (impute_draw_ref.check_law / check_frequencies state each bound).

Measured on an MI355X, worst got / tolerance per case (printed by the tests): see DESIGN section 21.
"""
import contextlib
import functools
import importlib
import types

import numpy as np
import pytest

from tools import impute_draw_ref as ir
from tools import missing_ref as mr

pytestmark = pytest.mark.gpu

CORRELATED = ("correlated", 3)
VALUE_CASES = tuple(c for c in mr.CASES if c[1] == 3) + (CORRELATED,)
VALUE_SEED, VALUE_DRAWS = 11, 3             # (tests/test_impute_draws_cpu.py checks the excused share of this seed)
LAW_SEED = 5


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@functools.lru_cache(maxsize=None)
def case_ref(D, K):
    """(case, reference): computed once, shared, never modified."""
    c = mr.make_correlated_case() if (D, K) == CORRELATED else mr.make_case(D, K)
    return c, mr.reference(c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"])


@functools.lru_cache(maxsize=None)
def law_ref(D, r, df, n=ir.LAW_POINTS):
    c = ir.law_case(D, r, df, n=n)
    return c, mr.reference(c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"])


def dummy_model(D, K):
    """What a Predictor reads of a fitted model; the worker below is handed the case's own parameters instead of its conversion."""
    post = dict(kappa=np.ones(3 * K), nu=np.full(3 * K, D + 3.0), m=np.zeros((3 * K, D)), U=np.tile(np.eye(D), (3 * K, 1, 1)), logdet_psi=np.zeros(3 * K))
    s = types.SimpleNamespace(K=K, prior=types.SimpleNamespace(kind=0, dim=D), post=post, alpha=10.0, points_count=np.full(K, 10), wk=types.SimpleNamespace(device=0))
    return types.SimpleNamespace(sampler=s)


def case_worker(pkg, c):
    class CaseWorker(pkg.Worker):
        def set_predictive_niw(self, m, R, logdet, df, weights):
            super().set_predictive_niw(c["m"], c["R"].reshape(c["K"], -1), c["logdet"], c["df"], c["w"])
    return CaseWorker


def predictor(pkg, score, c, capacity):
    return score.Predictor(dummy_model(c["D"], c["K"]), capacity=capacity, worker_factory=case_worker(pkg, c))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ structure
def test_structure(pkg, score, tmp_path):
    import torch
    binding = importlib.import_module(pkg.__name__ + ".binding")
    c = ir.structure_case()
    D, K, n, m = c["D"], c["K"], c["n"], 3
    assert (D, K, n) == (5, 4, 133) and c["w"][2] == 0
    data = np.ascontiguousarray(c["X"].T)
    miss, r, listed, over = mr.classify(c["X"])
    assert {0, n - 1, 63, 64, 50, 52, 53} <= set(np.flatnonzero(listed | over).tolist()) and over[52] and listed[53] and r[50] == 4 and np.isinf(c["X"][53]).any()
    res = {}
    for cap in (40, 64, n):
        with predictor(pkg, score, c, cap) as p:
            res[cap] = p.impute(data, draws=m, seed=7, return_components=True)
            counts = p.missing_counts
            if cap == 40:
                p._wk.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)              # a range is one tile of the sweep
                tiled = p.impute(data, draws=m, seed=7, return_components=True)
                other_seed = p.impute(data, draws=m, seed=8)
                mean = p.impute(data)
                assert p.missing_counts == counts == (int(listed.sum()), int(over.sum()))
                p.save(str(tmp_path / "model.npz"))
            if cap == n:                                                        # the ABI's draw0: three calls of one draw each
                pieces = [torch.empty((n, 1, D), dtype=torch.float32, device="cuda:0") for _ in range(m)]
                comps = [torch.empty((1, n), dtype=torch.int32, device="cuda:0") for _ in range(m)]
                for j in range(m):
                    p._wk.impute_draws_into(pieces[j], 7, 0, draw0=j, comp=comps[j])
                pieced = (np.stack([t.cpu().numpy()[:, 0, :].T for t in pieces]), np.concatenate([t.cpu().numpy() for t in comps]))
    out, comp = res[n]
    assert isinstance(out, np.ndarray) and out.shape == (m, D, n) and out.dtype == np.float32
    assert isinstance(comp, np.ndarray) and comp.shape == (m, n) and comp.dtype == np.int32
    # ---- the same bits whatever the capacity, the table budget, the cut into calls, and after save / load
    assert same(res[40], res[n]) and same(res[64], res[n]) and same(tiled, res[n]) and same(pieced, res[n])
    with score.Predictor.load(str(tmp_path / "model.npz"), capacity=64, worker_factory=case_worker(pkg, c)) as q:
        assert same(q.impute(data, draws=m, seed=7, return_components=True), res[n])
    # ---- everything that is not a gap of a marginalised point: the input, bit for bit; over the cap: the NaN stays
    gaps = np.isnan(data)
    for j in range(m):
        assert np.array_equal(bits(out[j])[~gaps], bits(data)[~gaps])
        assert np.isnan(out[j][:, over][gaps[:, over]]).all()
    fin = listed & ~np.isinf(c["X"]).any(1)
    drawn = out[:, :, fin][:, gaps[:, fin]]                                     # (m, gaps of the marginalised points with finite features)
    assert np.isfinite(drawn).all() and drawn.shape[1] >= 20
    # ---- seeds and draws differ, the mean imputation is something else again
    assert (drawn[0] != drawn[1]).all() and (drawn[1] != drawn[2]).all() and (other_seed[:, :, fin][:, gaps[:, fin]] != drawn).all()
    assert (mean[:, fin][gaps[:, fin]] != drawn[0]).all()
    # ---- comp: -1 exactly off the marginalised points, never the empty cluster
    assert ((comp == -1) == ~listed[None, :]).all() and ((comp[:, listed] >= 0) & (comp[:, listed] < K) & (comp[:, listed] != 2)).all()
    assert len(np.unique(comp[:, listed])) >= 2


def test_nothing_depends_on_what_earlier_kernels_left_in_lds_or_registers(pkg, score):
    """The copy and draw kernels (and list and patch in front of them) with LDS and the register files refilled with a NaN pattern in front
    of every launch (tests/tools/poison.py through DPMM_LAUNCH's hook): the same bits."""
    from tools import poison
    poison.build()                      # (a build failure is a failure here, not a skip)
    binding = importlib.import_module(pkg.__name__ + ".binding")
    c, _ = case_ref(65, 3)
    data = np.ascontiguousarray(c["X"].T)
    res = []
    for dirty in (False, True):
        with (poison.poisoned_kernel_launches(binding, 0xffffffff) if dirty else contextlib.nullcontext()) as launches:
            with predictor(pkg, score, c, 40) as p:
                res.append(p.impute(data, draws=2, seed=3, return_components=True))
    assert launches[0] > 10 and same(res[0], res[1])


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("D,K", VALUE_CASES)
def test_values_against_float64(pkg, score, D, K):
    c, ref = case_ref(D, K)
    n = c["n"]
    data = np.ascontiguousarray(c["X"].T)
    with predictor(pkg, score, c, 40) as p:
        out, comp = p.impute(data, draws=VALUE_DRAWS, seed=VALUE_SEED, return_components=True)
    assert ((comp == -1) == ~ref["listed"][None, :]).all() and (comp[:, ref["listed"]] < c["K"]).all()
    chk = np.flatnonzero(ref["check"])
    R = ir.draw(c, ref, np.arange(n, dtype=np.uint64), VALUE_DRAWS, VALUE_SEED, comp=comp, bounds=True, points=chk)
    worst = 0.0
    for i in chk:
        got = out[:, ref["miss"][i], i]                                         # (draws, r): the gaps in increasing feature order
        assert np.isfinite(got).all(), i
        worst = max(worst, float((np.abs(got - R["x"][int(i)]) / R["bound"][int(i)]).max()))
    with np.errstate(all="ignore"):
        rel = np.expm1(2 * ref["bound"].max(0)) + mr.EPS * (c["K"] + 16)
    differ = comp[:, chk] != R["own"][:, chk]
    excused = np.stack([ir.excused(R["p"][chk], R["u"][j, chk], rel[chk]) for j in range(VALUE_DRAWS)])
    print(f"D={D} K={K}: {len(chk)} marginalised points x {VALUE_DRAWS} draws, worst |x - ref| / bound {worst:.2e}; components: {int(differ.sum())} differ, "
          f"{int(excused.sum())} of {excused.size} excused")
    assert worst <= 1.0
    assert not (differ & ~excused).any() and excused.mean() <= 0.01


# ------------------------------------------------------------------------------------------------ the law
@pytest.mark.parametrize("D,r,df", ir.LAW_CASES)
def test_the_law(pkg, score, D, r, df):
    c, ref = law_ref(D, r, df)
    n, nd = c["n"], ir.LAW_DRAWS
    data = np.ascontiguousarray(c["X"].T)
    with predictor(pkg, score, c, 512) as p:                                    # four slabs, the last one short
        out, comp = p.impute(data, draws=nd, seed=LAW_SEED, return_components=True)
    assert (comp >= 0).all() and np.isfinite(out).all()
    truth = ir.draw(c, ref, np.arange(n, dtype=np.uint64), nd, LAW_SEED, comp=comp)       # L, t, q_o of the clusters the GPU drew
    df64 = c["df"].astype(np.float64)
    u = np.stack([ir.standardise(out[:, ref["miss"][i], i], truth["parts"][i], comp[:, i], df64, D) for i in range(n)])
    checked = ir.check_law(u, comp.T, df64 + D - r)
    x2, lim = ir.check_frequencies(comp.T, truth["p"])
    print(f"D={D} r={r}: {n} points x {nd} draws, clusters checked {checked}, component frequencies X^2 = {x2:.2f} (bound {lim:.1f}), "
          f"components that differ from the reference's {int((comp != truth['own']).sum())}")


def test_the_mean_of_many_draws_is_the_mean_imputation(pkg, score):
    """100 gapped points, 256 draws: E[x_M | x_O] = sum_k p_k (m_M - t_k) is what `impute(data)` returns, so the mean of the draws lies
    within 6 of its standard errors (from the draws' own sample variance; 400 values, each beyond with probability 2e-9 under normality --
    the t_120 tails of one draw are averaged out over 256) of it."""
    c, ref = law_ref(64, 4, 60.0, n=100)
    data = np.ascontiguousarray(c["X"].T)
    with predictor(pkg, score, c, 64) as p:
        draws = p.impute(data, draws=256, seed=21)
        mean = p.impute(data)
    gaps = np.isnan(data)
    d = draws[:, gaps].astype(np.float64)                                       # (256, 400)
    se = d.std(0, ddof=1) / np.sqrt(256)
    zs = np.abs(d.mean(0) - mean[gaps]) / se
    print(f"mean of 256 draws against impute: worst {zs.max():.2f} standard errors over {zs.size} values")
    assert d.shape == (256, 400) and zs.max() < 6.0


# ------------------------------------------------------------------------------------------------ smoke
def test_every_float_type_on_the_device_and_a_host_array(pkg, score):
    import torch
    c, ref = case_ref(16, 3)
    with np.errstate(over="ignore"):
        X = c["X"].astype(np.float16).astype(np.float32)                        # exact in every float type below but bfloat16
    host = np.ascontiguousarray(X.T)
    with predictor(pkg, score, c, 64) as p:
        want = p.impute(host, draws=2, seed=1, return_components=True)
        assert isinstance(want[0], np.ndarray)
        for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
            t = torch.as_tensor(host, device="cuda:0").to(dt)
            out, comp = p.impute(t, draws=2, seed=1, return_components=True)
            assert out.device == t.device and out.dtype == torch.float32 and tuple(out.shape) == (2, 16, c["n"])
            assert comp.device == t.device and comp.dtype == torch.int32 and tuple(comp.shape) == (2, c["n"])
            seen = t.float().cpu().numpy()
            gaps = np.isnan(seen)
            assert np.array_equal(bits(out[1].cpu().numpy())[~gaps], bits(seen)[~gaps])
            if dt != torch.bfloat16:
                assert same((out.cpu().numpy(), comp.cpu().numpy()), want)
