"""CPU-side checks of drawing points from a fitted model: the seventh header and its bindings, the alias-table builder, the argument
checks of Predictor.sample, and the statistical assertions of tests/test_gpu_sample.py run against the numpy reference sampler
(tests/tools/sample_ref.py) with the seeds the GPU tests use -- the thresholds hold for a correct sampler and reject three wrong ones."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import sample_ref as R

PRIOR_NIW, PRIOR_MULT = 0, 1


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


# ------------------------------------------------------------------------------------------------ header and exports
def test_header_compiles_as_c_and_its_functions_are_bound_and_exported(pkg):
    header = os.path.join(ROOT, "include", "dpmm_hip_sample.h")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", header])
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["dpmm_sample_points_device", "dpmm_set_sampler_mult", "dpmm_set_sampler_niw"]
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_SAMPLE) == declared
    assert int(re.search(r"#define DPMM_SAMPLE_MAX_TRIALS_SPARSE (\d+)", src).group(1)) == binding.SAMPLE_MAX_TRIALS_SPARSE == R.SPARSE_CAP
    assert int(re.search(r"#define DPMM_SAMPLE_MAX_TRIALS_DENSE (\d+)", src).group(1)) == binding.SAMPLE_MAX_TRIALS_DENSE
    # the request structure of the binding has the header's members, in order
    body = src[src.index("typedef struct {"):src.index("} dpmm_sample_request;")]
    members = re.findall(r"\*?\s*\b(\w+);", body)
    assert members == [f[0] for f in binding.SampleRequest._fields_]
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for name in declared:
        assert hasattr(lib, name), name
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                                # additive: the version stays
    mk = open(os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc", "Makefile")).read()
    assert "build/sample.o" in mk and "dpmm_hip_sample.h" in mk
    host = importlib.import_module(pkg.__name__ + ".host")
    assert callable(host.sample) and callable(host.Predictor.sample)


def test_stream_ids_are_new(pkg):
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    ids = {}
    for f in ("dpmm_device.h", "niw_master.hip", "mult_master.hip"):
        for name, val in re.findall(r"\b(STREAM_[A-Z_]+)\s*=\s*(\d+)", open(os.path.join(csrc, f)).read()):
            ids[name] = int(val)
    assert len(set(ids.values())) == len(ids), ids
    assert (ids["STREAM_SAMPLE_NORMAL"], ids["STREAM_SAMPLE_CHI"], ids["STREAM_SAMPLE_MULT"]) == (R.STREAM_NORMAL, R.STREAM_CHI, R.STREAM_MULT)


def test_philox_restatement_known_answers():
    """Random123's known-answer vectors of philox4x32-10 (counter, key) -> the reference's word order (i low, i high, block, stream)."""
    assert [int(v) for v in R.philox(0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = R.philox(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v) for v in ones] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


# ------------------------------------------------------------------------------------------------ alias tables
@pytest.mark.parametrize("D", [1, 2, 3, 127, 1000, 4097])
def test_alias_tables_realise_theta(score, D):
    rng = np.random.default_rng(D)
    theta = np.stack([rng.dirichlet(np.ones(D)), rng.dirichlet(np.full(D, 0.05)), np.full(D, 1.0 / D), np.eye(D)[D // 2],
                      np.where(np.arange(D) % 2 == 0, 1.0, 0.0) / ((D + 1) // 2)])
    thr, alias = score.alias_tables(theta)
    assert thr.dtype == np.uint32 and alias.dtype == np.int32 and thr.shape == alias.shape == theta.shape
    assert (alias >= 0).all() and (alias < D).all()
    got = R.alias_probabilities(thr, alias)
    assert np.abs(got - theta).max() <= D * 2.0 ** -32
    # a category of probability 0 is never produced: its bucket never accepts, and it is nobody's alias
    for k in range(len(theta)):
        zero = np.flatnonzero(theta[k] == 0)
        assert (thr[k, zero] == 0).all() and (alias[k, zero] != zero).all()
        assert not np.isin(alias[k], zero).any()
        assert (got[k, zero] == 0).all()


def test_reference_counts_follow_theta(score):
    """The reference's alias draw itself: 2e6 trials reproduce theta within 6 binomial standard deviations per category."""
    D, n, trials = 37, 500, 4000
    theta = np.random.default_rng(1).dirichlet(np.full(D, 0.7))[None, :]
    theta[0, 5] += theta[0, 6]
    theta[0, 6] = 0.0
    thr, alias = score.alias_tables(theta)
    c = R.mult_counts(thr, alias, np.zeros(n, int), np.arange(n), 9, trials)
    assert (c.sum(1) == trials).all() and (c[:, 6] == 0).all()
    tot, N = c.sum(0), n * trials
    assert (np.abs(tot - N * theta[0]) <= 6 * np.sqrt(N * theta[0] * (1 - theta[0])) + 1e-9).all()


# ------------------------------------------------------------------------------------------------ argument checks
class _Worker:
    """Stands in for binding.Worker where no GPU is: what Predictor's constructor and sample()'s argument checks touch."""

    def __init__(self, *a, **kw):
        pass

    def set_predictive_niw(self, *a):
        pass

    def set_predictive_mult(self, *a):
        pass

    def close(self):
        pass


def test_argument_checks(pkg, score):
    binding = importlib.import_module(pkg.__name__ + ".binding")
    post, _, _, _ = R.niw_model(3, 2, 60.0, 1)
    niw = score.Predictor.load(R.predictor_file(PRIOR_NIW, 3, 1.0, [5.0, 7.0], post), worker_factory=_Worker)
    mult = score.Predictor.load(R.predictor_file(PRIOR_MULT, 4, 1.0, [5.0, 7.0], dict(alpha=np.ones((2, 4)))), worker_factory=_Worker)
    with pytest.raises(ValueError, match="trials"):
        niw.sample(10, trials=5)
    with pytest.raises(ValueError, match="sparse"):
        niw.sample(10, sparse=True)
    with pytest.raises(ValueError, match="negative"):
        niw.sample(-1)
    with pytest.raises(ValueError, match="trials"):
        mult.sample(10)
    with pytest.raises(ValueError, match="negative"):
        mult.sample(-1, trials=3)
    with pytest.raises(ValueError, match="at least 1"):
        mult.sample(10, trials=0)
    with pytest.raises(ValueError, match="DPMM_SAMPLE_MAX_TRIALS_SPARSE"):
        mult.sample(10, trials=binding.SAMPLE_MAX_TRIALS_SPARSE + 1, sparse=True)
    with pytest.raises(RuntimeError, match="cannot draw"):                # no quiet fall-back where the worker has no sampler
        mult.sample(10, trials=3)
    niw.close()
    with pytest.raises(RuntimeError, match="closed"):
        niw.sample(10)


def test_cluster_sizes_are_a_function_of_seed_and_n(score):
    post, _, _, _ = R.niw_model(3, 3, 60.0, 1)
    p = score.Predictor.load(R.predictor_file(PRIOR_NIW, 3, 0.5, [5.0, 0.0, 7.0], post), worker_factory=_Worker)
    w = (np.array([5.0, 0.0, 7.0]) + 0.5) / 13.5
    for n, seed in ((0, 0), (1, 3), (1000, 7), (10 ** 7, 2 ** 63)):
        got = p.cluster_sizes(n, seed)
        assert got.dtype == np.int64 and got.sum() == n and np.array_equal(got, p.cluster_sizes(n, seed))
        assert np.array_equal(got, R.cluster_sizes(w, n, seed))
    _, m, A, df = p.sampler_tables()
    _, m2, A2, df2 = R.niw_model(3, 3, 60.0, 1)
    assert np.allclose(m, m2) and np.allclose(A, A2, rtol=1e-14) and np.allclose(df, df2)


# ------------------------------------------------------------------------------------------------ the statistical assertions, on the reference
LAW_N = 20100


def _law_case(D):
    """The model, seed and points of tests/test_gpu_sample.py::test_niw_law, drawn by the reference."""
    _, m, A, df = R.niw_model(D, 2, 60.0, D)
    n_k = R.cluster_sizes(np.array([0.005, 0.995]), LAW_N, 1000 + D)
    lab = R.labels_of(n_k)
    return m, A, df, lab, np.arange(LAW_N), 1000 + D


@pytest.mark.parametrize("D", [1, 2, 3, 17, 33, 64, 65, 128, 256])
def test_law_checks_hold_for_the_reference_sampler(D):
    m, A, df, lab, idx, seed = _law_case(D)
    x = R.niw_points(m, A, df, lab, idx, seed)
    sel = lab == 1
    assert sel.sum() > 19000
    R.check_whitened(R.whiten(x[sel], m[1], A[1]), df[1])


@pytest.mark.parametrize("mutate", ["transpose", "last_column", "reuse"])
@pytest.mark.parametrize("D", [2, 17, 33, 65, 256])
def test_law_checks_reject_wrong_samplers(D, mutate):
    """A transposed factor, a missed last normal (D not a multiple of the block included) and a normal used twice each miss a check."""
    m, A, df, lab, idx, seed = _law_case(D)
    sel = lab == 1
    x = R.niw_points(m, A, df, lab[sel], idx[sel], seed, mutate=mutate)
    with pytest.raises(AssertionError):
        R.check_whitened(R.whiten(x, m[1], A[1]), df[1])


def test_tested_coordinates():
    for D in (1, 17):
        assert R.tested_coordinates(D) == list(range(D))
    for D in (33, 64, 65, 128, 256):
        c = R.tested_coordinates(D)
        assert len(c) == len(set(c)) == 16 and c[0] == 0 and c[-1] == D - 1 and all(0 <= a < D for a in c)
    assert {15, 16, 31, 32} <= set(R.tested_coordinates(33)) and {63, 64} <= set(R.tested_coordinates(65))


def test_chi2_reference_is_chi2():
    """The bounded Marsaglia-Tsang restatement against scipy's chi^2, shapes below and above 1 (KS, lambda = 3.3 as in check_whitened)."""
    from scipy import stats
    n = 20000
    for df in (0.6, 1.0, 3.5, 60.0, 5000.0):
        g = R.chi2(np.full(n, df), np.arange(n), 17)
        assert R.ks_distance(g, stats.chi2(df).cdf) < R.KS_LAMBDA / np.sqrt(n), df
