"""CPU checks of tests/tools/predictive_ref.py, the reference and the bound tests/test_gpu_predictive.py holds the Student-t table to:
the reference equals scipy's multivariate t; a numpy Float32 restatement of the kernel is accepted and every listed mistake (in the
kernel's epilogue, in dpmm_set_predictive_niw's constant, in host/priors.py's conversion) is rejected, at every case; the bound is within
test_loglik_table's tolerance for at least 95 % of the bulk points of every case, so it is not vacuous."""
import importlib

import numpy as np
import pytest

from oracle import oracle as orc
from tools import predictive_ref as pr


@pytest.fixture(scope="module")
def priors():
    from __graft_entry__ import load_package
    return importlib.import_module(load_package().__name__ + ".host.priors")


_cases = {}


def case(D, K):
    """(inputs, want, parts, bound) of a case, computed once and never modified."""
    if (D, K) not in _cases:
        c = pr.make_case(D, K)
        want, parts = pr.student_t_table(c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"])
        _cases[D, K] = (c, want, parts, pr.error_bound(c["X"], c["m"], c["R"], c["df"], parts))
    return _cases[D, K]


def args_of(c):
    return c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"]


def rejected(got, want, bound, q):
    try:
        pr.check_table(got, want, bound, q)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("D", [1, 2, 5])
def test_reference_equals_scipy_multivariate_t(D):
    from scipy.stats import multivariate_t
    c, want, parts, _ = case(D, 3)
    ok = np.isfinite(c["X"]).all(1) & (np.abs(c["X"]).max(1) < 1e20)         # (scipy has no answer for the NaN and the 1e25 point)
    for k in range(3):
        R = c["R"][k].astype(np.float64)
        ref = multivariate_t(loc=c["m"][k].astype(np.float64), shape=np.linalg.inv(R.T @ R), df=float(c["df"][k])).logpdf(
            c["X"][ok].astype(np.float64)) + np.log(np.float64(c["w"][k]))
        # logdet is the table's own input, a Float32: its rounding (2^-25 |logdet|) is the one difference beyond Float64 noise
        np.testing.assert_allclose(want[k, ok], ref, rtol=1e-9, atol=1e-9 + 2.0 ** -24 * abs(float(c["logdet"][k])))


@pytest.mark.parametrize("D,K", pr.CASES)
def test_planted_points_are_what_they_claim(D, K):
    c, want, parts, bound = case(D, K)
    for i, k in c["planted"]["mean"]:
        assert parts["q"][k, i] == 0.0 and want[k, i] == parts["cst"][k]
    for i, k in c["planted"]["far"]:
        assert 0.9e6 * D < parts["q"][k, i] < 1.1e6 * D                      # 1e3 sd out; nowhere near the Float32 range
    for i in c["planted"]["huge"]:
        assert np.all(parts["q"][:, i] > 1e6 * pr.FLT_MAX) and np.all(np.isfinite(want[:, i]))
    for i, _ in c["planted"]["nan"]:
        assert np.isnan(want[:, i]).all()
    assert np.isfinite(want[:, c["bulk"]]).all() and parts["q"][:, c["bulk"]].max() < 1e-6 * pr.FLT_MAX
    assert c["bulk"].sum() == c["n"] - 7


@pytest.mark.parametrize("D,K", pr.CASES)
def test_emulation_accepted_every_mistake_rejected(D, K):
    c, want, parts, bound = case(D, K)
    worst = pr.check_table(pr.emulate_f32(*args_of(c)), want, bound, parts["q"])
    print(f"D={D} K={K}: Float32 emulation max |err| / bound = {worst:.3f}")
    for mutation in pr.MUTATIONS:
        if mutation == "hdf_padded" and D % 16 == 0:
            continue                                                        # (the padded dimension is D: not a mistake there)
        assert rejected(pr.emulate_f32(*args_of(c), mutation=mutation), want, bound, parts["q"]), mutation


@pytest.mark.parametrize("D,K", pr.CASES)
def test_bound_is_not_vacuous(D, K):
    c, want, parts, bound = case(D, K)
    own, every = pr.bulk_share(bound, want, c["bulk"], c["lab"]), pr.bulk_share(bound, want, c["bulk"])
    print(f"D={D} K={K}: bound within 1e-3 + 2e-5 |want| for {own:.3f} of the bulk under its own cluster, {every:.3f} of all entries")
    assert own >= 0.95
    if D <= 64:                                                             # (see predictive_ref.conditioning for the wider ones)
        assert every >= 0.95


# ------------------------------------------------------------------------------------------------ the host conversion
@pytest.mark.parametrize("D", sorted(set(pr.DIMS) | set(pr.POSTERIOR_DIMS)))
def test_conversion_accepted_inverted_c_rejected(priors, D):
    P = pr.make_posterior(D)
    cap = pr.Capture()
    priors.niw_hyperparams(1.0, np.zeros(D), D + 3.0, np.eye(D)).predictive_table(cap, P["post"], list(range(P["K"])), P["w"])
    m, R, logdet, df, w = cap.args
    assert np.array_equal(m, P["post"]["m"]) and np.array_equal(df.astype(np.float64), P["post"]["nu"] - D + 1)      # Float32 values by construction
    want, parts, bound = pr.posterior_reference(P, cap.args, orc.niw_posterior_predictive)
    worst = pr.check_table(pr.emulate_f32(P["X"], m, R, logdet, df, w), want, bound, parts["q"])
    share = pr.bulk_share(bound, want, P["bulk"], P["lab"])
    print(f"D={D}: conversion + Float32 emulation max |err| / bound = {worst:.3f}; bound within the loglik tolerance for {share:.3f} of the points")
    assert share >= 0.95
    # c -> 1 / c: R = U^-1 / sqrt(c) becomes U^-1 sqrt(c), logdet = D log c + ... becomes -D log c + ...
    c = P["c"]
    assert np.all(np.abs(np.log(c)) > 0.1)
    Rm = R.reshape(-1, D, D).astype(np.float64) * c[:, None, None]
    ldm = logdet.astype(np.float64) - 2 * D * np.log(c)
    assert rejected(pr.emulate_f32(P["X"], m, Rm, ldm, df, w), want, bound, parts["q"])
