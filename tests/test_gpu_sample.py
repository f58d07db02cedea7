"""GPU tests of Predictor.sample (host/score.py) over include/dpmm_hip_sample.h (csrc/sample.hip).

Multinomial draws are integer-only, so dense and sparse counts are compared with tests/tools/sample_ref.py bit for bit.  NIW draws are
checked three ways: structure (seeds, capacity, save / load, labels), closeness to the Float64 restatement made from the same random words,
and the law itself by the checks of sample_ref.check_whitened, whose thresholds tests/test_sample_cpu.py verifies on the reference with
the seeds used here.

Closeness bound.  The kernel's z differs from the reference's by the Float32 evaluation of sqrt(-2 log u) cos / sin(2 pi u'): the fast
logarithm is good to 2^-21.4 absolutely near 1 and to 2 ulp elsewhere, the fast sine / cosine to 2^-21.2 on the first period, and
d sqrt(-2 log u) = d log u / r with r >= 1e-3 for all but one in 2e6 of the normals: |dz| < 1e-3.  The product adds D Float32 roundings of
terms of size |A_ab z_b|.  Hence |x - ref| <= 2e-3 s sum_b |A_ab| (1 + |z_b|) + 2^-20 |ref| with room to spare."""
import importlib

import numpy as np
import pytest
import torch

from tools import predictive_ref as pr
from tools import sample_ref as R

pytestmark = pytest.mark.gpu

PRIOR_NIW, PRIOR_MULT = 0, 1
TRIALS = (1, 2, 63, 64, 65, 1000, R.SPARSE_CAP)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


def seed_with(weights, n, want):
    """The first seed whose host draw of the cluster sizes satisfies `want`."""
    return next(s for s in range(100000) if want(R.cluster_sizes(weights, n, s)))


# ------------------------------------------------------------------------------------------------ Multinomial, exact
def mult_model(D, K):
    """(points_count, alpha' (K, D)).  K = 3: a cluster nobody is drawn from, one with a single category of mass 1, one whose theta has
    exact zeros (every second category, D > 1); K = 1: all categories positive."""
    rng = np.random.default_rng(100 * D + K)
    if K == 1:
        return np.array([5.0]), rng.dirichlet(np.ones(D))[None, :] * 1000.0
    th = np.zeros((3, D))
    th[0] = rng.dirichlet(np.ones(D))
    th[1, D // 2] = 1.0
    keep = np.arange(D) % 2 == 0
    th[2, keep] = rng.dirichlet(np.ones(int(keep.sum())))
    return np.array([0.0, 1.0, 60.0]), th * 1000.0


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("D", [1, 2, 127, 128, 129, 1000, 5000, 65536])
def test_multinomial_counts_equal_the_reference_bit_for_bit(score, D, K):
    pc, alpha_post = mult_model(D, K)
    n = 40 if K == 1 else 61
    w = pc / pc.sum()
    seed = 3 if K == 1 else seed_with(w, n, lambda nk: nk[0] == 0 and nk[1] == 1)
    n_k = R.cluster_sizes(w, n, seed)
    lab = R.labels_of(n_k)
    with score.Predictor.load(R.predictor_file(PRIOR_MULT, D, 0.0, pc, dict(alpha=alpha_post)), capacity=16) as p:
        _, theta, thr, alias = p.sampler_tables()
        for trials in TRIALS:
            want = R.mult_counts(thr, alias, lab, np.arange(n), seed, trials)
            assert (want.sum(1) == trials).all()
            assert (want[theta[lab] == 0] == 0).all()                 # a category of probability 0 is never drawn
            sp, lab_s = p.sample(n, seed=seed, trials=trials, sparse=True)
            assert sp.layout == torch.sparse_csc and tuple(sp.shape) == (D, n)
            cp, rv, nz = sp.ccol_indices().cpu().numpy(), sp.row_indices().cpu().numpy(), sp.values().cpu().numpy()
            assert cp.dtype == np.int64 and rv.dtype == np.int64 and nz.dtype == np.float32
            assert cp[0] == 0 and cp[-1] == len(rv) == len(nz) and (np.diff(cp) >= 1).all() and (nz >= 1).all()
            inner = np.ones(len(rv), bool)
            inner[cp[:-1]] = False                                    # first entry of every column
            assert (np.diff(rv)[inner[1:]] > 0).all(), "row indices must increase strictly inside a column"
            img = np.zeros((n, D), np.int64)
            img[np.repeat(np.arange(n), np.diff(cp)), rv] = nz.astype(np.int64)
            assert np.array_equal(img, want), (D, K, trials, "sparse")
            assert np.array_equal(lab_s.cpu().numpy(), lab + 1)
            if D <= 5000:
                x, lab_d = p.sample(n, seed=seed, trials=trials)
                assert tuple(x.shape) == (D, n) and x.dtype == torch.float32 and x.T.is_contiguous()
                assert np.array_equal(x.T.cpu().numpy().astype(np.int64), want), (D, K, trials, "dense")
                assert np.array_equal(lab_d.cpu().numpy(), lab + 1)


def test_multinomial_sparse_draw_goes_through_predict_unchanged(pkg, score):
    """The sparse draw is well-formed by the library's own definition (dpmm_upload_points_csc_device accepts it in place), and
    Predictor.predict labels it as it labels its dense image."""
    binding = importlib.import_module(pkg.__name__ + ".binding")
    sparse = importlib.import_module(pkg.__name__ + ".host.sparse")
    D, n, K = 300, 500, 3
    rng = np.random.default_rng(4)
    alpha_post = rng.dirichlet(np.full(D, 0.3), K) * 500.0 + 0.01
    with score.Predictor.load(R.predictor_file(PRIOR_MULT, D, 0.5, np.array([30.0, 50.0, 20.0]), dict(alpha=alpha_post)), capacity=128) as p:
        sp, lab = p.sample(n, seed=11, trials=40, sparse=True)
        got = p.predict(sp)[0].cpu().numpy()
        cp, rv, nz = sp.ccol_indices().cpu().numpy(), sp.row_indices().cpu().numpy(), sp.values().cpu().numpy()
        img = np.zeros((D, n), np.float32)
        img[rv, np.repeat(np.arange(n), np.diff(cp))] = nz
        assert (img.sum(0) == 40).all()
        want = p.predict(torch.tensor(img, device=sp.device))[0].cpu().numpy()
    assert np.array_equal(got, want)
    assert (got == lab.cpu().numpy()).mean() > 0.9                    # (well separated clusters: most points go back to their own)
    wk = binding.Worker(PRIOR_MULT, D, n, device=0)
    try:
        wk.upload_points_csc_tensor(sparse.as_csc(sp), 0, n)
    finally:
        wk.close()


# ------------------------------------------------------------------------------------------------ NIW
def niw_predictor(score, D, K, df, pc, capacity, seed=1):
    post, m, A, dfs = R.niw_model(D, K, df, seed)
    return score.Predictor.load(R.predictor_file(PRIOR_NIW, D, 0.0, pc, post), capacity=capacity), m, A, dfs


def assert_close_to_reference(x, m, A, df, lab, idx, seed):
    """The bound of the module's description, on the points (n, D) with global indices idx."""
    ref = R.niw_points(m, A, df, lab, idx, seed)
    z = R.normals(idx, m.shape[1], seed)
    s = np.sqrt(df[lab] / R.chi2(df[lab], idx, seed))
    bound = np.empty_like(ref)
    for k in np.unique(lab):
        sel = lab == k
        bound[sel] = 2e-3 * s[sel, None] * ((1 + np.abs(z[sel])) @ np.abs(A[k]).T)
    bound += 2.0 ** -20 * np.abs(ref)
    err = np.abs(x - ref)
    print(f"closeness: max |x - ref| / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all(), f"max |x - ref| / bound = {(err / bound).max():.3g}"


def test_niw_structure(score, tmp_path):
    D, K, n = 5, 4, 1000
    pc = np.array([3.0, 0.0, 5.0, 2.0])
    w = pc / pc.sum()
    draws = {}
    for cap in (64, 100, n):
        p, m, A, df = niw_predictor(score, D, K, 60.0, pc, cap)
        with p:
            x, lab = p.sample(n, seed=7)
            assert tuple(x.shape) == (D, n) and x.dtype == torch.float32 and x.T.is_contiguous() and lab.dtype == torch.int64
            draws[cap] = (x.T.cpu().numpy().copy(), lab.cpu().numpy().copy())
            if cap == 100:
                again, other = p.sample(n, seed=7)[0].T.cpu().numpy(), p.sample(n, seed=8)[0].T.cpu().numpy()
                p.save(str(tmp_path / "model.npz"))
    x0, lab0 = draws[n]
    assert np.isfinite(x0).all()
    assert np.array_equal(again, draws[100][0]) and not np.array_equal(other, draws[100][0])
    for cap in (64, 100):                                             # capacity-invariant, bit for bit
        assert np.array_equal(draws[cap][0], x0) and np.array_equal(draws[cap][1], lab0)
    n_k = R.cluster_sizes(w, n, 7)
    assert (np.diff(lab0) >= 0).all() and np.array_equal(np.bincount(lab0 - 1, minlength=K), n_k) and n_k[1] == 0
    with score.Predictor.load(str(tmp_path / "model.npz"), capacity=333) as q:
        assert np.array_equal(q.sample(n, seed=7)[0].T.cpu().numpy(), x0)
    assert_close_to_reference(x0.astype(np.float64), m, A, df, lab0 - 1, np.arange(n), 7)


@pytest.mark.parametrize("size", [1, 63, 64, 65])
def test_niw_cluster_sizes_around_a_tile(score, size):
    """Clusters of 0, 1, 63, 64 and 65 points: sizes (size, 0, rest) picked by the seed of the host's draw."""
    D, K, n = 7, 3, 129
    pc = np.array([1.0, 0.0, 1.0])
    seed = seed_with(pc / pc.sum(), n, lambda nk: nk[0] == size) if size > 1 else 0
    if size == 1:
        pc, n = np.array([1.0, 0.0, 128.0]), 129
        seed = seed_with(pc / pc.sum(), n, lambda nk: nk[0] == 1)
    n_k = R.cluster_sizes(pc / pc.sum(), n, seed)
    assert n_k[0] == size and n_k[1] == 0
    p, m, A, df = niw_predictor(score, D, K, 50.0, pc, 4096)
    with p:
        x, lab = p.sample(n, seed=seed)
    x, lab = x.T.cpu().numpy().astype(np.float64), lab.cpu().numpy()
    assert np.isfinite(x).all() and np.array_equal(lab - 1, R.labels_of(n_k))
    assert_close_to_reference(x, m, A, df, lab - 1, np.arange(n), seed)


LAW_N = 20100


@pytest.mark.parametrize("D", [1, 2, 3, 17, 33, 64, 65, 128, 256])
def test_niw_law(score, D):
    pc = np.array([0.005, 0.995])
    p, m, A, df = niw_predictor(score, D, 2, 60.0, pc, 4096, seed=D)
    with p:
        x, lab = p.sample(LAW_N, seed=1000 + D)
    x, lab = x.T.cpu().numpy().astype(np.float64), lab.cpu().numpy()
    assert np.isfinite(x).all()
    sel = lab == 2
    assert sel.sum() > 19000
    head = np.arange(min(LAW_N, 2000 if D > 64 else 6000))
    assert_close_to_reference(x[head], m, A, df, lab[head] - 1, head, 1000 + D)
    R.check_whitened(R.whiten(x[sel], m[1], A[1]), df[1])


# ------------------------------------------------------------------------------------------------ closing the loop with scoring
def test_mean_log_density_of_the_draw_is_the_negative_entropy(pkg, score):
    host = importlib.import_module(pkg.__name__ + ".host")
    priors = importlib.import_module(pkg.__name__ + ".host.priors")
    D, n = 8, 30000
    data, _, _, _ = host.generate_gaussian_data(6000, D, 3, 80.0, seed=5)
    res = host.fit(data, 10.0, iters=30, seed=11, burnout=5, verbose=False)
    with score.Predictor(res[8], capacity=8192) as p:
        x, lab = p.sample(n, seed=21)
        got = p.score_samples(x).cpu().numpy().astype(np.float64)
        _, m, A, df = p.sampler_tables()
        cap = pr.Capture()
        priors.niw_hyperparams(1.0, np.zeros(D), D + 3.0, np.eye(D)).predictive_table(cap, p.post, list(range(p.K)), p.weights)
        n_k = p.cluster_sizes(n, 21)
    assert np.array_equal(lab.cpu().numpy() - 1, R.labels_of(n_k))
    ref_x = R.niw_points(m, A, df, R.labels_of(n_k), np.arange(n), 21)
    table, _ = pr.student_t_table(ref_x, *cap.args)
    mx = table.max(0)
    want = mx + np.log(np.exp(table - mx).sum(0))
    se = np.sqrt(got.var(ddof=1) / n + want.var(ddof=1) / n)
    print(f"mean log-density: drawn {got.mean():.5f}, reference {want.mean():.5f}, combined standard error {se:.5f}")
    assert abs(got.mean() - want.mean()) <= 6 * se
