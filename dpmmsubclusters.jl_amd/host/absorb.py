"""Folding a batch into a served NIW model: the conjugate update from per-cluster sufficient statistics, on the host in Float64.

The NIW prior is conjugate, so the posterior a `Predictor` carries -- kappa, nu, m and U with nu psi = U U' per cluster -- is the exact
prior of the next batch.  Given the batch's N_k = sum_i w_ik, sums_k = sum_i w_ik x_i and S_k = sum_i w_ik x_i x_i'
(`Predictor.statistics`, include/dpmm_hip_batchstats.h), for every cluster with N_k > 0:

    kappa' = kappa + N        nu' = nu + N        m' = (kappa m + sums) / kappa'
    U' U'^T = nu' psi' = U U^T + S + kappa m m^T - kappa' m' m'^T

-- priors/niw.jl:20-31 with the cluster's own posterior in the prior's place -- factorised as `niw_hyperparams.posterior` does (the
reverse Cholesky of host/csrc/hostmath.h, U upper triangular), logdet_psi recomputed.  The arithmetic is the library's own
(`native.niw_posterior`), called with Float64 kappa and nu: `niw_hyperparams.__init__` rounds both to Float32, as the reference does for
a prior the user types in, which would lose the fractional N of soft weights -- so that constructor is not on this route.

The Dirichlet prior of the Multinomial is conjugate too, and its update is a sum: alpha' = alpha + sums (priors/multinomial_prior.jl:16-21
with the cluster's own posterior in the prior's place), from `Predictor.count_statistics` (include/dpmm_hip_countstats.h).
`dirichlet_absorb` keeps alpha' in Float64.  The reference stores Float32, and `multinomial_hyper.posterior` rounds to it, as is right for
one fit; a served cluster whose alpha has grown to 1e6 would lose a soft weight of 0.01 at every batch (the spacing of Float32 there is
0.0625) -- the reasoning of the note on kappa and nu above.  `predictive_table` widens alpha to Float64 anyway, and `save` / `load` keep
the type the array has.

`niw_graft` appends clusters: the posteriors `Predictor.grow` found for the points no cluster explains go behind the ones the model has,
which keep their numbers and their bits.  `dirichlet_graft` does the same for the alpha rows of a Multinomial model
(`Predictor.grow_counts`).
"""
import numpy as np

from . import native

POST_KEYS = ("kappa", "nu", "m", "U", "logdet_psi")


def niw_absorb(post, points_count, stats):
    """(post', points_count'): the posterior arrays of K clusters (`Predictor.post`: kappa, nu, logdet_psi (K,), m (K, D), U (K, D, D))
    and their point counts after the conjugate update with `stats` -- anything with N (K,), sums (K, D), S (K, D, D), e.g. a
    `BatchStatistics`.  Everything in Float64; the inputs are not modified.  A cluster with N_k == 0 keeps its bits.  ValueError for
    shapes that do not fit, a negative or non-finite N, non-finite sums or S, and for an update that is not positive definite."""
    missing = [k for k in POST_KEYS[:4] if k not in post]
    if missing:
        raise ValueError(f"niw_absorb is for NIW posteriors: post lacks {missing}")
    new = {k: np.array(post[k], np.float64 if k in POST_KEYS else None) for k in post}
    if "logdet_psi" not in new and new["U"].ndim == 3 and new["U"].shape[1:] == new["m"].shape[1:] * 2:      # (a model file written without it)
        new["logdet_psi"] = 2 * np.log(np.einsum("kii->ki", new["U"])).sum(1) - new["m"].shape[1] * np.log(new["nu"])
    K, D = new["m"].shape if new["m"].ndim == 2 else (0, 0)
    if new["m"].ndim != 2 or K < 1 or new["U"].shape != (K, D, D) or any(new[k].shape != (K,) for k in ("kappa", "nu", "logdet_psi")):
        raise ValueError("post must hold kappa, nu, logdet_psi (K,), m (K, D) and U (K, D, D)")
    count = np.array(points_count, np.float64)
    if count.shape != (K,):
        raise ValueError("points_count must have one entry per cluster")
    N, sums, S = (np.asarray(getattr(stats, f) if hasattr(stats, f) else stats[f], np.float64) for f in ("N", "sums", "S"))
    if N.shape != (K,) or sums.shape != (K, D) or S.shape != (K, D, D):
        raise ValueError(f"the statistics must be N ({K},), sums ({K}, {D}) and S ({K}, {D}, {D})")
    if not np.isfinite(N).all() or (N < 0).any():
        raise ValueError("N must be finite and non-negative")
    if not (np.isfinite(sums).all() and np.isfinite(S).all()):
        raise ValueError("sums and S must be finite")
    for k in np.flatnonzero(N > 0):
        U, nu = new["U"][k], float(new["nu"][k])
        kap1, nu1, m1, _, U1, ld1 = native.niw_posterior(float(new["kappa"][k]), nu, new["m"][k], (U @ U.T) / nu, N[k:k + 1], sums[k:k + 1], S[k:k + 1],
                                                         nthreads=1)
        if not np.isfinite(ld1[0]):
            raise ValueError(f"the update of cluster {k + 1} is not positive definite")
        new["kappa"][k], new["nu"][k], new["m"][k], new["U"][k], new["logdet_psi"][k] = kap1[0], nu1[0], m1[0], U1[0], ld1[0]
        count[k] += N[k]
    return new, count


def _niw_arrays(post, what):
    """The five posterior arrays of `post` in Float64 (copies), K and D; ValueError for anything that is not K >= 1 NIW posteriors."""
    missing = [k for k in POST_KEYS[:4] if k not in post]
    if missing:
        raise ValueError(f"niw_graft is for NIW posteriors: {what} lacks {missing}")
    a = {k: np.array(post[k], np.float64) for k in POST_KEYS if k in post}
    if "logdet_psi" not in a and a["U"].ndim == 3 and a["U"].shape[1:] == a["m"].shape[1:] * 2:      # (a model file written without it, as niw_absorb)
        a["logdet_psi"] = 2 * np.log(np.einsum("kii->ki", a["U"])).sum(1) - a["m"].shape[1] * np.log(a["nu"])
    if "logdet_psi" not in a:
        raise ValueError(f"{what} must hold kappa, nu, logdet_psi (K,), m (K, D) and U (K, D, D)")
    K, D = a["m"].shape if a["m"].ndim == 2 else (0, 0)
    if a["m"].ndim != 2 or K < 1 or D < 1 or a["U"].shape != (K, D, D) or any(a[k].shape != (K,) for k in ("kappa", "nu", "logdet_psi")):
        raise ValueError(f"{what} must hold kappa, nu, logdet_psi (K,), m (K, D) and U (K, D, D)")
    if not all(np.isfinite(a[k]).all() for k in POST_KEYS):
        raise ValueError(f"{what} holds an entry that is not finite")
    return a, K, D


def niw_graft(post, points_count, new_post, new_count):
    """(post', points_count'): the posterior arrays of K clusters (`Predictor.post`) and their point counts with the K' clusters of
    `new_post` (the same five arrays, e.g. rows 3 k of a sub-fit's `sampler.post`) and `new_count` appended behind them.  Everything in
    Float64; the inputs are not modified; rows 0 .. K - 1 keep their bits and their numbers.  ValueError for shapes that do not fit
    (another D among them), an entry that is not finite, a negative count, and K + K' > binding.MAX_CLUSTERS."""
    from .. import binding
    old, K, D = _niw_arrays(post, "post")
    new, Kn, Dn = _niw_arrays(new_post, "new_post")
    if Dn != D:
        raise ValueError(f"new_post has {Dn} features, post {D}")
    count, ncount = np.array(points_count, np.float64), np.array(new_count, np.float64)
    if count.shape != (K,) or ncount.shape != (Kn,):
        raise ValueError("points_count and new_count must have one entry per cluster")
    if not (np.isfinite(count).all() and np.isfinite(ncount).all()) or (count < 0).any() or (ncount < 0).any():
        raise ValueError("points_count and new_count must be finite and non-negative")
    if K + Kn > binding.MAX_CLUSTERS:
        raise ValueError(f"{K} + {Kn} clusters exceed binding.MAX_CLUSTERS = {binding.MAX_CLUSTERS}")
    return {k: np.concatenate([old[k], new[k]]) for k in POST_KEYS}, np.concatenate([count, ncount])


def dirichlet_absorb(post, points_count, stats):
    """(post', points_count'): the posterior of K Multinomial clusters (`Predictor.post`: alpha (K, D)) and their point counts after the
    conjugate update alpha' = alpha + sums with `stats` -- anything with N (K,) and sums (K, D), e.g. a `CountStatistics`.  Everything in
    Float64, so the alpha returned is Float64 whatever it was; the inputs are not modified.  A cluster with N_k == 0 keeps its values.
    ValueError for a posterior that is not a Multinomial one, shapes that do not fit, a negative or non-finite N, and non-finite or
    negative sums."""
    if "alpha" not in post:
        raise ValueError(f"dirichlet_absorb is for posteriors of the Multinomial prior: post lacks 'alpha' (it holds {sorted(post)})")
    new = {k: np.array(post[k], np.float64 if k == "alpha" else None) for k in post}
    alpha = new["alpha"]
    if alpha.ndim != 2 or alpha.shape[0] < 1:
        raise ValueError("post must hold alpha (K, D)")
    K, D = alpha.shape
    count = np.array(points_count, np.float64)
    if count.shape != (K,):
        raise ValueError("points_count must have one entry per cluster")
    N, sums = (np.asarray(getattr(stats, f) if hasattr(stats, f) else stats[f], np.float64) for f in ("N", "sums"))
    if N.shape != (K,) or sums.shape != (K, D):
        raise ValueError(f"the statistics must be N ({K},) and sums ({K}, {D})")
    if not np.isfinite(N).all() or (N < 0).any():
        raise ValueError("N must be finite and non-negative")
    if not np.isfinite(sums).all():
        raise ValueError("sums must be finite")
    if (sums < 0).any():
        raise ValueError("sums must be non-negative: counts are")
    hit = N > 0
    alpha[hit] += sums[hit]
    count[hit] += N[hit]
    return new, count


def dirichlet_graft(post, points_count, new_post, new_count):
    """(post', points_count'): the posterior of K Multinomial clusters (`Predictor.post`: alpha (K, D)) and their point counts with the K'
    alpha rows of `new_post` (e.g. rows 3 k of a sub-fit's `sampler.post`) and `new_count` appended behind them.  Everything in Float64;
    the inputs are not modified; rows 0 .. K - 1 keep their values -- their bits when alpha is Float64 already -- and their numbers.
    ValueError for a posterior that is not a Multinomial one, shapes that do not fit (another D among them), an entry that is not finite or
    negative, a count that is not finite or negative, and K + K' > binding.MAX_CLUSTERS."""
    from .. import binding
    for what, p in (("post", post), ("new_post", new_post)):
        if "alpha" not in p:
            raise ValueError(f"dirichlet_graft is for posteriors of the Multinomial prior: {what} lacks 'alpha' (it holds {sorted(p)})")
    old, new = np.array(post["alpha"], np.float64), np.array(new_post["alpha"], np.float64)
    if old.ndim != 2 or old.shape[0] < 1 or old.shape[1] < 1 or new.ndim != 2 or new.shape[0] < 1:
        raise ValueError("post and new_post must hold alpha (K, D)")
    (K, D), (Kn, Dn) = old.shape, new.shape
    if Dn != D:
        raise ValueError(f"new_post has {Dn} features, post {D}")
    for what, a in (("post", old), ("new_post", new)):
        if not np.isfinite(a).all() or (a < 0).any():
            raise ValueError(f"{what} holds an alpha that is not finite or is negative")
    count, ncount = np.array(points_count, np.float64), np.array(new_count, np.float64)
    if count.shape != (K,) or ncount.shape != (Kn,):
        raise ValueError("points_count and new_count must have one entry per cluster")
    if not (np.isfinite(count).all() and np.isfinite(ncount).all()) or (count < 0).any() or (ncount < 0).any():
        raise ValueError("points_count and new_count must be finite and non-negative")
    if K + Kn > binding.MAX_CLUSTERS:
        raise ValueError(f"{K} + {Kn} clusters exceed binding.MAX_CLUSTERS = {binding.MAX_CLUSTERS}")
    out = {k: np.array(v) for k, v in post.items() if k != "alpha"}
    out["alpha"] = np.concatenate([old, new])
    return out, np.concatenate([count, ncount])
