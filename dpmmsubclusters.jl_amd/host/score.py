"""Scoring new points with a fitted model, at any n: a reusable `Predictor` over include/dpmm_hip_score.h.

`predict(dp_model, data)` creates a worker, loads the K posterior predictives, allocates an n-sized table and frees everything -- per
call.  A `Predictor` does the fixed part ONCE (one worker of `capacity` points, the predictive parameters loaded once) and then scores
data of any n in slabs of `capacity` points: labels, probabilities, the best m clusters, and the mixture's log-density (the outlier score).

  * `data` is what `predict` takes: an array, a torch tensor on the CPU or a GPU (eight element types, any strides), sparse columns for
    the Multinomial prior; Dimensions x Samples.
  * a full slab of a device tensor is read in place (its address is the tensor's plus lo * stride_point); the last, short slab goes
    through a staging buffer of `capacity` points that the Predictor keeps, and its outputs are cut to length: the worker always sees
    `capacity` points.
  * results for a device tensor are tensors on its device, written there by the library; otherwise numpy arrays.
  * a Predictor belongs to one GPU; for several GPUs open one each.

The values are those of `predict` (same kernels, same arithmetic per point).  Two caveats, both for dense Multinomial data: the worker
picks its storage path (Float32 / bf16-exact / bytes) per upload, here per slab, `predict` for the whole data.  For data of one kind
throughout (all counts, all bf16-exact, all other fractions) the two agree bit for bit whatever the capacity; for mixed data the last
bits can depend on `capacity`.  And on the byte path every upload re-allocates the worker's Float32 image (it is freed once the byte copy
exists): the scoring calls allocate nothing, the uploads of count data do.
"""
import collections

import numpy as np

from .. import binding
from . import points as _points
from . import priors as _priors
from . import tensors as _tensors      # noqa: F401  (the recognisers of host/points.py, reachable from here: tests patch them under this name)
from . import project as _project
from . import absorb as _absorb
from . import condition as _condition
from .absorb import niw_absorb, niw_graft, dirichlet_absorb, dirichlet_graft      # noqa: F401


Exemplars = collections.namedtuple("Exemplars", "typical_idx typical_score fringe_idx fringe_score count skipped")
Exemplars.__doc__ = """What `Predictor.exemplars` returns: typical_idx, typical_score, fringe_idx, fringe_score (K, m) -- a list that was not asked
for is None -- count (K,) and skipped, an int."""

Overlap = collections.namedtuple("Overlap", "matrix mass count skipped")
Overlap.__doc__ = """What `Predictor.overlap` returns: matrix (K, K) float64, O[k][j] = sum_i p_ik p_ij; mass (K,) float64, sum_i p_ik; count (K,)
int64, the points labelled k + 1; skipped, an int -- numpy arrays always."""

BatchStatistics = collections.namedtuple("BatchStatistics", "N sums S count skipped incomplete held_out")
BatchStatistics.__doc__ = """What `Predictor.statistics` returns and `Predictor.absorb` folds in: N (K,), sums (K, D), S (K, D, D) float64 -- sum_i w_ik,
sum_i w_ik x_i, sum_i w_ik x_i x_i' over the points that take part; count (K,) int64, those of them labelled k + 1; skipped, incomplete,
held_out, ints, the points that took no part -- numpy arrays always."""

CountStatistics = collections.namedtuple("CountStatistics", "N sums count skipped incomplete held_out")
CountStatistics.__doc__ = """What `Predictor.count_statistics` returns and `Predictor.absorb_counts` folds in: N (K,), sums (K, D) float64 -- sum_i w_ik,
sum_i w_ik x_i over the points that take part; count (K,) int64, those of them labelled k + 1; skipped, incomplete, held_out, ints, the
points that took no part -- numpy arrays always."""

Typicality = collections.namedtuple("Typicality", "labels mahalanobis tail skipped incomplete")
Typicality.__doc__ = """What `Predictor.typicality` returns: labels (n,) int64 1-based, mahalanobis (n,) float32, tail (n,) float32 -- tensors on
the data's device for a device tensor, else numpy arrays -- and skipped, incomplete, ints: the points whose mahalanobis and tail are NaN."""

Explanation = collections.namedtuple("Explanation", "labels mahalanobis tail residual zscore feature_tail features skipped incomplete")
Explanation.__doc__ = """What `Predictor.explain` returns: labels, mahalanobis, tail, skipped, incomplete as `Typicality`; residual, zscore,
feature_tail float32 -- (D, n) in feature order with features None, or with top=m (n, m) and features (n, m) int32, 0-based, the m features of
largest |zscore|, largest first -- tensors on the data's device for a device tensor, else numpy arrays."""

GroupExplanation = collections.namedtuple("GroupExplanation", "labels mahalanobis tail group_mahalanobis group_tail names sizes skipped incomplete")
GroupExplanation.__doc__ = """What `Predictor.explain_groups` returns: labels, mahalanobis, tail, skipped, incomplete as `Typicality`;
group_mahalanobis, group_tail (G, n) float32 in the order of `groups` -- `.T` views of point-major memory, tensors on the data's device for
a device tensor, else numpy arrays; names, the keys of a dict of groups (None for a sequence); sizes, a tuple of the G group sizes."""

HeldOut = collections.namedtuple("HeldOut", "points index total skipped incomplete")
HeldOut.__doc__ = """What `Predictor.held_out` returns: points (D, stored) float32 -- a view of the (stored, D) buffer the GPU wrote -- and index
(stored,) int64, 0-based positions in `data`, increasing -- tensors on the data's device for a device tensor, else numpy arrays; total, the
held-out points there are (stored = min(total, max_points)); skipped, incomplete, ints, as `statistics` counts them."""

HeldOutCounts = collections.namedtuple("HeldOutCounts", "points index total total_entries skipped incomplete")
HeldOutCounts.__doc__ = """What `Predictor.held_out_counts` returns: points (D, stored), following the input -- a dense float32 tensor on the data's
device or a numpy array; a torch.sparse_csc tensor (int32 indices, float32 values) for a sparse tensor; a scipy CSC matrix for scipy or tuple
input -- and index (stored,) int64, 0-based positions in `data`, increasing; total, total_entries, the held-out points there are and their
entries (dense data: D each); skipped, incomplete, ints, as `count_statistics` counts them."""

Growth = collections.namedtuple("Growth", "added sizes index labels dropped total model")
Growth.__doc__ = """What `Predictor.grow` returns: added, the number of clusters appended; sizes (added,) int64, their points; index (kept,) int64,
the 0-based positions in `data` of the points that went into them, increasing, and labels (kept,) int64, their new 1-based cluster ids
(K_old + 1 ..) -- numpy arrays; dropped, the captured points that went nowhere (a value that is not finite, or a sub-cluster below
min_points); total, the held-out points there were; model, the sub-fit's dp_model (None when nothing was fitted)."""

Regression = collections.namedtuple("Regression", "mean std labels skipped")
Regression.__doc__ = """What `Regressor.predict` returns: mean (D_t, n) float32, std the same or None, labels (n,) int64 1-based -- tensors on the
data's device for a device tensor, else numpy arrays -- and skipped, an int: the points whose mean and std columns are NaN."""

RegressionDraws = collections.namedtuple("RegressionDraws", "values components labels skipped")
RegressionDraws.__doc__ = """What `Regressor.sample` returns: values (draws, D_t, n) float32, draw j of the targets of every point; components
(draws, n) int32, the 0-based cluster each draw came from (-1: the point took no part), or None; labels (n,) int64 1-based, the marginal
model's -- tensors on the data's device for a device tensor, else numpy arrays -- and skipped, an int: the points whose columns are NaN in
every draw."""

ConditionalCDF = collections.namedtuple("ConditionalCDF", "cdf sf labels skipped")
ConditionalCDF.__doc__ = """What `Regressor.cdf` returns: cdf and sf (D_t, n) float32, P(target <= y) and P(target > y) given the given features,
each summed from the side that does not cancel; labels (n,) int64 1-based, the marginal model's -- tensors on the data's device for a
device tensor, else numpy arrays -- and skipped, an int: the points whose columns are NaN."""

RegressionQuantiles = collections.namedtuple("RegressionQuantiles", "values levels labels skipped")
RegressionQuantiles.__doc__ = """What `Regressor.quantile` returns: values (L, D_t, n) float32, values[q, d, i] the y at which the conditional CDF
of target d of point i reaches levels[q] (the orientation of `sample`'s draws); levels, a tuple of floats as asked for; labels and skipped
as `ConditionalCDF`."""

Recommendation = collections.namedtuple("Recommendation", "features prob labels skipped")
Recommendation.__doc__ = """What `Predictor.recommend` returns: features (n, m) int32, 0-based, the m candidates of largest next-count probability,
largest first, ties to the lower index, -1 where a point has fewer than m candidates; prob (n, m) float32, their probabilities, NaN
there; labels (n,) int64 1-based, what `predict_labels` gives -- tensors on the data's device for a device tensor, else numpy arrays --
and skipped, an int: the points that are -1 / NaN throughout."""

CountExplanation = collections.namedtuple("CountExplanation", "features count expected residual feature_tail labels total skipped incomplete")
CountExplanation.__doc__ = """What `Predictor.explain_counts` returns: features (n, top) int32, 0-based, the candidates of largest |residual|, largest
first, ties to the lower index, -1 where a point has fewer than `top` candidates; count, expected, residual, feature_tail (n, top) float32:
the point's count of the feature, t theta, the signed binomial deviance residual and the exact one-sided binomial tail on the side of the
deviation, NaN there; labels (n,) int64 1-based, what `predict_labels` gives; total (n,) float64, the points' totals t, NaN for a skipped
point -- tensors on the data's device for a device tensor, else numpy arrays -- and skipped, incomplete, ints: the points that are -1 / NaN
throughout."""

ASSIGN_MODES = {"hard": binding.BATCHSTATS_HARD, "soft": binding.BATCHSTATS_SOFT}


class _Capture:
    """Receives what prior.predictive_table would hand a worker."""

    def predict_table_niw(self, m, R, logdet, df, weights, points=False):
        self.args = ("niw", (m, R, logdet, df, weights))

    def predict_table_mult(self, logp, weights, points=False):
        self.args = ("mult", (logp, weights))


def alias_tables(theta):
    """Walker / Vose alias tables of the rows of `theta` (K, D), probabilities summing to 1 per row, built in Float64:
    (thr (K, D) uint32, alias (K, D) int32).  A draw takes bucket j uniformly and returns j when a uniform 32-bit word is below thr[j],
    else alias[j]: category d has probability (thr[d] + sum over the buckets j with alias[j] = d of (2^32 - thr[j])) / (2^32 D), which is
    theta[d] to within 2^-32 (a threshold is rounded down to a multiple of 2^-32, and at most D buckets of weight 1 / D point at d).  A
    full bucket is its own alias, so its threshold decides nothing; a category of probability 0 has threshold 0 and is nobody's alias."""
    theta = np.atleast_2d(np.asarray(theta, np.float64))
    K, D = theta.shape
    thr = np.zeros((K, D), np.uint32)
    alias = np.zeros((K, D), np.int32)
    for k in range(K):
        p = (theta[k] * D).tolist()
        small = [j for j in range(D) if p[j] < 1.0]
        large = [j for j in range(D) if p[j] >= 1.0]
        prob = [1.0] * D
        al = list(range(D))
        while small and large:
            s, g = small.pop(), large.pop()
            prob[s], al[s] = p[s], g
            p[g] = (p[g] + p[s]) - 1.0
            (small if p[g] < 1.0 else large).append(g)
        for j in small:                           # what rounding left over: buckets that are full to within the rounding of the sums
            if theta[k, j] <= 0.0:
                raise ValueError("alias_tables: the probabilities of a row do not sum to 1")
        t = np.floor(np.asarray(prob) * 4294967296.0)
        thr[k] = np.minimum(t, 4294967295.0).astype(np.uint32)
        alias[k] = al
    return thr, alias


def _device_index(device):
    if device is None or isinstance(device, (int, np.integer)):
        return device
    if isinstance(device, str):
        import torch
        device = torch.device(device)
    return device.index


MISSING_MODES = ("propagate", "marginalize")
GAPS_MODES = ("incomplete", "marginalize")      # `gaps` of Predictor.typicality / explain


def _floors(min_logdens, min_tail):
    """The two floors of `statistics`, `held_out` and `grow` as floats or None; ValueError for a NaN min_logdens or a min_tail outside (0, 1]."""
    if min_logdens is not None:
        min_logdens = float(min_logdens)
        if min_logdens != min_logdens:
            raise ValueError("min_logdens must not be NaN")
    if min_tail is not None:
        min_tail = float(min_tail)
        if not 0.0 < min_tail <= 1.0:
            raise ValueError("min_tail must lie in (0, 1]")
    return min_logdens, min_tail


def _count_floors(min_logdens, min_logdens_per_count):
    """The two floors of `count_statistics`, `held_out_counts` and `grow_counts` as floats or None; ValueError for a NaN."""
    out = []
    for name, v in (("min_logdens", min_logdens), ("min_logdens_per_count", min_logdens_per_count)):
        if v is not None:
            v = float(v)
            if v != v:
                raise ValueError(f"{name} must not be NaN")
        out.append(v)
    return out


# What the two priors do not share in `statistics` / `absorb` / `held_out` / `grow` and their `*_counts` twins: the worker's methods
# (stats + "_begin" ..., set_second, holdout + "_begin" ...), the floors' validator and the name of the second one, the conjugate update and
# the graft of host/absorb.py with the rows of the posterior a graft takes, the result tuple, and the words of the messages.  The
# `set_predictive_*` call is the one `_predictive_args` names.
_Family = collections.namedtuple("_Family", "stats set_second holdout floors floor2 absorb graft post_keys result noun by held wrong_prior")
_FAMILY = {
    _priors.PRIOR_NIW: _Family("batchstats", "batchstats_set_min_tail", "holdout", _floors, "min_tail", _absorb.niw_absorb, _absorb.niw_graft,
                               _absorb.POST_KEYS, BatchStatistics, "batch", "by their tail", "held-out points",
                               "{what} is for the NIW prior and dense points: the Multinomial prior and sparse stores are out of scope here "
                               "-- a Multinomial model has {what}_counts"),
    _priors.PRIOR_MULT: _Family("countstats", "countstats_set_per_count", "countholdout", _count_floors, "min_logdens_per_count",
                                _absorb.dirichlet_absorb, _absorb.dirichlet_graft, ("alpha",), CountStatistics, "count", "per count",
                                "held-out count points", "{what} is for the Multinomial prior: an NIW model has {base}"),
}


def _need(wk, message, *methods):
    """`wk` if it has every one of `methods` -- a stand-in worker may lack a call -- else RuntimeError(message)."""
    if not all(hasattr(wk, f) for f in methods):
        raise RuntimeError(message)
    return wk


# The short-slab rule of `Predictor._walk`: the worker scores the zero padding of a short slab too, and the padding is not ours.  A call
# marks a row that took no part in one of its outputs -- NaN in the first element of a float row, a negative first element of an integer
# row -- and _first_nan(name) / _first_negative(name) give absent(views, rows): how many of `rows` of views[name] carry the mark.
def _first_nan(name):
    def absent(views, rows):
        a = views[name][rows]
        a = a.reshape(a.shape[0], -1)[:, 0]
        return int((a != a).sum())
    return absent


def _first_negative(name):
    def absent(views, rows):
        a = views[name][rows]
        return int((a.reshape(a.shape[0], -1)[:, 0] < 0).sum())
    return absent


class _CompStage:
    """The drawn clusters of a draw call.  The ABI's comp is [m][capacity], one slab's: the call writes `stage`, and slice_in(lo, hi) slices the
    slab's points into `comp` (m, n).  wanted=False: no comp; always=True: the stage exists without comp too (it tells who took no part)."""

    def __init__(self, opened, m, capacity, wanted, always=False):
        n, new = opened[0], opened[2]
        self.comp = new(m, (n,), "int32") if wanted else None
        self.stage = new(m, (capacity,), "int32") if n and (wanted or always) else None

    def slice_in(self, lo, hi):
        if self.comp is not None and self.stage is not None:
            self.comp[:, lo:hi] = self.stage[:, :hi - lo]

    def absent(self, views, rows):
        return int((self.stage[0, rows] < 0).sum())


class _Stages:
    """The staging of a Predictor's short slab as host/points.py asks for it -- "host", "dev", "csc" -- kept on the Predictor as
    `_host_stage`, `_dev_stage`, `_csc_stage`; suffix "_in": the D_in-wide ones of dense data that is projected on the way in."""

    def __init__(self, owner, suffix):
        self.owner, self.suffix = owner, suffix

    def get(self, kind, make, fits=lambda st: True):
        """The kept storage if there is one and it fits, else what `make()` returns, kept from now on."""
        name = f"_{kind}_stage{self.suffix}"
        if getattr(self.owner, name) is None or not fits(getattr(self.owner, name)):
            setattr(self.owner, name, make())
        return getattr(self.owner, name)


class Predictor:
    """Predictor(dp_model, capacity=65536, device=None, worker_factory=None, missing="propagate"): see the module's description.  Use as a
    context manager or close().

    missing="propagate": a NaN feature makes every result of its point NaN / "cluster 1", as the reference's dense matrix would.
    missing="marginalize" (NIW only): a NaN feature is a MISSING one.  A point with 1 .. min(16, D - 1) of them is scored by the marginal
    of every cluster's Student-t over the features it has (include/dpmm_hip_missing.h) -- labels, probabilities, top-m, log-density and
    exemplars all follow; a point with more keeps its NaN results.  `missing_counts` holds (marginalised, over the cap) of the last call,
    (0, 0) under "propagate".  `impute` fills the gaps under either setting."""

    def __init__(self, dp_model, capacity=65536, device=None, worker_factory=None, missing="propagate"):
        s = dp_model.sampler
        rows = [3 * k for k in range(s.K)]
        post = {k: np.asarray(v)[rows] for k, v in s.post.items()}
        if device is None:
            device = getattr(getattr(s, "wk", None), "device", 0)
        hyper = None
        if s.prior.kind == _priors.PRIOR_NIW and all(hasattr(s.prior, k) for k in ("kappa", "m", "nu", "psi")):      # what `grow` fits new clusters under
            hyper = {k: getattr(s.prior, k) for k in ("kappa", "m", "nu", "psi")}
        prior_alpha = getattr(s.prior, "alpha", None) if s.prior.kind == _priors.PRIOR_MULT else None      # what `grow_counts` fits new clusters under
        self._setup(s.prior.kind, s.prior.dim, s.alpha, np.asarray(s.points_count), post, capacity, device, worker_factory,
                    projection=getattr(dp_model, "projection", None), missing=missing, prior_hyper=hyper, prior_alpha=prior_alpha)

    def _setup(self, kind, D, alpha, points_count, post, capacity, device, worker_factory, projection=None, missing="propagate", prior_hyper=None,
               prior_alpha=None):
        # the Multinomial prior's Dirichlet alpha (D,) in Float64, or None: an NIW model, or a model file written without it
        self.prior_alpha = None if prior_alpha is None else np.array(prior_alpha, np.float64).ravel()
        # the model's NIW hyper-parameters kappa, m (D,), nu, psi (D, D) in Float64, or None: a model file written without them
        self.prior_hyper = None if prior_hyper is None else {k: np.array(prior_hyper[k], np.float64) for k in ("kappa", "m", "nu", "psi")}
        if missing not in MISSING_MODES:
            raise ValueError('missing must be "propagate" or "marginalize"')
        if missing == "marginalize" and int(kind) != _priors.PRIOR_NIW:
            raise ValueError('missing="marginalize" is for the NIW prior: the Multinomial prior has no missing features')
        self.missing, self.missing_counts = missing, (0, 0)
        self.projection = projection     # host/project.py: D_in-row data is projected on the way in (the worker holds the map)
        self.kind, self.D, self.alpha = int(kind), int(D), float(alpha)
        self.points_count = np.asarray(points_count, np.float64).copy()
        self.post = {k: np.array(v) for k, v in post.items()}
        self.K = len(self.points_count)
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be at least 1")
        self._device_arg = device
        idx = _device_index(device)
        self.device = 0 if idx is None else int(idx)
        w = self.points_count + self.alpha                                   # weights as predict forms them
        self.weights = (w / w.sum()).astype(np.float32)
        which, args = self._predictive_args()
        factory = worker_factory or binding.Worker
        self._wk = factory(self.kind, self.D, self.capacity, first_index=0, device=self.device, seed=0)
        try:
            (self._wk.set_predictive_niw if which == "niw" else self._wk.set_predictive_mult)(*args)      # ONCE
            if projection is not None:
                projection.apply(self._wk)                                                                # ... as well
            if missing == "marginalize":
                self._wk.set_option(binding.OPT_SCORE_MISSING, 1)                                         # ... and this
        except Exception:
            self._wk.close()
            self._wk = None
            raise
        self._host_stage = None          # (capacity, D) float32, the short slab of host data
        self._host_stage_in = self._dev_stage_in = None      # the same, D_in wide, for data that is projected on the way in
        self._dev_stage = None           # the same on the device, for the short slab of a device tensor
        self._csc_stage = None           # capacity + 1 offsets on the device, for the short slab of a sparse_csc tensor
        self._out_stage = {}             # outputs of a short slab: name -> array / tensor of `capacity` rows
        self._sampler_set = False        # the sampler's tables are formed and uploaded by the first sample()
        self._recommend_set = False      # ... and the next-count probabilities by the first recommend()
        self._count_explain_set = False  # ... and the logarithms and the order of theta by the first explain_counts()
        self._groups_set = None          # ... and the group tables by explain_groups(): the groups they were made for

    def _predictive_args(self):
        """("niw" | "mult", the arguments of the worker's set_predictive_*) for `self.post` and `self.weights`."""
        prior = (_priors.niw_hyperparams(1.0, np.zeros(self.D), self.D + 3.0, np.eye(self.D)) if self.kind == _priors.PRIOR_NIW
                 else _priors.multinomial_hyper(np.ones(self.D)))
        cap = _Capture()
        prior.predictive_table(cap, self.post, list(range(self.K)), self.weights)
        return cap.args

    # ---- life
    def close(self):
        if getattr(self, "_wk", None) is not None:
            self._wk.close()
            self._wk = None
        self._host_stage = self._dev_stage = self._csc_stage = self._host_stage_in = self._dev_stage_in = None
        self._out_stage = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- a model to serve, without the training data or the sampler
    def save(self, path):
        """One .npz: prior kind, D, alpha, points_count, the posterior arrays of the K clusters, the projection, if the model has one, and
        the NIW hyper-parameters `grow` fits new clusters under (prior_kappa, prior_m, prior_nu, prior_psi) or the Multinomial prior's
        alpha `grow_counts` fits them under (prior_alpha), if the Predictor has them."""
        np.savez(path, kind=np.int64(self.kind), D=np.int64(self.D), alpha=np.float64(self.alpha), points_count=self.points_count,
                 **{"post_" + k: v for k, v in self.post.items()}, **(self.projection.arrays("proj_") if self.projection is not None else {}),
                 **({"prior_" + k: v for k, v in self.prior_hyper.items()} if self.prior_hyper is not None else {}),
                 **({"prior_alpha": self.prior_alpha} if self.prior_alpha is not None else {}))

    @classmethod
    def load(cls, path, device=None, capacity=65536, worker_factory=None, missing="propagate"):
        with np.load(path) as z:
            post = {k[5:]: z[k] for k in z.files if k.startswith("post_")}
            hyper = {k: z["prior_" + k] for k in ("kappa", "m", "nu", "psi")} if all("prior_" + k in z.files for k in ("kappa", "m", "nu", "psi")) else None
            self = cls.__new__(cls)
            self._setup(int(z["kind"]), int(z["D"]), float(z["alpha"]), z["points_count"], post, capacity, 0 if device is None else device, worker_factory,
                        projection=_project.Projection.from_arrays(z, "proj_"), missing=missing, prior_hyper=hyper,
                        prior_alpha=z["prior_alpha"] if "prior_alpha" in z.files else None)
        return self

    # ---- the public methods
    def predict(self, data):
        """(labels (n,) int64 1-based, probs (n, K) float32): what `predict(dp_model, data)` returns."""
        r = self._run(data, labels=True, probs=True)
        return r["labels"], r["probs"]

    def predict_labels(self, data):
        return self._run(data, labels=True)["labels"]

    def predict_topk(self, data, m):
        """(labels, idx (n, m) int64 1-based, best first, probs (n, m)): the m most probable clusters of every point, 1 <= m <= min(K, 16)."""
        m = int(m)
        if not 1 <= m <= min(self.K, binding.SCORE_MAX_TOP):
            raise ValueError(f"m must be in 1..{min(self.K, binding.SCORE_MAX_TOP)}")
        r = self._run(data, labels=True, m=m)
        return r["labels"], r["top_idx"], r["top_prob"]

    def score_samples(self, data):
        """(n,) float32: log of the mixture's posterior predictive density at every point."""
        return self._run(data, logdens=True)["logdens"]

    # ---- calibrated outlier scores (include/dpmm_hip_typicality.h)
    def _gaps_option(self, gaps, what):
        """The value of DPMM_OPT_TYPICALITY_GAPS for a call with `gaps`; raises before the worker is touched."""
        if gaps not in GAPS_MODES:
            raise ValueError('gaps must be "incomplete" or "marginalize"')
        if gaps == "incomplete":
            return 0
        if self.kind != _priors.PRIOR_NIW:
            raise ValueError(f'{what}: gaps="marginalize" is for the NIW prior: the Multinomial prior has no missing features')
        if self.missing != "marginalize":
            raise ValueError(f'{what}: gaps="marginalize" needs a Predictor made with missing="marginalize"')
        return 1

    def _with_gaps(self, on, run):
        """run() with DPMM_OPT_TYPICALITY_GAPS set for its duration (the option is never touched by a default call)."""
        if not on:
            return run()
        self._wk.set_option(binding.OPT_TYPICALITY_GAPS, 1)
        try:
            return run()
        finally:
            self._wk.set_option(binding.OPT_TYPICALITY_GAPS, 0)

    def typicality(self, data, gaps="incomplete"):
        """How typical every point is of the cluster it is given: a `Typicality` tuple, computed on the GPU.

          labels        (n,) int64, 1-based: bit-identical to `predict_labels(data)`;
          mahalanobis   (n,) float32: q_i = |R_k (x_i - m_k)|^2 for k = labels[i] - 1, the squared Mahalanobis distance of the point under
                        its own cluster's posterior predictive t_df(m_k, Sigma_k), Sigma_k^-1 = R_k' R_k, evaluated in Float32 from the
                        Float32 x, m, R the worker holds (with a projection: in the projected space);
          tail          (n,) float32: P(Q >= q_i) for a draw from that predictive -- Q / D ~ F(D, df_k), so the tail is the regularised
                        incomplete beta function I_{df / (df + q)}(df / 2, D / 2) -- evaluated in Float64 and rounded once.  It is
                        uniform on (0, 1) for points that belong to the cluster, whatever D, the cluster's scale or weight, before and
                        after an `absorb`: tail < 1e-6 means the same everywhere, which no threshold on `score_samples` does.
                        q == 0 gives exactly 1; tails below the smallest normal Float32 may come back as 0;
          skipped       points whose row of the table holds a NaN or no finite entry (the rule of `overlap` and `statistics`);
          incomplete    points that are not skipped but have a feature that is not finite: under missing="marginalize" a point with
                        gaps is labelled, but with gaps="incomplete" (the default) q is not marginalised.
        Skipped and incomplete points have mahalanobis = tail = NaN.  NIW only: the Multinomial predictive has no closed-form tail.
        gaps="marginalize" (a Predictor made with missing="marginalize" only, else ValueError): a point with 1 .. min(16, D - 1) NaN
        features whose observed features are finite is SCORED under the marginal t_df(m_O, Sigma_OO) of its cluster over the r features O
        it has: mahalanobis is q_o = z_O' (Sigma_OO)^-1 z_O -- the squared residual of the small system that gave the point its table entry,
        Float64 rounded once -- and tail is I_{df / (df + q_o)}(df / 2, (D - r) / 2), uniform on (0, 1) as for a complete point.  (Imputing
        first and scoring the filled point gives the same q but judges it with D degrees of freedom: every such point looks more typical
        than it is.)  `incomplete` then counts only the points still not scored -- an observed feature that is not finite; points with more
        gaps stay skipped.  Complete points keep their bits; `statistics`, `absorb`, `held_out`, `grow` and `min_tail` never marginalise.
        `data` is what `predict` takes; for a device tensor the three arrays are tensors on its device, written there by the library,
        nothing of size n crossing the host link.  No result depends on `capacity` or the table budget, to the bit."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        if self.kind != _priors.PRIOR_NIW:
            raise ValueError("typicality is for the NIW prior: the Multinomial predictive has no closed-form tail")
        on = self._gaps_option(gaps, "typicality")
        wk = _need(self._wk, "this Predictor's worker cannot score typicality (no dpmm_typicality_points)", "typicality_points_into")
        spec = [("labels", (), "int64"), ("mahalanobis", (), "float32"), ("tail", (), "float32")]
        # (the padding of a short slab is equal points with finite features: skipped or not, never incomplete)
        out, (sk, inc) = self._with_gaps(on, lambda: self._walk(self._open(data), spec, lambda views, lo, hi: wk.typicality_points_into(views),
                                                                absent=_first_nan("mahalanobis")))
        return Typicality(out["labels"], out["mahalanobis"], out["tail"], sk, inc)

    # ---- per-feature explanations (include/dpmm_hip_explain.h)
    def explain(self, data, top=None, gaps="incomplete"):
        """WHICH features make a point atypical of the cluster it is given: an `Explanation` tuple, computed on the GPU.

        `typicality` says that a point is far out; the first question then is which features are off.  A per-feature marginal z-score
        answers it badly: in a correlated cluster a point can sit twelve conditional standard deviations out while every marginal looks
        ordinary.  Under the point's own Student-t predictive the law of one feature given ALL the others is again a Student-t in closed
        form.  With k = labels[i] - 1, z = x_i - m_k, A = R_k' R_k = Sigma_k^-1, g = A z, q = mahalanobis[i], df = df_k:

          labels, mahalanobis, tail, skipped, incomplete    the values and classes of `typicality(data)`, bit for bit;
          residual      e_d = x_d - E[x_d | the other features, k] = g_d / A_dd, in the units of the data;
          zscore        t_d = g_d sqrt((df + D - 1) / (A_dd (df + q - g_d^2 / A_dd))): for a point of the cluster a Student-t variable with
                        df + D - 1 degrees of freedom, whatever its other features are -- comparable across features, clusters and D;
          feature_tail  P(|T| >= |t_d|) for that Student-t, evaluated in Float64 and rounded once: uniform on (0, 1) for points of the
                        cluster; zscore == 0 gives exactly 1.  At D = 1 it is `tail`.
        top=None: residual, zscore, feature_tail are (D, n) float32 in feature order (point-major memory, the `.T` view of an (n, D) array,
        as `impute` returns) and features is None.
        top=m, 1 <= m <= min(D, 16): the three arrays are (n, m), the layout of `predict_topk`, and features (n, m) int32 holds the 0-based
        m features of largest |zscore|, largest first, ties to the lower index, a NaN zscore last; nothing of size D n is formed.
        Skipped and incomplete points (see `typicality`) have NaN in the three arrays and -1 in features.
        gaps="marginalize" (see `typicality`): a point with r gaps is explained under the marginal over its D_o = D - r observed features O.
        With P = (Sigma_OO)^-1 = A_OO - A_OM A_MM^-1 A_MO, g' = P z_O and q_o = mahalanobis: residual = g'_d / P_dd is x_d minus its
        expectation given the OTHER OBSERVED features, zscore = g'_d sqrt((df + D_o - 1) / (P_dd (df + q_o - g'_d^2 / P_dd))) a Student-t
        variable with df + D_o - 1 degrees of freedom and feature_tail its two-sided tail.  A missing feature has NaN in the three arrays
        (top=None) or, ranked last, NaN and -1 in features (top=m > D_o).
        Float32 arithmetic from the Float32 x, m, R the worker holds; include/dpmm_hip_explain.h states the error bounds.  With a
        projection, D and the feature indices are those of the PROJECTED space (the coordinates `Projection.transform` gives), not the
        source features.  NIW only.  `data` is what `predict` takes; for a device tensor every array is a tensor on its device, written
        there by the library.  No result depends on `capacity`, the cut into uploads or the table budget, to the bit."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        if self.kind != _priors.PRIOR_NIW:
            raise ValueError("explain is for the NIW prior: the Multinomial predictive has no closed-form tail")
        m = 0
        if top is not None:
            m = int(top)
            if m != top or not 1 <= m <= min(self.D, binding.EXPLAIN_MAX_TOP):
                raise ValueError(f"top must be None or an integer in 1..{min(self.D, binding.EXPLAIN_MAX_TOP)}")
        on = self._gaps_option(gaps, "explain")
        wk = _need(self._wk, "this Predictor's worker cannot explain points (no dpmm_explain_points)", "explain_points_into")
        width = (m or self.D,)
        spec = [("labels", (), "int64"), ("mahalanobis", (), "float32"), ("tail", (), "float32"), ("residual", width, "float32"),
                ("zscore", width, "float32"), ("feature_tail", width, "float32")] + ([("features", width, "int32")] if m else [])
        # (the padding of a short slab: as `typicality`, never incomplete)
        out, (sk, inc) = self._with_gaps(on, lambda: self._walk(self._open(data), spec, lambda views, lo, hi: wk.explain_points_into(views, top=m),
                                                                absent=_first_nan("mahalanobis")))
        rows = [out[name] if m else out[name].T for name in ("residual", "zscore", "feature_tail")]
        return Explanation(out["labels"], out["mahalanobis"], out["tail"], rows[0], rows[1], rows[2], out["features"] if m else None, sk, inc)

    # ---- explanations by groups of features (include/dpmm_hip_explain_groups.h)
    def explain_groups(self, data, groups):
        """WHICH GROUP of features makes a point atypical of the cluster it is given: a `GroupExplanation` tuple, computed on the GPU.

        `explain` conditions one feature on all the others.  Features often come in blocks -- the parts of a concatenated embedding, the
        channels of a sensor, the one-hot columns of a variable, the lags of a series -- and inside a correlated block every feature is
        explained away by its block-mates while the block as a whole can be impossible.  Under the point's own Student-t predictive the
        law of a block G of s features given the other D - s is again a Student-t in closed form.  With the notation of `explain`
        (A = R_k' R_k, g = A z, q = mahalanobis[i], df = df_k):

          labels, mahalanobis, tail, skipped, incomplete    the values and classes of `typicality(data)`, bit for bit;
          group_mahalanobis   q_G = g_G' A_GG^-1 g_G, the squared length of the conditional residual x_G - E[x_G | the other features, k]
                              in the conditional metric; q - q_G is the squared distance of the other features under their marginal;
          group_tail          P(F >= f_G / s) for f_G = q_G (df + D - s) / (df + q - q_G), F ~ F(s, df + D - s), evaluated in Float64 and
                              rounded once: uniform on (0, 1) for points of the cluster, whatever the other features are, and comparable
                              across groups of different sizes, clusters and D.  A group of one feature gives `explain`'s feature_tail,
                              the group of all features gives `tail`.
        groups: a sequence of sequences of 0-based feature indices, or a dict name -> indices (`names` then holds the keys, in order):
        1 .. 64 groups, none empty, pairwise disjoint, not necessarily covering all features; the indices of a group are sorted on the way
        in.  Anything else is a ValueError before the GPU is touched.  Both arrays are (G, n) float32 in the order of `groups`, `.T` views of
        point-major memory as `explain` returns.  Skipped and incomplete points (see `typicality`) have NaN in both; on a
        missing="marginalize" Predictor a point with gaps is incomplete here.
        The per-cluster tables (the inverse Cholesky factors of A_GG, Float64 on the host, `condition.group_factors`) are formed by the
        first call and again after `absorb`, `grow` or for other groups.  Float32 arithmetic from the Float32 x, m, R the worker holds;
        include/dpmm_hip_explain_groups.h states the error bounds.  With a projection the indices are those of the PROJECTED space.
        NIW only.  No result depends on `capacity`, the cut into uploads or the table budget, to the bit."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        if self.kind != _priors.PRIOR_NIW:
            raise ValueError("explain_groups is for the NIW prior: the Multinomial predictive has no closed-form tail")
        names, idx = _condition.check_groups(groups, self.D, binding.EXPLAIN_MAX_GROUPS)
        wk = _need(self._wk, "this Predictor's worker cannot explain groups (no dpmm_explain_groups_points)", "set_explain_groups", "explain_groups_points_into")
        opened = self._open(data)
        key = tuple(tuple(g) for g in idx)
        if self._groups_set != key:
            R = np.asarray(self._predictive_args()[1][1], np.float32)      # what the worker was given
            wk.set_explain_groups(idx, _condition.group_factors(R, idx))
            self._groups_set = key
        width = (len(idx),)
        spec = [("labels", (), "int64"), ("mahalanobis", (), "float32"), ("tail", (), "float32"), ("group_mahalanobis", width, "float32"),
                ("group_tail", width, "float32")]
        # (the padding of a short slab: as `typicality`, never incomplete)
        out, (sk, inc) = self._walk(opened, spec, lambda views, lo, hi: wk.explain_groups_points_into(views), absent=_first_nan("mahalanobis"))
        return GroupExplanation(out["labels"], out["mahalanobis"], out["tail"], out["group_mahalanobis"].T, out["group_tail"].T, names,
                                tuple(len(g) for g in idx), sk, inc)

    # ---- exemplars (include/dpmm_hip_rank.h)
    def exemplars(self, data, m, which="both"):
        """The m most and the m least typical points of every cluster, selected on the GPU: an `Exemplars` tuple.

        Every point is labelled as `predict_labels` labels it and scored by s = the log predictive density of its OWN cluster plus
        log w_k (the largest entry of its row of the table `predict` normalises).  Points whose row holds a NaN or whose s is not finite
        are counted in `skipped` and appear nowhere else.  For cluster k (row k of every array, k = 0 .. K-1, the cluster `predict`
        calls k + 1):
          typical_idx[k]   the m points of the cluster with the largest s, best first; typical_score[k] their s, non-increasing;
          fringe_idx[k]    the m points with the smallest s, worst first; fringe_score[k] non-decreasing;
          count[k]         the points of the cluster that take part.
        Equal scores go to the lower index in both lists.  Slots j >= count[k] hold index -1 and score NaN.
        Indices are 0-BASED positions along the Samples axis of `data` -- `data[:, idx]` are the points -- while labels are 1-based.
        which: "typical", "fringe" or "both"; the list not asked for is None.  1 <= m <= binding.RANK_MAX_M.
        `data` is what `predict` takes; for a device tensor the arrays are tensors on its device, else numpy arrays.  Nothing of size n
        is allocated or copied to the host; the result does not depend on `capacity`."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        m = int(m)
        if not 1 <= m <= binding.RANK_MAX_M:
            raise ValueError(f"m must be in 1..{binding.RANK_MAX_M}")
        mask = {"typical": binding.RANK_TYPICAL, "fringe": binding.RANK_FRINGE, "both": binding.RANK_TYPICAL | binding.RANK_FRINGE}.get(which)
        if mask is None:
            raise ValueError('which must be "typical", "fringe" or "both"')
        wk = _need(self._wk, "this Predictor's worker cannot rank points (no dpmm_rank_begin)", "rank_begin")
        opened = self._open(data)
        wk.rank_begin(m, mask)
        self._walk(opened, [], lambda views, lo, hi: wk.rank_accumulate(lo, hi - lo))
        r = wk.rank_read(device=opened[1])
        typ, fr = mask & binding.RANK_TYPICAL, mask & binding.RANK_FRINGE
        return Exemplars(r["typ_idx"] if typ else None, r["typ_score"] if typ else None, r["fringe_idx"] if fr else None,
                         r["fringe_score"] if fr else None, r["count"], int(r["skipped"][0]))

    # ---- cluster overlap (include/dpmm_hip_overlap.h)
    def overlap(self, data):
        """How the clusters of the model relate on `data`: an `Overlap` tuple, accumulated on the GPU in Float64.

          matrix[k][j]   sum_i p_ik p_ij, p_i. the probabilities `predict` returns for point i: the expected number of points the model
                         puts in cluster k + 1 on one draw and in j + 1 on another; symmetric bit for bit;
          mass[k]        sum_i p_ik, the expected size of the cluster;
          count[k]       the points `predict_labels` labels k + 1;
          skipped        points whose row of the table holds a NaN or no finite entry: they are counted here and add nothing else.
        Every entry of matrix and mass lies within a relative n * 2^-52 of `P.double().T @ P.double()` (of its column sums) for
        the (n, K) matrix P of `predict`, whatever `capacity` is; count and skipped are exact.  `data` is what `predict` takes.  The
        arrays are numpy arrays (K * K numbers); nothing of size n is allocated or copied to the host.  `host.merge_tree` turns the
        result into the agglomerative hierarchy of the clusters."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        wk = _need(self._wk, "this Predictor's worker cannot accumulate the cluster overlap (no dpmm_overlap_begin)", "overlap_begin")
        opened = self._open(data)
        wk.overlap_begin()
        self._walk(opened, [], lambda views, lo, hi: wk.overlap_accumulate(hi - lo))
        r = wk.overlap_read()
        return Overlap(r["overlap"], r["mass"], r["count"], int(r["skipped"][0]))

    # ---- batch statistics and the conjugate update (include/dpmm_hip_batchstats.h, host/absorb.py)
    def statistics(self, data, assign="hard", min_logdens=None, min_tail=None):
        """The per-cluster sufficient statistics of `data` under the model: a `BatchStatistics` tuple, accumulated on the GPU in Float64.

          N[k]      sum_i w_ik          sums[k]   sum_i w_ik x_i          S[k]   sum_i w_ik x_i x_i', symmetric bit for bit
        with w_ik = 1 for the cluster `predict_labels` gives the point (assign="hard": N == count) or the probability `predict` gives
        (assign="soft"), over the points that TAKE PART.  Every point is counted in exactly one of
          skipped      its row of the table holds a NaN or no finite entry (as `overlap` skips it);
          held_out     min_logdens is given and `score_samples` of the point lies below it, or min_tail is given (a number in (0, 1]), the
                       point's features are all finite and its `typicality` tail lies below it: an outlier is not folded into a cluster.
                       The tail is the calibrated floor -- min_tail=1e-6 means the same at every D, for every cluster and after every
                       `absorb`, which no value of min_logdens does; either floor holds a point out;
          incomplete   a feature is not finite -- under missing="marginalize" a point with gaps is labelled, yet its moments are unknown;
          count[k]     it takes part and `predict_labels` labels it k + 1.
        x_i is the point as the model sees it: Float32, and with a projection its projected coordinates.  Every entry lies within
        2 gamma(n + 2) sum_i w_ik |x_id| |x_ie| of any other Float64 evaluation, whatever `capacity` is (include/dpmm_hip_batchstats.h);
        the counters are exact.  NIW only.  `data` is what `predict` takes; the arrays are numpy arrays (K D^2 numbers), nothing of
        size n is allocated or copied to the host."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        if self.kind != _priors.PRIOR_NIW:
            raise ValueError("statistics are for the NIW prior: a Multinomial model has count_statistics / absorb_counts")
        return self._statistics(data, assign, min_logdens, min_tail)

    def _statistics(self, data, assign, floor, second):
        """`statistics` and `count_statistics` behind their prior checks: begin, the second floor, the walk, read, the prior's tuple."""
        f = _FAMILY[self.kind]
        if assign not in ASSIGN_MODES:
            raise ValueError('assign must be "hard" or "soft"')
        floor, second = f.floors(floor, second)
        wk = _need(self._wk, f"this Predictor's worker cannot accumulate {f.noun} statistics (no dpmm_{f.stats}_begin)", f.stats + "_begin")
        if second is not None:
            _need(wk, f"this Predictor's worker cannot hold points out {f.by} (no dpmm_{f.set_second})", f.set_second)
        opened = self._open(data)
        getattr(wk, f.stats + "_begin")(ASSIGN_MODES[assign], floor)
        if second is not None:
            getattr(wk, f.set_second)(second)
        self._walk(opened, [], lambda views, lo, hi: getattr(wk, f.stats + "_accumulate")(hi - lo))
        r = getattr(wk, f.stats + "_read")()
        return f.result(**{k: int(r[k][0]) if k in ("skipped", "incomplete", "held_out") else r[k] for k in f.result._fields})

    def _absorb_statistics(self, stats):
        """`absorb` and `absorb_counts` behind their statistics: the conjugate update, the weights re-formed, one reload."""
        if not stats.N.sum() > 0:
            return stats
        self.post, self.points_count = _FAMILY[self.kind].absorb(self.post, self.points_count, stats)
        w = self.points_count + self.alpha
        self.weights = (w / w.sum()).astype(np.float32)
        self._reload()
        self._sampler_set = False            # the sampler's tables are those of the old posterior
        self._recommend_set = False          # ... and so are the next-count probabilities
        self._count_explain_set = False      # ... and the tables of explain_counts
        return stats

    def _reload(self):
        """The predictive parameters of `self.post` and `self.weights` into the worker."""
        which, args = self._predictive_args()
        getattr(self._wk, "set_predictive_" + which)(*args)
        self._groups_set = None              # the group tables are those of the old parameters

    def absorb(self, data, assign="hard", min_logdens=None, min_tail=None):
        """Folds `data` into the model and returns the `BatchStatistics` it absorbed (see `statistics` for the arguments).

        The NIW prior is conjugate: the posterior this Predictor carries is the exact prior of the batch, and `niw_absorb` updates every
        cluster that received weight -- kappa, nu, m, U, logdet_psi -- and `points_count`, hence the mixture weights.  The predictive
        parameters are then reloaded into the same worker, once, so every later call and `save` see the updated model; an accumulation
        begun before (`overlap`, `exemplars` pieces at the binding level) is refused afterwards.  Statistics with N.sum() == 0 change
        nothing.  No new cluster is created: points far from every cluster are either absorbed by the nearest one or, with
        `min_logdens` or `min_tail`, held out and counted.  `held_out` collects those points and `grow` turns them into new clusters."""
        return self._absorb_statistics(self.statistics(data, assign=assign, min_logdens=min_logdens, min_tail=min_tail))

    # ---- held-out points and new clusters (include/dpmm_hip_holdout.h, host/absorb.py)
    def _capture_front(self, kind, data, floor, second, caps, what):
        """What `_capture` and `_capture_counts` check before they set their destination up: (worker, the opened data, the two floors)."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        f = _FAMILY[kind]
        if self.kind != kind:
            raise ValueError(f.wrong_prior.format(what=what, base=what[:-7]))
        floor, second = f.floors(floor, second)
        if floor is None and second is None:
            raise ValueError(f"{what} needs a floor: min_logdens or {f.floor2}")
        for name, v in caps.items():
            if v != int(v) or int(v) < 0:
                raise ValueError(f"{name} must be a non-negative integer")
        _need(self._wk, f"this Predictor's worker cannot collect {f.held} (no dpmm_{f.holdout}_begin)", f.holdout + "_begin")
        return self._wk, self._open(data), floor, second

    def _capture(self, data, min_logdens, min_tail, max_points, what):
        """The held-out points of `data` as the GPU compacted them: (points (stored, D) float32 tensor, index (stored,) int64 tensor, the
        worker's counters, the torch device of device data or None)."""
        wk, opened, min_logdens, min_tail = self._capture_front(_priors.PRIOR_NIW, data, min_logdens, min_tail, dict(max_points=max_points), what)
        n, dev = opened[0], opened[1]
        import torch
        cap = min(int(max_points), n)
        where = torch.device(getattr(wk, "holdout_device", None) or f"cuda:{self.device}")      # (a stand-in worker names where its buffers live)
        points = torch.empty((cap, self.D), dtype=torch.float32, device=where)
        index = torch.empty((cap,), dtype=torch.int64, device=where)
        wk.holdout_begin(points, index, cap, min_logdens, min_tail)
        self._walk(opened, [], lambda views, lo, hi: wk.holdout_accumulate(lo, hi - lo))
        r = wk.holdout_read()                              # (waits for the worker's stream: the buffers are complete)
        return points[:r["stored"]], index[:r["stored"]], r, dev

    def held_out(self, data, min_logdens=None, min_tail=None, max_points=1 << 20):
        """The points of `data` that `statistics` / `absorb` would HOLD OUT under the same floors -- those far from every cluster, the ones
        that say the data has changed -- collected on the GPU while the score table goes by: a `HeldOut` tuple.

          points       (D, stored) float32, the points as the model sees them (with a projection: their projected coordinates), in
                       increasing position; a view of the (stored, D) buffer the library wrote, the layout `fit` and `predict` read in place;
          index        (stored,) int64, their 0-based positions along the Samples axis of `data`;
          total        the held-out points there are; stored = min(total, max_points) -- the FIRST max_points of them are kept;
          skipped, incomplete   as `statistics` counts them (a point in either class is never held out).
        At least one floor is required; both are validated as `statistics` validates them, and either one holds a point out.  points and
        index are tensors on the data's device when `data` is a device tensor -- nothing of size n crosses the host link, and nothing of
        size n is allocated beyond the destination of min(max_points, n) points -- else numpy arrays.  The result does not depend on
        `capacity` or the table budget, to the bit.  NIW and dense points only: the Multinomial prior and sparse stores are out of scope,
        and so are several ranks (each Predictor collects from the data it is given)."""
        points, index, r, dev = self._capture(data, min_logdens, min_tail, max_points, "held_out")
        if dev is None:
            points, index = points.cpu().numpy(), index.cpu().numpy()
        return HeldOut(points.T, index, r["total"], r["skipped"], r["incomplete"])

    def _prior_object(self, prior):
        """The niw_hyperparams `grow` fits under: the caller's, else the model's."""
        if prior is None and self.prior_hyper is not None:
            h = self.prior_hyper
            prior = _priors.niw_hyperparams(float(h["kappa"]), h["m"], float(h["nu"]), h["psi"])
        if prior is None:
            raise ValueError("grow needs the model's NIW hyper-parameters and this Predictor has none (a model file written without "
                             "prior_kappa / prior_m / prior_nu / prior_psi): pass prior=niw_hyperparams(...)")
        if getattr(prior, "kind", None) != _priors.PRIOR_NIW or getattr(prior, "dim", None) != self.D:
            raise ValueError(f"prior must be niw_hyperparams over the model's {self.D} dimensions")
        return prior

    def grow(self, data, min_logdens=None, min_tail=None, prior=None, alpha=None, iters=100, min_points=None, max_points=1 << 20, seed=0, **fit_kw):
        """Adds clusters for the part of `data` the model does not explain, and returns a `Growth` tuple.

        The held-out points of `data` (`held_out`, the same floors) are clustered where the GPU left them by the project's own sampler --
        `fit(points, prior, alpha, iters=iters, seed=seed, verbose=False, **fit_kw)`; they are already in the model's space, so no
        projection is applied -- and every cluster of that sub-fit with at least `min_points` points (default D + 1) is appended to the
        served model: its posterior (rows 3 k of the sub-model's `sampler.post`) behind the K the model has (`niw_graft`), its size to
        `points_count`; the weights are re-formed from points_count + alpha and the predictive parameters reloaded into the same worker,
        once.  The old clusters keep their numbers and their bits; every later call and `save` see K + added clusters.
          prior        niw_hyperparams for the new clusters; default: the model's own (`prior_hyper`, recorded from the fitted model and
                       kept by `save` / `load`).  A model file written before they were kept has none: ValueError unless prior= is given;
          alpha        of the sub-fit; default: the Predictor's;
          dropped      captured points that went into no new cluster: one with a value that is not finite (only the min_logdens floor can
                       hold such a point out), or a member of a sub-cluster below min_points.
        Nothing left to cluster, or no sub-cluster large enough: added = 0 and the model is untouched.  Any failure before the reload leaves
        the Predictor as it was.  `grow` does NOT absorb the points that take part: the idiom is
            p.grow(batch, min_tail=t); p.absorb(batch, min_tail=t)
        where the second call sees the GROWN model -- the points of the new clusters now take part and are folded into them (again: their
        posteriors already hold them once; absorb the batch first and grow afterwards if that matters).  NIW only; the Multinomial prior,
        sparse stores, several ranks and merging a new cluster with an old one are out of scope."""
        if self.kind != _priors.PRIOR_NIW:
            raise ValueError("grow is for the NIW prior and dense points: the Multinomial prior and sparse stores are out of scope here "
                             "-- a Multinomial model has grow_counts")
        hyper = self._prior_object(prior)
        alpha = self.alpha if alpha is None else float(alpha)
        if not alpha > 0:
            raise ValueError("alpha must be positive")
        min_points = self.D + 1 if min_points is None else int(min_points)
        if min_points < 1:
            raise ValueError("min_points must be at least 1")
        points, index, r, _ = self._capture(data, min_logdens, min_tail, max_points, "grow")
        import torch
        total = r["total"]
        finite = torch.isfinite(points).all(1)
        dropped = int(points.shape[0] - int(finite.sum()))
        if dropped:
            points, index = points[finite], index[finite]
        return self._grow_from(points.T if points.shape[0] else None, index, dropped, total, hyper, alpha, iters, min_points, seed, fit_kw, "grow")

    def _grow_from(self, points, index, dropped, total, hyper, alpha, iters, min_points, seed, fit_kw, what):
        """The end of `grow` and `grow_counts`: `points` (None: there are none) and `index`, the captured points already cut to the
        finite ones, are clustered by the sub-fit, and its clusters of at least min_points points are grafted behind the model's."""
        none = np.zeros(0, np.int64)
        if points is None:
            return Growth(0, none, none, none, dropped, total, None)
        f, K0 = _FAMILY[self.kind], self.K
        from . import api as _api
        res = _api.fit(points, hyper, alpha, iters=int(iters), seed=seed, verbose=False, **fit_kw)
        model, lab = res[8], res[0]
        lab = (lab.cpu().numpy() if hasattr(lab, "cpu") else np.asarray(lab)).astype(np.int64)
        s = model.sampler
        sizes = np.bincount(lab - 1, minlength=s.K)
        if len(sizes) != s.K or len(lab) != index.shape[0]:
            raise RuntimeError(f"{what}: the sub-fit's labels do not match its clusters")
        keep = np.flatnonzero(sizes >= min_points)
        dropped += int(sizes.sum() - sizes[keep].sum())
        if len(keep) == 0:
            return Growth(0, none, none, none, dropped, total, model)
        post, count = f.graft(self.post, self.points_count, {k: np.asarray(s.post[k])[3 * keep] for k in f.post_keys}, sizes[keep])
        w = count + self.alpha
        old = self.post, self.points_count, self.weights, self.K
        self.post, self.points_count, self.weights, self.K = post, count, (w / w.sum()).astype(np.float32), len(count)
        try:
            self._reload()                                 # ONCE, with the new K
        except Exception:
            self.post, self.points_count, self.weights, self.K = old
            raise
        self._sampler_set = False                          # the sampler's tables are those of the old K
        self._recommend_set = False                        # ... and so are the next-count probabilities
        self._count_explain_set = False                    # ... and the tables of explain_counts
        new_id = np.zeros(s.K, np.int64)
        new_id[keep] = K0 + 1 + np.arange(len(keep))
        kept = new_id[lab - 1] > 0
        return Growth(len(keep), sizes[keep].astype(np.int64), index.cpu().numpy()[kept], new_id[lab - 1][kept], dropped, total, model)

    # ---- count statistics and the Dirichlet update (include/dpmm_hip_countstats.h, host/absorb.py)
    def count_statistics(self, data, assign="hard", min_logdens=None, min_logdens_per_count=None):
        """The per-cluster sufficient statistics of count `data` under a Multinomial model: a `CountStatistics` tuple, accumulated on the
        GPU in Float64.

          N[k]      sum_i w_ik          sums[k]   sum_i w_ik x_i
        with w_ik = 1 for the cluster `predict_labels` gives the point (assign="hard": N == count) or the probability `predict` gives
        (assign="soft"), over the points that TAKE PART.  Every point is counted in exactly one of
          skipped      its row of the table holds a NaN or no finite entry (as `overlap` skips it);
          held_out     min_logdens is given and `score_samples` of the point lies below it, or min_logdens_per_count is given, every value
                       of the point is finite, its total t (the Float64 sum of its values) is positive and `score_samples` of the point lies
                       below min_logdens_per_count * t: an outlier is not folded into a cluster.  The log-density scales with the number of
                       counts in the point, so min_logdens is mostly a length filter; the log-density PER COUNT -- the log of the inverse
                       perplexity -- is comparable across lengths and is what this prior has in the place of `min_tail`;
          incomplete   a value of it is not finite (of its D features, or of its stored entries when the data is sparse);
          count[k]     it takes part and `predict_labels` labels it k + 1.
        `data` is whatever `predict` takes for a Multinomial model -- a dense array or tensor, scipy CSC, the (colptr, rowval, nzval,
        shape) tuple, a torch.sparse_csc tensor on the host or the device -- and is read from the store the worker keeps it in: Float32,
        the lossless byte copy of small integer counts, or sparse columns; nothing is densified.  With assign="hard" and integer data the
        sums are exact and the same to the bit whatever the capacity or the store; otherwise every entry lies within
        2 gamma(n + 2) sum_i w_ik |x_id| of any other Float64 evaluation (include/dpmm_hip_countstats.h); the counters are exact.
        Multinomial only.  The arrays are numpy arrays (K D numbers), nothing of size n is allocated or copied to the host."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        if self.kind != _priors.PRIOR_MULT:
            raise ValueError("count_statistics are for the Multinomial prior: an NIW model has statistics / absorb")
        return self._statistics(data, assign, min_logdens, min_logdens_per_count)

    def absorb_counts(self, data, assign="hard", min_logdens=None, min_logdens_per_count=None):
        """Folds count `data` into a Multinomial model and returns the `CountStatistics` it absorbed (see `count_statistics`).

        The Dirichlet prior is conjugate: `dirichlet_absorb` adds the sums to alpha -- kept in Float64 from then on -- of every cluster
        that received weight, and N to `points_count`, hence the mixture weights.  The predictive parameters are then reloaded into the
        same worker, once, so every later call, `sample` and `save` see the updated model; an accumulation begun before is refused
        afterwards.  Statistics with N.sum() == 0 change nothing.  No new cluster is created: points far from every cluster are absorbed
        by the nearest one or, with a floor, held out and counted; `held_out_counts` collects those and `grow_counts` turns them into new
        clusters."""
        return self._absorb_statistics(self.count_statistics(data, assign=assign, min_logdens=min_logdens, min_logdens_per_count=min_logdens_per_count))

    # ---- held-out count points and new clusters (include/dpmm_hip_countholdout.h, host/absorb.py)
    def _capture_counts(self, data, min_logdens, min_logdens_per_count, max_points, max_entries, what):
        """The held-out points of count `data` as the GPU compacted them: (sparse?, the destination tensors cut to what was stored, the
        worker's counters, the Points description of `data`)."""
        wk, opened, min_logdens, per_count = self._capture_front(_priors.PRIOR_MULT, data, min_logdens, min_logdens_per_count,
                                                                 dict(max_points=max_points, max_entries=max_entries), what)
        n = opened[0]
        pts = _points.describe(data)
        sparse = pts.is_sparse and hasattr(wk, "upload_points_csc")          # (a worker without the sparse upload is given dense rows)
        import torch
        where = torch.device(getattr(wk, "holdout_device", None) or f"cuda:{self.device}")      # (a stand-in worker names where its buffers live)
        if sparse:
            nnz = int(pts.desc.nnz_extent) if hasattr(pts, "desc") else int(len(pts.csc.data))
            cap, ecap = min(int(max_points), n), min(int(max_entries), nnz)
            dst = dict(colptr=torch.empty((cap + 1,), dtype=torch.int64, device=where), rowval=torch.empty((ecap,), dtype=torch.int32, device=where),
                       val=torch.empty((ecap,), dtype=torch.float32, device=where), entry_cap=ecap)
        else:
            cap = min(int(max_points), n, int(max_entries) // self.D)
            dst = dict(points=torch.empty((cap, self.D), dtype=torch.float32, device=where))
        dst.update(index=torch.empty((cap,), dtype=torch.int64, device=where), cap=cap)
        wk.countholdout_begin(dst, min_logdens, per_count)
        self._walk(opened, [], lambda views, lo, hi: wk.countholdout_accumulate(lo, hi - lo))
        r = wk.countholdout_read()                         # (waits for the worker's stream: the buffers are complete)
        st, se = r["stored"], r["stored_entries"]
        if sparse:
            if cap == 0:
                dst["colptr"] = torch.zeros((1,), dtype=torch.int64, device=where)
            got = dict(colptr=dst["colptr"][:st + 1], rowval=dst["rowval"][:se], val=dst["val"][:se], index=dst["index"][:st])
        else:
            got = dict(points=dst["points"][:st], index=dst["index"][:st])
        return sparse, got, r, pts

    def held_out_counts(self, data, min_logdens=None, min_logdens_per_count=None, max_points=1 << 20, max_entries=1 << 24):
        """The points of count `data` that `count_statistics` / `absorb_counts` would HOLD OUT under the same floors -- the documents no
        topic of the model explains -- collected on the GPU while the score table goes by: a `HeldOutCounts` tuple.

          points       (D, stored), the points as the worker holds them, in increasing position, and following the input: dense data gives a
                       float32 tensor on the data's device (a view of the (stored, D) buffer the library wrote) or a numpy array for host
                       data; a torch.sparse_csc tensor gives one on its device, int32 indices (the int64 offsets cast alongside the int32
                       rows) and float32 values; scipy CSC or the (colptr, rowval, nzval, shape) tuple gives a scipy CSC matrix.  `fit` and
                       `predict` read these layouts in place;
          index        (stored,) int64, their 0-based positions along the Samples axis of `data`;
          total, total_entries   the held-out points there are and their entries (dense data: D per point);
          skipped, incomplete    as `count_statistics` counts them (a point in either class is never held out).
        At least one floor is required; either one holds a point out (see `count_statistics`).  The points kept are the longest prefix
        inside both caps: dense data keeps the first min(max_points, n, max_entries // D) held-out points; sparse data the first
        max_points whose entries all lie inside min(max_entries, nnz(data)) -- a point whose entries do not all fit is dropped with every
        point behind it.  Nothing of size n crosses the host link and nothing of size n is allocated beyond the destination.  The result
        does not depend on `capacity`, the caps or the table budget, to the bit.  Multinomial only; several ranks are out of scope."""
        sparse, got, r, pts = self._capture_counts(data, min_logdens, min_logdens_per_count, max_points, max_entries, "held_out_counts")
        index = got["index"]
        if not sparse:
            points = got["points"]
            if pts.torch_device is None:
                points, index = points.cpu().numpy(), index.cpu().numpy()
            points = points.T
        else:
            import torch
            stored = int(index.shape[0])
            if isinstance(data, torch.Tensor):
                points = torch.sparse_csc_tensor(got["colptr"].to(torch.int32), got["rowval"], got["val"], size=(self.D, stored)).to(data.device)
                index = index.to(data.device)
            else:
                import scipy.sparse
                points = scipy.sparse.csc_matrix((got["val"].cpu().numpy(), got["rowval"].cpu().numpy(), got["colptr"].cpu().numpy()), shape=(self.D, stored))
                index = index.cpu().numpy()
        return HeldOutCounts(points, index, r["total"], r["total_entries"], r["skipped"], r["incomplete"])

    def _prior_alpha_object(self, prior):
        """The multinomial_hyper `grow_counts` fits under: the caller's, else the model's."""
        if prior is None and self.prior_alpha is not None:
            prior = _priors.multinomial_hyper(self.prior_alpha)
        if prior is None:
            raise ValueError("grow_counts needs the model's Multinomial prior and this Predictor has none (a model file written without "
                             "prior_alpha): pass prior=multinomial_hyper(alpha)")
        if getattr(prior, "kind", None) != _priors.PRIOR_MULT or getattr(prior, "dim", None) != self.D:
            raise ValueError(f"prior must be multinomial_hyper over the model's {self.D} features")
        return prior

    def grow_counts(self, data, min_logdens=None, min_logdens_per_count=None, prior=None, alpha=None, iters=100, min_points=10, max_points=1 << 20,
                    max_entries=1 << 24, seed=0, **fit_kw):
        """Adds clusters for the part of count `data` the model does not explain, and returns a `Growth` tuple: `grow` for the Multinomial
        prior.

        The held-out points of `data` (`held_out_counts`, the same floors and caps) are clustered where the GPU left them -- sparse data
        stays sparse -- by the project's own sampler, `fit(points, prior, alpha, iters=iters, seed=seed, verbose=False, **fit_kw)`, and every
        cluster of that sub-fit with at least `min_points` points is appended to the served model: its alpha row (row 3 k of the
        sub-model's `sampler.post`) behind the K the model has (`dirichlet_graft`), its size to `points_count`; the weights are re-formed
        from points_count + alpha and the predictive parameters reloaded into the same worker, once.  The old clusters keep their numbers
        and their bits; every later call, `sample` and `save` see K + added clusters.
          prior        multinomial_hyper for the new clusters; default: the model's own (`prior_alpha`, recorded from the fitted model and
                       kept by `save` / `load`).  A model file written before it was kept has none: ValueError unless prior= is given;
          alpha        of the sub-fit; default: the Predictor's;
          dropped      captured points that went into no new cluster: one with a value that is not finite, or a member of a sub-cluster
                       below min_points.
        Nothing left to cluster, or no sub-cluster large enough: added = 0 and the model is untouched.  Any failure before the reload leaves
        the Predictor as it was.  `grow_counts` does NOT absorb: the idiom is
            p.grow_counts(batch, min_logdens_per_count=f); p.absorb_counts(batch, min_logdens_per_count=f)
        where the second call sees the GROWN model.  Multinomial only; several ranks and merging a new cluster with an old one are out of
        scope."""
        if self.kind != _priors.PRIOR_MULT:
            raise ValueError("grow_counts is for the Multinomial prior: an NIW model has grow")
        hyper = self._prior_alpha_object(prior)
        alpha = self.alpha if alpha is None else float(alpha)
        if not alpha > 0:
            raise ValueError("alpha must be positive")
        min_points = int(min_points)
        if min_points < 1:
            raise ValueError("min_points must be at least 1")
        sparse, got, r, _ = self._capture_counts(data, min_logdens, min_logdens_per_count, max_points, max_entries, "grow_counts")
        import torch
        total = r["total"]
        index = got["index"]
        stored = int(index.shape[0])
        if sparse:                                         # a value that is not finite drops its column
            colptr, rowval, val = got["colptr"], got["rowval"], got["val"]
            lens = colptr[1:] - colptr[:-1]
            finite = torch.ones((stored,), dtype=torch.bool, device=index.device)
            okv = torch.isfinite(val)
            if not bool(okv.all()):
                col = torch.repeat_interleave(torch.arange(stored, device=index.device), lens)
                finite[col[~okv]] = False
                keep_e = finite[col]
                rowval, val, lens = rowval[keep_e], val[keep_e], lens[finite]
                colptr = torch.cat([torch.zeros((1,), dtype=torch.int64, device=index.device), torch.cumsum(lens, 0)])
        else:
            finite = torch.isfinite(got["points"]).all(1)
        dropped = int(stored - int(finite.sum()))
        if dropped:
            index = index[finite]
        if index.shape[0] == 0:
            points = None
        elif sparse:
            points = torch.sparse_csc_tensor(colptr.to(torch.int32), rowval, val, size=(self.D, int(index.shape[0])))
        else:
            points = (got["points"][finite] if dropped else got["points"]).T
        return self._grow_from(points, index, dropped, total, hyper, alpha, iters, min_points, seed, fit_kw, "grow_counts")

    # ---- a fixed split of the features (host/condition.py, include/dpmm_hip_regress.h)
    def _refuse_conditioning(self, what):
        if self.kind != _priors.PRIOR_NIW:
            raise ValueError(f"{what} is for the NIW prior: a Multinomial model has no Gaussian marginals")
        if self.projection is not None:
            raise ValueError(f"{what} is refused for a model with a projection: its features are mixtures of the source features")

    def marginal(self, features, capacity=None, worker_factory=None, missing=None):
        """A new Predictor over exactly the features `features` (distinct 0-based indices, 1 <= len <= D - 1), in the order given: the
        marginal of an NIW posterior is an NIW posterior (host/condition.py), so everything a Predictor serves works on it -- `absorb`,
        `grow`, `save` and `load` included: the hyper-parameters are marginalised by the same rule.  capacity, device and `missing` are
        this Predictor's unless given.  NIW only, no projection; ValueError before any worker is made."""
        self._refuse_conditioning("marginal")
        idx = _condition.check_features(features, self.D)
        hyper = _condition.hyper_marginal(self.prior_hyper, idx) if self.prior_hyper is not None else None
        new = Predictor.__new__(Predictor)
        new._setup(self.kind, len(idx), self.alpha, self.points_count, _condition.niw_marginal(self.post, idx), capacity or self.capacity,
                   self._device_arg, worker_factory, missing=missing or self.missing, prior_hyper=hyper)
        return new

    def regressor(self, given, targets=None, capacity=None, worker_factory=None):
        """A `Regressor` from the features `given` to `targets` (default: every other feature): see the class."""
        return Regressor(self, given, targets, capacity=capacity, worker_factory=worker_factory)

    # ---- missing features (include/dpmm_hip_missing.h)
    def impute(self, data, draws=None, seed=0, return_components=False):
        """(D, n) float32: `data` converted to Float32 with the NaN features of every point that has 1 .. min(16, D - 1) of them replaced
        by sum_k p_k E[x_M | x_O, k] -- the conditional means of the clusters' Student-t predictives, mixed with the probabilities
        `predict` gives the point under missing="marginalize".  Everything else -- observed features, complete points, points with more NaN
        features than that -- is copied bit for bit.  NIW only; works under either `missing` setting and sets `missing_counts`.
        A numpy array for host data; for a device tensor a tensor on its device (point-major memory: the `.T` view of an (n, D) tensor),
        written there by the library, nothing of size n crossing the host link.  Integer data has no NaN and comes back converted.

        draws=m (an int >= 1): MULTIPLE IMPUTATION, (m, D, n) float32 -- m completed copies of the data, copy j with the gaps of every
        such point DRAWN from p(x_M | x_O) under the fitted mixture (include/dpmm_hip_impute.h: a cluster k ~ p_k, then the conditional
        Student-t of that cluster) in place of their mean; each [j] has the layout described above.  The mean is the right point estimate
        and the wrong data set (too little variance, inflated correlations, intervals too narrow downstream): analyse the m copies
        separately and pool.  Draw j of point i depends on (seed, i = its position in `data`, j, the point, the model) alone -- not on
        `capacity`, not on m: the first draws of a longer run are those of a shorter one.  return_components=True: also the (m, n) int32
        drawn clusters, 0-based, -1 for every point that was not drawn for.  The table is evaluated once per slab for all m draws."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        if self.kind != _priors.PRIOR_NIW:
            raise ValueError("impute is for the NIW prior: the Multinomial prior has no missing features")
        wk = self._wk
        if draws is not None:
            return self._impute_draws(data, draws, seed, return_components)
        if return_components:
            raise ValueError("return_components is for draws=m: the mean imputation mixes all clusters")
        _need(wk, "this Predictor's worker cannot impute points (no dpmm_impute_points)", "impute_points_into")
        out, _ = self._walk(self._open(data, refuse_projected="impute"), [("impute", (self.D,), "float32")],
                            lambda views, lo, hi: wk.impute_points_into(views["impute"]), counts=True)
        return out["impute"].T

    def _impute_draws(self, data, draws, seed, return_components):
        m, seed = int(draws), int(seed)
        if m < 1 or m != draws or m > binding.IMPUTE_MAX_DRAWS:
            raise ValueError(f"draws must be None or an integer in 1..{binding.IMPUTE_MAX_DRAWS}")
        if seed < 0 or seed >> 64:
            raise ValueError("seed must be in 0..2^64 - 1")
        wk = _need(self._wk, "this Predictor's worker cannot draw missing features (no dpmm_impute_draw_points)", "impute_draws_into")
        opened = self._open(data, refuse_projected="impute")
        cs = _CompStage(opened, m, self.capacity, return_components)

        def evaluate(views, lo, hi):
            wk.impute_draws_into(views["draws"], seed, lo, comp=cs.stage)          # the global index of a point is its position in `data`
            cs.slice_in(lo, hi)
        out = self._walk(opened, [("draws", (m, self.D), "float32")], evaluate, counts=True)[0]["draws"]      # (n, m, D): ld = m D, draw_stride = D
        res = out.permute(1, 2, 0) if hasattr(out, "permute") else out.transpose(1, 2, 0)
        return (res, cs.comp) if return_components else res

    # ---- drawing points (include/dpmm_hip_sample.h)
    def sampler_tables(self):
        """What the sampler uploads, formed in Float64: NIW ("niw", m (K, D), A (K, D, D) = sqrt(c) U, df (K,)) -- the posterior
        predictive MvT(df, m, A A') that `predict` scores with -- or ("mult", theta (K, D), thr, alias)."""
        if self.kind == _priors.PRIOR_NIW:
            kap, nu, U = (np.asarray(self.post[k], np.float64) for k in ("kappa", "nu", "U"))
            df = nu - self.D + 1
            c = (kap + 1) / (kap * df)
            return "niw", np.asarray(self.post["m"], np.float64), np.sqrt(c)[:, None, None] * np.triu(U), df
        a = np.asarray(self.post["alpha"], np.float64)
        theta = a / a.sum(1, keepdims=True)
        return ("mult", theta) + alias_tables(theta)

    def cluster_sizes(self, n, seed=0):
        """n_k ~ Multinomial(n, weights) from numpy's Philox generator: a function of (seed, n) and the model alone."""
        w = self.points_count + self.alpha
        return np.random.Generator(np.random.Philox(int(seed))).multinomial(int(n), w / w.sum()).astype(np.int64)

    def sample(self, n, seed=0, trials=None, sparse=False):
        """(data, labels): n new points from the fitted mixture, drawn on the GPU.

        data     (D, n), Dimensions x Samples, on this Predictor's device: a Float32 tensor whose memory is point-major (the `.T` view of
                 an (n, D) tensor: what `fit` and `predict` read in place), or with sparse=True (Multinomial) a torch.sparse_csc tensor
                 with Int64 indices and Float32 counts, rows strictly increasing inside a column, no stored zero.
        labels   (n,) int64 tensor, 1-based and NON-DECREASING: the points come grouped by cluster, as scikit-learn's
                 GaussianMixture.sample returns them (torch.randperm shuffles them).  The cluster sizes are one Multinomial(n, weights) draw
                 on the host (`cluster_sizes`).
        NIW: the posterior predictive Student-t that `predict` scores with.  Multinomial: Multinomial(trials, alpha' / sum(alpha')) -- `trials`
        per point is required (and refused for NIW); sparse=True allows at most binding.SAMPLE_MAX_TRIALS_SPARSE trials.
        Point i depends on (seed, i, its cluster, the model) only: the same seed gives the same bits whatever `capacity` is, and a
        Predictor restored by `load` draws what the saved one drew.  A model fitted with a projection draws in the PROJECTED space: the
        points have d rows, the coordinates `Projection.transform` gives, not the D_in of the original data."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        n, seed = int(n), int(seed)
        if n < 0:
            raise ValueError("n must not be negative")
        if seed < 0 or seed >> 64:
            raise ValueError("seed must be in 0..2^64 - 1")
        mult = self.kind == _priors.PRIOR_MULT
        if mult:
            if trials is None:
                raise ValueError("the Multinomial prior needs `trials`, the number of trials per point")
            trials = int(trials)
            if trials < 1:
                raise ValueError("trials must be at least 1")
            limit = binding.SAMPLE_MAX_TRIALS_SPARSE if sparse else binding.SAMPLE_MAX_TRIALS_DENSE
            if trials > limit:
                raise ValueError(f"trials must not exceed {limit}" + (" for sparse output (DPMM_SAMPLE_MAX_TRIALS_SPARSE)" if sparse else ""))
            if sparse and self.D > 65536:
                raise ValueError("sparse output needs D <= 65536")
        else:
            if trials is not None:
                raise ValueError("`trials` is for the Multinomial prior")
            if sparse:
                raise ValueError("sparse output is for the Multinomial prior")
        wk, cap, D = self._wk, self.capacity, self.D
        _need(wk, "this Predictor's worker cannot draw points (no dpmm_sample_points_device)", "sample_points_raw")
        import torch
        if not self._sampler_set:
            t = self.sampler_tables()
            if t[0] == "niw":
                wk.set_sampler_niw(t[1], t[2], t[3])
            else:
                wk.set_sampler_mult(t[2], t[3])
            self._sampler_set = True
        dev = torch.device("cuda", self.device)
        n_k = self.cluster_sizes(n, seed)
        starts = np.concatenate([[0], np.cumsum(n_k)]).astype(np.int64)
        tr = trials if mult else 0
        if not sparse:
            x = torch.empty((n, D), dtype=torch.float32, device=dev)
            labels = torch.empty((n,), dtype=torch.int64, device=dev)
            torch.cuda.current_stream(dev).synchronize()       # nothing queued on torch's stream still uses this memory
            for lo in range(0, n, cap):
                wk.sample_points_raw(lo, min(cap, n - lo), starts, seed, tr, x=x.data_ptr() + 4 * lo * D, ld=D, labels=labels.data_ptr() + 8 * lo)
            return x.T, labels
        colptr = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        nnz = 0
        for lo in range(0, n, cap):                             # pass 1: the offsets, slab by slab, each from the entries in front
            nnz += wk.sample_points_raw(lo, min(cap, n - lo), starts, seed, tr, colptr=colptr.data_ptr() + 8 * lo, nnz0=nnz)
        rowval = torch.empty((nnz,), dtype=torch.int64, device=dev)
        nzval = torch.empty((nnz,), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        if nnz:
            for lo in range(0, n, cap):                         # pass 2: the same draws, run-length encoded
                wk.sample_points_raw(lo, min(cap, n - lo), starts, seed, tr, colptr=colptr.data_ptr() + 8 * lo, rowval=rowval.data_ptr(),
                                     nzval=nzval.data_ptr(), nnz_extent=nnz)
        labels = torch.repeat_interleave(torch.arange(1, self.K + 1, dtype=torch.int64, device=dev), torch.as_tensor(n_k, device=dev), output_size=n)
        return torch.sparse_csc_tensor(colptr, rowval, nzval, size=(D, n)), labels

    # ---- the features a count point is expected to get next (include/dpmm_hip_recommend.h)
    def recommend(self, data, m, exclude_seen=True):
        """`Recommendation(features, prob, labels, skipped)`: for every point of count `data` the m features the fitted Multinomial mixture
        expects next, among those the point does not hold yet (exclude_seen=True) or among all D (False), 1 <= m <= min(D, 16).

        Under cluster k one more count falls on feature d with probability theta_kd = alpha'_kd / sum_d alpha'_kd -- the `theta` of
        `sampler_tables`, formed in Float64 -- and under the mixture with r_id = sum_k p_ik theta_kd, p_ik what `predict` returns.  A feature
        is SEEN by a point when its value there is not 0 (a stored entry that is not 0 for sparse data).  features holds the m candidates
        of largest r, largest first, ties to the lower index, 0-based as `explain` returns them; a point with fewer than m candidates has
        -1 / NaN behind them; a point with a NaN or no finite entry in its row of the table is -1 / NaN throughout and counted in
        `skipped`.  labels are those of `predict_labels`, from the same pass.  `data` is whatever `predict` takes for a Multinomial model
        and is read from the store the worker keeps it in -- Float32, bytes, sparse columns up to D = 65536 -- nothing is densified, and
        nothing of size n D or n K exists anywhere.  prob lies within (K + 2) 2^-24 of the Float64 value, relatively; the bits do not
        depend on `capacity`.  After `absorb_counts` and `grow_counts` the answer is that of the updated model."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        if self.kind != _priors.PRIOR_MULT:
            raise ValueError("recommend is for the Multinomial prior: an NIW model has regressor, which predicts features from given ones")
        m = int(m)
        top = min(self.D, binding.RECOMMEND_MAX_TOP)
        if not 1 <= m <= top:
            raise ValueError(f"m must be in 1..{top}")
        wk = _need(self._wk, "this Predictor's worker cannot recommend (no dpmm_recommend_points)", "recommend_points_into")
        opened = self._open(data)
        if not self._recommend_set:
            a = np.asarray(self.post["alpha"], np.float64)
            wk.set_recommend(a / a.sum(1, keepdims=True))
            self._recommend_set = True
        exclude_seen = bool(exclude_seen)
        # (the padding of a short slab is empty points: they have candidates unless they take no part)
        out, (sk, _) = self._walk(opened, [("features", (m,), "int32"), ("prob", (m,), "float32"), ("labels", (), "int64")],
                                  lambda views, lo, hi: wk.recommend_points_into(views, m, exclude_seen), absent=_first_negative("features"))
        return Recommendation(out["features"], out["prob"], out["labels"], sk)

    # ---- the features that put a count point out (include/dpmm_hip_count_explain.h)
    def count_explain_tables(self):
        """(log theta, log1p(-theta), order): the (K, D) tables `explain_counts` hands to the worker.  theta = alpha' / sum(alpha') in Float64
        (the `theta` of `sampler_tables`); order (K, D) int32: every cluster's features with log1p(-theta) non-decreasing -- theta
        non-increasing -- equal values in increasing index order.  Sorting by the logarithm the kernel reads, not by theta, makes the
        promise the sparse walk ends on hold whatever log1p rounds to."""
        a = np.asarray(self.post["alpha"], np.float64)
        theta = a / a.sum(1, keepdims=True)
        with np.errstate(divide="ignore"):
            lth, l1m = np.log(theta), np.log1p(-theta)
        return lth, l1m, np.argsort(l1m, axis=1, kind="stable").astype(np.int32)

    def explain_counts(self, data, top, side="both"):
        """WHICH features put a count point out of the cluster it is given: a `CountExplanation` tuple, computed on the GPU.

        `score_samples`, `count_statistics(min_logdens_per_count=...)` and `held_out_counts` say THAT a document, basket or play-list is
        unusual.  Under the plug-in predictive `predict` scores and `sample` draws from, Multinomial(t, theta_k) with k the point's label,
        t its total and theta_k = alpha'_k / sum(alpha'_k), the count x of feature d is Binomial(t, theta_kd).  Per point the `top`
        features, 1 <= top <= min(D, 16), of largest |residual|:

          residual      sign(x - t theta) sqrt(g), g = 2 [x log(x / (t theta)) + (t - x) log((t - x) / (t (1 - theta)))] the binomial deviance,
                        Float64, rounded to Float32 once.  The deviance, not a Pearson z-score, ranks: exp(-g / 2) is the Chernoff bound of
                        the tail, while a z-score puts every rare feature that occurs once above a common one at four times its expectation;
          count, expected    x and t theta;
          feature_tail  the exact one-sided binomial tail on the side of the deviation, P(X >= x) over, P(X <= x) under, 1 at x = t theta
                        (agreement to 2^-40): a regularised incomplete beta function in Float64, rounded once.  For values that are no
                        integers the continuous extension, no probability statement;
          features      0-based, largest |residual| as returned first, ties to the lower index; -1 / NaN behind the candidates.
        side: "both" ranks all D features, "over" those with x > t theta, "under" those with x < t theta.  A point with a NaN or no finite
        entry in its row of the table is `skipped` (total NaN); one with a value that is not finite or negative, or with t = 0, is
        `incomplete`; both are -1 / NaN throughout.  `data` is whatever `predict` takes for a Multinomial model and is read from the store
        the worker keeps it in -- Float32, bytes, sparse columns up to D = 65536 (work proportional to the point's entries) -- nothing is
        densified and nothing of size n D or n K exists.  include/dpmm_hip_count_explain.h states the error bounds; the bits do not depend
        on `capacity`.  After `absorb_counts` and `grow_counts` the answer is that of the updated model."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        if self.kind != _priors.PRIOR_MULT:
            raise ValueError("explain_counts is for the Multinomial prior: an NIW model has explain")
        if self.projection is not None:
            raise ValueError("explain_counts is refused for a model with a projection: its features are mixtures of the source features")
        m = int(top)
        cap = min(self.D, binding.COUNT_EXPLAIN_MAX_TOP)
        if m != top or not 1 <= m <= cap:
            raise ValueError(f"top must be an integer in 1..{cap}")
        if side not in binding.COUNT_EXPLAIN_SIDES:
            raise ValueError('side must be "both", "over" or "under"')
        wk = _need(self._wk, "this Predictor's worker cannot explain count points (no dpmm_count_explain_points)", "count_explain_points_into")
        opened = self._open(data)
        if not self._count_explain_set:
            wk.set_count_explain(*self.count_explain_tables())
            self._count_explain_set = True
        cap_n = self.capacity

        def evaluate(views, lo, hi):
            sk, inc = wk.count_explain_points_into(views, m, side)
            if hi - lo < cap_n:      # the padding of a short slab is empty points: incomplete (t = 0) unless their row is skipped (total NaN)
                tot = views["total"][hi - lo:]
                inc -= int((tot == tot).sum())
            return sk, inc
        spec = [("features", (m,), "int32")] + [(name, (m,), "float32") for name in ("count", "expected", "residual", "feature_tail")] + \
               [("labels", (), "int64"), ("total", (), "float64")]
        out, (sk, inc) = self._walk(opened, spec, evaluate, absent=_first_nan("total"))
        return CountExplanation(out["features"], out["count"], out["expected"], out["residual"], out["feature_tail"], out["labels"], out["total"], sk, inc)

    # ---- slabs
    def _spec(self, labels, logdens, m, probs):
        spec = []
        if labels:
            spec.append(("labels", (), "int64"))
        if logdens:
            spec.append(("logdens", (), "float32"))
        if m:
            spec += [("top_idx", (m,), "int64"), ("top_prob", (m,), "float32")]
        if probs:
            spec.append(("probs", (self.K,), "float32"))
        return spec

    def _open(self, data, refuse_projected=None):
        """What every walk over `data` in slabs of `capacity` points needs: (n, dev, new, upload).  dev: the torch device of device data,
        else None; new(rows, tail, dtype name): an empty result array / tensor where the results go; upload(lo, hi): the worker's points
        become the points lo..hi-1, zero padded (empty columns for sparse data) to `capacity`."""
        if self._wk is None:
            raise RuntimeError("this Predictor is closed")
        wk, cap = self._wk, self.capacity
        pts = _points.describe(data)
        if pts.torch_device is not None and pts.device_index(self._device_arg) != self.device:
            raise ValueError(f"the data tensor lives on {pts.torch_device}, this Predictor on device {self.device}: open one Predictor per GPU")
        if pts.is_sparse and self.kind != _priors.PRIOR_MULT:
            raise TypeError("sparse data is for the Multinomial prior")
        D, n = pts.D, pts.N
        proj = self.projection if self.projection is not None and not pts.is_sparse and D == self.projection.D_in else None
        if proj is None and D != self.D:               # (d-row data is taken as already projected)
            raise ValueError("data dimension does not match the model")
        if proj is not None and (refuse_projected or self.missing == "marginalize"):
            # one NaN source feature poisons all d projected coordinates: nothing is left to marginalise over
            what = refuse_projected or 'missing="marginalize"'
            raise ValueError(f"{what} takes data in the model's {self.D} projected coordinates, not the {D} source features of the projection")
        projected = proj is not None
        pts = pts.served(wk, projected)                # (a stand-in worker without the device entry points: host data)
        dev = pts.torch_device
        if dev is not None:
            import torch
            new = lambda rows, tail, dt: torch.empty((rows,) + tail, dtype=getattr(torch, dt), device=dev)      # noqa: E731
            pts.synchronize()
        else:
            new = lambda rows, tail, dt: np.empty((rows,) + tail, dt)      # noqa: E731
        stages = _Stages(self, "_in" if projected else "")

        def upload(lo, hi):                            # a full slab where it is; the short one through the staging the Predictor keeps
            if hi - lo == cap:
                pts.upload(wk, lo, hi, projected)
            else:
                pts.padded(lo, hi, cap, stages).upload(wk, 0, cap, projected)
        return n, dev, new, upload

    def _walk(self, opened, spec, evaluate, counts=False, absent=None):
        """The one walk over opened data in slabs of `capacity` points: every slab is uploaded and `evaluate(views, lo, hi)` called with its
        outputs as `spec` lists them -- slices of the result for a full slab, the staging outputs the Predictor keeps for the short one, whose
        first hi - lo rows are then copied.  Sets `missing_counts` (the worker is asked under "marginalize", or if `counts`).
        absent: the call counts -- `evaluate` returns what the worker reported, skipped or (skipped, incomplete) -- and the walk owns the
        sums: the worker scored the zero padding of a short slab too, which is not ours, so absent(views, rows), how many of `rows` took no
        part, is counted over the padded rows and taken off `skipped`.  Returns (results, (skipped, incomplete)); without `absent` nothing is
        counted and the pair is (0, 0)."""
        n, dev, new, upload = opened
        wk, cap = self._wk, self.capacity
        out = {name: new(n, tail, dt) for name, tail, dt in spec}
        total = np.zeros(2, np.int64)
        took = [0, 0]
        for lo in range(0, n, cap):
            hi = min(n, lo + cap)
            full = hi - lo == cap
            upload(lo, hi)
            if full:
                views = {name: out[name][lo:hi] for name, _, _ in spec}
            else:
                key = "dev" if dev is not None else "host"
                views = {}
                for name, tail, dt in spec:
                    b = self._out_stage.get((key, name))
                    if b is None or tuple(b.shape[1:]) != tail or (dev is not None and b.device != dev):
                        b = self._out_stage[(key, name)] = new(cap, tail, dt)
                    views[name] = b
            got = evaluate(views, lo, hi)
            if absent is not None:
                for i, c in enumerate(got if isinstance(got, tuple) else (got,)):
                    took[i] += c
                if not full:
                    took[0] -= absent(views, slice(hi - lo, cap))
            if counts or self.missing == "marginalize":
                total += np.asarray(wk.score_missing_counts(), np.int64)
            if not full:
                for name, _, _ in spec:
                    out[name][lo:hi] = views[name][:hi - lo]
        self.missing_counts = (int(total[0]), int(total[1]))
        return out, tuple(took)

    def _run(self, data, labels=False, logdens=False, m=0, probs=False):
        wk = self._wk
        return self._walk(self._open(data), self._spec(labels, logdens, m, probs), lambda views, lo, hi: wk.score_points_into(views, m=m))[0]


class Regressor:
    """Regressor(predictor, given, targets=None): Gaussian-mixture regression from the features `given` to `targets` of a fitted NIW model
    (include/dpmm_hip_regress.h).  `given` and `targets` are lists of distinct 0-based feature indices, disjoint; `targets` defaults to
    every feature not in `given`; features in neither are marginalised away.  Use as a context manager or close().

    `marginal` is `predictor.marginal(given)`, made with missing="propagate" whatever the parent's setting, owned and closed by the
    Regressor.  The per-cluster tables B, c, V, h (host/condition.py) are formed in Float64 from the predictive parameters the marginal
    worker is handed -- m, R, logdet, df, w as the Float32 values it receives -- over given + targets, and refreshed whenever the marginal
    model's parameters change (`marginal.absorb`): the probabilities, h and df then follow the marginal model, while the conditional mean
    function c + B x and V stay those of the joint model the Regressor was made from -- data of the given features alone says nothing
    about the law of the targets given them."""

    def __init__(self, predictor, given, targets=None, capacity=None, worker_factory=None):
        predictor._refuse_conditioning("regressor")
        D = predictor.D
        self.given = _condition.check_features(given, D, "given")
        if targets is None:
            targets = [f for f in range(D) if f not in set(self.given)]
        self.targets = _condition.check_features(targets, D, "targets")
        if set(self.given) & set(self.targets):
            raise ValueError("given and targets must be disjoint")
        if len(self.targets) > binding.REGRESS_MAX_TARGETS:
            raise ValueError(f"at most {binding.REGRESS_MAX_TARGETS} targets")
        # the joint model over given + targets (the closure rule with D_o + D_t features: a permutation when nothing is left out)
        self._sub_post = _condition.niw_marginal(predictor.post, self.given + self.targets)
        self.D_o, self.D_t = len(self.given), len(self.targets)
        self.marginal = predictor.marginal(self.given, capacity=capacity, worker_factory=worker_factory, missing="propagate")
        self._tables_for = None
        try:
            self._refresh()
        except Exception:
            self.marginal.close()
            raise

    def _joint_parameters(self):
        """(m (K, D_o + D_t), R (K, (D_o + D_t)^2) upper triangular, Sigma^-1 = R'R) of the joint predictive over given + targets, in that
        order: the Float32 values a worker would be handed, widened to Float64 -- what the tables are formed from."""
        mg = self.marginal
        sub = Predictor.__new__(Predictor)      # only the conversion of host/priors.py is used: no worker
        sub.kind, sub.D, sub.K, sub.post, sub.weights = mg.kind, self.D_o + self.D_t, mg.K, self._sub_post, mg.weights
        m, R = sub._predictive_args()[1][:2]
        return np.asarray(m, np.float32).astype(np.float64), np.asarray(R, np.float32).astype(np.float64)

    def tables(self, factor=False):
        """(B (K, D_t, D_o), c (K, D_t), V (K, D_t), h (K,), df (K,)) in Float64 for the model as it stands; factor=True: W (K, D_t, D_t),
        upper triangular with W W' = (A_MM)^-1, as a sixth entry."""
        mg = self.marginal
        f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731  (what the worker receives)
        m, R = self._joint_parameters()
        B, c, V, *W = _condition.regression_tables(m, R, range(self.D_o), range(self.D_o, self.D_o + self.D_t), factor=factor)
        _, _, logdet, df, w = (f32(a) for a in mg._predictive_args()[1])
        return (B, c, V, _condition.table_constant(logdet, df, w, self.D_o), df) + tuple(W)

    def _refresh(self):
        """The worker's tables are those of the marginal model's posterior as it stands (absorb replaces `post` and reloads the worker)."""
        mg = self.marginal
        if mg._wk is None:
            raise RuntimeError("this Regressor is closed")
        if self._tables_for is mg.post:
            return
        _need(mg._wk, "this Regressor's worker cannot regress (no dpmm_set_regression)", "set_regression")
        draws = hasattr(mg._wk, "set_regression_factor")      # (a worker without it predicts; `sample` says what is missing)
        B, c, V, h, df, *W = self.tables(factor=draws)
        self._no_var = bool(np.any(df + self.D_o <= 2))
        mg._wk.set_regression(B, c, V, h)
        if draws:
            mg._wk.set_regression_factor(W[0])
        self._tables_for = mg.post
        self._levels_for = None      # (dpmm_set_regression invalidates the levels of `quantile`)

    def close(self):
        self.marginal.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def predict(self, data, return_std=False):
        """`Regression(mean, std, labels, skipped)` for `data` of D_o rows in the order of `given` (a caller holding the full table passes
        X[given]); every input kind the marginal Predictor takes.  mean[d, i] = sum_k p_ik (c_k + B_k x_i)_d with the probabilities
        `marginal.predict` returns; std (return_std=True) the root of the mixture's predictive variance per target; labels the marginal
        model's.  A point with a NaN or no finite entry in its row of the table, or a feature that is not finite, takes no part: NaN
        columns, counted in `skipped`."""
        mg = self.marginal
        self._refresh()
        if return_std and self._no_var:
            raise ValueError("return_std needs df + D_o > 2 for every cluster: a conditional law has no variance")
        wk = mg._wk
        spec = [("mean", (self.D_t,), "float32")] + ([("std", (self.D_t,), "float32")] if return_std else []) + [("labels", (), "int64")]
        # (the padding of a short slab is zeros: points that take part, but if they did not, not ours)
        out, (sk, _) = mg._walk(mg._open(data), spec, lambda views, lo, hi: wk.regress_points_into(views["mean"], views.get("std"), views["labels"]),
                                absent=_first_nan("mean"))
        return Regression(out["mean"].T, out["std"].T if return_std else None, out["labels"], sk)

    def sample(self, data, draws=1, seed=0, return_components=False):
        """`RegressionDraws(values, components, labels, skipped)`: `draws` DRAWS of the targets of every point of `data` (D_o rows in the
        order of `given`, every input kind `predict` takes) from their law given the given features under the fitted mixture
        (include/dpmm_hip_regress_draw.h): a cluster k ~ p_ik, then that cluster's conditional Student-t.  Where `predict` gives one
        number per target -- a mean that can lie between the modes, where no data is -- the draws keep the modes and how the targets move
        together: joint intervals, quantiles, P(target a > target b), completions of a table.  values (draws, D_t, n) float32, the
        orientation of `impute(draws=m)`.  Draw j of point i depends on (seed, i = its position in `data`, j, the point, the model) alone
        -- not on `capacity`, not on `draws`: the first draws of a longer run are those of a shorter one.  A point that takes no part
        (see `predict`) has NaN in every draw and component -1, and is counted once in `skipped`.  The draws of a slab come from one
        evaluation of the table; the labels cost a second one."""
        mg = self.marginal
        self._refresh()
        m, seed = int(draws), int(seed)
        if m < 1 or m != draws or m > binding.REGRESS_MAX_DRAWS:
            raise ValueError(f"draws must be an integer in 1..{binding.REGRESS_MAX_DRAWS}")
        if seed < 0 or seed >> 64:
            raise ValueError("seed must be in 0..2^64 - 1")
        wk = _need(mg._wk, "this Regressor's worker cannot draw the targets (no dpmm_regress_draw_points)", "regress_draw_points_into", "set_regression_factor")
        opened = mg._open(data)
        cs = _CompStage(opened, m, mg.capacity, return_components, always=True)      # (a component of -1 is the mark of a point that took no part)

        def evaluate(views, lo, hi):
            sk = wk.regress_draw_points_into(views["draws"], seed, lo, comp=cs.stage)      # the global index of a point is its position in `data`
            wk.score_points_into({"labels": views["labels"]})
            cs.slice_in(lo, hi)
            return sk
        out, (sk, _) = mg._walk(opened, [("draws", (m, self.D_t), "float32"), ("labels", (), "int64")], evaluate, absent=cs.absent)      # (n, m, D_t): ld = m D_t, draw_stride = D_t
        vals = out["draws"]
        vals = vals.permute(1, 2, 0) if hasattr(vals, "permute") else vals.transpose(1, 2, 0)
        return RegressionDraws(vals, cs.comp, out["labels"], sk)


    # ---- calibrated probabilities (include/dpmm_hip_regress_cdf.h)
    def _cdf_worker(self, what):
        self._refresh()
        return _need(self.marginal._wk, f"this Regressor's worker cannot give {what} (no dpmm_regress_cdf_points)", "regress_cdf_points_into",
                     "set_regression_levels", "regress_quantile_points_into")

    def cdf(self, data, y):
        """`ConditionalCDF(cdf, sf, labels, skipped)`: for every point of `data` (D_o rows in the order of `given`, every input kind
        `predict` takes) and every target d, the probability under the fitted mixture that the target lies at or below the observed
        y[d, i], and above it: F = sum_k p_ik T_{df_k + D_o}((y - mu_ikd) / sigma_ikd), the mixture of the clusters' conditional Student-t
        laws -- exact where `std` describes a bimodal law badly, and needing no draws.  y: a (D_t, n) numpy array or torch tensor of any
        real dtype in the order of `targets` (on the data's device if `data` is a device tensor; host data takes an array or a CPU tensor), converted to float32 slab by slab.
        cdf and sf are each summed in Float64 from the side of every component that does not cancel, so a value 40 standard deviations
        out has sf = 1e-30, not 0 (Float32: below 2^-150 a value is returned as 0).  A NaN in y gives NaN in that entry only, -Inf / +Inf give exactly 0 / 1; a point that takes no
        part (see `predict`) has NaN columns and is counted in `skipped`.  Needs no df + D_o > 2."""
        mg = self.marginal
        wk, cap = self._cdf_worker("the conditional CDF"), mg.capacity
        opened = mg._open(data)
        n, dev, new = opened[0], opened[1], opened[2]
        y_dev = getattr(y, "device", None) if hasattr(y, "data_ptr") else None
        if y_dev is not None and dev is None and y_dev.type == "cpu":      # host data: a CPU tensor is as good as an array
            import torch
            y, y_dev = (y if y.dtype in (torch.float32, torch.float64) else y.to(torch.float32)).numpy(), None
        if y_dev is None:
            y = np.asarray(y)
            if y.dtype.kind not in "fiub":
                raise TypeError("y must hold real numbers")
        if tuple(y.shape) != (self.D_t, n):
            raise ValueError(f"y must be (D_t, n) = ({self.D_t}, {n}), in the order of `targets`")
        if (dev is None) != (y_dev is None) or (dev is not None and y_dev != dev):
            raise ValueError("y must live where the data lives: host memory (a numpy array or a CPU tensor) for host data, the data's device for a device tensor")
        ys = new(cap, (self.D_t,), "float32") if n else None      # y of one slab, point-major as the worker reads it, zeros behind the slab's points

        def evaluate(views, lo, hi):
            m = hi - lo
            if dev is not None:
                import torch
                ys[:m] = y[:, lo:hi].T.to(torch.float32)
            else:
                ys[:m] = y[:, lo:hi].T
            ys[m:] = 0
            return wk.regress_cdf_points_into(ys, views["cdf"], views["sf"], views["labels"])
        out, (sk, _) = mg._walk(opened, [("cdf", (self.D_t,), "float32"), ("sf", (self.D_t,), "float32"), ("labels", (), "int64")], evaluate,
                                absent=_first_nan("cdf"))
        return ConditionalCDF(out["cdf"].T, out["sf"].T, out["labels"], sk)

    def quantile(self, data, levels=(0.05, 0.5, 0.95)):
        """`RegressionQuantiles(values, levels, labels, skipped)`: values[q, d, i] is the y at which the conditional CDF of target d of
        point i (see `cdf`) reaches levels[q] -- medians and prediction intervals without draws.  levels: 1 to 16 numbers strictly
        inside (0, 1), in any order.  A point that could belong to one cluster only gets that cluster's Student-t quantile (level 0.5:
        the bits of `predict`'s mean); otherwise a safeguarded Newton solve on the mixture CDF runs on the GPU, to the Float32 value at
        which the CDF crosses the level.  Values are non-decreasing in the level, and a value depends on (the point, the model, the
        level) alone.  Skipped points as in `cdf`."""
        mg = self.marginal
        wk = self._cdf_worker("conditional quantiles")
        lv = np.atleast_1d(np.asarray(levels, np.float64))
        if lv.ndim != 1 or not 1 <= len(lv) <= binding.REGRESS_MAX_LEVELS:
            raise ValueError(f"levels: 1 to {binding.REGRESS_MAX_LEVELS} numbers")
        if not np.all((lv > 0) & (lv < 1)):
            raise ValueError("levels must lie strictly inside (0, 1)")
        inc, back = np.unique(lv, return_inverse=True)      # the worker solves them in increasing order
        key = (tuple(inc), self._tables_for)
        if getattr(self, "_levels_for", None) is None or self._levels_for[0] != key[0] or self._levels_for[1] is not key[1]:
            df = np.asarray(mg._predictive_args()[1][3], np.float32).astype(np.float64)      # (what the worker holds, as `tables` widens it)
            wk.set_regression_levels(inc, _condition.student_t_ppf(inc, df + self.D_o))
            self._levels_for = key
        L = len(inc)
        out, (sk, _) = mg._walk(mg._open(data), [("values", (L, self.D_t), "float32"), ("labels", (), "int64")],
                                lambda views, lo, hi: wk.regress_quantile_points_into(views["values"], views["labels"]), absent=_first_nan("values"))
        vals = out["values"]
        vals = vals.permute(1, 2, 0) if hasattr(vals, "permute") else vals.transpose(1, 2, 0)
        vals = vals[back.tolist()] if hasattr(vals, "permute") else vals[back]
        return RegressionQuantiles(vals, tuple(float(v) for v in lv), out["labels"], sk)

    def interval(self, data, level=0.9):
        """(lower, upper), each (D_t, n): the central prediction interval of every target at coverage `level`, 0 < level < 1 -- `quantile`
        at (1 - level) / 2 and (1 + level) / 2."""
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie strictly inside (0, 1)")
        q = self.quantile(data, ((1.0 - float(level)) / 2.0, (1.0 + float(level)) / 2.0))
        return q.values[0], q.values[1]


def regress(dp_model, data, given, targets=None, return_std=False, **kw):
    """Mixture regression from the features `given` to `targets` (opens a Predictor and its Regressor, runs, closes): see `Regressor`;
    `data` has the rows of `given`; kw: capacity, device, worker_factory."""
    factory = kw.pop("worker_factory", None)
    with Predictor(dp_model, worker_factory=factory, **kw) as p:
        with p.regressor(given, targets, worker_factory=factory) as r:
            return r.predict(data, return_std=return_std)


def regress_sample(dp_model, data, given, targets=None, draws=1, seed=0, **kw):
    """Draws of the features `targets` given the features `given` (opens a Predictor and its Regressor, draws, closes): see
    `Regressor.sample`; `data` has the rows of `given`; kw: return_components, capacity, device, worker_factory."""
    factory = kw.pop("worker_factory", None)
    comps = kw.pop("return_components", False)
    with Predictor(dp_model, worker_factory=factory, **kw) as p:
        with p.regressor(given, targets, worker_factory=factory) as r:
            return r.sample(data, draws=draws, seed=seed, return_components=comps)


def regress_cdf(dp_model, data, y, given, targets=None, **kw):
    """Conditional CDF of the observed `targets` y given the features `given` (opens a Predictor and its Regressor, runs, closes): see
    `Regressor.cdf`; `data` has the rows of `given`, y those of `targets`; kw: capacity, device, worker_factory."""
    factory = kw.pop("worker_factory", None)
    with Predictor(dp_model, worker_factory=factory, **kw) as p:
        with p.regressor(given, targets, worker_factory=factory) as r:
            return r.cdf(data, y)


def regress_quantile(dp_model, data, given, targets=None, levels=(0.05, 0.5, 0.95), **kw):
    """Conditional quantiles of the features `targets` given the features `given` (opens a Predictor and its Regressor, runs, closes):
    see `Regressor.quantile`; kw: capacity, device, worker_factory."""
    factory = kw.pop("worker_factory", None)
    with Predictor(dp_model, worker_factory=factory, **kw) as p:
        with p.regressor(given, targets, worker_factory=factory) as r:
            return r.quantile(data, levels)


def recommend(dp_model, data, m, exclude_seen=True, **kw):
    """`Predictor.recommend` in one call: the m features every count point of `data` is expected to get next under the fitted Multinomial
    model (keywords: those of Predictor)."""
    with Predictor(dp_model, **kw) as p:
        return p.recommend(data, m, exclude_seen=exclude_seen)


def explain_counts(dp_model, data, top, side="both", **kw):
    """`Predictor.explain_counts` in one call: the `top` features that put every count point of `data` out of its cluster under the fitted
    Multinomial model (keywords: those of Predictor)."""
    with Predictor(dp_model, **kw) as p:
        return p.explain_counts(data, top, side=side)


def score_samples(dp_model, data, **kw):
    """Log-density of every point under the fitted mixture (opens a Predictor, runs, closes); kw: capacity, device, worker_factory."""
    with Predictor(dp_model, **kw) as p:
        return p.score_samples(data)


def predict_topk(dp_model, data, m, **kw):
    """(labels, idx (n, m), probs (n, m)) of the m most probable clusters (opens a Predictor, runs, closes)."""
    with Predictor(dp_model, **kw) as p:
        return p.predict_topk(data, m)


def exemplars(dp_model, data, m, **kw):
    """The m most and least typical points of every cluster (opens a Predictor, runs, closes): see `Predictor.exemplars`;
    kw: which, capacity, device, worker_factory."""
    which = kw.pop("which", "both")
    with Predictor(dp_model, **kw) as p:
        return p.exemplars(data, m, which=which)


def typicality(dp_model, data, **kw):
    """Labels, squared Mahalanobis distances and their calibrated tails (opens a Predictor, runs, closes): see `Predictor.typicality`;
    kw: gaps, capacity, device, worker_factory, missing."""
    gaps = kw.pop("gaps", "incomplete")
    with Predictor(dp_model, **kw) as p:
        return p.typicality(data, gaps=gaps)


def explain(dp_model, data, top=None, **kw):
    """Per-feature conditional residuals, z-scores and tails of every point under its own cluster (opens a Predictor, runs, closes): see
    `Predictor.explain`; kw: gaps, capacity, device, worker_factory, missing."""
    gaps = kw.pop("gaps", "incomplete")
    with Predictor(dp_model, **kw) as p:
        return p.explain(data, top=top, gaps=gaps)


def explain_groups(dp_model, data, groups, **kw):
    """`Predictor.explain_groups` in one call: which group of features makes every point of `data` atypical of its cluster, a
    `GroupExplanation` tuple; kw: capacity, device, worker_factory, missing."""
    with Predictor(dp_model, **kw) as p:
        return p.explain_groups(data, groups)


def held_out(dp_model, data, **kw):
    """The points of `data` below the model's floors, collected on the GPU (opens a Predictor, runs, closes): see `Predictor.held_out`;
    kw: min_logdens, min_tail, max_points, capacity, device, worker_factory, missing."""
    args = {k: kw.pop(k) for k in ("min_logdens", "min_tail", "max_points") if k in kw}
    with Predictor(dp_model, **kw) as p:
        return p.held_out(data, **args)


def held_out_counts(dp_model, data, **kw):
    """The points of count `data` below a Multinomial model's floors, collected on the GPU (opens a Predictor, runs, closes): see
    `Predictor.held_out_counts`; kw: min_logdens, min_logdens_per_count, max_points, max_entries, capacity, device, worker_factory."""
    args = {k: kw.pop(k) for k in ("min_logdens", "min_logdens_per_count", "max_points", "max_entries") if k in kw}
    with Predictor(dp_model, **kw) as p:
        return p.held_out_counts(data, **args)


def overlap(dp_model, data, **kw):
    """The overlap matrix of the clusters on `data` (opens a Predictor, runs, closes): see `Predictor.overlap`;
    kw: capacity, device, worker_factory, missing."""
    with Predictor(dp_model, **kw) as p:
        return p.overlap(data)


def statistics(dp_model, data, **kw):
    """The per-cluster sufficient statistics of `data` under the model (opens a Predictor, runs, closes): see `Predictor.statistics`;
    kw: assign, min_logdens, min_tail, capacity, device, worker_factory, missing."""
    assign, min_logdens, min_tail = kw.pop("assign", "hard"), kw.pop("min_logdens", None), kw.pop("min_tail", None)
    with Predictor(dp_model, **kw) as p:
        return p.statistics(data, assign=assign, min_logdens=min_logdens, min_tail=min_tail)


def count_statistics(dp_model, data, **kw):
    """The per-cluster count statistics of `data` under a Multinomial model (opens a Predictor, runs, closes): see
    `Predictor.count_statistics`; kw: assign, min_logdens, min_logdens_per_count, capacity, device, worker_factory."""
    assign, min_logdens, per_count = kw.pop("assign", "hard"), kw.pop("min_logdens", None), kw.pop("min_logdens_per_count", None)
    with Predictor(dp_model, **kw) as p:
        return p.count_statistics(data, assign=assign, min_logdens=min_logdens, min_logdens_per_count=per_count)


def impute(dp_model, data, draws=None, seed=0, return_components=False, **kw):
    """`data` with its missing (NaN) features filled in -- or, with draws=m, m copies with the gaps drawn -- (opens a Predictor, runs,
    closes): see `Predictor.impute`; kw: capacity, device, worker_factory, missing."""
    with Predictor(dp_model, **kw) as p:
        return p.impute(data, draws=draws, seed=seed, return_components=return_components)


def sample(dp_model, n, seed=0, trials=None, sparse=False, **kw):
    """(data, labels): n new points from the fitted mixture (opens a Predictor, draws, closes); kw: capacity, device, worker_factory."""
    with Predictor(dp_model, **kw) as p:
        return p.sample(n, seed=seed, trials=trials, sparse=sparse)
