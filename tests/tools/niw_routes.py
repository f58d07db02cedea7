"""Host-side companion of tests/test_gpu_niw_routes.py: the LDS arithmetic of launch_direct (csrc/niw_sweep.hip) restated, problems whose
screened sweep has a KNOWN evaluated set, and the Float64 quantities from which that set is predicted.  No GPU is needed for any of it
(tests/test_niw_routes_cpu.py).

Geometry of paired_problem.  S = ceil(K / 2) sites on a line along the LAST feature, SPACING standard deviations apart; clusters k and
k + S share site k (K odd: cluster S - 1 is alone at its site) with means `gap` standard deviations apart.  The last feature is
independent of the others in every covariance, so the upper-triangular factor R (inv Sigma = R'R) carries the site term in its last row
alone, with the same entry (variance 1) in every cluster: every screen of the sweep that looks at the last rows of R z (4-row tail
test, 16-row matrix screen) sees ALL of the distance between two sites, and a site one step further away costs at least
SPACING^2 / 2 = 512 nats more whatever the clusters' other features do.  The other variances are 0.9 .. 1.1 plus a
small random part: a cluster of another site gains at most ~0.2 D nats from its determinant and shape and loses 512 from the distance
-- below 2^-149 of the row maximum (103.3 nats) with room for the screens' margin of 50 (DPMM_OPT_SCREEN_MARGIN's default), for every
D <= 256.  separation() measures it.

What a tile evaluates (tile_sets).  The reference clusters are the previous labels of the tile's first and last point (and, D <= 64, of
up to two more points); every other cluster is dropped when an UPPER bound of its value is below (best reference value - margin) for
every point of the tile.  The bounds differ by kernel and stage, but all are sound and the last one every candidate meets is the 16-row
screen, cst_k - |rows 16 screen_block(D) .. of R_k (x - mu_k)|^2 / 2.  So, in Float64: a cluster whose VALUE is within the margin of a
point's row maximum is evaluated for sure; a cluster whose 16-row bound is below the threshold for every point is dropped for sure.
Where the two sets coincide the tile's evaluated set -- `nev` of the compact table -- is known without running the kernel."""
import numpy as np

MARGIN = 50.0                    # DPMM_OPT_SCREEN_MARGIN's default (nats)
SPACING = 32.0                   # distance between neighbouring sites, in standard deviations of the last feature
LOG_DENORMAL = 149 * np.log(2.0)   # a weight below 2^-149 of the row maximum is an exact zero of the Float32 draw

CU_LDS, ROW_BYTES, SCREEN_BYTES = 160 * 1024, 1024, 1088      # per CU | one table row of a workgroup (4 waves x 64 points) | screen operands of a cluster
OCCUPANCY = {1: 4, 2: 3, 4: 2}


def nb_of(D):
    for nb, top in ((1, 16), (2, 32), (4, 64), (8, 128), (16, 256)):
        if D <= top:
            return nb
    raise ValueError(D)


def tile_points(NB):
    """Points per wave tile (D <= 64) or per workgroup tile of four 32-point waves (D >= 65)."""
    return 64 if NB <= 4 else 128


def screen_block(D):
    """The block of 16 features whose rows of R z the 16-row screen sums, and from which the tail screens take a point's last features:
    the one that holds features D-4 .. D-1.  The kernels pick it at run time: NB is 4 for every D in 33 .. 64, 8 up to 128 and 16
    beyond, so block NB - 1 is padding for D <= 48, D <= 112 and D in 129 .. 240."""
    return (D - 1) // 16


def max_sites_per_window(P, order, prev0, width=64):
    """The largest number of sites that `width` consecutive positions of the visiting order touch (by previous label)."""
    st = P["site"][prev0[order]]
    return max(len(np.unique(st[lo:lo + width])) for lo in range(0, max(1, len(st) - width + 1)))


def budgets(NB):
    """launch_direct's LDS budget for niw_sweep_direct_kernel<NB, 4, OCC>: table rows, compact slots, and the largest K whose screen operands
    are staged in LDS beside the table (None: no such K -- NB = 1 has no screen)."""
    per_wg = CU_LDS // OCCUPANCY[NB]
    rows = (per_wg - 512) // ROW_BYTES
    slots = min(64, rows // 2)

    def screen_lds(K):
        lds_rows = K if K <= rows else slots
        slot_bytes = 4 * ((K + 3) & ~3) if K > rows else 0
        return NB >= 2 and lds_rows * ROW_BYTES + K * SCREEN_BYTES + slot_bytes + 1024 <= per_wg

    fits = [K for K in range(1, 1025) if screen_lds(K)]
    return dict(rows=rows, compact_slots=slots, screen_lds_max=max(fits) if fits else None)


def sites_of(K):
    S = (K + 1) // 2
    return S, np.arange(K) % S


def paired_problem(D, n, K, seed, gap=1.5, shuffled=False, empty=(), mixed=None, head=0):
    """A problem in the format of test_gpu_niw.make_problem (module docstring for the geometry).  Points come sorted by true cluster, the
    same number for every cluster that is not in `empty` (clusters left without a point: the bin-sorted order then puts their neighbours'
    blocks next to each other), after `head` leading points of cluster 0 (whole tiles of one label: what the reference bracket asks
    for); shuffled=True permutes the storage order.  mixed = a sequence of site counts: wave tile t of the STORAGE
    order holds points of mixed[t % len] neighbouring sites, sorted by site (the compact-table case whose tiles evaluate a known number
    of clusters)."""
    rng = np.random.default_rng(seed)
    S, site = sites_of(K)
    pos = SPACING * (np.arange(S) - 0.5 * (S - 1))
    mus = np.zeros((3 * K, D))
    half = np.empty((S, D))
    for s in range(S):
        u = rng.normal(size=D)
        half[s] = 0.5 * gap * u / np.linalg.norm(u)
    for k in range(K):
        mus[3 * k] = half[site[k]] * (1.0 if k < S else -1.0)
        mus[3 * k, D - 1] += pos[site[k]]
        d = rng.normal(size=D) * (0.8 / np.sqrt(D))
        mus[3 * k + 1] = mus[3 * k] + d
        mus[3 * k + 2] = mus[3 * k] - d
    A = rng.normal(size=(3 * K, D, D)) * (0.3 / np.sqrt(D))
    A[:, D - 1, :] = 0.0                                       # the last feature: independent of the others
    Sig = A @ A.transpose(0, 2, 1) + np.eye(D) * (0.9 + 0.2 * rng.random((3 * K, 1, 1)))
    Sig[:, D - 1, D - 1] = 1.0                                 # ... with the same variance in every cluster: distances between sites compare exactly
    invS = np.linalg.inv(Sig)
    invS = 0.5 * (invS + invS.transpose(0, 2, 1))
    logdet = np.linalg.slogdet(Sig)[1]
    if mixed is None:
        live = np.setdiff1d(np.arange(K), np.asarray(empty, np.int64))
        z = np.concatenate([np.zeros(head, np.int64), live[(np.arange(n - head) * len(live)) // (n - head)]])
    else:
        z = np.empty(n, np.int64)
        for t, lo in enumerate(range(0, n, 64)):
            m = mixed[t % len(mixed)]
            first = (5 * t) % (S - m + 1) if m < S else 0
            cnt = min(64, n - lo)
            st = first + (np.arange(cnt) * m) // cnt
            other = (np.arange(cnt) & 1) * S
            z[lo:lo + cnt] = np.where(st + other < K, st + other, st)
    L = np.linalg.cholesky(Sig[0::3])
    E = rng.normal(size=(n, D))
    X = np.empty((n, D), np.float32)
    for k in np.unique(z):
        X[z == k] = mus[3 * k] + E[z == k] @ L[k].T
    if shuffled:
        p = rng.permutation(n)
        X, z = np.ascontiguousarray(X[p]), z[p]
    w = rng.dirichlet(np.ones(K) * 5).astype(np.float32)
    lr = rng.dirichlet(np.ones(2) * 5, size=K).astype(np.float32)
    return dict(D=D, n=n, K=K, X=X, mu=mus.astype(np.float32), invS=invS.reshape(3 * K, -1).astype(np.float32),
                logdet=logdet.astype(np.float32), w=w, lr=lr, z=z, S=S, site=site)


def rotated_labels(P):
    """0-based labels that are deliberately wrong: every point in the cluster of the NEXT site (same half where that cluster exists)."""
    K, S = P["K"], P["S"]
    k = (P["z"] % S + 1) % S + S * (P["z"] >= S)
    return np.where(k < K, k, k - S)


def table_f64(P, which=0, screen_rows_from=None):
    """(K, n) Float64, in the convention of dpmm_debug_loglik / dpmm_debug_subloglik (no 2 pi term): -(logdet + q) / 2 + log weight of the
    Float32 parameters, for the cluster rows (which = 0) or the left / right sub-cluster rows (1 / 2; weight = lr).  With
    screen_rows_from = r: q is replaced by the sum over rows r.. of R (x - mu) -- the 16-row screen's lower bound of q (R = L',
    inv Sigma = L L' as dpmm_set_params_niw factors it), i.e. an upper bound of the value."""
    K, n, D = P["K"], P["n"], P["D"]
    X = P["X"].astype(np.float64)
    wt = P["w"] if which == 0 else P["lr"][:, which - 1]
    out = np.empty((K, n))
    for k in range(K):
        j = 3 * k + which
        Z = X - P["mu"][j].astype(np.float64)
        M = P["invS"][j].astype(np.float64).reshape(D, D)
        if screen_rows_from is None:
            q = np.einsum("ni,ni->n", Z @ M, Z)
        else:
            r = screen_rows_from
            Rt = np.linalg.cholesky(M)[r:, r:]                 # (R[r:, r:])' -- rows r.. of the upper-triangular R touch columns r.. only
            q = ((Z[:, r:] @ Rt) ** 2).sum(1)
        out[k] = -0.5 * (np.float64(P["logdet"][j]) + q) + np.log(np.float64(wt[k]))
    return out


def separation(P, T):
    """The largest value, relative to the row maximum, that any point has under a cluster of ANOTHER site than its own (nats, negative)."""
    other = P["site"][:, None] != P["site"][P["z"]][None, :]
    return float((T - T.max(0))[other].max())


def visiting_order(labels0, sub):
    """The order a statistics pass leaves: a stable sort by bin 2 (label - 1) + (sub - 1)."""
    return np.argsort(2 * np.asarray(labels0) + (np.asarray(sub) - 1), kind="stable")


def tile_sets(P, T, U, order, prev0, extra_refs):
    """Per tile of the visiting order: (references, clusters evaluated for sure, clusters that may be evaluated) -- module docstring.
    prev0: previous labels, 0-based, by point.  extra_refs: 2 for the D <= 64 kernel, 0 for the D >= 65 one."""
    tile = tile_points(nb_of(P["D"]))
    top = T.max(0)
    out = []
    for lo in range(0, P["n"], tile):
        pts = order[lo:lo + tile]
        pl = prev0[pts]
        refs = [int(pl[0])] + ([int(pl[-1])] if pl[-1] != pl[0] else [])
        added = 0
        for k in pl:                                           # further references: the first `extra_refs` other labels in visiting order
            if added == extra_refs:
                break
            if int(k) not in refs:
                refs.append(int(k))
                added += 1
        thr = T[refs][:, pts].max(0) - MARGIN
        slack = 1e-2 + 1e-4 * np.abs(thr)
        sure = set(np.flatnonzero((T[:, pts] >= top[pts] - MARGIN + slack).any(1)).tolist()) | set(refs)
        may = set(np.flatnonzero((U[:, pts] >= thr - slack).any(1)).tolist()) | set(refs)
        out.append((refs, sure, may))
    return out


def distinct_labels(order, labels0, group):
    """Number of distinct labels in every group of `group` consecutive positions of the visiting order, summed."""
    return sum(len(np.unique(labels0[order[lo:lo + group]])) for lo in range(0, len(order), group))


# --------------------------------------------------------------------------- the cases, shared by the CPU and the GPU test
# (D, K, variant).  "sorted": points and previous labels by true cluster, visited in the bin-sorted order of a statistics pass.
# "shuffled": storage order permuted and no statistics pass -- the sweep walks the storage order, every tile a mixture of sites.
# "boundary": clusters 32 .. 63 hold no point, so the block of cluster 31 is followed by the block of cluster 64 (another word of the
# bitmaps, another 64-cluster chunk).  "wrong": previous labels rotated by one site.  "mixed": paired_problem's `mixed` tiles, no
# statistics pass (the compact table's slots run out in most tiles and are exactly used up in some).
MIXED_SITES = (13, 14, 15, 20, 26, 27, 32)


def all_cases():
    c = [(D, K, "sorted") for D in (3, 16) for K in (39, 40, 41, 65, 300)]
    c += [(D, K, "sorted") for D in (17, 32) for K in (25, 26, 27, 52, 53, 54, 65, 129)]
    c += [(D, 65, "shuffled") for D in (17, 32)] + [(D, 129, "mixed") for D in (17, 32)]
    c += [(D, K, "sorted") for D in (33, 64) for K in (38, 39, 79, 80)] + [(64, 65, "sorted"), (64, 65, "shuffled")]
    c += [(48, 65, "sorted"), (36, 65, "sorted"), (36, 65, "shuffled")]      # NB = 4 with block 3 all padding: the last features sit in block 2
    c += [(D, K, "sorted") for D in (65, 128) for K in (31, 33, 63, 64, 65, 129)]
    c += [(128, 65, "shuffled"), (128, 65, "boundary"), (128, 65, "wrong"), (72, 1024, "sorted")]
    c += [(129, 33, "sorted"), (129, 65, "sorted"), (256, 65, "sorted"), (256, 65, "shuffled"), (256, 65, "boundary"), (256, 65, "wrong")]
    c += [(68, 33, "sorted"), (132, 33, "sorted"), (144, 65, "sorted")]       # screened (D a multiple of 4) with the last features NOT in block NB - 1
    return c


def n_of(D):
    return 3000 if D <= 64 else 1500      # 46 wave tiles of 64 + one of 56 | 11 tiles of 128 + one of 92


HEAD = 300                       # D >= 65: two whole 128-point tiles of cluster 0 (its partner, cluster S, sits in another word from K = 65 on)


def case_problem(D, K, variant):
    kw = dict(head=HEAD) if D >= 65 and variant != "mixed" else {}
    if variant == "shuffled":
        kw["shuffled"] = True
    elif variant == "boundary":
        kw["empty"] = range(32, 64)
    elif variant == "mixed":
        kw["mixed"] = MIXED_SITES
    return paired_problem(D, n_of(D), K, seed=1000 * D + K, **kw)


def screened(D, K):
    """Does the sweep of this shape screen?  D <= 16 never; elsewhere the last screen needs K > 1, and D >= 65 also the 4-row tail
    records, which exist for D a multiple of 4 only."""
    return K > 1 and D > 16 and (D <= 64 or D % 4 == 0)
