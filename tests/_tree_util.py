"""Level problems, a brute-force fp64 oracle and the comparison rule shared by tests/test_tree_oracle.py
(CPU) and tests/test_gpu_tree_kernels.py (the tree.hip kernels)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

GINI, ENTROPY = 0, 1
RTOL, ATOL = 1e-5, 1e-6  # gains: fp64 in the kernel, cast to fp32 (tests/test_gpu_models.py's tolerance)
LDS_BUDGET = 96 * 1024

# Row counts every split-matrix case mixes: empty, one row, below / at / above the 256-thread workgroup
# (the "small node" / "large node" histogram paths of a chunk with more than 64 slots), one node of
# thousands of rows, and counts c that are no power of two with c * slots no multiple of 256: the small-node
# path splits the pair index j = slot * c + row with a float reciprocal, and at j = a multiple of c (and
# just below one) the estimate lands on either side, so the +-1 correction step runs.
NODE_COUNTS = [0, 1, 63, 255, 256, 257, 3000, 37, 201, 2, 130]
N_ROWS = 3500

# (K, maxbins, m, F): the split-search matrix (the path each reaches is named in test_gpu_tree_kernels.py)
SPLIT_SHAPES = [
    (2, 2, 1, 3),
    (5, 32, 13, 13),
    (9, 32, 12, 12),
    (17, 32, 12, 12),
    (32, 32, 8, 8),
    (6, 33, 10, 10),
    (6, 64, 10, 10),
    (32, 64, 30, 30),
    (5, 32, 100, 120),
    (3, 7, 5, 5),
]
ROUTE_SHAPES = [(5, 32, 13, 13), (32, 64, 30, 30), (5, 32, 100, 120)]


def chunking(K, maxbins, m):
    fc = max(1, min(m, LDS_BUDGET // (maxbins * K * 4)))
    return fc, (m + fc - 1) // fc


def default_nbins(F, maxbins, seed):
    """Per-feature bin counts that always hold 1 (no threshold), 2 and maxbins, cycling so that any large
    subset of the features holds every kind."""
    rs = np.random.RandomState(seed + 17)
    nb = rs.randint(1, maxbins + 1, size=F)
    nb[0::4] = maxbins
    nb[1::4] = 1
    nb[2::4] = min(2, maxbins)
    return nb.astype(np.int32)


def make_level(N, F, K, maxbins, nbins_per_feature, node_counts, m, seed, weights=(1, 2)):
    """One tree level as the kernels take it (CPU tensors): bins [F][N] uint8 with bins[f] < nbins[f] <=
    maxbins, labels, the nodes' rows / weights listed contiguously (rows of different nodes may overlap),
    key = the node of every listed row, feats [A][m] distinct features per node in random order.
    ``weights`` = (lo, hi): integer weights drawn from lo..hi inclusive (non-negative; sums << 2^24)."""
    rs = np.random.RandomState(seed)
    nb = np.asarray(nbins_per_feature, dtype=np.int32)
    assert nb.shape == (F,) and nb.min() >= 1 and nb.max() <= maxbins <= 64 and m <= F
    label = rs.randint(0, K, size=N).astype(np.int32)
    noise = 0.3 + 1.5 * rs.rand(F)  # a different signal strength per feature: distinct gains
    bins = np.empty((F, N), dtype=np.uint8)
    for f in range(F):
        v = (label / float(K) + noise[f] * rs.rand(N)) / (1.0 + noise[f])
        bins[f] = np.minimum((v * nb[f]).astype(np.int64), nb[f] - 1).astype(np.uint8)
    rows, keys = [], []
    for a, c in enumerate(node_counts):
        rows.append(np.sort(rs.permutation(N)[:c]))
        keys.append(np.full(c, a, dtype=np.int64))
    rows = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    row_w = rs.randint(weights[0], weights[1] + 1, size=rows.shape[0]).astype(np.float32)
    count = np.asarray(node_counts, dtype=np.int32)
    start = (np.cumsum(count) - count).astype(np.int32)
    feats = np.stack([rs.permutation(F)[:m] for _ in node_counts]).astype(np.int32)
    t = torch.from_numpy
    return SimpleNamespace(N=N, F=F, K=K, maxbins=maxbins, m=m, A=len(node_counts), bins=t(bins), nbins=t(nb),
                           label=t(label), rows=t(rows), row_w=t(row_w), node_start=t(start), node_count=t(count),
                           key=t(keys), feats=t(feats))


def on(lv, dev):
    """The level's tensors on ``dev`` (a copy of the namespace)."""
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(lv).items()}
    return SimpleNamespace(**d)


def _imp(c, kind):
    w = float(c.sum())
    if w <= 0.0:
        return 0.0
    p = c / w
    if kind == GINI:
        return 1.0 - float((p * p).sum())
    p = p[p > 0]
    return -float((p * np.log2(p)).sum())


def brute_hist(lv):
    """[A][m][maxbins][K] fp64 weighted class histograms, one (node, slot) at a time."""
    bins, label = lv.bins.numpy(), lv.label.numpy()
    rows, w = lv.rows.numpy(), lv.row_w.numpy().astype(np.float64)
    feats, start, count = lv.feats.numpy(), lv.node_start.numpy(), lv.node_count.numpy()
    hist = np.zeros((lv.A, lv.m, lv.maxbins, lv.K), dtype=np.float64)
    for a in range(lv.A):
        r = rows[start[a]:start[a] + count[a]]
        wa = w[start[a]:start[a] + count[a]]
        ya = label[r]
        for s in range(lv.m):
            np.add.at(hist[a, s], (bins[feats[a, s], r], ya), wa)
    return hist


def brute_level(lv, min_instances, min_info_gain, impurity, hist=None):
    """Plain fp64 oracle of one level: for every node the gain of every (slot, bin) threshold (-inf where
    the threshold does not exist or a child is lighter than min_instances), the left class counts, the
    node totals and the argmax under the tie rule highest gain, then lowest slot, then lowest bin.
    ``valid`` is False where no threshold qualifies or the best gain is below min_info_gain."""
    hist = brute_hist(lv) if hist is None else hist
    A, m, nb, K = hist.shape
    nbf, feats = lv.nbins.numpy(), lv.feats.numpy()
    gain = np.full((A, m, nb), -np.inf)
    left = np.zeros((A, m, nb, K))
    total = np.zeros((A, K))
    best_slot, best_bin = np.zeros(A, np.int64), np.zeros(A, np.int64)
    best_gain = np.full(A, -np.inf)
    for a in range(A):
        total[a] = hist[a, 0].sum(0)
        wt = float(total[a].sum())
        ip = _imp(total[a], impurity)
        for s in range(m):
            run = np.zeros(K)
            for b in range(nb):
                run = run + hist[a, s, b]
                left[a, s, b] = run
                if b >= nbf[feats[a, s]] - 1:
                    continue
                right = total[a] - run
                wl, wr = float(run.sum()), float(right.sum())
                if wl < min_instances or wr < min_instances or wt <= 0.0:
                    continue
                g = ip - (wl / wt) * _imp(run, impurity) - (wr / wt) * _imp(right, impurity)
                gain[a, s, b] = g
                if g > best_gain[a]:  # strict: the first (lowest slot, then lowest bin) maximum stays
                    best_gain[a], best_slot[a], best_bin[a] = g, s, b
    valid = np.isfinite(best_gain) & (best_gain >= min_info_gain)
    return SimpleNamespace(gain=gain, left=left, total=total, slot=best_slot, bin=best_bin, best=best_gain,
                           valid=valid, hist=hist, min_info_gain=min_info_gain)


def _tol(g):
    return ATOL + RTOL * abs(g)


def near_tie_nodes(orc):
    """Nodes whose best and second-best DISTINCT oracle gains differ by less than the gain tolerance: the
    only nodes where the kernel's (slot, bin) may differ from the oracle's argmax."""
    near = np.zeros(len(orc.best), dtype=bool)
    for a in range(len(orc.best)):
        if not orc.valid[a]:
            continue
        g = orc.gain[a]
        lower = g[np.isfinite(g) & (g < orc.best[a])]
        near[a] = lower.size > 0 and orc.best[a] - lower.max() < _tol(orc.best[a])
    return near


def check_level(got, orc, feats, what=""):
    """Compare a LevelResult (any device) with brute_level's tables; returns the near-tie node count."""
    gain, feat, bin_ = got.gain.cpu().numpy(), got.feat.cpu().numpy(), got.bin.cpu().numpy()
    left, total = got.left.cpu().numpy().astype(np.float64), got.total.cpu().numpy().astype(np.float64)
    feats = feats.cpu().numpy() if torch.is_tensor(feats) else feats
    near = near_tie_nodes(orc)
    A = len(orc.best)
    assert gain.shape == (A,) and left.shape == orc.total.shape
    for a in range(A):
        tag = f"{what} node {a}"
        assert np.array_equal(total[a], orc.total[a]), f"{tag}: total {total[a]} != {orc.total[a]}"
        if not orc.valid[a]:
            assert gain[a] == -np.inf, f"{tag}: no valid split, kernel gain {gain[a]}"
            continue
        assert np.isfinite(gain[a]), f"{tag}: oracle best {orc.best[a]} at {orc.slot[a], orc.bin[a]}, kernel -inf"
        slots = np.nonzero(feats[a] == feat[a])[0]
        assert slots.size == 1, f"{tag}: feature {feat[a]} is not one of the node's"
        s, b = int(slots[0]), int(bin_[a])
        og = orc.gain[a, s, b]
        assert np.isfinite(og), f"{tag}: kernel chose ({s}, {b}), no valid threshold there"
        assert abs(float(gain[a]) - og) <= _tol(og), f"{tag}: gain {gain[a]} vs oracle {og} at ({s}, {b})"
        assert np.array_equal(left[a], orc.left[a, s, b]), f"{tag}: left {left[a]} != {orc.left[a, s, b]}"
        if near[a]:
            assert orc.best[a] - og <= _tol(orc.best[a]), f"{tag}: near tie, chose gain {og} < best {orc.best[a]}"
        else:
            assert (s, b) == (orc.slot[a], orc.bin[a]), \
                f"{tag}: chose ({s}, {b}) gain {og}, oracle ({orc.slot[a]}, {orc.bin[a]}) gain {orc.best[a]}"
    assert int(near.sum()) * 10 <= A, f"{what}: {int(near.sum())} near-tie nodes of {A}"
    return int(near.sum())


@functools.lru_cache(maxsize=None)
def split_case(K, maxbins, m, F):
    """The level of one split-matrix shape (shared, read-only) and its fp64 histograms."""
    seed = 1000 * K + 10 * maxbins + m
    lv = make_level(N_ROWS, F, K, maxbins, default_nbins(F, maxbins, seed), NODE_COUNTS, m, seed)
    return lv, brute_hist(lv)


@functools.lru_cache(maxsize=None)
def split_oracle(K, maxbins, m, F, impurity):
    # min_instances = 1, not 0: with 0 the oracle's clamp of an empty node's weight and the kernel's
    # wt > 0 guard legitimately differ on empty nodes
    lv, hist = split_case(K, maxbins, m, F)
    return brute_level(lv, 1.0, 0.0, impurity, hist)


def assert_same(a, b, what=""):
    """Two LevelResults bit for bit (integer weights: every sum is exact in any order)."""
    for k in ("gain", "feat", "bin", "left", "total"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape, f"{what} {k}: shape {tuple(x.shape)} vs {tuple(y.shape)}"
        if x.dtype.is_floating_point:  # bitwise (-inf == -inf; no NaN is ever produced)
            same = torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
        else:
            same = torch.equal(x, y)
        assert same, f"{what}: {k} differs"


def plan_words(counts, prows):
    """tree_plan_kernel's layout: [items, big nodes, A, 0], item_start [A + 1], big_rank [A] (-1 = not big),
    big_list [big nodes valid], item_node [items]: a node of <= prows rows is one item, a bigger one
    ceil(count / prows) items and the next big-node rank."""
    A = len(counts)
    big = [c > prows for c in counts]
    zc = [-(-c // prows) if g else 1 for c, g in zip(counts, big)]
    item_start = [0] + list(np.cumsum(zc))
    big_list = [a for a in range(A) if big[a]]
    big_rank = [big_list.index(a) if big[a] else -1 for a in range(A)]
    item_node = [a for a in range(A) for _ in range(zc[a])]
    return dict(head=[item_start[-1], len(big_list), A, 0], item_start=item_start, big_rank=big_rank,
                big_list=big_list, item_node=item_node)


def random_forest_soa(T, K, F, max_depth, seed, x_pool=None):
    """Hand-made forest in the SoA layout of forest_predict ([T][maxn], feature < 0 = leaf): random valid
    trees of depth <= max_depth (children always at larger indices), thresholds drawn from ``x_pool`` (so
    some feature values equal a threshold exactly), non-negative leaf stats with some all-zero leaves."""
    rs = np.random.RandomState(seed)
    maxn = 2 ** (max_depth + 1) - 1
    feature = np.full((T, maxn), -1, np.int32)
    thr = np.zeros((T, maxn), np.float32)
    left = np.zeros((T, maxn), np.int32)
    right = np.zeros((T, maxn), np.int32)
    stats = np.zeros((T, maxn, K), np.float32)
    for t in range(T):
        nxt, todo = 1, [(0, 0)]
        while todo:
            n, d = todo.pop()
            if d < max_depth and rs.rand() < 0.8:
                feature[t, n] = rs.randint(0, F)
                thr[t, n] = rs.choice(x_pool) if x_pool is not None and rs.rand() < 0.5 else rs.randn()
                left[t, n], right[t, n] = nxt, nxt + 1
                todo += [(nxt, d + 1), (nxt + 1, d + 1)]
                nxt += 2
            elif rs.rand() < 0.85:  # (else: a leaf whose stats are all zero)
                stats[t, n] = rs.randint(0, 50, size=K)
    f = torch.from_numpy
    return f(feature), f(thr), f(left), f(right), f(stats)


# ---- shared cases of the one-hot-aware, planned and sibling-subtraction tests ----
SPARSE_COUNTS = [0, 1, 2, 63, 255, 257, 1500, 300, 37, 700]
PROWS = 64
PLAN_COUNTS = [0, 1, PROWS - 1, PROWS, PROWS + 1, 2 * PROWS, 2 * PROWS + 1, 10 * PROWS + 3]


@functools.lru_cache(maxsize=None)
def sparse_case(K):
    """2 one-hot blocks (columns 0..4 and 5..8; -1 = no entry; columns 4 and 8 are never set and column 3
    is declared without a threshold: nbins 1) beside 4 numeric columns 9..12, maxbins 32; the dense bins
    are the densified form bins_hybrid would write (a one-hot column's bin is 1 where it is the row's entry
    and the column has its threshold)."""
    N, F, maxbins = 2000, 13, 32
    nb = np.array([2, 2, 2, 1, 1, 2, 2, 2, 1, 32, 1, 2, 17], dtype=np.int32)
    lv = make_level(N, F, K, maxbins, nb, SPARSE_COUNTS, F, 77 + K)
    rs = np.random.RandomState(5 + K)
    y = lv.label.numpy()
    c0 = np.where(rs.rand(N) < 0.15, -1, (y + rs.randint(0, 2, N)) % 4)
    c1 = np.where(rs.rand(N) < 0.2, -1, 5 + (y // 2 + rs.randint(0, 2, N)) % 3)
    cat = np.stack([c0, c1], 1).astype(np.int32)
    bins = lv.bins.numpy().copy()
    bins[:9] = 0
    for c in range(2):
        r = np.nonzero(cat[:, c] >= 0)[0]
        f = cat[r, c]
        keep = nb[f] >= 2
        bins[f[keep], r[keep]] = 1
    lv.bins = torch.from_numpy(bins)
    lv.cat = torch.from_numpy(cat)
    lv.onehot = torch.tensor([1] * 9 + [0] * 4, dtype=torch.uint8)
    return lv


@functools.lru_cache(maxsize=None)
def planned_case(permuted):
    counts = list(PLAN_COUNTS)
    if permuted:
        counts = [counts[i] for i in np.random.RandomState(3).permutation(len(counts))]
    return make_level(1500, 13, 5, 32, default_nbins(13, 32, 9), counts, 13, 40 + int(permuted))


@functools.lru_cache(maxsize=None)
def sibling_case():
    """A parent level (every feature, in order, as the builder searches when it subtracts) and the level of
    its children: every parent's rows split on feature 0 at bin 15 (even parents) or 5 (odd ones).  Returns (parent level, child level
    with every child's rows listed, child level with only the lighter siblings' rows, parent_of,
    derive_from) — the heavier child (the right one on a weight tie) is derived, as the frontier kernel
    marks it."""
    F, K, maxbins = 6, 5, 32
    par = make_level(1500, F, K, maxbins, default_nbins(F, maxbins, 2), [300, 2 * PROWS + 1, PROWS, 40, 700], F, 21)
    par.feats = torch.arange(F, dtype=torch.int32).repeat(par.A, 1)
    rows, w = par.rows.numpy(), par.row_w.numpy()
    st, ct = par.node_start.numpy(), par.node_count.numpy()
    b0 = par.bins.numpy()[0]
    parts, parent_of, derive_from = [], [], []
    for p in range(par.A):
        r, ww = rows[st[p]:st[p] + ct[p]], w[st[p]:st[p] + ct[p]]
        goes_left = b0[r] <= (15 if p % 2 == 0 else 5)
        parts += [(r[goes_left], ww[goes_left]), (r[~goes_left], ww[~goes_left])]
        wl, wr = ww[goes_left].sum(), ww[~goes_left].sum()
        parent_of += [p, p]
        derive_from += ([2 * p + 1, -1] if wl > wr else [-1, 2 * p])

    def level(skip_derived):
        lv = SimpleNamespace(**vars(par))
        use = [(np.zeros(0, np.int32), np.zeros(0, np.float32)) if skip_derived and derive_from[i] >= 0 else pr
               for i, pr in enumerate(parts)]
        cnt = np.array([len(r) for r, _ in use], dtype=np.int32)
        lv.A = len(use)
        lv.rows = torch.from_numpy(np.concatenate([r for r, _ in use]).astype(np.int32))
        lv.row_w = torch.from_numpy(np.concatenate([x for _, x in use]).astype(np.float32))
        lv.node_count = torch.from_numpy(cnt)
        lv.node_start = torch.from_numpy((np.cumsum(cnt) - cnt).astype(np.int32))
        lv.key = torch.from_numpy(np.repeat(np.arange(lv.A), cnt).astype(np.int64))
        lv.feats = torch.arange(F, dtype=torch.int32).repeat(lv.A, 1)
        return lv

    return (par, level(False), level(True), torch.tensor(parent_of, dtype=torch.int32),
            torch.tensor(derive_from, dtype=torch.int32))
