"""A numpy oracle of the forest level loop's bookkeeping (tree_level.hip), one plain function per phase, the
comparison rule and the case generators shared by tests/test_tree_level_oracle.py (CPU) and
tests/test_gpu_tree_level.py (the kernels).

Every class count and weight a generator makes is dyadic (a multiple of 0.25) and every sum stays below
2^24, so each fp32 sum a kernel forms is exact in any order and no impurity lands near the 1e-12 cut:
every comparison is bit equality (``same``), NaN and -0.0 included."""
import functools
from types import SimpleNamespace

import numpy as np

GINI, ENTROPY = 0, 1
GROUP_CH = 1024  # rows per grouping chunk (one wave), 4 chunks per workgroup
I32, F32, I64 = np.int32, np.float32, np.int64


# ---- the oracle ----------------------------------------------------------------------------------------
def bits(x):
    """The int32 bit pattern of fp32 ``x`` (a scalar or an array)."""
    return np.asarray(x, dtype=F32).view(I32)


def _weight(c):
    return np.asarray(c, dtype=F32).sum(-1, dtype=F32)


def _impurity(c, w, kind):
    """fp64 impurity of the fp32 class counts ``c`` [..., K] of weight ``w`` (empty: weight clamped)."""
    p = np.asarray(c, dtype=np.float64) / np.maximum(np.asarray(w, dtype=np.float64), 1e-30)[..., None]
    if kind == GINI:
        return 1.0 - (p * p).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0).sum(-1)


def _candidate(c, kind, min2):
    w = _weight(c)
    return (_impurity(c, w, kind) > 1e-12) & (w >= F32(min2)), w


def root_frontier(stats, impurity, min2):
    """``stats`` [Tn, K] root class counts -> ct, cn, tlo [Tn + 1], cand_idx[:, 0] (-1: not a candidate, the
    entry is not written), scal = [0, candidates, 1, bits(max candidate weight) or 0]."""
    cand, w = _candidate(stats, impurity, min2)
    ct = np.nonzero(cand)[0].astype(I32)
    tlo = np.concatenate([[0], np.cumsum(cand)]).astype(I32)
    col0 = np.where(cand, tlo[:-1], -1).astype(I32)
    wbits = int(bits(w[cand].max())) if ct.size else 0
    return ct, np.zeros_like(ct), tlo, col0, np.array([0, ct.size, 1, wbits], dtype=I32)


def level_keys(node_of, cand_idx):
    """[T, N]: the candidate index of the node each row sits in, -1 for a row that is done or whose node is
    no candidate of this level."""
    t = np.arange(node_of.shape[0])[:, None]
    return np.where(node_of >= 0, cand_idx[t, np.maximum(node_of, 0)], -1).astype(I32)


def group(node_of, cand_idx, tlo, W):
    """The active (tree, row) pairs in the order of a stable sort of their keys over (tree, row):
    counts [A], starts [A], rows [total] (row ids inside the tree), row_w [total]; A = tlo[-1]."""
    key = level_keys(node_of, cand_idx)
    T, N = key.shape
    for t in range(T):  # the frontier is tree-ordered: tree t's candidates are [tlo[t], tlo[t + 1])
        k = key[t][key[t] >= 0]
        assert k.size == 0 or (k.min() >= tlo[t] and k.max() < tlo[t + 1])
    flat = key.reshape(-1)
    sel = np.nonzero(flat >= 0)[0]
    order = sel[np.argsort(flat[sel], kind="stable")]
    A = int(tlo[-1])
    counts = np.bincount(flat[sel], minlength=A).astype(I32)
    starts = (np.cumsum(counts) - counts).astype(I32)
    return counts, starts, (order % N).astype(I32), np.asarray(W, dtype=F32).reshape(-1)[order]


def decide(gain, left, total, impurity, min2):
    """[5, A] fp32: do_split (gain > 0 and finite), left / right child is a candidate of the next level
    (fp64 impurity > 1e-12 and fp32 weight >= min2), left / right weight."""
    gain = np.asarray(gain, dtype=F32)
    left = np.asarray(left, dtype=F32)
    right = np.asarray(total, dtype=F32) - left
    okl, wl = _candidate(left, impurity, min2)
    okr, wr = _candidate(right, impurity, min2)
    with np.errstate(invalid="ignore"):
        split = (gain > 0) & np.isfinite(gain)
    return np.stack([split.astype(F32), okl.astype(F32), okr.astype(F32), wl, wr]).astype(F32)


def frontier(ct, cn, tlo, dec, n_nodes, cand_idx, derive=False):
    """The frontier update of one level.  ``dec`` [5, A] (decide's record), ``n_nodes`` [Tn] nodes per tree,
    ``cand_idx`` [Tn, maxn].  Splitting candidates, in frontier order, get consecutive child-id pairs inside
    their tree; children flagged as candidates become the next frontier in (split, left-then-right) order.
    With ``derive``, of two candidate siblings the heavier (the right one on a tie) is derived: its
    cand_idx entry is -1 and derive_from names its sibling."""
    Tn = len(n_nodes)
    assert int(tlo[-1]) == len(ct) and np.all(np.diff(ct) >= 0)
    ds = dec[0] > 0
    dsi = np.nonzero(ds)[0].astype(I64)
    ti, ni = ct[ds].astype(I64), cn[ds].astype(I64)
    S = len(dsi)
    rank = np.arange(S) - np.searchsorted(ti, ti, side="left")
    cl = (n_nodes[ti] + 2 * rank).astype(I64)
    nn_next = (n_nodes + 2 * np.bincount(ti, minlength=Tn)).astype(I32)
    side = np.tile([0, 1], S)
    e_tree, e_node = np.repeat(ti, 2), np.repeat(cl, 2) + side
    e_flag = dec[1 + side, np.repeat(dsi, 2)] > 0
    e_w = dec[3 + side, np.repeat(dsi, 2)]
    q = np.cumsum(e_flag) - e_flag  # next-candidate index of a flagged entry
    ct_next, cn_next = e_tree[e_flag].astype(I32), e_node[e_flag].astype(I32)
    A_next = len(ct_next)
    tlo_next = np.searchsorted(ct_next, np.arange(Tn + 1), side="left").astype(I32)
    sib = np.arange(2 * S) ^ 1
    derived = np.zeros(2 * S, dtype=bool)
    if derive:
        derived = e_flag & e_flag[sib] & ((e_w > e_w[sib]) | ((e_w == e_w[sib]) & (side == 1)))
    ci = cand_idx.copy()
    ci[e_tree[e_flag], e_node[e_flag]] = np.where(derived[e_flag], -1, q[e_flag])
    per_tree = int(np.diff(tlo_next).max()) if Tn else 0
    wbits = int(bits(e_w[e_flag].max())) if A_next else 0
    out = SimpleNamespace(n_nodes_next=nn_next, ti=ti, ni=ni, cl=cl, dsi=dsi, ct_next=ct_next, cn_next=cn_next,
                          tlo_next=tlo_next, cand_idx=ci, scal=np.array([S, A_next, per_tree, wbits], dtype=I32))
    if derive:
        out.parent_of = np.repeat(dsi, 2)[e_flag].astype(I32)
        out.derive_from = np.where(derived, q[sib], -1)[e_flag].astype(I32)
    return out


FOREST_FIELDS = ("feature", "split_bin", "thresh", "left", "right", "gains", "stats")


def commit(arrs, ti, ni, cl, dsi, feat, bin_, gain, rleft, rtotal, thr_mat):
    """Copies of the forest arrays (a namespace of FOREST_FIELDS, [Tn, maxn] and stats [Tn, maxn, K]) with
    every split of the level written: the node's feature / bin / threshold / children / weighted gain
    (fp32 gain x fp32 node weight) and both children's class counts."""
    o = SimpleNamespace(**{k: getattr(arrs, k).copy() for k in FOREST_FIELDS})
    f, b = feat[dsi], bin_[dsi]
    o.feature[ti, ni] = f
    o.split_bin[ti, ni] = b
    o.thresh[ti, ni] = thr_mat[f, b]
    o.left[ti, ni] = cl
    o.right[ti, ni] = cl + 1
    o.gains[ti, ni] = np.asarray(gain, dtype=F32)[dsi] * _weight(rtotal[dsi])
    o.stats[ti, cl] = rleft[dsi]
    o.stats[ti, cl + 1] = np.asarray(rtotal, dtype=F32)[dsi] - np.asarray(rleft, dtype=F32)[dsi]
    return o


def partition(node_of, feature, split_bin, left, bins):
    """Rows of a split node move to left + (bin > split_bin); rows of any other node, and rows already
    at -1, are done (-1).  ``bins`` [F, N] uint8."""
    T, N = node_of.shape
    t = np.arange(T)[:, None]
    n = np.maximum(node_of, 0)
    f = feature[t, n]
    b = bins[np.maximum(f, 0), np.arange(N)[None, :]].astype(I64)
    child = left[t, n] + (b > split_bin[t, n])
    return np.where((node_of >= 0) & (f >= 0), child, -1).astype(I32)


# ---- the comparison rule ---------------------------------------------------------------------------------
def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view(I32) if a.dtype == F32 else a


def same(got, want, what=""):
    """Two arrays of one dtype and shape, bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    g, w = _raw(got), _raw(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} entries differ, first at {i}: "
                             f"got {got[i]!r}, want {want[i]!r}")


def same_fields(got, want, fields, what=""):
    """``same`` over the named fields of two namespaces / dicts."""
    get = (lambda o, k: o[k]) if isinstance(got, dict) else getattr
    getw = (lambda o, k: o[k]) if isinstance(want, dict) else getattr
    for k in fields:
        same(get(got, k), getw(want, k), f"{what} {k}")


GROUP_FIELDS = ("counts", "starts", "rows", "row_w")
FRONTIER_FIELDS = ("n_nodes_next", "ti", "ni", "cl", "dsi", "ct_next", "cn_next", "tlo_next", "cand_idx", "scal")
DERIVE_FIELDS = ("parent_of", "derive_from")


def group_ns(node_of, cand_idx, tlo, W):
    return SimpleNamespace(**dict(zip(GROUP_FIELDS, group(node_of, cand_idx, tlo, W))))


# ---- the case generators -----------------------------------------------------------------------------
def assert_dyadic(*arrays):
    """Every value is a non-negative multiple of 0.25 and the whole array sums below 2^24: any fp32 sum of
    a subset, in any order, is exact."""
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        assert np.all(np.isfinite(a)) and np.all(a >= 0) and np.all(a * 4 == np.round(a * 4))
        assert a.sum(-1).max(initial=0.0) < 2 ** 24
    return True


def _counts(rs, K, kind, min2):
    """Class counts [K] of one node of the named kind (K = 1: every non-empty node is pure)."""
    c = np.zeros(K, dtype=F32)
    a, b = (rs.permutation(K)[:2] if K >= 2 else (0, 0))
    if kind == "pure":
        c[a] = 0.25 * rs.randint(4 * int(min2), 400)
    elif kind == "exact":  # weight exactly min2 over two classes
        c[a] += 1.0
        c[b] += min2 - 1.0
    elif kind == "below":  # weight min2 - 0.25
        c[a] += 1.0
        c[b] += min2 - 1.25
    elif kind == "ordinary":  # some classes empty (entropy: p = 0 terms)
        c[:] = 0.25 * rs.randint(0, 200, size=K) * (rs.rand(K) < 0.7)
        c[a] += min2
        c[b] += 0.25
    else:
        assert kind == "empty"
    return c


KINDS = ("ordinary", "pure", "empty", "exact", "below")


@functools.lru_cache(maxsize=None)
def root_case(Tn, K, min2):
    """Root stats [Tn, maxn, K] with maxn = 3: node 0 cycles through KINDS (shuffled), nodes 1 and 2 hold
    non-zero junk a correct kernel never reads."""
    rs = np.random.RandomState(Tn * 100 + K)
    kinds = [KINDS[i] for i in rs.permutation(np.arange(Tn) % len(KINDS))]
    stats = (7.0 + rs.randint(0, 90, size=(Tn, 3, K))).astype(F32)
    for t in range(Tn):
        stats[t, 0] = _counts(rs, K, kinds[t], float(min2))
    assert_dyadic(stats[:, 0])
    return SimpleNamespace(Tn=Tn, K=K, maxn=3, min2=float(min2), stats=stats, kinds=kinds)


ROOT_TN = [1, 63, 1024, 1025, 2500]
CLASS_COUNTS = [1, 6, 33]
MIN2 = [2, 10]
IMPURITIES = [GINI, ENTROPY]

# (T, N, candidates per tree)
GROUP_SHAPES = [
    (1, 1, (1,)),
    (1, 63, (1,)),
    (3, 1024, (2, 0, 3)),
    (3, 1025, (3, 1, 0)),
    (5, 4100, (0, 64, 0, 129, 1)),
    (2, 2049, (65, 1)),
]
# the grouping's LDS limit: (T, N, candidates, nt_max passed) with maxn 8191
GROUP_LDS_SHAPES = [(1, 6000, (4096,), 4096), (1, 6000, (2500,), 4096)]


@functools.lru_cache(maxsize=None)
def group_case(T, N, cands, maxn=None):
    """node_of [T, N], cand_idx [T, maxn], tlo, W for one grouping call.  Of a tree's nodes, its candidates
    are a random subset (in random order of node id); rows sit in candidates, in nodes that are no candidate
    (cand_idx -1) or are out of bag (-1).  The last candidate of a tree with >= 2 has no rows.  Where the
    sizes allow: rows 0..63 of a tree share one key, rows 64..127 hold 64 different keys, and the second
    1024-row chunk of the last tree with candidates is fully inactive."""
    rs = np.random.RandomState(T * 7 + N)
    nt_real = max(cands)
    maxn = maxn or nt_real + 6
    tlo = np.concatenate([[0], np.cumsum(cands)]).astype(I32)
    cand_idx = np.full((T, maxn), -1, dtype=I32)
    node_of = np.empty((T, N), dtype=I32)
    spare = []
    for t, nt in enumerate(cands):
        nodes = rs.permutation(maxn)
        cnodes, others = nodes[:nt], nodes[nt:]
        spare.append(others[0])
        cand_idx[t, cnodes] = tlo[t] + np.arange(nt)
        fill = cnodes[:-1] if nt >= 2 else cnodes  # the last candidate keeps no rows
        u = rs.rand(N)
        pick = fill[rs.randint(0, len(fill), size=N)] if nt else np.full(N, -1)
        node_of[t] = np.where(u < 0.2, -1, np.where(u < 0.35, others[rs.randint(0, len(others), size=N)], pick))
        if nt and N >= 64:
            node_of[t, :64] = fill[0]
        if nt >= 65 and N >= 128:
            node_of[t, 64:128] = fill[:64]
    last = max(t for t, nt in enumerate(cands) if nt)
    if N > 2 * GROUP_CH:
        node_of[last, GROUP_CH:2 * GROUP_CH] = np.where(rs.rand(GROUP_CH) < 0.5, -1, spare[last])
    W = (0.25 * rs.randint(1, 13, size=(T, N))).astype(F32)
    assert_dyadic(W.reshape(1, -1))
    return SimpleNamespace(T=T, N=N, maxn=maxn, A=int(tlo[-1]), nt_max=nt_real, tlo=tlo, cand_idx=cand_idx,
                           node_of=node_of, W=W)


MAX_BIN = 63  # ForestBuilder: maxBins <= 64
PARTITION_SHAPES = [(2, 5), (3, 700_001)]  # the second: T * N > 8192 x 256 threads (the grid-stride loop)


@functools.lru_cache(maxsize=None)
def partition_case(T, N):
    """node_of [T, N] with rows at -1, per-node splits with some nodes at feature -1, bins [F, N] uint8 whose
    values are 0, MAX_BIN, or the split bin / split bin + 1 of the node of the row in tree 0 or 1."""
    rs = np.random.RandomState(N % 1000 + T)
    F, maxn = 3, 7
    feature = rs.randint(-1, F, size=(T, maxn)).astype(I32)
    feature[:, 0], feature[:, 1] = 0, -1
    split_bin = rs.randint(0, MAX_BIN, size=(T, maxn)).astype(I32)
    left = rs.randint(1, 1000, size=(T, maxn)).astype(I32)
    node_of = rs.randint(-1, maxn, size=(T, N)).astype(I32)
    node_of[0, :3] = [0, 0, -1]
    node_of[:, 3:5] = 0  # node 0 splits on feature 0 at bin 31 in every tree: rows 3 / 4 sit at 31 / 32
    split_bin[:, 0] = 31
    cand_idx = rs.randint(-1, 50, size=(T, maxn)).astype(I32)  # (the keys kernel's table)
    bins = np.empty((F, N), dtype=np.uint8)
    for f in range(F):
        sb = split_bin[f % min(T, 2), np.maximum(node_of[f % min(T, 2)], 0)]
        bins[f] = np.choose(rs.randint(0, 4, size=N), [np.zeros(N, I64), np.full(N, MAX_BIN), sb, sb + 1])
    bins[:, 0], bins[:, 1], bins[0, 3], bins[0, 4] = 0, MAX_BIN, 31, 32
    return SimpleNamespace(T=T, N=N, F=F, maxn=maxn, feature=feature, split_bin=split_bin, left=left,
                           node_of=node_of, cand_idx=cand_idx, bins=bins)


DECIDE_A = [1, 255, 256, 257]
DECIDE_K = [1, 2, 6, 33]
GAINS = np.array([0.5, 0.0, -0.25, np.nan, np.inf, -np.inf, 1e-30, -0.0], dtype=F32)


@functools.lru_cache(maxsize=None)
def decide_case(A, K, min2):
    """gain [A] cycling through GAINS, left / total [A, K] whose left and right children cycle through KINDS
    with different periods (every pair of kinds occurs once A >= 25)."""
    rs = np.random.RandomState(A * 50 + K)
    left = np.stack([_counts(rs, K, KINDS[a % 5], float(min2)) for a in range(A)])
    right = np.stack([_counts(rs, K, KINDS[(a // 5 + a) % 5], float(min2)) for a in range(A)])
    total = left + right
    assert_dyadic(left, right, total)
    gain = GAINS[(np.arange(A) + A) % len(GAINS)].copy()
    return SimpleNamespace(A=A, K=K, min2=float(min2), gain=gain, left=left, total=total)


FRONTIER_A = [1, 7, 8, 9, 1023, 8191, 8192, 8193, 20000]
SPLIT_PROB = [0.0, 0.5, 1.0]


@functools.lru_cache(maxsize=None)
def frontier_case(A, p_split):
    """A tree-ordered frontier of A candidates over Tn trees (about every third tree has none), distinct
    node ids inside a tree, node counters that differ per tree, a [5, A] decision record whose child flags
    are independent of the split flag and whose child weights tie often, and a cand_idx matrix full of stale
    non-negative entries."""
    rs = np.random.RandomState(A + int(10 * p_split))
    Tn = 1 if A == 1 else min(300, A // 3 + 2)
    has = rs.rand(Tn) < 0.67
    has[rs.randint(0, Tn)] = True
    if Tn >= 3:
        has[1] = False
    ct = np.sort(np.nonzero(has)[0][rs.randint(0, int(has.sum()), size=A)]).astype(I32)
    per = np.bincount(ct, minlength=Tn)
    n_nodes = (per + rs.randint(1, 9, size=Tn)).astype(I32)
    cn = np.concatenate([np.sort(rs.permutation(n_nodes[t])[:per[t]]) for t in range(Tn)]).astype(I32)
    tlo = np.concatenate([[0], np.cumsum(per)]).astype(I32)
    maxn = int((n_nodes + 2 * per).max()) + 2
    dec = np.empty((5, A), dtype=F32)
    dec[0] = rs.rand(A) < p_split
    dec[1:3] = rs.rand(2, A) < 0.6
    dec[3:5] = 0.25 * rs.randint(8, 14, size=(2, A))
    assert_dyadic(dec[3:5])
    cand_idx = (1_000_000 + np.arange(Tn * maxn)).reshape(Tn, maxn).astype(I32)
    return SimpleNamespace(A=A, Tn=Tn, maxn=maxn, ct=ct, cn=cn, tlo=tlo, dec=dec, n_nodes=n_nodes,
                           cand_idx=cand_idx)


COMMIT_S = [1, 256, 257]


@functools.lru_cache(maxsize=None)
def commit_case(S, K):
    """A level of A = S + 5 searched candidates of which S split, over 3 trees: commit records as the
    frontier kernel writes them, a LevelResult, thresholds [F, 40] of which 32 bins are used, and forest
    arrays full of junk."""
    rs = np.random.RandomState(S * 10 + K)
    Tn, F, ldthr, A = 3, 5, 40, S + 5
    dsi = np.sort(rs.permutation(A)[:S]).astype(I64)
    ti = np.sort(rs.randint(0, Tn, size=S)).astype(I64)
    per = np.bincount(ti, minlength=Tn)
    n_nodes = per + rs.randint(1, 5, size=Tn)
    ni = np.concatenate([rs.permutation(n_nodes[t])[:per[t]] for t in range(Tn)]).astype(I64)
    cl = (n_nodes[ti] + 2 * (np.arange(S) - np.searchsorted(ti, ti))).astype(I64)
    maxn = int((n_nodes + 2 * per).max()) + 3
    feat = rs.randint(0, F, size=A).astype(I32)
    bin_ = rs.randint(0, 32, size=A).astype(I32)
    gain = rs.rand(A).astype(F32)
    rleft = (0.25 * rs.randint(0, 200, size=(A, K))).astype(F32)
    rtotal = rleft + (0.25 * rs.randint(0, 200, size=(A, K))).astype(F32)
    assert_dyadic(rleft, rtotal)
    thr_mat = rs.randn(F, ldthr).astype(F32)
    arrs = SimpleNamespace(feature=rs.randint(-9, -1, size=(Tn, maxn)).astype(I32),
                           split_bin=rs.randint(100, 200, size=(Tn, maxn)).astype(I32),
                           thresh=rs.randn(Tn, maxn).astype(F32),
                           left=rs.randint(-99, -1, size=(Tn, maxn)).astype(I32),
                           right=rs.randint(-99, -1, size=(Tn, maxn)).astype(I32),
                           gains=rs.randn(Tn, maxn).astype(F32),
                           stats=(1000.0 + rs.randint(0, 50, size=(Tn, maxn, K))).astype(F32))
    return SimpleNamespace(S=S, K=K, A=A, Tn=Tn, F=F, ldthr=ldthr, maxn=maxn, ti=ti, ni=ni, cl=cl, dsi=dsi, feat=feat,
                           bin=bin_, gain=gain, rleft=rleft, rtotal=rtotal, thr_mat=thr_mat, arrs=arrs)


# ---- whole fits: the problem, the CPU builder's forest and the chained oracle ---------------------------
FIT_N, FIT_T, FIT_K, FIT_F, FIT_DEPTH, FIT_SEED = 700, 5, 4, 6, 10, 11
# (min_instances, impurity, featureSubsetStrategy)
FIT_CASES = [(1, "gini", "sqrt"), (5, "gini", "sqrt"), (1, "entropy", "sqrt"), (5, "entropy", "sqrt"),
             (1, "gini", "all")]


@functools.lru_cache(maxsize=None)
def fit_problem():
    import torch

    rs = np.random.RandomState(5)
    y = rs.randint(0, FIT_K, size=FIT_N)
    x = (rs.randn(FIT_N, FIT_F) + 0.8 * rs.randn(FIT_K, FIT_F)[y]).astype(F32)
    return torch.from_numpy(x), torch.from_numpy(y.astype(I64))


def fit_builder(min_inst, impurity, subset):
    from har.models.tree import ForestBuilder

    return ForestBuilder(FIT_K, FIT_T, FIT_DEPTH, 32, min_inst, 0.0, impurity, subset, bootstrap=True,
                         seed=FIT_SEED)


@functools.lru_cache(maxsize=None)
def fit_setup(min_inst, impurity, subset):
    """The CPU builder's forest and the level loop's inputs as numpy: bins [F, N], nbins, thr_mat, labels,
    bootstrap weights [T, N] (Poisson counts), root stats, the subset size m."""
    import torch

    from har.models.tree import subset_size

    x, y = fit_problem()
    b = fit_builder(min_inst, impurity, subset)
    ref = b.fit(x, y)
    W = b.bootstrap_weights(FIT_N, torch.device("cpu")).numpy().astype(F32)
    root = np.stack([np.bincount(y.numpy(), weights=W[t], minlength=FIT_K) for t in range(FIT_T)]).astype(F32)
    assert_dyadic(W.reshape(1, -1), root)
    maxn = ref.feature.shape[1]
    return SimpleNamespace(b=b, ref=ref, W=W, root=root, maxn=maxn, bins=b.bins.numpy(), nbins=b.nbins,
                           thr_mat=b.thr_mat.numpy(), y32=y.to(torch.int32), m=subset_size(subset, FIT_F, FIT_T),
                           min2=float(2 * min_inst), impurity=GINI if impurity == "gini" else ENTROPY)


def fit_state(fs):
    """The loop's initial state as the device builder sets it up."""
    Tn, maxn, K = FIT_T, fs.maxn, FIT_K
    arrs = SimpleNamespace(feature=np.full((Tn, maxn), -1, I32), split_bin=np.zeros((Tn, maxn), I32),
                           thresh=np.zeros((Tn, maxn), F32), left=np.zeros((Tn, maxn), I32),
                           right=np.zeros((Tn, maxn), I32), gains=np.zeros((Tn, maxn), F32),
                           stats=np.zeros((Tn, maxn, K), F32))
    arrs.stats[:, 0] = fs.root
    node_of = np.where(fs.W == 0, -1, 0).astype(I32)
    return arrs, node_of, np.ones(Tn, dtype=I32), np.full((Tn, maxn), -1, dtype=I32)


def level_feats(fs, ct, cn):
    from har.ops import rng

    if fs.m >= FIT_F:
        return np.tile(np.arange(FIT_F, dtype=I32), (len(ct), 1))
    return rng.feature_subsets(FIT_SEED, ct.astype(I64), cn.astype(I64), FIT_F, fs.m).astype(I32)


def split_search(fs, g, feats, hprev=None, parent_of=None, derive_from=None):
    """The part not under test: the library's CPU histogram + split search for one grouped level (``g``:
    group's outputs), as numpy (gain, feat, bin, left, total) plus the fp64 histograms.  A derived node
    (derive_from >= 0; no rows were grouped for it) takes parent - sibling, exact for integer weights."""
    import torch

    from har.ops import tree as T

    A = len(g.counts)
    key = torch.from_numpy(np.repeat(np.arange(A), g.counts).astype(I64))
    hist = T.level_histogram(torch.from_numpy(fs.bins), fs.y32, torch.from_numpy(g.rows), torch.from_numpy(g.row_w),
                             key, A, torch.from_numpy(feats), FIT_K, fs.b.max_bins)
    if derive_from is not None:
        d = np.nonzero(derive_from >= 0)[0]
        hist[torch.from_numpy(d)] = hprev[torch.from_numpy(parent_of[d].astype(I64))] \
            - hist[torch.from_numpy(derive_from[d].astype(I64))]
    r = T.split_from_hist(hist, torch.from_numpy(feats), fs.nbins, fs.b.min_inst, fs.b.min_gain, fs.impurity)
    return SimpleNamespace(gain=r.gain.numpy(), feat=r.feat.numpy(), bin=r.bin.numpy(),
                           left=np.ascontiguousarray(r.left.numpy()), total=np.ascontiguousarray(r.total.numpy())), hist


def chained_oracle(fs, derive=False, on_level=None):
    """The oracle phases chained level by level into a whole fit.  ``on_level(depth, lv)`` sees every
    level's inputs and oracle outputs (the teacher-forced GPU test replays them on the kernels).  Returns the
    forest arrays and n_nodes."""
    arrs, node_of, n_nodes, cand_idx = fit_state(fs)
    ct, cn, tlo, col0, scal = root_frontier(fs.root, fs.impurity, fs.min2)
    cand_idx[:, 0] = col0
    root = SimpleNamespace(ct=ct, cn=cn, tlo=tlo, col0=col0, scal=scal)
    hprev = parent_of = derive_from = None
    for depth in range(FIT_DEPTH):
        if len(ct) == 0:
            break
        g = group_ns(node_of, cand_idx, tlo, fs.W)
        feats = level_feats(fs, ct, cn)
        res, hist = split_search(fs, g, feats, hprev, parent_of, derive_from)
        dec = decide(res.gain, res.left, res.total, fs.impurity, fs.min2)
        fr = frontier(ct, cn, tlo, dec, n_nodes, cand_idx, derive)
        lv = SimpleNamespace(depth=depth, root=root, ct=ct, cn=cn, tlo=tlo, node_of=node_of, cand_idx=cand_idx,
                             n_nodes=n_nodes, arrs=arrs, group=g, feats=feats, res=res, dec=dec, fr=fr)
        if fr.scal[0] > 0:
            arrs = commit(arrs, fr.ti, fr.ni, fr.cl, fr.dsi, res.feat, res.bin, res.gain, res.left, res.total,
                          fs.thr_mat)
            node_of = partition(node_of, arrs.feature, arrs.split_bin, arrs.left, fs.bins)
        lv.arrs_next, lv.node_of_next = arrs, node_of
        if on_level is not None:
            on_level(depth, lv)
        if fr.scal[0] == 0:
            break
        n_nodes, cand_idx = fr.n_nodes_next, fr.cand_idx
        ct, cn, tlo = fr.ct_next, fr.cn_next, fr.tlo_next
        if derive:
            hprev, parent_of, derive_from = hist, fr.parent_of, fr.derive_from
    return arrs, n_nodes


def assert_forest(arrs, n_nodes, ref, what=""):
    """The oracle's / device loop's forest against a ForestArrays of the CPU builder, node for node."""
    same(n_nodes.astype(I64), np.asarray(ref.n_nodes, dtype=I64), f"{what} n_nodes")
    for mine, theirs in (("feature", "feature"), ("thresh", "threshold"), ("left", "left"), ("right", "right"),
                         ("stats", "stats"), ("gains", "gain")):
        same(getattr(arrs, mine), getattr(ref, theirs).numpy(), f"{what} {mine}")
