"""tree.hip at kernel level against fp64 oracles: the histogram / split kernel on every route and search
path, the load-balanced plan and planned modes, sibling subtraction, forest_predict and tree_init.

The oracle (tests/_tree_util.py ``brute_level``) is checked on its own in tests/test_tree_oracle.py.  Every
weight is a non-negative integer, so class sums are exact in any order: totals / left counts must equal the
oracle exactly, the different routes must agree bit for bit, and the (slot, bin) winner must be the
oracle's argmax (highest gain, lowest slot, lowest bin) except on near-tie nodes (``check_level``)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _tree_util as U
from har.ops import _native, rng
from har.ops import tree as T

pytestmark = pytest.mark.gpu

IMPURITIES = [U.GINI, U.ENTROPY]
FIELDS = ("gain", "feat", "bin", "left", "total")


def _native_split(d, min_inst=1.0, min_gain=0.0, impurity=U.GINI, **kw):
    return T.hist_split_native(d.bins, d.nbins, d.label, d.rows, d.row_w, d.node_start, d.node_count, d.feats, d.K,
                               d.maxbins, min_inst, min_gain, impurity, **kw)


def _planned_split(d, impurity=U.GINI, prows=U.PROWS, **kw):
    return T.hist_split_planned(d.bins, d.nbins, d.label, d.rows, d.row_w, d.node_start, d.node_count, d.feats, d.K,
                                d.maxbins, 1.0, 0.0, impurity, rows_bound=max(1, int(d.rows.numel())), prows=prows,
                                **kw)


def _custom_level(bins, nbins, label, nodes, feats, K, maxbins):
    """A hand-made level: bins [F][N], nodes = [(rows, weights), ...], feats [A][m]."""
    cnt = np.array([len(r) for r, _ in nodes], dtype=np.int32)
    t = torch.from_numpy
    feats = np.asarray(feats, dtype=np.int32)
    return SimpleNamespace(
        N=bins.shape[1], F=bins.shape[0], K=K, maxbins=maxbins, m=feats.shape[1], A=len(nodes),
        bins=t(np.ascontiguousarray(bins, dtype=np.uint8)), nbins=t(np.asarray(nbins, dtype=np.int32)),
        label=t(np.asarray(label, dtype=np.int32)),
        rows=t(np.concatenate([np.asarray(r, dtype=np.int32) for r, _ in nodes])),
        row_w=t(np.concatenate([np.asarray(w, dtype=np.float32) for _, w in nodes])),
        node_start=t((np.cumsum(cnt) - cnt).astype(np.int32)), node_count=t(cnt),
        key=t(np.repeat(np.arange(len(nodes)), cnt).astype(np.int64)), feats=t(feats))


# ---- (a) split-search matrix, mode 0 ----
# (2, 2, 1)    smallest of everything: one slot, odd f_n (the pair search's second half idle)
# (5, 32, 13)  pair search, odd f_n, the rows-per-instruction (rpi) histogram path
# (9 | 17, 32, 12)  partial last class group of split_search_pairs<8>;  (32, 32, 8) KMAX
# (6, 33 | 64, 10)  one-slot-per-wave search, scan over all 64 lanes
# (32, 64, 30) fc = 12: 3 feature chunks, the last of 6 slots
# (5, 32, 100) F = 120: f_n > 64, the large-node (>= 256 rows) and small-node histogram paths
# (3, 7, 5)    maxbins no power of two
@pytest.mark.parametrize("impurity", IMPURITIES)
@pytest.mark.parametrize("shape", U.SPLIT_SHAPES, ids=str)
def test_split_matrix(cuda, shape, impurity):
    lv, _ = U.split_case(*shape)
    orc = U.split_oracle(*shape, impurity)
    got = _native_split(U.on(lv, cuda), impurity=impurity)
    U.check_level(got, orc, lv.feats, f"{shape}")


# ---- (b) the other routes equal mode 0 bit for bit ----
class _SliceOwner:
    """One "rank" owning the node slice [a0, a1) (tests/test_gpu_models.py)."""

    def __init__(self, a0, a1):
        self.a0, self.a1 = a0, a1

    def reduce_scatter(self, hist):
        return hist[self.a0:self.a1].clone(), self.a0, self.a1

    def all_gather(self, local, A):
        out = torch.zeros(A, *local.shape[1:], dtype=local.dtype, device=local.device)
        out[self.a0:self.a1] = local
        return out


@pytest.mark.parametrize("impurity", IMPURITIES)
@pytest.mark.parametrize("shape", U.ROUTE_SHAPES, ids=str)
def test_routes_equal_fused(cuda, shape, impurity):
    lv, _ = U.split_case(*shape)
    d = U.on(lv, cuda)
    base = _native_split(d, impurity=impurity)
    U.check_level(base, U.split_oracle(*shape, impurity), lv.feats)
    rm = d.bins.t().contiguous()
    U.assert_same(_native_split(d, impurity=impurity, bins_rm=rm), base, "row-major bins")
    U.assert_same(_native_split(d, impurity=impurity, allreduce=lambda t: None), base, "mode 1 + mode 2")
    # max_rows 5000 -> 3 row chunks, 9000 -> 5: neither divides 256 / 257 / 37, and 2- / 1- / 0-row nodes
    # leave workgroups of grid.z without rows
    for max_rows in (5000, 9000):
        U.assert_same(_native_split(d, impurity=impurity, max_rows=max_rows), base, f"row chunks {max_rows}")
    U.assert_same(_native_split(d, impurity=impurity, max_rows=5000, bins_rm=rm, allreduce=lambda t: None), base,
                  "row chunks + row-major + all-reduce")
    for a0, a1, kw in ((1, 4, {}), (0, 1, {}), (lv.A - 3, lv.A, {}), (2, 9, dict(max_rows=5000))):
        own = _native_split(d, impurity=impurity, owner=_SliceOwner(a0, a1), **kw)
        part = T.LevelResult(**{k: getattr(own, k)[a0:a1] for k in FIELDS})
        ref = T.LevelResult(**{k: getattr(base, k)[a0:a1] for k in FIELDS})
        U.assert_same(part, ref, f"owner slice [{a0}, {a1})")


# ---- (c) guards and ties ----
@pytest.mark.parametrize("maxbins", [8, 64])
@pytest.mark.parametrize("impurity", IMPURITIES)
def test_min_instances_exactly_met(cuda, maxbins, impurity):
    """One feature per node, bin weights 3 | 2 | 4 | 3: threshold 0 has wl == 3 and threshold 2 has wr == 3.
    Node 0's best threshold is 0 (a pure left child), node 1 reads the mirrored column, so its best is 2.
    With min_instances = 3 both are eligible and win; with 4 only threshold 1 is left."""
    b = np.array([0, 0, 1, 2, 2, 3])
    label = np.array([0, 0, 1, 1, 0, 1])
    w = np.array([1, 2, 2, 2, 2, 3], dtype=np.float32)
    rows = np.arange(6)
    lv = _custom_level(np.stack([b, 3 - b]), [4, 4], label, [(rows, w), (rows, w)], [[0], [1]], 2, maxbins)
    d = U.on(lv, cuda)
    for min_inst, want in ((3.0, [0, 2]), (4.0, [1, 1])):
        orc = U.brute_level(lv, min_inst, 0.0, impurity)
        assert orc.bin.tolist() == want and orc.valid.all()
        assert np.isfinite(orc.gain[:, 0, :3]).sum() == (6 if min_inst == 3.0 else 2)
        got = _native_split(d, min_inst=min_inst, impurity=impurity)
        U.check_level(got, orc, lv.feats, f"min_instances {min_inst}")
        assert got.bin.cpu().tolist() == want
    got = _native_split(d, min_inst=7.0, impurity=impurity)  # no threshold leaves 7 on both sides
    assert torch.isinf(got.gain).all() and (got.gain < 0).all()


@pytest.mark.parametrize("impurity", IMPURITIES)
@pytest.mark.parametrize("shape", [(5, 32, 13, 13), (6, 64, 10, 10)], ids=str)
def test_min_info_gain_boundary(cuda, shape, impurity):
    lv, hist = U.split_case(*shape)
    d = U.on(lv, cuda)
    a = 6  # the 3000-row node
    g = float(U.split_oracle(*shape, impurity).best[a])
    assert g > 1e-3
    for min_gain, kept in ((g * (1 - 1e-3), True), (g * (1 + 1e-3), False)):
        orc = U.brute_level(lv, 1.0, min_gain, impurity, hist)
        assert bool(orc.valid[a]) == kept
        # (no other node's best gain sits within the gain tolerance of the bound)
        assert all(abs(x - min_gain) > 1e-4 * min_gain for x in orc.best if np.isfinite(x))
        got = _native_split(d, min_gain=min_gain, impurity=impurity)
        U.check_level(got, orc, lv.feats, f"min_info_gain {min_gain}")
        assert bool(torch.isfinite(got.gain[a])) == kept


@pytest.mark.parametrize("impurity", IMPURITIES)
@pytest.mark.parametrize("shape", [(5, 32, 13, 13), (6, 64, 10, 10)], ids=str)
def test_pure_nodes(cuda, shape, impurity):
    """Single-class nodes: every gain is exactly 0, so the winner is the first valid threshold in (slot, bin)
    order with gain 0; any min_info_gain > 0 leaves no split."""
    K, maxbins, m, F = shape
    base, _ = U.split_case(*shape)
    lv = SimpleNamespace(**vars(base))
    lv.label = torch.zeros_like(base.label)  # class 0: the low bins are the populated ones
    feats = base.feats.clone()
    for a in range(lv.A):  # feature 0 (nbins = maxbins) in slot 0 of every node
        j = int((feats[a] == 0).nonzero()[0])
        feats[a, j], feats[a, 0] = feats[a, 0], 0
    lv.feats = feats
    orc = U.brute_level(lv, 1.0, 0.0, impurity)
    assert (orc.best[orc.valid] == 0).all() and orc.valid[6] and (orc.slot[6], orc.bin[6]) == (0, 0)
    d = U.on(lv, cuda)
    got = _native_split(d, impurity=impurity)
    U.check_level(got, orc, lv.feats, "pure")
    assert float(got.gain[6]) == 0.0 and int(got.feat[6]) == 0 and int(got.bin[6]) == 0
    assert (got.gain.cpu()[torch.from_numpy(orc.valid)] == 0).all()
    none = _native_split(d, min_gain=1e-6, impurity=impurity)
    assert torch.isinf(none.gain).all() and (none.gain < 0).all()


def _dup_level(K, maxbins, m, s1, s2):
    """A level whose features 1 and 2 hold the same, strongly informative column, listed at slots s1, s2."""
    lv = SimpleNamespace(**vars(U.make_level(2500, m, K, maxbins, U.default_nbins(m, maxbins, 3),
                                             [0, 1, 40, 300, 2000, 257, 63, 700, 129, 5], m, 600 + K)))
    rs = np.random.RandomState(K)
    y = lv.label.numpy()
    col = np.minimum(y * maxbins // K + rs.randint(0, 2, y.shape[0]), maxbins - 1).astype(np.uint8)
    bins, nb = lv.bins.clone(), lv.nbins.clone()
    bins[1] = bins[2] = torch.from_numpy(col)
    nb[1] = nb[2] = maxbins
    others = [f for f in range(m) if f not in (1, 2)]
    row = np.empty(m, dtype=np.int32)
    row[[s1, s2]] = [1, 2]
    row[[s for s in range(m) if s not in (s1, s2)]] = others
    lv.bins, lv.nbins = bins, nb
    lv.feats = torch.from_numpy(np.tile(row, (lv.A, 1)))
    return lv


@pytest.mark.parametrize("impurity", IMPURITIES)
@pytest.mark.parametrize("K,maxbins,m,lo,hi", [(5, 32, 13, 2, 9), (32, 64, 30, 3, 20), (32, 64, 30, 13, 14)])
def test_exact_tie_between_slots(cuda, K, maxbins, m, lo, hi, impurity):
    """The same column at two feature ids: the gains are bitwise equal, the lower slot wins — within one
    chunk, across two chunks (K = 32, maxbins = 64: chunks of 12 slots, ``_best_chunk``'s rule) and inside
    the second chunk."""
    fc, _ = U.chunking(K, maxbins, m)
    assert (lo // fc != hi // fc) == ((lo, hi) == (3, 20))
    for s1, s2, winner in ((lo, hi, 1), (hi, lo, 2)):
        lv = _dup_level(K, maxbins, m, s1, s2)
        d = U.on(lv, cuda)
        orc = U.brute_level(lv, 1.0, 0.0, impurity)
        got = _native_split(d, impurity=impurity)
        U.check_level(got, orc, lv.feats, "duplicate column")
        big = [a for a in range(lv.A) if lv.node_count[a] >= 257]
        assert all(int(got.feat[a]) == winner for a in big), (got.feat.cpu().tolist(), winner)
        # the tie is bitwise: each of the two features alone gives the identical gain and bin
        single = []
        for f in (1, 2):
            one = SimpleNamespace(**vars(d))
            one.feats = torch.full((lv.A, 1), f, dtype=torch.int32, device=cuda)
            one.m = 1
            single.append(_native_split(one, impurity=impurity))
        assert torch.equal(single[0].gain.view(torch.int32), single[1].gain.view(torch.int32))
        assert torch.equal(single[0].bin, single[1].bin) and torch.equal(single[0].left, single[1].left)
        for a in big:
            assert torch.equal(got.gain[a].view(torch.int32), single[0].gain[a].view(torch.int32))


@pytest.mark.parametrize("maxbins", [32, 64])
@pytest.mark.parametrize("impurity", IMPURITIES)
def test_equal_gain_bins_lowest_wins(cuda, maxbins, impurity):
    """Node 0: rows in bins 0 and 4 only of a 6-bin feature — thresholds 0..3 give the same partition, hence
    the same gain bit for bit.  Node 1 (gini): class counts (1, 3) | (5, 3) | (1, 3) over three bins —
    threshold 0 and threshold 1 are mirror images, and every term of both gains (weights 4 / 16 and 12 / 16,
    impurities 0.375 and 0.5, parent 126 / 256) is a short dyadic number, so both are exactly 3 / 128
    whatever the order of the operations.  The lower bin must win both."""
    rs = np.random.RandomState(0)
    n0 = 40
    b0 = np.where(np.arange(n0) < 25, 0, 4)
    y0 = np.where(b0 == 0, rs.randint(0, 2, n0), 1)
    cls = [(1, 3), (5, 3), (1, 3)]
    b1 = np.concatenate([np.full(c0 + c1, b) for b, (c0, c1) in enumerate(cls)])
    y1 = np.concatenate([np.array([0] * c0 + [1] * c1) for c0, c1 in cls])
    bins = np.zeros((2, n0 + len(b1)), dtype=np.uint8)
    bins[0, :n0], bins[1, n0:] = b0, b1
    label = np.concatenate([y0, y1])
    nodes = [(np.arange(n0), np.ones(n0, np.float32)), (np.arange(n0, n0 + len(b1)), np.ones(len(b1), np.float32))]
    lv = _custom_level(bins, [6, 3], label, nodes, [[0], [1]], 2, maxbins)
    orc = U.brute_level(lv, 1.0, 0.0, impurity)
    assert len(set(orc.gain[0, 0, :4].tolist())) == 1 and orc.bin[0] == 0 and orc.best[0] > 0.01
    got = _native_split(U.on(lv, cuda), impurity=impurity)
    assert int(got.bin[0]) == 0 and abs(float(got.gain[0]) - orc.best[0]) <= 1e-6
    assert torch.equal(got.left[0].cpu(), torch.from_numpy(orc.left[0, 0, 0]).float())
    if impurity == U.GINI:
        assert orc.gain[1, 0, 0] == orc.gain[1, 0, 1] == 3.0 / 128.0
        assert int(got.bin[1]) == 0 and float(got.gain[1]) == 3.0 / 128.0
        assert got.left[1].cpu().tolist() == [1.0, 3.0]


# ---- (d) one-hot-aware variant ----
@pytest.mark.parametrize("impurity", IMPURITIES)
@pytest.mark.parametrize("K", [6, 12])  # 12: class totals by LDS atomics (ktot) instead of registers
def test_onehot_aware_equals_dense(cuda, K, impurity):
    lv = U.sparse_case(K)
    d = U.on(lv, cuda)
    sp = T.SparseTreeInput(d.cat.contiguous(), d.onehot.contiguous(), lv.F)
    dense = _native_split(d, impurity=impurity)
    U.check_level(dense, U.brute_level(lv, 1.0, 0.0, impurity), lv.feats, "dense")
    U.assert_same(_native_split(d, impurity=impurity, sparse=sp), dense, "one-hot-aware, fused")
    U.assert_same(_native_split(d, impurity=impurity, sparse=sp, allreduce=lambda t: None), dense,
                  "one-hot-aware, mode 1 + mode 2")
    U.assert_same(_planned_split(d, impurity=impurity, sparse=sp), dense, "one-hot-aware, planned")


# ---- (e) plans and planned modes ----
def _run_plan(cuda, counts, prows, a_dev_count=None):
    A = len(counts)
    cd = torch.tensor(counts, dtype=torch.int32, device=cuda)
    items_ub = A + sum(counts) // prows
    plan = torch.full((4 + (A + 1) + 3 * A + items_ub,), -7, dtype=torch.int32, device=cuda)
    ad = None if a_dev_count is None else torch.tensor([a_dev_count], dtype=torch.int32, device=cuda)
    _native.kernels().tree_plan(cd.data_ptr(), A, prows, plan.data_ptr(), 1, 0, 0, 0,
                                0 if ad is None else ad.data_ptr(), _native.stream_ptr())
    return plan.cpu().tolist()


def _check_plan(words, counts, prows):
    A = len(counts)
    want = U.plan_words(counts, prows)
    nbig, items = want["head"][1], want["head"][0]
    o = 4
    assert words[:4] == want["head"]
    assert words[o:o + A + 1] == want["item_start"]
    o += A + 1
    assert words[o:o + A] == want["big_rank"]
    o += A
    assert words[o:o + nbig] == want["big_list"]
    o += A
    assert words[o:o + items] == want["item_node"]


@pytest.mark.parametrize("permuted", [False, True])
def test_plan_words(cuda, permuted):
    counts = U.planned_case(permuted).node_count.tolist()
    _check_plan(_run_plan(cuda, counts, U.PROWS), counts, U.PROWS)


def test_plan_words_many_nodes_and_device_count(cuda):
    """1025 nodes: a thread of the one-workgroup plan kernel owns two nodes; with ``a_dev`` the level's node
    count comes from the device (700) and the host's 1025 is only a bound."""
    counts = np.random.RandomState(4).randint(0, 6, size=1025).tolist()
    _check_plan(_run_plan(cuda, counts, 2), counts, 2)
    _check_plan(_run_plan(cuda, counts, 2, a_dev_count=700), counts[:700], 2)
    _check_plan(_run_plan(cuda, counts, 2, a_dev_count=1), counts[:1], 2)


@pytest.mark.parametrize("impurity", IMPURITIES)
@pytest.mark.parametrize("permuted", [False, True])
def test_planned_equals_fused_and_store(cuda, permuted, impurity):
    lv = U.planned_case(permuted)
    d = U.on(lv, cuda)
    orc = U.brute_level(lv, 1.0, 0.0, impurity)
    base = _native_split(d, impurity=impurity)
    U.check_level(base, orc, lv.feats, "fused")
    U.assert_same(_planned_split(d, impurity=impurity), base, "planned")
    U.assert_same(_planned_split(d, impurity=impurity, bins_rm=d.bins.t().contiguous()), base, "planned, row-major")
    ad = torch.tensor([lv.A], dtype=torch.int32, device=cuda)
    U.assert_same(_planned_split(d, impurity=impurity, a_dev=ad.data_ptr()), base, "planned, device count")
    store = torch.full((lv.A * lv.m * lv.maxbins * lv.K,), float("nan"), device=cuda)
    U.assert_same(_planned_split(d, impurity=impurity, store=store), base, "planned, by-node store")
    assert np.array_equal(store.cpu().numpy().astype(np.float64).reshape(orc.hist.shape), orc.hist)


@pytest.mark.parametrize("impurity", IMPURITIES)
def test_sibling_subtraction(cuda, impurity):
    """Mode 5 as the builder drives it (models/tree.py _levels_device_frontier): the parent level keeps its
    histograms (``store``); the child level lists the lighter siblings' rows only (a derived node has 0
    rows), and gets hprev = the parents' store, derive_from / parent_of = the frontier's marks."""
    par, full, light, parent_of, derive_from = U.sibling_case()
    assert (derive_from >= 0).sum() == par.A and (light.node_count[derive_from >= 0] == 0).all()
    slot = par.m * par.maxbins * par.K
    dp, df, dl = U.on(par, cuda), U.on(full, cuda), U.on(light, cuda)
    store_p = torch.full((par.A * slot,), float("nan"), device=cuda)
    res_p = _planned_split(dp, impurity=impurity, store=store_p)
    orc_p = U.brute_level(par, 1.0, 0.0, impurity)
    U.check_level(res_p, orc_p, par.feats, "parents")
    assert np.array_equal(store_p.cpu().numpy().astype(np.float64).reshape(orc_p.hist.shape), orc_p.hist)
    store_f = torch.full((full.A * slot,), float("nan"), device=cuda)
    res_f = _planned_split(df, impurity=impurity, store=store_f)
    orc_f = U.brute_level(full, 1.0, 0.0, impurity)
    U.check_level(res_f, orc_f, full.feats, "children")
    store_d = torch.full((full.A * slot,), float("nan"), device=cuda)
    res_d = T.hist_split_planned(dl.bins, dl.nbins, dl.label, dl.rows, dl.row_w, dl.node_start, dl.node_count,
                                 dl.feats, dl.K, dl.maxbins, 1.0, 0.0, impurity, rows_bound=int(df.rows.numel()),
                                 prows=U.PROWS, store=store_d, hprev=store_p, derive_from=derive_from.to(cuda),
                                 parent_of=parent_of.to(cuda))
    U.assert_same(res_d, res_f, "derived level")
    assert torch.equal(store_d, store_f)
    assert np.array_equal(store_d.cpu().numpy().astype(np.float64).reshape(orc_f.hist.shape), orc_f.hist)


# ---- (f) forest_predict ----
GRID = np.arange(-3.0, 3.5, 0.5).astype(np.float32)  # feature values and thresholds share it: x == thr occurs


def _predict_inputs(n, F, seed):
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(n, F, generator=g) * 2).round().clamp(-6, 6) / 2
    X[torch.rand(n, F, generator=g) < 0.1] = float("nan")
    return X


def _predict_oracle(X, forest, max_depth, normalize):
    feature, thr, left, right, stats = forest
    return T.forest_predict_torch(X.double(), feature, thr.double(), left, right, stats.double(), max_depth, normalize)


# K: the KC = 8 / 16 / 32 instantiations at and just past their bounds; ntrees < 16: lane-per-row kernel,
# >= 16: wave-per-row (65: lane 0 owns two trees, the others one)
@pytest.mark.parametrize("ntrees", [1, 15, 16, 65])
@pytest.mark.parametrize("K", [1, 8, 9, 16, 17, 32])
def test_forest_predict_matrix(cuda, K, ntrees):
    F = 7
    for max_depth in (0, 6):
        forest = U.random_forest_soa(ntrees, K, F, max_depth, 100 * K + ntrees, x_pool=GRID)
        fd = [t.to(cuda) for t in forest]
        if max_depth:
            assert (forest[0] >= 0).any() and (forest[4][forest[0] < 0].sum(-1) == 0).any()
        for n in (1, 3, 255, 257):
            X = _predict_inputs(n, F, n + K)
            if n > 3:
                assert torch.isnan(X).any() and torch.isin(X, torch.from_numpy(GRID)).any()
            for normalize in (True, False):
                ref = _predict_oracle(X, forest, max_depth, normalize)
                nat = T.forest_predict_native(X.to(cuda), *fd, max_depth, normalize)
                torch.testing.assert_close(nat.cpu().double(), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("ntrees", [1, 16])
def test_forest_predict_edges_by_hand(cuda, ntrees):
    """x == threshold goes left, NaN goes right, an all-zero leaf adds 0 when normalized."""
    feature = torch.tensor([[0, -1, 1, -1, -1]], dtype=torch.int32).repeat(ntrees, 1)
    thr = torch.tensor([[0.5, 0, -1.0, 0, 0]], dtype=torch.float32).repeat(ntrees, 1)
    left = torch.tensor([[1, 0, 3, 0, 0]], dtype=torch.int32).repeat(ntrees, 1)
    right = torch.tensor([[2, 0, 4, 0, 0]], dtype=torch.int32).repeat(ntrees, 1)
    stats = torch.zeros(ntrees, 5, 2)
    stats[:, 1] = torch.tensor([1.0, 3.0])
    stats[:, 3] = torch.tensor([2.0, 0.0])  # node 4: the all-zero leaf
    nan = float("nan")
    X = torch.tensor([[0.5, 9.0], [0.5000001, -1.0], [nan, -1.0], [nan, nan], [0.6, -0.5], [-7.0, nan]])
    fd = [t.to(cuda) for t in (feature, thr, left, right, stats)]
    leaf = torch.tensor([[1.0, 3.0], [2.0, 0.0], [2.0, 0.0], [0.0, 0.0], [0.0, 0.0], [1.0, 3.0]])
    raw = T.forest_predict_native(X.to(cuda), *fd, 2, False).cpu()
    assert torch.equal(raw, leaf * ntrees)
    norm = T.forest_predict_native(X.to(cuda), *fd, 2, True).cpu()
    want = leaf / leaf.sum(1, keepdim=True).clamp_min(1.0) * ntrees
    torch.testing.assert_close(norm, want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("ntrees", [3, 20])
def test_forest_predict_non_contiguous_input(cuda, ntrees):
    """Column- and row-sliced views: the kernel gets the contiguous copy's own leading dimension."""
    F, K, depth = 7, 5, 5
    forest = U.random_forest_soa(ntrees, K, F, depth, 9 + ntrees, x_pool=GRID)
    fd = [t.to(cuda) for t in forest]
    wide = _predict_inputs(301, F + 6, 1).to(cuda)
    for view in (wide[:, :F], wide[::2], wide[::2, :F], wide[1::3, 2:F + 2]):
        assert not view.is_contiguous()
        ref = _predict_oracle(view.cpu(), forest, depth, True)
        nat = T.forest_predict_native(view, *fd, depth, True)
        torch.testing.assert_close(nat.cpu().double(), ref, rtol=1e-5, atol=1e-5)
        assert torch.equal(nat, T.forest_predict_native(view.clone(memory_format=torch.contiguous_format), *fd, depth,
                                                        True))


# ---- (g) tree_init ----
def _tree_init(cuda, seed, tree0, ntrees, row0, n, cdf, rw, y, K, maxn=3):
    W = torch.full((ntrees, n), -5.0, device=cuda)
    node_of = torch.full((ntrees, n), 9, dtype=torch.int32, device=cuda)
    stats = torch.zeros(ntrees, maxn, K, device=cuda)
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    rwd = None if rw is None else torch.from_numpy(rw).to(cuda).contiguous()
    yd = torch.from_numpy(y).to(cuda)
    _native.kernels().tree_init(seed, tree0, ntrees, row0, n, [] if cdf is None else [int(v) for v in cdf],
                                0 if rwd is None else rwd.data_ptr(), yd.data_ptr(), K, W.data_ptr(),
                                node_of.data_ptr(), stats.data_ptr(), maxn * K, bad.data_ptr(), _native.stream_ptr())
    return W.cpu().numpy(), node_of.cpu().numpy(), stats.cpu().numpy(), int(bad.item())


@pytest.mark.parametrize("use_rw", [False, True])
@pytest.mark.parametrize("ncdf", [0, 15])
@pytest.mark.parametrize("K", [1, 32])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049])
def test_tree_init(cuda, n, K, ncdf, use_rw):
    seed, tree0, ntrees, row0 = 11, 5, 3, 1000
    rs = np.random.RandomState(n + K)
    y = rs.randint(0, K, size=n).astype(np.int32)
    cdf = rng.poisson_thresholds(1.0) if ncdf else None
    assert cdf is None or len(cdf) == ncdf
    rw = None
    if use_rw:  # 0 / 1 fold masks; tree 1 sees no row at all
        rw = rs.randint(0, 2, size=(ntrees, n)).astype(np.float32)
        rw[1] = 0
    W, node_of, stats, bad = _tree_init(cuda, seed, tree0, ntrees, row0, n, cdf, rw, y, K)
    want = rng.bootstrap_weights(seed, range(tree0, tree0 + ntrees), n, row0, cdf).astype(np.float32)
    if rw is not None:
        want = want * rw
    assert bad == 0
    assert np.array_equal(W, want)
    assert np.array_equal(node_of, np.where(want == 0, -1, 0))
    root = np.stack([np.bincount(y, weights=want[t], minlength=K) for t in range(ntrees)])
    assert np.array_equal(stats[:, 0], root) and not stats[:, 1:].any()


@pytest.mark.parametrize("n", [1, 2049])
def test_tree_init_bad_flags(cuda, n):
    """Bit 0: a label outside [0, K); bit 1: a weight that is no integer (or is negative / >= 2^24).  The bits
    are OR-ed, so one cannot erase the other."""
    K = 4
    y = np.random.RandomState(n).randint(0, K, size=n).astype(np.int32)
    ones = np.ones((2, n), dtype=np.float32)
    assert _tree_init(cuda, 1, 0, 2, 0, n, None, ones, y, K)[3] == 0
    for label in (K, -1):
        yb = y.copy()
        yb[n // 2] = label
        assert _tree_init(cuda, 1, 0, 2, 0, n, None, None, yb, K)[3] == 1
    for w, flag in ((0.5, 2), (1.5, 2), (2.0, 0), (0.0, 0), (-1.0, 2), (2.0 ** 24, 2), (2.0 ** 24 - 1, 0)):
        rw = ones.copy()
        rw[1, n - 1] = w
        assert _tree_init(cuda, 1, 0, 2, 0, n, None, rw, y, K)[3] == flag, w
    yb, rw = y.copy(), ones.copy()
    yb[0], rw[0, n // 3] = K, 0.25
    assert _tree_init(cuda, 1, 0, 2, 0, n, None, rw, yb, K)[3] == 3


# ---- fractional row weights are rejected on the device path ----
def _forest_problem():
    g = torch.Generator().manual_seed(5)
    mu = torch.randn(3, 6, generator=g) * 1.5
    y = torch.randint(0, 3, (600,), generator=g)
    return mu[y] + torch.randn(600, 6, generator=g), y


def _fit(device, X, y, rw, bootstrap=None):
    from har.models.tree import ForestBuilder

    b = ForestBuilder(3, num_trees=2, max_depth=4, seed=3, bootstrap=bootstrap)
    return b.fit(X.to(device), y.to(device), row_weight=rw.to(device))


def test_fractional_row_weight_rejected_on_device(cuda):
    """One 0.5 among unit weights (no bootstrap, so the product stays 0.5): the device path, whose histograms
    count in uint32, refuses the fit; the CPU builder takes the weights as given.  With the Poisson
    bootstrap a block of 1.5 weights meets odd draws."""
    X, y = _forest_problem()
    rw = torch.ones(2, 600)
    rw[1, 17] = 0.5
    with pytest.raises(ValueError, match="row weights"):
        _fit(cuda, X, y, rw, bootstrap=False)
    assert _fit("cpu", X, y, rw, bootstrap=False).n_nodes.min() >= 3
    rw[1, :200] = 1.5
    assert (rng.bootstrap_weights(3, [1], 200, 0, rng.poisson_thresholds(1.0)) % 2 == 1).any()
    with pytest.raises(ValueError, match="row weights"):
        _fit(cuda, X, y, rw)
    assert _fit("cpu", X, y, rw).n_nodes.min() >= 3


@pytest.mark.parametrize("bootstrap", [False, None])
def test_integer_row_weight_fits_on_both(cuda, bootstrap):
    X, y = _forest_problem()
    rw = torch.ones(2, 600)
    rw[1, 17] = 2.0
    rw[0, 5] = 0.0
    cpu, gpu = _fit("cpu", X, y, rw, bootstrap), _fit(cuda, X, y, rw, bootstrap)
    assert np.array_equal(cpu.n_nodes, gpu.n_nodes) and cpu.n_nodes.min() >= 3
    for k in ("feature", "threshold", "left", "right", "stats"):
        assert torch.equal(getattr(cpu, k), getattr(gpu, k).cpu()), k
