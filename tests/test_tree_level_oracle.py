"""The numpy oracle of the level loop's bookkeeping (tests/_tree_level_util.py) checked on its own (no GPU):
chained level by level it reproduces the CPU builder's forest bit for bit — which is what entitles it to judge
the tree_level.hip kernels in tests/test_gpu_tree_level.py — its grouping equals the CPU builder's, the
comparison rule rejects each kind of wrong result the kernels could produce, and every generated case keeps
the dyadic / < 2^24 contract that makes bit equality the right demand."""
import copy

import numpy as np
import pytest
import torch

import _tree_level_util as L


def _chain(min_inst, impurity, subset, derive):
    fs = L.fit_setup(min_inst, impurity, subset)
    seen = []
    arrs, n_nodes = L.chained_oracle(fs, derive=derive, on_level=lambda d, lv: seen.append(lv))
    L.assert_forest(arrs, n_nodes, fs.ref, f"{min_inst, impurity, subset}")
    # the problem is worth the name: several levels, the frontier thins out before maxDepth, and with
    # min_instances 5 some child is refused for its weight alone
    assert len(seen) >= 5 and int(n_nodes.max()) > 15
    assert seen[-1].depth < L.FIT_DEPTH - 1 or seen[-1].fr.scal[1] < 2 * seen[-1].fr.scal[0]
    if derive:
        assert any((lv.fr.derive_from >= 0).any() for lv in seen)


@pytest.mark.parametrize("min_inst,impurity,subset", L.FIT_CASES, ids=str)
def test_chained_oracle_equals_cpu_builder(min_inst, impurity, subset):
    """Oracle phases + the library's split search, to exhaustion, against ForestBuilder's CPU branch: n_nodes,
    feature, threshold, left, right, stats, gain."""
    _chain(min_inst, impurity, subset, derive=False)


def test_chained_oracle_with_derived_siblings_equals_cpu_builder():
    """featureSubsetStrategy "all" (a child searches its parent's features): the heavier sibling's histogram
    is parent - sibling and its rows are not grouped; the forest is the same."""
    _chain(1, "gini", "all", derive=True)


def test_group_equals_cpu_builder_grouping():
    """``group`` against the CPU builder's own lines (nonzero + stable argsort of the keys), on the frontier
    of every level of a fit."""
    fs = L.fit_setup(1, "gini", "sqrt")
    levels = []
    L.chained_oracle(fs, on_level=lambda d, lv: levels.append(lv))
    for lv in levels:
        node_of, W = torch.from_numpy(lv.node_of), torch.from_numpy(fs.W)
        cand_idx = torch.from_numpy(lv.cand_idx).long()
        # cand_idx keeps stale entries of earlier levels (no row sits in those nodes): the builder's is fresh
        fresh = torch.full_like(cand_idx, -1)
        fresh[torch.from_numpy(lv.ct).long(), torch.from_numpy(lv.cn).long()] = torch.arange(len(lv.ct))
        key = torch.where(node_of >= 0, fresh.gather(1, node_of.clamp_min(0).long()),
                          torch.full_like(node_of, -1, dtype=torch.int64))
        tt, rr = torch.nonzero(key >= 0, as_tuple=True)
        kk = key[tt, rr]
        order = torch.argsort(kk, stable=True)
        L.same(lv.group.rows, rr[order].to(torch.int32).numpy(), f"level {lv.depth} rows")
        L.same(lv.group.row_w, W[tt[order], rr[order]].numpy(), f"level {lv.depth} row_w")
        L.same(lv.group.counts, torch.bincount(kk, minlength=len(lv.ct)).to(torch.int32).numpy(), "counts")
        L.same(L.level_keys(lv.node_of, lv.cand_idx), key.to(torch.int32).numpy(), f"level {lv.depth} keys")


# ---- the comparison rule rejects wrong results ----
def _fails(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def test_comparison_rejects_unstable_grouping():
    c = L.group_case(*L.GROUP_SHAPES[2])
    good = L.group_ns(c.node_of, c.cand_idx, c.tlo, c.W)
    L.same_fields(good, copy.deepcopy(good), L.GROUP_FIELDS)
    a = int(np.argmax(good.counts >= 2))
    i = int(good.starts[a])
    bad = copy.deepcopy(good)
    bad.rows[[i, i + 1]] = bad.rows[[i + 1, i]]  # two rows of one key, swapped: still grouped, not stable
    bad.row_w[[i, i + 1]] = bad.row_w[[i + 1, i]]
    _fails(L.same_fields, bad, good, L.GROUP_FIELDS)


def test_comparison_rejects_wrong_frontier():
    c = L.frontier_case(1023, 0.5)
    good = L.frontier(c.ct, c.cn, c.tlo, c.dec, c.n_nodes, c.cand_idx, derive=True)
    fields = L.FRONTIER_FIELDS + L.DERIVE_FIELDS
    L.same_fields(good, copy.deepcopy(good), fields)
    # one tree's child ids shifted by 2
    t = int(good.ti[len(good.ti) // 2])
    bad = copy.deepcopy(good)
    bad.cl[bad.ti == t] += 2
    _fails(L.same_fields, bad, good, fields)
    # the derive tie flipped to the left child
    e = np.nonzero((good.derive_from >= 0) & (good.cn_next % 2 == (c.n_nodes[good.ct_next] + 1) % 2))[0]
    w = c.dec[3:5, good.parent_of]
    e = e[w[0, e] == w[1, e]]
    assert e.size, "the case holds no sibling pair of equal weight"
    r = int(e[0])  # a derived right child of a tie; its sibling is the entry before it
    bad = copy.deepcopy(good)
    bad.derive_from[r], bad.derive_from[r - 1] = -1, r
    bad.cand_idx[bad.ct_next[r], bad.cn_next[r]] = r
    bad.cand_idx[bad.ct_next[r - 1], bad.cn_next[r - 1]] = -1
    _fails(L.same_fields, bad, good, fields)
    for k in ("derive_from", "cand_idx"):  # (each of the two arrays alone gives it away)
        _fails(L.same, getattr(bad, k), getattr(good, k))
    # a tlo_next entry of a candidate-less tree dropped
    empty = np.nonzero(np.diff(good.tlo_next) == 0)[0]
    assert empty.size
    bad = copy.deepcopy(good)
    bad.tlo_next = np.delete(bad.tlo_next, empty[0])
    _fails(L.same_fields, bad, good, fields)
    bad.tlo_next = np.append(bad.tlo_next, good.tlo_next[-1])  # ... and the rest shifted up to keep the length
    if not np.array_equal(bad.tlo_next, good.tlo_next):
        _fails(L.same_fields, bad, good, fields)


def test_comparison_rejects_split_on_nan_gain():
    c = L.decide_case(257, 6, 2)
    good = L.decide(c.gain, c.left, c.total, L.GINI, c.min2)
    L.same(good, good.copy())
    a = int(np.argmax(np.isnan(c.gain)))
    assert np.isnan(c.gain[a]) and good[0, a] == 0.0
    bad = good.copy()
    bad[0, a] = 1.0
    _fails(L.same, bad, good)
    # every non-positive or non-finite gain refuses the split; -0.0 and the smallest positive gain differ
    assert good[0].tolist() == [float(g > 0 and np.isfinite(g)) for g in c.gain]
    assert {float(good[0, i]) for i in range(c.A) if c.gain[i] == np.float32(1e-30)} == {1.0}


def test_comparison_rejects_row_at_split_bin_moved_right():
    c = L.partition_case(*L.PARTITION_SHAPES[0])
    good = L.partition(c.node_of, c.feature, c.split_bin, c.left, c.bins)
    L.same(good, good.copy())
    assert c.bins[0, 3] == c.split_bin[0, 0] and c.node_of[0, 3] == 0 and good[0, 3] == c.left[0, 0]
    assert good[0, 4] == c.left[0, 0] + 1  # (the row one bin above goes right)
    bad = good.copy()
    bad[0, 3] += 1
    _fails(L.same, bad, good)
    # a row already at -1 stays, a row of a node without a split finishes
    assert good[0, 2] == -1 and np.all(good[c.node_of == 1] == -1)


def test_same_compares_bits_dtypes_and_shapes():
    x = np.array([0.0, np.nan, 1.0], dtype=np.float32)
    L.same(x, x.copy())
    _fails(L.same, x, np.array([-0.0, np.nan, 1.0], dtype=np.float32))
    _fails(L.same, x, x.astype(np.float64))
    _fails(L.same, x, x[:2])
    _fails(L.same, np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int64))


# ---- the generators keep their contract on every case the GPU file uses ----
def test_generated_cases_are_dyadic_and_in_range():
    for min2 in L.MIN2:
        for K in L.CLASS_COUNTS:
            for Tn in L.ROOT_TN:
                c = L.root_case(Tn, K, min2)
                L.assert_dyadic(c.stats[:, 0])
                w = c.stats[:, 0].sum(1)
                assert Tn < 5 or {"exact", "below", "empty", "pure", "ordinary"} == set(c.kinds)
                assert all(w[t] == min2 for t in range(Tn) if c.kinds[t] == "exact")
                assert all(w[t] == min2 - 0.25 for t in range(Tn) if c.kinds[t] == "below")
            for S in L.COMMIT_S:
                c = L.commit_case(S, K)
                L.assert_dyadic(c.rleft, c.rtotal, c.rtotal - c.rleft)
                assert c.bin.max() < 32 < c.ldthr and len(set(zip(c.ti.tolist(), c.ni.tolist()))) == S
                assert c.cl.max() + 1 < c.maxn
        for K in L.DECIDE_K:
            for A in L.DECIDE_A:
                c = L.decide_case(A, K, min2)
                L.assert_dyadic(c.left, c.total, c.total - c.left)
                if A >= 255:
                    for g in (np.isnan(c.gain), np.isposinf(c.gain), np.isneginf(c.gain), c.gain > 0, c.gain < 0,
                              c.gain == 0):
                        assert g.any()
    for shape in L.GROUP_SHAPES + [s[:3] + (8191,) for s in L.GROUP_LDS_SHAPES]:
        c = L.group_case(*shape)
        L.assert_dyadic(c.W.reshape(1, -1))
        g = L.group_ns(c.node_of, c.cand_idx, c.tlo, c.W)
        assert c.node_of.min() == -1 or c.N == 1
        assert c.node_of.max() < c.maxn and int(g.counts.sum()) == len(g.rows) < c.T * c.N or c.N == 1
        if max(shape[2]) >= 2:
            assert (g.counts == 0).any(), "a candidate without rows"
        if c.N > 2 * L.GROUP_CH:  # the fully inactive chunk
            t = max(i for i, n in enumerate(shape[2]) if n)
            assert np.all(L.level_keys(c.node_of, c.cand_idx)[t, L.GROUP_CH:2 * L.GROUP_CH] == -1)
    for A in L.FRONTIER_A:
        for p in L.SPLIT_PROB:
            c = L.frontier_case(A, p)
            L.assert_dyadic(c.dec[3:5])
            f = L.frontier(c.ct, c.cn, c.tlo, c.dec, c.n_nodes, c.cand_idx, derive=True)
            assert f.n_nodes_next.max() <= c.maxn and c.cand_idx.min() >= 0
            assert A < 7 or (np.diff(c.tlo) == 0).any(), "a candidate-less tree"
            assert len(set(zip(c.ct.tolist(), c.cn.tolist()))) == A
            if p == 0.0:
                assert f.scal.tolist() == [0, 0, 0, 0] and not f.tlo_next.any()
                L.same(f.n_nodes_next, c.n_nodes)
                L.same(f.cand_idx, c.cand_idx)
            if p > 0 and A >= 1023:
                d = f.derive_from >= 0
                w = c.dec[3:5, f.parent_of]
                assert (d & (w[0] == w[1])).any() and (~d).any() and len(set(c.n_nodes.tolist())) > 1
    assert 2 * L.frontier(*[getattr(L.frontier_case(20000, 1.0), k) for k in
                            ("ct", "cn", "tlo", "dec", "n_nodes", "cand_idx")]).scal[0] == 40000
    for shape in L.PARTITION_SHAPES:
        c = L.partition_case(*shape)
        assert c.bins.min() == 0 and c.bins.max() == L.MAX_BIN and (c.feature == -1).any()
        assert (c.node_of == -1).any() and c.split_bin.max() < L.MAX_BIN
    assert L.PARTITION_SHAPES[1][0] * L.PARTITION_SHAPES[1][1] > 8192 * 256
