"""The brute-force fp64 tree-level oracle of tests/_tree_util.py checked on its own (no GPU): every case
the kernel tests use keeps its near-tie nodes — the only ones excused from the exact (slot, bin) check —
within 1 in 10, and the library's torch oracle ``hist_split_torch`` agrees with the brute-force one."""
import numpy as np
import pytest
import torch

import _tree_util as U
from har.ops import tree as T

IMPURITIES = [U.GINI, U.ENTROPY]


def _cap(orc, what):
    near = U.near_tie_nodes(orc)
    assert int(near.sum()) * 10 <= len(near), f"{what}: near-tie nodes {np.nonzero(near)[0].tolist()} of {len(near)}"


@pytest.mark.parametrize("impurity", IMPURITIES)
@pytest.mark.parametrize("shape", U.SPLIT_SHAPES, ids=str)
def test_near_tie_cap_split_matrix(shape, impurity):
    orc = U.split_oracle(*shape, impurity)
    _cap(orc, f"{shape} impurity {impurity}")
    # the mix holds nodes with and without a valid split
    assert not orc.valid[0] and not orc.valid[1] and (shape[1] == 2 or orc.valid[6])


@pytest.mark.parametrize("impurity", IMPURITIES)
def test_near_tie_cap_other_cases(impurity):
    for K in (6, 12):
        _cap(U.brute_level(U.sparse_case(K), 1.0, 0.0, impurity), f"sparse K={K}")
    for permuted in (False, True):
        _cap(U.brute_level(U.planned_case(permuted), 1.0, 0.0, impurity), f"planned permuted={permuted}")
    par, child, _, _, _ = U.sibling_case()
    _cap(U.brute_level(par, 1.0, 0.0, impurity), "sibling parents")
    _cap(U.brute_level(child, 1.0, 0.0, impurity), "sibling children")


@pytest.mark.parametrize("impurity", IMPURITIES)
@pytest.mark.parametrize("shape", [(5, 32, 13, 13), (6, 64, 10, 10), (3, 7, 5, 5)], ids=str)
def test_hist_split_torch_matches_brute_force(shape, impurity):
    lv, hist = U.split_case(*shape)
    orc = U.split_oracle(*shape, impurity)
    got = T.hist_split_torch(lv.bins, lv.nbins, lv.label, lv.rows, lv.row_w, lv.key, lv.A, lv.feats, lv.K, lv.maxbins,
                             1.0, 0.0, impurity)
    U.check_level(got, orc, lv.feats, "hist_split_torch")
    th = T.level_histogram(lv.bins, lv.label, lv.rows, lv.row_w, lv.key, lv.A, lv.feats, lv.K, lv.maxbins)
    assert np.array_equal(th.numpy(), hist)


def test_check_level_rejects_wrong_results():
    """The comparison rule itself: a shifted bin, a wrong left count and a finite gain on a node without a
    split must each fail it."""
    shape = (5, 32, 13, 13)
    lv, _ = U.split_case(*shape)
    orc = U.split_oracle(*shape, U.GINI)
    good = T.hist_split_torch(lv.bins, lv.nbins, lv.label, lv.rows, lv.row_w, lv.key, lv.A, lv.feats, lv.K,
                              lv.maxbins, 1.0, 0.0, U.GINI)
    U.check_level(good, orc, lv.feats)
    a = 6
    for field, delta in (("bin", 1), ("left", 1.0), ("total", 1.0)):
        bad = T.LevelResult(**{k: getattr(good, k).clone() for k in ("gain", "feat", "bin", "left", "total")})
        getattr(bad, field)[a] += delta
        with pytest.raises(AssertionError):
            U.check_level(bad, orc, lv.feats)
    bad = T.LevelResult(**{k: getattr(good, k).clone() for k in ("gain", "feat", "bin", "left", "total")})
    bad.gain[0] = 0.0  # the empty node
    with pytest.raises(AssertionError):
        U.check_level(bad, orc, lv.feats)


def test_chunking_of_the_matrix_shapes():
    """The feature-chunk sizes the GPU cases are chosen for (ops/tree.py: fc = min(m, 96 KiB / slot bytes))."""
    assert T.LDS_BUDGET == U.LDS_BUDGET
    assert U.chunking(32, 64, 30) == (12, 3) and U.chunking(5, 32, 100) == (100, 1)
    assert U.chunking(5, 32, 13) == (13, 1) and U.chunking(2, 2, 1) == (1, 1)


def test_plan_words_definition():
    p = U.plan_words([0, 1, 64, 65, 129], 64)
    assert p["head"] == [1 + 1 + 1 + 2 + 3, 2, 5, 0]
    assert p["item_start"] == [0, 1, 2, 3, 5, 8] and p["big_rank"] == [-1, -1, -1, 0, 1]
    assert p["big_list"] == [3, 4] and p["item_node"] == [0, 1, 2, 3, 3, 4, 4, 4]
