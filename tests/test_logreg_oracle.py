"""The logistic-regression test oracle and builders (tests/_logreg_util.py) checked on their own, and
against the CPU (torch) branches of the project: no GPU needed."""
import itertools

import numpy as np
import pytest
import torch

import _logreg_util as LU
from _logreg_util import f64


def _eval_inputs(p, S, T, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    F, K = p.F, p.K
    inv_std = (torch.rand(S, F, generator=g) + 0.5).to(f64)
    pmask = torch.ones(S, K, F + 1, dtype=f64)
    pmask[:, :, F // 2] = 0
    if K == 2:
        pmask[:, 0, :] = 0
    rw = torch.ones(S, p.N) if p.rw is None else p.rw
    inv_wsum = 1.0 / rw.to(f64).sum(1)
    xt = torch.randn(S * T, K, F + 1, generator=g).to(f64) * scale
    return xt, inv_std, pmask, inv_wsum


@pytest.mark.parametrize("K", [2, 6, 16])
def test_oracle_gradient_matches_finite_differences(K):
    """Central differences of the oracle's own fp64 loss along single coordinates.

    With step h the truncation error is at most h^2 M3 / 6, M3 bounding the third derivative of the
    loss along the coordinate: for coefficient (k, j) that is sum_i w_i (x_ij inv_std_j)^3 kappa3(p_ik)
    with sum_i w_i = 1 and |kappa3| = |p (1 - p) (1 - 2 p)| <= 1 / (6 sqrt 3) < 0.1, so
    M3 <= 0.1 (max|x| max inv_std)^3 (the intercept has x = 1).  The two loss values each carry a
    round-off of a few eps |loss| (an N-term fp64 sum of positive terms, pairwise in torch), so the
    quotient carries at most 4 eps max(1, |loss|) / h.  h = eps^(1/3) = 6.06e-6 balances the two; the
    bound asserted is their sum (~1e-9 here), nothing fitted to the result."""
    p = LU.make_problem(300, K, (7, 5), 6, seed=10 + K, weights="frac", S=2)
    S, T = 2, 1
    xt, inv_std, pmask, inv_wsum = _eval_inputs(p, S, T, seed=K)
    ref = LU.oracle_eval(p.X, p.y, p.rw, xt, T, inv_std, pmask, inv_wsum)
    eps = 2.0 ** -52
    h = eps ** (1.0 / 3.0)
    M3 = 0.1 * (max(1.0, float(p.X.abs().max())) * float(inv_std.max())) ** 3
    bound = h * h * M3 / 6 + 4 * eps * max(1.0, float(ref.loss.abs().max())) / h
    assert bound < 1e-8
    D = K * (p.F + 1)
    g = torch.Generator().manual_seed(99)
    coords = torch.randperm(D, generator=g)[:24].tolist()
    coords += [0 * (p.F + 1) + p.F // 2, (K - 1) * (p.F + 1) + p.F, (K - 1) * (p.F + 1)]  # frozen, intercept, row K-1
    for bt in range(S * T):
        for e in coords:
            d = torch.zeros_like(xt)
            d.view(S * T, D)[bt, e] = h
            lp = LU.oracle_eval(p.X, p.y, p.rw, xt + d, T, inv_std, pmask, inv_wsum).loss[bt]
            lm = LU.oracle_eval(p.X, p.y, p.rw, xt - d, T, inv_std, pmask, inv_wsum).loss[bt]
            fd = float(lp - lm) / (2 * h)
            assert abs(fd - float(ref.G[bt, e])) <= bound, (bt, e, fd, float(ref.G[bt, e]), bound)
    assert float(ref.G.view(S * T, K, p.F + 1)[:, :, p.F // 2].abs().max()) == 0.0
    if K == 2:
        assert float(ref.G.view(S * T, K, p.F + 1)[:, 0].abs().max()) == 0.0


@pytest.mark.parametrize("N,K,widths,Fd,weights", [(400, 6, (9, 4), 5, "frac"), (257, 12, (), 37, "binary")])
def test_oracle_eval_agrees_with_eval_torch(N, K, widths, Fd, weights):
    from har.ops.logreg import LogregDesign

    p = LU.make_problem(N, K, widths, Fd, seed=3, weights=weights, S=2)
    S, T = 2, 2
    xt, inv_std, pmask, inv_wsum = _eval_inputs(p, S, T, seed=4)
    ref = LU.oracle_eval(p.X, p.y, p.rw, xt, T, inv_std, pmask, inv_wsum)
    loss, G = LogregDesign(p.hm, p.y, p.rw.double(), K, native=False).eval_torch(xt, T, inv_std, pmask, inv_wsum)
    torch.testing.assert_close(ref.loss, loss, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref.G, G, rtol=1e-12, atol=1e-12)
    # the by-products are consistent with the gradient: intercept gradient = column sums of R
    torch.testing.assert_close(ref.R.sum(1) * pmask.repeat_interleave(T, 0)[:, :, p.F],
                               ref.G.view(S * T, K, p.F + 1)[:, :, p.F], rtol=1e-12, atol=1e-15)
    assert ref.Z.shape == (S * T, N, K)


@pytest.mark.parametrize("binomial,standardization,fit_intercept,weighted",
                         list(itertools.product([False, True], [True, False], [True, False], [False, True])))
def test_oracle_setup_agrees_with_cpu_setup(binomial, standardization, fit_intercept, weighted):
    from har.models.logreg import FitSpec, LogisticRegression

    K = 2 if binomial else 6
    p = LU.make_problem(300, K, (6, 5), 4, seed=21, empty=[(0, 2)], weights="frac" if weighted else "none", S=2,
                        const_dense=1)
    regs, alphas = [0.1, 0.3], [0.0, 0.2]
    specs = [FitSpec(None if p.rw is None else p.rw[i], regs[i], alphas[i]) for i in range(2)]
    est = LogisticRegression(standardization=standardization, fitIntercept=fit_intercept)
    c = est._setup(p.hm, p.y, specs, K, None)
    design, is_bin, Kp = c[0], c[1], c[2]
    assert is_bin == binomial and Kp == K
    rw = torch.ones(2, p.N) if p.rw is None else p.rw
    summ = LU.oracle_summary(p.X, p.y, rw, K)
    torch.testing.assert_close(design.summary(), summ, rtol=1e-12, atol=1e-9)
    o = LU.oracle_prepare(summ, regs, alphas, Kp, K, standardization, fit_intercept, binomial)
    for got, want in zip(c[3:], o):
        torch.testing.assert_close(got.double().reshape(want.shape), want, rtol=1e-5, atol=1e-6)
    frozen = [2, p.F - p.Fd + 1]  # the empty category and the constant dense column
    assert float(o[0][:, frozen].abs().max()) == 0.0 and float(c[3][:, frozen].abs().max()) == 0.0
    for t in (o[2], o[3].view(2, Kp, -1), o[4].view(2, Kp, -1), o[5]):
        assert float(t[:, :, frozen].abs().max()) == 0.0
    assert float(o[3].view(2, Kp, -1)[:, :, p.F].abs().max()) == 0.0  # intercept unregularized
    if binomial:
        assert float(o[2][:, 0].abs().max()) == 0.0 and float(o[5][:, 0].abs().max()) == 0.0


def test_oracle_prepare_small_weight_sum_divisor():
    """wsum <= 1: the variance divisor is max(wsum - 1, 1) = 1, i.e. var = (E x^2 - mean^2) wsum."""
    X = torch.tensor([[1.0], [3.0]])
    y = torch.tensor([0, 1])
    rw = torch.tensor([[0.25, 0.25]])
    summ = LU.oracle_summary(X, y, rw, 2)
    assert summ.tolist() == [[0.5, 1.0, 2.5, 0.25, 0.25]]
    inv_std = LU.oracle_prepare(summ, [0.0], [0.0], 2, 2, True, True, True)[0]
    assert float(inv_std[0, 0]) == pytest.approx(1.0 / np.sqrt((5.0 - 4.0) * 0.5), rel=1e-15)


@pytest.mark.parametrize("SL", [1, 16])
def test_oracle_col_slices_equals_cpu_col_slice(SL):
    from har.ops.logreg import LogregDesign

    p = LU.make_problem(900, 4, (30, 8), 3, seed=5, popular={0: (4, 0.5)}, empty=[(1, 3)])
    d = LogregDesign(p.hm, p.y, None, 4, native=False)
    d.SL = SL
    cs = d.col_slice()
    assert cs.shape[0] == p.F + 2
    assert np.array_equal(cs.numpy().astype(np.int64), LU.oracle_col_slices(d.csc_off.numpy(), SL))
    # and the scan by hand on a tiny offset list: lengths 0, 1, 16, 17 at SL = 16 -> 0, 1, 1, 2 slices
    assert LU.oracle_col_slices([0, 0, 1, 17, 34], 16).tolist() == [0, 0, 1, 2, 4]


def test_oracle_col_blocks_ok_accepts_and_rejects():
    off = np.array([0, 40, 40, 45, 45], dtype=np.int64)     # F + 1 = 4 columns (the last: intercept)
    SL = 16
    cs = LU.oracle_col_slices(off, SL)                      # 3, 0, 1, 0 slices
    assert cs.tolist() == [0, 3, 3, 4, 4]
    srow = [0, 16, 32, 40, 45]
    blk = [[0, 2, 0, 3], [2, 4, 3, 4]]
    assert LU.oracle_col_blocks_ok(blk, srow, cs, off, SL)
    for bad_blk, bad_srow in (([[0, 2, 0, 3]], srow), ([[0, 2, 0, 3], [3, 4, 4, 4]], srow),
                              ([[0, 2, 0, 2], [2, 4, 3, 4]], srow), (blk, [0, 16, 32, 41, 45]),
                              (blk, [0, 16, 32, 40, 44])):
        with pytest.raises(AssertionError):
            LU.oracle_col_blocks_ok(bad_blk, bad_srow, cs, off, SL)
    # more than 256 slices in a block of two columns is refused, in a single column it is fine
    off2 = np.array([0, 16 * 200, 16 * 400, 16 * 400], dtype=np.int64)
    cs2 = LU.oracle_col_slices(off2, SL)
    srow2 = list(range(0, 16 * 400 + 1, 16))
    with pytest.raises(AssertionError):
        LU.oracle_col_blocks_ok([[0, 3, 0, 400]], srow2, cs2, off2, SL)
    off3 = np.array([0, 16 * 400, 16 * 400], dtype=np.int64)
    assert LU.oracle_col_blocks_ok([[0, 1, 0, 400], [1, 2, 400, 400]], srow2, LU.oracle_col_slices(off3, SL), off3, SL)


def test_loss_fixed_point_mirror():
    g = torch.Generator().manual_seed(0)
    vals = (torch.randn(200, generator=g, dtype=f64) * 3).tolist() + [0.0, -0.0, 1.0, -1.0, 2.0 ** -41, -2.0 ** -41,
                                                                       3 * 2.0 ** -41, 2.0 ** 23 - 2.0 ** -20,
                                                                       -(2.0 ** 23 - 2.0 ** -20), 1234.56789, -7e6]
    for v in vals:
        p = LU.loss_fx_encode(v)
        assert p[4] == 0.0 and all(0 <= x <= 65535 for x in p[:3]) and -32768 <= p[3] <= 32767
        assert all(float(np.float32(x)) == x for x in p)        # every piece is an fp32 integer
        assert abs(LU.loss_fx_decode(p) - v) <= 2.0 ** -41
    assert LU.loss_fx_encode(2.0 ** -41) == [0.0] * 5 and LU.loss_fx_encode(3 * 2.0 ** -41)[0] == 2.0  # ties to even
    assert LU.loss_fx_encode(-2.0 ** -40) == [65535.0, 65535.0, 65535.0, -1.0, 0.0]
    for bad in (2.0 ** 23, -2.0 ** 23, float("inf"), float("-inf"), float("nan")):
        assert LU.loss_fx_encode(bad) == [0.0, 0.0, 0.0, 0.0, 1.0]
        assert np.isnan(LU.loss_fx_decode(LU.loss_fx_encode(bad)))
    # 8 ranks: the piecewise sums stay fp32 integers (< 2^24) and decode to the sum of the values
    eight = vals[:8]
    enc = np.array([LU.loss_fx_encode(v) for v in eight], dtype=np.float32)
    tot = enc.sum(axis=0, dtype=np.float32)
    assert np.array_equal(tot.astype(np.float64), np.array([LU.loss_fx_encode(v) for v in eight]).sum(axis=0))
    assert abs(LU.loss_fx_decode(tot.tolist()) - sum(eight)) <= 8 * 2.0 ** -41
    # and the mirror is the torch twin the data-parallel path uses
    from har.ops.logreg import pack_bucket

    tw = pack_bucket(torch.zeros(0), torch.tensor(vals + [float("nan")], dtype=f64)).view(-1, 5)
    assert tw.tolist() == [LU.loss_fx_encode(v) for v in vals + [float("nan")]]


def test_builder_keeps_its_promises():
    from har.ops.logreg import SLICE_ROWS

    p = LU.make_problem(5000, 3, (6,), 2, seed=1, popular={0: (2, 0.9)}, empty=[(0, 4)], weights="frac", S=2)
    assert int((p.cat[:, 0] == 2).sum()) > 256 * SLICE_ROWS           # the forced popular category
    assert int((p.cat[:, 0] == 4).sum()) == 0 and float(p.X[:, 4].abs().max()) == 0.0
    assert int((p.cat[:, 0] == -1).sum()) > 0 and int(p.cat[0, 0]) == -1
    assert torch.equal(p.hm.to_dense(), p.X)
    local = torch.where(p.hm.cat.long() >= 0, p.hm.cat.long() - 0, p.hm.cat.long())
    assert torch.equal(local, p.cat)
    zero = float((p.rw == 0).float().mean())
    assert 0.15 < zero < 0.25 and float(p.rw.max()) < 2.0 and float(p.rw[p.rw > 0].min()) > 0.0
    assert len(torch.unique(p.rw)) > 100                              # fractional, not 0/1
    q = LU.make_problem(40, 6, (6, 6, 6), 3, seed=2, const_dense=0, weights="binary")
    assert bool((q.cat[0] == -1).all()) and q.C == 3 and q.F == 21 and q.blocks == [(0, 6), (6, 6), (12, 6)]
    assert float((q.X[:, 18] - LU.CONST_VALUE).abs().max()) == 0.0
    assert set(torch.unique(q.rw).tolist()) <= {0.0, 1.0}
    z = LU.make_problem(3000, 6, (600,), 4, seed=3, zipf=1.0)
    counts = torch.bincount(z.cat[:, 0][z.cat[:, 0] >= 0], minlength=600)
    assert int(counts[0]) > 10 * SLICE_ROWS and int((counts == 0).sum()) > 0 and int((counts > 0).sum()) > 256
    one = LU.make_problem(1, 2, (4,), 3, seed=4, weights="frac", S=2)
    assert float(one.rw.sum(1).min()) > 0                              # no spec without weight
