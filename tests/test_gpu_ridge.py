"""RidgeClassifier on the device: every kernel of csrc/kernels/ridge.hip against the definitions of
har/ops/ridge.py — the moments exactly on exact-arithmetic data and within the chain bound on real data, the
factorisation and the solve within Higham's componentwise bounds, the fit against the fp64 oracle."""
import numpy as np
import pytest
import torch

from _ridge_util import (EXACT_D, EXACT_F, EXACT_K, EXACT_N, EXCLUDED_CAP, FIT_ALPHAS, FIT_CASES, R, chain_bound,
                         exact_case, excluded_rows, fit_case, gamma, real_case, spd_batch)
from har.models.ridge import RidgeClassificationModel, RidgeClassifier
from har.ops import _native
from har.ops import ridge as RD
from har.utils import persist

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    return torch.device("cuda:0")


def _moments(case, K, dev, cps=None):
    X, y, rows, off, mean, inv_std = case
    Af, Aall = RD.moments_native(X.to(dev), y.to(dev), rows.to(dev), off, mean.to(dev), inv_std.to(dev), K, cps)
    Dq = X.shape[1] + K + 1
    return (None if Af is None else Af.cpu()), Aall.cpu(), Dq


def test_constants():
    mod = _native.kernels()
    assert mod.ridge_chunk_rows() == RD.R and mod.ridge_panel() == RD.PANEL and mod.ridge_max_dim() == RD.MAX_DIM


# ------------------------------------------------------------------ 1. moments, exact
@pytest.mark.parametrize("D", EXACT_D)
def test_gram_exact(cuda, D):
    for K in EXACT_K:
        for N in EXACT_N:
            for F in EXACT_F:
                case = exact_case(D, K, N, F)
                assert not torch.equal(case[2], torch.arange(N, dtype=torch.int32)) or N == 1
                Af, Aall, Dq = _moments(case, K, cuda)
                of, oall = RD.moments_torch(*case, K, chain="fp64")      # exact data: every evaluation order agrees
                assert torch.equal(Aall[:Dq, :Dq], torch.triu(oall)), (D, K, N, F)
                assert not bool(Aall[Dq:].any()) and not bool(Aall[:, Dq:].any())
                if F > 1:
                    assert torch.equal(Af[:, :Dq, :Dq], torch.triu(of)), (D, K, N, F)
                    assert float(Af[:, Dq - 1, Dq - 1].sum()) == N


# ------------------------------------------------------------------ 2. moments, real-valued
def test_gram_real_valued_within_the_chain_bound(cuda):
    """Every entry within gamma_R sum |a_i a_j| of the fp64 evaluation on the same fp32 rows.  Measured on the
    MI355X: largest error / bound 0.0391 (PARITY.md)."""
    case = real_case()
    K = 6
    Af, Aall, Dq = _moments(case, K, cuda)
    ref, bound = chain_bound(*case, K)
    err = (Af[:, :Dq, :Dq] - torch.triu(ref)).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"ridge_gram largest error / bound: {ratio:.4f}")
    assert bool((err <= torch.triu(bound)).all())
    Af2, Aall2, _ = _moments(case, K, cuda)
    assert torch.equal(Af, Af2) and torch.equal(Aall, Aall2)                 # two runs: bitwise
    for cps in (1, 3):                                                      # other workgroup splits: 2^-50 relative
        Af3, Aall3, _ = _moments(case, K, cuda, cps)
        assert bool(((Af3 - Af).abs() <= 2.0 ** -50 * Af.abs()).all())
        assert bool(((Aall3 - Aall).abs() <= 2.0 ** -50 * Aall.abs()).all())


# ------------------------------------------------------------------ 3. factorisation, 4. solve
SHAPES = [(1, 0), (61, 2), (63, 0), (62, 2), (64, 0), (63, 2), (65, 0), (127, 2), (129, 0), (194, 6), (200, 0)]


def _factor_bounds(Sysf, M, Bc, D, K):
    L = torch.tril(Sysf[:D, :D])
    g = 2.0 * gamma(D + 2, 2.0 ** -53)
    low = torch.tril(torch.ones(D, D, dtype=torch.bool))
    assert bool((((L @ L.T - M).abs() <= g * (L.abs() @ L.abs().T)) | ~low).all())
    if K:
        Yt = Sysf[D:D + K, :D]
        assert bool(((Yt @ L.T - Bc.T).abs() <= g * (Yt.abs() @ L.abs().T)).all())
    return L


@pytest.mark.parametrize("D,K", SHAPES)
@pytest.mark.parametrize("batch", [1, 7])
def test_cholesky_and_solve_within_highams_bounds(cuda, D, K, batch):
    Sys, M, Bc = spd_batch(D, K, batch)
    bad = 3 if batch == 7 else None
    col = min(5, D - 1)
    S2 = Sys.clone()
    if bad is not None:
        S2[bad, col, col] = -1.0                                             # indefinite: the pivot of column col
    dS = S2.to(cuda)
    info = RD.cholesky_native(dS, D, K)
    out = dS.cpu()
    assert info.tolist() == [col + 1 if s == bad else 0 for s in range(batch)]
    assert not bool(out[:, :, D:].any()) and not bool(out[:, D + K:].any())   # nothing outside the bordered image
    Ls = {}
    for s in range(batch):
        if s != bad:
            assert not bool(torch.triu(out[s, :D, :D], 1).any())
            Ls[s] = _factor_bounds(out[s], M[s], Bc[s], D, K)
    if bad is not None:                                                      # the other six are unaffected
        dS0 = Sys.to(cuda)
        RD.cholesky_native(dS0, D, K)
        ref = dS0.cpu()
        for s in Ls:
            assert torch.equal(out[s], ref[s])
    if K == 0:
        return
    W64, W = RD.backsolve_native(dS, D, K, info)
    W64, W = W64.cpu(), W.cpu()
    g = 2.0 * gamma(3 * D + 1, 2.0 ** -53)
    for s in range(batch):
        if s == bad:
            assert not bool(W64[s].any()) and not bool(W[s].any())           # a failed system: W = 0
            continue
        Wd = W64[s, :, :D].T                                                 # [D, K] before the fp32 rounding
        L = Ls[s]
        assert bool(((M[s] @ Wd - Bc[s]).abs() <= g * (L.abs() @ L.abs().T @ Wd.abs())).all())
        assert torch.equal(W[s], W64[s, :, :D].float()) and not bool(W64[s, :, D:].any())


# ------------------------------------------------------------------ 5. fit end to end
@pytest.mark.parametrize("D", FIT_CASES)
def test_fit_end_to_end(cuda, D):
    """Tolerance: 10 x the difference of the fp64 oracle and the oracle on chunked fp32 chains (measured 1.0e-6 at
    D = 43, 6.5e-7 at D = 130; PARITY.md).  On the MI355X the fit's W and b differ from the fp64 oracle by 1.0e-7
    / 6.0e-8 (D = 43) and 6.5e-8 / 6.0e-8 (D = 130), with no mismatching row."""
    c = fit_case(D)
    o = c["o64"]
    X = c["X"].to(cuda)
    r = RD.fit_native(X, c["y"].to(cuda), c["fold"], c["F"], list(FIT_ALPHAS), c["mean"], c["inv_std"], c["K"],
                      keep_w64=True)
    errW = float((r.W64.cpu() - o.W64).abs().max())
    errb = float((r.b_all.cpu().double() - o.b_all.double()).abs().max())
    ex = excluded_rows(c)
    mism = (r.fold_pred.cpu() != o.fold_pred) & ~ex
    print(f"D = {D}: |W - oracle| {errW:.3e}, |b - oracle| {errb:.3e}, tolerance {c['tol']:.3e}; excluded "
          f"{int(ex.sum())}, mismatching {int(mism.sum())}; cvCorrect {r.cvCorrect} (oracle {o.cvCorrect})")
    assert r.info == [0] * len(o.info)
    assert errW <= c["tol"] and errb <= c["tol"]
    assert float(ex.double().mean()) <= EXCLUDED_CAP
    assert int(mism.sum()) == 0
    assert r.chosen == o.chosen and r.alpha == o.alpha


# ------------------------------------------------------------------ 6. batching, reproducibility, no host read
def test_workspace_batching_and_reproducibility(cuda):
    c = fit_case(43)
    X, y = c["X"].to(cuda), c["y"].to(cuda)
    args = (X, y, c["fold"], c["F"], list(FIT_ALPHAS), c["mean"], c["inv_std"], c["K"])
    a = RD.fit_native(*args, keep_w64=True)
    b = RD.fit_native(*args, keep_w64=True)
    ldn = RD.up64(43 + 6)
    small = RD.fit_native(*args, workspace_bytes=2 * ldn * ldn * 8, keep_w64=True)   # two systems at a time
    for other in (b, small):
        assert torch.equal(a.W_all, other.W_all) and torch.equal(a.b_all, other.b_all) and torch.equal(a.W64, other.W64)
        assert torch.equal(a.Wx, other.Wx) and torch.equal(a.bx, other.bx) and torch.equal(a.fold_pred, other.fold_pred)
        assert (a.chosen, a.cvCorrect, a.info) == (other.chosen, other.cvCorrect, other.info)
    p = RD.prepare_native(X, y, c["fold"], c["F"], list(FIT_ALPHAS), c["mean"], c["inv_std"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # a synchronizing call (any device -> host read) raises
    try:
        r = RD.fit_device(X, p, c["K"], workspace_bytes=2 * ldn * ldn * 8)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(r["packed"][0]) == a.chosen and torch.equal(r["W"], a.W_all)


def test_range_is_refused_before_any_launch(cuda):
    X = torch.zeros(4, 3, device=cuda)
    y = torch.zeros(4, dtype=torch.int64, device=cuda)
    one = torch.ones(3)
    for kw in (dict(F=17, alphas=[1.0], K=2), dict(F=1, alphas=[1.0] * 17, K=2), dict(F=1, alphas=[1.0], K=33),
               dict(F=1, alphas=[0.0], K=2)):
        with pytest.raises(ValueError):
            RD.fit_native(X, y, np.zeros(4, dtype=np.int64), kw["F"], kw["alphas"], one, one, kw["K"])


# ------------------------------------------------------------------ 7. serving and persistence
def test_serving_and_persistence(cuda, tmp_path):
    c = fit_case(43)
    est = RidgeClassifier(alphas=list(FIT_ALPHAS), numFolds=5, seed=1)
    m = est.fit_tensors(c["X"].to(cuda), c["y"].to(cuda), c["K"])
    assert m.device.type == "cuda" and m.summary.info == [0] * 24 and m.alpha in FIT_ALPHAS
    Xq = c["X"][:777].to(cuda)
    raw, prob, pred = m.predict_all(Xq)
    assert raw.shape == (777, 6) and torch.equal(pred, RD.first_argmax(raw)) and torch.equal(pred, raw.argmax(dim=1))
    # the fixture's classes overlap on purpose (held-out accuracy 0.63 at D = 43, chance 1 / 6)
    assert float((pred.cpu() == c["y"][:777]).double().mean()) > 0.5
    cpu = RidgeClassificationModel(m.Wx.cpu(), m.bx.cpu(), m.alpha, device="cpu")
    assert float((cpu.predict_raw(c["X"][:777]) - raw.cpu()).abs().max()) < 1e-4
    persist.save(m, str(tmp_path / "ridge"))
    r = persist.load(str(tmp_path / "ridge"), device=cuda)
    assert isinstance(r, RidgeClassificationModel) and r.summary == m.summary
    assert torch.equal(r.predict_raw(Xq), raw)
