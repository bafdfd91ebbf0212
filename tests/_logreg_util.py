"""fp64 oracles and problem builders for the direct tests of the logistic-regression kernels
(csrc/kernels/logreg_qn.hip: evaluation, gradient, column slices, loss decode; csrc/kernels/logreg_setup.hip:
summarizer and prepare), in plain torch / numpy / Python on the CPU.

Everything here starts from the DENSE fp32 design matrix ``X [N, F]``: the one-hot blocks occupy the
first columns, the ``Fd`` dense columns the last ones.  The hybrid layout the kernels read is derived
from it with ``features.hybrid.from_dense`` only at the very end, so no oracle depends on the hybrid
index code (CSC row lists, column map, slices, blocks) it is there to check.

* ``make_problem``: labels, one-hot categories (rows without a category, forced popular / empty
  categories, Zipf-like popularity), dense columns (optionally one constant column) and row weights.
* ``oracle_eval``: the objective of ``LogregDesign.eval_torch`` — margins, shifted log-sum-exp, weighted
  mean cross entropy, residual rows, masked and scaled gradient — written again from the dense matrix.
* ``oracle_summary`` / ``oracle_prepare``: the weighted summarizer row and Spark's setup (unbiased
  weighted variance with the ``max(wsum - 1, 1)`` divisor, frozen zero-variance columns, binomial pivot
  row, unregularized intercept, ``log1p`` centred priors or the class-1 logit).
* ``oracle_col_slices`` / ``oracle_col_blocks_ok``: the integer slice scan and the invariants of the
  gradient kernel's column blocks.
* ``loss_fx_encode`` / ``loss_fx_decode``: the 2^-40 fixed-point loss transport in Python integers.
"""
from types import SimpleNamespace

import numpy as np
import torch

f64, f32 = torch.float64, torch.float32
CONST_VALUE = 2.0  # value of the constant dense column, see make_problem


# ------------------------------------------------------------------------------------------ builder
def make_problem(N, K, block_widths, Fd, seed, *, popular=None, empty=(), weights="none", S=1, zipf=None,
                 const_dense=None, device="cpu"):
    """A labelled design of ``N`` rows, ``K`` classes, one one-hot block per entry of ``block_widths``
    (columns first) and ``Fd`` dense columns (columns last).

    ``popular={block: (category, share)}`` gives that category about ``share`` of the rows;
    ``empty=[(block, category), ...]`` lists categories no row takes (their rows hold no category
    instead); ``zipf=a`` draws every block's categories with probability ~ 1 / (c + 1)^a.  Otherwise a
    row's category is uniform over the block's ``w`` categories and "none" (``-1``), half the rows
    correlated with the label.  Row 0 holds no category in any block.
    ``const_dense=j`` sets dense column ``j`` to ``CONST_VALUE`` = 2: a power of two, so that every
    fp64 partial sum of ``w x`` and ``w x^2`` is exactly 2 or 4 times the matching partial sum of ``w``
    (scaling by a power of two commutes with rounding) and the variance of the column is EXACTLY zero
    for any weights, as long as a summarizer adds ``w``, ``w x`` and ``w x^2`` in the same order.
    ``weights``: ``"none"`` (``rw`` is None), ``"binary"`` (0/1, about a quarter zeros) or ``"frac"``
    (uniform in (0, 2) with about 20 % exact zeros), ``[S, N]`` fp32; a spec whose weights would all be
    zero gets weight 1 on row 0.

    Returns a namespace: ``X`` fp32 ``[N, F]``, ``y`` int64, ``rw`` (or None), ``cat`` ``[N, C]`` (the
    block-local category or -1), ``blocks`` ``[(offset, width)]``, ``F``, ``Fd``, ``C``, ``K``, ``N`` and
    ``hm``, the HybridMatrix of ``X`` on ``device``."""
    from har.features.hybrid import from_dense

    g = torch.Generator().manual_seed(seed)
    popular = dict(popular or {})
    blocks, off = [], 0
    for w in block_widths:
        blocks.append((off, int(w)))
        off += int(w)
    F = off + Fd
    X = torch.zeros(N, F)
    y = torch.randint(0, K, (N,), generator=g)
    cat = torch.full((N, len(blocks)), -1, dtype=torch.int64)
    for bi, (o, w) in enumerate(blocks):
        if zipf is not None:
            p = 1.0 / torch.arange(1, w + 1, dtype=f64) ** float(zipf)
            idx = torch.multinomial(p / p.sum(), N, replacement=True, generator=g)
        else:
            idx = torch.randint(0, w + 1, (N,), generator=g)              # w == no category
            idx = torch.where(torch.rand(N, generator=g) < 0.5, (y * 7) % (w + 1), idx)
        if bi in popular:
            pc, share = popular[bi]
            idx = torch.where(torch.rand(N, generator=g) < share, torch.full_like(idx, int(pc)), idx)
        for eb, ec in empty:
            if eb == bi:
                idx = torch.where(idx == int(ec), torch.full_like(idx, w), idx)
        if N:
            idx[0] = w
        ok = idx < w
        cat[:, bi] = torch.where(ok, idx, torch.full_like(idx, -1))
        X[torch.nonzero(ok).squeeze(1), o + idx[ok]] = 1.0
    if Fd:
        X[:, F - Fd:] = torch.randn(N, Fd, generator=g) + y[:, None].float() * 0.3
        if const_dense is not None:
            X[:, F - Fd + int(const_dense)] = CONST_VALUE
    if weights == "none":
        rw = None
    else:
        if weights == "binary":
            rw = (torch.rand(S, N, generator=g) > 0.25).float()
        elif weights == "frac":
            rw = torch.rand(S, N, generator=g) * 2.0
            rw = torch.where(rw == 0, torch.ones_like(rw), rw)
            rw = torch.where(torch.rand(S, N, generator=g) < 0.2, torch.zeros_like(rw), rw)
        else:
            raise ValueError(f"weights must be none, binary or frac, got {weights!r}")
        dead = rw.sum(1) == 0
        rw[dead, 0] = 1.0
    hm = from_dense(X.to(device), blocks)
    assert hm is not None and hm.cat.shape[1] == len(blocks) and hm.dense.shape[1] == Fd
    return SimpleNamespace(X=X, y=y, rw=rw, cat=cat, blocks=blocks, F=F, Fd=Fd, C=len(blocks), K=K, N=N, hm=hm)


# ------------------------------------------------------------------------------------------ objective
def oracle_eval(X, y, rw, xt, T, inv_std, pmask, inv_wsum, dtype=f64):
    """The data objective of ``S * T`` trial points ``xt [S*T, K, F+1]`` (last column: intercepts) over
    the dense ``X [N, F]``: model ``bt`` belongs to spec ``bt // T`` (row weights ``rw[s]`` or ones,
    ``inv_std[s]``, ``pmask[s]``, ``inv_wsum[s]``).  Returns ``loss [BT]``, ``G [BT, K*(F+1)]`` (masked,
    scaled by inv_std), the raw margins ``Z [BT, N, K]`` and the residual rows ``R [BT, N, K]``.
    ``dtype=torch.float32`` runs the same lines in fp32 (the measured error scale of two tests)."""
    X = X.to(dtype)
    N, F = X.shape
    BT, K = xt.shape[0], xt.shape[1]
    rows = torch.arange(N)
    y = y.long()
    loss, G, Zs, Rs = [], [], [], []
    for bt in range(BT):
        s = bt // T
        istd, pm = inv_std[s].to(dtype), pmask[s].to(dtype)
        W = xt[bt, :, :F].to(dtype) * istd[None, :] * pm[:, :F]
        b = xt[bt, :, F].to(dtype) * pm[:, F]
        Z = X @ W.T + b[None, :]                                        # margins [N, K]
        m = Z.max(dim=1).values
        lse = m + torch.log(torch.exp(Z - m[:, None]).sum(dim=1))       # shifted log-sum-exp
        w = (torch.ones(N, dtype=dtype) if rw is None else rw[s].to(dtype)) * inv_wsum[s].to(dtype)
        loss.append((w * (lse - Z[rows, y])).sum())
        P = torch.exp(Z - lse[:, None])
        P[rows, y] -= 1.0
        R = w[:, None] * P                                              # residual rows [N, K]
        g = torch.cat([(R.T @ X) * istd[None, :], R.sum(dim=0)[:, None]], dim=1) * pm
        G.append(g.reshape(-1))
        Zs.append(Z)
        Rs.append(R)
    return SimpleNamespace(loss=torch.stack(loss), G=torch.stack(G), Z=torch.stack(Zs), R=torch.stack(Rs))


# ------------------------------------------------------------------------------------------ setup
def oracle_summary(X, y, rw, K):
    """``[S, 1 + 2F + K]`` fp64: sum w, sum w x, sum w x^2 per column, weighted class counts (``rw``
    None: one row of an unweighted design).  The weight sum is taken as the column of ones of the same
    reduction as the feature columns, so all of them add their rows in one order (see make_problem)."""
    X = X.to(f64)
    N, F = X.shape
    rwd = torch.ones(1, N, dtype=f64) if rw is None else rw.to(f64)
    M = torch.cat([torch.ones(N, 1, dtype=f64), X, X * X,
                   torch.nn.functional.one_hot(y.long(), K).to(f64)], dim=1)        # [N, 1 + 2F + K]
    return (rwd[:, :, None] * M[None, :, :]).sum(dim=1)


def oracle_prepare(summary, reg, alpha, Kp, K, standardization, fit_intercept, binomial):
    """Spark's LogisticRegression setup from the summary rows ``[B, 1 + 2F + K]``, in fp64:
    ``inv_std [B, F]``, ``inv_wsum [B]``, ``pmask [B, Kp, F+1]``, ``l2 [B, Kp*(F+1)]``, ``l1`` (same
    shape), ``x0 [B, Kp, F+1]``."""
    summary = summary.to(f64)
    B = summary.shape[0]
    F = (summary.shape[1] - 1 - K) // 2
    reg = torch.as_tensor(reg, dtype=f64).reshape(B)
    alpha = torch.as_tensor(alpha, dtype=f64).reshape(B)
    wsum = summary[:, 0]
    mean = summary[:, 1:1 + F] / wsum[:, None]
    ex2 = summary[:, 1 + F:1 + 2 * F] / wsum[:, None]
    counts = summary[:, 1 + 2 * F:]
    var = (ex2 - mean * mean) * (wsum / torch.clamp(wsum - 1.0, min=1.0))[:, None]   # unbiased, weighted
    sd = torch.sqrt(torch.clamp(var, min=0.0))
    live = sd > 0
    safe = torch.where(live, sd, torch.ones_like(sd))
    inv_std = torch.where(live, 1.0 / safe if standardization else torch.ones_like(sd), torch.zeros_like(sd))
    pmask = torch.ones(B, Kp, F + 1, dtype=f64)
    pmask[:, :, :F] = live.to(f64)[:, None, :]          # a zero-variance column is frozen at 0
    if not fit_intercept:
        pmask[:, :, F] = 0
    if binomial:
        pmask[:, 0, :] = 0                              # pivot: the class-0 row stays 0
    notb = torch.ones(F + 1, dtype=f64)
    notb[F] = 0                                         # the intercept is never regularized
    l2 = ((reg * (1 - alpha))[:, None, None] * pmask * notb).reshape(B, -1)
    l1 = ((reg * alpha)[:, None, None] * pmask * notb).reshape(B, -1)
    x0 = torch.zeros(B, Kp, F + 1, dtype=f64)
    if fit_intercept:
        if binomial:
            p1 = torch.clamp(counts[:, 1] / counts.sum(dim=1), 1e-12, 1 - 1e-12)
            x0[:, 1, F] = torch.log(p1 / (1 - p1))
        else:
            raw = torch.log1p(counts)
            x0[:, :, F] = raw[:, :Kp] - raw.sum(dim=1, keepdim=True) / Kp
    return inv_std, 1.0 / wsum, pmask, l2, l1, x0 * pmask


# ------------------------------------------------------------------------------------------ slices
def oracle_col_slices(csc_off, SL):
    """Exclusive scan over the F + 1 columns of ceil(rows / SL): ``[F + 2]`` int64."""
    off = np.asarray(csc_off, dtype=np.int64)
    n = (off[1:] - off[:-1] + SL - 1) // SL
    out = np.zeros(off.shape[0], dtype=np.int64)
    out[1:] = np.cumsum(n)
    return out


def oracle_col_blocks_ok(blk, srow, col_slice, csc_off, SL):
    """The invariants of ``LogregDesign.col_blocks()`` (raises AssertionError naming the broken one):
    the blocks partition the columns [0, F + 1) in order; each holds at most 256 columns, and at most
    256 slices unless it is a single column; its slice range is its columns' range of ``col_slice``;
    ``srow`` is non-decreasing, slice j of column c starts at ``csc_off[c] + j * SL`` and the last entry
    is ``csc_off[F + 1]``."""
    blk = np.asarray(blk, dtype=np.int64).reshape(-1, 4)
    srow = np.asarray(srow, dtype=np.int64)
    cs = np.asarray(col_slice, dtype=np.int64)
    off = np.asarray(csc_off, dtype=np.int64)
    F1 = off.shape[0] - 1
    assert np.array_equal(cs[:F1 + 1], oracle_col_slices(off, SL)[:F1 + 1]), "col_slice is not the slice scan"
    assert blk.shape[0] >= 1 and blk[0, 0] == 0 and blk[-1, 1] == F1, "blocks do not span [0, F + 1)"
    for i, (c0, c1, s0, s1) in enumerate(blk):
        assert c0 < c1, f"block {i} is empty"
        if i:
            assert c0 == blk[i - 1, 1], f"block {i} does not start where block {i - 1} ends"
        assert c1 - c0 <= 256, f"block {i} has {c1 - c0} columns"
        assert (s0, s1) == (cs[c0], cs[c1]), f"block {i}: slice range is not its columns' range"
        assert s1 - s0 <= 256 or c1 - c0 == 1, f"block {i} has {s1 - s0} slices over {c1 - c0} columns"
    total = int(cs[F1])
    assert srow.shape[0] == total + 1, "srow length is not slices + 1"
    assert np.all(srow[1:] >= srow[:-1]), "srow decreases"
    ns = cs[1:F1 + 1] - cs[:F1]
    col_of = np.repeat(np.arange(F1), ns)
    j = np.arange(total) - cs[col_of]
    assert np.array_equal(srow[:total], off[col_of] + j * SL), "a slice does not start at csc_off[c] + j SL"
    assert srow[total] == off[F1], "srow does not end at csc_off[F + 1]"
    return True


# ------------------------------------------------------------------------------------------ loss fixed point
LOSS_FX_ONE = 1 << 40
LOSS_FX_LIMIT = float(1 << 23)


def loss_fx_encode(l):
    """A loss as 2^-40 fixed point in four 16-bit pieces (three unsigned, the top one signed) and a
    flag: ``[p0, p1, p2, p3, flag]`` as Python floats holding integers.  ``!(|l| < 2^23)`` (too large,
    infinite or NaN) gives ``[0, 0, 0, 0, 1]``.  Rounding: to nearest, ties to even."""
    l = float(l)
    if not abs(l) < LOSS_FX_LIMIT:
        return [0.0, 0.0, 0.0, 0.0, 1.0]
    q = round(l * LOSS_FX_ONE)      # exact product (a power of two), Python rounds half to even
    return [float(q & 0xffff), float((q >> 16) & 0xffff), float((q >> 32) & 0xffff), float(q >> 48), 0.0]


def loss_fx_decode(p):
    """The value of (a sum of) encoded rows: NaN when the flag piece is non-zero."""
    if p[4] != 0:
        return float("nan")
    q = int(p[0]) + (int(p[1]) << 16) + (int(p[2]) << 32) + (int(p[3]) << 48)
    return q / LOSS_FX_ONE
