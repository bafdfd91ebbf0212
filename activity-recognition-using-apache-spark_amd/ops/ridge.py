"""Ridge classification from Gram moments with one-pass k-fold selection of the penalty: every operation
defined ONCE here as PyTorch code.

That code is the CPU path and the fp64 oracle of the HIP kernels in ``csrc/kernels/ridge.hip``; the ``*_native``
front-ends launch the kernels, and ``fit`` dispatches on the rows' device (a GPU tensor REQUIRES the kernels).

Working rows.  ``z = fl32(fl32(x - mean) * inv_std)``: two fp32 roundings, no contraction, so torch on the CPU
reproduces the kernel's staging bit for bit.  ``mean`` and ``inv_std = fl32(1 / std)`` are the whole table's (fp64
sums, population std; a constant column, or ``standardize=False``, keeps scale 1).  Only features enter them.

Targets are one-vs-rest, ``T[n, c] = +1`` when ``y[n] == c`` else ``-1``; the augmented row is ``a = [z | T | 1]``
with ``Dq = D + K + 1`` columns.

Moments.  ``A_f = sum over fold f's rows of a a^T`` holds ``G_f``, ``B_f = Z_f^T T_f``, the column sums and the
count.  Its defined value: the fold's rows in table order, cut into chunks of ``R`` rows from the fold's start;
every chunk entry is a row-ordered fp32 fma chain from zero; the chunk results are added in fp64 in ascending
order; ``A_all`` adds the folds in ascending order.  ``moments_torch(..., chain="fp64")`` evaluates the same sums
in fp64 throughout (the reference of the error bound).

Systems.  For fold f the training part is every other fold, for the final model everything: with ``u = A_all -
A_f`` entrywise (``u = A_all`` for the final model), ``q = D + K`` the column of ones and ``n = u[q, q]``,

    entry(r, c) = (u[c, r] - (u[c, q] * u[r, q]) / n)  (+ alpha when r == c),

one rounding per operation in exactly this order (the quotient is 0 when ``n == 0``).  Rows ``r < D`` are ``M =
G - s s^T / n + alpha I``, rows ``D .. D + K - 1`` the border ``Bc^T``.  ``W = M^-1 Bc`` by Cholesky in fp64, the
unpenalised intercept ``b = (t - W^T s) / n`` (exact by the centring identity).  ``alpha > 0`` is required, so M
is positive definite for any N and D.  System ``s`` of the ``(F + 1) * len(alphas)`` (``len(alphas)`` when ``F ==
1``) is fold ``s // len(alphas)`` (the last one: all rows) at ``alphas[s % len(alphas)]``.

Selection.  Model (f, alpha) scores fold f's rows; the alpha with the largest summed correct count wins, ties
go to the larger alpha; the final model is the all-rows system at that alpha.  Without folds (``F == 1``) nothing
is scored, every count is 0, and the same rule takes the largest alpha.

Prediction.  ``raw = z W + b``, prediction = the first argmax, ``probability = softmax(raw)`` (uncalibrated; it
exists so that HMMSmoother can consume it).  ``fold_standardization`` folds mean and scale into the weights
once, so serving is one product on the raw rows.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _native

R = 256                 # ridge.hip RG_R: rows of one fp32 chain
PANEL = 64              # ridge.hip RS_PANEL: columns of one Cholesky panel
MAX_DIM = 10240         # D + K + 1
MIN_CLASSES, MAX_CLASSES = 2, 32
MAX_FOLDS = 16
MAX_ALPHAS = 16
MAX_ROWS = (1 << 31) - 256
WORKSPACE_BYTES = 4 << 30
_TARGET_GROUPS = 2048   # workgroups ridge_gram aims at when it splits the folds' chunk lists


def default_alphas() -> List[float]:
    return [float(v) for v in np.logspace(-3, 3, 10)]


def check_range(D: int, K: int, F: int = 1, alphas: Optional[Sequence[float]] = None, N: Optional[int] = None):
    if int(D) < 1 or int(D) + int(K) + 1 > MAX_DIM:
        raise ValueError(f"ridge takes D >= 1 with D + K + 1 <= {MAX_DIM}, got D = {D}, K = {K}")
    if not MIN_CLASSES <= int(K) <= MAX_CLASSES:
        raise ValueError(f"ridge takes {MIN_CLASSES}..{MAX_CLASSES} classes, got {K}")
    if not 1 <= int(F) <= MAX_FOLDS:
        raise ValueError(f"ridge takes 1..{MAX_FOLDS} folds, got {F}")
    if alphas is not None:
        if not 1 <= len(alphas) <= MAX_ALPHAS:
            raise ValueError(f"ridge takes 1..{MAX_ALPHAS} alphas, got {len(alphas)}")
        if not all(np.isfinite(float(v)) and float(v) > 0 for v in alphas):
            raise ValueError(f"ridge alphas must be positive and finite, got {list(alphas)}")
    if N is not None and not 1 <= int(N) <= MAX_ROWS:
        raise ValueError(f"ridge takes 1..{MAX_ROWS} rows, got {N}")


def up64(v: int) -> int:
    return (int(v) + 63) // 64 * 64


def num_systems(F: int, nalpha: int) -> int:
    return (F + 1 if F > 1 else 1) * nalpha


# ------------------------------------------------------------------ working rows
def standardizer(X: torch.Tensor, standardize: bool = True):
    """(mean, inv_std) fp32 [D] of the whole table from fp64 sums."""
    xd = X.double()
    n = max(X.shape[0], 1)
    mean = xd.sum(dim=0) / n
    if not standardize:
        return mean.float(), torch.ones_like(mean, dtype=torch.float32)
    sd = (((xd - mean.view(1, -1)) ** 2).sum(dim=0) / n).sqrt()
    sd = torch.where((sd > 0) & torch.isfinite(sd), sd, torch.ones_like(sd))
    return mean.float(), (1.0 / sd).float()


def working_rows(X: torch.Tensor, mean: torch.Tensor, inv_std: torch.Tensor) -> torch.Tensor:
    return ((X.float() - mean.float().view(1, -1)) * inv_std.float().view(1, -1)).contiguous()


def augment(Z: torch.Tensor, y: torch.Tensor, K: int) -> torch.Tensor:
    """fp32 [N, D + K + 1]: [z | T | 1]."""
    N = Z.shape[0]
    T = torch.where(y.long().view(-1, 1) == torch.arange(K, device=Z.device).view(1, -1), 1.0, -1.0).float()
    return torch.cat([Z.float(), T, torch.ones(N, 1, dtype=torch.float32, device=Z.device)], dim=1)


def fold_order(fold, F: int):
    """(rows int32 [N] grouped by fold in table order, offsets: F + 1 python ints) from host fold ids."""
    fold = np.asarray(fold.cpu() if isinstance(fold, torch.Tensor) else fold).astype(np.int64)
    if fold.size and (fold.min() < 0 or fold.max() >= F):
        raise ValueError(f"ridge fold ids must lie in [0, {F})")
    order = np.argsort(fold, kind="stable").astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(fold, minlength=F))]).astype(np.int64)
    return torch.from_numpy(order), [int(v) for v in off]


# ------------------------------------------------------------------ 1. moments
def _fma32(acc: torch.Tensor, prod64: torch.Tensor) -> torch.Tensor:
    """fl32(acc + p) for fp32 ``acc`` and an fp64 ``p`` that is an exact product of two fp32 values: the fp64 sum
    rounded to odd (TwoSum), then to fp32 — a correctly rounded fmaf."""
    a = acc.double()
    s = a + prod64
    bb = s - a
    err = (a - (s - bb)) + (prod64 - bb)
    bits = s.view(torch.int64)
    fix = (err != 0) & ((bits & 1) == 0) & torch.isfinite(s)
    toward = torch.where(err > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    s = torch.where(fix, torch.nextafter(s, toward), s)
    return s.float()


def _chain_chunks(A: torch.Tensor) -> torch.Tensor:
    """fp64 [Dq, Dq]: the chunked fp32 chains of one fold's augmented rows (table order)."""
    n, Dq = A.shape
    out = torch.zeros(Dq, Dq, dtype=torch.float64)
    if n == 0:
        return out
    nch = -(-n // R)
    pad = torch.zeros(nch * R, Dq, dtype=torch.float32)
    pad[:n] = A
    pad = pad.view(nch, R, Dq).double()
    acc = torch.zeros(nch, Dq, Dq, dtype=torch.float32)
    for r in range(R):   # every chunk advances its chains by one row
        v = pad[:, r, :]
        acc = _fma32(acc, v.unsqueeze(2) * v.unsqueeze(1))
    for c in range(nch):
        out = out + acc[c].double()
    return out


def moments_torch(X, y, rows, off, mean, inv_std, K: int, chain: str = "fp32"):
    """(A_f fp64 [F, Dq, Dq], A_all fp64 [Dq, Dq]), full symmetric matrices.  ``chain="fp32"``: the defined value;
    ``"fp64"``: the same sums of the same fp32 rows in fp64."""
    F = len(off) - 1
    A = augment(working_rows(X.cpu(), mean.cpu(), inv_std.cpu()), y.cpu(), K)
    Dq = A.shape[1]
    Af = torch.zeros(F, Dq, Dq, dtype=torch.float64)
    rows = rows.cpu().long()
    for f in range(F):
        Ar = A[rows[off[f]:off[f + 1]]]
        if chain == "fp32":
            Af[f] = _chain_chunks(Ar)
        else:
            Ad = Ar.double()
            Af[f] = Ad.T @ Ad
    Aall = torch.zeros(Dq, Dq, dtype=torch.float64)
    for f in range(F):
        Aall = Aall + Af[f]
    return Af, Aall


def auto_chunks_per_group(off: Sequence[int], Dq: int) -> int:
    """Chunks one ``ridge_gram`` workgroup takes: from the shapes alone."""
    nt = up64(Dq) // 64
    pairs = nt * (nt + 1) // 2
    chunks = sum(-(-(off[f + 1] - off[f]) // R) for f in range(len(off) - 1))
    return max(1, -(-chunks * pairs // _TARGET_GROUPS))


def moments_native(X, y, rows, off, mean, inv_std, K: int, chunks_per_group: Optional[int] = None):
    """``ridge_gram`` + ``ridge_gram_reduce``: (A_f fp64 [F, ldq, ldq] or None when F == 1, A_all fp64 [ldq, ldq]);
    entries i <= j are written, the rest is zero."""
    N, D = X.shape
    F = len(off) - 1
    check_range(D, K, F, N=N)
    if X.dtype != torch.float32 or X.stride(1) != 1 or y.dtype != torch.int32 or not y.is_contiguous() or \
            rows.dtype != torch.int32 or not rows.is_contiguous() or rows.numel() != off[-1] or y.numel() != N:
        raise ValueError("ridge moments: X fp32 [N, D] with unit column stride, y int32 [N], rows int32 [off[-1]]")
    for t in (mean, inv_std):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != D:
            raise ValueError("ridge moments: mean / inv_std fp32 [D]")
    Dq = D + K + 1
    ldq = up64(Dq)
    cps = auto_chunks_per_group(off, Dq) if chunks_per_group is None else int(chunks_per_group)
    if cps < 1:
        raise ValueError("ridge moments: chunks_per_group >= 1")
    nt = ldq // 64
    pairs = nt * (nt + 1) // 2
    smax = max(1, max(-(-(-(-(off[f + 1] - off[f]) // R)) // cps) for f in range(F)))
    dev = X.device
    slabs = torch.empty(F * smax * pairs * 4096, dtype=torch.float64, device=dev)
    Af = torch.zeros(F, ldq, ldq, dtype=torch.float64, device=dev) if F > 1 else None
    Aall = torch.zeros(ldq, ldq, dtype=torch.float64, device=dev)
    mod, st = _native.kernels(), _native.stream_ptr()
    args = (X.data_ptr(), X.stride(0), y.data_ptr(), rows.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), list(off), D,
            K, cps, slabs.data_ptr(), _native.ptr(Af), Aall.data_ptr())
    mod.ridge_gram(*args, False, st)
    mod.ridge_gram(*args, True, st)
    return Af, Aall


# ------------------------------------------------------------------ 2. systems, factorisation, solve
def systems_torch(Af, Aall, alphas, D: int, K: int) -> torch.Tensor:
    """fp64 [S, D + K, D + K]: rows < D the lower triangle of M, rows D.. the border Bc^T, the rest zero."""
    F = 1 if Af is None else Af.shape[0]
    A = len(alphas)
    n2, q = D + K, D + K
    out = torch.zeros(num_systems(F, A), n2, n2, dtype=torch.float64)
    mask = torch.tril(torch.ones(n2, n2, dtype=torch.bool))
    mask[:, D:] = False
    for s in range(out.shape[0]):
        fi, ai = divmod(s, A)
        u = Aall if (F == 1 or fi == F) else Aall - Af[fi]
        u = torch.triu(u) + torch.triu(u, 1).T         # the kernels read the upper triangle
        n = u[q, q]
        sq = u[:n2, q]
        ct = (sq.view(-1, 1) * sq.view(1, -1)) / n if n > 0 else torch.zeros(n2, n2, dtype=torch.float64)
        m = u[:n2, :n2] - ct
        m = m + torch.diag(torch.full((n2,), float(alphas[ai]), dtype=torch.float64))
        out[s] = torch.where(mask, m, torch.zeros_like(m))
    return out


def solve_torch(Sys: torch.Tensor, D: int, K: int, Aall=None, Af=None, nalpha: int = 1):
    """(W fp64 [S, K, D], b fp64 [S, K] or None without moments, info int32 [S]) by torch's Cholesky."""
    S = Sys.shape[0]
    W = torch.zeros(S, K, D, dtype=torch.float64)
    b = torch.zeros(S, K, dtype=torch.float64) if Aall is not None else None
    info = torch.zeros(S, dtype=torch.int32)
    F = 1 if Af is None else Af.shape[0]
    q = D + K
    for s in range(S):
        M = torch.tril(Sys[s, :D, :D])
        M = M + torch.tril(M, -1).T
        L, fl = torch.linalg.cholesky_ex(M)
        info[s] = int(fl)
        if int(fl) != 0:
            continue
        W[s] = torch.cholesky_solve(Sys[s, D:D + K, :D].T.contiguous(), L).T
        if b is not None:
            fi = s // nalpha
            u = Aall if (F == 1 or fi == F) else Aall - Af[fi]
            u = torch.triu(u) + torch.triu(u, 1).T
            n = u[q, q]
            b[s] = (u[D:D + K, q] - W[s] @ u[:D, q]) / n if n > 0 else 0.0
    return W, b, info


def _solve_args(Af, Aall, alphas_t, D, K, F, nalpha, s0, ns, Sys, info, W64, W, b):
    return (_native.ptr(Af), _native.ptr(Aall), _native.ptr(alphas_t), D, K, F, nalpha, s0, ns, Sys.data_ptr(),
            info.data_ptr(), _native.ptr(W64), _native.ptr(W), _native.ptr(b), _native.stream_ptr())


def cholesky_native(Sys: torch.Tensor, D: int, K: int, info: Optional[torch.Tensor] = None):
    """Factor a batch [S, ldn, ldn] (ldn = D + K rounded up to 64, rows D.. the border) in place; returns info."""
    S, ldn = Sys.shape[0], up64(D + K)
    if Sys.dtype != torch.float64 or not Sys.is_contiguous() or tuple(Sys.shape) != (S, ldn, ldn) or \
            not 1 <= S <= MAX_ALPHAS:
        raise ValueError(f"ridge cholesky: fp64 [1..{MAX_ALPHAS}, {ldn}, {ldn}], contiguous")
    info = torch.zeros(S, dtype=torch.int32, device=Sys.device) if info is None else info
    _native.kernels().ridge_solve(1, *_solve_args(None, None, None, D, K, 1, S, 0, S, Sys, info, None, None, None))
    return info


def backsolve_native(Sys: torch.Tensor, D: int, K: int, info: torch.Tensor):
    """(W64 [S, K, ldn], W fp32 [S, K, D]) from a factored batch."""
    S, ldn = Sys.shape[0], up64(D + K)
    if Sys.dtype != torch.float64 or not Sys.is_contiguous() or tuple(Sys.shape) != (S, ldn, ldn) or \
            not 1 <= S <= MAX_ALPHAS or K < 1:
        raise ValueError(f"ridge backsolve: fp64 [1..{MAX_ALPHAS}, {ldn}, {ldn}], contiguous, K >= 1")
    W64 = torch.empty(S, K, ldn, dtype=torch.float64, device=Sys.device)
    W = torch.empty(S, K, D, dtype=torch.float32, device=Sys.device)
    _native.kernels().ridge_solve(2, *_solve_args(None, None, None, D, K, 1, S, 0, S, Sys, info, W64, W, None))
    return W64, W


def systems_native(Af, Aall, alphas_t, D: int, K: int, s0: int, ns: int) -> torch.Tensor:
    F = 1 if Af is None else Af.shape[0]
    ldn = up64(D + K)
    Sys = torch.empty(ns, ldn, ldn, dtype=torch.float64, device=Aall.device)
    info = torch.zeros(num_systems(F, alphas_t.numel()), dtype=torch.int32, device=Aall.device)
    _native.kernels().ridge_solve(0, *_solve_args(Af, Aall, alphas_t, D, K, F, alphas_t.numel(), s0, ns, Sys, info,
                                                  None, None, None))
    return Sys


# ------------------------------------------------------------------ 3. scoring and selection
def fold_standardization(W: torch.Tensor, b: torch.Tensor, mean: torch.Tensor, inv_std: torch.Tensor):
    """(Wx fp32 [..., K, D], bx fp32 [..., K]) with ``x Wx^T + bx = z W^T + b`` up to rounding, from fp64."""
    Wd = W.double() * inv_std.double()
    return Wd.float(), (b.double() - (Wd * mean.double()).sum(dim=-1)).float()


def choose_alpha(correct: torch.Tensor, alphas_t: torch.Tensor) -> torch.Tensor:
    """Index (0-d int64) of the alpha with the largest count; ties go to the larger alpha."""
    A = alphas_t.numel()
    rank = torch.argsort(torch.argsort(alphas_t.double())).to(torch.int64)
    return torch.argmax(correct.to(torch.int64) * A + rank.to(correct.device))


def first_argmax(raw: torch.Tensor) -> torch.Tensor:
    K = raw.shape[-1]
    m = raw.max(dim=-1, keepdim=True).values
    idx = torch.arange(K, device=raw.device).expand_as(raw)
    return torch.where(raw == m, idx, torch.full_like(idx, K)).min(dim=-1).values.clamp_max(K - 1)


@dataclass
class RidgeFit:
    W: torch.Tensor           # fp32 [K, D]: the chosen model on the working rows
    b: torch.Tensor           # fp32 [K]
    Wx: torch.Tensor          # fp32 [K, D]: the same model on the raw rows
    bx: torch.Tensor          # fp32 [K]
    alpha: float
    chosen: int
    cvCorrect: List[int]      # per alpha
    info: List[int]           # per system
    W_all: torch.Tensor       # fp32 [S, K, D]
    b_all: torch.Tensor       # fp32 [S, K]
    fold_pred: Optional[torch.Tensor]   # int64 [N, len(alphas)]: every row under its own fold's models (F > 1)
    W64: Optional[torch.Tensor] = None  # fp64 [S, K, D]


def _finish(W_all, b_all, mean, inv_std, alphas, correct, chosen, info, fold_pred, W64, F):
    A = len(alphas)
    s = (F if F > 1 else 0) * A + chosen
    Wx, bx = fold_standardization(W_all[s], b_all[s], mean, inv_std)
    return RidgeFit(W_all[s], b_all[s], Wx, bx, float(alphas[chosen]), chosen, [int(v) for v in correct],
                    [int(v) for v in info], W_all, b_all, fold_pred, W64)


def fit_torch(X, y, fold, F: int, alphas, mean, inv_std, K: int, chain: str = "fp64") -> RidgeFit:
    """The oracle and the CPU path: fp64 moments (``chain="fp32"``: the kernels' chunked fp32 chains), fp64 solve and
    fp64 scores."""
    N, D = X.shape
    check_range(D, K, F, alphas, N)
    X, y = X.cpu().float(), y.cpu()
    rows, off = fold_order(fold, F)
    Af, Aall = moments_torch(X, y, rows, off, mean, inv_std, K, chain)
    Sys = systems_torch(Af if F > 1 else None, Aall, alphas, D, K)
    W, b, info = solve_torch(Sys, D, K, Aall, Af if F > 1 else None, len(alphas))
    A = len(alphas)
    alphas_t = torch.tensor([float(v) for v in alphas], dtype=torch.float64)
    correct = torch.zeros(A, dtype=torch.int64)
    fold_pred = None
    if F > 1:
        Z = working_rows(X, mean.cpu(), inv_std.cpu()).double()
        fid = torch.as_tensor(np.asarray(fold)).long()
        raw = torch.einsum("nd,skd->nsk", Z, W[:F * A]) + b[:F * A].unsqueeze(0)
        pred = first_argmax(raw).view(N, F, A)
        fold_pred = pred.gather(1, fid.view(N, 1, 1).expand(N, 1, A)).squeeze(1)
        correct = (fold_pred == y.long().view(N, 1)).sum(dim=0)
    chosen = int(choose_alpha(correct, alphas_t))
    return _finish(W.float(), b.float(), mean.cpu(), inv_std.cpu(), alphas, correct, chosen, info, fold_pred, W, F)


def pad_rows(X: torch.Tensor) -> torch.Tensor:
    """The rows as gemm_f32 takes them: a multiple of 4 columns, 16-byte aligned (a copy only when they are not)."""
    N, D = X.shape
    if D % 4 == 0 and X.is_contiguous() and X.data_ptr() % 16 == 0:
        return X
    Xp = torch.zeros(N, (D + 3) // 4 * 4, dtype=torch.float32, device=X.device)
    Xp[:, :D] = X
    return Xp


def scores_native(X: torch.Tensor, Wx: torch.Tensor, bx: torch.Tensor) -> torch.Tensor:
    """fp32 [N, C]: ``X Wx^T + bx`` for Wx [C, D] through ``gemm_f32`` (bias epilogue)."""
    from .gemm import EPI_BIAS_F32, gemm_f32

    N, D = X.shape
    C = Wx.shape[0]
    Xp = pad_rows(X)
    Dp, Cp = Xp.shape[1], max(8, (C + 7) // 8 * 8)
    Wp = torch.zeros(Cp, Dp, dtype=torch.float32, device=X.device)
    Wp[:C, :D] = Wx
    bp = torch.zeros(Cp, dtype=torch.float32, device=X.device)
    bp[:C] = bx
    out = torch.empty(N, Cp, dtype=torch.float32, device=X.device)
    gemm_f32(Xp, Wp, out, M=N, N=Cp, K=Dp, layout=0, epi=EPI_BIAS_F32, bias=bp)
    return out[:, :C]


def prepare_native(X, y, fold, F: int, alphas, mean, inv_std):
    """Device inputs of ``fit_device`` from host fold ids: everything that is uploaded before the first launch."""
    dev = X.device
    rows, off = fold_order(fold, F)
    fid = torch.as_tensor(np.asarray(fold.cpu() if isinstance(fold, torch.Tensor) else fold).astype(np.int64))
    return {"rows": rows.to(dev), "off": off, "fid": fid.to(dev),
            "y32": y.to(device=dev, dtype=torch.int32).contiguous(),
            "mean": mean.to(dev).float().contiguous(), "inv_std": inv_std.to(dev).float().contiguous(),
            "alphas_t": torch.tensor([float(v) for v in alphas], dtype=torch.float64).to(dev)}


def fit_device(X, p, K: int, workspace_bytes: Optional[int] = None, chunks_per_group: Optional[int] = None):
    """The kernel sequence, no host read: gram, reduce, then per batch of systems fill / factor / back-solve, one
    scoring product, the counts and the choice.  Returns device tensors (packed = [chosen, counts, info])."""
    N, D = X.shape
    dev = X.device
    off, alphas_t, y32, mean, inv_std = p["off"], p["alphas_t"], p["y32"], p["mean"], p["inv_std"]
    F, A = len(off) - 1, alphas_t.numel()
    S = num_systems(F, A)
    ldn = up64(D + K)
    budget = WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    per = max(1, min(S, budget // (ldn * ldn * 8)))
    mod = _native.kernels()

    Af, Aall = moments_native(X, y32, p["rows"], off, mean, inv_std, K, chunks_per_group)
    Sys = torch.empty(per, ldn, ldn, dtype=torch.float64, device=dev)
    info = torch.zeros(S, dtype=torch.int32, device=dev)
    W64 = torch.empty(S, K, ldn, dtype=torch.float64, device=dev)
    W = torch.empty(S, K, D, dtype=torch.float32, device=dev)
    b = torch.empty(S, K, dtype=torch.float32, device=dev)
    for s0 in range(0, S, per):   # the batching changes no result: the systems are independent
        args = _solve_args(Af, Aall, alphas_t, D, K, F, A, s0, min(per, S - s0), Sys, info, W64, W, b)
        for step in (0, 1, 2):
            mod.ridge_solve(step, *args)
    correct = torch.zeros(A, dtype=torch.int64, device=dev)
    fold_pred = None
    if F > 1:
        Wx, bx = fold_standardization(W[:F * A], b[:F * A], mean, inv_std)
        raw = scores_native(X, Wx.reshape(F * A * K, D), bx.reshape(F * A * K))
        pred = first_argmax(raw.reshape(N, F * A, K)).view(N, F, A)
        fold_pred = pred.gather(1, p["fid"].view(N, 1, 1).expand(N, 1, A)).squeeze(1)
        correct = (fold_pred == y32.long().view(N, 1)).sum(dim=0)
    chosen = choose_alpha(correct, alphas_t)
    packed = torch.cat([chosen.view(1), correct, info.to(torch.int64)])
    return {"W": W, "b": b, "W64": W64, "fold_pred": fold_pred, "packed": packed, "Af": Af, "Aall": Aall}


def fit_native(X, y, fold, F: int, alphas, mean, inv_std, K: int, workspace_bytes: Optional[int] = None,
               chunks_per_group: Optional[int] = None, keep_w64: bool = False) -> RidgeFit:
    """``prepare_native`` + ``fit_device`` + the ONE host read of the fit (chosen index, counts, info)."""
    N, D = X.shape
    check_range(D, K, F, alphas, N)
    A = len(alphas)
    if X.dtype != torch.float32 or X.stride(1) != 1:
        X = X.float().contiguous()
    p = prepare_native(X, y, fold, F, alphas, mean, inv_std)
    r = fit_device(X, p, K, workspace_bytes, chunks_per_group)
    host = r["packed"].cpu()
    return _finish(r["W"], r["b"], p["mean"], p["inv_std"], alphas, host[1:1 + A], int(host[0]), host[1 + A:],
                   r["fold_pred"], r["W64"][:, :, :D] if keep_w64 else None, F)


def fit(X, y, fold, F: int, alphas, mean, inv_std, K: int, native: Optional[bool] = None, **kw) -> RidgeFit:
    native = X.is_cuda if native is None else native
    if native:
        return fit_native(X, y, fold, F, alphas, mean, inv_std, K, **kw)
    return fit_torch(X, y, fold, F, alphas, mean, inv_std, K)


def predict_raw(X: torch.Tensor, Wx: torch.Tensor, bx: torch.Tensor, native: Optional[bool] = None) -> torch.Tensor:
    """fp32 [N, K] on the raw rows."""
    native = X.is_cuda if native is None else native
    if native:
        return scores_native(X.float(), Wx, bx)
    return X.float() @ Wx.T + bx
