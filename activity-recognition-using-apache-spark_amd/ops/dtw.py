"""Banded dynamic time warping between raw windows and the nearest-neighbour search under it: every
operation defined ONCE here as PyTorch code.

That code is the CPU path and the oracle of the HIP kernels in ``csrc/kernels/dtw.hip``; every ``*_torch``
function has a ``*_native`` front-end, and the plain names dispatch on the tensors' device (a GPU tensor
REQUIRES the kernels, as everywhere in the project).

Windows.  ``[W, A]``: W samples of A axes (1..9), time-major; a feature row is the flattened window, sample i
axis a at ``i * A + a``.  The functions take the windows as ``[N, W, A]``.  Inputs are finite: a NaN or an
infinity in a window is outside the definition (the minimum of the recurrence is not specified for them).

Cost.  For a query q and a reference r of the same W and a Sakoe-Chiba radius R, ``0 <= R <= W - 1``::

    c(i, j) = sum_a (q[i, a] - r[j, a])^2        axes in ascending order, for |i - j| <= R
    D(0, 0) = c(0, 0)
    D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1))    predecessors inside the band and the grid
    dtw(q, r) = D(W-1, W-1)

the squared-cost form, no square root inside the recurrence.  R = 0 is the squared Euclidean distance, R = W - 1
is unconstrained.  The oracle runs the recurrence in fp64; the kernel in fp32: ``d * d`` for axis 0, one fma per
further axis, ONE add per cell — the same sequence for a pair wherever it sits.  All terms are non-negative and
``min`` is exact, so ``|dtw_fp32 - dtw| <= gamma * dtw`` with ``gamma = 2 (2 W + A + 2) 2^-24`` (``gamma``).

Neighbours.  ``ops/knn.py``'s rule on the pairs ``(dtw(q_n, r_m), m)``: the k smallest in lexicographic order,
ascending, as ``idx`` int32 [N, k] and ``d2`` fp32 [N, k]; the pair (n, m) is skipped when ``qgroup[n] >= 0 and
qgroup[n] == rgroup[m]``; missing entries are ``(-1, +inf)``.  The vote is ``ops.knn.vote`` unchanged.

Normalisation.  ``zscore``: per window and per axis, ``(x - mean) / std`` with the fp64 moments over the W
samples; a constant axis keeps scale 1 (``ops/gmm.py``'s rule).  It is cold code in torch, before the search.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native
from . import knn as KN
from .knn import SearchResult, VoteResult, WEIGHTS  # noqa: F401  (the vote and its result types are kNN's)

MAX_W = 512                  # dtw.hip: samples per window
MAX_RADIUS = 64              # dtw.hip: the band is 2 R + 1 registers of a lane
MAX_AXES = 9
MAX_K = 64                   # one list entry per lane
MAX_CLASSES = KN.MAX_CLASSES
MAX_ROWS = (1 << 31) - 256   # queries / references (int32 indices)
MAX_COST_ROWS = 65535 * 64   # references of one dtw_cost launch (one workgroup row per slab)
MAX_SPLITS = 1024
ORACLE_CELLS = 1 << 24       # fp64 entries of one block of queries in the PyTorch path
NORMALIZE = ("none", "zscore")


def check_range(k: Optional[int] = None, W: Optional[int] = None, A: Optional[int] = None,
                radius: Optional[int] = None, C: Optional[int] = None, N: Optional[int] = None,
                M: Optional[int] = None, weights: Optional[str] = None):
    """The native range, on every device: k 1..64, W 1..512, A 1..9, 0 <= radius <= min(W - 1, 64), classes
    1..32, up to 2^31 - 256 rows."""
    if k is not None and not 1 <= int(k) <= MAX_K:
        raise ValueError(f"DTW takes k in 1..{MAX_K}, got {k}")
    if W is not None and not 1 <= int(W) <= MAX_W:
        raise ValueError(f"DTW takes windows of 1..{MAX_W} samples, got {W}")
    if A is not None and not 1 <= int(A) <= MAX_AXES:
        raise ValueError(f"DTW takes 1..{MAX_AXES} axes, got {A}")
    if radius is not None:
        if not 0 <= int(radius) <= MAX_RADIUS:
            raise ValueError(f"DTW takes a band radius in 0..{MAX_RADIUS}, got {radius}")
        if W is not None and int(radius) > int(W) - 1:
            raise ValueError(f"DTW takes a band radius of at most W - 1 = {int(W) - 1}, got {radius}")
    if C is not None and not 1 <= int(C) <= MAX_CLASSES:
        raise ValueError(f"DTW takes 1..{MAX_CLASSES} classes, got {C}")
    if N is not None and not 0 <= int(N) <= MAX_ROWS:
        raise ValueError(f"DTW takes up to {MAX_ROWS} query windows, got {N}")
    if M is not None and not 1 <= int(M) <= MAX_ROWS:
        raise ValueError(f"DTW takes 1..{MAX_ROWS} reference windows, got {M}")
    if weights is not None and weights not in WEIGHTS:
        raise ValueError(f"DTW weights must be one of {WEIGHTS}, got {weights!r}")


def gamma(W: int, A: int) -> float:
    """The relative error bound of an fp32 cost (module docstring)."""
    return 2.0 * (2 * W + A + 2) * 2.0 ** -24


def query_rows() -> int:
    """Queries of one workgroup of the kernels (the tests place their shapes around it)."""
    return int(_native.kernels().dtw_query_rows())


def slab_rows() -> int:
    """References of one slab of the kernels: one per lane."""
    return int(_native.kernels().dtw_slab_rows())


def auto_splits(N: int, M: int) -> int:
    """Reference splits the front-end takes when the caller names none."""
    return int(_native.kernels().dtw_auto_splits(int(N), int(M)))


def _check_windows(Q, R, radius):
    if Q.dim() != 3 or R.dim() != 3:
        raise ValueError("dtw: windows are [N, W, A] and [M, W, A]")
    if Q.shape[1:] != R.shape[1:]:
        raise ValueError(f"dtw: queries {tuple(Q.shape[1:])} and references {tuple(R.shape[1:])} differ in [W, A]")
    check_range(W=Q.shape[1], A=Q.shape[2], radius=radius, N=Q.shape[0], M=R.shape[0])


def as_windows(X: torch.Tensor, axes: int) -> torch.Tensor:
    """Feature rows [N, W * axes] -> windows [N, W, axes] (a view)."""
    if X.dim() != 2 or int(axes) < 1 or X.shape[1] % int(axes) != 0 or X.shape[1] == 0:
        raise ValueError(f"dtw: rows of {tuple(X.shape)} are not windows of {axes} axes")
    return X.reshape(X.shape[0], X.shape[1] // int(axes), int(axes))


def zscore(X: torch.Tensor) -> torch.Tensor:
    """Per-window, per-axis z-normalisation of [N, W, A] windows, fp32; a constant axis keeps scale 1."""
    xd = X.double()
    mean = xd.mean(dim=1, keepdim=True)
    sd = ((xd - mean) ** 2).mean(dim=1, keepdim=True).sqrt()
    sd = torch.where((sd > 0) & torch.isfinite(sd), sd, torch.ones_like(sd))
    return ((xd - mean) / sd).float().contiguous()


def normalize(X: torch.Tensor, how: str) -> torch.Tensor:
    if how not in NORMALIZE:
        raise ValueError(f"DTW normalize must be one of {NORMALIZE}, got {how!r}")
    return zscore(X) if how == "zscore" else X.float().contiguous()


# ------------------------------------------------------------------ 1. cost
def _cost_block(q: torch.Tensor, r: torch.Tensor, radius: int, dtype) -> torch.Tensor:
    """[n, M] costs of one block of queries: vectorised across the pairs, sequential over the cells."""
    n, W, A = q.shape
    M = r.shape[0]
    inf = float("inf")
    prev = torch.full((n, M, W), inf, dtype=dtype, device=q.device)
    for i in range(W):
        lo, hi = max(0, i - radius), min(W - 1, i + radius)
        c = torch.zeros(n, M, hi - lo + 1, dtype=dtype, device=q.device)
        for a in range(A):   # axes in ascending order
            d = q[:, i, a].view(n, 1, 1) - r[:, lo:hi + 1, a].view(1, M, -1)
            c = c + d * d
        cur = torch.full((n, M, W), inf, dtype=dtype, device=q.device)
        # min(D(i-1, j), D(i-1, j-1)) for the whole row, then the scan over D(i, j-1)
        up = prev[:, :, lo:hi + 1]
        diag = torch.full_like(up, inf)
        if lo >= 1:
            diag = prev[:, :, lo - 1:hi]
        elif hi >= 1:
            diag[:, :, 1:] = prev[:, :, 0:hi]
        best = torch.minimum(up, diag)
        for t in range(hi - lo + 1):
            j = lo + t
            b = best[:, :, t]
            if i == 0 and j == 0:
                b = torch.zeros_like(b)
            elif t > 0:
                b = torch.minimum(b, cur[:, :, j - 1])
            cur[:, :, j] = c[:, :, t] + b
        prev = cur
    return prev[:, :, W - 1]


def _cost_chunks(Q, R, radius, dtype):
    _check_windows(Q, R, radius)
    N, W, _ = Q.shape
    M = R.shape[0]
    out = torch.empty(N, M, dtype=dtype, device=Q.device)
    q, r = Q.to(dtype), R.to(dtype)
    step = max(1, ORACLE_CELLS // max(1, M * W))
    for lo in range(0, N, step):
        out[lo:lo + step] = _cost_block(q[lo:lo + step], r, int(radius), dtype)
    return out


def cost_torch(Q: torch.Tensor, R: torch.Tensor, radius: int) -> torch.Tensor:
    """fp64 [N, M]: the definition, in fp64."""
    return _cost_chunks(Q, R, radius, torch.float64)


def cost_torch_fp32(Q: torch.Tensor, R: torch.Tensor, radius: int) -> torch.Tensor:
    """The same recurrence in fp32 tensors (the probe's device baseline; not the kernel's rounding order)."""
    return _cost_chunks(Q, R, radius, torch.float32)


def _f32w(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 3:
        raise ValueError(f"dtw: {what} must be fp32, contiguous, [rows, W, A]")
    return t


def _i32c(t, n, what):
    if t is None:
        return None
    if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"dtw: {what} must be int32, contiguous, [{n}]")
    return t


def cost_native(Q: torch.Tensor, R: torch.Tensor, radius: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [N, M] by ``dtw_cost``: one launch."""
    _check_windows(Q, R, radius)
    _f32w(Q, "queries"), _f32w(R, "references")
    N, W, A = Q.shape
    M = R.shape[0]
    if M > MAX_COST_ROWS:
        raise ValueError(f"dtw_cost takes up to {MAX_COST_ROWS} references, got {M}")
    if out is None:
        out = torch.empty(N, M, dtype=torch.float32, device=Q.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (N, M) or not out.is_contiguous() or out.device != Q.device:
        raise ValueError("dtw: the cost output is fp32 [N, M], contiguous, on the queries' device")
    if N > 0:
        _native.kernels().dtw_cost(Q.data_ptr(), N, R.data_ptr(), M, W, A, int(radius), out.data_ptr(),
                                   _native.stream_ptr())
    return out


def cost(Q, R, radius: int, native: Optional[bool] = None) -> torch.Tensor:
    """[N, M] costs: fp32 from the kernel on the device, the fp64 definition on the host."""
    native = Q.is_cuda if native is None else native
    return cost_native(Q, R, radius) if native else cost_torch(Q, R, radius)


# ------------------------------------------------------------------ 2. search
def _check_search(Q, R, k, radius, qgroup, rgroup, y, C, weights):
    _check_windows(Q, R, radius)
    check_range(k=k, C=C if y is not None else None, weights=weights)
    if (qgroup is None) != (rgroup is None):
        raise ValueError("dtw: the exclusion takes both qgroup and rgroup")
    if qgroup is not None and (qgroup.numel() != Q.shape[0] or rgroup.numel() != R.shape[0]):
        raise ValueError("dtw: qgroup [N] and rgroup [M]")
    if y is not None and y.numel() != R.shape[0]:
        raise ValueError("dtw: one label per reference window")


def lists_from_cost(cost_nm: torch.Tensor, k: int, qgroup=None, rgroup=None):
    """(idx int32 [N, k], d2 fp32 [N, k]) of a cost matrix: a stable ascending sort IS the (cost, index) order."""
    N, M = cost_nm.shape
    s = cost_nm
    if qgroup is not None and rgroup is not None:
        qg = qgroup.long().view(-1, 1)
        s = torch.where((qg >= 0) & (qg == rgroup.long().view(1, -1)), torch.full_like(s, float("inf")), s)
    idx = torch.full((N, k), -1, dtype=torch.int32, device=s.device)
    d2 = torch.full((N, k), float("inf"), dtype=torch.float32, device=s.device)
    kk = min(k, M)
    v, i = torch.sort(s, dim=1, stable=True)
    v, i = v[:, :kk], i[:, :kk]
    ok = torch.isfinite(v)
    idx[:, :kk] = torch.where(ok, i, torch.full_like(i, -1)).to(torch.int32)
    d2[:, :kk] = torch.where(ok, v, torch.full_like(v, float("inf"))).float()
    return idx, d2


def neighbors_torch(Q, R, k: int, radius: int, qgroup=None, rgroup=None):
    _check_search(Q, R, k, radius, qgroup, rgroup, None, 0, None)
    N, W, _ = Q.shape
    M = R.shape[0]
    idx = torch.empty(N, int(k), dtype=torch.int32, device=Q.device)
    d2 = torch.empty(N, int(k), dtype=torch.float32, device=Q.device)
    step = max(1, ORACLE_CELLS // max(1, M * W))
    for lo in range(0, N, step):
        c = cost_torch(Q[lo:lo + step], R, radius)
        idx[lo:lo + step], d2[lo:lo + step] = lists_from_cost(c, int(k), None if qgroup is None else
                                                                qgroup[lo:lo + step], rgroup)
    return idx, d2


def search_torch(Q, R, k: int, radius: int, qgroup=None, rgroup=None, y=None, C: int = 0, weights: str = "uniform",
                 **_unused) -> SearchResult:
    _check_search(Q, R, k, radius, qgroup, rgroup, y, C, weights)
    idx, d2 = neighbors_torch(Q, R, k, radius, qgroup, rgroup)
    return SearchResult(idx, d2, None if y is None else KN.vote_torch(idx, d2, y, C, weights))


def search_native(Q, R, k: int, radius: int, qgroup=None, rgroup=None, y=None, C: int = 0, weights: str = "uniform",
                  splits: Optional[int] = None, idx_out=None, d2_out=None) -> SearchResult:
    """``dtw_search`` + ``dtw_merge`` (+ ``knn_merge_vote`` in its vote-only mode): no device -> host read."""
    _check_search(Q, R, k, radius, qgroup, rgroup, y, C, weights)
    mod = _native.kernels()
    _f32w(Q, "queries"), _f32w(R, "references")
    N, W, A = Q.shape
    M = R.shape[0]
    k = int(k)
    qgroup, rgroup = _i32c(qgroup, N, "qgroup"), _i32c(rgroup, M, "rgroup")
    nslabs = -(-M // mod.dtw_slab_rows())
    if splits is None:
        S = mod.dtw_auto_splits(max(N, 1), M)
    else:
        if int(splits) < 1:
            raise ValueError(f"dtw: splits must be >= 1, got {splits}")
        S = min(int(splits), nslabs, MAX_SPLITS)
    dev = Q.device
    idx = torch.empty(N, k, dtype=torch.int32, device=dev) if idx_out is None else idx_out
    d2 = torch.empty(N, k, dtype=torch.float32, device=dev) if d2_out is None else d2_out
    for t, dt in ((idx, torch.int32), (d2, torch.float32)):
        if t.dtype != dt or tuple(t.shape) != (N, k) or not t.is_contiguous() or t.device != dev:
            raise ValueError("dtw: outputs idx int32 / d2 fp32 [N, k], contiguous, on the queries' device")
    if y is not None:
        y = _i32c(y, M, "labels")
    if N > 0:
        ps = torch.empty(S, N, k, dtype=torch.float32, device=dev)
        pi = torch.empty(S, N, k, dtype=torch.int32, device=dev)
        st = _native.stream_ptr()
        mod.dtw_search(Q.data_ptr(), N, R.data_ptr(), M, W, A, int(radius), k, S, _native.ptr(qgroup),
                       _native.ptr(rgroup), ps.data_ptr(), pi.data_ptr(), st)
        mod.dtw_merge(ps.data_ptr(), pi.data_ptr(), S, N, k, idx.data_ptr(), d2.data_ptr(), st)
    v = None
    if y is not None:
        v = KN.vote_native(idx, d2, y, C, weights) if N > 0 else KN.vote_torch(idx, d2, y, C, weights)
    return SearchResult(idx, d2, v)


def search(Q, R, k: int, radius: int, native: Optional[bool] = None, **kw) -> SearchResult:
    native = Q.is_cuda if native is None else native
    if native:
        if kw.get("y") is not None:
            kw["y"] = kw["y"].to(torch.int32).contiguous()
        return search_native(Q, R, k, radius, **kw)
    return search_torch(Q, R, k, radius, **kw)


def neighbors_native(Q, R, k: int, radius: int, qgroup=None, rgroup=None, splits=None, idx_out=None, d2_out=None):
    r = search_native(Q, R, k, radius, qgroup, rgroup, splits=splits, idx_out=idx_out, d2_out=d2_out)
    return r.idx, r.d2


def neighbors(Q, R, k: int, radius: int, qgroup=None, rgroup=None, native: Optional[bool] = None, **kw):
    """(idx int32 [N, k], d2 fp32 [N, k])."""
    r = search(Q, R, k, radius, native, qgroup=qgroup, rgroup=rgroup, **kw)
    return r.idx, r.d2
