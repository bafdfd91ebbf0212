"""Exact k-nearest neighbours and the neighbour vote: every operation defined ONCE here as PyTorch code.

That code is the CPU path and the oracle of the HIP kernels in ``csrc/kernels/knn.hip``; every ``*_torch``
function has a ``*_native`` front-end, and the plain names dispatch on the tensors' device (a GPU tensor
REQUIRES the kernels, as everywhere in the project).

Working rows.  ``Z = (X - mean) / std`` in fp32 with the training rows' fp32 column means and (population)
standard deviations from fp64 sums, rounded once; a constant column keeps scale 1 (``ops/gmm.py``'s rule).
Without standardising only the mean is removed (``std = 1``).

Score.  ``s[n, m] = h[m] - <q_n, r_m>`` with ``h[m] = ||r_m||^2 / 2`` (``kmeans.center_h``), the order of the
squared distance ``nrm[n] + 2 s``.  ``d2 = float32(max(0, nrm[n] + 2 s))`` in fp64 from the score, with
``kmeans.row_norms``.  The oracle evaluates the score in fp64, the kernel on the fp32 matrix cores.

Neighbours.  The neighbours of row n are the k smallest PAIRS ``(s[n, m], m)`` in lexicographic order (ties go
to the lower reference index), returned ascending as ``idx`` int32 [N, k] and ``d2`` fp32 [N, k].  The total
order makes the answer one set: it cannot depend on the insertion order, on how the references are split or
on how the queries are batched, and the first k' entries of a k-search are the k'-search.

Exclusion.  With ``qgroup`` int32 [N] and ``rgroup`` int32 [M] the pair (n, m) is skipped when
``qgroup[n] >= 0 and qgroup[n] == rgroup[m]``.  A row with fewer than k admissible references (M < k
included) ends in ``idx = -1``, ``d2 = +inf``; the vote ignores those entries.

Vote.  The class weight ``c[n, j]`` is the sum of ``w_i`` over the valid neighbours of class j, in list order.
``"uniform"``: ``w = 1``.  ``"distance"``: ``w = 1 / sqrt(d2)`` in fp64; when a valid neighbour has ``d2 == 0``
those neighbours get 1 and the others 0 (scikit-learn's rule).  ``rawPrediction = c``, ``probability = c /
sum c`` (uniform over the classes when no neighbour is valid), prediction = the first argmax.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _native
from . import kmeans as KM

MAX_K = 64                   # knn.hip: one list entry per lane
MAX_D = 256                  # knn.hip: the A fragment is at most 64 registers
MAX_CLASSES = 32
MAX_ROWS = (1 << 31) - 256   # queries / references (int32 indices, grid.x)
MAX_SPLITS = 1024
ORACLE_CHUNK = 4096          # queries per block of fp64 scores in the PyTorch path
WEIGHTS = ("uniform", "distance")


def check_range(k: int, D: int, C: Optional[int] = None, N: Optional[int] = None, M: Optional[int] = None,
                weights: Optional[str] = None):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"KNN takes k in 1..{MAX_K}, got {k}")
    if not 1 <= int(D) <= MAX_D:
        raise ValueError(f"KNN takes 1..{MAX_D} features, got {D}")
    if C is not None and not 1 <= int(C) <= MAX_CLASSES:
        raise ValueError(f"KNN takes 1..{MAX_CLASSES} classes, got {C}")
    if N is not None and not 0 <= int(N) <= MAX_ROWS:
        raise ValueError(f"KNN takes up to {MAX_ROWS} query rows, got {N}")
    if M is not None and not 1 <= int(M) <= MAX_ROWS:
        raise ValueError(f"KNN takes 1..{MAX_ROWS} reference rows, got {M}")
    if weights is not None and weights not in WEIGHTS:
        raise ValueError(f"KNN weights must be one of {WEIGHTS}, got {weights!r}")


def slab_rows(D: int) -> int:
    """Reference rows of one LDS slab of ``knn_search`` (the tests place their shapes around it)."""
    return int(_native.kernels().knn_slab_rows(int(D)))


def query_rows() -> int:
    return int(_native.kernels().knn_query_rows())


def auto_splits(N: int, M: int, D: int) -> int:
    """Reference splits the front-end takes when the caller names none."""
    return int(_native.kernels().knn_auto_splits(int(N), int(M), int(D)))


# ------------------------------------------------------------------ working rows
def standardizer(X: torch.Tensor, standardize: bool = True):
    """(mean, std) fp32 [D] from fp64 sums; a constant column, or ``standardize=False``, has std = 1."""
    xd = X.double()
    n = max(X.shape[0], 1)
    mean = xd.sum(dim=0) / n
    if not standardize:
        return mean.float(), torch.ones_like(mean, dtype=torch.float32)
    sd = (((xd - mean.view(1, -1)) ** 2).sum(dim=0) / n).sqrt()
    sd = torch.where((sd > 0) & torch.isfinite(sd), sd, torch.ones_like(sd))
    return mean.float(), sd.float()


def working_rows(X: torch.Tensor, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    return ((X.float() - mean.view(1, -1)) / std.view(1, -1)).contiguous()


def reference_h(R: torch.Tensor) -> torch.Tensor:
    return KM.center_h(R)


# ------------------------------------------------------------------ 1. search
def scores_torch(Q, R, h, qgroup=None, rgroup=None) -> torch.Tensor:
    """fp64 [N, M]; an excluded pair is +inf."""
    s = KM.scores_torch(Q, R, h)
    if qgroup is not None and rgroup is not None:
        qg = qgroup.long().view(-1, 1)
        s = torch.where((qg >= 0) & (qg == rgroup.long().view(1, -1)), torch.full_like(s, float("inf")), s)
    return s


def partial_torch(Q, R, h, k: int, qgroup=None, rgroup=None, offset: int = 0):
    """The sorted list of one block of references: (scores fp64 [N, k], indices int32 [N, k] + ``offset``),
    missing entries (+inf, -1).  A stable ascending sort of the scores IS the (score, index) order."""
    N, M = Q.shape[0], R.shape[0]
    ps = torch.full((N, k), float("inf"), dtype=torch.float64, device=Q.device)
    pi = torch.full((N, k), -1, dtype=torch.int32, device=Q.device)
    kk = min(k, M)
    for lo in range(0, N, ORACLE_CHUNK):
        hi = min(N, lo + ORACLE_CHUNK)
        s = scores_torch(Q[lo:hi], R, h, None if qgroup is None else qgroup[lo:hi], rgroup)
        v, i = torch.sort(s, dim=1, stable=True)
        v, i = v[:, :kk], i[:, :kk]
        ok = torch.isfinite(v)
        ps[lo:hi, :kk] = torch.where(ok, v, torch.full_like(v, float("inf")))
        pi[lo:hi, :kk] = torch.where(ok, i + offset, torch.full_like(i, -1)).to(torch.int32)
    return ps, pi


def merge_torch(ps: torch.Tensor, pi: torch.Tensor, k: int):
    """The k smallest pairs of partial lists [S, N, k'] under the (score, index) order."""
    S, N, kp = ps.shape
    s = ps.permute(1, 0, 2).reshape(N, S * kp)
    i = pi.permute(1, 0, 2).reshape(N, S * kp).long()
    key = torch.where(i >= 0, i, torch.full_like(i, 1 << 40))   # missing entries last among equals
    o = torch.sort(key, dim=1, stable=True).indices
    s, i = s.gather(1, o), i.gather(1, o)
    o = torch.sort(s, dim=1, stable=True).indices[:, :k]
    s, i = s.gather(1, o), i.gather(1, o)
    if s.shape[1] < k:
        pad = k - s.shape[1]
        s = torch.cat([s, torch.full((N, pad), float("inf"), dtype=s.dtype, device=s.device)], dim=1)
        i = torch.cat([i, torch.full((N, pad), -1, dtype=i.dtype, device=i.device)], dim=1)
    return s, i.to(torch.int32)


def finish_torch(Q, s, idx):
    """d2 fp32 of the listed pairs from their scores."""
    d2 = (KM.row_norms(Q).view(-1, 1) + 2.0 * s.double()).clamp_min(0.0).float()
    return torch.where(idx >= 0, d2, torch.full_like(d2, float("inf")))


def neighbors_torch(Q, R, h, k: int, qgroup=None, rgroup=None):
    check_range(k, Q.shape[1], N=Q.shape[0], M=R.shape[0])
    s, idx = partial_torch(Q, R, h, int(k), qgroup, rgroup)
    return idx, finish_torch(Q, s, idx)


# ------------------------------------------------------------------ 2. vote
@dataclass
class VoteResult:
    raw: torch.Tensor    # float64 [N, C] class weights
    prob: torch.Tensor   # float64 [N, C]
    pred: torch.Tensor   # int64 [N]


def vote_torch(idx, d2, y, C: int, weights: str = "uniform", k: Optional[int] = None) -> VoteResult:
    """The vote over the first ``k`` entries of every list (all of them when not given)."""
    k = idx.shape[1] if k is None else int(k)
    check_range(k, 1, C=C, weights=weights)
    idx, d2 = idx[:, :k].long(), d2[:, :k].double()
    N = idx.shape[0]
    valid = idx >= 0
    cls = y.long()[idx.clamp_min(0)]
    if weights == "uniform":
        w = valid.double()
    else:
        zero = valid & (d2 == 0)
        anyzero = zero.any(dim=1, keepdim=True)
        inv = 1.0 / torch.where(valid & ~zero, d2, torch.ones_like(d2)).sqrt()
        w = torch.where(anyzero, zero.double(), torch.where(valid, inv, torch.zeros_like(inv)))
    raw = torch.zeros(N, C, dtype=torch.float64, device=idx.device)
    for i in range(k):   # in list order: one fixed rounding sequence
        raw.scatter_add_(1, cls[:, i:i + 1], w[:, i:i + 1])
    tot = torch.zeros(N, dtype=torch.float64, device=idx.device)
    for j in range(C):
        tot = tot + raw[:, j]
    prob = torch.where(tot.view(N, 1) > 0, raw / torch.where(tot > 0, tot, torch.ones_like(tot)).view(N, 1),
                       torch.full_like(raw, 1.0) / C)
    return VoteResult(raw, prob, raw.argmax(dim=1))


def _i32c(t, n, what):
    if t is None:
        return None
    if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"knn: {what} must be int32, contiguous, [{n}]")
    return t


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2:
        raise ValueError(f"knn: {what} must be fp32, contiguous, [rows, D]")
    return t


def vote_native(idx, d2, y, C: int, weights: str = "uniform", k: Optional[int] = None) -> VoteResult:
    N, ldk = idx.shape
    k = ldk if k is None else int(k)
    check_range(k, 1, C=C, weights=weights)
    if k > ldk or idx.dtype != torch.int32 or d2.dtype != torch.float32 or not idx.is_contiguous() or \
            not d2.is_contiguous() or d2.shape != idx.shape:
        raise ValueError("knn vote: idx int32 / d2 fp32 [N, >= k], contiguous")
    y = _i32c(y, y.numel(), "labels")
    dev = idx.device
    raw = torch.empty(N, C, dtype=torch.float64, device=dev)
    prob = torch.empty(N, C, dtype=torch.float64, device=dev)
    pred = torch.empty(N, dtype=torch.int32, device=dev)
    _native.kernels().knn_merge_vote(0, 0, 0, 0, 0, N, k, ldk, idx.data_ptr(), d2.data_ptr(), y.data_ptr(), y.numel(),
                                     int(C), WEIGHTS.index(weights), raw.data_ptr(), prob.data_ptr(), pred.data_ptr(),
                                     _native.stream_ptr())
    return VoteResult(raw, prob, pred.long())


def vote(idx, d2, y, C: int, weights: str = "uniform", k: Optional[int] = None, native: Optional[bool] = None):
    native = idx.is_cuda if native is None else native
    if native:
        return vote_native(idx, d2, y.to(torch.int32).contiguous(), C, weights, k)
    return vote_torch(idx, d2, y, C, weights, k)


# ------------------------------------------------------------------ search + vote front-ends
@dataclass
class SearchResult:
    idx: torch.Tensor               # int32 [N, k]
    d2: torch.Tensor                # float32 [N, k]
    vote: Optional[VoteResult]      # with labels


def _check_search(Q, R, h, k, qgroup, rgroup, y, C, weights):
    if Q.dim() != 2 or R.dim() != 2 or Q.shape[1] != R.shape[1] or h.numel() != R.shape[0]:
        raise ValueError("knn: queries [N, D], references [M, D] and h [M] must match")
    check_range(k, Q.shape[1], C=C if y is not None else None, N=Q.shape[0], M=R.shape[0], weights=weights)
    if (qgroup is None) != (rgroup is None):
        raise ValueError("knn: the exclusion takes both qgroup and rgroup")
    if y is not None and y.numel() != R.shape[0]:
        raise ValueError("knn: one label per reference row")


def search_torch(Q, R, h, k: int, qgroup=None, rgroup=None, y=None, C: int = 0, weights: str = "uniform",
                 **_unused) -> SearchResult:
    _check_search(Q, R, h, k, qgroup, rgroup, y, C, weights)
    idx, d2 = neighbors_torch(Q, R, h, k, qgroup, rgroup)
    return SearchResult(idx, d2, None if y is None else vote_torch(idx, d2, y, C, weights))


def search_native(Q, R, h, k: int, qgroup=None, rgroup=None, y=None, C: int = 0, weights: str = "uniform",
                  splits: Optional[int] = None, idx_out=None, d2_out=None) -> SearchResult:
    """``knn_search`` + ``knn_merge_vote``: two launches, no device -> host read."""
    _check_search(Q, R, h, k, qgroup, rgroup, y, C, weights)
    mod = _native.kernels()
    N, D = Q.shape
    M = R.shape[0]
    k = int(k)
    _f32c(Q, "queries"), _f32c(R, "references")
    if h.dtype != torch.float32 or not h.is_contiguous():
        raise ValueError("knn: h must be fp32 and contiguous")
    qgroup, rgroup = _i32c(qgroup, N, "qgroup"), _i32c(rgroup, M, "rgroup")
    nslabs = -(-M // mod.knn_slab_rows(D))
    if splits is None:
        S = mod.knn_auto_splits(max(N, 1), M, D)
    else:
        if int(splits) < 1:
            raise ValueError(f"knn: splits must be >= 1, got {splits}")
        S = min(int(splits), nslabs, MAX_SPLITS)
    dev = Q.device
    idx = torch.empty(N, k, dtype=torch.int32, device=dev) if idx_out is None else idx_out
    d2 = torch.empty(N, k, dtype=torch.float32, device=dev) if d2_out is None else d2_out
    for t, dt in ((idx, torch.int32), (d2, torch.float32)):
        if t.dtype != dt or tuple(t.shape) != (N, k) or not t.is_contiguous() or t.device != dev:
            raise ValueError("knn: outputs idx int32 / d2 fp32 [N, k], contiguous, on the queries' device")
    v = None
    raw = prob = pred = None
    if y is not None:
        y = _i32c(y, M, "labels")
        raw = torch.empty(N, C, dtype=torch.float64, device=dev)
        prob = torch.empty(N, C, dtype=torch.float64, device=dev)
        pred = torch.empty(N, dtype=torch.int32, device=dev)
    if N > 0:
        ps = torch.empty(S, N, k, dtype=torch.float32, device=dev)
        pi = torch.empty(S, N, k, dtype=torch.int32, device=dev)
        st = _native.stream_ptr()
        mod.knn_search(Q.data_ptr(), N, R.data_ptr(), h.data_ptr(), M, D, k, S, _native.ptr(qgroup), _native.ptr(rgroup),
                       ps.data_ptr(), pi.data_ptr(), st)
        mod.knn_merge_vote(ps.data_ptr(), pi.data_ptr(), S, Q.data_ptr(), D, N, k, k, idx.data_ptr(), d2.data_ptr(),
                           _native.ptr(y), M, int(C) if y is not None else 0, WEIGHTS.index(weights), _native.ptr(raw),
                           _native.ptr(prob), _native.ptr(pred), st)
    if y is not None:
        v = VoteResult(raw, prob, pred.long())
    return SearchResult(idx, d2, v)


def search(Q, R, h, k: int, native: Optional[bool] = None, **kw) -> SearchResult:
    native = Q.is_cuda if native is None else native
    if native:
        if kw.get("y") is not None:
            kw["y"] = kw["y"].to(torch.int32).contiguous()
        return search_native(Q, R, h, k, **kw)
    return search_torch(Q, R, h, k, **kw)


def neighbors_native(Q, R, h, k: int, qgroup=None, rgroup=None, splits=None, idx_out=None, d2_out=None):
    r = search_native(Q, R, h, k, qgroup, rgroup, splits=splits, idx_out=idx_out, d2_out=d2_out)
    return r.idx, r.d2


def neighbors(Q, R, h, k: int, qgroup=None, rgroup=None, native: Optional[bool] = None, **kw):
    """(idx int32 [N, k], d2 fp32 [N, k])."""
    r = search(Q, R, h, k, native, qgroup=qgroup, rgroup=rgroup, **kw)
    return r.idx, r.d2
