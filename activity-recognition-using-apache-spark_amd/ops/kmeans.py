"""K-means and the squared-Euclidean silhouette: every operation defined ONCE here as PyTorch code.

That code is the CPU path and the oracle of the HIP kernels in ``csrc/kernels/kmeans.hip``; every
``*_torch`` function has a ``*_native`` front-end, and the plain names dispatch on the tensors' device
(a GPU tensor REQUIRES the kernels, as everywhere in the project).

Working rows.  ``Xc = X - mean`` with the fp32 column means (fp64 sums, rounded once), subtracted once
per fit.  K-means is translation invariant; centring keeps the expanded distance below free of large
cancellations.  Models store their centres in the original coordinates (``C + mean``).

Score.  ``s[n, k] = h[k] - <Xc[n], C[k]>`` with ``h[k] = ||C[k]||^2 / 2`` (``center_h``: fp64, features in
order, rounded to fp32).  The assignment is the argmin over k; TIES GO TO THE LOWEST k.  The oracle
evaluates the score in fp64, the kernel on the fp32 matrix cores.  The squared distance is
``d2 = float32(max(0, nrm[n] + 2 s))`` (fp64 arithmetic on the score), where the row norm is
``nrm = (p0 + p1) + (p2 + p3)``, ``p_j`` = the fp64 sum of ``Xc[n, f]^2`` over f = j, j + 4, ... in that
order (``row_norms``; an fp32 square is exact in fp64, so this is one fixed rounding sequence).

Fixed-point accumulation.  Per fit and feature f, ``2^e[f]`` is the largest power of two with
``max|Xc[:, f]| * 2^e[f] < 2^30`` (an all-zero column: e = 0; ``feature_scales``).  A row of integer
weight w (1 without a weight vector; 0 = the row is ignored) adds ``w * rint(Xc[n, f] * 2^e[f])`` — the
scaling is exact, the value an int32 — to an int64 ``[K, D]`` sum, ``w`` to an int64 ``[K]`` count and
``w * rint(nrm[n] * 2^q)`` to an int64 ``[K]`` norm channel, where ``2^q`` is the largest power of two with
``max_n nrm[n] * 2^q < 2^36`` (``norm_scale``).  The three live in ONE flat int64 buffer
``[K*D | K | K]``.  All sums are exact integers, so the order of the adds (atomics, workgroups, ranks)
cannot matter.  The total weight must stay below 2^26.

Update.  ``C_new[k, f] = float32(float64(sum[k, f]) * 2^-e[f] / count[k])``; an empty cluster keeps its
centre (Spark's behaviour).  ``moved = max_k ||C_new[k] - C[k]||^2`` in fp64, features in order, every
operation rounded on its own; the fit has converged when ``moved <= tol^2``.

Cost.  ``cost = sum_n w[n] * d2[n]`` as fp64 per-workgroup partials reduced in a fixed order.

Silhouette (Spark's squared-Euclidean form, O(N K)).  With the per-cluster moments N_k (count), Y_k
(sum of rows) and Psi_k (sum of ||x||^2), the mean squared distance of row n to cluster k is
``||x||^2 + Psi_k / N_k - 2 <x, Y_k> / N_k``; for the row's own cluster a the mean over the OTHER members
is that value times ``N_a / (N_a - 1)``.  ``s = (b - a) / max(a, b)`` with b the minimum over the other
non-empty clusters; a singleton cluster, or no other cluster, gives 0.  The kernel is the assignment
kernel's product with operand rows ``Y_k / N_k`` and ``h = Psi_k / (2 N_k)``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native, rng

MAX_K = 256                  # kmeans.hip: centres
MAX_D = 256                  # kmeans.hip: features (four 16-row tiles and a 16-centre slab fit the LDS)
MAX_ROWS = (1 << 31) - 256   # kmeans.hip: row chunks on grid.x
MAX_WEIGHT = 1 << 26         # total integer weight: |sum| < 2^30 * 2^26, norm channel < 2^36 * 2^26
QBITS = 30
NORM_BITS = 36


def check_native_range(k: int, D: int, N: Optional[int] = None):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"KMeans takes k in 1..{MAX_K}, got {k}")
    if not 1 <= int(D) <= MAX_D:
        raise ValueError(f"KMeans takes 1..{MAX_D} features, got {D}")
    if N is not None and not 1 <= int(N) <= MAX_ROWS:
        raise ValueError(f"KMeans takes 1..{MAX_ROWS} rows, got {N}")


def rows_per_block() -> int:
    """Rows a ``kmeans_assign`` workgroup takes (the tests place their shapes around it)."""
    return int(_native.kernels().kmeans_rows_per_block())


def native_plan(D: int, K: int):
    """(centres per LDS slab, slabs, accumulators in LDS?, LDS bytes) of a shape."""
    kt, npass, lds_acc, nbytes = _native.kernels().kmeans_plan(int(D), int(K))
    return kt, npass, bool(lds_acc), nbytes


# ------------------------------------------------------------------ per-fit constants
def column_means(X: torch.Tensor) -> torch.Tensor:
    return (X.double().sum(dim=0) / max(X.shape[0], 1)).float()


def _pow2_below(amax: torch.Tensor, bits: int) -> torch.Tensor:
    """int32 e: the largest with amax * 2^e < 2^bits (amax = 0: e = 0), clamped so 2^e is a normal fp32."""
    _, ex = torch.frexp(amax.double())          # amax = fr * 2^ex, fr in [0.5, 1): amax < 2^ex
    e = torch.where(amax > 0, bits - ex, torch.zeros_like(ex))
    return e.clamp(-100, 100).to(torch.int32)


def feature_scales(Xc: torch.Tensor) -> torch.Tensor:
    """fp32 [D]: 2^e[f]."""
    amax = Xc.abs().amax(dim=0) if Xc.shape[0] else torch.zeros(Xc.shape[1], device=Xc.device)
    return torch.ldexp(torch.ones_like(amax, dtype=torch.float32), _pow2_below(amax, QBITS))


def row_norms(Xc: torch.Tensor) -> torch.Tensor:
    """fp64 [N]: (p0 + p1) + (p2 + p3), p_j the in-order sum of the squares of features j, j + 4, ..."""
    N, D = Xc.shape
    Dp = (D + 3) // 4 * 4
    sq = torch.zeros(N, Dp, dtype=torch.float64, device=Xc.device)
    sq[:, :D] = Xc.double() ** 2
    sq = sq.view(N, Dp // 4, 4)
    p = torch.zeros(N, 4, dtype=torch.float64, device=Xc.device)
    for i in range(Dp // 4):
        p = p + sq[:, i]
    return (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])


def norm_scale(nrm: torch.Tensor) -> torch.Tensor:
    """fp64 [1] on the rows' device: 2^q."""
    mx = nrm.max().reshape(1) if nrm.numel() else torch.zeros(1, dtype=torch.float64, device=nrm.device)
    return torch.ldexp(torch.ones(1, dtype=torch.float64, device=nrm.device), _pow2_below(mx, NORM_BITS))


def center_h(C: torch.Tensor) -> torch.Tensor:
    """fp32 [K]: ||C[k]||^2 / 2, summed in fp64 over the features in order."""
    cd = C.double()
    acc = torch.zeros(C.shape[0], dtype=torch.float64, device=C.device)
    for f in range(C.shape[1]):
        acc = acc + cd[:, f] * cd[:, f]
    return (0.5 * acc).float()


def acc_size(K: int, D: int) -> int:
    return K * (D + 2)


def acc_views(acc: torch.Tensor, K: int, D: int):
    """(sums [K, D], counts [K], norms [K]) of the flat accumulator buffer."""
    return acc[:K * D].view(K, D), acc[K * D:K * D + K], acc[K * D + K:K * D + 2 * K]


# ------------------------------------------------------------------ random init
def random_init_keys(seed: int, n_rows: int, row_offset: int = 0) -> np.ndarray:
    """uint64 keys of rows [row_offset, row_offset + n_rows): Philox word << 32 | global row id (distinct)."""
    ids = np.arange(row_offset, row_offset + n_rows, dtype=np.uint64)
    return (rng.uniform_u32(seed, rng.STREAM_KMEANS_INIT, ids).astype(np.uint64) << np.uint64(32)) | ids


def random_init_rows(seed: int, k: int, n_rows: int, row_offset: int = 0) -> np.ndarray:
    """Global ids of the (at most) k rows of the shard with the smallest keys, by ascending key.  The k
    smallest of the union of the shards' picks are the pick of the whole table: shard independent."""
    keys = np.sort(random_init_keys(seed, n_rows, row_offset))[:k]
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ------------------------------------------------------------------ 1. assignment + accumulation
@dataclass
class AssignResult:
    assign: Optional[torch.Tensor]   # int32 [N]
    d2: Optional[torch.Tensor]       # float32 [N]
    part: Optional[torch.Tensor]     # float64 cost partials (one here; one per workgroup from the kernel)


def scores_torch(Xc: torch.Tensor, C: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """fp64 [N, K]."""
    return h.double().view(1, -1) - Xc.double() @ C.double().t()


def accumulate_torch(Xc, assign, w, scale, nscale, K: int, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Add the rows' fixed-point values into the flat int64 buffer (allocated zero when not given)."""
    N, D = Xc.shape
    dev = Xc.device
    if acc is None:
        acc = torch.zeros(acc_size(K, D), dtype=torch.int64, device=dev)
    a = assign.long()
    ok = (a >= 0) & (a < K)
    wv = torch.ones(N, dtype=torch.int64, device=dev) if w is None else w.long()
    wv = torch.where(ok, wv, torch.zeros_like(wv))
    a = a.clamp(0, K - 1)
    sums, counts, norms = acc_views(acc, K, D)
    q = torch.round(Xc * scale.view(1, D)).long() * wv.view(N, 1)
    sums.index_add_(0, a, q)
    counts.index_add_(0, a, wv)
    norms.index_add_(0, a, torch.round(row_norms(Xc) * nscale.double()).long() * wv)
    return acc


def assign_torch(Xc, C, h, w=None, scale=None, nscale=None, acc=None, want_assign=True, want_cost=True):
    K = C.shape[0]
    s = scores_torch(Xc, C, h)
    smin = s.min(dim=1).values
    a = s.argmin(dim=1).to(torch.int32)        # first minimum: the lowest k
    d2 = (row_norms(Xc) + 2.0 * smin).clamp_min(0.0).float()
    if acc is not None:
        accumulate_torch(Xc, a, w, scale, nscale, K, acc)
    part = None
    if want_cost:
        wd = torch.ones_like(d2, dtype=torch.float64) if w is None else w.double()
        part = (wd * d2.double()).sum().reshape(1)
    return AssignResult(a, d2, part)


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"kmeans: {what} must be fp32 and contiguous")
    return t


def assign_native(Xc, C, h, w=None, scale=None, nscale=None, acc=None, want_assign=True, want_cost=True,
                  assign_out=None, d2_out=None, part_out=None):
    mod = _native.kernels()
    N, D = Xc.shape
    K = C.shape[0]
    check_native_range(K, D)
    _f32c(Xc, "rows"), _f32c(C, "centres"), _f32c(h, "h")
    if C.shape[1] != D or h.numel() != K:
        raise ValueError("kmeans: centres [K, D] and h [K] must match the rows")
    if w is not None and (w.dtype != torch.int32 or w.numel() != N):
        raise ValueError("kmeans: weights int32 [N]")
    if acc is not None and (acc.dtype != torch.int64 or acc.numel() != acc_size(K, D) or scale is None or nscale is None):
        raise ValueError("kmeans: accumulators int64 [K * (D + 2)] with scale and norm scale")
    dev = Xc.device
    nb = max(1, -(-N // mod.kmeans_rows_per_block()))
    a = d2 = part = None
    if want_assign:
        a = torch.empty(N, dtype=torch.int32, device=dev) if assign_out is None else assign_out
        d2 = torch.empty(N, dtype=torch.float32, device=dev) if d2_out is None else d2_out
    if want_cost:
        part = torch.zeros(nb, dtype=torch.float64, device=dev) if part_out is None else part_out
    mod.kmeans_assign(Xc.data_ptr(), N, D, K, C.data_ptr(), h.data_ptr(), _native.ptr(w), 0, _native.ptr(scale),
                      _native.ptr(nscale), _native.ptr(a), _native.ptr(d2), _native.ptr(acc), _native.ptr(part),
                      _native.stream_ptr())
    return AssignResult(a, d2, part)


def accumulate_native(Xc, assign, w, scale, nscale, K: int, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``accumulate_torch`` through the kernel's given-labels mode (no product)."""
    N, D = Xc.shape
    check_native_range(K, D)
    _f32c(Xc, "rows")
    if acc is None:
        acc = torch.zeros(acc_size(K, D), dtype=torch.int64, device=Xc.device)
    lab = assign.to(torch.int32).contiguous()
    _native.kernels().kmeans_assign(Xc.data_ptr(), N, D, K, 0, 0, _native.ptr(w), lab.data_ptr(), scale.data_ptr(),
                                    nscale.data_ptr(), 0, 0, acc.data_ptr(), 0, _native.stream_ptr())
    return acc


def assign(Xc, C, h, native: Optional[bool] = None, **kw) -> AssignResult:
    native = Xc.is_cuda if native is None else native
    if native:
        return assign_native(Xc, C, h, **kw)
    for k in ("assign_out", "d2_out", "part_out"):
        kw.pop(k, None)
    return assign_torch(Xc, C, h, **kw)


def accumulate(Xc, assign_, w, scale, nscale, K, acc=None, native: Optional[bool] = None):
    native = Xc.is_cuda if native is None else native
    return (accumulate_native if native else accumulate_torch)(Xc, assign_, w, scale, nscale, K, acc)


# ------------------------------------------------------------------ 2. update
@dataclass
class FitState:
    """Device-resident state of one fit (what ``kmeans_update`` reads and writes)."""
    C: torch.Tensor          # float32 [K, D] working-coordinate centres
    h: torch.Tensor          # float32 [K]
    acc: torch.Tensor        # int64 [K * (D + 2)]
    state: torch.Tensor      # int32 [2]: iterations, converged
    cost_hist: torch.Tensor  # float64 [maxIter]
    moved: torch.Tensor      # float64 [1]
    sizes: torch.Tensor      # int64 [K]: counts behind the last update
    Cnew: torch.Tensor       # float32 [K, D] scratch

    @classmethod
    def alloc(cls, C: torch.Tensor, max_iter: int) -> "FitState":
        K, D = C.shape
        dev = C.device
        C = C.contiguous().clone()
        return cls(C, center_h(C), torch.zeros(acc_size(K, D), dtype=torch.int64, device=dev),
                   torch.zeros(2, dtype=torch.int32, device=dev),
                   torch.zeros(max(max_iter, 1), dtype=torch.float64, device=dev),
                   torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(K, dtype=torch.int64, device=dev),
                   torch.empty_like(C))


def new_centers(acc, scale, C) -> torch.Tensor:
    K, D = C.shape
    sums, counts, _ = acc_views(acc, K, D)
    inv = 1.0 / scale.double()
    mean = (sums.double() * inv.view(1, D)) / counts.double().clamp_min(1.0).view(K, 1)
    return torch.where((counts > 0).view(K, 1), mean.float(), C)


def reduce_cost(part: torch.Tensor) -> torch.Tensor:
    """The fixed-order sum of the cost partials: lane t sums partials t, t + 256, ... in order, then the
    halving tree over the 256 lanes (what ``kmeans_update`` does with its 256 threads)."""
    n = part.numel()
    p = torch.zeros(-(-max(n, 1) // 256) * 256, dtype=torch.float64, device=part.device)
    p[:n] = part.reshape(-1)
    p = p.view(-1, 256)
    v = torch.zeros(256, dtype=torch.float64, device=part.device)
    for i in range(p.shape[0]):
        v = v + p[i]
    o = 128
    while o > 0:
        v = v[:o] + v[o:2 * o]
        o >>= 1
    return v[0]


def update_torch(st: FitState, scale, cost, tol2: float, max_iter: int) -> FitState:
    """One Lloyd update on the state, in place; ``cost`` fp64 partials in their reduction order."""
    K, D = st.C.shape
    it, conv = (int(v) for v in st.state.tolist())
    if conv == 0 and it < max_iter:
        Cn = new_centers(st.acc, scale, st.C)
        diff = Cn.double() - st.C.double()
        m2 = torch.zeros(K, dtype=torch.float64, device=st.C.device)
        for f in range(D):
            m2 = m2 + diff[:, f] * diff[:, f]
        moved = m2.max()
        c = reduce_cost(cost)
        st.sizes.copy_(acc_views(st.acc, K, D)[1])
        st.C.copy_(Cn)
        st.h.copy_(center_h(Cn))
        st.cost_hist[it] = c
        st.moved[0] = moved
        st.state[0] = it + 1
        st.state[1] = int(bool(moved <= tol2))
    st.acc.zero_()
    return st


def update_native(st: FitState, scale, cost, tol2: float, max_iter: int) -> FitState:
    K, D = st.C.shape
    check_native_range(K, D)
    if cost.dtype != torch.float64 or st.cost_hist.numel() < max_iter:
        raise ValueError("kmeans update: fp64 cost partials and a history of maxIter entries")
    _native.kernels().kmeans_update(st.acc.data_ptr(), scale.data_ptr(), K, D, cost.data_ptr(), cost.numel(),
                                    int(max_iter), float(tol2), st.C.data_ptr(), st.Cnew.data_ptr(), st.h.data_ptr(),
                                    st.state.data_ptr(), st.cost_hist.data_ptr(), st.moved.data_ptr(),
                                    st.sizes.data_ptr(), _native.stream_ptr())
    return st


def update(st: FitState, scale, cost, tol2: float, max_iter: int, native: Optional[bool] = None) -> FitState:
    native = st.C.is_cuda if native is None else native
    return (update_native if native else update_torch)(st, scale, cost, tol2, max_iter)


# ------------------------------------------------------------------ 3. silhouette
def silhouette_rows_torch(Xc: torch.Tensor, labels: torch.Tensor, K: int) -> torch.Tensor:
    """fp64 [N]: the O(N K) definition from the exact fp64 moments."""
    N, D = Xc.shape
    xd = Xc.double()
    lab = labels.long()
    nrm = (xd * xd).sum(dim=1)
    cnt = torch.bincount(lab, minlength=K).double()
    Y = torch.zeros(K, D, dtype=torch.float64, device=Xc.device).index_add_(0, lab, xd)
    Psi = torch.zeros(K, dtype=torch.float64, device=Xc.device).index_add_(0, lab, nrm)
    nz = cnt.clamp_min(1.0)
    dist = nrm.view(N, 1) + (Psi / nz).view(1, K) - 2.0 * (xd @ (Y / nz.view(K, 1)).t())     # [N, K]
    dist = dist.clamp_min(0.0)
    own = torch.nn.functional.one_hot(lab, K).bool()
    na = cnt[lab]
    a = dist.gather(1, lab.view(N, 1)).squeeze(1) * na / (na - 1.0).clamp_min(1.0)
    other = torch.where(own | (cnt <= 0).view(1, K), torch.full_like(dist, float("inf")), dist)
    b = other.min(dim=1).values
    mx = torch.maximum(a, b)
    ok = (na > 1) & torch.isfinite(b) & (mx > 0)
    return torch.where(ok, (b - a) / torch.where(ok, mx, torch.ones_like(mx)), torch.zeros_like(mx))


def silhouette_operands(acc, scale, nscale, K: int, D: int):
    """(cluster means fp32 [K, D], h = Psi / (2 N) fp32 [K], sizes fp64 [K]) from the integer moments."""
    sums, counts, norms = acc_views(acc, K, D)
    cnt = counts.double()
    nz = cnt.clamp_min(1.0)
    M = ((sums.double() / scale.double().view(1, D)) / nz.view(K, 1)).float().contiguous()
    hp = (norms.double() / nscale.double() / nz * 0.5).float().contiguous()
    return M, hp, cnt.contiguous()


def silhouette_native(Xc, labels, K: int, rows_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mean silhouette (fp64 scalar tensor on the device) through the kernels: the integer moments by
    the given-labels accumulation, then the product with the silhouette epilogue."""
    N, D = Xc.shape
    check_native_range(K, D)
    _f32c(Xc, "rows")
    mod = _native.kernels()
    lab = labels.to(torch.int32).contiguous()
    scale = feature_scales(Xc)
    nscale = norm_scale(row_norms(Xc))
    acc = accumulate_native(Xc, lab, None, scale, nscale, K)
    M, hp, cnt = silhouette_operands(acc, scale, nscale, K, D)
    part = torch.zeros(max(1, -(-N // mod.kmeans_rows_per_block())), dtype=torch.float64, device=Xc.device)
    mod.kmeans_silhouette(Xc.data_ptr(), N, D, K, M.data_ptr(), hp.data_ptr(), lab.data_ptr(), cnt.data_ptr(),
                          _native.ptr(rows_out), part.data_ptr(), _native.stream_ptr())
    return part.sum() / max(N, 1)


def silhouette(X: torch.Tensor, labels: torch.Tensor, K: int, native: Optional[bool] = None) -> torch.Tensor:
    """Mean squared-Euclidean silhouette of ``labels`` (in [0, K)) over the rows of ``X`` (fp64 scalar tensor)."""
    native = X.is_cuda if native is None else native
    Xc = (X.float() - column_means(X.float()).view(1, -1)).contiguous()
    if native:
        return silhouette_native(Xc, labels, K)
    return silhouette_rows_torch(Xc, labels, K).mean() if X.shape[0] else torch.zeros((), dtype=torch.float64)
