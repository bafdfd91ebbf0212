"""Gaussian mixtures (EM, full or diagonal covariances): every operation defined ONCE here as PyTorch code.

That code is the CPU path and the oracle of the HIP kernels in ``csrc/kernels/gmm.hip``; every ``*_torch``
function has a ``*_native`` front-end, and the plain names dispatch on the tensors' device (a GPU tensor
REQUIRES the kernels, as everywhere in the project).

Working rows.  ``Z = (X - mean) * inv_std`` in fp32, with the fp32 column means and (population) standard
deviations from fp64 sums, rounded once; a constant column gets ``inv_std = 1`` (and ``std = 1``).  A
full-covariance mixture is affine invariant, so standardising is free in exact arithmetic; it keeps the
fp32 products well scaled on mixed-scale columns.  Models keep ``mean`` and ``std`` and report means and
covariances in the original coordinates.

Component operands.  For component k: ``mu_k`` fp32 [D], ``W_k = L_k^{-T}`` fp32 [D, D] (upper triangular,
``Sigma_k = L_k L_k^T``, Cholesky in fp64) and ``c_k = log pi_k - (D/2) log 2pi - sum_i log L_k[i, i]`` in
fp32; ``c_k = -inf`` for a zero weight.

E-step.  ``d = z_n - mu_k``, ``y = d W_k``, ``q[n, k] = sum_j y_j^2``, ``t = c_k - q / 2``,
``lse[n] = logsumexp_k t``, ``r[n, k] = exp(t - lse)``; the prediction is the argmax of r, TIES GO TO THE
LOWEST k.  The oracle evaluates in fp64 from the fp32 operands; the kernel runs ``d W_k`` on
``v_mfma_f32_16x16x4_f32`` (d by one fp32 subtract) and the epilogue in fp32 as ``m = max t``,
``e = exp(t - m)``, ``s = sum e``, ``lse = m + log s``, ``r = e / s``, prediction = the first argmax of r.

Moments.  Rows have fp32 weights ``w >= 0`` (1 without a weight vector); the moments are taken about the
OLD mean: ``N_k = sum w r``, ``S1_k = sum w r d`` [D], ``S2_k = sum w r d d^T`` [D, D].  Centring on the old
mean leaves ``Sigma`` below without an ``E[xx^T] - mu mu^T`` cancellation: the correction term vanishes as
EM converges.  A workgroup of the kernel's persistent grid keeps its accumulators in LDS across its row
tiles and stores one fp32 slab ``[K][1 + Dp + Dp*Dp]`` (Dp = D rounded up to 4; S2 valid for i <= j) at its
end; ``reduce_slabs`` sums the slabs in order in fp64.

Finish (per component, fp64).  ``delta = S1 / N_k``, ``mu_new = mu + delta``,
``Sigma = S2 / N_k - delta delta^T + regCovar * I`` in working coordinates (``diag``: the off-diagonal
entries are zeroed here, nothing else differs), ``pi_k = N_k / sum N``; then the Cholesky factor L,
``W = L^{-T}`` and ``c_k``.  A component with ``N_k = 0``, or one that meets a non-positive or non-finite
pivot, keeps its mu and W (its c is rebuilt from the kept factor: ``sum log L_ii = -sum log W_ii``); its
weight is still ``N_k / sum N``.

Control.  ``loglik = sum_n w_n lse[n]``: fp64 per-workgroup partials reduced in the fixed order of
``ops.kmeans.reduce_cost``.  ``hist[it] = loglik``; the fit has converged when
``|loglik - loglik_prev| <= tol`` (Spark's rule, on the total).  Once converged, or after ``maxIter``
iterations, further steps leave the state untouched.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native, rng
from .kmeans import reduce_cost

MAX_K = 64                  # gmm.hip: components
MAX_D = 128                 # gmm.hip: features (an fp64 D x D factor fits the LDS)
MAX_ROWS = (1 << 31) - 64   # gmm.hip: 32-bit row tiles
LOG_2PI = math.log(2.0 * math.pi)


def check_native_range(k: int, D: int, N: Optional[int] = None):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"GaussianMixture takes k in 1..{MAX_K}, got {k}")
    if not 1 <= int(D) <= MAX_D:
        raise ValueError(f"GaussianMixture takes 1..{MAX_D} features, got {D}")
    if N is not None and not 1 <= int(N) <= MAX_ROWS:
        raise ValueError(f"GaussianMixture takes 1..{MAX_ROWS} rows, got {N}")


def rows_per_block() -> int:
    """Rows of a ``gmm_estep`` tile (the tests place their shapes around it)."""
    return int(_native.kernels().gmm_rows_per_block())


def grid(N: int, D: int, K: int, max_blocks: int = 0) -> int:
    """Workgroups (= moment slabs = log-likelihood partials) of a ``gmm_estep`` launch."""
    return int(_native.kernels().gmm_grid(int(N), int(D), int(K), int(max_blocks)))


def group(D: int, K: int) -> int:
    """Components whose moment accumulators a ``gmm_estep`` workgroup keeps in LDS at a time (K: one pass
    over the rows; fewer: one pass per group, the later ones reading w r back from a scratch)."""
    return int(_native.kernels().gmm_group(int(D), int(K)))


def padded(D: int) -> int:
    return (int(D) + 3) // 4 * 4


def slab_size(D: int) -> int:
    Dp = padded(D)
    return 1 + Dp + Dp * Dp


# ------------------------------------------------------------------ working rows
def standardizer(X: torch.Tensor):
    """(mean, std, inv_std) fp32 [D] from fp64 sums; a constant column has std = inv_std = 1."""
    xd = X.double()
    n = max(X.shape[0], 1)
    mean = xd.sum(dim=0) / n
    var = ((xd - mean.view(1, -1)) ** 2).sum(dim=0) / n
    sd = var.sqrt()
    sd = torch.where((sd > 0) & torch.isfinite(sd), sd, torch.ones_like(sd))
    return mean.float(), sd.float(), (1.0 / sd).float()


def working_rows(X: torch.Tensor, mean: torch.Tensor, inv_std: torch.Tensor) -> torch.Tensor:
    return ((X.float() - mean.view(1, -1)) * inv_std.view(1, -1)).contiguous()


def random_init_rows(seed: int, k: int, n_rows: int) -> np.ndarray:
    """Ids of the k rows with the smallest Philox keys of ``STREAM_GMM_INIT``, by ascending key."""
    ids = np.arange(n_rows, dtype=np.uint64)
    keys = (rng.uniform_u32(seed, rng.STREAM_GMM_INIT, ids).astype(np.uint64) << np.uint64(32)) | ids
    return (np.sort(keys)[:k] & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ------------------------------------------------------------------ operands
def component_c(pi: torch.Tensor, logdet_l: torch.Tensor, D: int) -> torch.Tensor:
    """fp32 [K]: log pi - D/2 log 2pi - sum log L_ii (fp64 arithmetic; pi = 0 gives -inf)."""
    return (torch.log(pi.double()) - 0.5 * D * LOG_2PI - logdet_l.double()).float()


def operands(mu: torch.Tensor, Sigma: torch.Tensor, pi: torch.Tensor):
    """(mu fp32 [K, D], W fp32 [K, D, D], c fp32 [K]) of means, covariances and weights."""
    K, D = mu.shape
    L = torch.linalg.cholesky(Sigma.double())
    eye = torch.eye(D, dtype=torch.float64, device=mu.device).expand(K, D, D)
    W = torch.linalg.solve_triangular(L, eye, upper=False).transpose(-1, -2)
    logdet = torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(dim=1)
    return mu.float().contiguous(), W.float().contiguous(), component_c(pi, logdet, D)


# ------------------------------------------------------------------ 1. E-step + moments
@dataclass
class EstepResult:
    q: Optional[torch.Tensor] = None       # [N, K]
    resp: Optional[torch.Tensor] = None    # [N, K]
    lse: Optional[torch.Tensor] = None     # [N]
    pred: Optional[torch.Tensor] = None    # int32 [N]
    Nk: Optional[torch.Tensor] = None      # fp64 [K]
    S1: Optional[torch.Tensor] = None      # fp64 [K, D]
    S2: Optional[torch.Tensor] = None      # fp64 [K, D, D]
    part: Optional[torch.Tensor] = None    # fp64 log-likelihood partials (one here; one per workgroup)
    slabs: Optional[torch.Tensor] = None   # fp32 [G, K, slab] (kernel only)

    @property
    def loglik(self) -> torch.Tensor:
        return reduce_cost(self.part)


def q_torch(Z, mu, W, dtype=torch.float64) -> torch.Tensor:
    """[N, K] squared Mahalanobis distances, evaluated in ``dtype`` from the fp32 operands."""
    Zd = Z.to(dtype)
    cols = []
    for k in range(mu.shape[0]):
        y = (Zd - mu[k].to(dtype).view(1, -1)) @ W[k].to(dtype)
        cols.append((y * y).sum(dim=1))
    return torch.stack(cols, dim=1)


def softmax_torch(q, c, dtype=torch.float64):
    """(t, lse, r, pred int32) of q [N, K] and c [K]; the first argmax."""
    t = c.to(dtype).view(1, -1) - 0.5 * q.to(dtype)
    lse = torch.logsumexp(t, dim=1)
    r = torch.exp(t - lse.view(-1, 1))
    return t, lse, r, r.argmax(dim=1).to(torch.int32)


def moments_torch(Z, mu, r, w=None):
    """fp64 (N_k [K], S1 [K, D], S2 [K, D, D]) about ``mu`` of the responsibilities ``r``."""
    K, D = mu.shape
    Zd = Z.double()
    wr = r.double() if w is None else r.double() * w.double().view(-1, 1)
    S1 = torch.zeros(K, D, dtype=torch.float64, device=Z.device)
    S2 = torch.zeros(K, D, D, dtype=torch.float64, device=Z.device)
    for k in range(K):
        d = Zd - mu[k].double().view(1, -1)
        wd = d * wr[:, k].view(-1, 1)
        S1[k] = wd.sum(dim=0)
        S2[k] = wd.t() @ d
    return wr.sum(dim=0), S1, S2


def estep_torch(Z, mu, W, c, w=None, want_moments=True, dtype=torch.float64) -> EstepResult:
    q = q_torch(Z, mu, W, dtype)
    _, lse, r, pred = softmax_torch(q, c, dtype)
    wl = lse.double() if w is None else lse.double() * w.double()
    out = EstepResult(q, r, lse, pred, part=wl.sum().reshape(1))
    if want_moments:
        out.Nk, out.S1, out.S2 = moments_torch(Z, mu, r, w)
    return out


def reduce_slabs(slabs: torch.Tensor, K: int, D: int):
    """fp64 (N_k, S1, S2) of the kernel's slabs [G, K, slab]: summed in slab order, S2 mirrored from its
    upper triangle."""
    Dp = padded(D)
    s = torch.zeros(K, slab_size(D), dtype=torch.float64, device=slabs.device)
    for g in range(slabs.shape[0]):
        s = s + slabs[g].double()
    S2 = s[:, 1 + Dp:].view(K, Dp, Dp)[:, :D, :D]
    up = torch.triu(S2)
    return s[:, 0].clone(), s[:, 1:1 + D].clone(), up + torch.triu(S2, 1).transpose(-1, -2)


def make_slabs(Nk, S1, S2, nslab: int = 1) -> torch.Tensor:
    """fp32 slabs [nslab, K, slab] that sum to the given moments (equal shares), as ``gmm_finish`` reads them."""
    K, D = S1.shape
    Dp = padded(D)
    s = torch.zeros(K, slab_size(D), dtype=torch.float64, device=S1.device)
    s[:, 0] = Nk
    s[:, 1:1 + D] = S1
    s2 = torch.zeros(K, Dp, Dp, dtype=torch.float64, device=S1.device)
    s2[:, :D, :D] = torch.triu(S2.double())
    s[:, 1 + Dp:] = s2.view(K, Dp * Dp)
    return (s / nslab).float().unsqueeze(0).repeat(nslab, 1, 1).contiguous()


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"gmm: {what} must be fp32 and contiguous")
    return t


def _check_operands(Z, mu, W, c):
    N, D = Z.shape
    K = mu.shape[0]
    check_native_range(K, D)
    _f32c(Z, "rows"), _f32c(mu, "mu"), _f32c(W, "W"), _f32c(c, "c")
    if tuple(mu.shape) != (K, D) or tuple(W.shape) != (K, D, D) or c.numel() != K:
        raise ValueError("gmm: mu [K, D], W [K, D, D] and c [K] must match the rows")
    return N, D, K


def estep_native(Z, mu, W, c, w=None, want_moments=True, want_resp=True, want_q=False, max_blocks: int = 0,
                 slabs_out=None, part_out=None, state=None, max_iter: int = 1) -> EstepResult:
    """The kernel.  ``max_blocks`` (private: the tests) lowers the cap of the persistent grid; with ``state``
    (a fit's {iterations, converged}) the launch does nothing once the fit is over."""
    mod = _native.kernels()
    N, D, K = _check_operands(Z, mu, W, c)
    if w is not None and (w.dtype != torch.float32 or w.numel() != N or not w.is_contiguous()):
        raise ValueError("gmm: weights fp32 [N]")
    dev = Z.device
    G = mod.gmm_grid(N, D, K, int(max_blocks))
    out = EstepResult()
    if want_resp:
        out.resp = torch.empty(N, K, dtype=torch.float32, device=dev)
        out.lse = torch.empty(N, dtype=torch.float32, device=dev)
        out.pred = torch.empty(N, dtype=torch.int32, device=dev)
    if want_q:
        out.q = torch.empty(N, K, dtype=torch.float32, device=dev)
    if want_moments:
        out.slabs = torch.empty(G, K, slab_size(D), dtype=torch.float32, device=dev) if slabs_out is None else slabs_out
        if out.slabs.shape[0] != G:
            raise ValueError(f"gmm: {G} moment slabs")
    wr = None
    if want_moments and mod.gmm_group(D, K) < K:     # component groups: the w r scratch of the later passes
        wr = torch.empty(N, K, dtype=torch.float32, device=dev)
    out.part = torch.zeros(G, dtype=torch.float64, device=dev) if part_out is None else part_out
    if out.part.numel() != G:
        raise ValueError(f"gmm: {G} log-likelihood partials")
    mod.gmm_estep(Z.data_ptr(), N, D, K, mu.data_ptr(), W.data_ptr(), c.data_ptr(), _native.ptr(w),
                  _native.ptr(out.resp), _native.ptr(out.lse), _native.ptr(out.pred), _native.ptr(out.q),
                  _native.ptr(out.slabs), out.part.data_ptr(), int(max_blocks), _native.ptr(state), int(max_iter),
                  _native.ptr(wr), _native.stream_ptr())
    return out


def estep(Z, mu, W, c, w=None, native: Optional[bool] = None, **kw) -> EstepResult:
    native = Z.is_cuda if native is None else native
    if native:
        return estep_native(Z, mu, W, c, w, **kw)
    return estep_torch(Z, mu, W, c, w, want_moments=kw.get("want_moments", True))


# ------------------------------------------------------------------ 2. finish
@dataclass
class FinishResult:
    mu: torch.Tensor       # fp32 [K, D]
    W: torch.Tensor        # fp32 [K, D, D]
    c: torch.Tensor        # fp32 [K]
    Nk: torch.Tensor       # fp64 [K]
    pi: torch.Tensor       # fp64 [K]
    mu64: Optional[torch.Tensor] = None     # the oracle's unrounded values
    Sigma: Optional[torch.Tensor] = None    # fp64 [K, D, D] working coordinates (kept components: NaN-free junk)
    W64: Optional[torch.Tensor] = None
    updated: Optional[torch.Tensor] = None  # bool [K]


def finish_torch(Nk, S1, S2, mu, W, reg: float, diag: bool = False) -> FinishResult:
    K, D = mu.shape
    dev = mu.device
    Nk = Nk.double()
    ntot = Nk.sum()
    pi = torch.where(ntot > 0, Nk / ntot.clamp_min(1e-300), torch.zeros_like(Nk))
    live = Nk > 0
    nz = torch.where(live, Nk, torch.ones_like(Nk))
    delta = S1.double() / nz.view(K, 1)
    eye = torch.eye(D, dtype=torch.float64, device=dev)
    Sigma = S2.double() / nz.view(K, 1, 1) - delta.unsqueeze(2) * delta.unsqueeze(1)
    if diag:
        Sigma = Sigma * eye
    Sigma = Sigma + float(reg) * eye
    Sigma = torch.where(live.view(K, 1, 1) & torch.isfinite(Sigma).all(dim=2).all(dim=1).view(K, 1, 1), Sigma,
                        eye.expand(K, D, D))
    L, info = torch.linalg.cholesky_ex(Sigma)
    ok = live & (info == 0).to(dev) & torch.isfinite(L).all(dim=2).all(dim=1)
    L = torch.where(ok.view(K, 1, 1), L, eye.expand(K, D, D))
    Wn = torch.linalg.solve_triangular(L, eye.expand(K, D, D), upper=False).transpose(-1, -2)
    W64 = torch.where(ok.view(K, 1, 1), Wn, W.double())
    mu64 = torch.where(ok.view(K, 1), mu.double() + delta, mu.double())
    logdet = torch.where(ok, torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(dim=1),
                         -torch.log(torch.diagonal(W.double(), dim1=-2, dim2=-1)).sum(dim=1))
    return FinishResult(mu64.float().contiguous(), W64.float().contiguous(), component_c(pi, logdet, D), Nk, pi,
                        mu64, Sigma, W64, ok)


def finish_native(slabs, mu, W, c, Nk, pi, reg: float, diag: bool = False, state=None, max_iter: int = 1):
    """``gmm_finish`` on the slabs [G, K, slab]; mu, W, c, Nk, pi are updated in place."""
    K, D = mu.shape
    check_native_range(K, D)
    _f32c(slabs, "slabs"), _f32c(mu, "mu"), _f32c(W, "W"), _f32c(c, "c")
    if slabs.dim() != 3 or tuple(slabs.shape[1:]) != (K, slab_size(D)):
        raise ValueError("gmm: slabs [G, K, 1 + Dp + Dp * Dp]")
    if Nk.dtype != torch.float64 or pi.dtype != torch.float64:
        raise ValueError("gmm: fp64 N_k and weights")
    _native.kernels().gmm_finish(slabs.data_ptr(), int(slabs.shape[0]), K, D, int(bool(diag)), int(max_iter),
                                 float(reg), mu.data_ptr(), W.data_ptr(), c.data_ptr(), Nk.data_ptr(), pi.data_ptr(),
                                 _native.ptr(state), _native.stream_ptr())


# ------------------------------------------------------------------ 3. the EM step
@dataclass
class FitState:
    """Device-resident state of one fit (what ``gmm_finish`` and ``gmm_control`` read and write)."""
    mu: torch.Tensor      # float32 [K, D]
    W: torch.Tensor       # float32 [K, D, D]
    c: torch.Tensor       # float32 [K]
    Nk: torch.Tensor      # float64 [K]
    pi: torch.Tensor      # float64 [K]
    state: torch.Tensor   # int32 [2]: iterations, converged
    hist: torch.Tensor    # float64 [maxIter]

    @classmethod
    def alloc(cls, mu, W, c, pi, max_iter: int) -> "FitState":
        dev = mu.device
        K = mu.shape[0]
        return cls(mu.float().contiguous().clone(), W.float().contiguous().clone(), c.float().contiguous().clone(),
                   torch.zeros(K, dtype=torch.float64, device=dev), pi.double().contiguous().clone(),
                   torch.zeros(2, dtype=torch.int32, device=dev),
                   torch.zeros(max(max_iter, 1), dtype=torch.float64, device=dev))


def step_torch(st: FitState, Z, w, reg: float, diag: bool, tol: float, max_iter: int, dtype=torch.float64):
    """One EM iteration on the state, in place (reads the state: the CPU path)."""
    it, conv = (int(v) for v in st.state.tolist())
    if conv or it >= max_iter:
        return st
    e = estep_torch(Z, st.mu, st.W, st.c, w, True, dtype)
    f = finish_torch(e.Nk, e.S1, e.S2, st.mu, st.W, reg, diag)
    st.mu.copy_(f.mu), st.W.copy_(f.W), st.c.copy_(f.c), st.Nk.copy_(f.Nk), st.pi.copy_(f.pi)
    ll = e.loglik.double()
    st.hist[it] = ll
    st.state[0] = it + 1
    st.state[1] = int(it > 0 and bool((ll - st.hist[it - 1]).abs() <= tol))
    return st


def step_native(st: FitState, Z, w, reg: float, diag: bool, tol: float, max_iter: int, slabs, part,
                max_blocks: int = 0):
    """``gmm_estep`` (moments only) + ``gmm_finish`` + ``gmm_control``: three launches, no host read; all
    three return at once when the state says the fit is over."""
    estep_native(Z, st.mu, st.W, st.c, w, want_moments=True, want_resp=False, max_blocks=max_blocks,
                 slabs_out=slabs, part_out=part, state=st.state, max_iter=max_iter)
    finish_native(slabs, st.mu, st.W, st.c, st.Nk, st.pi, reg, diag, st.state, max_iter)
    _native.kernels().gmm_control(part.data_ptr(), part.numel(), int(max_iter), float(tol), st.state.data_ptr(),
                                  st.hist.data_ptr(), _native.stream_ptr())
    return st
