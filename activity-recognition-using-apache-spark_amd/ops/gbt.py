"""Gradient-boosted trees: the five per-round operations, each defined ONCE here as PyTorch code.

That code is the CPU path and the oracle of the HIP kernels in ``csrc/kernels/gbt.hip``; every
``*_torch`` function has a ``*_native`` front-end, and the plain names dispatch on the tensors'
device (a GPU tensor REQUIRES the kernels, as everywhere in the project).

Objective: multinomial softmax log-loss, Newton boosting.  Round m grows K regression trees in lock
step (one per class) over the shared uint8 feature-major bins.  Trees are stored in heap order
(children of node n are 2n + 1 and 2n + 2, level d = nodes [2^d - 1, 2^(d+1) - 1)).

Fixed point: the per-row derivatives g = w (p_k - [y = k]) and h = w max(p_k (1 - p_k), 1e-16) are
rounded to int32 multiples of 2^-20 (``rint``) before anything is summed.  Histograms, node totals and
the prefix sums of the split search are therefore exact integer sums — independent of the order of
the adds — so fits are bitwise reproducible and the histogram / split kernels equal these
definitions bit for bit.  The gain

    gain = 1/2 [GL^2 / (HL + lambda) + GR^2 / (HR + lambda) - G^2 / (H + lambda)]

is evaluated in fp64 from the integers (scaled by 2^-20) in one fixed operation order without fused
multiply-adds: ``score(G, H) = (g * g) / (h + lambda)``, ``gain = 0.5 * ((sl + sr) - sp)``.

Histogram cells carry three channels (sum g, sum h, rows of nonzero weight): the row count is what
``minInstancesPerNode`` is checked against (h can round to 0, so it cannot stand in for a count).
Node totals are the sums over the bins of feature 0.  A cut "bin <= b" (b < nbins[f] - 1) is valid
when both children hold >= minInstancesPerNode rows of nonzero weight, both H + lambda are positive
and gain > minInfoGain; ties go to the lowest feature, then the lowest bin.
Leaf value = -stepSize * (G / (H + lambda)) (0 when H + lambda is not positive).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native, rng

QBITS = 20
Q = float(1 << QBITS)
INV_Q = 1.0 / Q
HESS_FLOOR = 1e-16
HCH = 3                      # histogram channels: g, h, rows of nonzero weight
MAX_CLASSES = 32             # gbt.hip: one lane per (row, class), a row within 32 lanes
MAX_DEPTH = 6                # gbt.hip: a level's LDS histogram [2^level][features][bins][3]
MAX_BINS = 64                # gbt.hip: one lane per bin in the split search
MAX_ROWS = (1 << 26) - 1024   # gbt.hip: at most 65,535 row chunks of 1,024 rows on grid.y


def check_native_range(max_depth: int, max_bins: int, num_classes: int):
    if not 1 <= int(max_depth) <= MAX_DEPTH:
        raise ValueError(f"GBT maxDepth must be in 1..{MAX_DEPTH}, got {max_depth}")
    if not 2 <= int(max_bins) <= MAX_BINS:
        raise ValueError(f"GBT maxBins must be in 2..{MAX_BINS}, got {max_bins}")
    if not 2 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"GBT takes 2..{MAX_CLASSES} classes, got {num_classes}")


@dataclass
class GBTArrays:
    """Node arrays of T trees in heap order, [T, maxn] (stats [T, maxn, K]: the leaf value at the
    tree's class t % K, 0 elsewhere — the layout ``har_forest_predict`` sums)."""
    feature: torch.Tensor    # int32, -1 = leaf
    split_bin: torch.Tensor  # int32
    thresh: torch.Tensor     # float32
    left: torch.Tensor       # int32
    right: torch.Tensor      # int32
    gains: torch.Tensor      # float32
    value: torch.Tensor      # float32 leaf value of every node
    stats: torch.Tensor      # float32 [T, maxn, K]

    @classmethod
    def alloc(cls, T: int, max_depth: int, K: int, device) -> "GBTArrays":
        maxn = (1 << (max_depth + 1)) - 1
        i32 = dict(dtype=torch.int32, device=device)
        f32 = dict(dtype=torch.float32, device=device)
        return cls(torch.full((T, maxn), -1, **i32), torch.zeros(T, maxn, **i32), torch.zeros(T, maxn, **f32),
                   torch.zeros(T, maxn, **i32), torch.zeros(T, maxn, **i32), torch.zeros(T, maxn, **f32),
                   torch.zeros(T, maxn, **f32), torch.zeros(T, maxn, K, **f32))

    @property
    def maxn(self) -> int:
        return int(self.feature.shape[1])


@dataclass
class SplitResult:
    """The decisions of one level, [K, 2^level]: feat -1 = leaf; sums = GL, HL, CL, G, H, C (int64)."""
    feat: torch.Tensor
    bin: torch.Tensor
    gain: torch.Tensor   # float64, -inf = no valid cut
    sums: torch.Tensor   # int64 [K, nodes, 6]


# ------------------------------------------------------------------ subsample weights
def round_weights(seed: int, rnd: int, N: int, rate: float, device, row_offset: int = 0) -> Optional[torch.Tensor]:
    """0/1 Bernoulli(rate) weights of boosting round ``rnd`` (int32 [N]; None = every row): the Philox
    row stream keyed by (seed, round, global row id), the table of ``rng.bernoulli_thresholds``."""
    if rate >= 1.0:
        return None
    thr = rng.bernoulli_thresholds(rate)
    stream = rng.STREAM_BOOTSTRAP_BASE + int(rnd)
    if torch.device(device).type == "cuda":
        thr_t = torch.from_numpy(thr.astype(np.uint32).view(np.int32)).to(device)
        out = torch.empty(N, dtype=torch.int32, device=device)
        _native.kernels().philox_buckets(seed, stream, row_offset, N, thr_t.data_ptr(), 1, out.data_ptr(),
                                         _native.stream_ptr())
        return out
    w = rng.bootstrap_weights(seed, [rnd], N, row_offset, thr)[0]
    return torch.from_numpy(w.astype(np.int32)).to(device)


# ------------------------------------------------------------------ 1. derivatives
def grad_float(margins: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor] = None):
    """fp64 g, h [K, N] and the summed log-loss (over ALL rows, unweighted) of fp32 margins [N, K]."""
    m = margins.double()
    N, K = m.shape
    mx = m.max(dim=1, keepdim=True).values
    e = torch.exp(m - mx)
    se = e.sum(dim=1, keepdim=True)
    p = e / se
    onehot = torch.nn.functional.one_hot(y.long().clamp(0, K - 1), K).to(p.dtype) * ((y >= 0) & (y < K)).view(-1, 1)
    g = p - onehot
    h = (p * (1.0 - p)).clamp_min(HESS_FLOOR)
    if w is not None:
        on = (w != 0).view(-1, 1)
        g = torch.where(on, g, torch.zeros_like(g))
        h = torch.where(on, h, torch.zeros_like(h))
    loss = (((torch.log(se) + mx) - m) * onehot).sum()
    return g.t().contiguous(), h.t().contiguous(), loss


def quantize(v: torch.Tensor) -> torch.Tensor:
    """rint(v * 2^20) as int32 (round half to even)."""
    return torch.round(v.double() * Q).to(torch.int32)


def grad_torch(margins, y, w=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """qgh int32 [K, N, 2] and the loss partials (one element here; the kernel writes one per workgroup)."""
    g, h, loss = grad_float(margins, y, w)
    return torch.stack([quantize(g), quantize(h)], dim=-1).contiguous(), loss.reshape(1)


def grad_native(margins, y32, w=None, want_q: bool = True, loss_out: Optional[torch.Tensor] = None):
    mod = _native.kernels()
    N, K = margins.shape
    if not (margins.dtype == torch.float32 and margins.is_contiguous() and y32.dtype == torch.int32):
        raise ValueError("gbt grad: margins fp32 contiguous [N, K], labels int32")
    nb = mod.gbt_grad_blocks(N, K)
    qgh = torch.empty(K, N, 2, dtype=torch.int32, device=margins.device) if want_q else None
    if loss_out is None:
        loss_out = torch.empty(max(nb, 1), dtype=torch.float64, device=margins.device)
    if N == 0:
        loss_out.zero_()
    mod.gbt_grad(margins.data_ptr(), y32.data_ptr(), _native.ptr(w), N, K, _native.ptr(qgh), loss_out.data_ptr(),
                 _native.stream_ptr())
    return qgh, loss_out


def grad(margins, y32, w=None):
    return grad_native(margins, y32, w) if margins.is_cuda else grad_torch(margins, y32, w)


# ------------------------------------------------------------------ 2. level histograms
def hist_torch(bins, qgh, w, node_of, level: int, max_bins: int) -> torch.Tensor:
    """int64 [K, 2^level, F, max_bins, 3]: sums of (g, h, [w != 0]) of the rows sitting in the level's nodes."""
    F, N = bins.shape
    K = qgh.shape[0]
    nodes, first = 1 << level, (1 << level) - 1
    dev = bins.device
    nd = node_of.long() - first                                   # [K, N]
    valid = (nd >= 0) & (nd < nodes)
    cnt = torch.ones(N, dtype=torch.int64, device=dev) if w is None else (w != 0).long()
    vals = torch.cat([qgh.long(), cnt.view(1, N, 1).expand(K, N, 1)], dim=-1)   # [K, N, 3]
    b = bins.long()                                               # [F, N]
    kk = torch.arange(K, device=dev).view(K, 1, 1)
    ff = torch.arange(F, device=dev).view(1, F, 1)
    flat = ((kk * nodes + nd.clamp(0, nodes - 1).view(K, 1, N)) * F + ff) * max_bins + b.view(1, F, N)   # [K, F, N]
    ok = valid.view(K, 1, N) & (b < max_bins).view(1, F, N)
    hist = torch.zeros(K * nodes * F * max_bins, HCH, dtype=torch.int64, device=dev)
    hist.index_add_(0, flat[ok], vals.view(K, 1, N, HCH).expand(K, F, N, HCH)[ok])
    return hist.view(K, nodes, F, max_bins, HCH)


def hist_native(bins, qgh, w, node_of, level: int, max_bins: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    F, N = bins.shape
    K = qgh.shape[0]
    nodes = 1 << level
    if out is None:
        out = torch.empty(K, nodes, F, max_bins, HCH, dtype=torch.int64, device=bins.device)
    _native.kernels().gbt_hist(bins.data_ptr(), qgh.data_ptr(), _native.ptr(w), node_of.data_ptr(), N, F, K, max_bins,
                               level, out.data_ptr(), _native.stream_ptr())
    return out


# ------------------------------------------------------------------ 3. split search + commit
def _score(G: torch.Tensor, H: torch.Tensor, lam: float):
    g = G.double() * INV_Q
    d = H.double() * INV_Q + lam
    pos = d > 0
    return torch.where(pos, (g * g) / torch.where(pos, d, torch.ones_like(d)), torch.zeros_like(d)), pos


def leaf_value(G: torch.Tensor, H: torch.Tensor, lam: float, step: float) -> torch.Tensor:
    g = G.double() * INV_Q
    d = H.double() * INV_Q + lam
    pos = d > 0
    return torch.where(pos, -(step * (g / torch.where(pos, d, torch.ones_like(d)))), torch.zeros_like(d)).float()


def split_torch(hist, nbins, lam: float, min_inst: int, min_gain: float) -> SplitResult:
    K, nodes, F, B, _ = hist.shape
    dev = hist.device
    lanes = torch.arange(B, device=dev)
    nb = nbins.long().clamp(1, B)
    inb = (lanes.view(1, B) < nb.view(F, 1))                      # [F, B]
    hm = hist * inb.view(1, 1, F, B, 1).long()
    tot = hm[:, :, 0].sum(dim=2)                                  # [K, nodes, 3] (feature 0)
    G, H, C = (tot[..., c].view(K, nodes, 1, 1) for c in range(3))
    cum = hm.cumsum(dim=3)
    GL, HL, CL = cum[..., 0], cum[..., 1], cum[..., 2]            # [K, nodes, F, B]
    sp, _ = _score(G, H, lam)
    sl, lpos = _score(GL, HL, lam)
    sr, rpos = _score(G - GL, H - HL, lam)
    gain = 0.5 * ((sl + sr) - sp)
    valid = ((lanes.view(1, B) < (nb - 1).view(F, 1)).view(1, 1, F, B) & (CL >= min_inst) & ((C - CL) >= min_inst)
             & lpos & rpos & (gain > min_gain))
    neg = torch.full_like(gain, float("-inf"))
    gv = torch.where(valid, gain, neg).view(K, nodes, F * B)
    best = torch.argmax(gv, dim=2)                                # first maximum: lowest feature, then lowest bin
    bg = gv.gather(2, best.unsqueeze(-1)).squeeze(-1)
    split = torch.isfinite(bg)
    f, b = best // B, best % B
    pick = lambda t: t.reshape(K, nodes, F * B).gather(2, best.unsqueeze(-1)).squeeze(-1)
    zero = torch.zeros(K, nodes, dtype=torch.int64, device=dev)
    sums = torch.stack([torch.where(split, pick(GL), zero), torch.where(split, pick(HL), zero),
                        torch.where(split, pick(CL), zero), tot[..., 0], tot[..., 1], tot[..., 2]], dim=-1)
    return SplitResult(torch.where(split, f, torch.full_like(f, -1)).to(torch.int32),
                       torch.where(split, b, torch.zeros_like(b)).to(torch.int32), bg, sums.contiguous())


def commit_torch(res: SplitResult, arrs: GBTArrays, level: int, tree0: int, thr_mat, lam: float, step: float):
    """Write the level's decisions into trees tree0 .. tree0 + K - 1 (what the split kernel does itself)."""
    K, nodes = res.feat.shape
    dev = res.feat.device
    first = nodes - 1
    t = (tree0 + torch.arange(K, device=dev)).view(K, 1).expand(K, nodes)
    n = (first + torch.arange(nodes, device=dev)).view(1, nodes).expand(K, nodes)
    kk = torch.arange(K, device=dev).view(K, 1).expand(K, nodes)
    GL, HL, G, H = res.sums[..., 0], res.sums[..., 1], res.sums[..., 3], res.sums[..., 4]
    split = res.feat >= 0
    if level == 0:
        v = leaf_value(G, H, lam, step)
        arrs.value[t, n] = v
        arrs.stats[t, n, kk] = v
    f = res.feat.long().clamp_min(0)
    b = res.bin.long()
    arrs.feature[t, n] = res.feat
    arrs.split_bin[t, n] = res.bin
    arrs.thresh[t, n] = torch.where(split, thr_mat[f, b.clamp(0, thr_mat.shape[1] - 1)], torch.zeros_like(res.gain).float())
    arrs.left[t, n] = torch.where(split, 2 * n + 1, torch.zeros_like(n)).to(torch.int32)
    arrs.right[t, n] = torch.where(split, 2 * n + 2, torch.zeros_like(n)).to(torch.int32)
    arrs.gains[t, n] = torch.where(split, res.gain, torch.zeros_like(res.gain)).float()
    ts, ns, ks = t[split], n[split], kk[split]
    vl = leaf_value(GL, HL, lam, step)[split]
    vr = leaf_value(G - GL, H - HL, lam, step)[split]
    arrs.value[ts, 2 * ns + 1] = vl
    arrs.value[ts, 2 * ns + 2] = vr
    arrs.stats[ts, 2 * ns + 1, ks] = vl
    arrs.stats[ts, 2 * ns + 2, ks] = vr


def split_native(hist, nbins, thr_mat, arrs: GBTArrays, level: int, tree0: int, lam: float, step: float,
                 min_inst: int, min_gain: float, out: Optional[SplitResult] = None) -> SplitResult:
    """Split search AND commit of one level in one launch."""
    K, nodes, F, B, _ = hist.shape
    dev = hist.device
    if out is None:
        out = SplitResult(torch.empty(K, nodes, dtype=torch.int32, device=dev),
                          torch.empty(K, nodes, dtype=torch.int32, device=dev),
                          torch.empty(K, nodes, dtype=torch.float64, device=dev),
                          torch.empty(K, nodes, 6, dtype=torch.int64, device=dev))
    a = arrs
    _native.kernels().gbt_split(hist.data_ptr(), nbins.data_ptr(), thr_mat.data_ptr(), F, K, B, thr_mat.shape[1], level,
                                tree0, a.maxn, float(lam), float(step), float(min_gain), int(min_inst),
                                out.feat.data_ptr(), out.bin.data_ptr(), out.gain.data_ptr(), out.sums.data_ptr(),
                                a.feature.data_ptr(), a.split_bin.data_ptr(), a.thresh.data_ptr(), a.left.data_ptr(),
                                a.right.data_ptr(), a.gains.data_ptr(), a.value.data_ptr(), a.stats.data_ptr(),
                                _native.stream_ptr())
    return out


# ------------------------------------------------------------------ 4. partition
def partition_torch(node_of, bins, arrs: GBTArrays, level: int, tree0: int) -> torch.Tensor:
    """Rows in a split node of the level move to its child (weight-0 rows too); returns node_of."""
    K, N = node_of.shape
    nodes, first = 1 << level, (1 << level) - 1
    dev = node_of.device
    t = (tree0 + torch.arange(K, device=dev)).view(K, 1).expand(K, N)
    n = node_of.long()
    inlvl = (n >= first) & (n < first + nodes)
    nc = n.clamp(0, arrs.maxn - 1)
    f = arrs.feature[t, nc].long()
    move = inlvl & (f >= 0)
    b = bins[f.clamp_min(0), torch.arange(N, device=dev).view(1, N).expand(K, N)].long()
    child = 2 * n + 1 + (b > arrs.split_bin[t, nc].long()).long()
    return torch.where(move, child, n).to(torch.int32)


def partition_native(node_of, bins, arrs: GBTArrays, level: int, tree0: int) -> torch.Tensor:
    K, N = node_of.shape
    _native.kernels().gbt_partition(node_of.data_ptr(), bins.data_ptr(), arrs.feature.data_ptr(),
                                    arrs.split_bin.data_ptr(), N, bins.shape[0], K, level, tree0, arrs.maxn,
                                    _native.stream_ptr())
    return node_of


# ------------------------------------------------------------------ 5. margin update
def update_torch(margins, node_of, arrs: GBTArrays, tree0: int) -> torch.Tensor:
    K, N = node_of.shape
    t = (tree0 + torch.arange(K, device=node_of.device)).view(K, 1).expand(K, N)
    margins += arrs.value[t, node_of.long()].t()
    return margins


def update_native(margins, node_of, arrs: GBTArrays, tree0: int) -> torch.Tensor:
    K, N = node_of.shape
    _native.kernels().gbt_update(margins.data_ptr(), node_of.data_ptr(), arrs.value.data_ptr(), N, K, tree0, arrs.maxn,
                                 _native.stream_ptr())
    return margins


# ------------------------------------------------------------------ one round
def grow_round(bins, nbins, thr_mat, qgh, w, arrs: GBTArrays, tree0: int, max_depth: int, max_bins: int, lam: float,
               step: float, min_inst: int, min_gain: float, native: Optional[bool] = None, node_of=None,
               hist_buf=None) -> torch.Tensor:
    """Grow the K trees of one round from the quantized derivatives (level-wise to ``max_depth``); returns
    node_of [K, N] = the leaf of every training row.  ``native`` defaults to the tensors' device: on a GPU
    every level is three launches (histogram, split + commit, partition) and nothing is read back."""
    native = bins.is_cuda if native is None else native
    K, N = qgh.shape[0], qgh.shape[1]
    F = bins.shape[0]
    if node_of is None:
        node_of = torch.zeros(K, N, dtype=torch.int32, device=bins.device)
    else:
        node_of.zero_()
    for level in range(max_depth):
        if native:
            out = None
            if hist_buf is not None:
                out = hist_buf[:K * (1 << level) * F * max_bins * HCH].view(K, 1 << level, F, max_bins, HCH)
            hist = hist_native(bins, qgh, w, node_of, level, max_bins, out=out)
            split_native(hist, nbins, thr_mat, arrs, level, tree0, lam, step, min_inst, min_gain)
            node_of = partition_native(node_of, bins, arrs, level, tree0)
        else:
            hist = hist_torch(bins, qgh, w, node_of, level, max_bins)
            res = split_torch(hist, nbins, lam, min_inst, min_gain)
            commit_torch(res, arrs, level, tree0, thr_mat, lam, step)
            node_of = partition_torch(node_of, bins, arrs, level, tree0)
    return node_of


def update(margins, node_of, arrs: GBTArrays, tree0: int, native: Optional[bool] = None):
    native = margins.is_cuda if native is None else native
    return (update_native if native else update_torch)(margins, node_of, arrs, tree0)
