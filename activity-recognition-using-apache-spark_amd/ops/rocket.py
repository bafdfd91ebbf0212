"""MiniRocket-style convolutional window features: the definition (float64 torch) and the native front-end.

A window has ``W >= 9`` samples ``x_c[t]`` on ``A`` axes (3, 6 or 9).

* **Kernels**: 84, one per 3-subset ``{a < b < c}`` of the taps ``{0..8}`` in the order of
  ``itertools.combinations(range(9), 3)``; taps are 2 on the subset and -1 elsewhere (they sum to 0).
* **Dilations**: ``d_e = 2^e``, ``e = 0 .. floor(log2((W - 1) / 8))``.
* **Combination** ``(e, k)``: a non-empty axis subset ``mask[e, k]`` (bit ``c`` = axis ``c``) and ``q``
  biases ``b[e, k, 0..q)``.
* **Convolution**: ``C[t] = sum_{c in mask} sum_j w_k[j] x_c[t + (j - 4) d]``, samples outside ``[0, W)``
  being 0.
* **Counted range**: ``[0, W)`` when ``e + k`` is even (padded), ``[4 d, W - 4 d)`` otherwise (valid only);
  its length ``L >= 1``.
* **Feature**: ``fp32(#{t in range : C[t] > b}) / fp32(L)`` (PPV, a strict comparison), in column
  ``(e * 84 + k) * q + i``.

``rocket_counts_torch`` / ``rocket_features_torch`` evaluate this in float64 (the oracle and the CPU path);
``rocket_features_into`` runs the HIP kernel (``rocket.hip``) on device streams.  The weights are integers,
so on integer-valued samples the kernel's fp32 sums are exact and its counts equal the oracle's.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

from . import _native

N_KERNELS = 84
AXES_OK = (3, 6, 9)


def rocket_kernels() -> torch.Tensor:
    """[84, 9] float64 tap weights, rows in ``itertools.combinations(range(9), 3)`` order."""
    w = -torch.ones(N_KERNELS, 9, dtype=torch.float64)
    for k, sub in enumerate(itertools.combinations(range(9), 3)):
        w[k, list(sub)] = 2.0
    return w


def rocket_dilations(window: int) -> List[int]:
    """``[2^e]`` for ``e = 0 .. floor(log2((W - 1) / 8))``."""
    if window < 9:
        raise ValueError("a rocket window must hold at least 9 samples")
    out, d = [], 1
    while 8 * d <= window - 1:
        out.append(d)
        d *= 2
    return out


def rocket_names(n_features: int) -> List[str]:
    return [f"RKT{i:05d}" for i in range(n_features)]


def _window_count(n_samples: int, window: int, stride: int) -> int:
    return 0 if n_samples < window else (n_samples - window) // stride + 1


@dataclass
class RocketParams:
    """The fitted (or hand-built) parameters of the transform.  ``masks`` int32 ``[n_dil, 84]`` axis bit
    sets and ``biases`` float32 ``[n_dil, 84, q]`` are kept on the CPU; ``on(device)`` caches device copies."""

    window: int
    axes: int
    masks: torch.Tensor
    biases: torch.Tensor
    _dev: Dict[str, tuple] = field(default_factory=dict, repr=False, compare=False)

    def __post_init__(self):
        if self.axes not in AXES_OK:
            raise ValueError("axes must be 3, 6 or 9")
        n_dil = len(rocket_dilations(self.window))
        m, b = self.masks, self.biases
        if m.dtype != torch.int32 or tuple(m.shape) != (n_dil, N_KERNELS):
            raise ValueError(f"masks must be int32 [{n_dil}, {N_KERNELS}]")
        if b.dtype != torch.float32 or b.dim() != 3 or tuple(b.shape[:2]) != (n_dil, N_KERNELS) or b.shape[2] < 1:
            raise ValueError(f"biases must be float32 [{n_dil}, {N_KERNELS}, q >= 1]")
        self.masks, self.biases = m.detach().cpu().contiguous(), b.detach().cpu().contiguous()
        if int(self.masks.min()) < 1 or int(self.masks.max()) >= (1 << self.axes):
            raise ValueError("every axis subset must be non-empty and within the stream's axes")
        if not bool(torch.isfinite(self.biases).all()):
            raise ValueError("biases must be finite")

    @property
    def dilations(self) -> List[int]:
        return rocket_dilations(self.window)

    @property
    def q(self) -> int:
        return int(self.biases.shape[2])

    @property
    def n_features(self) -> int:
        return N_KERNELS * len(self.dilations) * self.q

    def on(self, device) -> tuple:
        """(masks, biases) on ``device`` (copied once per device)."""
        device = torch.device(device)
        if device.type == "cpu":
            return self.masks, self.biases
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.masks.to(device), self.biases.to(device))
        return self._dev[key]

    def range_lengths(self) -> torch.Tensor:
        """int64 [n_dil, 84]: the length L of every combination's counted range."""
        d = torch.tensor(self.dilations).view(-1, 1)
        odd = (torch.arange(len(self.dilations)).view(-1, 1) + torch.arange(N_KERNELS).view(1, -1)) % 2 == 1
        return torch.where(odd, self.window - 8 * d, torch.full_like(d, self.window)).expand(-1, N_KERNELS).clone()


def _check_stream(stream: torch.Tensor, params: RocketParams, window: int, stride: int) -> None:
    if stream.dim() != 2 or stream.shape[1] not in AXES_OK:
        raise ValueError("stream must be [samples, axes] with 3, 6 or 9 axes")
    if not stream.dtype.is_floating_point:
        raise ValueError("stream must be a floating-point tensor")
    if window < 9 or stride <= 0:
        raise ValueError("window must be >= 9 samples and stride positive")
    if params.window != window or params.axes != stream.shape[1]:
        raise ValueError(f"parameters are for windows of {params.window} samples on {params.axes} axes")


def _taps(x: torch.Tensor, d: int) -> torch.Tensor:
    """x [n, A, W] float64 -> the 9 dilated taps of every position, [n, A, 9, W] (zeros outside the window)."""
    W = x.shape[-1]
    xp = torch.nn.functional.pad(x, (4 * d, 4 * d))
    return torch.stack([xp[..., j * d: j * d + W] for j in range(9)], 2)


def _mask_bits(masks: torch.Tensor, axes: int) -> torch.Tensor:
    """int [...] bit sets -> float64 [..., axes] 0/1."""
    return ((masks.long()[..., None] >> torch.arange(axes, device=masks.device)) & 1).double()


def _windows(stream: torch.Tensor, window: int, stride: int, w0: int, m: int) -> torch.Tensor:
    return stream[w0 * stride: (w0 + m - 1) * stride + window].double().unfold(0, window, stride)[:m]  # [m, A, W]


def rocket_conv_torch(stream: torch.Tensor, params: RocketParams, window: int, stride: int,
                      win_idx: Optional[torch.Tensor] = None, combo_idx: Optional[torch.Tensor] = None,
                      absolute: bool = False) -> torch.Tensor:
    """The float64 convolution ``C``.  Without indices: every window and combination,
    ``[n_windows, n_dil * 84, W]`` (small inputs only).  With ``win_idx`` / ``combo_idx`` (equal-length index
    tensors, ``combo = e * 84 + k``): one row per pair, ``[P, W]``.  ``absolute``: the sum of ``|w_j x|`` over
    the same taps and axes instead (the magnitude behind a rounding bound)."""
    _check_stream(stream, params, window, stride)
    A, dev = stream.shape[1], stream.device
    nw = _window_count(stream.shape[0], window, stride)
    wk = rocket_kernels().to(dev)
    masks = params.on(dev)[0]
    dil = params.dilations
    if absolute:
        wk = wk.abs()
    if win_idx is None:
        x = _windows(stream, window, stride, 0, nw) if nw else torch.empty(0, A, window, dtype=torch.float64, device=dev)
        if absolute:
            x = x.abs()
        return torch.cat([torch.einsum("ka,kj,najw->nkw", _mask_bits(masks[e], A), wk, _taps(x, d))
                          for e, d in enumerate(dil)], 1)
    win_idx = torch.as_tensor(win_idx, device=dev).long()
    combo_idx = torch.as_tensor(combo_idx, device=dev).long()
    out = torch.empty(win_idx.numel(), window, dtype=torch.float64, device=dev)
    pos = torch.arange(window, device=dev)
    for e, d in enumerate(dil):
        sel = torch.nonzero(combo_idx // N_KERNELS == e).flatten()
        if not sel.numel():
            continue
        rows = (win_idx[sel, None] * stride + pos[None, :]).reshape(-1)
        x = stream.index_select(0, rows).double().view(sel.numel(), window, A).transpose(1, 2)
        if absolute:
            x = x.abs()
        k = combo_idx[sel] % N_KERNELS
        out[sel] = torch.einsum("pa,pj,pajw->pw", _mask_bits(masks[e][k], A), wk[k], _taps(x, d))
    return out


_CHUNK_BYTES = 1 << 28  # float64 temporaries per chunk of windows


def _range_mask(e: int, d: int, window: int, device) -> torch.Tensor:
    """bool [84, W]: the counted positions of every kernel at dilation index ``e``."""
    t = torch.arange(window, device=device)
    valid = (t >= 4 * d) & (t < window - 4 * d)
    odd = (torch.arange(N_KERNELS, device=device) + e) % 2 == 1
    return torch.where(odd[:, None], valid[None, :], torch.ones_like(valid)[None, :])


def _count_chunks(stream: torch.Tensor, params: RocketParams, window: int, stride: int):
    """Yield int64 counts ``[m, F]`` per chunk of windows.  Every window is reduced on its own, so its row
    does not depend on which other windows share its chunk."""
    S, A = stream.shape
    dev = stream.device
    nw = _window_count(S, window, stride)
    wk = rocket_kernels().to(dev)
    masks, biases = params.on(dev)
    b64 = biases.double()
    q = params.q
    per = max(1, _CHUNK_BYTES // (N_KERNELS * window * 8 * max(A, q // 8 + 1)))
    for w0 in range(0, nw, per):
        m = min(per, nw - w0)
        x = _windows(stream, window, stride, w0, m)
        cols = []
        for e, d in enumerate(params.dilations):
            C = torch.einsum("ka,kj,najw->nkw", _mask_bits(masks[e], A), wk, _taps(x, d))      # [m, 84, W]
            hit = (C[:, :, None, :] > b64[e][None, :, :, None]) & _range_mask(e, d, window, dev)[None, :, None, :]
            cols.append(hit.sum(-1).reshape(m, N_KERNELS * q))
        yield torch.cat(cols, 1)


def rocket_counts_torch(stream: torch.Tensor, params: RocketParams, window: int, stride: int) -> torch.Tensor:
    """The float64 oracle's counts, int32 ``[n_windows, F]``."""
    _check_stream(stream, params, window, stride)
    parts = [c for c in _count_chunks(stream, params, window, stride)]
    if parts:
        return torch.cat(parts).to(torch.int32)
    return torch.empty(0, params.n_features, dtype=torch.int32, device=stream.device)


def counts_to_features(counts: torch.Tensor, params: RocketParams) -> torch.Tensor:
    """``fp32(count) / fp32(L)``: one correctly rounded fp32 division."""
    L = params.range_lengths().to(counts.device).float().repeat_interleave(params.q, 1).reshape(1, -1)
    return counts.float() / L


def rocket_features_torch(stream: torch.Tensor, params: RocketParams, window: int, stride: int) -> torch.Tensor:
    """CPU path and oracle: the float64 definition, returned as float32 ``[n_windows, F]``."""
    return counts_to_features(rocket_counts_torch(stream, params, window, stride), params)


_LONG_WARNED = set()


def _is_long(err: RuntimeError) -> bool:
    return "contract violation code -5" in str(err)


def _long_windows(stream: torch.Tensor, params: RocketParams, window: int, stride: int) -> torch.Tensor:
    """Windows the HIP kernel does not take (contract code -5: the zero-padded window image does not fit the
    LDS): the float64 torch definition on the stream's device, with a one-time warning per shape."""
    key = (stream.shape[1], window, params.q)
    if key not in _LONG_WARNED:
        _LONG_WARNED.add(key)
        import warnings

        warnings.warn(f"rocket_features: {key[0]}-axis windows of {window} samples ({params.n_features} features) "
                      f"do not fit the kernel's LDS; computed with the torch definition on {stream.device}")
    return rocket_counts_torch(stream, params, window, stride)


def rocket_features_into(stream: torch.Tensor, params: RocketParams, window: int, stride: int, out: torch.Tensor,
                         col0: int, counts: Optional[torch.Tensor] = None) -> None:
    """Device path: the kernel writes fp32 columns ``[col0, col0 + F)`` of the existing rows ``out`` (no copy);
    ``counts``, if given, is an int32 ``[n_windows, F]`` buffer that receives the raw counts.  Every argument is
    validated (``ValueError``) before any launch."""
    _check_stream(stream, params, window, stride)
    if not stream.is_cuda:
        raise ValueError("rocket_features_into is the device path; use rocket_features_torch on the CPU")
    if stream.dtype != torch.float32:
        raise ValueError("the device path takes a float32 stream")
    S, A = stream.shape
    nw = _window_count(S, window, stride)
    F = params.n_features
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != nw or col0 < 0 or out.shape[1] < col0 + F or \
            (nw and out.stride(1) != 1) or out.device != stream.device:
        raise ValueError(f"out must be float32 rows [{nw}, >= {col0 + F}] with unit column stride on {stream.device}")
    if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (nw, F) or
                               not counts.is_contiguous() or counts.device != stream.device):
        raise ValueError(f"counts must be a contiguous int32 [{nw}, {F}] buffer on {stream.device}")
    if not nw:
        return
    s = stream.contiguous()
    masks, biases = params.on(stream.device)
    try:
        _native.kernels().rocket_features(s.data_ptr(), S, A, window, stride, nw, len(params.dilations), params.q,
                                          masks.data_ptr(), biases.data_ptr(), out.data_ptr(), out.stride(0), col0,
                                          _native.ptr(counts), _native.stream_ptr())
    except RuntimeError as e:
        if not _is_long(e):
            raise
        c = _long_windows(s, params, window, stride)
        out[:, col0: col0 + F] = counts_to_features(c, params)
        if counts is not None:
            counts.copy_(c)


def rocket_features(stream: torch.Tensor, params: RocketParams, window: int, stride: int) -> torch.Tensor:
    """[S, A] raw samples -> fp32 [n_windows, F] (the HIP kernel on device tensors, the definition on the CPU)."""
    _check_stream(stream, params, window, stride)
    if not stream.is_cuda:
        return rocket_features_torch(stream, params, window, stride)
    out = torch.empty(_window_count(stream.shape[0], window, stride), params.n_features, dtype=torch.float32,
                      device=stream.device)
    rocket_features_into(stream.float(), params, window, stride, out, 0)
    return out


def fit_rocket_params(stream: torch.Tensor, window: int, stride: int, num_features: int = 1680,
                      seed: int = 2018) -> RocketParams:
    """Draw the axis subsets and fit the biases (cold path: torch on the stream's device).

    All random draws come from a CPU ``torch.Generator().manual_seed(seed)`` in this order, so they do not
    depend on the device: (1) ``u`` float64 ``[n_dil * 84]`` — subset size ``m = min(A, floor(2^(u log2(A+1))))``;
    (2) float64 ``[n_dil * 84, A]`` whose row-wise ``argsort`` is the permutation — the subset is its first ``m``
    axes; (3) ``randint(n_windows)`` ``[n_dil * 84]`` — the example window of every combination.  The biases of
    a combination are the quantiles at levels ``(i + 1) / (q + 1)`` (``torch.quantile``, linear) of the float64
    convolution of its example window over its counted range, rounded to float32."""
    if stream.dim() != 2 or stream.shape[1] not in AXES_OK:
        raise ValueError("stream must be [samples, axes] with 3, 6 or 9 axes")
    dil = rocket_dilations(window)
    if stride <= 0:
        raise ValueError("stride must be positive")
    A = stream.shape[1]
    nw = _window_count(stream.shape[0], window, stride)
    if nw < 1:
        raise ValueError("the stream holds no whole window")
    n_dil = len(dil)
    nc = n_dil * N_KERNELS
    q = max(1, int(num_features) // nc)
    g = torch.Generator().manual_seed(int(seed))
    u = torch.rand(nc, generator=g, dtype=torch.float64)
    order = torch.rand(nc, A, generator=g, dtype=torch.float64).argsort(1)
    example = torch.randint(0, nw, (nc,), generator=g)
    m = torch.clamp(torch.floor(torch.pow(2.0, u * math.log2(A + 1))).long(), 1, A)
    chosen = torch.arange(A).view(1, -1) < m.view(-1, 1)                       # first m of the permutation
    masks = (chosen.long() << order).sum(1).to(torch.int32).view(n_dil, N_KERNELS)
    tmp = RocketParams(window, A, masks, torch.zeros(n_dil, N_KERNELS, q))
    C = rocket_conv_torch(stream, tmp, window, stride, example, torch.arange(nc)).cpu()   # [nc, W]
    levels = (torch.arange(q, dtype=torch.float64) + 1) / (q + 1)
    biases = torch.empty(nc, q, dtype=torch.float32)
    for i in range(nc):
        e, k = divmod(i, N_KERNELS)
        lo, hi = (4 * dil[e], window - 4 * dil[e]) if (e + k) % 2 else (0, window)
        biases[i] = torch.quantile(C[i, lo:hi], levels).float()
    return RocketParams(window, A, masks, biases.view(n_dil, N_KERNELS, q))
