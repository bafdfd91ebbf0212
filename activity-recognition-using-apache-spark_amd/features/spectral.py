"""Spectral window features of raw accelerometer / IMU streams.

The activities differ mainly in cadence, which the time-domain columns of ``features.window`` only see
through ``*PEAK``.  Per window and axis, from the raw samples ``x[0..W)`` (no taper) with ``K = W // 2``
bins ``k = 1..K`` (DC excluded, the Nyquist bin as is)::

    X_k = sum_n x[n] e^{-2 pi i k n / W}      P_k = |X_k|^2      f_k = k hz / W      total = sum_k P_k

* band fraction ``b`` (``NBANDS`` = 8): sum of ``P_k`` over ``((k - 1) * NBANDS) // K == b``, over ``total``
  (bands without a bin, ``K < 8``, are 0);
* dominant frequency: ``f_k`` at the largest ``P_k`` (the lowest ``k`` among equals);
* centroid: ``sum f_k P_k / total``;
* entropy: ``-sum p_k ln p_k / ln K`` with ``p_k = P_k / total`` (``0 ln 0 = 0``; 0 when ``K == 1``);
* a constant axis-window (``max == min``) or ``total == 0``: all 11 features are 0.

A constant offset adds exactly 0 to every bin ``k >= 1``, so an implementation may subtract any pivot.

Feature row for A axes (``spectral_feature_names``):
``[A x 8 band fractions][dominant Hz: A][centroid Hz: A][entropy: A]``.

GPU: one HIP kernel (``har_spectral_features``, the DFT as an exact-fp32 GEMM on the matrix cores with the
feature epilogue fused behind it).  CPU: the float64 definition in PyTorch (oracle).
"""
from __future__ import annotations

import math
from typing import List, Sequence

import torch

from ..ops import _native

NBANDS = 8
# the longest window the kernel takes (har_spectral_max_window() of the native module); longer windows
# run the torch definition on the stream's device
SPECTRAL_MAX_WINDOW = 2048


def n_spectral_features(axes: int) -> int:
    return (NBANDS + 3) * axes


def spectral_feature_names(axis_names: Sequence[str] = ("X", "Y", "Z")) -> List[str]:
    names = [f"{a}BAND{b}" for a in axis_names for b in range(NBANDS)]
    for suf in ("DOMFREQ", "CENTROID", "SPECENT"):
        names += [a + suf for a in axis_names]
    return names


def _window_count(n_samples: int, window: int, stride: int) -> int:
    return 0 if n_samples < window else (n_samples - window) // stride + 1


def _check(stream: torch.Tensor, window: int, stride: int) -> None:
    A = stream.shape[1]
    if A % 3 or A > 9 or A == 0:
        raise ValueError("axes must be 3, 6 or 9")
    if window < 3 or stride <= 0:
        raise ValueError("window must be >= 3 samples and stride positive")


_CHUNK_BYTES = 1 << 28  # float64 temporaries per chunk of windows


def _power_chunks(stream: torch.Tensor, window: int, stride: int):
    """Yield ``(x [n, A, W] float64, P [n, A, K] float64)`` per chunk of windows.  Every (window, axis) is
    reduced on its own along the last dimension, so a window's numbers do not depend on which other
    windows share its chunk (sharded streams give the rows of the whole stream)."""
    S, A = stream.shape
    W, K = window, window // 2
    nw = _window_count(S, W, stride)
    dev = stream.device
    k = torch.arange(1, K + 1, device=dev)
    n = torch.arange(W, device=dev)
    ang = ((k[:, None] * n[None, :]) % W).double() * (2.0 * math.pi / W)  # (k n) mod W: exact angles
    cos, sin = torch.cos(ang), torch.sin(ang)                             # [K, W]
    per = max(1, _CHUNK_BYTES // (A * K * W * 8 * 2))
    for w0 in range(0, nw, per):
        m = min(per, nw - w0)
        x = stream[w0 * stride: (w0 + m - 1) * stride + W].double().unfold(0, W, stride)[:m]  # [m, A, W]
        d = (x - x.mean(-1, keepdim=True))[:, :, None, :]                  # any pivot: conditioning only
        re = (d * cos).sum(-1)
        im = (d * sin).sum(-1)
        yield x, re * re + im * im


def spectral_power_torch(stream: torch.Tensor, window: int, stride: int) -> torch.Tensor:
    """float64 ``P_k``, ``k = 1..W // 2``, of every (window, axis): ``[n_windows, A, K]``."""
    _check(stream, window, stride)
    parts = [P for _, P in _power_chunks(stream, window, stride)]
    if parts:
        return torch.cat(parts)
    return torch.empty(0, stream.shape[1], window // 2, dtype=torch.float64, device=stream.device)


def spectral_features_torch(stream: torch.Tensor, window: int, stride: int, hz: float) -> torch.Tensor:
    """CPU/oracle implementation: the float64 definition, returned as float32."""
    _check(stream, window, stride)
    A = stream.shape[1]
    W, K = window, window // 2
    dev = stream.device
    k = torch.arange(1, K + 1, device=dev)
    band = ((k - 1) * NBANDS) // K
    onehot = torch.nn.functional.one_hot(band, NBANDS).double()           # [K, 8]
    f = k.double() * (hz / W)
    outs = []
    for x, P in _power_chunks(stream, window, stride):
        m = x.shape[0]
        total = P.sum(-1)
        live = (x.max(-1).values > x.min(-1).values) & (total > 0)         # [m, A]
        safe = torch.where(live, total, torch.ones_like(total))[..., None]
        p = P / safe
        bands = (p[..., None] * onehot).sum(-2)                            # [m, A, 8]
        dom = f[P.argmax(-1)]                                              # first maximum: the lowest k
        cen = (p * f).sum(-1)
        ent = -torch.xlogy(p, p).sum(-1) / math.log(K) if K > 1 else torch.zeros_like(total)
        row = torch.cat([bands.reshape(m, A * NBANDS), dom, cen, ent], 1)
        mask = torch.cat([live[..., None].expand(m, A, NBANDS).reshape(m, A * NBANDS), live, live, live], 1)
        outs.append(torch.where(mask, row, torch.zeros_like(row)).float())
    if outs:
        return torch.cat(outs)
    return torch.empty(0, n_spectral_features(A), dtype=torch.float32, device=dev)


_LONG_WARNED = set()


def _is_long(err: RuntimeError) -> bool:
    return "contract violation code -5" in str(err)


def _long_windows(stream: torch.Tensor, window: int, stride: int, hz: float) -> torch.Tensor:
    """Windows the HIP kernel does not take (contract code -5: longer than ``SPECTRAL_MAX_WINDOW``): the
    float64 torch definition on the stream's device, with a one-time warning per shape."""
    key = (stream.shape[1], window)
    if key not in _LONG_WARNED:
        _LONG_WARNED.add(key)
        import warnings

        warnings.warn(f"spectral_features: {key[0]}-axis windows of {window} samples exceed the kernel's maximum "
                      f"({SPECTRAL_MAX_WINDOW}); computed with the torch definition on {stream.device}")
    return spectral_features_torch(stream, window, stride, hz)


def spectral_features_into(stream: torch.Tensor, window: int, stride: int, hz: float, out: torch.Tensor,
                           col0: int) -> None:
    """Device path: the kernel writes fp32 columns ``[col0, col0 + 11 A)`` of the rows ``out`` (no copy)."""
    S, A = stream.shape
    nw = _window_count(S, window, stride)
    if not nw:
        return
    s = stream.contiguous().float()
    try:
        _native.kernels().spectral_features(s.data_ptr(), S, A, window, stride, nw, float(hz), out.data_ptr(),
                                            out.stride(0), col0, _native.stream_ptr())
    except RuntimeError as e:
        if not _is_long(e):
            raise
        out[:, col0: col0 + n_spectral_features(A)] = _long_windows(s, window, stride, hz)


def spectral_features(stream: torch.Tensor, window: int, stride: int, hz: float) -> torch.Tensor:
    """[S, A] raw samples -> [n_windows, 11 A] spectral features (GPU kernel on device tensors; windows
    longer than the kernel's maximum: the torch definition on the device, with a warning)."""
    _check(stream, window, stride)
    if not stream.is_cuda:
        return spectral_features_torch(stream, window, stride, hz)
    S, A = stream.shape
    out = torch.empty(_window_count(S, window, stride), n_spectral_features(A), dtype=torch.float32,
                      device=stream.device)
    spectral_features_into(stream, window, stride, hz, out, 0)
    return out


def spectral_features_mlp(stream: torch.Tensor, window: int, stride: int, hz: float, mean: torch.Tensor,
                          inv_std: torch.Tensor, out: torch.Tensor, col0: int) -> torch.Tensor:
    """Training-input mode: bf16 ``(f - mean) * inv_std`` of the 11 A spectral features (``mean`` /
    ``inv_std``: their 11 A statistics) into columns ``[col0, col0 + 11 A)`` of the existing bf16 rows
    ``out`` [n_windows, >= col0 + 11 A].  The features are never NaN, so there is no fill value."""
    _check(stream, window, stride)
    S, A = stream.shape
    nw = _window_count(S, window, stride)
    F = n_spectral_features(A)
    if out.dtype != torch.bfloat16 or out.dim() != 2 or out.shape[0] != nw or out.shape[1] < col0 + F or \
            out.stride(1) != 1 or col0 < 0:
        raise ValueError(f"out must be bf16 rows [{nw}, >= {col0 + F}] with unit column stride")
    if mean.numel() != F or inv_std.numel() != F:
        raise ValueError(f"mean / inv_std must hold the {F} spectral statistics")
    if not nw:
        return out
    if not stream.is_cuda:
        X = spectral_features_torch(stream, window, stride, hz)
        out[:, col0: col0 + F] = ((X - mean.float().cpu()) * inv_std.float().cpu()).to(torch.bfloat16)
        return out
    s = stream.contiguous().float()
    m = mean.float().contiguous()
    r = inv_std.float().contiguous()
    try:
        _native.kernels().spectral_features_mlp(s.data_ptr(), S, A, window, stride, nw, float(hz), m.data_ptr(),
                                                r.data_ptr(), out.data_ptr(), out.stride(0), col0,
                                                _native.stream_ptr())
    except RuntimeError as e:
        if not _is_long(e):
            raise
        out[:, col0: col0 + F] = ((_long_windows(s, window, stride, hz) - m) * r).to(torch.bfloat16)
    return out
