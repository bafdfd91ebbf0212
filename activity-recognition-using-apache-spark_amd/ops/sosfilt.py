"""IIR conditioning of raw ``[S, A]`` streams by cascaded second-order sections, defined ONCE here as PyTorch code.

``sosfilt_torch`` / ``sosfiltfilt_torch`` are the CPU path and the oracle of the HIP kernels in
``csrc/kernels/sosfilt.hip``; ``sosfilt_native`` is their front-end and ``sosfilt`` / ``sosfiltfilt`` dispatch on
the stream's device (a GPU tensor REQUIRES the kernels, as everywhere in the project).

Sections
    ``sos`` fp64 ``[S, 6]`` rows ``(b0, b1, b2, 1, a1, a2)``, 1..4 of them.  ``butter_sos`` designs Butterworth
    low / high passes of order 1..4 (bilinear transform with prewarping, closed form, fp64); an odd order has one
    first-order section (``b2 = a2 = 0``), which comes first.

Recurrence, per axis and per segment, direct form II transposed, in fp64, in sample order; per section
    ``y = b0 x + s1;  s1 = (b1 x - a1 y) + s2;  s2 = b2 x - a2 y``
    and the next section's ``x`` is this one's ``y``.  The last section's ``y`` is rounded once to fp32.

Segments
    ``seg_offsets`` host int64 ``[0, ..., S]``, strictly ascending (``hmm``'s ``seq_offsets``).  The state is set
    at every segment start: to ``sos_zi(sos) * x[start]`` for ``init="step"`` (the steady state of a constant
    input at that level: no start-up transient on a signal that sits on gravity), to zero for ``init="zero"``.
    ``reverse=True`` runs every segment from its last sample to its first.

Zero phase
    ``sosfiltfilt_torch``: the forward pass, rounded to fp32, then the reverse pass on that result, both with
    ``init="step"`` — ``scipy.signal.sosfiltfilt(..., padtype=None, padlen=0)`` with an fp32 intermediate.

Limits (``check_range``, ``ValueError`` on every device before any launch)
    A in 1..9, 1..4 sections, S < 2^31 - 256, finite coefficients, and the conditioning guard
    ``max_{0 <= k <= 4096} max|M^k| <= 2^20`` on the cascade's transition matrix ``M`` (``state_space``): the
    kernels carry chunk states as products with powers of ``M`` in fp64, and at 2^20 a carry loses about
    ``2^20 * 2^5 * 2^-53 = 2^-28`` relative to the signal — still below half an fp32 ulp.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native

MAX_SECTIONS = 4
MAX_AXES = 9
MAX_SAMPLES = (1 << 31) - 256
MAX_ORDER = 4
GUARD_STEPS = 4096
GUARD_BOUND = float(1 << 20)
MAX_CHUNK = 256              # sosfilt.hip: a block's span of chunks sits in 64 KiB of LDS
MAX_GROUP = 64
MODES = {"filter": 0, "split": 1, "body": 2}   # y [S, A] | [x - y | y] [S, 2A] | x - y [S, A]
PHASES = ("chunk_state", "carry_scan", "apply")


# ------------------------------------------------------------------ design
def butter_sos(order: int, cutoff_hz: float, hz: float, btype: str = "low") -> torch.Tensor:
    """Butterworth sections fp64 [ceil(order / 2), 6].  With ``W = tan(pi fc / hz)`` (the prewarped cutoff under
    ``s = (1 - z^-1) / (1 + z^-1)``) the pole pair at angle ``theta_k = (2k + 1) pi / (2n)`` gives
    ``H(s) = W^2 / (s^2 + 2 sin(theta_k) W s + W^2)`` (high: ``s^2`` on top), the real pole of an odd order
    ``W / (s + W)`` (high: ``s``)."""
    if btype not in ("low", "high"):
        raise ValueError(f"btype must be 'low' or 'high', got {btype!r}")
    if not 1 <= int(order) <= MAX_ORDER or int(order) != order:
        raise ValueError(f"the designer takes orders 1..{MAX_ORDER}, got {order}")
    if not (0.0 < float(cutoff_hz) < 0.5 * float(hz)) or not math.isfinite(float(hz)):
        raise ValueError(f"the cutoff must lie in (0, hz / 2) = (0, {0.5 * float(hz):g}), got {cutoff_hz}")
    n = int(order)
    W = math.tan(math.pi * float(cutoff_hz) / float(hz))
    rows = []
    if n % 2:
        a0 = 1.0 + W
        b = (W / a0, W / a0, 0.0) if btype == "low" else (1.0 / a0, -1.0 / a0, 0.0)
        rows.append([*b, 1.0, (W - 1.0) / a0, 0.0])
    for k in range(n // 2):
        q = 2.0 * math.sin((2 * k + 1) * math.pi / (2 * n))
        a0 = 1.0 + q * W + W * W
        b = (W * W / a0, 2.0 * W * W / a0, W * W / a0) if btype == "low" else (1.0 / a0, -2.0 / a0, 1.0 / a0)
        rows.append([*b, 1.0, 2.0 * (W * W - 1.0) / a0, (1.0 - q * W + W * W) / a0])
    return torch.tensor(rows, dtype=torch.float64)


def _as_sos(sos) -> torch.Tensor:
    s = torch.as_tensor(sos, dtype=torch.float64).detach().cpu()
    if s.dim() != 2 or s.shape[1] != 6:
        raise ValueError("sos must be [sections, 6] rows (b0, b1, b2, 1, a1, a2)")
    if not 1 <= s.shape[0] <= MAX_SECTIONS:
        raise ValueError(f"the filter takes 1..{MAX_SECTIONS} sections, got {s.shape[0]}")
    if not bool(torch.isfinite(s).all()):
        raise ValueError("sos holds a non-finite coefficient")
    if not bool((s[:, 3] == 1.0).all()):
        raise ValueError("sos rows must be normalised: a0 = 1")
    return s.contiguous()


def sos_zi(sos) -> torch.Tensor:
    """fp64 [sections, 2]: the section states (s1, s2) of the steady response to a unit step
    (``scipy.signal.sosfilt_zi``), in closed form."""
    s = torch.as_tensor(sos, dtype=torch.float64).detach().cpu()
    zi = torch.zeros(s.shape[0], 2, dtype=torch.float64)
    scale = 1.0
    for j, (b0, b1, b2, _, a1, a2) in enumerate(s.tolist()):
        if 1.0 + a1 + a2 == 0.0:
            raise ValueError("a section with a pole at z = 1 has no steady step response: use init='zero'")
        g = (b0 + b1 + b2) / (1.0 + a1 + a2)
        s2 = b2 - a2 * g
        s1 = b1 - a1 * g + s2
        zi[j, 0], zi[j, 1] = s1 * scale, s2 * scale
        scale *= g
    return zi


def _step_np(s: np.ndarray, z: np.ndarray, x: float) -> Tuple[np.ndarray, float]:
    z = z.copy()
    for j in range(s.shape[0]):
        b0, b1, b2, _, a1, a2 = s[j]
        y = b0 * x + z[2 * j]
        z[2 * j] = (b1 * x - a1 * y) + z[2 * j + 1]
        z[2 * j + 1] = b2 * x - a2 * y
        x = y
    return z, x


def state_space(sos):
    """The cascade as one linear system ``z' = M z + v x``, ``y = c . z + d x`` over the 2 S states
    ``z = (s1_0, s2_0, s1_1, s2_1, ...)``: fp64 numpy ``(M [2S, 2S], v [2S], c [2S], d)``, read off the
    recurrence itself (a unit state or a unit input through one step)."""
    s = torch.as_tensor(sos, dtype=torch.float64).detach().cpu().numpy()
    n = 2 * s.shape[0]
    M, c = np.zeros((n, n)), np.zeros(n)
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        M[:, i], c[i] = _step_np(s, e, 0.0)
    v, d = _step_np(s, np.zeros(n), 1.0)
    return M, v, c, float(d)


_GUARD_CACHE: dict = {}


def power_growth(sos, steps: int = GUARD_STEPS) -> float:
    """``max_{0 <= k <= steps} max|M^k|`` in fp64 on the host (inf when a power overflows)."""
    s = torch.as_tensor(sos, dtype=torch.float64).detach().cpu().contiguous()
    key = (s.numpy().tobytes(), int(steps))
    if key not in _GUARD_CACHE:
        M = state_space(s)[0]
        X, worst = np.eye(M.shape[0]), 1.0
        with np.errstate(all="ignore"):
            for _ in range(int(steps)):
                X = X @ M
                m = float(np.abs(X).max())
                if not math.isfinite(m):
                    worst = math.inf
                    break
                worst = max(worst, m)
        if len(_GUARD_CACHE) > 64:
            _GUARD_CACHE.clear()
        _GUARD_CACHE[key] = worst
    return _GUARD_CACHE[key]


def check_range(stream: torch.Tensor, sos) -> torch.Tensor:
    """Validate the stream's shape and the sections (``ValueError``); returns the sections as host fp64."""
    if stream.dim() != 2 or stream.dtype != torch.float32:
        raise ValueError("stream must be fp32 [S, A]")
    S, A = stream.shape
    if not 1 <= A <= MAX_AXES:
        raise ValueError(f"the filter takes 1..{MAX_AXES} axes, got {A}")
    if S >= MAX_SAMPLES:
        raise ValueError(f"the filter takes fewer than 2^31 - 256 samples, got {S}")
    s = _as_sos(sos)
    g = power_growth(s)
    if not g <= GUARD_BOUND:
        raise ValueError(f"the sections are too ill-conditioned for chunked evaluation: max|M^k| = {g:.3g} over "
                         f"k <= {GUARD_STEPS} exceeds 2^20 (split the design into lower orders or raise the cutoff)")
    return s


def _host_offsets(seg_offsets, S: int) -> torch.Tensor:
    if seg_offsets is None:
        return torch.tensor([0, S], dtype=torch.int64)
    off = torch.as_tensor(seg_offsets)
    if off.dtype != torch.int64 or off.dim() != 1 or off.numel() < 1:
        raise ValueError("seg_offsets must be an int64 vector [segments + 1]")
    off = off.cpu()
    if int(off[0]) != 0 or int(off[-1]) != S:
        raise ValueError(f"seg_offsets must run from 0 to S = {S}, got {int(off[0])} .. {int(off[-1])}")
    if off.numel() > 1 and not bool((off[1:] > off[:-1]).all()):
        raise ValueError("seg_offsets must be strictly increasing (no empty segment)")
    return off


def _check_init(init: str) -> bool:
    if init not in ("step", "zero"):
        raise ValueError(f"init must be 'step' or 'zero', got {init!r}")
    return init == "step"


# ------------------------------------------------------------------ the definition
def sosfilt_torch(stream: torch.Tensor, sos, seg_offsets=None, init: str = "step", reverse: bool = False, *,
                  out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The sequential recurrence, vectorised ACROSS segments and axes only (sample tau of every segment that has
    one is a single batched update; nothing is reassociated along time).  ``out_dtype=torch.float64`` returns the
    result before its rounding to fp32."""
    s = check_range(stream, sos)
    step = _check_init(init)
    S, A = stream.shape
    off = _host_offsets(seg_offsets, S)
    dev = stream.device
    y = torch.empty(S, A, dtype=torch.float64, device=dev)
    if S == 0:
        return y.to(out_dtype)
    coef = s.tolist()
    zi = sos_zi(s).tolist() if step else [[0.0, 0.0]] * s.shape[0]
    lens = off[1:] - off[:-1]
    nseg = lens.numel()
    order = torch.argsort(lens, descending=True, stable=True)   # longest first: the running ones are a prefix
    slen = lens[order]
    first = (off[1:][order] - 1 if reverse else off[:-1][order]).to(dev)
    sign = -1 if reverse else 1
    maxlen = int(slen[0])
    nact = (nseg - torch.searchsorted(slen.flip(0).contiguous(), torch.arange(maxlen, dtype=torch.int64), right=True)).tolist()
    x0 = stream[first].double()                                                  # [nseg, A]
    s1 = [x0 * z[0] if step else torch.zeros_like(x0) for z in zi]
    s2 = [x0 * z[1] if step else torch.zeros_like(x0) for z in zi]
    for tau in range(maxlen):
        n = nact[tau]
        rows = first[:n] + sign * tau
        x = stream[rows].double()
        for j, (b0, b1, b2, _, a1, a2) in enumerate(coef):
            v = b0 * x + s1[j][:n]
            s1[j][:n] = (b1 * x - a1 * v) + s2[j][:n]
            s2[j][:n] = b2 * x - a2 * v
            x = v
        y[rows] = x
    return y.to(out_dtype)


def sosfiltfilt_torch(stream: torch.Tensor, sos, seg_offsets=None) -> torch.Tensor:
    """Zero-phase: forward, round to fp32, reverse on that result; both passes ``init="step"``."""
    fwd = sosfilt_torch(stream, sos, seg_offsets, "step", False)
    return sosfilt_torch(fwd, sos, seg_offsets, "step", True)


# ------------------------------------------------------------------ kernels
def chunk_len() -> int:
    """Samples per chunk of the native scan."""
    return int(_native.kernels().sosfilt_chunk_len())


def scan_group() -> int:
    """Chunks per group of the native carry scan."""
    return int(_native.kernels().sosfilt_scan_group())


def scan_levels(S: int, L: int, G: int) -> list:
    """Element counts of the grouped carry scan: n[0] = ceil(S / L) chunks, n[l + 1] = ceil(n[l] / G) while
    n[l] > G (the launcher computes the same list)."""
    n = [-(-int(S) // int(L))]
    while n[-1] > G:
        n.append(-(-n[-1] // G))
    return n


def carry_powers(sos, L: int, G: int, levels: int) -> np.ndarray:
    """fp64 [levels, G, 2S, 2S]: entry (l, k) = P_l^(k + 1) with P_0 = M^L and P_(l+1) = P_l^G — inside a group of
    level l the transition between neighbours is the constant P_l.  Computed once on the host."""
    M = state_space(sos)[0]
    n = M.shape[0]
    out = np.zeros((levels, G, n, n))
    with np.errstate(all="ignore"):
        P = np.linalg.matrix_power(M, int(L))
        for l in range(levels):
            X = P
            for k in range(G):
                out[l, k] = X
                X = X @ P
            P = out[l, G - 1]
    return out


_POWER_CACHE: dict = {}


def _upload(t: torch.Tensor, dev) -> torch.Tensor:
    """Host -> device without a synchronising call: through pinned memory, asynchronously."""
    return t.pin_memory().to(dev, non_blocking=True)


def _device_powers(s: torch.Tensor, L: int, G: int, levels: int, dev) -> torch.Tensor:
    # the copy is enqueued on the stream current at first use and nothing orders another stream behind it, so a
    # table belongs to the stream that uploaded it: the stream is part of the key
    key = (s.numpy().tobytes(), L, G, levels, str(dev), _native.stream_ptr(dev))
    t = _POWER_CACHE.get(key)
    if t is None:
        if len(_POWER_CACHE) > 32:
            _POWER_CACHE.clear()
        t = _upload(torch.from_numpy(carry_powers(s, L, G, levels)).contiguous(), dev)
        _POWER_CACHE[key] = t
    return t


def sosfilt_native(stream: torch.Tensor, sos, seg_offsets=None, init: str = "step", reverse: bool = False,
                   mode: str = "filter", comp: Optional[torch.Tensor] = None, chunk: Optional[int] = None,
                   group: Optional[int] = None, out: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None, phases: Optional[Tuple[int, int]] = None,
                   offsets_device: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The HIP filter of a device stream (``csrc/kernels/sosfilt.hip``).  ``mode`` picks the output (``MODES``);
    ``comp`` [S, A] replaces ``x`` in the complement ``x - y`` (the zero-phase second pass filters the first
    pass's output but subtracts from the raw stream); ``chunk`` / ``group`` override the chunk length L and the
    scan group G (tests cross several scan levels on small streams); ``out`` a contiguous fp32 buffer to fill,
    ``workspace`` a uint8 scratch tensor to reuse, ``phases`` = (first, last) of ``PHASES`` to run over that
    workspace, ``offsets_device`` the segment offsets already on the device."""
    s = check_range(stream, sos)
    step = _check_init(init)
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r} ({' | '.join(MODES)})")
    if not stream.is_cuda:
        raise ValueError("sosfilt_native takes a device stream")
    S, A = stream.shape
    off = _host_offsets(seg_offsets, S)
    OA = 2 * A if mode == "split" else A
    dev = stream.device
    if comp is not None:
        if mode == "filter":
            raise ValueError("comp needs a complement mode (split | body)")
        if comp.dtype != torch.float32 or tuple(comp.shape) != (S, A) or comp.device != dev:
            raise ValueError(f"comp must be fp32 [{S}, {A}] on the stream's device")
        comp = comp.contiguous()
    if out is None:
        out = torch.empty(S, OA, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (S, OA) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be contiguous fp32 [{S}, {OA}] on the stream's device")
    mod = _native.kernels()
    L = int(chunk) if chunk is not None else int(mod.sosfilt_chunk_len())
    G = int(group) if group is not None else int(mod.sosfilt_scan_group())
    if not 1 <= L <= MAX_CHUNK or not 2 <= G <= MAX_GROUP:
        raise ValueError(f"chunk length in 1..{MAX_CHUNK} and scan group in 2..{MAX_GROUP}, got {L}, {G}")
    if S == 0:
        return out
    ns = s.shape[0]
    levels = len(scan_levels(S, L, G))
    need = int(mod.sosfilt_workspace_bytes(S, A, ns, L, G))
    if need < 0:
        raise ValueError(f"sosfilt: shape S = {S}, A = {A}, sections = {ns}, L = {L}, G = {G} is out of range")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_cuda:
        raise ValueError(f"workspace must be a device uint8 tensor of >= {need} bytes")
    nseg = off.numel() - 1
    if nseg == 1:
        off_ptr = 0                      # one segment: the kernels need no offsets
    else:
        off_d = offsets_device if offsets_device is not None else _upload(off, dev)
        if off_d.dtype != torch.int64 or off_d.numel() != nseg + 1 or not off_d.is_cuda:
            raise ValueError("offsets_device must be the int64 offsets on the device")
        off_ptr = off_d.data_ptr()
    powers = _device_powers(s, L, G, levels, dev)
    x = stream.contiguous()
    zi = sos_zi(s) if step else torch.zeros(ns, 2, dtype=torch.float64)
    lo, hi = phases if phases is not None else (0, len(PHASES) - 1)
    mod.sosfilt(x.data_ptr(), _native.ptr(comp), out.data_ptr(), off_ptr, S, nseg, A, ns, L, G, int(bool(reverse)),
                int(step), MODES[mode], s[:, [0, 1, 2, 4, 5]].reshape(-1).tolist(), zi.reshape(-1).tolist(),
                powers.data_ptr(), levels, workspace.data_ptr(), workspace.numel(), int(lo), int(hi),
                _native.stream_ptr())
    return out


def _complement(x: torch.Tensor, y: torch.Tensor, mode: str) -> torch.Tensor:
    if mode == "filter":
        return y
    body = x - y
    return body if mode == "body" else torch.cat([body, y], 1)


def sosfilt(stream: torch.Tensor, sos, seg_offsets=None, init: str = "step", reverse: bool = False,
            mode: str = "filter") -> torch.Tensor:
    """fp32 [S, A] (``mode="split"``: [S, 2A] = [x - y | y]); dispatches on the stream's device."""
    if stream.is_cuda:
        return sosfilt_native(stream, sos, seg_offsets, init, reverse, mode)
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r} ({' | '.join(MODES)})")
    return _complement(stream, sosfilt_torch(stream, sos, seg_offsets, init, reverse), mode)


def sosfiltfilt(stream: torch.Tensor, sos, seg_offsets=None, mode: str = "filter") -> torch.Tensor:
    """The zero-phase form; dispatches on the stream's device.  On the device the second pass writes the
    complement against the raw stream in the same launch."""
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r} ({' | '.join(MODES)})")
    if stream.is_cuda:
        fwd = sosfilt_native(stream, sos, seg_offsets, "step", False)
        return sosfilt_native(fwd, sos, seg_offsets, "step", True, mode, comp=stream if mode != "filter" else None)
    return _complement(stream, sosfiltfilt_torch(stream, sos, seg_offsets), mode)
