"""HMM smoothing of per-window class scores: exact Viterbi decoding, defined ONCE here as PyTorch code.

``viterbi_torch`` is the CPU path and the oracle of the HIP kernels in ``csrc/kernels/hmm.hip``;
``viterbi_native`` is their front-end and ``viterbi`` dispatches on the tensors' device (a GPU tensor
REQUIRES the kernels, as everywhere in the project).

Inputs
    ``E``   int32 [T, K]  quantised emission scores
    ``A``   int32 [K, K]  ``A[i, j]`` = score of the transition i -> j
    ``pi``  int32 [K]     score of starting in a state
    ``seq_offsets`` int64 [S + 1], ``seq_offsets[0] = 0``, ``seq_offsets[S] = T``, strictly increasing
    (no empty sequence).  The S sequences are decoded independently.

Quantisation
    ``quantize_logprob(x) = rint(max(x, -32.0) * 2^20)``, computed in fp64 by torch ops and stored as
    int32 (values above +32 — a scaled likelihood can be positive — are clamped too), so every value
    lies in [-2^25, 2^25] and a log-probability in [-2^25, 0].  The kernels never take a logarithm:
    they consume these integers (the device's ``log`` is not the host's bit for bit, and one quantum
    can flip a path).  The floor also stands for "forbidden".  All accumulation is int64; a step adds
    at most 2^26 in magnitude, so 2^31 steps fit.

Recurrence, per sequence
    ``d_0(j) = pi(j) + E_0(j)``
    ``d_t(j) = max_i (d_{t-1}(i) + A(i, j)) + E_t(j)``, ``psi_t(j)`` = the lowest ``i`` attaining that max
    ``s_{T-1}`` = the lowest argmax of ``d_{T-1}``, ``s_{t-1} = psi_t(s_t)``
    i.e. among all best-scoring paths the one that is smallest when paths are compared from the last
    position backwards.

Outputs
    ``path`` int32 [T], ``score`` int64 [S] (the best path score of each sequence, in quanta).

Limits
    1 <= K <= 32, T < 2^31; T = 0 returns empty tensors without a launch; violations raise
    ``ValueError`` on every device.

Because every score is an integer, the max-plus products the kernels form over chunks of steps are
exact and associative: the parallel decode equals this sequential definition bit for bit, ties included.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _native

QBITS = 20
Q = float(1 << QBITS)
LOG_FLOOR = -32.0
LOG_CEIL = 32.0
MAX_STATES = 32              # hmm.hip: a state per lane, a chunk within 32 lanes
MAX_STEPS = (1 << 31) - 1


def quantize_logprob(x: torch.Tensor) -> torch.Tensor:
    """rint(clamp(x, -32, 32) * 2^20) as int32, in fp64 (round half to even; -inf and NaN -> the floor)."""
    v = torch.nan_to_num(x.double(), nan=LOG_FLOOR, posinf=LOG_CEIL, neginf=LOG_FLOOR)
    return torch.round(v.clamp(LOG_FLOOR, LOG_CEIL) * Q).to(torch.int32)


def emission_scores(prob: torch.Tensor, prior: Optional[torch.Tensor] = None, mode: str = "scaled") -> torch.Tensor:
    """int32 [T, K] emission scores of class probabilities [T, K] (fp64 torch ops on ``prob``'s device).

    ``mode="scaled"``: log(p / prior), the hybrid-HMM scaled likelihood (a classifier's posterior
    divided by the class prior is proportional to p(x | class)); ``mode="posterior"``: log p."""
    p = prob.double()
    if mode == "scaled":
        if prior is None:
            raise ValueError("emission mode 'scaled' needs the class priors")
        p = p / prior.to(device=p.device, dtype=torch.float64).view(1, -1)
    elif mode != "posterior":
        raise ValueError(f"unknown emission mode {mode!r} (scaled | posterior)")
    return quantize_logprob(torch.log(p))


# ------------------------------------------------------------------ argument checks
def _host_offsets(seq_offsets, T: int) -> torch.Tensor:
    off = torch.as_tensor(seq_offsets)
    if off.dtype != torch.int64 or off.dim() != 1 or off.numel() < 1:
        raise ValueError("seq_offsets must be an int64 vector [S + 1]")
    off = off.cpu()  # pass the offsets as a host tensor: a device tensor is read back here, before the decode
    if int(off[0]) != 0 or int(off[-1]) != T:
        raise ValueError(f"seq_offsets must run from 0 to T = {T}, got {int(off[0])} .. {int(off[-1])}")
    if off.numel() > 1 and not bool((off[1:] > off[:-1]).all()):
        raise ValueError("seq_offsets must be strictly increasing (no empty sequence)")
    return off


def check_args(E: torch.Tensor, A: torch.Tensor, pi: torch.Tensor, seq_offsets) -> torch.Tensor:
    """Validate shapes, dtypes and limits (``ValueError``); returns the offsets as a host tensor."""
    if E.dim() != 2 or E.dtype != torch.int32:
        raise ValueError("E must be int32 [T, K]")
    T, K = E.shape
    if not 1 <= K <= MAX_STATES:
        raise ValueError(f"the decoder takes 1..{MAX_STATES} states, got {K}")
    if T > MAX_STEPS:
        raise ValueError(f"the decoder takes fewer than 2^31 steps, got {T}")
    if A.dtype != torch.int32 or tuple(A.shape) != (K, K):
        raise ValueError(f"A must be int32 [{K}, {K}]")
    if pi.dtype != torch.int32 or tuple(pi.shape) != (K,):
        raise ValueError(f"pi must be int32 [{K}]")
    return _host_offsets(seq_offsets, T)


def _lowest_argmax(c: torch.Tensor, dim: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(max, the lowest index attaining it) along ``dim`` — spelled out, not left to argmax's tie rule."""
    mx = c.max(dim=dim, keepdim=True).values
    n = c.shape[dim]
    shape = [1] * c.dim()
    shape[dim] = n
    iota = torch.arange(n, device=c.device).view(shape)
    arg = torch.where(c == mx, iota, torch.full_like(iota, n)).min(dim=dim).values
    return mx.squeeze(dim), arg


# ------------------------------------------------------------------ the definition
def viterbi_torch(E: torch.Tensor, A: torch.Tensor, pi: torch.Tensor, seq_offsets) -> Tuple[torch.Tensor, torch.Tensor]:
    """The sequential recurrence, vectorised ACROSS sequences only (step tau of every sequence that has
    one is a single batched update; nothing is reassociated along time)."""
    off = check_args(E, A, pi, seq_offsets)
    T, K = E.shape
    dev = E.device
    S = off.numel() - 1
    path = torch.empty(T, dtype=torch.int32, device=dev)
    score = torch.empty(S, dtype=torch.int64, device=dev)
    if T == 0:
        return path, score
    A64, pi64 = A.long(), pi.long()
    lens = off[1:] - off[:-1]
    # longest first: the sequences still running at step tau are then a prefix of the order
    order = torch.argsort(lens, descending=True, stable=True)
    slen = lens[order]
    starts = off[:-1][order].to(dev)
    maxlen = int(slen[0])
    # nact[tau] = sequences with a step tau (length > tau)
    nact = (S - torch.searchsorted(slen.flip(0).contiguous(), torch.arange(maxlen, dtype=torch.int64), right=True)).tolist()
    psi = torch.empty(T, K, dtype=torch.int64, device=dev)
    d = pi64.view(1, K) + E[starts].long()                                     # [S, K]
    for tau in range(1, maxlen):
        n = nact[tau]
        rows = starts[:n] + tau
        best, arg = _lowest_argmax(d[:n, :, None] + A64[None, :, :], dim=1)    # over i, per (sequence, j)
        psi[rows] = arg
        d[:n] = best + E[rows].long()
    best, s = _lowest_argmax(d, dim=1)                                         # every sequence's d at its last step
    score[order.to(dev)] = best
    for tau in range(maxlen - 1, -1, -1):
        n = nact[tau]
        rows = starts[:n] + tau
        if tau + 1 < maxlen:
            m = nact[tau + 1]                                                  # those with a step tau + 1
            if m:
                s[:m] = psi[rows[:m] + 1].gather(1, s[:m, None]).squeeze(1)
        path[rows] = s[:n].to(torch.int32)
    return path, score


# ------------------------------------------------------------------ kernels
def chunk_len() -> int:
    """Steps per chunk of the native decode."""
    return int(_native.kernels().hmm_chunk_len())


def scan_group() -> int:
    """Chunks per group of the native decode's two-level scans."""
    return int(_native.kernels().hmm_scan_group())


PHASES = ("flags", "chunk_matrices", "chunk_scan", "forward", "map_scan", "backtrace", "scores")


def viterbi_native(E: torch.Tensor, A: torch.Tensor, pi: torch.Tensor, seq_offsets, chunk: Optional[int] = None,
                   out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, workspace: Optional[torch.Tensor] = None,
                   phases: Optional[Tuple[int, int]] = None, offsets_device: Optional[torch.Tensor] = None):
    """The HIP decode of device tensors.  ``chunk`` overrides the chunk length, ``out`` = (path, score)
    buffers to fill, ``workspace`` a uint8 scratch tensor to reuse, ``phases`` = (first, last) of
    ``PHASES`` to run over that workspace (probes time them one by one)."""
    off = check_args(E, A, pi, seq_offsets)
    if not (E.is_cuda and A.is_cuda and pi.is_cuda):
        raise ValueError("viterbi_native takes device tensors")
    T, K = E.shape
    S = off.numel() - 1
    dev = E.device
    path, score = out if out is not None else (torch.empty(T, dtype=torch.int32, device=dev),
                                               torch.empty(S, dtype=torch.int64, device=dev))
    if path.dtype != torch.int32 or path.numel() != T or score.dtype != torch.int64 or score.numel() != S \
            or not (path.is_contiguous() and score.is_contiguous()):
        raise ValueError("out = (int32 [T], int64 [S]) contiguous")
    if T == 0:
        return path, score
    mod = _native.kernels()
    L = int(chunk) if chunk is not None else int(mod.hmm_chunk_len())
    if L < 1:
        raise ValueError(f"chunk length must be >= 1, got {L}")
    need = int(mod.hmm_workspace_bytes(T, K, S, L))
    if need < 0:
        raise ValueError(f"hmm decode: shape T = {T}, K = {K}, S = {S}, L = {L} is out of range")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_cuda:
        raise ValueError(f"workspace must be a device uint8 tensor of >= {need} bytes")
    E, A, pi = E.contiguous(), A.contiguous(), pi.contiguous()
    off_d = offsets_device if offsets_device is not None else off.to(dev)
    lo, hi = phases if phases is not None else (0, len(PHASES) - 1)
    mod.hmm_viterbi(E.data_ptr(), A.data_ptr(), pi.data_ptr(), off_d.data_ptr(), T, K, S, L, workspace.data_ptr(),
                    workspace.numel(), path.data_ptr(), score.data_ptr(), int(lo), int(hi), _native.stream_ptr())
    return path, score


def viterbi(E: torch.Tensor, A: torch.Tensor, pi: torch.Tensor, seq_offsets) -> Tuple[torch.Tensor, torch.Tensor]:
    """(path int32 [T], score int64 [S]); dispatches on ``E``'s device."""
    return viterbi_native(E, A, pi, seq_offsets) if E.is_cuda else viterbi_torch(E, A, pi, seq_offsets)


# ------------------------------------------------------------------ timelines
def segments(path: torch.Tensor, seq_offsets) -> List[Tuple[int, int, int, int]]:
    """Run-length encoding of a decoded batch: (sequence, first row, last row, state) per maximal run of
    one state inside one sequence, in row order."""
    p = path.detach().cpu().long()
    T = p.numel()
    off = _host_offsets(seq_offsets, T)
    if T == 0:
        return []
    brk = torch.zeros(T, dtype=torch.bool)
    brk[off[:-1]] = True
    brk[1:] |= p[1:] != p[:-1]
    first = torch.nonzero(brk).squeeze(1)
    last = torch.cat([first[1:] - 1, torch.tensor([T - 1])])
    seq = torch.searchsorted(off, first, right=True) - 1
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(seq, first, last, p[first])]


def count_segments(path: torch.Tensor, seq_offsets) -> int:
    return len(segments(path, seq_offsets))
