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

Posteriors
    ``forward_backward_torch`` / ``forward_backward_native`` / ``forward_backward`` (further down) are the
    same three for the sum-product semiring: fp64 in the probability domain (``emission_likelihoods``,
    ``transition_probs``, ``start_probs`` turn the integer scores into ``B``, ``P``, ``p0``), giving the
    state posteriors ``gamma``, the per-sequence log-likelihoods and the summed pairwise posteriors ``xi``
    of Baum-Welch.  Floating-point sums are not associative, so there the kernels
    (``csrc/kernels/hmm_fb.hip``) agree with the definition within a derived rounding bound, not bit for bit.
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


# ------------------------------------------------------------------ posteriors: forward-backward
# Everything below is fp64 in the PROBABILITY domain: the sum-product semiring (+, x) over positive values
# replaces Viterbi's (max, +) over integers.  ``forward_backward_torch`` is the CPU path and the oracle of
# ``csrc/kernels/hmm_fb.hip``.
#
# Kernel precondition (documented, never checked by a device read): ``B`` in [2^-93, 1] with a 1 in every
# row, ``P`` and ``p0`` in [2^-52, 1].  ``emission_likelihoods`` / ``transition_probs`` / ``start_probs``
# produce such values by construction (e^-64 > 2^-93; e^-32 / K row-normalised stays above 2^-52).
FB_PHASES = ("flags", "chunk_products", "prefix_scan", "suffix_scan", "chunk_pass", "reductions")
FB_VARIANTS = {"auto": 0, "lanes": 1, "mfma": 2}   # phase 1 at K > 8: (i, j)-lane LDS kernel | f64 MFMA


def emission_likelihoods(E: torch.Tensor) -> torch.Tensor:
    """fp64 [T, K]: ``exp((E_t(j) - max_j E_t(j)) * 2^-20)`` — every row's maximum is exactly 1 and every
    entry at least e^-64 (the scores lie in [-2^25, 2^25])."""
    if E.dim() != 2 or E.dtype != torch.int32:
        raise ValueError("E must be int32 [T, K]")
    e = E.long()
    if e.shape[0] == 0:
        return torch.empty(e.shape, dtype=torch.float64, device=E.device)
    return torch.exp((e - e.max(dim=1, keepdim=True).values).double() / Q)


def transition_probs(qA: torch.Tensor) -> torch.Tensor:
    """fp64 [K, K]: ``exp(qA * 2^-20)`` with every row normalised to sum 1."""
    p = torch.exp(qA.double() / Q)
    return p / p.sum(dim=1, keepdim=True)


def start_probs(qpi: torch.Tensor) -> torch.Tensor:
    """fp64 [K]: ``exp(qpi * 2^-20)`` normalised to sum 1."""
    p = torch.exp(qpi.double() / Q)
    return p / p.sum()


def loglik_of_scores(loglik: torch.Tensor, E: torch.Tensor, seq_offsets) -> torch.Tensor:
    """The log-likelihood under the scores ``E`` themselves: adds back ``2^-20 * sum_t max_j E_t(j)`` per
    sequence (an exact int64 segment sum) to the ``loglik`` of ``emission_likelihoods(E)``."""
    T = E.shape[0]
    off = _host_offsets(seq_offsets, T)
    if T == 0:
        return loglik.clone()
    mx = E.long().max(dim=1).values
    cs = torch.cat([torch.zeros(1, dtype=torch.int64, device=E.device), torch.cumsum(mx, 0)])
    off_d = off.to(E.device)
    return loglik + (cs[off_d[1:]] - cs[off_d[:-1]]).double() / Q


def check_fb_args(B: torch.Tensor, P: torch.Tensor, p0: torch.Tensor, seq_offsets) -> torch.Tensor:
    """Validate shapes, dtypes and limits (``ValueError``); returns the offsets as a host tensor."""
    if B.dim() != 2 or B.dtype != torch.float64:
        raise ValueError("B must be fp64 [T, K]")
    T, K = B.shape
    if not 1 <= K <= MAX_STATES:
        raise ValueError(f"forward-backward takes 1..{MAX_STATES} states, got {K}")
    if T > MAX_STEPS:
        raise ValueError(f"forward-backward takes fewer than 2^31 steps, got {T}")
    if P.dtype != torch.float64 or tuple(P.shape) != (K, K):
        raise ValueError(f"P must be fp64 [{K}, {K}]")
    if p0.dtype != torch.float64 or tuple(p0.shape) != (K,):
        raise ValueError(f"p0 must be fp64 [{K}]")
    return _host_offsets(seq_offsets, T)


def _fb_empty(T: int, K: int, S: int, dev, want_xi: bool):
    return (torch.empty(T, K, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float64, device=dev),
            torch.zeros(K, K, dtype=torch.float64, device=dev) if want_xi else None)


def forward_backward_torch(B: torch.Tensor, P: torch.Tensor, p0: torch.Tensor, seq_offsets, want_xi: bool = False):
    """The sequential scaled recurrences, vectorised ACROSS sequences only (like ``viterbi_torch``).

    ``gamma`` fp64 [T, K]: ``gamma_t(j) = P(s_t = j | the whole sequence)``, every row normalised by its
    own sum; ``loglik`` fp64 [S]: the log of the sum over all paths; ``xi`` fp64 [K, K] (``want_xi``): the
    sum over every step t that does not start a sequence of the pairwise posterior of (s_{t-1}, s_t), each
    step's K x K table normalised by its own sum."""
    off = check_fb_args(B, P, p0, seq_offsets)
    T, K = B.shape
    dev = B.device
    S = off.numel() - 1
    gamma, loglik, xi = _fb_empty(T, K, S, dev, want_xi)
    if T == 0:
        return gamma, loglik, xi
    lens = off[1:] - off[:-1]
    order = torch.argsort(lens, descending=True, stable=True)
    slen = lens[order]
    starts = off[:-1][order].to(dev)
    maxlen = int(slen[0])
    nact = (S - torch.searchsorted(slen.flip(0).contiguous(), torch.arange(maxlen, dtype=torch.int64), right=True)).tolist()
    alpha = torch.empty(T, K, dtype=torch.float64, device=dev)      # each row scaled to sum 1
    a = p0.view(1, K) * B[starts]                                   # [S, K]
    c = a.sum(1, keepdim=True)
    a = a / c
    alpha[starts] = a
    ll = torch.log(c.squeeze(1))
    for tau in range(1, maxlen):
        n = nact[tau]
        rows = starts[:n] + tau
        x = (a[:n] @ P) * B[rows]
        c = x.sum(1, keepdim=True)
        a[:n] = x / c
        alpha[rows] = a[:n]
        ll[:n] += torch.log(c.squeeze(1))
    loglik[order.to(dev)] = ll
    beta = torch.ones(S, K, dtype=torch.float64, device=dev)        # any positive scale: gamma and xi normalise
    for tau in range(maxlen - 1, -1, -1):
        n = nact[tau]
        rows = starts[:n] + tau
        if tau + 1 < maxlen:
            m = nact[tau + 1]                                       # those with a step tau + 1
            if m:
                w = B[rows[:m] + 1] * beta[:m]                      # [m, K] over j
                if want_xi:
                    x = alpha[rows[:m]][:, :, None] * P[None, :, :] * w[:, None, :]
                    xi += (x / x.sum(dim=(1, 2), keepdim=True)).sum(0)
                nb = w @ P.t()
                beta[:m] = nb / nb.sum(1, keepdim=True)
            # a sequence whose last step is tau keeps beta = 1
        g = alpha[rows] * beta[:n]
        gamma[rows] = g / g.sum(1, keepdim=True)
    return gamma, loglik, xi


def forward_backward_native(B: torch.Tensor, P: torch.Tensor, p0: torch.Tensor, seq_offsets, want_xi: bool = False,
                            chunk: Optional[int] = None, out=None, workspace: Optional[torch.Tensor] = None,
                            phases: Optional[Tuple[int, int]] = None, offsets_device: Optional[torch.Tensor] = None,
                            variant: str = "auto"):
    """The HIP forward-backward of device tensors (``csrc/kernels/hmm_fb.hip``).  ``chunk`` overrides the
    chunk length, ``out`` = (gamma, loglik, xi | None) buffers to fill, ``workspace`` a uint8 scratch tensor
    to reuse, ``phases`` = (first, last) of ``FB_PHASES`` to run over that workspace, ``variant`` the phase-1
    kernel at K > 8 (``FB_VARIANTS``)."""
    off = check_fb_args(B, P, p0, seq_offsets)
    if not (B.is_cuda and P.is_cuda and p0.is_cuda):
        raise ValueError("forward_backward_native takes device tensors")
    if variant not in FB_VARIANTS:
        raise ValueError(f"unknown variant {variant!r} ({' | '.join(FB_VARIANTS)})")
    T, K = B.shape
    S = off.numel() - 1
    dev = B.device
    gamma, loglik, xi = out if out is not None else _fb_empty(T, K, S, dev, want_xi)
    ok = gamma.dtype == torch.float64 and gamma.numel() == T * K and gamma.is_contiguous() \
        and loglik.dtype == torch.float64 and loglik.numel() == S and loglik.is_contiguous() \
        and (not want_xi or (xi is not None and xi.dtype == torch.float64 and xi.numel() == K * K and xi.is_contiguous()))
    if not ok:
        raise ValueError("out = (fp64 [T, K], fp64 [S], fp64 [K, K] with want_xi) contiguous")
    if T == 0:
        return gamma, loglik, (xi if want_xi else None)
    mod = _native.kernels()
    L = int(chunk) if chunk is not None else int(mod.hmm_chunk_len())
    if L < 1:
        raise ValueError(f"chunk length must be >= 1, got {L}")
    need = int(mod.hmm_fb_workspace_bytes(T, K, S, L, bool(want_xi)))
    if need < 0:
        raise ValueError(f"hmm forward-backward: shape T = {T}, K = {K}, S = {S}, L = {L} is out of range")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_cuda:
        raise ValueError(f"workspace must be a device uint8 tensor of >= {need} bytes")
    B, P, p0 = B.contiguous(), P.contiguous(), p0.contiguous()
    off_d = offsets_device if offsets_device is not None else off.to(dev)
    lo, hi = phases if phases is not None else (0, len(FB_PHASES) - 1)
    mod.hmm_forward_backward(B.data_ptr(), P.data_ptr(), p0.data_ptr(), off_d.data_ptr(), T, K, S, L,
                             workspace.data_ptr(), workspace.numel(), gamma.data_ptr(), loglik.data_ptr(),
                             xi.data_ptr() if want_xi else 0, int(lo), int(hi), FB_VARIANTS[variant],
                             _native.stream_ptr())
    return gamma, loglik, (xi if want_xi else None)


def forward_backward(B: torch.Tensor, P: torch.Tensor, p0: torch.Tensor, seq_offsets, want_xi: bool = False):
    """(gamma fp64 [T, K], loglik fp64 [S], xi fp64 [K, K] | None); dispatches on ``B``'s device."""
    if B.is_cuda:
        return forward_backward_native(B, P, p0, seq_offsets, want_xi)
    return forward_backward_torch(B, P, p0, seq_offsets, want_xi)


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
