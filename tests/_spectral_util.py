"""The launch-plan table, the probe stream and the derived error bounds shared by tests/test_spectral_exact.py
(CPU: the preconditions and the mutants) and tests/test_gpu_spectral_exact.py (the spectral kernel,
csrc/kernels/spectral.hip, against the float64 oracle ``spectral_features_torch`` / ``spectral_power_torch``).

The probe stream
----------------
Axis ``c`` holds the exactly representable base ``BASE[c % 3]`` (9.75, -80.5, 0.25) plus sparse spikes of
amplitude ``+-2^j``, ``j`` in -1, 0, 1, about six per window, at seeded positions.  In fp32 as in fp64

* ``d = x - x[0]`` is exact, and where sample 0 of a window carries no spike ``d`` is exactly sparse with
  entries ``+-0.5, +-1, +-2``: every product ``d * twiddle`` is exact and only the ``m`` non-zero terms of a
  row round when they are accumulated;
* every bin carries O(1 / K) of the power and depends on ``m`` table entries only, so one dropped bin, one bin
  in the wrong band or a wrong table index at one sample moves a feature by far more than the fp32 path can.
  A single wrong entry (k, n) moves an aggregate by at most ``4 pi / W^2`` of the total: visible for
  ``W <= 200``, inside the bounds for most bins from ``W = 1024`` on (tests/test_spectral_exact.py).

Windows that do not overlap (``stride >= W``) also carry closed-form rows: a constant axis-window,
a centre impulse (an exact K-way tie), a Nyquist tone, a pure tone in the last bin tile with a phase and an
offset, and a window whose sample 0 carries a spike (dense ``d``).  Every shape has a constant row, and two
rows of exactly two spikes, one of them on the last sample and on a sample of the ``W % 4`` tail.

The bounds (``analyse``)
------------------------
``u = 2^-24`` is the unit roundoff of fp32.  For one row, with ``S1 = sum |d_n|`` and ``m`` non-zero ``d_n``:

``re_k``, ``im_k``  The kernel accumulates ``sum_n d_n t_n`` with the twiddles ``t`` rounded once to fp32
    (``|dt| <= u |t| <= u``, plus 2^-50 for the two float64 libraries' own cos / sin) and one rounding of the
    partial sum (``<= S1`` in magnitude) per non-zero term after the first; zero terms add exactly.  Where some
    ``d_n`` is no power of two its product may round (one more ``u |d_n|``), where ``x - x[0]`` itself rounds in
    fp32 the operand is off by ``u |d_n|``.  Together ``|d re_k|, |d im_k| <= delta = S1 ((1 + u)^r - 1 + 2^-50)``
    with ``r = 1 + (m - 1) + [some d no power of two] + [some d inexact]``: ``m`` for a sparse row, about ``W``
    for a dense one.
``P_k``  ``fma(re, re, im * im) * scale``: ``a_k = 2 (|re| + |im|) delta + 2 delta^2`` from the operands and
    three roundings, ``e_k = a_k + ((1 + u)^3 - 1) (P_k + a_k)``.  The prescale (``2 / (W * W var)``, the
    kernel's floor included) is common to all bins of a row; the features do not depend on it, only the size
    of ``P ln P`` does, so the bound takes the float64 value.
sums  Every lane adds its ``ntiles`` bins, a 16-lane reduction adds four more times: a sum of non-negative
    terms ``v`` is off by at most ``g sum v``, ``g = (1 + u)^(ntiles + 4) - 1`` (``sum |v|`` for ``P ln P``).
band fraction ``f = N / T``  ``dN = E + g (N + E)`` with ``E`` the band's ``sum e_k``, ``dT`` the same over all
    bins; ``(dN + f dT) / (T - dT)`` plus ``4 u f``: the reciprocal (1 ulp = ``2 u``), the product and the
    oracle's own rounding to fp32.
centroid / hz ``c = M / (T W)``, ``M = sum k P_k`` (``k`` exact, one fma per bin): ``(dM + (M / T) dT) / ((T - dT) W)
    + 6 u c`` (reciprocal, two products, ``hz / W``, the oracle's rounding).
entropy ``H = (ln T - S / T) / ln K``, ``S = sum P ln P``: per bin the larger change of ``P ln P`` over
    ``[P - e, P + e]`` (it is convex) plus ``5 u |P ln P|`` (a native log of 1 ulp, its product with ``ln 2``
    rounded twice, the product with ``P``) plus 2^-110 (powers below the smallest normal count as 0), summed
    as above; ``dA = (dS + |S / T| dT) / (T - dT) + 3 u |S / T|``; ``dL = dT / (T - dT) + 4 u |ln T|``;
    ``dH = (dL + dA + u |ln T - S / T|) / ln K + 6 u H``.
dominant frequency  The reported value is an exact bin ``k hz / W``; with ``rho = max e_k / max P_k`` the row's
    relative power bound, the bin's float64 power is at least ``(1 - 2 rho) max P``.  Centre-impulse rows of an
    even window are an exact tie in fp32 (their table entries are (+-1, ~1e-16)): bin 1 outright.

Nothing here is fitted to the kernel.  ``check`` prints the largest ``error / bound`` of every group.

``structured_stream`` holds clipped, square-ish windows whose quarter-rate bin cancels down to one table entry
of ~1e-16 (``model_powers``): a prescaled power below the smallest normal fp32 number, which a logarithm that
flushes denormals would turn into an infinite entropy.
"""
from dataclasses import dataclass, field
from functools import lru_cache
import math

import numpy as np
import torch

import _window_util as WU

HZ = WU.HZ                    # 50 Hz: exact in fp32
TAIL = WU.TAIL                # samples of NaN after the stream
BASE = (9.75, -80.5, 0.25)
U32 = 2.0 ** -24
NB = 8
NFA = NB + 3
K64, K160 = 64 * 1024, 160 * 1024
offsets = WU.offsets

# (axes, W, stride, n_windows, budget, windows per block, waves, staged bytes): what ``make_plan``
# (csrc/kernels/spectral.hip) decides, derived by hand; ``plan`` below is the launcher's rule in Python and
# tests/test_spectral_exact.py holds the two against each other.  "64K" / "160K": the first budget that takes
# 4, 2 or 1 waves' worth of whole windows; "loop": the fallback loop over fewer windows than one wave holds.
SHAPES = [
    (3, 200, 100, 43, "64K", 21, 4, 28016),      # 63 rows, the last wave holds 15
    (6, 200, 100, 21, "64K", 10, 4, 28016),      # 60 rows, the last wave holds 12
    (9, 200, 200, 15, "64K", 7, 4, 52016),
    (3, 193, 97, 43, "64K", 21, 4, 27164),       # one-window last block: 579 floats, a scalar tail of 3
    (3, 500, 250, 21, "64K", 10, 2, 37016),      # 21 windows: 70,016 bytes
    (3, 1024, 512, 11, "64K", 5, 1, 45072),      # 10 windows: 75,792 bytes
    (9, 1500, 100, 15, "160K", 7, 4, 87616),     # one window is 66,016 bytes: over 64 KB
    (9, 1500, 1000, 7, "160K", 3, 2, 138016),    # 7 windows: 282,016 bytes; 27 rows
    (9, 2048, 2048, 3, "160K", 1, 1, 90128),     # 3 windows: 237,584 bytes; 9 rows
    (3, 2047, 2047, 11, "160K", 5, 1, 139220),   # odd W, W % 4 == 3, K = 1023
    (3, 2048, 3000, 9, "loop", 4, 1, 148976),    # 5 windows: 184,976 bytes; 12 rows
    (6, 2048, 5000, 3, "loop", 1, 1, 65552),     # 2 windows: 185,552 bytes; one is 16 bytes over 64 KB
    (3, 3, 1, 43, "64K", 21, 4, 324),            # W < 32 (k % W), K = 1
    (3, 5, 2, 43, "64K", 21, 4, 604),            # K = 2
    (6, 16, 3, 21, "64K", 10, 4, 1176),          # K = 8
    (9, 33, 11, 15, "64K", 7, 4, 3852),          # K = 16
    (3, 200, 100, 1, "64K", 1, 1, 4016),         # short stream: one window, 3 rows
    (3, 200, 100, 11, "64K", 11, 3, 16016),      # wpb = n_windows: 33 rows, a 3-wave block of 192 threads
    (3, 200, 100, 22, "64K", 21, 4, 28016),      # blocks of 21 and 1
]


def shape_id(shape) -> str:
    return "%dx%d/%d*%d" % shape[:4]


def tab_floats(W: int) -> int:
    return (2 * W + 3) & ~3


def staged_bytes(A: int, W: int, stride: int, wpb: int) -> int:
    return (tab_floats(W) + ((wpb - 1) * stride + W) * A + 4) * 4


def plan(A: int, W: int, stride: int, n_windows: int):
    """``make_plan`` in Python: (budget, windows per block, waves, staged bytes), or None."""
    def take(name, wpb):
        return name, wpb, (wpb * A + 15) // 16, staged_bytes(A, W, stride, wpb)

    for name, budget in (("64K", K64), ("160K", K160)):
        for waves in (4, 2, 1):
            wpb = min(16 * waves // A, max(n_windows, 1))
            if staged_bytes(A, W, stride, wpb) <= budget:
                return take(name, wpb)
    for wpb in range(16 // A - 1, 0, -1):
        if staged_bytes(A, W, stride, wpb) <= K160:
            return take("loop", wpb)
    return None


def n_samples(shape) -> int:
    A, W, stride, nwin = shape[:4]
    return (nwin - 1) * stride + W


def seed_of(shape) -> int:
    A, W, stride, nwin = shape[:4]
    return 100003 * A + 31 * W + 7 * stride + nwin


def tail_sample(W: int) -> int:
    """A sample of the ``W % 4`` tail (the last, partial group of four) that is not the pivot; without a tail
    (``W % 4 == 0``) the last sample but one."""
    return max(W - W % 4, 1) if W % 4 else W - 2


TONE_AMP, TONE_PHASE, NYQ_AMP = 1.5, 0.7, 0.5


def tone_bin(W: int) -> int:
    return max(W // 2 - 2, 1)  # in the last bin tile for every W


@dataclass
class Probe:
    buf: torch.Tensor          # fp32 [r0 + S + TAIL, A]: NaN, the stream, NaN
    r0: int
    S: int
    shape: tuple
    rows: dict = field(default_factory=dict)   # kind -> (window, axis)

    def view(self, buf: torch.Tensor = None) -> torch.Tensor:
        b = self.buf if buf is None else buf
        return b[self.r0: self.r0 + self.S]


@lru_cache(maxsize=None)
def _samples(shape):
    """([S, A] float32 samples, {kind: (window, axis)}) of one table row."""
    A, W, stride, nwin = shape[:4]
    S = n_samples(shape)
    rng = np.random.default_rng(seed_of(shape))
    p = min(6.0 / W, 0.5)
    hit = rng.random((S, A)) < p
    amp = np.ldexp(1.0, rng.integers(-1, 2, size=(S, A))) * rng.choice([-1.0, 1.0], size=(S, A))
    sp = np.where(hit, amp, 0.0)
    base = np.array([BASE[c % 3] for c in range(A)])
    rows = {}

    def span(w):
        return slice(w * stride, w * stride + W)

    # (written into ``sp``, before the closed-form rows overwrite whole cells of ``x``: ``taken`` keeps those
    # cells away from these two rows)
    # two rows with exactly two spikes: amplitude 2 on the last sample (on a sample of the W % 4 tail) and
    # amplitude 1 next to it, so that a twiddle index off by one at that sample turns the pair's interference
    wl = 1 if nwin > 1 else 0
    sp[span(wl), 0] = 0.0
    sp[wl * stride + W - 1, 0] = 2.0
    sp[wl * stride + W - 2, 0] = 1.0
    rows["last"] = (wl, 0)
    wt = 2 if nwin > 2 else 0
    nt = tail_sample(W)
    sp[span(wt), 2] = 0.0
    sp[wt * stride + nt, 2] = -2.0
    sp[wt * stride + (nt - 1 if nt > 1 else nt + 1), 2] = 1.0
    rows["tail"] = (wt, 2)
    x = base + sp
    if stride >= W:
        nrows = nwin * A
        step = (nrows - 2) // 8
        # the impulse sits in the last block (one window): the tie is decided in a block with idle rows
        taken = [rows["last"], rows["tail"], (nwin - 1, A - 1)]
        cells = []
        for i in range(8):
            c = divmod(1 + i * step, A)
            if c not in taken and c not in cells:
                cells.append(c)
        kinds = ["const", "tone", "spike0"] + ([] if W % 2 else ["nyquist", "impulse"])
        cells = cells[:len(kinds)]
        if len(kinds) == 5:
            cells[4] = (nwin - 1, A - 1)
        n = np.arange(W)
        for kind, (w, a) in zip(kinds, cells):
            rows[kind] = (w, a)
            seg = x[span(w), a]
            if kind == "const":
                seg[:] = base[a]
            elif kind == "tone":
                seg[:] = base[a] + TONE_AMP * np.cos(2 * np.pi * tone_bin(W) * n / W + TONE_PHASE)
            elif kind == "spike0":
                seg[0] = base[a] - 0.5
            elif kind == "nyquist":
                seg[:] = base[a] + NYQ_AMP * (1 - 2 * (n % 2))
            else:
                seg[:] = base[a]
                seg[W // 2] += 2.0
    else:
        wc = min(3, nwin - 1)
        x[span(wc), 1] = base[1]
        rows["const"] = (wc, 1)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x, rows


def probe_stream(shape, r0: int = 0) -> Probe:
    """The probe stream of one table row, ``r0`` samples into a NaN-filled buffer with TAIL samples of NaN
    after it: a read outside the stream that reaches a result shows up as NaN.  The samples do not depend on
    ``r0``; the stream ends with the last sample of its last window."""
    A = shape[0]
    x, rows = _samples(shape)
    S = x.shape[0]
    buf = torch.full((r0 + S + TAIL, A), float("nan"), dtype=torch.float32)
    buf[r0: r0 + S] = torch.from_numpy(x.copy())
    return Probe(buf, r0, S, shape, dict(rows))


def impulse_shape(W: int):
    """The one-window stream of the centre-impulse sweep."""
    return (3, W, W, 1) + plan(3, W, W, 1)


IMPULSE_AMP = (1.0, -2.0, 0.5)


def impulse_stream(W: int, r0: int = 0) -> Probe:
    """One window of W samples, an impulse of a power of two on sample W // 2 of every axis."""
    x = np.tile(np.array(BASE), (W, 1))
    x[W // 2] += np.array(IMPULSE_AMP)
    buf = torch.full((r0 + W + TAIL, 3), float("nan"), dtype=torch.float32)
    buf[r0: r0 + W] = torch.from_numpy(x.astype(np.float32))
    return Probe(buf, r0, W, impulse_shape(W), {"impulse": (0, a) for a in range(3)})


STRUCTURED_W = (2048, 2040, 2000, 1536, 1024)


def structured_stream(W: int, r0: int = 0) -> Probe:
    """One window of clipped, square-ish data: a clipped sine, a hard-clipped sine and a square wave.  Their
    symmetry cancels most bins almost exactly; what is left of a bin can be one table entry of ~1e-16, and
    after the prescale ``2 / (W * W var)`` its power lies below the smallest normal fp32 (``model_powers``)."""
    n = np.arange(W)
    x = np.stack([np.clip(BASE[0] + 8 * np.sin(2 * np.pi * 5 * n / W), 9.0, 10.5),
                  BASE[1] + np.clip(64 * np.sin(2 * np.pi * 8 * n / W + 0.3), -0.5, 0.5),
                  BASE[2] + np.where((n // 64) % 2 == 0, 1.0, -1.0)], 1).astype(np.float32)
    buf = torch.full((r0 + W + TAIL, 3), float("nan"), dtype=torch.float32)
    buf[r0: r0 + W] = torch.from_numpy(x)
    return Probe(buf, r0, W, (3, W, W, 1) + plan(3, W, W, 1), {})


def model_powers(x: np.ndarray) -> np.ndarray:
    """Prescaled fp32 bin powers [R, K] of the rows x [R, W] under a plain model of the kernel's accumulation:
    one fused multiply-add per sample in ascending order, the fp32 table, ``fma(re, re, im * im) * scale``."""
    R, W = x.shape
    K = W // 2
    f = np.float32
    x = x.astype(f)
    c64, s64, idx = _table(W, K)
    c, s = c64.astype(f).astype(np.float64), s64.astype(f).astype(np.float64)
    d = (x - x[:, :1]).astype(f)
    d64 = d.astype(np.float64)
    re = np.zeros((R, K), f)
    im = np.zeros((R, K), f)
    for n in range(1, W):
        re = (re.astype(np.float64) + d64[:, n:n + 1] * c[idx[:, n]][None, :]).astype(f)
        im = (im.astype(np.float64) + d64[:, n:n + 1] * s[idx[:, n]][None, :]).astype(f)
    t1, t2 = d.sum(1, dtype=f), (d * d).sum(1, dtype=f)
    wv = np.maximum(t2 - t1 * t1 / f(W), f(1e-4) * t2)
    scale = (f(2) / (f(W) * wv)).astype(f)
    p = (re.astype(np.float64) ** 2 + (im * im).astype(np.float64)).astype(f)
    return (p * scale[:, None]).astype(f)


def impulse_expected(W: int, hz: float = HZ) -> np.ndarray:
    """[11] closed form of a centre-impulse row: flat spectrum."""
    K = W // 2
    k = np.arange(1, K + 1)
    out = np.zeros(NFA)
    out[:NB] = np.bincount(((k - 1) * NB) // K, minlength=NB) / K
    out[NB] = hz / W
    out[NB + 1] = hz * (K + 1) / (2 * W)
    out[NB + 2] = 1.0 if K > 1 else 0.0
    return out


# ---------------------------------------------------------------------------------------------------------
# float64 spectra (numpy), with the mutants of tests/test_spectral_exact.py as switches


def windows_of(x: np.ndarray, W: int, stride: int, nwin: int) -> np.ndarray:
    """[S, A] -> [nwin, A, W] float64"""
    idx = np.arange(nwin)[:, None] * stride + np.arange(W)[None, :]
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)[idx].transpose(0, 2, 1))


@lru_cache(maxsize=8)
def _table(W: int, kmax: int):
    """float64 twiddles and the index matrix (k n) mod W, k = 1..kmax"""
    ang = np.arange(W) * (2.0 * math.pi / W)
    k = np.arange(1, kmax + 1)
    idx = (k[:, None] * np.arange(W)[None, :]) % W
    return np.cos(ang), np.sin(ang), idx


def dft(d: np.ndarray, W: int, kmax: int, tw_off=None):
    """re, im [R, kmax] of the rows d [R, W] in float64.  ``tw_off = (n, ks)``: the table index of sample n is
    off by one for the bins ks (None: all)."""
    c, s, idx = _table(W, kmax)
    if tw_off is not None:
        n, ks = tw_off
        idx = idx.copy()
        sel = slice(None) if ks is None else np.asarray(ks) - 1
        idx[sel, n] = (idx[sel, n] + 1) % W
    return d @ c[idx].T, d @ s[idx].T


def features64(x: np.ndarray, hz: float = HZ, *, drop_last=False, band_shift=0, tie_high=False, tw_off=None,
               keep_cols=False, P=None) -> np.ndarray:
    """[..., W] float64 rows -> [..., 11] features of the definition (8 band fractions, dominant frequency,
    centroid, entropy), pivot x[0].  The switches are the mutants."""
    lead, W = x.shape[:-1], x.shape[-1]
    x = x.reshape(-1, W)
    K = W // 2
    kmax = 16 * ((K + 15) // 16) if keep_cols else K
    if P is None:
        re, im = dft(x - x[:, :1], W, kmax, tw_off)
        P = re * re + im * im
    else:
        P = P.reshape(-1, P.shape[-1]).copy()
    if drop_last:
        P[:, K - 1] = 0.0
    k = np.arange(1, kmax + 1)
    band = ((k - 1 + band_shift) * NB) // K
    if band_shift:
        band = np.minimum(band, NB - 1)
    T = P.sum(1)
    live = (x.max(1) > x.min(1)) & (T > 0)
    Ts = np.where(live, T, 1.0)
    p = P / Ts[:, None]
    out = np.zeros((x.shape[0], NFA))
    for b in range(NB):
        out[:, b] = p[:, band == b].sum(1)
    am = (kmax - 1 - P[:, ::-1].argmax(1)) if tie_high else P.argmax(1)
    out[:, NB] = (am + 1) * hz / W
    out[:, NB + 1] = (p * k).sum(1) * hz / W
    if K > 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, NB + 2] = -np.where(p > 0, p * np.log(p), 0.0).sum(1) / math.log(K)
    out[~live] = 0.0
    return out.reshape(lead + (NFA,))


def features32(x: np.ndarray, hz: float = HZ, pivot: np.ndarray = None) -> np.ndarray:
    """A plain fp32 model of the kernel's arithmetic in numpy (sequential fp32 accumulation over the samples,
    fp32 table, fp32 epilogue): [R, W] -> [R, 11].  ``pivot`` [R]: the value subtracted instead of x[0]."""
    R, W = x.shape
    K = W // 2
    f = np.float32
    x = x.astype(f)
    c64, s64, idx = _table(W, K)
    c, s = c64.astype(f), s64.astype(f)
    piv = x[:, 0] if pivot is None else pivot.astype(f)
    d = (x - piv[:, None]).astype(f)
    re = np.zeros((R, K), f)
    im = np.zeros((R, K), f)
    for n in range(W):
        re = (re + d[:, n:n + 1] * c[idx[:, n]][None, :]).astype(f)
        im = (im + d[:, n:n + 1] * s[idx[:, n]][None, :]).astype(f)
    dd = (x - x[:, :1]).astype(f)
    t1, t2 = dd.sum(1, dtype=f), (dd * dd).sum(1, dtype=f)
    wv = np.maximum(t2 - t1 * t1 / f(W), f(1e-4) * t2)
    scale = np.where(wv > 0, f(2) / (f(W) * np.where(wv > 0, wv, f(1))), f(1)).astype(f)
    P = ((re * re + im * im) * scale[:, None]).astype(f)
    k = np.arange(1, K + 1)
    band = ((k - 1) * NB) // K
    T = P.sum(1, dtype=f)
    live = (x.max(1) > x.min(1)) & (T > 0)
    inv = (f(1) / np.where(live, T, f(1))).astype(f)
    out = np.zeros((R, NFA), f)
    for b in range(NB):
        out[:, b] = P[:, band == b].sum(1, dtype=f) * inv
    out[:, NB] = (P.argmax(1) + 1).astype(f) * f(hz) / f(W)
    out[:, NB + 1] = (P * k.astype(f)).sum(1, dtype=f) * inv * (f(hz) / f(W))
    if K > 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            pl = np.where(P > 0, P * np.log(np.where(P > 0, P, f(1))), f(0)).astype(f)
        ent = (np.log(np.where(live, T, f(1))) - pl.sum(1, dtype=f) * inv) * (f(1) / np.log(f(K)))
        out[:, NB + 2] = np.maximum(ent, f(0))
    out[~live] = 0
    return out


def to_rows(F: np.ndarray) -> np.ndarray:
    """[nwin, A, 11] per-axis features -> [nwin, 11 A] rows: [A x 8 bands][dominant: A][centroid: A][entropy: A]"""
    nwin, A = F.shape[:2]
    return np.concatenate([F[:, :, :NB].reshape(nwin, A * NB), F[:, :, NB], F[:, :, NB + 1], F[:, :, NB + 2]], 1)


def per_axis(rows, A: int) -> np.ndarray:
    """[nwin, 11 A] rows -> [nwin, A, 11] float64"""
    r = np.asarray(rows, dtype=np.float64)
    nwin = r.shape[0]
    return np.concatenate([r[:, :NB * A].reshape(nwin, A, NB),
                           r[:, NB * A:].reshape(nwin, 3, A).transpose(0, 2, 1)], 2)


# ---------------------------------------------------------------------------------------------------------
# bounds


@dataclass
class Analysis:
    x: np.ndarray          # [nwin, A, W] float64 windows
    P: np.ndarray          # [nwin, A, K] float64 powers (pivot x[0])
    bound: np.ndarray      # [nwin, A, 11] absolute bounds (bands, -, centroid / hz, entropy)
    rho: np.ndarray        # [nwin, A] relative power bound max e_k / max P_k
    live: np.ndarray       # [nwin, A]
    sparse: np.ndarray     # [nwin, A] sample 0 carries no spike and d is exactly sparse
    m: np.ndarray          # [nwin, A] non-zero terms


def _xlogx(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(v > 0, v * np.log(np.where(v > 0, v, 1.0)), 0.0)


def analyse_windows(x: np.ndarray) -> Analysis:
    """The float64 spectrum and the derived bounds (module docstring) of the windows x [nwin, A, W]."""
    nwin, A, W = x.shape
    K = W // 2
    ntiles = (K + 15) // 16
    u = U32
    xr = x.reshape(-1, W)
    d = xr - xr[:, :1]
    d32 = d.astype(np.float32).astype(np.float64)
    inexact = (d32 != d).any(1)
    nz = d != 0
    m = nz.sum(1)
    S1 = np.abs(d).sum(1)
    mant, _ = np.frexp(d)
    notpow2 = (nz & (np.abs(mant) != 0.5)).any(1)
    r = 1 + np.maximum(m - 1, 0) + notpow2 + inexact
    delta = S1 * ((1 + u) ** r - 1 + 2.0 ** -50)
    re, im = dft(d, W, K)
    P = re * re + im * im
    a = 2 * (np.abs(re) + np.abs(im)) * delta[:, None] + 2 * delta[:, None] ** 2
    e = a + ((1 + u) ** 3 - 1) * (P + a)
    t1, t2 = d.sum(1), (d * d).sum(1)
    wv = np.maximum(t2 - t1 * t1 / W, 1e-4 * t2)
    live = (xr.max(1) > xr.min(1)) & (P.sum(1) > 0)
    s = np.where(wv > 0, 2.0 / (W * np.where(wv > 0, wv, 1.0)), 1.0)
    Ps, es = P * s[:, None], e * s[:, None]
    g = (1 + u) ** (ntiles + 4) - 1
    k = np.arange(1, K + 1)
    band = ((k - 1) * NB) // K
    T, ET = Ps.sum(1), es.sum(1)
    T = np.where(live, T, 1.0)
    dT = ET + g * (T + ET)
    den = np.maximum(T - dT, 1e-300)
    bound = np.zeros((xr.shape[0], NFA))
    for b in range(NB):
        N, E = Ps[:, band == b].sum(1), es[:, band == b].sum(1)
        f = N / T
        bound[:, b] = (E + g * (N + E) + f * dT) / den + 4 * u * f
    M, EM = (Ps * k).sum(1), (es * k).sum(1)
    dM = EM + g * (M + EM)
    c = M / T / W
    bound[:, NB + 1] = (dM + (M / T) * dT) / den / W + 6 * u * c
    if K > 1:
        t = _xlogx(Ps)
        dt = np.maximum(np.abs(_xlogx(Ps + es) - t), np.abs(_xlogx(np.maximum(Ps - es, 0.0)) - t))
        dt = dt + 5 * u * np.abs(t) + 2.0 ** -110
        Sabs, Dt = np.abs(t).sum(1), dt.sum(1)
        dS = Dt + g * (Sabs + Dt)
        Aq = t.sum(1) / T
        dA = (dS + np.abs(Aq) * dT) / den + 3 * u * np.abs(Aq)
        L = np.log(T)
        dL = dT / den + 4 * u * np.abs(L)
        H = (L - Aq) / math.log(K)
        bound[:, NB + 2] = (dL + dA + u * np.abs(L - Aq)) / math.log(K) + 6 * u * np.abs(H)
    bound[~live] = 0.0
    pmax = P.max(1)
    rho = np.where(live, e.max(1) / np.where(pmax > 0, pmax, 1.0), 0.0)
    sparse = (~notpow2) & (~inexact) & (m <= 64) & live
    sh = (nwin, A)
    return Analysis(x, P.reshape(sh + (K,)), bound.reshape(sh + (NFA,)), rho.reshape(sh), live.reshape(sh),
                    sparse.reshape(sh), m.reshape(sh))


@lru_cache(maxsize=None)
def analyse(shape) -> Analysis:
    A, W, stride, nwin = shape[:4]
    return analyse_windows(windows_of(_samples(shape)[0], W, stride, nwin))


@lru_cache(maxsize=None)
def reference(shape) -> np.ndarray:
    """[nwin, A, 11] float64 view of the oracle's rows (``spectral_features_torch``) for a table row, computed
    once on the CPU; the dominant column is taken from the oracle's float64 powers in ``check``."""
    from har.features.spectral import spectral_features_torch

    A, W, stride = shape[:3]
    return per_axis(spectral_features_torch(probe_stream(shape).view(), W, stride, HZ).numpy(), A)


def measure(out, ref: np.ndarray, an: Analysis, W: int, hz: float = HZ, impulse_rows=()) -> dict:
    """Largest ``error / bound`` per feature group of the rows ``out`` [nwin, 11 A] against the oracle's
    per-axis features ``ref`` [nwin, A, 11], as {"bands", "centroid", "entropy", "dominant", "flat",
    "finite"}; "dominant" is the largest ``(max P - P[k]) / (2 rho max P)`` (inf: no bin, or a centre-impulse
    row that is not bin 1), "flat" the count of non-zeros in constant rows, "finite" a bool.  ``where`` holds
    the (window, axis) of each largest ratio."""
    nwin, A = an.live.shape
    K = W // 2
    o = per_axis(out, A)
    res = {"finite": bool(np.isfinite(o).all()), "where": {}}
    o = np.nan_to_num(o, nan=1e30, posinf=1e30, neginf=-1e30)
    live = an.live
    res["flat"] = int(np.count_nonzero(o[~live]))

    def ratio(name, err, bnd):
        q = np.where(live[..., None] if err.ndim == 3 else live, err / np.maximum(bnd, 1e-300), 0.0)
        q = np.where((err == 0), 0.0, q)
        res[name] = float(q.max()) if q.size else 0.0
        if q.size:
            res["where"][name] = tuple(int(i) for i in np.unravel_index(int(q.argmax()), q.shape)[:2])

    ratio("bands", np.abs(o[..., :NB] - ref[..., :NB]), an.bound[..., :NB])
    ratio("centroid", np.abs(o[..., NB + 1] - ref[..., NB + 1]) / hz, an.bound[..., NB + 1])
    ratio("entropy", np.abs(o[..., NB + 2] - ref[..., NB + 2]), an.bound[..., NB + 2])
    kf = o[..., NB] * W / hz
    k = np.round(kf)
    # two fp32 roundings (k * hz, / W): the reported frequency is within 1e-6 k of bin k
    isbin = (np.abs(kf - k) <= 1e-6 * np.maximum(k, 1)) & (k >= 1) & (k <= K)
    ki = np.clip(k, 1, K).astype(np.int64) - 1
    pk = np.take_along_axis(an.P, ki[..., None], 2)[..., 0]
    pmax = an.P.max(2)
    short = (pmax - pk) / np.maximum(2 * an.rho * pmax, 1e-300)
    short = np.where(pk >= pmax, 0.0, short)
    short = np.where(isbin, short, np.inf)
    for (w, a) in impulse_rows:
        short[w, a] = 0.0 if (isbin[w, a] and k[w, a] == 1) else np.inf
    short = np.where(live, short, 0.0)
    res["dominant"] = float(short.max())
    res["where"]["dominant"] = tuple(int(i) for i in np.unravel_index(int(short.argmax()), short.shape))
    return res


def worst(res: dict) -> float:
    """One number for a mutant: the largest ratio; inf where a hard demand (finite, flat rows) fails."""
    if not res["finite"] or res["flat"]:
        return float("inf")
    return max(res["bands"], res["centroid"], res["entropy"], res["dominant"])


def impulse_rows_of(shape) -> tuple:
    rows = _samples(shape)[1]
    return (rows["impulse"],) if "impulse" in rows and shape[1] % 2 == 0 else ()


def check(out, shape, label: str = "") -> dict:
    """Assert the rows ``out`` (fp32 [nwin, 11 A], on the CPU) of a table row against the oracle with the
    derived bounds, printing every largest ``error / bound`` first."""
    A, W, stride, nwin = shape[:4]
    assert tuple(out.shape) == (nwin, NFA * A) and out.dtype == torch.float32
    res = measure(out.numpy(), reference(shape), analyse(shape), W, HZ, impulse_rows_of(shape))
    report(res, shape_id(shape) + label)
    verdict(res)
    return res


def report(res: dict, label: str) -> None:
    print("%s: error / bound  bands %.3g  centroid %.3g  entropy %.3g  dominant shortfall / (2 rho) %.3g  at %s"
          % (label, res["bands"], res["centroid"], res["entropy"], res["dominant"], res["where"]))


def verdict(res: dict) -> None:
    assert res["finite"], "non-finite output (the NaN poison around the stream, or a non-finite entropy)"
    assert res["flat"] == 0, "a constant axis-window has non-zero columns"
    for name in ("bands", "centroid", "entropy", "dominant"):
        assert res[name] <= 1.0, "%s: error / bound = %g at (window, axis) %s" % (name, res[name], res["where"][name])


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
