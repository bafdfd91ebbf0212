"""The exact-arithmetic stream, the dispatch table and the column checks shared by tests/test_window_exact.py
(CPU: the preconditions) and tests/test_gpu_window_exact.py (the window kernels against the float64 oracle).

The stream holds small integers pushed through an exact affine map per axis, so that in fp32 as in fp64

* every (window, axis) has min and max exactly ``off`` and ``10 scale + off`` (range 10, 20 or 5), so the bin
  scale ``10 / range`` is exactly 1, 0.5 or 2 and ``(x - lo) * scale`` is an exact integer 0..10: no sample can
  move between bins, and a count that is off by one is a wrong kernel, not a rounding;
* every sum and sum of squares is exact (< 2^24 in units of 1/4), so avg and energy carry only the roundings
  of ``1 / W`` and one product;
* the peak threshold ``mean + (max - mean) / 2`` is far (>= 1e-3) from every sample it does not equal, so the
  set of peaks — hence ``npk``, ``first`` and ``last`` — is the same in both precisions;
* neighbouring samples are often equal: the ``x > prev && x >= next`` rule's plateau half decides peaks.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

HZ = 50.0                     # 20 ms per sample: exact in fp32
SCALE = (1.0, 2.0, 0.5)       # axis c of a triad: x = v * SCALE[c] + OFF[c], v an integer in 0..10
OFF = (0.0, -8.0, 3.0)
TAIL = 32                     # samples of NaN after the stream (>= 64 floats for 3 axes)

# (axes, W, stride, kernel, lanes per group, run length C, windows per block) — the dispatch table, re-derived
# from ``launch_axes`` (csrc/kernels/window.hip) by ``dispatch`` below; tests/test_window_exact.py holds the
# two against each other.  "fix": the fixed-length-run instantiations (8 x 25, 16 x 13); "reg": the runtime-C
# register kernel (17- or 31-register instantiation); "fb": the one-image-per-window fallback kernel.
SHAPES = [
    (3, 200, 100, "fix", 8, 25, 32),     # D = 0: the 1B-sample pass
    (3, 193, 97, "fix", 8, 25, 32),      # D = 7
    (6, 200, 100, "fix", 8, 25, 16),     # two triads
    (3, 97, 40, "reg", 8, 13, 32),       # 17-register instantiation, D = 7
    (3, 240, 80, "reg", 8, 31, 32),      # 31-register instantiation, D = 8
    (3, 248, 124, "reg", 8, 31, 24),     # D = 0; 3-wave block (4 waves: 49,216 bytes > 48 KB)
    (3, 200, 200, "fix", 16, 13, 16),    # D = 8; padded images (pitch 624) on an aligned stream
    (9, 200, 200, "fix", 16, 13, 4),     # padded (pitch 1808), three triads
    (3, 208, 208, "fix", 16, 13, 16),    # D = 0; 624 % 32 == 16: never padded
    (3, 195, 195, "fix", 16, 13, 16),    # D = 13; 585 % 4 != 0: never padded
    (3, 48, 48, "reg", 16, 5, 16),       # D = 32; 144 % 32 == 16: never padded
    (3, 64, 64, "reg", 16, 5, 16),       # D = 16; padded (pitch 208)
    (9, 500, 500, "reg", 32, 17, 2),     # D = 44
    (3, 700, 350, "reg", 32, 23, 8),     # D = 36
    (6, 1100, 1100, "reg", 64, 19, 1),   # D = 116
    (3, 1984, 1984, "reg", 64, 31, 2),   # D = 0
    (3, 1985, 1000, "fb", 16, 125, 4),   # n_samples * A % 4 == 3
    (3, 1986, 1000, "fb", 16, 125, 4),   # n_samples * A % 4 == 2
    (3, 3, 1, "reg", 8, 5, 32),          # D = 37
    (3, 5, 2, "reg", 8, 5, 32),          # D = 35
    (6, 16, 3, "reg", 8, 5, 16),         # D = 24
    (9, 33, 11, "reg", 8, 5, 8),         # D = 7
]


def shape_id(shape) -> str:
    return "%dx%d/%d" % shape[:3]


def offsets(axes: int):
    """Base offsets (samples) of the stream inside its buffer: every 16-byte phase of a 3-axis stream."""
    return (0, 1, 2, 3) if axes == 3 else (0, 1)


def n_windows(shape) -> int:
    """Two full blocks and a last block that holds one window."""
    return 2 * shape[6] + 1


def n_samples(shape) -> int:
    return (n_windows(shape) - 1) * shape[2] + shape[1]


SHARD_SKIP = 63  # the shard test's first owned window starts this many samples into the shard


def shard_len(shape) -> int:
    """Samples of the shard test's shard: the skipped ones, the row's windows, and 17 that no window takes."""
    return SHARD_SKIP + n_samples(shape) + 17


def _nrm_floats(A: int) -> int:
    return (2 * (17 * A + 4 * (A // 3)) + 3) & ~3


def dispatch(A: int, W: int, stride: int, aligned: bool = True, mlp: bool = False):
    """``launch_axes`` in Python: (kernel, lanes per group, C, D, windows per block, padded image pitch or 0)."""
    T3 = A // 3
    lpw = C = 0
    lanes = 8 if stride < W else 16
    while lanes <= 64 and not lpw:
        for c in range(5, 32, 2):
            if lanes * c >= W:
                lpw, C = lanes, c
                break
        lanes *= 2
    NR = _nrm_floats(A) if mlp else 0
    if lpw:
        gpw = 64 // lpw
        pimg = lpw == 16 and A % 2 == 1 and stride == W and (W * A) % 4 == 0 and aligned and (W * A) % 32 != 16
        ipw = W * A + (16 - W * A) % 32 if pimg else 0
        fixc = (lpw, C) in ((8, 25), (16, 13))
        slack = max(16, (lpw * C - W) * A + 4) if fixc else 16

        def span_bytes(wpb):
            if ipw:
                return 4 * (NR + 12 + wpb * ipw + slack)
            return 4 * (NR + 12 + ((wpb - 1) * stride + W) * A + slack)

        m = 0
        for mm in range(4 // T3, 0, -1):
            if span_bytes(mm * gpw) <= 48 * 1024:
                m = mm
                break
        if not m and span_bytes(gpw) <= 160 * 1024:
            m = 1
        if m:
            return ("fix" if fixc else "reg"), lpw, C, lpw * C - W, m * gpw, ipw
    n = W * A

    def conflict_free(pitch):
        return len({((lane // 16) * pitch + (lane % 16) * A) % 64 for lane in range(64)}) == 64

    pitch = n
    if not (stride == W and n % 4 == 0 and (conflict_free(n) or A % 2 == 0)):
        want = (16 * A) % 64 if A % 2 else 32
        pitch = n + (want - n) % 64
    waves = 0
    for w in range(4, 0, -1):
        if w % T3 == 0 and 4 * (12 + (4 * w // T3) * pitch + 16) <= 64 * 1024:
            waves = w
            break
    if not waves and 4 * (12 + 4 * pitch + 16) <= 160 * 1024:
        waves = T3
    if not waves:
        return "wide", 16, (W + 15) // 16, 0, 0, 0
    return "fb", 16, (W + 15) // 16, 0, 4 * waves // T3, pitch


def columns(A: int):
    """The column slices of a feature row for A axes."""
    T3 = A // 3
    o, cols = 0, {}
    for name, n in (("bins", 10 * A), ("avg", A), ("peak", A), ("absdev", A), ("std", A), ("resultant", T3),
                    ("min", A), ("max", A), ("energy", A), ("corr", 3 * T3)):
        cols[name] = slice(o, o + n)
        o += n
    assert o == 17 * A + 4 * T3
    return cols


EXACT_COLS = ("bins", "min", "max", "avg", "energy")   # independent of summation order and precision
LOOSE_COLS = ("absdev", "std", "resultant", "corr")


@lru_cache(maxsize=None)
def int_draws(S: int, A: int, W: int, seed: int) -> np.ndarray:
    """[S, A] integers in 0..10, i.i.d., with one 0 and one 10 planted per axis at seeded positions of every
    aligned block of ``p = (W + 1) // 2`` samples.  A window of W >= 2 p - 1 samples holds a whole block
    wherever it starts, so every (window, axis) has min 0 and max 10."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 11, size=(S, A))
    p = (W + 1) // 2
    for b0 in range(0, S, p):
        n = min(p, S - b0)
        if n < 2:
            continue  # (a partial last block: no window relies on it)
        for a in range(A):
            i, j = rng.choice(n, 2, replace=False)
            v[b0 + i, a] = 0
            v[b0 + j, a] = 10
    v.setflags(write=False)
    return v


@dataclass
class ExactStream:
    buf: torch.Tensor      # fp32 [r0 + S + TAIL, A]: NaN, the stream, NaN
    r0: int
    S: int
    ints: np.ndarray       # [S, A] the integer draws
    cols: dict

    def view(self, buf: torch.Tensor = None) -> torch.Tensor:
        """The stream inside ``buf`` (default: the host buffer; pass a device copy of it)."""
        b = self.buf if buf is None else buf
        return b[self.r0: self.r0 + self.S]


def seed_of(shape) -> int:
    A, W, stride = shape[:3]
    return 1000 * A + 7 * W + stride


def int_stream(shape, r0: int = 0, seed: int = None, S: int = None) -> ExactStream:
    """The exact stream of one table row (``S`` samples; default: exactly the row's ``n_windows``), ``r0``
    samples into a NaN-filled buffer with TAIL samples of NaN after it: a read outside ``[0, S)`` that reaches
    a result shows up as NaN.  The samples do not depend on ``r0``."""
    A, W = shape[0], shape[1]
    S = n_samples(shape) if S is None else S
    v = int_draws(S, A, W, seed_of(shape) if seed is None else seed)
    sc = np.array([SCALE[c % 3] for c in range(A)])
    of = np.array([OFF[c % 3] for c in range(A)])
    x = (v * sc + of).astype(np.float32)
    buf = torch.full((r0 + S + TAIL, A), float("nan"), dtype=torch.float32)
    buf[r0: r0 + S] = torch.from_numpy(x)
    return ExactStream(buf, r0, S, v, columns(A))


DEGENERATE_Q = (2.0 ** -123, 2.0 ** -128, 2.0 ** -130)
FLT_MAX = float(np.finfo(np.float32).max)


def degenerate_stream(shape, q: float, r0: int = 0) -> ExactStream:
    """``int_stream`` with the second axis of every triad replaced by ``v * q`` (``q`` a power of two,
    offset 0): every (window, axis) of it has min 0 and max ``10 q``.  The other axes keep the exact stream.

    q = 2^-123: range 10 * 2^-123, bin scale exactly 2^123 — a small but legitimate range;
    q = 2^-128: range 10 * 2^-128 = 1.25 * 2^-125 (a normal float), ``10 / range`` = 2^128 overflows fp32; the
                samples ``v q`` are denormal for v <= 3 and normal above;
    q = 2^-130: the same with every sample (v <= 10 < 16) denormal."""
    es = int_stream(shape, r0)
    A = shape[0]
    x = torch.from_numpy(es.ints.astype(np.float64) * q).float()
    assert torch.equal(x.double(), torch.from_numpy(es.ints.astype(np.float64) * q)), "v * q must be exact in fp32"
    buf = es.buf.clone()
    for a in range(1, A, 3):
        buf[r0: r0 + es.S, a] = x[:, a]
    return ExactStream(buf, r0, es.S, es.ints, es.cols)


def degenerate_bins_fp32(x: torch.Tensor, W: int, stride: int, scaled: bool = False):
    """The window kernels' bin arithmetic in plain fp32 torch on the CPU, denormals kept as the kernels keep
    them (their code objects run with fp32 denormals on): per (window, axis)

        range = max - min
        sc    = 0                               if range == 0 (a flat axis: every sample in bin 0)
                min(fl(10 / range), FLT_MAX)    otherwise (the scale saturates where 10 / range overflows)
        bin   = min(trunc(fl(fl(x - min) * sc)), 9)

    Returns the int64 counts [n_windows, A, 10] (``scaled``: also the products ``(x - min) * sc``)."""
    assert x.dtype == torch.float32 and not x.is_cuda
    tiny = torch.tensor([2.0 ** -130], dtype=torch.float32)
    assert float(tiny * 0.5) == 2.0 ** -131, "this process flushes fp32 denormals: the emulation needs them"
    w = x.unfold(0, W, stride)                                   # [nw, A, W]
    lo, hi = w.min(-1).values, w.max(-1).values
    rng = hi - lo
    sc = torch.where(rng > 0, (10.0 / rng).clamp_max(FLT_MAX), torch.zeros_like(rng))
    p = (w - lo[..., None]) * sc[..., None]
    assert p.dtype == torch.float32
    counts = torch.nn.functional.one_hot(p.to(torch.int64).clamp_max(9), 10).sum(-2)
    return (counts, p) if scaled else counts


@lru_cache(maxsize=None)
def degenerate_reference(shape, q: float) -> torch.Tensor:
    """The float64 oracle's rows of ``degenerate_stream(shape, q)`` (computed once; do not modify)."""
    from har.features.window import window_features_torch

    return window_features_torch(degenerate_stream(shape, q).view(), shape[1], shape[2], HZ)


@lru_cache(maxsize=None)
def reference(shape) -> torch.Tensor:
    """The float64 oracle's rows for a table row (computed once; do not modify)."""
    from har.features.window import window_features_torch

    es = int_stream(shape)
    return window_features_torch(es.view(), shape[1], shape[2], HZ)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def axis_columns(A: int, name: str, axes) -> list:
    """Column indices of the per-axis feature ``name`` (10 per axis for "bins", else 1) for the given axes."""
    s = columns(A)[name]
    per = (s.stop - s.start) // A
    return [s.start + a * per + j for a in axes for j in range(per)]


def check_exact(out: torch.Tensor, ref: torch.Tensor, A: int, W: int, axes=None) -> None:
    """A kernel's fp32 rows against the float64 oracle's on the exact stream (both on the CPU).

    bins       |out W - round(ref W)| <= 1e-3: (x - lo) * sc is an exact integer, no sample may move
    min, max   bit-equal
    avg,       rtol 2.5e-7, atol 0: the sum is exact; one rounding of 1 / W, one of the product, one of the
    energy     reference: 3 * 2^-24 = 1.8e-7
    peak       same NaN pattern; rtol 1e-6: last - first and npk exact, v_rcp_f32 within 1 ulp (2^-23), two
               products and the reference's rounding: 5 * 2^-24 = 3.0e-7
    absdev, std, resultant, corr   rtol = atol = 2e-4, the tolerance tests/test_window.py uses
    all        no NaN outside the peak columns

    ``axes``: only the per-axis columns (bins, avg, peak, absdev, std, min, max, energy) of these axes, with
    the same bounds; the per-triad columns (resultant, corr) are then left out."""
    c = columns(A)
    assert out.shape == ref.shape and out.dtype == torch.float32
    if axes is None:
        sel = {name: list(range(s.start, s.stop)) for name, s in c.items()}
        loose = LOOSE_COLS
    else:
        sel = {name: axis_columns(A, name, axes) for name in c if name not in ("resultant", "corr")}
        loose = ("absdev", "std")
    o, r = out.double(), ref.double()
    notpeak = sorted(i for name, idx in sel.items() if name != "peak" for i in idx)
    assert not bool(torch.isnan(out[:, notpeak]).any()), "NaN outside the peak columns: a read outside the stream"
    cnt = o[:, sel["bins"]] * W
    want = torch.round(r[:, sel["bins"]] * W)
    err = (cnt - want).abs()
    assert float(err.max()) <= 1e-3, "bin counts differ: max |out W - count| = %g at %s" % (
        float(err.max()), tuple(int(i) for i in np.unravel_index(int(err.argmax()), err.shape)))
    for name in ("min", "max"):
        assert torch.equal(bits(out[:, sel[name]]), bits(ref[:, sel[name]])), name
    for name in ("avg", "energy"):
        torch.testing.assert_close(o[:, sel[name]], r[:, sel[name]], rtol=2.5e-7, atol=0, msg=lambda m, n=name: n + ": " + m)
    po, pr = o[:, sel["peak"]], r[:, sel["peak"]]
    assert torch.equal(torch.isnan(po), torch.isnan(pr)), "peak columns: NaN pattern (fewer than two peaks) differs"
    torch.testing.assert_close(po, pr, rtol=1e-6, atol=0, equal_nan=True, msg=lambda m: "peak: " + m)
    for name in loose:
        torch.testing.assert_close(out[:, sel[name]], ref[:, sel[name]], rtol=2e-4, atol=2e-4,
                                   msg=lambda m, n=name: n + ": " + m)
