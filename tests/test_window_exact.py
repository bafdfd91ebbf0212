"""Preconditions of the exact-count window tests (tests/test_gpu_window_exact.py), on the CPU: the stream of
``_window_util.int_stream`` really has the properties that let the GPU test demand exact bin counts, exact
peak sets and bit-equal extrema from the kernels, and the dispatch table it runs matches the launcher's rules.
If a seed violates one of these, change the seed (``_window_util.seed_of``), never a bound.

Also the preconditions of tests/test_gpu_window_degenerate.py: the streams with an axis whose bin scale
``10 / range`` is huge or overflows fp32, and the fp32 emulation of the kernels' documented rule for them."""
import numpy as np
import pytest
import torch

import _window_util as U
from har.features.window import n_features, window_count, window_features_torch


def _windows(shape):
    """float64 [nwin, A, W] windows of the exact stream and the integer draws in the same layout."""
    A, W, stride = shape[:3]
    es = U.int_stream(shape)
    x = es.view().double().unfold(0, W, stride)
    v = torch.from_numpy(es.ints.copy()).unfold(0, W, stride)
    assert x.shape == (U.n_windows(shape), A, W)
    return x, v


def test_dispatch_table_matches_launcher_rules():
    """Every table row as ``launch_axes`` (csrc/kernels/window.hip) decides it, for fp32 and MLP rows and for
    aligned and unaligned streams: the group width is the smallest of 8 (overlapping windows only) / 16 / 32 /
    64 lanes with an odd run C <= 31 and lanes * C >= W; the block takes the most waves (a multiple of the
    triads, at most 4) whose staged span fits 48 KB.  Spot values of the hand derivation:

    * (3, 248, 124): 4 waves stage (12 + (31 * 124 + 248) * 3 + 16) * 4 = 49,216 bytes > 49,152, so 3 waves,
      24 windows per block;
    * (3, 1984, 1984): two windows are (12 + 3968 * 3 + 16) * 4 = 47,728 bytes (48,176 with the MLP rows'
      112-float normalization image), three do not fit: 2 windows per block;
    * (6, 1100, 1100): two windows (52,912 bytes) do not fit, one 2-wave block per window;
    * (3, 200, 200) pads its images to 624 floats and (9, 200, 200) to 1808 (both 16 mod 32) on a 16-byte
      aligned stream only; 208 x 3 = 624 and 48 x 3 = 144 are 16 mod 32 already and 195 x 3 is no multiple of
      4: those three are never padded;
    * W = 1985 / 1986 exceed 64 x 31: the fallback kernel, image pitch 6000 = 48 mod 64, 96,112 bytes for the
      four images of a 1-wave block."""
    for shape in U.SHAPES:
        A, W, stride, kind, lpw, C, wpb = shape
        for aligned in (True, False):
            for mlp in (False, True):
                k, l, c, D, w, ipw = U.dispatch(A, W, stride, aligned, mlp)
                assert (k, l, c, w) == (kind, lpw, C, wpb), (shape, aligned, mlp)
                if kind != "fb":
                    assert D == lpw * C - W and c % 2 == 1 and c <= 31
                if not aligned:
                    assert kind == "fb" or ipw == 0
    pitch = {s[:3]: U.dispatch(*s[:3])[5] for s in U.SHAPES}
    assert pitch[(3, 200, 200)] == 624 and pitch[(9, 200, 200)] == 1808 and pitch[(3, 64, 64)] == 208
    assert pitch[(3, 208, 208)] == pitch[(3, 195, 195)] == pitch[(3, 48, 48)] == 0
    assert pitch[(3, 1985, 1000)] == pitch[(3, 1986, 1000)] == 6000
    D = {s[:3]: U.dispatch(*s[:3])[3] for s in U.SHAPES}
    assert [D[k] for k in ((3, 200, 100), (3, 193, 97), (3, 97, 40), (3, 240, 80), (3, 248, 124), (3, 200, 200),
                           (3, 208, 208), (3, 195, 195), (3, 48, 48), (3, 64, 64), (9, 500, 500), (3, 700, 350),
                           (6, 1100, 1100), (3, 1984, 1984), (3, 3, 1), (3, 5, 2), (6, 16, 3), (9, 33, 11))] == \
        [0, 7, 7, 8, 0, 8, 0, 13, 32, 16, 44, 36, 116, 0, 37, 35, 24, 7]
    assert (U.n_samples((3, 1985, 1000, "fb", 16, 125, 4)) * 3) % 4 == 3
    assert (U.n_samples((3, 1986, 1000, "fb", 16, 125, 4)) * 3) % 4 == 2
    # the unaligned bases give every 16-byte phase of the stream's first float
    assert sorted({(r0 * 3 * 4) % 16 for r0 in U.offsets(3)}) == [0, 4, 8, 12]
    assert [(r0 * 6 * 4) % 16 for r0 in U.offsets(6)] == [0, 8] and [(r0 * 9 * 4) % 16 for r0 in U.offsets(9)] == [0, 4]


def test_stream_buffer_is_poisoned_and_offset_independent():
    shape = U.SHAPES[1]
    a, b = U.int_stream(shape, 0), U.int_stream(shape, 3)
    assert torch.equal(a.view(), b.view()) and a.S == U.n_samples(shape)
    assert window_count(a.S, shape[1], shape[2]) == U.n_windows(shape)
    assert (a.S - shape[1]) % shape[2] == 0  # nothing after the last window
    assert b.buf.shape[0] == 3 + b.S + U.TAIL and U.TAIL * shape[0] >= 64
    assert bool(torch.isnan(b.buf[:3]).all()) and bool(torch.isnan(b.buf[3 + b.S:]).all())
    assert not bool(torch.isnan(b.view()).any())
    assert sum(s.stop - s.start for s in a.cols.values()) == n_features(shape[0])


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_id)
def test_exact_stream_preconditions(shape):
    x, v = _windows(shape)
    _preconditions(shape, x, v, U.reference(shape).double())


def test_shard_stream_preconditions():
    """The stream of the shard test (the 1B-pass shape, its windows starting 63 samples into the shard: the
    planted blocks are aligned to the shard, not to the windows)."""
    shape = U.SHAPES[0]
    A, W, stride = shape[:3]
    es = U.int_stream(shape, S=U.shard_len(shape))
    seg = es.view()[U.SHARD_SKIP:]
    assert window_count(seg.shape[0], W, stride) == U.n_windows(shape) and (U.SHARD_SKIP * A * 4) % 16 == 4
    x = seg.double().unfold(0, W, stride)
    v = torch.from_numpy(es.ints[U.SHARD_SKIP:].copy()).unfold(0, W, stride)
    _preconditions(shape, x, v, window_features_torch(seg, W, stride, U.HZ).double())


def _preconditions(shape, x, v, ref):
    A, W, stride, kind, lpw, C, wpb = shape
    c = U.columns(A)
    sc = torch.tensor([U.SCALE[a % 3] for a in range(A)], dtype=torch.float64)
    of = torch.tensor([U.OFF[a % 3] for a in range(A)], dtype=torch.float64)
    # range exactly 10 * scale, extrema exactly the planted ones (float32 values, so bit-equal is possible)
    assert torch.equal(ref[:, c["min"]], of.expand_as(ref[:, c["min"]]))
    assert torch.equal(ref[:, c["max"]], (10 * sc + of).expand_as(ref[:, c["max"]]))
    # every sum and sum of squares (run positions past the window included: up to 64 * 31 samples) is an
    # integer multiple of 1/4 below 2^24 / 4 ... exact in fp32
    assert float((x * x).sum(-1).max()) * 4 * max(1.0, lpw * C / W if kind != "fb" else 1.0) < 2 ** 24
    # integer counts, and the oracle's bins are the integer histogram of the draws (10 folded into bin 9)
    cnt = ref[:, c["bins"]] * W
    assert float((cnt - cnt.round()).abs().max()) <= 1e-3
    hist = torch.nn.functional.one_hot(v.clamp(max=9), 10).sum(-2).reshape(x.shape[0], A * 10)
    assert torch.equal(cnt.round().long(), hist)
    assert bool((hist.reshape(-1, A, 10).sum(-1) == W).all())
    # the peak threshold is far from every sample it does not equal ...
    mean = x.mean(-1)
    mx = x.max(-1).values
    thr = mean + 0.5 * (mx - mean)
    gap = (x - thr[..., None]).abs() / sc[None, :, None]
    assert float(gap[gap > 0].min()) >= 1e-3
    # ... and where a sample equals it in float64, fp32 agrees: the kernels' mean is the exact sum times
    # fl(1 / W) (also tried one ulp either way), the threshold mean + 0.5 * (max - mean) with every
    # operation rounded (the halving is exact, so a fused multiply-add gives the same)
    S32 = x.sum(-1).numpy().astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), x.sum(-1).numpy())
    inv = np.float32(1.0) / np.float32(W)
    x32, mx32 = x.numpy().astype(np.float32), mx.numpy().astype(np.float32)
    above = (x > thr[..., None]).numpy()
    for iw in (np.nextafter(inv, np.float32(0)), inv, np.nextafter(inv, np.float32(1))):
        m32 = (S32 * iw).astype(np.float32)
        t32 = (m32 + np.float32(0.5) * (mx32 - m32).astype(np.float32)).astype(np.float32)
        assert np.array_equal(x32 > t32[..., None], above)
    # peaks (the oracle's rule), plateaus, and plateau peaks on the last sample of a lane's run
    mid = x[..., 1:-1]
    pk = (mid > x[..., :-2]) & (mid >= x[..., 2:]) & (mid > thr[..., None])
    npk = pk.sum(-1)
    assert torch.equal(npk >= 2, ~torch.isnan(ref[:, c["peak"]]))
    plateau = (mid > x[..., :-2]) & (mid == x[..., 2:])
    assert int(plateau.sum()) > 0
    if W > 5:
        assert float((npk >= 2).double().mean()) > 0.5
    if W >= 33:
        assert int((npk < 2).sum()) == 0
    if kind != "fb" and W >= 33:
        t = torch.arange(1, W - 1)
        assert int((pk & plateau & (t % C == C - 1)).sum()) > 0, "no plateau peak closes a lane's run"
        assert int((pk & (t % C == 0)).sum()) > 0, "no peak opens a lane's run"


def _degenerate(shape, q):
    """The degenerate stream of a row, its emulated counts / scaled samples and the integer draws per window."""
    A, W, stride = shape[:3]
    es = U.degenerate_stream(shape, q)
    counts, p = U.degenerate_bins_fp32(es.view(), W, stride, scaled=True)
    v = torch.from_numpy(es.ints.copy()).unfold(0, W, stride)
    assert counts.shape == (U.n_windows(shape), A, 10) and p.shape == v.shape
    return es, counts, p, v


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_id)
def test_degenerate_stream_is_the_exact_stream_with_a_tiny_second_axis(shape):
    A, W, stride = shape[:3]
    base = U.int_stream(shape)
    for q in U.DEGENERATE_Q:
        es = U.degenerate_stream(shape, q, 1)
        x = es.view()
        assert torch.equal(es.view(), U.degenerate_stream(shape, q).view()) and es.S == base.S
        assert bool(torch.isnan(es.buf[:1]).all()) and bool(torch.isnan(es.buf[1 + es.S:]).all())
        for a in range(A):
            if a % 3 != 1:
                assert torch.equal(x[:, a], base.view()[:, a])
                continue
            assert np.array_equal(x[:, a].double().numpy(), es.ints[:, a] * q)   # v * q, exact
            w = x[:, a].unfold(0, W, stride)
            assert bool((w.min(-1).values == 0).all()) and bool((w.max(-1).values == np.float32(10 * q)).all())
        # the three regimes: a finite scale of exactly 2^123; an overflowing one over a normal range with
        # normal and denormal samples; the same with every sample denormal
        rng = torch.tensor(10 * q, dtype=torch.float32)
        tiny = float(np.finfo(np.float32).tiny)
        if q == 2.0 ** -123:
            assert float(10.0 / rng) == 2.0 ** 123
        else:
            assert bool(torch.isinf(10.0 / rng)) and float(rng) > 0
            pos = x[:, 1][x[:, 1] > 0]
            assert bool((pos < tiny).all()) == (q == 2.0 ** -130)
            if W >= 33:  # (shorter windows hold little beside the planted 0 and 10)
                assert bool((pos < tiny).any())
            assert (float(rng) >= tiny) == (q == 2.0 ** -128)


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_id)
def test_degenerate_emulation_equals_the_oracle_where_the_scale_is_finite(shape):
    """q = 2^-123: ``10 / range`` is exactly 2^123 and ``(x - lo) * sc`` the integer draw, so the fp32 rule
    must give the float64 oracle's bins on every axis — the saturation touches no legitimate small range."""
    A, W = shape[:2]
    q = 2.0 ** -123
    es, counts, p, v = _degenerate(shape, q)
    ref = U.degenerate_reference(shape, q).double()
    want = torch.round(ref[:, es.cols["bins"]] * W).long().view(-1, A, 10)
    assert torch.equal(counts, want)
    assert torch.equal(p.double(), v.double())
    assert torch.equal(counts, torch.nn.functional.one_hot(v.clamp(max=9), 10).sum(-2))


@pytest.mark.parametrize("q", U.DEGENERATE_Q[1:], ids=["2^-128", "2^-130"])
@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_id)
def test_degenerate_emulation_counts_where_the_scale_overflows(shape, q):
    """``10 / range`` = +inf: with the scale saturated at FLT_MAX the ten counts of such an axis are integers
    >= 0 that sum to W, every sample equal to the window's minimum lies in bin 0, and ``(x - lo) * sc`` stays
    below 11 (here: below 10, since range * FLT_MAX < 10 wherever 10 / range overflows).  In closed form
    ``v q * FLT_MAX`` is ``v (1 - 2^-24)`` at q = 2^-128 (bin v - 1, draw 0 in bin 0) and a quarter of that at
    q = 2^-130 (bin ceil(v / 4) - 1).  The other axes keep the oracle's bins."""
    A, W = shape[:2]
    es, counts, p, v = _degenerate(shape, q)
    assert counts.dtype == torch.int64 and bool((counts >= 0).all()) and bool((counts.sum(-1) == W).all())
    ref = U.degenerate_reference(shape, q).double()
    want = torch.round(ref[:, es.cols["bins"]] * W).long().view(-1, A, 10)
    for a in range(A):
        if a % 3 != 1:
            assert torch.equal(counts[:, a], want[:, a])
            continue
        pa, va = p[:, a], v[:, a]
        assert bool(torch.isfinite(pa).all()) and float(pa.max()) < 11 and float(pa.max()) < 10 and float(pa.min()) == 0
        assert bool((pa[va == 0] == 0).all()) and int(counts[:, a, 0].min()) >= 1
        assert bool((counts[:, a, 0] >= (va == 0).sum(-1)).all())
        b = (va - 1).clamp(min=0) if q == 2.0 ** -128 else ((va + 3) // 4 - 1).clamp(min=0)
        assert torch.equal(counts[:, a], torch.nn.functional.one_hot(b, 10).sum(-2))
        assert not torch.equal(counts[:, a], want[:, a])   # (the float64 definition's bins: not the fp32 rule's)


def test_check_exact_on_an_axis_subset():
    """``check_exact(axes=...)`` takes the per-axis columns of those axes only: an edit of another axis or of
    a per-triad column passes, the same edits as below on a chosen axis do not."""
    shape = U.SHAPES[2]
    A, W = shape[0], shape[1]
    ref = U.reference(shape)
    c = U.columns(A)
    keep = [a for a in range(A) if a % 3 != 1]
    assert U.axis_columns(A, "bins", [1]) == list(range(10, 20)) and U.axis_columns(A, "max", [0, 5]) == [
        c["max"].start, c["max"].start + 5]
    out = ref.clone()
    out[:, U.axis_columns(A, "bins", [1, 4])] = 7.0
    out[:, U.axis_columns(A, "std", [4])] = float("nan")
    out[:, c["corr"]] = float("nan")
    out[:, c["resultant"]] = -1.0
    U.check_exact(out, ref, A, W, axes=keep)
    with pytest.raises(AssertionError):
        U.check_exact(out, ref, A, W)
    for name, a in (("bins", 0), ("bins", 5), ("min", 2), ("energy", 3), ("std", 0), ("peak", 5)):
        bad = ref.clone()
        col = U.axis_columns(A, name, [a])[0]
        bad[3, col] = float("nan") if name == "peak" else bad[3, col] + 1.0 / W
        with pytest.raises(AssertionError):
            U.check_exact(bad, ref, A, W, axes=keep)


def test_check_exact_rejects_one_moved_sample():
    """The checker itself: the oracle's rows pass; one sample moved between two bins, an extremum one ulp
    off, a peak gained or a NaN outside the peak columns do not."""
    shape = U.SHAPES[1]
    A, W = shape[0], shape[1]
    ref = U.reference(shape)
    c = U.columns(A)
    U.check_exact(ref.clone(), ref, A, W)

    def bad(edit):
        out = ref.clone()
        edit(out)
        with pytest.raises(AssertionError):
            U.check_exact(out, ref, A, W)

    def move(o):
        o[5, 3] += 1.0 / W
        o[5, 4] -= 1.0 / W

    def one_ulp(o):
        o[2, c["max"].start] = float(np.nextafter(np.float32(o[2, c["max"].start]), np.float32(100)))

    def peak_lost(o):
        o[7, c["peak"].start + 1] = float("nan")

    def peak_count(o):  # npk one too many at the same first / last
        o[7, c["peak"].start] *= 1 - 1.0 / 6

    def poison(o):
        o[0, c["corr"].start] = float("nan")

    def avg(o):
        o[1, c["avg"].start] *= 1 + 4e-7

    for e in (move, one_ulp, peak_lost, peak_count, poison, avg):
        bad(e)
