"""Preconditions of the spectral probe tests (tests/test_gpu_spectral_exact.py), on the CPU: the plan table is
what ``make_plan`` (csrc/kernels/spectral.hip) decides, the probe stream of ``_spectral_util`` has the
properties its bounds rest on, the closed-form rows have their closed forms, and the checker, with those
bounds, rejects every float64 mutant of the definition by a factor of at least 4 on a sparse row of every
shape the mutant applies to.  The twiddle mutant is one wrong entry (k, n) for W <= 200 and every bin's index
at one sample on all shapes: one entry of a window of 500 samples or more moves no aggregate by 4 x the fp32
bound (the note above ``test_mutant_one_twiddle_entry_off_by_one``).  If a shape misses that factor, change the stream or its seed
(``_spectral_util.seed_of``), never the factor or a bound."""
import math

import numpy as np
import pytest
import torch

import _spectral_util as U
from har.features.spectral import spectral_features_torch, spectral_power_torch

FACTOR = 4.0


def test_plan_table_matches_launcher_rules():
    """Every table row as ``make_plan`` decides it.  ``bytes(wpb) = (tab_floats(W) + ((wpb - 1) stride + W) A
    + 4) * 4`` with ``tab_floats(W) = (2 W + 3) & ~3``; the first of 4, 2, 1 waves (``wpb = min(16 waves / A,
    n_windows)``) that fits 64 KB, else 160 KB, else the loop ``wpb = 16 / A - 1 .. 1``.  Spot values of the
    hand derivation:

    * (3, 200, 100): 21 windows are (400 + (20 * 100 + 200) * 3 + 4) * 4 = 28,016 bytes; 63 rows in 4 waves;
    * (3, 500, 250): 21 windows are 70,016 bytes > 65,536, so 2 waves, 10 windows, 37,016 bytes;
    * (3, 1024, 512): 10 windows are 75,792 bytes, so 1 wave, 5 windows, 45,072 bytes;
    * (9, 1500, 100): one window is 66,016 bytes > 64 KB, so the 160 KB budget at 4 waves: 7 windows, 87,616;
    * (9, 1500, 1000): 7 windows are 282,016 bytes, 3 windows (27 rows, 2 waves) 138,016;
    * (9, 2048, 2048): 3 windows are 237,584 bytes, one (9 rows) 90,128;
    * (3, 2047, 2047): tab_floats = 4096, 5 windows (4 * 2047 + 2047) * 3 floats: 139,220 bytes, K = 1023;
    * (3, 2048, 3000): 5 windows are 184,976 bytes > 163,840, so the loop: 4 windows, 148,976 bytes;
    * (6, 2048, 5000): 2 windows are 185,552 bytes, the loop's one window 65,552: 16 bytes over 64 KB;
    * (3, 200, 100) with 11 windows: wpb = 11, 33 rows, 3 waves; with one window: 3 rows, 1 wave."""
    for shape in U.SHAPES:
        assert U.plan(*shape[:4]) == shape[4:], shape
        A, W, stride, nwin, budget, wpb, waves, nbytes = shape
        assert nbytes <= (U.K64 if budget == "64K" else U.K160) and waves == (wpb * A + 15) // 16 <= 4
        if budget != "64K":
            assert U.staged_bytes(A, W, stride, min(16 // A, nwin)) > U.K64  # one wave's windows do not fit 64 KB
    sb = U.staged_bytes
    assert U.tab_floats(200) == 400 and U.tab_floats(193) == 388 and U.tab_floats(2047) == 4096 and U.tab_floats(3) == 8
    assert sb(3, 200, 100, 21) == 28016 and sb(6, 200, 100, 10) == 28016 and sb(9, 200, 200, 7) == 52016
    assert sb(3, 500, 250, 21) == 70016 > U.K64 >= sb(3, 500, 250, 10) == 37016
    assert sb(3, 1024, 512, 10) == 75792 > U.K64 >= sb(3, 1024, 512, 5) == 45072
    assert sb(9, 1500, 100, 1) == 66016 > U.K64 and sb(9, 1500, 100, 7) == 87616 <= U.K160
    assert sb(9, 1500, 1000, 7) == 282016 > U.K160 >= sb(9, 1500, 1000, 3) == 138016
    assert sb(9, 2048, 2048, 3) == 237584 > U.K160 >= sb(9, 2048, 2048, 1) == 90128
    assert sb(3, 2047, 2047, 5) == 139220
    assert sb(3, 2048, 3000, 5) == 184976 > U.K160 >= sb(3, 2048, 3000, 4) == 148976
    assert sb(6, 2048, 5000, 2) == 185552 > U.K160 and sb(6, 2048, 5000, 1) == 65552 == U.K64 + 16
    plans = {s[:4]: s[4:7] for s in U.SHAPES}
    assert plans[(3, 200, 100, 11)] == ("64K", 11, 3) and plans[(3, 200, 100, 1)] == ("64K", 1, 1)
    assert plans[(3, 200, 100, 22)] == ("64K", 21, 4) and plans[(3, 2048, 3000, 9)] == ("loop", 4, 1)
    # all ten outcomes of make_plan are in the table
    assert {(s[4], s[6]) for s in U.SHAPES} >= {(b, w) for b in ("64K", "160K") for w in (4, 2, 1)} | {("64K", 3)}
    assert sum(1 for s in U.SHAPES if s[4] == "loop") == 2
    # two full blocks and a last block of one window, except the short streams
    assert all(s[3] == 2 * s[5] + 1 for s in U.SHAPES[:16])
    # the one-window last block of (3, 193, 97): 579 floats, a 16-byte body of 144 float4 and a scalar tail of 3
    assert 193 * 3 == 579 and 579 % 4 == 3
    # the base offsets give every 16-byte phase of the stream's first float
    assert sorted({(r0 * 3 * 4) % 16 for r0 in U.offsets(3)}) == [0, 4, 8, 12]
    assert [(r0 * 6 * 4) % 16 for r0 in U.offsets(6)] == [0, 8] and [(r0 * 9 * 4) % 16 for r0 in U.offsets(9)] == [0, 4]


def test_probe_stream_is_poisoned_and_offset_independent():
    for shape in (U.SHAPES[3], U.SHAPES[2]):
        A, W, stride, nwin = shape[:4]
        r1 = U.offsets(A)[-1]
        a, b = U.probe_stream(shape, 0), U.probe_stream(shape, r1)
        assert torch.equal(a.view(), b.view()) and a.S == U.n_samples(shape) == (nwin - 1) * stride + W
        assert b.buf.shape[0] == r1 + b.S + U.TAIL and U.TAIL * A >= 64
        assert bool(torch.isnan(b.buf[:r1]).all()) and bool(torch.isnan(b.buf[r1 + b.S:]).all())
        assert not bool(torch.isnan(b.view()).any())
    p = U.impulse_stream(30, 2)
    assert p.S == 30 and bool(torch.isnan(p.buf[:2]).all()) and bool(torch.isnan(p.buf[32:]).all())


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_id)
def test_probe_stream_preconditions(shape):
    A, W, stride, nwin = shape[:4]
    K = W // 2
    an = U.analyse(shape)
    x, rows = U._samples(shape)
    assert x.dtype == np.float32 and x.shape == (U.n_samples(shape), A)
    # at least half of the rows live, at least one constant row, sparse rows on most of the live ones
    assert an.live.mean() >= 0.5 and int((~an.live).sum()) >= 1 and not an.live[rows["const"]]
    assert an.sparse.sum() * 2 >= an.live.sum() or W < 32
    # x - x[0] is exact in fp32 everywhere but in the pure tone; the non-zero d of a sparse row are powers of
    # two (+-0.5, +-1, +-2 where sample 0 has no spike), so their products with the twiddles are exact
    d = an.x - an.x[..., :1]
    exact = d.astype(np.float32).astype(np.float64) == d
    for w in range(nwin):
        for a in range(A):
            assert exact[w, a].all() or rows.get("tone") == (w, a)
    sp = d[an.sparse]
    assert np.isin(np.abs(sp), (0.0, 0.5, 1.0, 2.0, 4.0)).all() and (an.m[an.sparse] <= 64).all()
    # the planted spikes of the twiddle mutants sit in sparse rows
    (wl, al), (wt, at) = rows["last"], rows["tail"]
    assert an.sparse[wl, al] and d[wl, al, W - 1] == 2.0
    assert an.sparse[wt, at] and d[wt, at, U.tail_sample(W)] == -2.0
    assert W % 4 == 0 or U.tail_sample(W) >= W - W % 4 or W == 3
    # every bin of a sparse row carries O(1 / K) of the power: none more than m^2 / (m K) ... sum |d|^2 / T
    if K >= 8:
        share = an.P[an.sparse] / an.P[an.sparse].sum(-1, keepdims=True)
        assert float(share.max()) <= 16.0 / K
    # the oracle's float64 powers are the util's (pivot x[0] against the oracle's mean: rounding only)
    P = spectral_power_torch(U.probe_stream(shape).view(), W, stride).numpy()
    assert P.shape == an.P.shape
    assert float(np.abs(P - an.P).max()) <= 1e-9 * float(an.P.max())
    # ... and the oracle's rows are the util's float64 features to fp32 rounding; the oracle itself sits far
    # inside the bounds (it would otherwise eat the budget of the kernel)
    own = U.measure(U.to_rows(U.features64(an.x)), U.reference(shape), an, W, U.HZ)
    assert own["finite"] and own["flat"] == 0 and max(own["bands"], own["centroid"], own["entropy"]) <= 0.1
    # a plain fp32 model of the kernel's arithmetic stays inside the bounds
    emu = U.features32(an.x.reshape(-1, W)).reshape(nwin, A, U.NFA)
    res = U.measure(U.to_rows(emu), U.reference(shape), an, W, U.HZ, U.impulse_rows_of(shape))
    U.report(res, U.shape_id(shape) + " fp32 model")
    U.verdict(res)


@pytest.mark.parametrize("shape", [s for s in U.SHAPES if s[2] >= s[1]], ids=U.shape_id)
def test_closed_form_rows(shape):
    """The oracle's values of the planted rows equal their formulas (to float64 rounding of a W-term sum and
    the fp32 rounding of the oracle's output)."""
    A, W, stride, nwin = shape[:4]
    K = W // 2
    rows = U._samples(shape)[1]
    ref = U.reference(shape)
    an = U.analyse(shape)
    tol = 1e-6
    w, a = rows["const"]
    assert not an.live[w, a] and not ref[w, a].any()
    w, a = rows["spike0"]
    assert an.live[w, a] and not an.sparse[w, a] and an.m[w, a] >= W - 64
    w, a = rows["tone"]
    k0 = U.tone_bin(W)
    assert 16 * ((K + 15) // 16 - 1) < k0 <= K  # in the last bin tile
    assert ref[w, a, U.NB] == np.float32(k0 * U.HZ / W) and ref[w, a, ((k0 - 1) * 8) // K] > 1 - 1e-4
    assert abs(ref[w, a, U.NB + 1] - k0 * U.HZ / W) < 1e-3 * U.HZ and ref[w, a, U.NB + 2] < 1e-3
    if W % 2:
        assert "impulse" not in rows and "nyquist" not in rows
        return
    w, a = rows["nyquist"]
    want = np.zeros(U.NFA)
    want[7], want[U.NB], want[U.NB + 1] = 1.0, K * U.HZ / W, K * U.HZ / W
    assert np.abs(ref[w, a] - want).max() <= tol * U.HZ
    assert an.P[w, a, K - 1] == (U.NYQ_AMP * W) ** 2 and float(an.P[w, a, :K - 1].max()) < 1e-20 * an.P[w, a, K - 1]
    w, a = rows["impulse"]
    assert w == nwin - 1  # in the one-window last block
    want = U.impulse_expected(W)
    sel = [i for i in range(U.NFA) if i != U.NB]  # the oracle's own argmax is decided by its rounding noise
    assert np.abs(ref[w, a, sel] - want[sel]).max() <= tol * U.HZ
    # pivot x[0]: the entries touched are (+-1, ~1e-16) and every P_k is the same float64 and the same fp32
    assert (an.P[w, a] == 4.0).all()
    c, s, idx = U._table(W, K)
    assert set(np.abs(c[idx[:, W // 2]].astype(np.float32))) == {1.0}
    assert float(np.abs(s[idx[:, W // 2]]).max()) < 1e-15


@pytest.mark.parametrize("W", range(3, 73))
def test_centre_impulse_sweep_closed_form(W):
    """The one-window centre-impulse stream for every W in 3..72: flat spectrum, fractions bincount / K,
    entropy 1 (0 for K = 1), centroid hz (K + 1) / (2 W); an exact tie for even W."""
    K = W // 2
    p = U.impulse_stream(W)
    shape = p.shape
    assert shape[4:7] == ("64K", 1, 1)
    an = U.analyse_windows(U.windows_of(p.view().numpy(), W, W, 1))
    amp2 = np.array(U.IMPULSE_AMP) ** 2
    assert np.abs(an.P / amp2[None, :, None] - 1).max() <= 1e-12 and an.sparse.all() and (an.m == 1).all()
    if W % 2 == 0:
        assert (an.P == amp2[None, :, None]).all()
    ref = U.per_axis(spectral_features_torch(p.view(), W, W, U.HZ).numpy(), 3)
    want = np.tile(U.impulse_expected(W), (1, 3, 1))
    sel = [i for i in range(U.NFA) if i != U.NB]
    assert np.abs(ref[..., sel] - want[..., sel]).max() <= 1e-6 * U.HZ
    # the closed form passes the checker, "highest k" does not (even W, K > 1)
    imp = tuple((0, a) for a in range(3)) if W % 2 == 0 else ()
    ok = U.measure(U.to_rows(want), ref, an, W, U.HZ, imp)
    U.verdict(ok)
    if W % 2 == 0 and K > 1:
        bad = U.measure(U.to_rows(U.features64(an.x, tie_high=True)), ref, an, W, U.HZ, imp)
        assert U.worst(bad) == float("inf")


@pytest.mark.parametrize("W", U.STRUCTURED_W)
def test_structured_windows_reach_the_denormal_range(W):
    """Why tests/test_gpu_spectral_exact.py runs the clipped, square-ish windows: under a plain fp32 model of
    the kernel's accumulation a bin of them (the quarter-rate bin K / 2, whose table entries are 0, +-1 and
    ~1e-16) keeps a prescaled power that is positive and below the smallest normal fp32 number.  ``P ln P`` of
    such a power is below 2^-119 in magnitude, yet a logarithm that takes it for zero makes the entropy
    infinite.  The float64 definition is finite and inside its bounds."""
    probe = U.structured_stream(W)
    assert probe.shape[4:7] == ("64K", 1, 1)
    x = probe.view().numpy()
    P = U.model_powers(x.T.copy())
    tiny = np.finfo(np.float32).tiny
    assert int(((P > 0) & (P < tiny)).sum()) >= 1
    an = U.analyse_windows(U.windows_of(x, W, W, 1))
    assert an.live.all() and np.isfinite(an.bound).all() and float(an.bound.max()) < 1e-2
    ref = U.per_axis(spectral_features_torch(probe.view(), W, W, U.HZ).numpy(), 3)
    U.verdict(U.measure(U.to_rows(U.features64(an.x)), ref, an, W, U.HZ))


# ---------------------------------------------------------------------------------------------------------
# mutants


def _mutant(shape, **kw):
    """worst error / bound of a float64 mutant over the sparse rows of a shape (the other rows' bounds are
    wider: a dense row may hide what a sparse one shows)."""
    A, W, stride, nwin = shape[:4]
    an = U.analyse(shape)
    rows = U.to_rows(U.features64(an.x, **kw))
    keep = an.sparse.copy()
    for cell in U.impulse_rows_of(shape):
        keep[cell] = True
    return _worst_on(shape, rows, keep)


def _worst_on(shape, rows, keep):
    A, W = shape[:2]
    an = U.analyse(shape)
    ref = U.reference(shape)
    out = np.where(np.repeat(keep[..., None], U.NFA, 2), U.per_axis(rows, A), ref)
    # rows outside ``keep`` take the oracle's values; their dominant column must still be a bin
    out[..., U.NB] = np.where(keep, out[..., U.NB], (an.P.argmax(2) + 1) * U.HZ / W)
    out[~an.live] = 0.0
    return U.worst(U.measure(U.to_rows(out), ref, an, W, U.HZ, U.impulse_rows_of(shape)))


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_id)
def test_checker_accepts_the_definition_on_sparse_rows(shape):
    assert _mutant(shape) <= 0.1


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_id)
def test_mutant_last_bin_dropped(shape):
    assert _mutant(shape, drop_last=True) >= FACTOR


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_id)
def test_mutant_band_boundary_moved_up_by_one_bin(shape):
    assert _mutant(shape, band_shift=1) >= FACTOR


# K = 1: bin 1 can only move up
@pytest.mark.parametrize("shape", [s for s in U.SHAPES if s[1] // 2 > 1], ids=U.shape_id)
def test_mutant_band_boundary_moved_down_by_one_bin(shape):
    assert _mutant(shape, band_shift=-1) >= FACTOR


@pytest.mark.parametrize("shape", [s for s in U.SHAPES if U.impulse_rows_of(s)], ids=U.shape_id)
def test_mutant_tie_rule_highest_k(shape):
    assert _mutant(shape, tie_high=True) == float("inf")
    # ... and it is the centre-impulse row that says so
    w, a = U.impulse_rows_of(shape)[0]
    an = U.analyse(shape)
    keep = np.zeros_like(an.sparse)
    keep[w, a] = True
    assert _worst_on(shape, U.to_rows(U.features64(an.x, tie_high=True)), keep) == float("inf")
    assert _worst_on(shape, U.to_rows(U.features64(an.x)), keep) <= 1.0


# K = 1 (W = 3): a live row is (1, 0, ..., 0 | hz / 3, hz / 3, 0) whatever its one bin holds, so mutants that
# only change the bin's value do not apply
_SPECTRUM = [s for s in U.SHAPES if s[1] // 2 > 1]


# One wrong table entry (k, n) changes X_k by d_n (t[kn + 1] - t[kn]), |.| <= |d_n| 2 pi / W, hence P_k by at
# most 2 |X_k| |d_n| 2 pi / W and an aggregate by that over T ~ K sum d^2: for the two-spike rows (a, b) at
# most 2 a b / (a^2 + b^2) * 2 pi / (W K) <= 4 pi / W^2 of the total, and much less for most bins (the phase
# factor sin(2 pi k dn / W) of the pair).  At W = 2048 that is 3e-6 of the total, against a band bound of
# about (2 (ntiles + 4) + 4) u f = 1e-6 for f = 1 / 8 from the epilogue's fp32 sums alone: no stream makes one
# entry 4 x visible in the aggregates there, whichever bin it is in.  So the single-entry mutant runs where the
# aggregates can see it (W <= 200: every probed bin and both samples), and on every shape the mutant is the
# coarser "every bin's index at one sample" (the K entries a wrong index register or tail step would hit).
# Measured worst ratios of the single entry at n = W - 1 over the bins 1, K / 2, K: 3x500: 2.2 (bin K);
# 3x1024: 0.06; 9x1500 (both strides): 0.014; 9x2048, 3x2047, 3x2048/3000, 6x2048/5000: 0.005.
_SINGLE = [s for s in _SPECTRUM if s[1] <= 200]
_BLIND = [s for s in _SPECTRUM if s[1] >= 500]


@pytest.mark.parametrize("shape", _SINGLE, ids=U.shape_id)
def test_mutant_one_twiddle_entry_off_by_one(shape):
    """One (k, n): the bins 1, K / 2 and K at the last sample and at the tail sample."""
    W = shape[1]
    K = W // 2
    assert len(_SINGLE) + len(_BLIND) == len(_SPECTRUM)
    for n in sorted({W - 1, U.tail_sample(W)}):
        for k in sorted({1, max(K // 2, 1), K}):
            assert _mutant(shape, tw_off=(n, [k])) >= FACTOR, (n, k)


@pytest.mark.parametrize("shape", _SPECTRUM, ids=U.shape_id)
def test_mutant_every_bins_twiddle_index_off_by_one_at_last_sample(shape):
    W = shape[1]
    assert _mutant(shape, tw_off=(W - 1, None)) >= FACTOR


@pytest.mark.parametrize("shape", [s for s in _SPECTRUM if s[1] % 4], ids=U.shape_id)
def test_mutant_every_bins_twiddle_index_off_by_one_in_the_tail(shape):
    W = shape[1]
    n = U.tail_sample(W)
    assert n >= W - W % 4
    assert _mutant(shape, tw_off=(n, None)) >= FACTOR


@pytest.mark.parametrize("shape", [s for s in U.SHAPES if (s[1] // 2) % 16], ids=U.shape_id)
def test_mutant_columns_past_K_of_the_last_tile_kept(shape):
    assert _mutant(shape, keep_cols=True) >= FACTOR


@pytest.mark.parametrize("shape", _SPECTRUM, ids=U.shape_id)
def test_mutant_pivot_from_a_neighbouring_row(shape):
    """In exact arithmetic any pivot gives the same bins k >= 1, so this mutant is the fp32 model of the
    kernel's arithmetic with the next axis' first sample as the pivot: ``d`` is then dense and about 10, and
    the roundings of W products and W partial sums show.  (The same model with the right pivot passes:
    test_probe_stream_preconditions.)"""
    A, W, stride, nwin = shape[:4]
    an = U.analyse(shape)
    piv = np.roll(an.x[..., 0], -1, axis=1).reshape(-1)
    emu = U.features32(an.x.reshape(-1, W), pivot=piv).reshape(nwin, A, U.NFA)
    assert _worst_on(shape, U.to_rows(emu), an.sparse) >= FACTOR


def test_checker_rejects_poison_and_a_live_constant_row():
    shape = U.SHAPES[3]
    A, W = shape[:2]
    an, ref = U.analyse(shape), U.reference(shape)
    good = U.to_rows(ref)
    U.verdict(U.measure(good, ref, an, W, U.HZ))
    bad = good.copy()
    bad[4, 2 * A + 1] = float("nan")
    assert not U.measure(bad, ref, an, W, U.HZ)["finite"]
    bad = good.copy()
    bad[5, 10 * A] = float("inf")
    with pytest.raises(AssertionError):
        U.verdict(U.measure(bad, ref, an, W, U.HZ))
    w, a = U._samples(shape)[1]["const"]
    bad = good.copy()
    bad[w, 8 * A + a] = U.HZ / W
    assert U.measure(bad, ref, an, W, U.HZ)["flat"] == 1
    bad = good.copy()
    bad[0, 8 * A] *= 1 + 1e-4  # not a bin
    assert U.measure(bad, ref, an, W, U.HZ)["dominant"] == float("inf")
    assert math.isinf(U.worst(U.measure(bad, ref, an, W, U.HZ)))
