"""The spectral kernel (csrc/kernels/spectral.hip) on the probe stream of ``_spectral_util``: every outcome of
``make_plan``, streams that do not start on a 16-byte boundary, closed-form rows, and bounds derived from what
the fp32 path can do (``_spectral_util``'s docstring).  tests/test_spectral_exact.py proves on the CPU that the
table is the launcher's, that the stream has the properties the bounds rest on, and that the checker rejects
the mutants of the definition by a factor of at least 4.

Plans (``_spectral_util.SHAPES``; ``2 wpb + 1`` windows — two full blocks and a last block of one window — and
a stream that ends with its last sample):

    axes, W, stride    plan                               reaches for the first time
    3, 200, 100        64 KB, 4 waves, wpb 21             (r0 != 0: the scalar staging branch)
    6, 200, 100        64 KB, 4 waves, wpb 10             a last wave of 12 rows
    9, 200, 200        64 KB, 4 waves, wpb 7              closed-form rows
    3, 193, 97         64 KB, 4 waves, wpb 21             nspan % 4 == 3 in the one-window last block
    3, 500, 250        64 KB, 2 waves, wpb 10             the 2-wave plan
    3, 1024, 512       64 KB, 1 wave, wpb 5
    9, 1500, 100       160 KB, 4 waves, wpb 7             the 160 KB budget
    9, 1500, 1000      160 KB, 2 waves, wpb 3
    9, 2048, 2048      160 KB, 1 wave, wpb 1
    3, 2047, 2047      160 KB, 1 wave, wpb 5              odd W at the largest size, K = 1023
    3, 2048, 3000      fallback loop, wpb 4               the loop
    6, 2048, 5000      fallback loop, wpb 1
    3, 3, 1 / 3, 5, 2 / 6, 16, 3 / 9, 33, 11              W < 32 (k % W), K = 1, 2, 8, 16
    3, 200, 100 with 1, 11 and 22 windows                 wpb = n_windows: 1 wave; 3 waves (192 threads); 21 + 1

Base offsets r0 = 0..3 samples (3 axes: the stream's first float at byte 0, 12, 8, 4 of a 16-byte line) and
r0 = 0, 1 (6 axes: byte 8; 9 axes: byte 4).

Beside the table: the centre impulse alone for every W in 3..72, clipped square-ish windows at W = 1024..2048
whose quarter-rate bin keeps a power in the fp32 denormal range (the entropy's ``P ln P``), every window
launched alone, guarded output columns, the bf16 MLP rows bit for bit, determinism and the contract."""
import warnings

import numpy as np
import pytest
import torch

import _spectral_util as U
from har.features import spectral as smod
from har.features.spectral import (n_spectral_features, spectral_features, spectral_features_into,
                                   spectral_features_mlp, spectral_features_torch)

pytestmark = pytest.mark.gpu

CASES = [(s, r0) for s in U.SHAPES for r0 in U.offsets(s[0])]


def _case_id(case):
    return "%s+%d" % (U.shape_id(case[0]), case[1])


def _on_device(probe, cuda):
    """The probe stream inside its poisoned buffer on the device, at the intended 16-byte phase."""
    view = probe.view(probe.buf.to(cuda))
    assert view.data_ptr() % 16 == (probe.r0 * probe.shape[0] * 4) % 16 and view.is_contiguous()
    return view


def _kernel(view, W, stride):
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the kernel itself: no fallback on these shapes
        return spectral_features(view, W, stride, U.HZ)


def _stats(A, cuda):
    F = n_spectral_features(A)
    g = torch.Generator().manual_seed(11 + A)
    return F, torch.randn(F, generator=g).to(cuda), (torch.rand(F, generator=g) + 0.5).to(cuda)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_spectral_kernel_probe_against_oracle(cuda, case):
    """Every table row at every base offset against the float64 oracle with the derived bounds: band
    fractions, centroid / hz and entropy per row, the dominant frequency an exact bin within twice the row's
    relative power bound of the maximum (bin 1 outright for the centre impulse), constant rows exactly 0,
    everything finite and nothing of the NaN poison around the stream."""
    shape, r0 = case
    A, W, stride, nwin = shape[:4]
    view = _on_device(U.probe_stream(shape, r0), cuda)
    out = _kernel(view, W, stride).cpu()
    U.check(out, shape, "+%d" % r0)


@pytest.mark.parametrize("W", range(3, 73))
def test_centre_impulse_alone(cuda, W):
    """One window with an impulse on sample W // 2 of every axis, for every W in 3..72: the device's band
    mapping (fractions bincount / K), the ``W < 32`` index path at every W % 4 and both parities, K < 8.
    Even W: an exact K-way tie, bin 1 outright."""
    probe = U.impulse_stream(W, W % 4)
    view = _on_device(probe, cuda)
    out = _kernel(view, W, W).cpu()
    an = U.analyse_windows(U.windows_of(probe.view().numpy(), W, W, 1))
    imp = tuple((0, a) for a in range(3)) if W % 2 == 0 else ()
    want = np.tile(U.impulse_expected(W), (1, 3, 1))
    res = U.measure(out.numpy(), want, an, W, U.HZ, imp)
    U.report(res, "impulse W=%d (closed form)" % W)
    U.verdict(res)
    ref = U.per_axis(spectral_features_torch(probe.view(), W, W, U.HZ).numpy(), 3)
    U.verdict(U.measure(out.numpy(), ref, an, W, U.HZ, imp))


@pytest.mark.parametrize("W", U.STRUCTURED_W)
def test_structured_windows_are_finite(cuda, W):
    """Clipped, square-ish windows near the largest W: bins that cancel down to one table entry of ~1e-16
    carry a prescaled power in the fp32 denormal range (tests/test_spectral_exact.py).  ``0 ln 0 = 0`` and
    ``|P ln P| < 2^-119`` for such a power: the entropy stays finite and inside its bound."""
    probe = U.structured_stream(W, 1)
    view = _on_device(probe, cuda)
    out = _kernel(view, W, W).cpu()
    an = U.analyse_windows(U.windows_of(probe.view().numpy(), W, W, 1))
    ref = U.per_axis(spectral_features_torch(probe.view(), W, W, U.HZ).numpy(), 3)
    res = U.measure(out.numpy(), ref, an, W, U.HZ)
    U.report(res, "structured W=%d" % W)
    print("  entropy", out[0, 30:].tolist())
    U.verdict(res)


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_id)
def test_window_rows_do_not_depend_on_the_launch(cuda, shape):
    """Every window computed alone — ``spectral_features`` on the slice ``[w stride, w stride + W)``: one
    window, wpb = 1, its own alignment — is bit-equal to its row in the batched call."""
    A, W, stride, nwin = shape[:4]
    assert U.plan(A, W, stride, 1)[1] == 1
    view = _on_device(U.probe_stream(shape, 0), cuda)
    rows = _kernel(view, W, stride)
    alone = torch.cat([_kernel(view[w * stride: w * stride + W], W, stride) for w in range(nwin)])
    assert alone.shape == rows.shape
    diff = U.bits(alone) != U.bits(rows)
    assert not bool(diff.any()), "windows %s differ" % sorted(set(diff.nonzero()[:, 0].tolist()))


# a 4-wave shared-span plan (unaligned too), closed-form rows, the 160 KB budget at one wave, the loop
_GUARDED = [(U.SHAPES[0], 0), (U.SHAPES[3], 1), (U.SHAPES[2], 1), (U.SHAPES[8], 0), (U.SHAPES[11], 1)]


@pytest.mark.parametrize("case", _GUARDED, ids=_case_id)
def test_kernel_writes_only_its_columns(cuda, case):
    """``ld_out > col0 + 11 A`` and ``col0 > 0`` in a poisoned buffer with guard rows before and after: only
    the 11 A columns of the ``n_windows`` rows change, for the fp32 rows and for the bf16 MLP rows."""
    shape, r0 = case
    A, W, stride, nwin = shape[:4]
    view = _on_device(U.probe_stream(shape, r0), cuda)
    F, mean, inv_std = _stats(A, cuda)
    col0, ld = 5, F + 5 + 7
    plain = _kernel(view, W, stride)
    big = torch.full((nwin + 4, ld), -7.0, device=cuda)
    spectral_features_into(view, W, stride, U.HZ, big[2: 2 + nwin], col0)
    assert torch.equal(U.bits(big[2: 2 + nwin, col0: col0 + F]), U.bits(plain))
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[2: 2 + nwin, col0: col0 + F] = False
    assert bool((big[mask] == -7.0).all())
    bigb = torch.full((nwin + 4, ld), 0x7FC1, dtype=torch.int16, device=cuda)
    ob = bigb.view(torch.bfloat16)[2: 2 + nwin]
    assert spectral_features_mlp(view, W, stride, U.HZ, mean, inv_std, ob, col0) is ob
    assert bool((bigb[mask] == 0x7FC1).all())
    got = bigb[2: 2 + nwin, col0: col0 + F]
    assert not bool((got == 0x7FC1).all(0).any())  # every column was written
    tight = torch.empty(nwin, F, dtype=torch.bfloat16, device=cuda)
    spectral_features_mlp(view, W, stride, U.HZ, mean, inv_std, tight, 0)
    assert torch.equal(got, U.bits(tight))


_MLP = [(U.SHAPES[0], 0), (U.SHAPES[0], 1), (U.SHAPES[2], 1), (U.SHAPES[5], 0), (U.SHAPES[7], 1), (U.SHAPES[9], 3),
        (U.SHAPES[10], 0), (U.SHAPES[15], 1)]


@pytest.mark.parametrize("case", _MLP, ids=_case_id)
def test_mlp_rows_are_the_fp32_rows_standardized(cuda, case):
    """The two instantiations share all arithmetic up to the last line, so the bf16 rows are bit-equal to
    ``((fp32 rows - mean) * inv_std).to(bfloat16)`` computed by torch from the fp32 kernel's own output: two
    fp32 operations and one round-to-nearest-even."""
    shape, r0 = case
    A, W, stride, nwin = shape[:4]
    view = _on_device(U.probe_stream(shape, r0), cuda)
    F, mean, inv_std = _stats(A, cuda)
    v = _kernel(view, W, stride)
    rows = torch.empty(nwin, F, dtype=torch.bfloat16, device=cuda)
    spectral_features_mlp(view, W, stride, U.HZ, mean, inv_std, rows, 0)
    want = ((v - mean) * inv_std).to(torch.bfloat16)
    ne = U.bits(rows) != U.bits(want)
    print("%s: %d of %d bf16 elements differ" % (_case_id(case), int(ne.sum()), ne.numel()))
    assert not bool(ne.any())


@pytest.mark.parametrize("shape", [U.SHAPES[6], U.SHAPES[10]], ids=U.shape_id)
def test_two_calls_same_bits(cuda, shape):
    A, W, stride, nwin = shape[:4]
    assert shape[4] in ("160K", "loop")
    view = _on_device(U.probe_stream(shape, 1), cuda)
    assert torch.equal(U.bits(_kernel(view, W, stride)), U.bits(_kernel(view, W, stride)))


def test_contract_raises_before_any_launch(cuda):
    """Axes 4, window 2, stride 0 and a stream shorter than its windows: an error and an untouched output,
    from the Python front end and from the native entry point."""
    from har.ops import _native

    k = _native.kernels()
    for axes, W, stride in ((4, 200, 100), (3, 2, 1), (3, 200, 0)):
        s = torch.ones(400, axes, device=cuda)
        with pytest.raises(ValueError):
            spectral_features(s, W, stride, U.HZ)
        out = torch.full((3, 64), -7.0, device=cuda)
        with pytest.raises(RuntimeError, match="contract violation code -2"):
            k.spectral_features(s.data_ptr(), 400, axes, W, stride, 3, U.HZ, out.data_ptr(), 64, 0, _native.stream_ptr())
        assert bool((out == -7.0).all())
    s = torch.ones(399, 3, device=cuda)  # three windows of 200 at stride 100 need 400 samples
    out = torch.full((3, 64), -7.0, device=cuda)
    with pytest.raises(RuntimeError, match="contract violation code -3"):
        k.spectral_features(s.data_ptr(), 399, 3, 200, 100, 3, U.HZ, out.data_ptr(), 64, 0, _native.stream_ptr())
    ob = torch.full((3, 64), 0x7FC1, dtype=torch.int16, device=cuda)
    m = torch.zeros(33, device=cuda)
    with pytest.raises(RuntimeError, match="contract violation code -3"):
        k.spectral_features_mlp(s.data_ptr(), 399, 3, 200, 100, 3, U.HZ, m.data_ptr(), m.data_ptr(), ob.data_ptr(), 64, 0,
                                _native.stream_ptr())
    with pytest.raises(RuntimeError, match="contract violation code -4"):  # a row narrower than col0 + 11 A
        k.spectral_features(s.data_ptr(), 399, 3, 200, 100, 2, U.HZ, out.data_ptr(), 64, 32, _native.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ob == 0x7FC1).all())
    assert spectral_features(s, 200, 100, U.HZ).shape == (2, 33)       # the front end takes the whole windows
    assert spectral_features(s[:150], 200, 100, U.HZ).shape == (0, 33)  # ... and none


def test_window_2049_takes_the_torch_definition_with_one_warning(cuda, monkeypatch):
    monkeypatch.setattr(smod, "_LONG_WARNED", set())
    W = smod.SPECTRAL_MAX_WINDOW + 1
    g = torch.Generator().manual_seed(7)
    s = torch.randn(W + 100, 3, generator=g).to(cuda)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a = spectral_features(s, W, 100, U.HZ)
        b = spectral_features(s, W, 100, U.HZ)
    assert len([r for r in rec if "exceed the kernel's maximum" in str(r.message)]) == 1
    assert a.shape == (2, 33) and torch.equal(a, b) and torch.equal(a, spectral_features_torch(s, W, 100, U.HZ))
