"""The spectral HIP kernel (csrc/kernels/spectral.hip) against the float64 definition
(``spectral_features_torch``, computed on the device): fp32 rows, bf16 MLP rows, the combined featurizer."""
import functools
import warnings

import pytest
import torch

from har.data.synth import StreamSpec, generate_stream
from har.features.spectral import (SPECTRAL_MAX_WINDOW, n_spectral_features, spectral_features,
                                   spectral_features_torch, spectral_power_torch)
from har.features.window import (WindowFeaturizer, n_features, window_count, window_features, window_features_mlp,
                                 window_spectral_features_mlp)

TOL = 2e-4  # the tolerance tests/test_window.py uses for the window kernel against its float64 oracle


def _hz(axes):
    return 50.0 if axes == 9 else 20.0


@functools.lru_cache(maxsize=None)
def _case(axes, window, stride):
    """(stream on the device, oracle rows, oracle float64 spectrum), computed once per shape"""
    n_seg = 8 if window >= SPECTRAL_MAX_WINDOW else 64
    s, _ = generate_stream(n_seg, StreamSpec(axes=axes, window=max(window, 16), seed=axes + window))
    s = s[: s.shape[0] - 13].to("cuda:0")
    return s, spectral_features_torch(s, window, stride, _hz(axes)), spectral_power_torch(s, window, stride)


def _check(out, s, ref, P, window, stride, hz):
    """Band fractions, entropy and centroid / hz within TOL of the definition; constant axis-windows exactly 0;
    the dominant frequency an exact bin k hz / W, 1 <= k <= K, whose float64 power is within 1e-4 of the
    largest (no allowance for mismatches)."""
    A, W, K = s.shape[1], window, window // 2
    assert out.shape == ref.shape == (window_count(s.shape[0], W, stride), n_spectral_features(A))
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    nb = 8 * A
    print(f"W={W} A={A} stride={stride}: max |d fraction| {float((out[:, :nb] - ref[:, :nb]).abs().max()):.3g}, "
          f"|d centroid / hz| {float((out[:, 9 * A:10 * A] - ref[:, 9 * A:10 * A]).abs().max()) / hz:.3g}, "
          f"|d entropy| {float((out[:, 10 * A:] - ref[:, 10 * A:]).abs().max()):.3g}")
    torch.testing.assert_close(out[:, :nb], ref[:, :nb], rtol=TOL, atol=TOL)
    torch.testing.assert_close(out[:, 10 * A:], ref[:, 10 * A:], rtol=TOL, atol=TOL)
    torch.testing.assert_close(out[:, 9 * A:10 * A] / hz, ref[:, 9 * A:10 * A] / hz, rtol=TOL, atol=TOL)
    x = s.unfold(0, W, stride)[: out.shape[0]]                      # [nw, A, W]
    live = (x.max(-1).values > x.min(-1).values) & (P.sum(-1) > 0)  # [nw, A]
    cols = out.reshape(out.shape[0], -1)
    per_axis = torch.cat([cols[:, :nb].reshape(-1, A, 8), cols[:, nb:].reshape(-1, 3, A).transpose(1, 2)], 2)
    assert int(torch.count_nonzero(per_axis[~live])) == 0  # all 11 columns of a constant axis-window
    dom = out[:, 8 * A:9 * A].double()
    kf = dom * W / hz
    k = kf.round()
    # two fp32 roundings (k * hz, / W) of 2^-24 each: the reported frequency is within 1e-6 k of bin k
    assert bool(((kf - k).abs() <= 1e-6 * k)[live].all())
    assert bool(((k >= 1) & (k <= K))[live].all())
    pk = P.gather(2, (k.long().clamp(1, K) - 1)[..., None])[..., 0]
    pmax = P.max(-1).values
    print(f"  dominant bin: {int(((k.long() - 1) != P.argmax(-1))[live].sum())} of {int(live.sum())} differ from the "
          f"oracle's argmax; min P[k] / max P {float((pk / pmax)[live].min()) if bool(live.any()) else 1.0:.8f}")
    assert bool((pk >= (1 - 1e-4) * pmax)[live].all())


SHAPES = [(3, 200, 200), (3, 200, 100), (9, 500, 250), (6, 97, 31), (3, 193, 97), (3, 17, 17), (3, 8, 8), (3, 5, 2),
          (3, 3, 1), (3, 1024, 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("axes,window,stride", SHAPES)
def test_spectral_kernel_matches_definition(cuda, axes, window, stride):
    s, ref, P = _case(axes, window, stride)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no fallback on these shapes
        out = spectral_features(s, window, stride, _hz(axes))
    _check(out, s, ref, P, window, stride, _hz(axes))


@pytest.mark.gpu
def test_spectral_kernel_largest_window(cuda):
    """The largest window the kernel itself takes: no fallback warning."""
    from har.ops import _native

    W = SPECTRAL_MAX_WINDOW
    assert W >= 2048 and _native.kernels().spectral_max_window() == W
    s, ref, P = _case(3, W, W)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = spectral_features(s, W, W, 20.0)
    assert not [r for r in rec if "spectral_features" in str(r.message)]
    _check(out, s, ref, P, W, W, 20.0)


@pytest.mark.gpu
def test_spectral_long_window_falls_back_with_warning(cuda, monkeypatch):
    from har.features import spectral as smod

    monkeypatch.setattr(smod, "_LONG_WARNED", set())
    s, ref, P = _case(9, 2600, 1300)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = spectral_features(s, 2600, 1300, 50.0)
        spectral_features(s, 2600, 1300, 50.0)
    assert len([r for r in rec if "exceed the kernel's maximum" in str(r.message)]) == 1  # once per shape
    _check(out, s, ref, P, 2600, 1300, 50.0)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [200, 100])
def test_spectral_kernel_clipped_and_constant_windows(cuda, stride):
    """The stream of test_window_kernel_saturated_and_constant_runs: runs at the clip value and constant
    windows.  Constant axis-windows are exactly 0 in all 11 columns (checked in _check), the rest match."""
    W = 200
    s, _ = generate_stream(40, StreamSpec(axes=3, window=W, seed=21), cuda)
    s = s.clone()
    hi = float(s.max()) * 0.25
    s = s.clamp(max=hi)
    s[5 * W:7 * W] = 1.5
    s[11 * W:11 * W + 60, 1] = 9.0
    nwin = (s.shape[0] - W) // stride + 1
    s = s[: (nwin - 1) * stride + W].contiguous()
    x = s.unfold(0, W, stride)
    assert int((x.max(-1).values == x.min(-1).values).sum()) >= 3  # there are constant axis-windows
    out = spectral_features(s, W, stride, 20.0)
    _check(out, s, spectral_features_torch(s, W, stride, 20.0), spectral_power_torch(s, W, stride), W, stride, 20.0)


@pytest.mark.gpu
def test_spectral_kernel_grid_tails(cuda):
    """4,099 windows of 200 x 3 at stride 100: several workgroups per CU slot and a ragged last tile."""
    W, stride, nwin = 200, 100, 4099
    n = (nwin - 1) * stride + W
    s, _ = generate_stream((n + W - 1) // W, StreamSpec(axes=3, window=W, seed=5), cuda)
    s = s[:n].contiguous()
    assert window_count(s.shape[0], W, stride) == nwin
    out = spectral_features(s, W, stride, 20.0)
    _check(out, s, spectral_features_torch(s, W, stride, 20.0), spectral_power_torch(s, W, stride), W, stride, 20.0)


@pytest.mark.gpu
@pytest.mark.parametrize("axes,window,stride", [(3, 200, 100), (9, 500, 500)])
def test_combined_mlp_rows(cuda, axes, window, stride):
    hz = _hz(axes)
    s, _ = generate_stream(48, StreamSpec(axes=axes, window=window, seed=axes + 7), cuda)
    F, Fs = n_features(axes), n_spectral_features(axes)
    pad = (F + Fs + 31) // 32 * 32
    g = torch.Generator(device=cuda).manual_seed(3)
    mean = torch.randn(F + Fs, device=cuda, generator=g)
    inv_std = torch.rand(F + Fs, device=cuda, generator=g) + 0.5
    rows = window_spectral_features_mlp(s, window, stride, hz, mean, inv_std, pad)
    nw = window_count(s.shape[0], window, stride)
    assert rows.shape == (nw, pad) and rows.dtype == torch.bfloat16
    assert torch.count_nonzero(rows[:, F + Fs:]) == 0
    feats = torch.cat([window_features(s, window, stride, hz), spectral_features(s, window, stride, hz)], 1)
    want = ((torch.nan_to_num(feats, nan=-1.0) - mean) * inv_std).to(torch.bfloat16)
    torch.testing.assert_close(rows[:, :F + Fs].float(), want.float(), rtol=2 ** -7, atol=1e-6)
    alone = window_features_mlp(s, window, stride, hz, mean[:F], inv_std[:F], pad)
    assert torch.equal(rows[:, :F].view(torch.int16), alone[:, :F].view(torch.int16))


@pytest.mark.gpu
def test_featurizer_transform_is_both_kernels_in_one_buffer(cuda):
    s, _, _ = _case(3, 200, 100)
    fz = WindowFeaturizer(hz=20.0, seconds=10.0, overlap=0.5, spectral=True)
    rows = fz.transform(s)
    assert rows.shape[1] == len(fz.names) == 88 and rows.is_contiguous()
    want = torch.cat([window_features(s, 200, 100, 20.0), spectral_features(s, 200, 100, 20.0)], 1)
    assert torch.equal(rows.view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
def test_spectral_kernel_is_deterministic(cuda):
    s, _, _ = _case(3, 200, 100)
    a = spectral_features(s, 200, 100, 20.0)
    b = spectral_features(s, 200, 100, 20.0)
    assert torch.equal(a, b)
