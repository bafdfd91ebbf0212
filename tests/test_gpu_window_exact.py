"""The window kernels (csrc/kernels/window.hip) on the exact-arithmetic stream of ``_window_util``: exact bin
counts, exact peak sets, bit-equal extrema, every dispatch of the launcher, and streams that do not start on a
16-byte boundary.  tests/test_window_exact.py proves on the CPU that the stream allows these demands.

Dispatch (``_window_util.SHAPES``, re-derived from ``launch_axes``; ``nwin = 2 wpb + 1`` windows — two full
blocks and a last block of one window — and a stream that ends with its last window):

    axes, W, stride    kernel                                    wpb   reaches for the first time
    3, 200, 100        8 x 25 fixed runs, D = 0                   32   (r0 != 0: scalar staging)
    3, 193, 97         8 x 25 fixed, D = 7                        32
    6, 200, 100        8 x 25 fixed, two triads                   16
    3, 97, 40          8 x 13, 17-register instantiation, D = 7   32
    3, 240, 80         8 x 31, 31-register instantiation, D = 8   32
    3, 248, 124        8 x 31, D = 0                              24   8 x 31 with D = 0; a 3-wave block
    3, 200, 200        16 x 13 fixed, D = 8, padded (pitch 624)   16   r0 != 0: contiguous images
    9, 200, 200        16 x 13 fixed, padded (pitch 1808)          4   r0 = 1: contiguous images
    3, 208, 208        16 x 13 fixed, D = 0, never padded         16   16 x 13 with D = 0 (the LPW * RCMAX == W
                                                                       branch); stride == W, W A % 4 == 0,
                                                                       contiguous images on an aligned stream
    3, 195, 195        16 x 13 fixed, D = 13, never padded        16
    3, 48, 48          16 x 5, D = 32, never padded               16   as 208 for the 17-register instantiation
    3, 64, 64          16 x 5, D = 16, padded (pitch 208)         16
    9, 500, 500        32 x 17, D = 44                             2
    3, 700, 350        32 x 23, D = 36                             8
    6, 1100, 1100      64 x 19, D = 116                            1
    3, 1984, 1984      64 x 31, D = 0                              2
    3, 1985, 1000      fallback, n_samples A % 4 == 3              4   the float4 staging's tail of 3 floats;
                                                                       r0 != 0: its scalar branch at 3 axes
    3, 1986, 1000      fallback, n_samples A % 4 == 2              4   ... of 2 floats
    3, 3, 1 / 3, 5, 2 / 6, 16, 3 / 9, 33, 11   8 x 5, D = 37 / 35 / 24 / 7   32 / 32 / 16 / 8

Base offsets r0 = 0..3 samples (3 axes: the stream's first float at byte 0, 12, 8, 4 of a 16-byte line) and
r0 = 0, 1 (6 axes: byte 8; 9 axes: byte 4).  Every r0 != 0 of a register-kernel row runs that kernel's scalar
staging loop (``done = 0``), which no earlier test reached: in all of them every block's source is 16-byte
aligned."""
import warnings

import pytest
import torch

import _window_util as U
from har.features.window import (WindowFeaturizer, _window_features_into, n_features, window_count, window_features,
                                 window_features_mlp)

pytestmark = pytest.mark.gpu

CASES = [(s, r0) for s in U.SHAPES for r0 in U.offsets(s[0])]
UNALIGNED = [c for c in CASES if c[1]]


def _case_id(case):
    return "%s+%d" % (U.shape_id(case[0]), case[1])


def _on_device(shape, r0, cuda, S=None):
    """The exact stream ``r0`` samples into its poisoned buffer on the device: (ExactStream, device view)."""
    es = U.int_stream(shape, r0, S=S)
    view = es.view(es.buf.to(cuda))
    assert view.data_ptr() % 16 == (r0 * shape[0] * 4) % 16 and view.is_contiguous()
    return es, view


def _stats(A, cuda):
    """Seeded random standardization statistics and the padded row width of the MLP rows."""
    F = n_features(A)
    g = torch.Generator().manual_seed(5 + A)
    mean = torch.randn(F, generator=g).to(cuda)
    inv_std = (torch.rand(F, generator=g) + 0.5).to(cuda)
    return F, mean, inv_std, (F + 31) // 32 * 32


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_window_kernel_exact_against_oracle(cuda, case):
    """Every table row at every base offset against the float64 oracle, with the bounds of
    ``_window_util.check_exact``: integer bin counts with no sample moved, bit-equal min / max, avg / energy
    to 2.5e-7, the same peak sets (NaN pattern, then rtol 1e-6: ``last - first`` and ``npk`` exact), and no
    NaN from the poison around the stream."""
    shape, r0 = case
    A, W, stride = shape[:3]
    es, view = _on_device(shape, r0, cuda)
    assert window_count(es.S, W, stride) == U.n_windows(shape)
    out = window_features(view, W, stride, U.HZ).cpu()
    U.check_exact(out, U.reference(shape), A, W)


@pytest.mark.parametrize("case", UNALIGNED, ids=_case_id)
def test_window_view_and_copy_same_bits(cuda, case):
    """Staging only moves data: an unaligned view of the stream and its (aligned) copy run the same template
    instantiation — scalar against 16-byte staging, contiguous against padded images (the run-time ``ipw``)
    — and must give the same bits, for the fp32 rows, the MLP rows and the ``[time | spectral]`` rows (the
    spectral kernel's own staging has the same two branches)."""
    shape, r0 = case
    A, W, stride = shape[:3]
    es, view = _on_device(shape, r0, cuda)
    copy = view.clone()
    assert copy.data_ptr() % 16 == 0
    assert torch.equal(U.bits(window_features(view, W, stride, U.HZ)), U.bits(window_features(copy, W, stride, U.HZ)))
    F, mean, inv_std, pad = _stats(A, cuda)
    a = window_features_mlp(view, W, stride, U.HZ, mean, inv_std, pad)
    b = window_features_mlp(copy, W, stride, U.HZ, mean, inv_std, pad)
    assert a.shape == (U.n_windows(shape), pad) and torch.equal(U.bits(a), U.bits(b))
    fz = WindowFeaturizer(hz=U.HZ, spectral=True)
    fz.window, fz.stride = W, stride
    sa, sb = fz.transform(view), fz.transform(copy)
    assert sa.shape == (U.n_windows(shape), 28 * A + 4 * (A // 3))
    assert not bool(torch.isnan(sa[:, F:]).any()), "spectral columns: a read outside the stream"
    assert torch.equal(U.bits(sa), U.bits(sb))


@pytest.mark.parametrize("case", [c for c in CASES if c[1] < 2], ids=_case_id)
def test_window_mlp_rows_exact(cuda, case):
    """MLP rows against the fp32 rows ``v`` of the same stream.  On the exact columns (bins, min, max, avg,
    energy) both instantiations compute the same fp32 ``v`` — exact sums, the same two roundings — and then
    ``(v - mean) * inv_std`` as two fp32 operations and one round-to-nearest-even: bit-equal.  On the other
    columns the two instantiations may contract or order their fp32 sums differently: a few fp32 ulps of the
    feature (4 * 2^-24 max(|v|, 1), through the affine map) and then one bf16 ulp (rtol 2^-7).  Pad columns
    zero."""
    shape, r0 = case
    A, W, stride = shape[:3]
    es, view = _on_device(shape, r0, cuda)
    F, mean, inv_std, pad = _stats(A, cuda)
    v = window_features(view, W, stride, U.HZ)
    mo = window_features_mlp(view, W, stride, U.HZ, mean, inv_std, pad)
    assert mo.shape == (U.n_windows(shape), pad) and mo.dtype == torch.bfloat16
    assert torch.count_nonzero(mo[:, F:]) == 0
    vf = torch.nan_to_num(v, nan=-1.0)
    want = ((vf - mean) * inv_std).to(torch.bfloat16)
    for name in U.EXACT_COLS:
        s = es.cols[name]
        assert torch.equal(U.bits(mo[:, s]), U.bits(want[:, s])), name
    for name in ("peak",) + U.LOOSE_COLS:
        s = es.cols[name]
        got, ref = mo[:, s].float(), want[:, s].float()
        tol = 2.0 ** -7 * ref.abs() + 2.0 ** -22 * vf[:, s].abs().clamp_min(1.0) * inv_std[s]
        assert bool(((got - ref).abs() <= tol).all()), (name, float(((got - ref).abs() - tol).max()))


# one fixed-run shared-span shape, one padded-image shape, one 64-lane shape, the fallback kernel
_GUARDED = [U.SHAPES[0], U.SHAPES[6], U.SHAPES[15], U.SHAPES[16]]


@pytest.mark.parametrize("shape", _GUARDED, ids=U.shape_id)
def test_window_kernels_write_only_their_rows_and_columns(cuda, shape):
    """Output wider and longer than the kernel's rows, prefilled with a sentinel (-7 in fp32 rows, the bf16
    NaN pattern 0x7FC1 in MLP rows): the kernel's columns of the first ``nwin`` rows equal the plain call's,
    every other element keeps the sentinel."""
    A, W, stride = shape[:3]
    nwin = U.n_windows(shape)
    es, view = _on_device(shape, 0, cuda)
    F, mean, inv_std, pad = _stats(A, cuda)
    out = torch.full((nwin + 3, F + 5), -7.0, device=cuda)
    _window_features_into(view, W, stride, U.HZ, out)
    assert torch.equal(U.bits(out[:nwin, :F]), U.bits(window_features(view, W, stride, U.HZ)))
    assert bool((out[:, F:] == -7.0).all()) and bool((out[nwin:] == -7.0).all())
    sentinel = torch.full((nwin + 3, pad + 16), 0x7FC1, dtype=torch.int16, device=cuda)
    for width in (pad, pad + 16):  # rows `pad` apart (the kernel writes in place), then a wider buffer
        ob = sentinel[:, :width].contiguous().view(torch.bfloat16)
        res = window_features_mlp(view, W, stride, U.HZ, mean, inv_std, pad, out=ob)
        assert res is ob
        assert torch.equal(U.bits(ob[:nwin, :pad]), U.bits(window_features_mlp(view, W, stride, U.HZ, mean, inv_std, pad)))
        raw = ob.view(torch.int16)
        assert bool((raw[nwin:] == 0x7FC1).all()) and bool((raw[:, pad:] == 0x7FC1).all())


def test_window_wide_fallback_writes_only_its_rows(cuda):
    """Windows whose images exceed the LDS (9 axes x 2,600 samples: contract code -5) take the torch
    definition on the device; with guarded output it too fills only its rows and columns."""
    A, W, stride, nwin = 9, 2600, 1300, 3
    g = torch.Generator().manual_seed(1)
    s = torch.randint(0, 11, ((nwin - 1) * stride + W, A), generator=g).float().to(cuda)
    F, mean, inv_std, pad = _stats(A, cuda)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = window_features(s, W, stride, U.HZ)
        out = torch.full((nwin + 2, F + 3), -7.0, device=cuda)
        _window_features_into(s, W, stride, U.HZ, out)
        ob = torch.full((nwin + 2, pad + 16), 0x7FC1, dtype=torch.int16, device=cuda).view(torch.bfloat16)
        window_features_mlp(s, W, stride, U.HZ, mean, inv_std, pad, out=ob)
        plain = window_features_mlp(s, W, stride, U.HZ, mean, inv_std, pad)
    assert ref.shape == (nwin, F)
    assert torch.equal(U.bits(out[:nwin, :F]), U.bits(ref))
    assert bool((out[:, F:] == -7.0).all()) and bool((out[nwin:] == -7.0).all())
    raw = ob.view(torch.int16)
    assert torch.equal(raw[:nwin, :pad], plain.view(torch.int16))
    assert bool((raw[nwin:] == 0x7FC1).all()) and bool((raw[:, pad:] == 0x7FC1).all())


def test_sharded_features_at_an_offset_off_the_stride(cuda):
    """A shard whose global offset (37) is no multiple of the stride: the first owned window starts at global
    sample 100, local sample 63 — a pointer 756 bytes into the shard, 4-byte aligned only.  The rows, fp32 and
    through the stream pass's MLP-input closure, are bit-equal to featurizing a copy of ``local[63:]``, and
    match the float64 oracle exactly."""
    from har.features.window import window_features_torch
    from har.parallel.dist import DistContext
    from har.parallel.stream import sharded_window_features

    fz = WindowFeaturizer(hz=20.0, seconds=10.0, overlap=0.5)
    assert (fz.window, fz.stride) == (200, 100)
    shape = U.SHAPES[0]
    L = U.shard_len(shape)  # (17 samples after the last whole window: dropped)
    assert U.SHARD_SKIP == 63
    es, local = _on_device(shape, 0, cuda, S=L)
    ctx = DistContext(rank=0, local_rank=0, world_size=1, device=cuda, backend=None)
    rows, first = sharded_window_features(ctx, local, fz, offset=37, total=37 + L)
    seg = local[63:].clone()
    assert first == 1 and rows.shape == (U.n_windows(shape), n_features(3))
    assert torch.equal(U.bits(rows), U.bits(fz.transform(seg)))
    U.check_exact(rows.cpu(), window_features_torch(es.view()[63:], 200, 100, 20.0), 3, 200)
    F, mean, inv_std, pad = _stats(3, cuda)

    def inputs(s):  # bench.py's stream-pass closure
        return window_features_mlp(s, fz.window, fz.stride, fz.hz, mean, inv_std, pad, -1.0)

    mrows, mfirst = sharded_window_features(ctx, local, fz, offset=37, total=37 + L, transform=inputs)
    assert mfirst == 1 and mrows.shape == (U.n_windows(shape), pad)
    assert torch.equal(U.bits(mrows), U.bits(inputs(seg)))
