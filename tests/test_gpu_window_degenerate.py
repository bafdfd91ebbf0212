"""The window kernels (csrc/kernels/window.hip) on an axis whose bin scale ``10 / range`` is not a finite fp32.

``range = max - min`` of a (window, axis) below ``10 / FLT_MAX`` (2.94e-38: some normal and every denormal
range) makes ``fl(10 / range)`` +inf.  Unsaturated, ``(x - lo) * sc`` is then +inf for ``x > lo`` and NaN for
``x == lo``; the register kernels use it, unclamped, as a shift into the packed per-lane counts of the axis.  The
documented rule (features/window.py): the scale saturates at FLT_MAX, so the product stays below 10 and every
dispatch — fixed runs, runtime runs, the fallback kernel, fp32 and MLP rows — counts the same bins.

The streams are ``_window_util.degenerate_stream``: the exact stream with the second axis of every triad
replaced by ``v q``, q = 2^-123 (scale exactly 2^123: the float64 oracle's bins), 2^-128 (overflow; normal and
denormal samples) and 2^-130 (overflow; every sample denormal).  tests/test_window_exact.py checks the streams
and the fp32 emulation of the rule on the CPU.  Every row of the dispatch table runs at base offset 0, and the
first fixed-run, runtime-run and fallback rows also one sample into the buffer (scalar staging).

Not asserted (recorded as test properties): the non-bin columns of the tiny axis other than min and max — at
these magnitudes their fp32 squares underflow, the oracle comparison means nothing — and the resultant and
correlation columns, which involve that axis."""
import pytest
import torch

import _window_util as U
from har.features.window import n_features, window_features, window_features_mlp

pytestmark = pytest.mark.gpu


def _first(kind):
    return next(s for s in U.SHAPES if s[3] == kind)


CASES = [(s, 0) for s in U.SHAPES] + [(_first(k), 1) for k in ("fix", "reg", "fb")]
Q_IDS = ["2^-123", "2^-128", "2^-130"]


def _case_id(case):
    return "%s+%d" % (U.shape_id(case[0]), case[1])


def _stats(A, cuda):
    """Seeded random standardization statistics and the padded row width of the MLP rows."""
    F = n_features(A)
    g = torch.Generator().manual_seed(5 + A)
    mean = torch.randn(F, generator=g).to(cuda)
    inv_std = (torch.rand(F, generator=g) + 0.5).to(cuda)
    return F, mean, inv_std, (F + 31) // 32 * 32


@pytest.mark.parametrize("q", U.DEGENERATE_Q, ids=Q_IDS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_window_kernel_on_a_degenerate_axis(cuda, case, q, record_property):
    shape, r0 = case
    A, W, stride = shape[:3]
    nwin = U.n_windows(shape)
    es = U.degenerate_stream(shape, q, r0)
    view = es.view(es.buf.to(cuda))
    assert view.data_ptr() % 16 == (r0 * A * 4) % 16 and view.is_contiguous()
    ref = U.degenerate_reference(shape, q)
    want = U.degenerate_bins_fp32(es.view(), W, stride)            # [nwin, A, 10]
    tiny = list(range(1, A, 3))
    rest = [a for a in range(A) if a % 3 != 1]
    c = es.cols

    out_d = window_features(view, W, stride, U.HZ)
    out = out_d.cpu()
    assert out.shape == (nwin, n_features(A))
    # the tiny axes: integer counts, exactly the documented rule's
    bcols = U.axis_columns(A, "bins", tiny)
    cnt = out[:, bcols].double() * W
    wt = want[:, tiny].reshape(nwin, -1)
    err = (cnt - wt.double()).abs()
    assert float(err.max()) <= 1e-3, "tiny axis: max |out W - count| = %g; window 0 gives %s for %s" % (
        float(err.max()), cnt[0, :10].tolist(), wt[0, :10].tolist())
    assert torch.equal(cnt.round().long().view(nwin, len(tiny), 10).sum(-1), torch.full((nwin, len(tiny)), W))
    for name in ("min", "max"):
        cols = U.axis_columns(A, name, tiny)
        assert torch.equal(U.bits(out[:, cols]), U.bits(ref[:, cols])), name
    # the other axes: every column of their own, with the exact stream's bounds — nothing spills over
    U.check_exact(out, ref, A, W, axes=rest)
    # recorded, not asserted
    other = [i for n in ("avg", "peak", "absdev", "std", "energy") for i in U.axis_columns(A, n, tiny)]
    record_property("tiny_axis_other_columns_absmax", float(torch.nan_to_num(out[:, other]).abs().max()))
    for name in ("resultant", "corr"):
        d = torch.nan_to_num(out[:, c[name]].double() - ref[:, c[name]].double(), nan=float("inf")).abs().max()
        record_property(name + "_max_abs_diff", float(d))

    # MLP rows: the same counts under the standardization
    F, mean, inv_std, pad = _stats(A, cuda)
    mo = window_features_mlp(view, W, stride, U.HZ, mean, inv_std, pad)
    assert mo.shape == (nwin, pad) and mo.dtype == torch.bfloat16 and torch.count_nonzero(mo[:, F:]) == 0
    s = c["bins"]
    # (as tests/test_gpu_window_exact.py: on the exact columns both instantiations compute the same fp32
    # value, then (v - mean) * inv_std as two fp32 operations and one rounding to bf16)
    same = ((out_d[:, s] - mean[s]) * inv_std[s]).to(torch.bfloat16)
    assert torch.equal(U.bits(mo[:, s]), U.bits(same)), "MLP rows: bin columns differ from the fp32 rows'"
    # un-standardized against the emulation, with that test's tolerance (one bf16 ulp of the standardized
    # value, 2^-7, and 2^-22 max(|v|, 1) of the feature) carried through the affine map
    v = (want.double() / W).reshape(nwin, -1)
    got = mo[:, s].double().cpu() / inv_std[s].double().cpu() + mean[s].double().cpu()
    tol = 2.0 ** -7 * (v - mean[s].double().cpu()).abs() + 2.0 ** -22 * v.clamp_min(1.0)
    # (every axis: on the other axes the emulation's counts are the oracle's, tests/test_window_exact.py)
    assert bool(((got - v).abs() <= tol).all()), float(((got - v).abs() - tol).max())
