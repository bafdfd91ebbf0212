"""The HIP stream filter (``csrc/kernels/sosfilt.hip``) against the definition (``har.ops.sosfilt.sosfilt_torch``)
run on the CPU over the same bits.

Exact probes — integer inputs through sections whose arithmetic is exact in fp64 — are compared with
``torch.equal``; real-valued streams within ``2^-24 |y64| + tol`` of the definition before its rounding, where
``tol = 100 d`` and ``d`` is the largest difference, on that input, between two fp64 evaluation orders that are
both references (the sequential definition and ``_sosfilt_util.chunked_state_space``); every such test prints
``d``, ``tol`` and the largest error as a fraction of ``tol`` (PARITY.md "StreamFilter" records them)."""
import numpy as np
import pytest
import torch

from _sosfilt_util import (EXACT_PROBES, ORDER8_SOS, REAL_DESIGNS, chunked_state_space, flip_segments, int_stream, offsets, probe_sos,
                           real_stream)
from har.features.filter import StreamFilter
from har.ops import sosfilt as F

pytestmark = pytest.mark.gpu

L, G = 8, 4            # the override: 17 chunks -> 5 groups -> 2 groups, three scan levels at 135 samples
SIZES = (1, L - 1, L, L + 1, 3 * L + 5, L * G + 1, L * G * G + 7)


def _segmentations(S):
    edges = [c * L for c in range(1, S // L + 1)]
    return {
        "one": offsets([], S),
        "chunk_edges": offsets(edges, S),
        "edges_minus_1": offsets([e - 1 for e in edges], S),
        "edges_plus_1": offsets([e + 1 for e in edges], S),
        "inside_one_chunk": offsets([L + 1, L + 2, L + 5, 3 * L + 3, 3 * L + 4], S),
        "length_1": offsets(range(S), S),
    }


def _run(cuda, x, sos, off, init="zero", reverse=False, mode="filter", **kw):
    return F.sosfilt_native(x.to(cuda), sos, off, init, reverse, mode, **kw).cpu()


@pytest.mark.parametrize("A", [1, 3, 6, 9])
@pytest.mark.parametrize("name", sorted(EXACT_PROBES))
def test_exact_probes_three_scan_levels(cuda, name, A):
    sos = probe_sos(name)
    assert len(F.scan_levels(SIZES[-1], L, G)) == 3
    for S in SIZES:
        x = int_stream(S, A, 100 * A + S)
        for seg, off in _segmentations(S).items():
            for reverse in (False, True):
                want = F.sosfilt_torch(x, sos, off, "zero", reverse)
                got = _run(cuda, x, sos, off, "zero", reverse, chunk=L, group=G)
                assert got.dtype == torch.float32 and torch.equal(got, want), (S, seg, reverse)


@pytest.mark.parametrize("name", sorted(EXACT_PROBES))
def test_exact_probes_default_launch(cuda, name):
    """The default chunk length and scan group: around one chunk, a tail, and L G + 1 samples (two levels)."""
    Ld, Gd = F.chunk_len(), F.scan_group()
    sos = probe_sos(name)
    for S in (1, Ld - 1, Ld, Ld + 1, 3 * Ld + 5, Ld * Gd + 1):
        for A in (3, 9):
            x = int_stream(S, A, S + A)
            off = offsets([Ld, Ld + 1, 5 * Ld - 1, 800, 1500], S)                  # every segment <= 1,000 samples
            for reverse in (False, True):
                assert torch.equal(_run(cuda, x, sos, off, "zero", reverse), F.sosfilt_torch(x, sos, off, "zero", reverse))


def test_reverse_equals_flipping_each_segment(cuda):
    S = SIZES[-1]
    x = int_stream(S, 3, 11)
    off = offsets([1, 9, 40, 41, 100], S)
    for name in sorted(EXACT_PROBES):
        sos = probe_sos(name)
        fwd_of_flipped = _run(cuda, flip_segments(x, off), sos, off, chunk=L, group=G)
        assert torch.equal(_run(cuda, x, sos, off, reverse=True, chunk=L, group=G), flip_segments(fwd_of_flipped, off))


@pytest.mark.parametrize("A", [1, 3, 9])
def test_complement_modes_and_guard_rows(cuda, A):
    """[x - y | y] and x - y from the kernel's own y; the output inside a NaN-filled buffer whose guard rows stay
    NaN; stream and output at addresses that are no multiple of 16 bytes."""
    sos = F.butter_sos(3, 0.3, 20.0)
    for S in (1, 3 * L + 5, 1500):
        kw = dict(chunk=L, group=G) if S < 1000 else {}
        xb = torch.full((S + 2, A), float("nan"), device=cuda)
        x = real_stream(S, A, S)
        xb[1:S + 1] = x.to(cuda)
        xv = xb[1:S + 1]
        off = offsets([S // 3, S // 3 + 1], S)
        y = F.sosfilt_native(xv, sos, off, "step", **kw)
        for mode, OA in (("filter", A), ("split", 2 * A), ("body", A)):
            for reverse in (False, True):
                yr = F.sosfilt_native(xv, sos, off, "step", reverse, **kw)
                buf = torch.full((S + 3, OA), float("nan"), device=cuda)
                out = F.sosfilt_native(xv, sos, off, "step", reverse, mode, out=buf[1:S + 1], **kw)
                assert out.data_ptr() == buf[1:].data_ptr()
                want = {"filter": yr, "split": torch.cat([xv - yr, yr], 1), "body": xv - yr}[mode]
                assert torch.equal(buf[1:S + 1], want)
                assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[S + 1:]).all())
        assert torch.equal(y.cpu(), F.sosfilt_native(x.to(cuda), sos, off, "step", **kw).cpu())    # aligned == unaligned
        other = real_stream(S, A, S + 1).to(cuda)
        got = F.sosfilt_native(xv, sos, off, "step", False, "split", comp=other, **kw)
        assert torch.equal(got, torch.cat([other - y, y], 1))


# ------------------------------------------------------------------ real-valued streams
@pytest.fixture(scope="module")
def real_cases():
    """(x, offsets) of the two streams; the references are computed once per (stream, design) on first use."""
    return {
        "20000x3": (real_stream(20000, 3, 21), offsets([1, 6000, 6001, 6064, 13000], 20000)),
        "4099x9": (real_stream(4099, 9, 22), None),
    }


_REF = {}


def _reference(real_cases, case, design, reverse=False, x=None):
    key = (case, design, reverse, x is not None)
    if key not in _REF or x is not None:
        xs, off = real_cases[case]
        xs = xs if x is None else x
        btype, n, fc, hz = design
        sos = F.butter_sos(n, fc, hz, btype)
        y64 = F.sosfilt_torch(xs, sos, off, "step", reverse, out_dtype=torch.float64)
        d = float((torch.from_numpy(chunked_state_space(xs, sos, off, "step", reverse, 64)) - y64).abs().max())
        if x is not None:
            return sos, off, y64, d
        _REF[key] = (sos, off, y64, d)
    return _REF[key]


def _assert_close(y_dev, y64, d, what):
    tol = 100.0 * d
    assert tol <= 2.0 ** -27 * float(y64.abs().max()), "the bound must keep rejecting a state carried in fp32"
    err = (y_dev.double() - y64).abs()
    excess = err - 2.0 ** -24 * y64.abs()
    print(f"{what}: d = {d:.3g}, tol = {tol:.3g}, largest error beyond the fp32 half ulp = {float(excess.max()) / tol:.3g} tol")
    assert bool((excess <= tol).all())


@pytest.mark.parametrize("design", REAL_DESIGNS, ids=lambda d: f"{d[0]}{d[1]}_{d[2]}_{d[3]:g}")
@pytest.mark.parametrize("case", ["20000x3", "4099x9"])
def test_real_streams_within_the_derived_bound(cuda, real_cases, case, design):
    sos, off, y64, d = _reference(real_cases, case, design)
    x = real_cases[case][0]
    y = _run(cuda, x, sos, off, "step")
    _assert_close(y, y64, d, f"{case} {design}")
    assert torch.equal(y, _run(cuda, x, sos, off, "step"))                          # two runs, the same bits
    sp = _run(cuda, x, sos, off, "step", mode="split")
    assert torch.equal(sp[:, x.shape[1]:], y) and torch.equal(sp[:, :x.shape[1]], x - y)


@pytest.mark.parametrize("design", [REAL_DESIGNS[0], REAL_DESIGNS[3]], ids=["low3_0.3_20", "high4_0.3_100"])
def test_zero_phase_within_the_derived_bound(cuda, real_cases, design):
    case = "20000x3"
    x, off = real_cases[case]
    sos = F.butter_sos(design[1], design[2], design[3], design[0])
    fwd = F.sosfilt_native(x.to(cuda), sos, off, "step")
    got = F.sosfiltfilt(x.to(cuda), sos, off).cpu()
    assert torch.equal(got, F.sosfilt_native(fwd, sos, off, "step", True).cpu())
    # the reverse pass of the definition on the kernel's own fp32 forward result
    _, _, y64, d = _reference(real_cases, case, design, True, x=fwd.cpu())
    _assert_close(got, y64, d, f"zero-phase {design}")
    _, _, f64, df = _reference(real_cases, case, design)
    _assert_close(fwd.cpu(), f64, df, f"forward {design}")
    z = StreamFilter(design[3], "split", sos=sos, zero_phase=True).transform(x.to(cuda), off).cpu()
    assert torch.equal(z[:, 3:], got) and torch.equal(z[:, :3], x - got)


def test_determinism_and_no_host_read(cuda):
    x = real_stream(5000, 3, 31).to(cuda)
    off = offsets([700, 701, 3000], 5000)
    for f in (StreamFilter(20.0, "split"), StreamFilter(20.0, "body", zero_phase=True), StreamFilter(50.0, "lowpass")):
        first = f.transform(x, off)                      # loads the module, uploads the carry powers once
        one = f.transform(x)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")          # a synchronizing call (any device -> host read) raises
        try:
            again = f.transform(x, off)
            again_one = f.transform(x)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(first, again) and torch.equal(one, again_one)


def test_limits_raise_before_a_launch(cuda):
    sos = F.butter_sos(3, 0.3, 20.0)
    x = torch.zeros(16, 3, device=cuda)
    with pytest.raises(ValueError, match="axes"):
        F.sosfilt(torch.zeros(4, 10, device=cuda), sos)
    with pytest.raises(ValueError, match="sections"):
        F.sosfilt(x, torch.cat([sos, sos, sos]))
    with pytest.raises(ValueError, match="samples"):
        F.sosfilt(torch.zeros(1, 3, device=cuda).expand(F.MAX_SAMPLES, 3), sos)      # a stride-0 view: no memory
    bad = sos.clone()
    bad[1, 4] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        F.sosfilt(x, bad)
    with pytest.raises(ValueError, match="ill-conditioned"):
        F.sosfilt(x, torch.tensor(ORDER8_SOS, dtype=torch.float64))
    with pytest.raises(ValueError, match="fp32"):
        F.sosfilt(x.double(), sos)
    for kw in (dict(chunk=0), dict(chunk=F.MAX_CHUNK + 1), dict(group=1), dict(group=F.MAX_GROUP + 1)):
        with pytest.raises(ValueError, match="chunk length"):
            F.sosfilt_native(x, sos, **kw)
    with pytest.raises(ValueError, match="seg_offsets"):
        F.sosfilt(x, sos, torch.tensor([0, 4, 4, 16], dtype=torch.int64))
    with pytest.raises(ValueError, match="comp"):
        F.sosfilt_native(x, sos, comp=x)
    with pytest.raises(ValueError, match="out must"):
        F.sosfilt_native(x, sos, mode="split", out=torch.empty(16, 3, device=cuda))
    with pytest.raises(ValueError, match="step"):
        F.sosfilt(x, probe_sos("running_sum"), None, "step")                         # a pole at z = 1 has no step state
    assert tuple(F.sosfilt(x[:0], sos, mode="split").shape) == (0, 6)                # nothing to launch


def test_split_feeds_the_window_featurizer(cuda):
    """[body | gravity] of a 3-axis stream is a 6-axis stream of ``window.hip``; on an exact probe the filter's
    outputs are the definition's bits, so the feature rows must be too."""
    from har.features.window import WindowFeaturizer

    x = int_stream(10 * 40 + 7, 3, 41)
    off = offsets([130, 131, 300], x.shape[0])
    f = StreamFilter(20.0, "split", sos=probe_sos("fir_into_sum"), init="zero")   # the probe as the low-pass branch
    assert f.out_axes(3) == 6
    z_dev = f.transform(x.to(cuda), off)
    z_def = f.transform(x, off)
    assert torch.equal(z_dev.cpu(), z_def)
    wf = WindowFeaturizer(hz=20.0, seconds=2.0, axis_names=f.names())
    rows = wf.transform(z_dev)
    want = wf.transform(z_def.to(cuda))
    assert rows.shape[0] == 10 and rows.shape[1] == len(wf.names)
    assert torch.equal(rows.view(torch.int32), want.view(torch.int32))      # bit patterns: a window without peaks is NaN
