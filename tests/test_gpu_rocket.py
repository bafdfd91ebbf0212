"""The rocket HIP kernel (csrc/kernels/rocket.hip) against the float64 definition (``ops.rocket``).

The kernels' weights are integers, so on integer-valued streams every fp32 sum is exact: counts and features
must EQUAL the oracle's.  On real-valued streams a count may differ only by positions whose float64 ``C`` lies
within the fp32 rounding bound of the bias (``_rocket_util.ambiguity``)."""
import functools
import warnings

import pytest
import torch

from _rocket_util import REAL_CASES, ambiguity, hand_masks, hand_params, int_stream, real_case
from har.features.rocket import RocketFeaturizer
from har.ops import _native
from har.ops import rocket as R
from har.ops.rocket import (N_KERNELS, RocketParams, rocket_conv_torch, rocket_counts_torch, rocket_dilations,
                            rocket_features_into, rocket_features_torch)

pytestmark = pytest.mark.gpu

WINDOWS = (9, 33, 64, 65, 200, 257, 600)
SHAPES = [(W, A) for W in WINDOWS for A in (3, 6)] + [(200, 9)]


def _run(s, p, W, stride, want_counts=True):
    nw = R._window_count(s.shape[0], W, stride)
    out = torch.full((nw, p.n_features), float("nan"), device=s.device)
    counts = torch.full((nw, p.n_features), -1, dtype=torch.int32, device=s.device) if want_counts else None
    rocket_features_into(s, p, W, stride, out, 0, counts)
    return out, counts


def _assert_exact(s, p, W, stride):
    out, counts = _run(s, p, W, stride)
    ref = rocket_counts_torch(s, p, W, stride)
    assert counts.shape == ref.shape and torch.equal(counts, ref)
    assert torch.equal(out, R.counts_to_features(ref, p))
    return ref


# ------------------------------------------------------------------ exact: integer streams, half-integer biases
@pytest.mark.parametrize("n_windows", (1, 5, 67))
@pytest.mark.parametrize("stride_kind", ("W", "W//2", "7"))
@pytest.mark.parametrize("W,A", SHAPES)
def test_exact_on_integer_streams(cuda, W, A, stride_kind, n_windows):
    stride = {"W": W, "W//2": W // 2, "7": 7}[stride_kind]
    s = int_stream(n_windows, W, stride, A).to(cuda)
    p = hand_params(W, A)
    sizes = {bin(int(m)).count("1") for m in p.masks.flatten()}
    assert sizes == set(range(1, A + 1))                       # every axis-subset size is exercised
    ref = _assert_exact(s, p, W, stride)
    assert ref.shape == (n_windows, N_KERNELS * len(rocket_dilations(W)) * 3)
    if n_windows * W >= 200:                                   # not a degenerate case: counts of both kinds occur
        L = p.range_lengths().to(cuda).repeat_interleave(3, 1).reshape(1, -1)
        assert bool((ref > 0).any()) and bool((ref < L).any())


# ------------------------------------------------------------------ ties: the comparison is strict
@pytest.mark.parametrize("W,A", [(33, 3), (200, 3), (257, 6), (200, 9)])
def test_ties_are_not_counted(cuda, W, A):
    s = int_stream(5, W, W, A, lo=-3, hi=3).to(cuda)
    masks = hand_masks(W, A)
    n_dil, q = masks.shape[0], 3
    tmp = RocketParams(W, A, masks, torch.zeros(n_dil, N_KERNELS, q))
    C = rocket_conv_torch(s, tmp, W, W)                        # [5, n_dil * 84, W], integers
    # biases = values C attains inside every combination's counted range (the middle is in both kinds of range)
    mid = W // 2
    b = torch.stack([C[0, :, mid], C[1, :, mid], C[2, :, max(mid - 1, 0)]], 1).float().view(n_dil, N_KERNELS, q)
    p = RocketParams(W, A, masks, b.cpu())
    assert torch.equal(p.biases.double(), b.double().cpu())    # integers: exact in fp32
    ref = _assert_exact(s, p, W, W)
    ties = (C[:, :, None, :] == b.double().view(1, -1, q, 1)).sum(-1)
    assert int(ties.sum()) >= 3 * n_dil * N_KERNELS and int(ref.sum()) > 0


# ------------------------------------------------------------------ zero and constant windows
@pytest.mark.parametrize("W,A", [(64, 3), (200, 3), (257, 6)])
def test_zero_and_constant_windows(cuda, W, A):
    masks = hand_masks(W, A)
    n_dil = masks.shape[0]
    b = torch.tensor([-0.5, 0.0, 0.5, 20.5]).repeat(n_dil, N_KERNELS, 1)
    p = RocketParams(W, A, masks, b)
    zero = torch.zeros(3 * W, A, device=cuda)
    ref = _assert_exact(zero, p, W, W)
    L = p.range_lengths().to(cuda)
    assert torch.equal(ref.view(3, n_dil, N_KERNELS, 4)[..., 0], L.expand(3, -1, -1).to(torch.int32))  # 0 > -0.5
    assert int(ref.view(3, n_dil, N_KERNELS, 4)[..., 1:].sum()) == 0                                  # 0 > 0 is false
    const = torch.full((3 * W, A), 7.0, device=cuda)
    ref = _assert_exact(const, p, W, W).view(3, n_dil, N_KERNELS, 4)
    odd = ((torch.arange(n_dil).view(-1, 1) + torch.arange(N_KERNELS).view(1, -1)) % 2 == 1).to(cuda)
    assert int(ref[:, odd][..., 1:].sum()) == 0            # valid-only ranges see the zero interior alone
    assert int(ref[:, ~odd][..., 2].sum()) > 0             # the padded edge is not zero


# ------------------------------------------------------------------ real-valued streams: the near-tie rule
@functools.lru_cache(maxsize=None)
def _real(n_windows, W, A):
    s, p = real_case(n_windows, W, A)
    s = s.to("cuda:0")
    return s, p, ambiguity(s, p, W, W)


@pytest.mark.parametrize("n_windows,W,A", REAL_CASES)
def test_real_valued_within_ambiguity(cuda, n_windows, W, A):
    s, p, (c64, amb, counted) = _real(n_windows, W, A)
    out, counts = _run(s, p, W, W)
    diff = (counts.long() - c64).abs()
    print(f"rocket real-valued ({n_windows}, {W}, {A}): largest |count_dev - count64| {int(diff.max())}, "
          f"cells differing {int((diff > 0).sum())} of {diff.numel()}, ambiguous positions {int(amb.sum())} "
          f"of {int(counted.sum())}")
    assert bool((diff <= amb).all())
    assert torch.equal(out, R.counts_to_features(counts, p))


# ------------------------------------------------------------------ layout
def test_layout_guards_stay_untouched(cuda):
    W, A, nw, col0 = 65, 3, 5, 5
    s = int_stream(nw, W, W, A).to(cuda)
    p = hand_params(W, A)
    F = p.n_features
    big = torch.full((nw + 2, col0 + F + 3), float("nan"), device=cuda)
    rocket_features_into(s, p, W, W, big[1: nw + 1], col0)
    assert torch.equal(big[1: nw + 1, col0: col0 + F], rocket_features_torch(s, p, W, W))
    assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all())
    assert bool(torch.isnan(big[:, :col0]).all()) and bool(torch.isnan(big[:, col0 + F:]).all())


# ------------------------------------------------------------------ determinism and invariance
def test_deterministic_and_independent_of_grouping(cuda):
    n_windows, W, A = REAL_CASES[0]
    s, p, _ = _real(n_windows, W, A)
    a, ca = _run(s, p, W, W)
    b, cb = _run(s, p, W, W)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    for i in (0, 1, 33, 66):                                   # alone == inside the batch of 67
        one, _ = _run(s[i * W: (i + 1) * W].contiguous(), p, W, W, want_counts=False)
        assert torch.equal(one[0], a[i])
    half, _ = _run(s, p, W, W // 2, want_counts=False)         # overlapping windows == the same windows gathered
    starts = torch.arange(half.shape[0], device=cuda) * (W // 2)
    idx = (starts.view(-1, 1) + torch.arange(W, device=cuda).view(1, -1)).reshape(-1)
    gathered, _ = _run(s.index_select(0, idx).contiguous(), p, W, W, want_counts=False)
    assert torch.equal(half, gathered)
    assert torch.equal(half[::2], a[: (half.shape[0] + 1) // 2])


def test_launch_issues_no_host_read(cuda):
    W, A = 200, 3
    s = int_stream(67, W, W, A).to(cuda)
    p = hand_params(W, A)
    out, counts = _run(s, p, W, W)                             # loads the module, copies the parameters once
    out2, counts2 = torch.empty_like(out), torch.empty_like(counts)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                    # a synchronizing call (any device -> host read) raises
    try:
        rocket_features_into(s, p, W, W, out2, 0, counts2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out, out2) and torch.equal(counts, counts2)


# ------------------------------------------------------------------ contract
def test_bad_arguments_raise_before_any_launch(cuda):
    W, A = 33, 3
    s = int_stream(5, W, W, A).to(cuda)
    p = hand_params(W, A)
    F = p.n_features
    out = torch.full((5, F), float("nan"), device=cuda)
    bad = [
        lambda: rocket_features_into(s.double(), p, W, W, out, 0),                            # stream dtype
        lambda: rocket_features_into(s, p, W, W, out.double(), 0),                            # out dtype
        lambda: rocket_features_into(s.flatten(), p, W, W, out, 0),                           # stream shape
        lambda: rocket_features_into(s, p, W, W, out[:4], 0),                                 # rows
        lambda: rocket_features_into(s, p, W, W, out, 1),                                     # short out
        lambda: rocket_features_into(s, p, W, W, out[:, : F - 1], 0),
        lambda: rocket_features_into(s, p, W, W, out, 0, torch.zeros(5, F, device=cuda)),     # counts dtype
        lambda: rocket_features_into(s, p, W, W, out, 0, torch.zeros(4, F, dtype=torch.int32, device=cuda)),
        lambda: rocket_features_into(s, p, 8, 8, out, 0),                                     # W < 9
        lambda: rocket_features_into(s, p, W, 0, out, 0),                                     # stride
        lambda: rocket_features_into(torch.zeros(5 * W, 4, device=cuda), p, W, W, out, 0),    # A = 4
        lambda: rocket_features_into(torch.zeros(5 * W, 6, device=cuda), p, W, W, out, 0),    # not the parameters' axes
        lambda: rocket_features_into(s, hand_params(65, A), W, W, out, 0),                    # not the parameters' window
        lambda: RocketParams(8, 3, torch.ones(1, N_KERNELS, dtype=torch.int32), torch.zeros(1, N_KERNELS, 1)),
        lambda: RocketParams(W, 4, p.masks, p.biases),
        lambda: RocketParams(W, A, torch.zeros_like(p.masks), p.biases),                      # an empty axis subset
        lambda: RocketParams(W, A, p.masks, p.biases.double()),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert bool(torch.isnan(out).all())                        # nothing ran
    k = _native.kernels()
    m, b = p.on(cuda)
    args = lambda **kw: {**dict(n_samples=s.shape[0], axes=A, window=W, stride=W, n_windows=5, n_dil=len(p.dilations),  # noqa: E731
                                q=p.q, ld=F, col0=0), **kw}

    def native(**kw):
        a = args(**kw)
        k.rocket_features(s.data_ptr(), a["n_samples"], a["axes"], a["window"], a["stride"], a["n_windows"], a["n_dil"],
                          a["q"], m.data_ptr(), b.data_ptr(), out.data_ptr(), a["ld"], a["col0"], 0,
                          _native.stream_ptr())

    for kw, code in ((dict(axes=4), -2), (dict(window=8), -2), (dict(n_dil=4), -2), (dict(q=0), -2),
                     (dict(n_windows=6), -3), (dict(ld=F - 1), -4), (dict(col0=1), -4)):
        with pytest.raises(RuntimeError, match=f"contract violation code {code}"):
            native(**kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_window_over_the_maximum_warns_once_and_matches(cuda):
    k = _native.kernels()
    assert k.rocket_max_window(4) == 0 and k.rocket_max_window(3) > k.rocket_max_window(6) > k.rocket_max_window(9) >= 600
    A = 3
    at = k.rocket_max_window(A)
    for W, expect_warning in ((at, False), (at + 4, True), (at + 4, False)):
        s = int_stream(2, W, W, A, seed=W).to(cuda)
        n_dil = len(rocket_dilations(W))
        p = RocketParams(W, A, hand_masks(W, A), torch.full((n_dil, N_KERNELS, 1), 0.5))
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            out, counts = _run(s, p, W, W)
        assert bool(rec) == expect_warning, [str(r.message) for r in rec]
        ref = rocket_counts_torch(s, p, W, W)
        assert torch.equal(counts, ref) and torch.equal(out, R.counts_to_features(ref, p))


# ------------------------------------------------------------------ end to end
def test_model_transform_on_device_matches_the_cpu_path(cuda):
    from har.data.synth import StreamSpec, generate_stream

    s, _ = generate_stream(67, StreamSpec())
    model = RocketFeaturizer().fit(s)
    assert model.num_features == 1680 and model.window == 200
    cpu = model.transform(s)
    dev = model.transform(s.to(cuda))
    assert dev.is_cuda and dev.dtype == torch.float32 and dev.shape == cpu.shape == (67, 1680)
    p = model.rocket_params
    _, amb, _ = ambiguity(s.to(cuda), p, 200, 200)
    L = p.range_lengths().float().repeat_interleave(p.q, 1).reshape(1, -1)
    c_cpu, c_dev = torch.round(cpu * L).long(), torch.round(dev.cpu() * L).long()
    assert torch.equal(c_cpu.float() / L, cpu) and torch.equal(c_dev.float() / L, dev.cpu())
    diff = (c_dev - c_cpu).abs()
    print(f"rocket end to end: largest |count_dev - count_cpu| {int(diff.max())}, mean |d feature| "
          f"{float((dev.cpu() - cpu).abs().mean()):.3g}")
    assert bool((diff <= amb.cpu()).all())
    buf = torch.full((67, 3 + 1680), float("nan"), device=cuda)  # the tail of a wider row buffer
    model.transform_into(s.to(cuda), buf, 3)
    assert torch.equal(buf[:, 3:], dev) and bool(torch.isnan(buf[:, :3]).all())
