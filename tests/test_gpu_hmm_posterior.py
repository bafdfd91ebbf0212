"""The HIP forward-backward (``csrc/kernels/hmm_fb.hip``) against the sequential definition
(``har.ops.hmm.forward_backward_torch``) run on the CPU over the same fp64 bits of ``B``, ``P`` and ``p0``.

Every comparison uses the derived bound ``eta(T, K) = 16 (K + 4) T 2^-53`` with T the batch length (see
``tests/test_hmm_posterior.py``): ``|x - ref| <= eta ref`` elementwise for ``gamma`` and ``xi`` (no absolute
term), ``|x - ref| <= eta (1 + |ref|)`` for ``loglik``.  At K > 8 both phase-1 kernels run (lanes and MFMA).

Each check prints its largest ``error / eta``."""
import math

import numpy as np
import pytest
import torch

from har.models import hmm as M
from har.models.hmm import HMMSmoother
from har.ops import hmm as H

pytestmark = pytest.mark.gpu

F64 = torch.float64
FLOOR = -(1 << 25)


def eta(T, K):
    return 16.0 * (K + 4) * max(T, 1) * 2.0 ** -53


def _offsets(lens):
    return torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)


def _scores(rng, shape, kind):
    if kind == "full":         # anything a quantised score can be: B down to e^-64, P down to the floor
        v = rng.integers(FLOOR, 1, size=shape)
    elif kind == "logprob":    # ordinary log-probabilities
        v = -(8.0 * rng.random(shape) * (1 << 20)).astype(np.int64)
    else:                      # a few quanta apart: near-ties everywhere
        v = rng.integers(-40, 1, size=shape)
    return torch.as_tensor(v, dtype=torch.int32)


def _problem(rng, T, K, kind="full"):
    """(B, P, p0) on the CPU through the module's helpers."""
    return (H.emission_likelihoods(_scores(rng, (T, K), kind)), H.transition_probs(_scores(rng, (K, K), kind)),
            H.start_probs(_scores(rng, (K,), kind)))


def _variants(K):
    return ("lanes", "mfma") if K > 8 else ("auto",)


def _ratio(x, ref, tol, loglik=False):
    x = x.cpu()
    assert x.shape == ref.shape and torch.isfinite(x).all()
    if not ref.numel():
        return 0.0
    bound = tol * (1 + ref.abs()) if loglik else tol * ref
    err = (x - ref).abs()
    assert bool((err[bound == 0] == 0).all())      # an exact zero (xi without an inner step) has no slack
    return float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0


def _check(cuda, B, P, p0, off, label="", **kw):
    T, K = B.shape
    tol = eta(T, K)
    want = H.forward_backward_torch(B, P, p0, off, want_xi=True)
    worst = 0.0
    for variant in _variants(K):
        got = H.forward_backward_native(B.to(cuda), P.to(cuda), p0.to(cuda), off, want_xi=True, variant=variant, **kw)
        assert all(g.dtype == F64 and g.is_cuda for g in got)
        r = (_ratio(got[0], want[0], tol), _ratio(got[1], want[1], tol, True), _ratio(got[2], want[2], tol))
        print(f"{label} T={T} K={K} {variant}: error/eta gamma {r[0]:.3g} loglik {r[1]:.3g} xi {r[2]:.3g}")
        assert max(r) <= 1.0, (label, T, K, variant, r)
        worst = max(worst, *r)
    return worst


@pytest.fixture(scope="module")
def LG(cuda):
    return H.chunk_len(), H.scan_group()


@pytest.mark.parametrize("K", [1, 2, 6, 8, 9, 17, 32])
def test_one_sequence_lengths(cuda, LG, K):
    L, G = LG
    rng = np.random.default_rng(K)
    for T in (1, 2, L - 1, L, L + 1, 3 * L + 5, G * L + 1):
        for kind in ("full", "near"):
            _check(cuda, *_problem(rng, T, K, kind), _offsets([T]), label=kind)


def test_layout_all_sequences_of_length_one(cuda, LG):
    L, _ = LG
    rng = np.random.default_rng(1)
    T = 3 * L + 5
    for K in (1, 6, 17):
        _check(cuda, *_problem(rng, T, K, "logprob"), _offsets([1] * T), label="len1")


def test_layout_boundaries_at_chunk_edges(cuda, LG):
    L, _ = LG
    rng = np.random.default_rng(2)
    cuts = [0, L - 1, L, L + 1, 2 * L, 2 * L + 1, 3 * L - 1, 3 * L, 4 * L + 3]
    off = torch.tensor(cuts, dtype=torch.int64)
    for K in (2, 6, 9):
        for kind in ("full", "near"):
            _check(cuda, *_problem(rng, cuts[-1], K, kind), off, label="edges " + kind)


def test_layout_one_long_sequence_between_short_ones(cuda, LG):
    L, G = LG
    rng = np.random.default_rng(4)
    lens = list(rng.integers(1, 9, size=60)) + [L * G + 77] + list(rng.integers(1, 9, size=60))
    for K in (6, 9):
        _check(cuda, *_problem(rng, int(np.sum(lens)), K, "logprob"), _offsets(lens), label="long+short")


@pytest.mark.parametrize("K", [3, 9])
def test_three_scan_levels_with_short_chunks(cuda, LG, K):
    """Chunk length 1 at G^2 + 70 steps and chunk length 5 at 5 G^2 + 70: G^2 + 1 chunks and more take a third
    level at a small T (chunk length 5 also runs the G^2 + 70 steps, on two levels)."""
    _, G = LG
    rng = np.random.default_rng(50 + K)
    T = G * G + 70
    B, P, p0 = _problem(rng, T, K, "logprob")
    lens = [T // 3, 1, T - T // 3 - 1]
    for chunk in (1, 5):
        _check(cuda, B, P, p0, _offsets([T]), label=f"chunk={chunk}", chunk=chunk)
        _check(cuda, B, P, p0, _offsets(lens), label=f"chunk={chunk}", chunk=chunk)
    T5 = 5 * G * G + 70
    _check(cuda, *_problem(rng, T5, K, "near"), _offsets([T5 // 2, T5 - T5 // 2]), label="chunk=5", chunk=5)


def _adversarial(T, K, seed=0):
    """Emission rows at the floor except one (moving) entry, transitions with forbidden entries, a start vector
    with one allowed state."""
    rng = np.random.default_rng(seed)
    E = torch.full((T, K), FLOOR, dtype=torch.int32)
    E[torch.arange(T), torch.as_tensor(rng.integers(0, K, T))] = 1 << 25
    logA = torch.as_tensor(np.log(rng.random((K, K)) + 0.05))
    logA[torch.as_tensor(rng.random((K, K)) < 0.4)] = float("-inf")
    logpi = torch.full((K,), float("-inf"), dtype=F64)
    logpi[K - 1] = 0.0
    return H.emission_likelihoods(E), H.transition_probs(H.quantize_logprob(logA)), H.start_probs(H.quantize_logprob(logpi))


@pytest.mark.parametrize("K", [6, 32])
def test_adversarial_floors_and_forbidden_transitions(cuda, LG, K):
    L, G = LG
    T = G * L + 1
    B, P, p0 = _adversarial(T, K)
    for off in (_offsets([T]), _offsets([1000, 1, T - 1001])):
        _check(cuda, B, P, p0, off, label="adversarial")
    gamma, ll, xi = H.forward_backward_native(B.to(cuda), P.to(cuda), p0.to(cuda), _offsets([T]), want_xi=True)
    assert bool((gamma > 0).all()) and bool((xi > 0).all()) and bool(torch.isfinite(ll).all())


def test_outputs_and_workspace_stay_inside_their_buffers(cuda, LG):
    L, G = LG
    rng = np.random.default_rng(8)
    lens = [L + 3, 1, 1, G * L + 9, 7]
    T, S = int(np.sum(lens)), len(lens)
    off = _offsets(lens)
    nan = float("nan")
    for K in (7, 9):     # K = 7 at an odd element offset: the 16-byte stores of gamma start one element late
        B, P, p0 = _problem(rng, T, K, "logprob")
        want = H.forward_backward_torch(B, P, p0, off, want_xi=True)
        need = int(H._native.kernels().hmm_fb_workspace_bytes(T, K, S, L, True))
        assert need >= int(H._native.kernels().hmm_fb_workspace_bytes(T, K, S, L, False))
        gbuf = torch.full((T * K + 128,), nan, dtype=F64, device=cuda)
        lbuf = torch.full((S + 64,), nan, dtype=F64, device=cuda)
        xbuf = torch.full((K * K + 64,), nan, dtype=F64, device=cuda)
        wbuf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=cuda)
        out = (gbuf[63:63 + T * K].view(T, K), lbuf[31:31 + S], xbuf[33:33 + K * K].view(K, K))
        for variant in _variants(K):
            gamma, ll, xi = H.forward_backward_native(B.to(cuda), P.to(cuda), p0.to(cuda), off, want_xi=True, out=out,
                                                      workspace=wbuf[256:256 + need], variant=variant)
            tol = eta(T, K)
            assert max(_ratio(gamma, want[0], tol), _ratio(ll, want[1], tol, True), _ratio(xi, want[2], tol)) <= 1.0
            assert bool(torch.isnan(gbuf[:63]).all()) and bool(torch.isnan(gbuf[63 + T * K:]).all())
            assert bool(torch.isnan(lbuf[:31]).all()) and bool(torch.isnan(lbuf[31 + S:]).all())
            assert bool(torch.isnan(xbuf[:33]).all()) and bool(torch.isnan(xbuf[33 + K * K:]).all())
            assert bool((wbuf[:256] == 0xA5).all()) and bool((wbuf[256 + need:] == 0xA5).all())
        with pytest.raises(ValueError):
            H.forward_backward_native(B.to(cuda), P.to(cuda), p0.to(cuda), off, want_xi=True, workspace=wbuf[:need - 1])


def test_xi_is_optional_and_runs_are_bitwise_reproducible(cuda, LG):
    L, G = LG
    rng = np.random.default_rng(9)
    lens = list(rng.integers(1, 200, size=40)) + [G * L + 1]
    off = _offsets(lens)
    for K in (6, 17):
        B, P, p0 = (t.to(cuda) for t in _problem(rng, int(np.sum(lens)), K, "logprob"))
        a = H.forward_backward_native(B, P, p0, off, want_xi=True)
        b = H.forward_backward_native(B, P, p0, off, want_xi=True)
        c = H.forward_backward_native(B, P, p0, off, want_xi=False)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert c[2] is None and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
        assert torch.equal(H.forward_backward(B, P, p0, off)[0], a[0])   # the dispatcher takes the kernels


def test_a_whole_call_makes_no_host_synchronisation(cuda, LG):
    L, G = LG
    rng = np.random.default_rng(10)
    lens = [L, 1, G * L + 3]
    T, S, K = int(np.sum(lens)), len(lens), 9
    off = _offsets(lens)
    B, P, p0 = _problem(rng, T, K, "logprob")
    want = H.forward_backward_torch(B, P, p0, off, want_xi=True)
    Bd, Pd, p0d, offd = B.to(cuda), P.to(cuda), p0.to(cuda), off.to(cuda)
    out = (torch.empty(T, K, dtype=F64, device=cuda), torch.empty(S, dtype=F64, device=cuda),
           torch.empty(K, K, dtype=F64, device=cuda))
    ws = torch.empty(int(H._native.kernels().hmm_fb_workspace_bytes(T, K, S, L, True)), dtype=torch.uint8, device=cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = H.forward_backward_native(Bd, Pd, p0d, off, want_xi=True, out=out, workspace=ws, offsets_device=offd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    tol = eta(T, K)
    assert max(_ratio(got[0], want[0], tol), _ratio(got[1], want[1], tol, True), _ratio(got[2], want[2], tol)) <= 1.0


def _stream_like(seed=11):
    g = torch.Generator().manual_seed(seed)
    K, lens = 6, [700, 1, 152, 152, 995]
    n = sum(lens)
    y = torch.repeat_interleave(torch.randint(0, K, (n // 8 + 1,), generator=g), 8)[:n]
    logits = torch.randn(n, K, generator=g, dtype=F64) * 1.5
    logits[torch.arange(n), y] += 2.0
    prob = torch.softmax(logits, dim=1)
    prob[5] = torch.tensor([1.0, 0, 0, 0, 0, 0], dtype=F64)      # exact zeros: the floor
    return K, y, prob, _offsets(lens)


def test_end_to_end_from_device_probabilities(cuda):
    K, y, prob, off = _stream_like()
    n = prob.shape[0]
    tol = eta(n, K)
    for emission in ("scaled", "posterior"):
        model = HMMSmoother(emission=emission).fit_labels(y, off, K)
        g_dev, l_dev = model.posterior(prob.to(cuda), off)
        g_cpu, l_cpu = model.posterior(prob, off)
        assert g_dev.is_cuda and l_dev.is_cuda and not g_cpu.is_cuda
        r = (_ratio(g_dev, g_cpu, tol), _ratio(l_dev, l_cpu, tol, True))
        print(f"end to end {emission}: error/eta gamma {r[0]:.3g} loglik {r[1]:.3g}")
        assert max(r) <= 1.0


def test_one_em_iteration_on_the_device(cuda):
    K, y, prob, off = _stream_like(12)
    model = HMMSmoother(stay=0.5).fit_stay(K)
    B = H.emission_likelihoods(model.emission_scores(prob))
    tol = eta(prob.shape[0], K)
    P1, p01, ll1 = M.baum_welch_step(B, model.P, model.p0, off, 1.0)
    P2, p02, ll2 = M.baum_welch_step(B.to(cuda), model.P.to(cuda), model.p0.to(cuda), off, 1.0)
    assert P2.is_cuda and p02.is_cuda and ll2.is_cuda
    r = (_ratio(P2, P1, tol), _ratio(p02, p01, tol), _ratio(ll2.view(1), ll1.view(1), tol, True))
    print(f"one EM iteration: error/eta P {r[0]:.3g} p0 {r[1]:.3g} loglik {r[2]:.3g}")
    assert max(r) <= 1.0
    # and the estimator end to end on the device: the same history as on the CPU
    from har.data.table import Column, Table

    tab = Table([Column("probability", "vector", prob.numpy())])
    a = HMMSmoother(stay=0.5, numClasses=K, emIter=2, emTol=0.0, sequenceCol="none", device="cpu").fit(tab)
    b = HMMSmoother(stay=0.5, numClasses=K, emIter=2, emTol=0.0, sequenceCol="none", device=cuda).fit(tab)
    assert b.emIterations == 2 and len(b.objectiveHistory) == 2
    np.testing.assert_allclose(b.objectiveHistory, a.objectiveHistory, rtol=tol)


def test_limits_raise_before_any_launch(cuda, LG):
    L, _ = LG
    o = lambda dev, *s: torch.ones(*s, dtype=F64, device=dev)
    for dev in (torch.device("cpu"), cuda):
        with pytest.raises(ValueError):
            H.forward_backward(o(dev, 5, 33), o(dev, 33, 33), o(dev, 33), torch.tensor([0, 5]))
        for bad in ([0, 3, 3, 5], [0, 4, 2, 5], [0, 4], [1, 5]):
            with pytest.raises(ValueError):
                H.forward_backward(o(dev, 5, 2), o(dev, 2, 2), o(dev, 2), torch.tensor(bad, dtype=torch.int64))
        g, l, x = H.forward_backward(o(dev, 0, 4), o(dev, 4, 4), o(dev, 4), torch.tensor([0], dtype=torch.int64), want_xi=True)
        assert g.shape == (0, 4) and l.shape == (0,) and x.shape == (4, 4) and g.device.type == dev.type
    # a chunk whose alpha rows do not fit a workgroup's LDS is a bad shape, not a launch
    with pytest.raises(ValueError):
        H.forward_backward_native(o(cuda, 8, 32), o(cuda, 32, 32), o(cuda, 32), torch.tensor([0, 8]), chunk=257)
    with pytest.raises(ValueError):
        H.forward_backward_native(o(cuda, 8, 2), o(cuda, 2, 2), o(cuda, 2), torch.tensor([0, 8]), variant="fast")
    nat = H._native.kernels()
    assert nat.hmm_fb_workspace_bytes(8, 33, 1, L, False) == -1 and nat.hmm_fb_workspace_bytes(8, 4, 9, L, False) == -1
