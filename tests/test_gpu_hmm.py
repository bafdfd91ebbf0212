"""The HIP Viterbi decode (``csrc/kernels/hmm.hip``) against the sequential definition
(``har.ops.hmm.viterbi_torch``) run on the CPU over the same int32 inputs.  Every score is an integer, so
every comparison is ``torch.equal`` on the path and on the scores — never a tolerance."""
import numpy as np
import pytest
import torch

from har.models.hmm import HMMSmoother
from har.ops import hmm as H

pytestmark = pytest.mark.gpu

FLOOR = -(1 << 25)


def _rand(rng, shape, kind="logprob"):
    if kind == "logprob":      # anything a quantised log-probability can be
        v = rng.integers(FLOOR, 1, size=shape)
    elif kind == "near":       # values a few quanta apart: near-ties everywhere
        v = rng.integers(-40, 1, size=shape)
    else:                      # three integer values: exact ties everywhere
        v = rng.integers(-2, 1, size=shape)
    return torch.as_tensor(v, dtype=torch.int32)


def _problem(rng, T, K, kind="logprob"):
    return _rand(rng, (T, K), kind), _rand(rng, (K, K), kind), _rand(rng, (K,), kind)


def _offsets(lens):
    return torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)


def _check(cuda, E, A, pi, off, **kw):
    want_p, want_s = H.viterbi_torch(E, A, pi, off)
    path, score = H.viterbi_native(E.to(cuda), A.to(cuda), pi.to(cuda), off, **kw)
    assert path.dtype == torch.int32 and score.dtype == torch.int64
    assert torch.equal(path.cpu(), want_p)
    assert torch.equal(score.cpu(), want_s)
    return path, score


@pytest.fixture(scope="module")
def LG(cuda):
    return H.chunk_len(), H.scan_group()


@pytest.mark.parametrize("K", [1, 2, 6, 8, 9, 17, 32])
def test_one_sequence_lengths(cuda, LG, K):
    L, G = LG
    rng = np.random.default_rng(K)
    # around one chunk, several chunks with a tail, and G + 1 chunks: the smallest decode whose chunk scan
    # takes the second level
    for T in (1, 2, L - 1, L, L + 1, 3 * L + 5, G * L + 1):
        for kind in ("logprob", "near"):
            E, A, pi = _problem(rng, T, K, kind)
            _check(cuda, E, A, pi, _offsets([T]))


@pytest.mark.parametrize("K", [3, 9])
def test_three_scan_levels_with_short_chunks(cuda, LG, K):
    """Chunk length 1 and 5: G^2 + 1 chunks take a third level at a small T."""
    _, G = LG
    rng = np.random.default_rng(50 + K)
    T = G * G + 70
    E, A, pi = _problem(rng, T, K, "near")
    lens = [T // 3, 1, T - T // 3 - 1]
    for chunk in (1, 5):
        _check(cuda, E, A, pi, _offsets([T]), chunk=chunk)
        _check(cuda, E, A, pi, _offsets(lens), chunk=chunk)


def test_layout_all_sequences_of_length_one(cuda, LG):
    L, _ = LG
    rng = np.random.default_rng(1)
    T = 3 * L + 5
    for K in (1, 6, 17):
        E, A, pi = _problem(rng, T, K)
        _check(cuda, E, A, pi, _offsets([1] * T))


def test_layout_boundaries_at_chunk_edges(cuda, LG):
    L, _ = LG
    rng = np.random.default_rng(2)
    cuts = [0, L - 1, L, L + 1, 2 * L, 2 * L + 1, 3 * L - 1, 3 * L, 4 * L + 3]
    off = torch.tensor(cuts, dtype=torch.int64)
    for K in (2, 6, 9):
        for kind in ("logprob", "coarse"):
            E, A, pi = _problem(rng, cuts[-1], K, kind)
            _check(cuda, E, A, pi, off)


def test_layout_random_short_sequences(cuda, LG):
    L, G = LG
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 9, size=(L * G) // 4 + 40)     # ~ L G + 180 steps: resets inside second-level products
    assert lens.sum() > L * G
    for K in (6, 32):
        E, A, pi = _problem(rng, int(lens.sum()), K, "near")
        _check(cuda, E, A, pi, _offsets(lens))


def test_layout_one_long_sequence_between_short_ones(cuda, LG):
    L, G = LG
    rng = np.random.default_rng(4)
    lens = list(rng.integers(1, 9, size=60)) + [L * G + 77] + list(rng.integers(1, 9, size=60))
    for K in (6, 9):
        E, A, pi = _problem(rng, int(np.sum(lens)), K, "near")
        _check(cuda, E, A, pi, _offsets(lens))


def test_ties(cuda, LG):
    L, _ = LG
    rng = np.random.default_rng(5)
    T = 3 * L + 5
    off = _offsets([L, 1, L + 4, L])
    for K in (2, 6, 9, 32):
        z = lambda *s: torch.zeros(*s, dtype=torch.int32)
        path, score = _check(cuda, z(T, K), z(K, K), z(K), off)          # all equal: the zero path
        assert int(path.abs().max()) == 0 and int(score.abs().max()) == 0
        E, A, pi = _problem(rng, T, K, "coarse")                          # three integer values
        _check(cuda, E, A, pi, off)
        _check(cuda, E, A, pi, _offsets([T]))
        if K >= 2:                                                         # two identical states
            E, A, pi = _problem(rng, T, K, "near")
            a, b = 0, K - 1
            E[:, b], pi[b] = E[:, a], pi[a]
            A[b, :] = A[a, :]
            A[:, b] = A[:, a]
            A[b, b] = A[a, a] = A[a, b] = A[b, a]
            path, _ = _check(cuda, E, A, pi, off)
            assert not bool((path == b).any())                             # the lower twin wins every tie


def test_floors_need_int64(cuda):
    """E, A and pi all at -2^25: 2^26 per step overflows an int32 accumulator after 32 steps."""
    T, K = 100, 2
    f = lambda *s: torch.full(s, FLOOR, dtype=torch.int32)
    path, score = _check(cuda, f(T, K), f(K, K), f(K), _offsets([T]))
    assert score.tolist() == [FLOOR * (2 * T)] and FLOOR * (2 * T) < -(1 << 31)
    _check(cuda, f(T, K), f(K, K), f(K), _offsets([40, 60]))


def test_forbidden_transitions(cuda, LG):
    """A at the floor off the band |i - j| <= 1: the path may only move to a neighbouring state."""
    L, _ = LG
    rng = np.random.default_rng(6)
    T = 3 * L + 5
    for K in (6, 9):
        i = torch.arange(K)
        band = (i[:, None] - i[None, :]).abs() <= 1
        A = torch.where(band, _rand(rng, (K, K), "near"), torch.full((K, K), FLOOR, dtype=torch.int32))
        E = torch.as_tensor(rng.integers(-(1 << 22), 1, size=(T, K)), dtype=torch.int32)
        path, _ = _check(cuda, E, A, _rand(rng, (K,), "near"), _offsets([T]))
        assert int((path[1:] - path[:-1]).abs().max()) <= 1


def test_outputs_and_workspace_stay_inside_their_buffers(cuda, LG):
    L, G = LG
    rng = np.random.default_rng(8)
    lens = [L + 3, 1, 1, G * L + 9, 7]
    T, S, K = int(np.sum(lens)), len(lens), 9
    E, A, pi = _problem(rng, T, K, "near")
    off = _offsets(lens)
    want_p, want_s = H.viterbi_torch(E, A, pi, off)
    need = int(H._native.kernels().hmm_workspace_bytes(T, K, S, L))
    pbuf = torch.full((T + 128,), -7, dtype=torch.int32, device=cuda)
    sbuf = torch.full((S + 64,), -7, dtype=torch.int64, device=cuda)
    wbuf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=cuda)
    path, score = H.viterbi_native(E.to(cuda), A.to(cuda), pi.to(cuda), off, out=(pbuf[64:64 + T], sbuf[32:32 + S]),
                                   workspace=wbuf[256:256 + need])
    assert torch.equal(path.cpu(), want_p) and torch.equal(score.cpu(), want_s)
    assert bool((pbuf[:64] == -7).all()) and bool((pbuf[64 + T:] == -7).all())
    assert bool((sbuf[:32] == -7).all()) and bool((sbuf[32 + S:] == -7).all())
    assert bool((wbuf[:256] == 0xA5).all()) and bool((wbuf[256 + need:] == 0xA5).all())
    with pytest.raises(ValueError):
        H.viterbi_native(E.to(cuda), A.to(cuda), pi.to(cuda), off, workspace=wbuf[:need - 1])


def test_decode_is_bitwise_reproducible(cuda, LG):
    L, G = LG
    rng = np.random.default_rng(9)
    lens = list(rng.integers(1, 200, size=40)) + [G * L + 1]
    E, A, pi = (t.to(cuda) for t in _problem(rng, int(np.sum(lens)), 6, "coarse"))
    a = H.viterbi_native(E, A, pi, _offsets(lens))
    b = H.viterbi_native(E, A, pi, _offsets(lens))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_end_to_end_from_probabilities(cuda):
    """Emission scores computed on the device; the oracle takes the SAME integers on the host."""
    g = torch.Generator().manual_seed(11)
    K, lens = 6, [700, 1, 152, 152, 995]
    n = sum(lens)
    y = torch.repeat_interleave(torch.randint(0, K, (n // 8 + 1,), generator=g), 8)[:n]
    logits = torch.randn(n, K, generator=g) * 1.5
    logits[torch.arange(n), y] += 2.0
    prob = torch.softmax(logits, dim=1)
    prob[5] = torch.tensor([1.0, 0, 0, 0, 0, 0])                 # exact zeros: the floor
    off = _offsets(lens)
    for emission in ("scaled", "posterior"):
        model = HMMSmoother(emission=emission).fit_labels(y, off, K)
        E_dev = model.emission_scores(prob.to(cuda))
        assert E_dev.is_cuda and E_dev.dtype == torch.int32 and int(E_dev.min()) == FLOOR
        E_host = E_dev.cpu()
        want_p, want_s = H.viterbi_torch(E_host, model.qA, model.qpi, off)
        path, score = H.viterbi(E_dev, model.qA.to(cuda), model.qpi.to(cuda), off)
        assert path.is_cuda and torch.equal(path.cpu(), want_p) and torch.equal(score.cpu(), want_s)
        # the model on device tensors = the CPU model given the same E
        p_dev, s_dev = model.decode_scores(E_dev, off)
        p_cpu, s_cpu = model.decode_scores(E_host, off)
        assert p_dev.is_cuda and not p_cpu.is_cuda
        assert torch.equal(p_dev.cpu(), p_cpu) and torch.equal(s_dev.cpu(), s_cpu)
        p2, s2 = model.decode(prob.to(cuda), off)
        assert torch.equal(p2, p_dev) and torch.equal(s2, s_dev)


def test_limits_raise_before_any_launch(cuda):
    z = lambda dev, *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    for dev in (torch.device("cpu"), cuda):
        with pytest.raises(ValueError):
            H.viterbi(z(dev, 5, 33), z(dev, 33, 33), z(dev, 33), torch.tensor([0, 5]))
        for bad in ([0, 3, 3, 5], [0, 4, 2, 5], [0, 4], [1, 5]):
            with pytest.raises(ValueError):
                H.viterbi(z(dev, 5, 2), z(dev, 2, 2), z(dev, 2), torch.tensor(bad, dtype=torch.int64))
        path, score = H.viterbi(z(dev, 0, 4), z(dev, 4, 4), z(dev, 4), torch.tensor([0], dtype=torch.int64))
        assert path.shape == (0,) and score.shape == (0,) and path.device.type == dev.type
