"""The GBT kernels (csrc/kernels/gbt.hip) against their PyTorch definitions in har/ops/gbt.py.

Derivatives are fixed point, so the histogram and split kernels must EQUAL the oracle (integers, and the
fp64 gain bit for bit); only har_gbt_grad may differ, by at most one 2^-20 quantum per value (its fp64
softmax is not the host's libm bit for bit)."""
import numpy as np
import pytest
import torch

from har.models.gbt import GBTClassifier
from har.ops import _native
from har.ops import gbt as G
from har.ops import tree as T

pytestmark = pytest.mark.gpu

ROWS_PER_BLOCK = 1024  # gbt.hip HIST_ROWS (checked below against the library)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ har_gbt_grad
@pytest.mark.parametrize("K", [2, 6, 17, 32])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_grad_within_one_quantum(cuda, K, N):
    g = _gen(100 * K + N)
    m = torch.randn(N, K, generator=g) * 4
    m[::7] = torch.where(torch.rand(m[::7].shape, generator=g) < 0.5, 100.0, -100.0)  # saturated rows
    m[0, 0] = 100.0
    y = torch.randint(0, K, (N,), generator=g).to(torch.int32)
    w = (torch.rand(N, generator=g) < 0.6).to(torch.int32)
    for wt in (None, w):
        q_ref, l_ref = G.grad_torch(m, y, wt)
        q, parts = G.grad_native(m.to(cuda), y.to(cuda), None if wt is None else wt.to(cuda))
        torch.cuda.synchronize()
        q, loss = q.cpu(), parts.sum().cpu()
        assert parts.numel() == _native.kernels().gbt_grad_blocks(N, K)
        assert torch.isfinite(loss)
        d = (q.long() - q_ref.long()).abs()
        share = (d == 0).double().mean().item()
        print(f"gbt_grad K={K} N={N} weights={wt is not None}: equal share {share:.6f}, max diff {int(d.max())}")
        assert int(d.max()) <= 1
        torch.testing.assert_close(loss, l_ref.sum(), rtol=1e-5, atol=0)
        if wt is not None:
            assert (q[:, wt == 0] == 0).all()
    # loss only (no derivative output)
    _, parts = G.grad_native(m.to(cuda), y.to(cuda), None, want_q=False)
    torch.testing.assert_close(parts.sum().cpu(), l_ref.sum(), rtol=1e-5, atol=0)


# ------------------------------------------------------------------ har_gbt_hist
def _hist_case(cuda, N, F, B, level, seed):
    g = _gen(seed)
    K = 3
    nodes, first = 1 << level, (1 << level) - 1
    bins = torch.randint(0, B, (F, N), generator=g).to(torch.uint8)
    qgh = torch.stack([torch.randint(-(1 << 20), (1 << 20) + 1, (K, N), generator=g),
                       torch.randint(0, (1 << 18) + 1, (K, N), generator=g)], dim=-1).to(torch.int32)
    w = (torch.rand(N, generator=g) < 0.7).to(torch.int32)
    qgh = qgh * w.view(1, N, 1)
    # rows spread over about half of the level's nodes (the others stay empty), some resting in earlier leaves
    live = torch.randperm(nodes, generator=g)[: max(1, nodes // 2)]
    node_of = (first + live[torch.randint(0, len(live), (K, N), generator=g)]).to(torch.int32)
    if level > 0:
        rest = torch.rand(K, N, generator=g) < 0.1
        node_of[rest] = torch.randint(0, first, (int(rest.sum()),), generator=g).to(torch.int32)
    ref = G.hist_torch(bins, qgh, w, node_of, level, B)
    got = G.hist_native(bins.to(cuda), qgh.to(cuda), w.to(cuda), node_of.to(cuda), level, B)
    assert torch.equal(got.cpu(), ref), (N, F, B, level)
    return ref


@pytest.mark.parametrize("N", [1, 255, 257, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK + 1, 2 * ROWS_PER_BLOCK - 1,
                               2 * ROWS_PER_BLOCK + 1])
def test_hist_equals_oracle(cuda, N):
    assert _native.kernels().gbt_hist_rows_per_block() == ROWS_PER_BLOCK
    seed = 0
    for F in (1, 15, 16, 17, 43):
        for B in (2, 32, 64):
            for level in range(6):
                seed += 1
                ref = _hist_case(cuda, N, F, B, level, 1000 * N + seed)
    assert int(ref[..., 2].sum()) > 0 or N == 1


def test_hist_unweighted_and_overflow_corner(cuda):
    # no weight vector: every row counts
    g = _gen(5)
    N, F, B, K = 700, 5, 32, 2
    bins = torch.randint(0, B, (F, N), generator=g).to(torch.uint8)
    qgh = torch.randint(-1000, 1000, (K, N, 2), generator=g).to(torch.int32)
    node_of = torch.randint(1, 3, (K, N), generator=g).to(torch.int32)
    ref = G.hist_torch(bins, qgh, None, node_of, 1, B)
    got = G.hist_native(bins.to(cuda), qgh.to(cuda), None, node_of.to(cuda), 1, B)
    assert torch.equal(got.cpu(), ref) and int(ref[..., 2].sum()) == K * F * N
    # two full row chunks into ONE (node, feature, bin) with the largest derivatives: each workgroup's int32
    # LDS cell reaches 2^30, the merged total 2^31 needs the int64 histogram
    N = 2 * ROWS_PER_BLOCK
    bins = torch.full((1, N), 5, dtype=torch.uint8)
    qgh = torch.tensor([1 << 20, 1 << 18], dtype=torch.int32).view(1, 1, 2).repeat(1, N, 1)
    node_of = torch.zeros(1, N, dtype=torch.int32)
    got = G.hist_native(bins.to(cuda), qgh.to(cuda), None, node_of.to(cuda), 0, 32).cpu()
    assert got[0, 0, 0, 5].tolist() == [N << 20, N << 18, N] and int(got.abs().sum()) == (N << 20) + (N << 18) + N
    assert torch.equal(got, G.hist_torch(bins, qgh, None, node_of, 0, 32))


# ------------------------------------------------------------------ har_gbt_split
def _split_both(cuda, hist, nbins, lam, min_inst, min_gain, level, F, B, step=0.1, tree0=2):
    K = hist.shape[0]
    thr = torch.arange(F * B, dtype=torch.float32).view(F, B) * 0.5
    ref = G.split_torch(hist, nbins, lam, min_inst, min_gain)
    a_ref = G.GBTArrays.alloc(tree0 + K, 6, K, "cpu")
    G.commit_torch(ref, a_ref, level, tree0, thr, lam, step)
    a = G.GBTArrays.alloc(tree0 + K, 6, K, cuda)
    got = G.split_native(hist.to(cuda), nbins.to(cuda), thr.to(cuda), a, level, tree0, lam, step, min_inst, min_gain)
    torch.cuda.synchronize()
    assert torch.equal(got.feat.cpu(), ref.feat)
    assert torch.equal(got.bin.cpu(), ref.bin)
    assert torch.equal(got.sums.cpu(), ref.sums)
    assert torch.equal(got.gain.cpu().view(torch.int64), ref.gain.view(torch.int64))  # fp64, bit for bit
    for name in ("feature", "split_bin", "thresh", "left", "right", "gains", "value", "stats"):
        assert torch.equal(getattr(a, name).cpu(), getattr(a_ref, name)), name
    return ref


@pytest.mark.parametrize("level,F,B", [(0, 43, 32), (3, 17, 64), (5, 5, 32), (2, 1, 2), (4, 16, 7)])
def test_split_equals_oracle_random(cuda, level, F, B):
    g = _gen(10 * level + F)
    K, N = 4, 3000
    nodes, first = 1 << level, (1 << level) - 1
    nbins = torch.randint(1, B + 1, (F,), generator=g).to(torch.int32)
    nbins[0] = B
    bins = (torch.randint(0, 1 << 16, (F, N), generator=g) % nbins.view(F, 1)).to(torch.uint8)
    w = (torch.rand(N, generator=g) < 0.8).to(torch.int32)
    qgh = torch.stack([torch.randint(-(1 << 20), (1 << 20) + 1, (K, N), generator=g),
                       torch.randint(0, (1 << 18) + 1, (K, N), generator=g)], dim=-1).to(torch.int32) * w.view(1, N, 1)
    node_of = (first + torch.randint(0, max(1, nodes - 1), (K, N), generator=g)).to(torch.int32)  # last node empty
    hist = G.hist_torch(bins, qgh, w, node_of, level, B)
    n_split = 0
    for lam, min_inst, min_gain in ((1.0, 1, 0.0), (0.0, 5, 0.0), (1e-6, 5, 1e-3), (1.0, 2000, 0.0)):
        ref = _split_both(cuda, hist, nbins, lam, min_inst, min_gain, level, F, B)
        n_split += int((ref.feat >= 0).sum())
        if nodes > 1:
            assert (ref.feat[:, -1] == -1).all()  # the empty node: no valid cut
    if F > 1 or B > 2:
        assert n_split > 0


def test_split_ties_and_tiny_denominators(cuda):
    g = _gen(77)
    K, N, F, B, level = 2, 500, 6, 16, 1
    bins = torch.randint(0, B, (F, N), generator=g).to(torch.uint8)
    bins[3] = bins[1]                       # a duplicated feature: exact ties between features 1 and 3
    bins[2][bins[2] == 7] = 8               # bin 7 of feature 2 is empty: cuts 6 and 7 tie
    bins[0] = bins[1]                       # ... and feature 0 duplicates them too: the lowest index must win
    qgh = torch.stack([torch.randint(-(1 << 20), (1 << 20) + 1, (K, N), generator=g),
                       torch.randint(0, 3, (K, N), generator=g)], dim=-1).to(torch.int32)   # h of 0..2 quanta
    node_of = torch.randint(1, 3, (K, N), generator=g).to(torch.int32)
    hist = G.hist_torch(bins, qgh, None, node_of, level, B)
    nbins = torch.full((F,), B, dtype=torch.int32)
    for lam in (1e-6, 0.0, 1.0):            # H + lambda near 1e-6 (and exactly H: zero denominators are no cut)
        ref = _split_both(cuda, hist, nbins, lam, 5, 0.0, level, F, B)
        assert (ref.feat != 3).all() and (ref.feat != 1).all()
    # only the tied pair: features 1 and 2 identical, nothing else splits
    h2 = torch.zeros_like(hist)
    h2[:, :, 0, 0] = hist[:, :, 0].sum(dim=2)
    h2[:, :, 1] = hist[:, :, 2]
    h2[:, :, 2] = hist[:, :, 2]
    nb2 = nbins.clone()
    nb2[0] = 1
    ref = _split_both(cuda, h2, nb2, 1.0, 1, 0.0, level, F, B)
    assert (ref.feat == 1).all() and (ref.bin != 7).all()


# ------------------------------------------------------------------ a round, a fit, prediction
N_FIT, F_FIT, K_FIT, D_FIT = 2000, 43, 6, 4


@pytest.fixture(scope="module")
def problem():
    g = _gen(2024)
    mu = torch.randn(K_FIT, F_FIT, generator=g)
    y = torch.randint(0, K_FIT, (N_FIT,), generator=g)
    X = mu[y] + 2.5 * torch.randn(N_FIT, F_FIT, generator=g)
    tt = T.ThresholdTable.from_any(T.thresholds_for(X, 32, seed=0))
    return X, y, tt


def _est(**kw):
    return GBTClassifier(maxIter=10, maxDepth=D_FIT, stepSize=0.1, seed=0, **kw)


@pytest.fixture(scope="module")
def cpu_fit(problem):
    X, y, tt = problem
    return _est().fit_tensors(X, y, K_FIT, thresholds=tt)


def test_teacher_forced_round(cuda, problem):
    from har.ops.stats import bin_features

    X, y, tt = problem
    g = _gen(9)
    margins = (torch.randn(N_FIT, K_FIT, generator=g) * 2).float()
    nbins = torch.from_numpy((tt.counts + 1).astype(np.int32))
    thr = torch.from_numpy(tt.padded(32))
    bins = bin_features(X, tt).contiguous()
    bins_d = bin_features(X.to(cuda), tt).contiguous()
    assert torch.equal(bins_d.cpu(), bins)
    y32 = y.to(torch.int32)
    w = G.round_weights(3, 0, N_FIT, 0.8, "cpu")
    w_d = G.round_weights(3, 0, N_FIT, 0.8, cuda)
    assert torch.equal(w_d.cpu(), w)
    md = margins.clone().to(cuda)
    qgh_d, _ = G.grad_native(md, y32.to(cuda), w_d)
    a_d = G.GBTArrays.alloc(K_FIT, D_FIT, K_FIT, cuda)
    node_d = G.grow_round(bins_d, nbins.to(cuda), thr.to(cuda), qgh_d, w_d, a_d, 0, D_FIT, 32, 1.0, 0.1, 1, 0.0)
    G.update(md, node_d, a_d, 0)
    torch.cuda.synchronize()
    # the oracle grows the round from the DEVICE's quantized derivatives
    qgh = qgh_d.cpu()
    a = G.GBTArrays.alloc(K_FIT, D_FIT, K_FIT, "cpu")
    node = G.grow_round(bins, nbins, thr, qgh, w, a, 0, D_FIT, 32, 1.0, 0.1, 1, 0.0)
    mc = G.update(margins.clone(), node, a, 0)
    for name in ("feature", "split_bin", "left", "right", "thresh"):
        assert torch.equal(getattr(a_d, name).cpu(), getattr(a, name)), name
    assert int((a.feature >= 0).sum()) >= K_FIT * 7  # the trees did grow
    assert torch.equal(node_d.cpu(), node)
    torch.testing.assert_close(a_d.value.cpu(), a.value, rtol=1e-6, atol=0)
    torch.testing.assert_close(a_d.stats.cpu(), a.stats, rtol=1e-6, atol=0)
    torch.testing.assert_close(md.cpu(), mc, rtol=1e-5, atol=0)


def test_fit_reproducible_and_loss_within_quantization_margin(cuda, problem, cpu_fit):
    """The device may differ from the oracle only by +-1 quantum in a derivative.  m = 3 x the largest relative
    change of the oracle's final training loss over 5 fits whose every quantized derivative is perturbed by a
    random -1 / 0 / +1 quantum; the device's final loss must be <= the oracle's x (1 + m)."""
    X, y, tt = problem
    Xd, yd = X.to(cuda), y.to(cuda)
    a = _est().fit_tensors(Xd, yd, K_FIT, thresholds=tt)
    b = _est().fit_tensors(Xd, yd, K_FIT, thresholds=tt)
    for name in ("feature", "threshold", "left", "right", "stats", "gain"):
        assert torch.equal(getattr(a.arrs, name), getattr(b.arrs, name)), name
    assert a.trainLossHistory == b.trainLossHistory and len(a.trainLossHistory) == 11
    base = cpu_fit.trainLossHistory[-1]
    spreads = []
    for s in range(5):
        g = _gen(500 + s)

        def hook(rnd, q, g=g):
            return q + torch.randint(-1, 2, q.shape, generator=g, dtype=torch.int32)

        pert = _est()._fit_tensors(X, y, K_FIT, thresholds=tt, q_hook=hook)
        spreads.append(abs(pert.trainLossHistory[-1] - base) / base)
    m = 3 * max(spreads)
    diff = (a.trainLossHistory[-1] - base) / base
    print(f"gbt fit: oracle loss {base:.9f}, device loss {a.trainLossHistory[-1]:.9f}, relative difference {diff:.3e}, "
          f"largest perturbed spread {max(spreads):.3e}, m {m:.3e}")
    assert a.trainLossHistory[-1] <= base * (1 + m)
    assert a.trainLossHistory[-1] < a.trainLossHistory[0]


def test_predict_all_equals_forest_oracle(cuda):
    """Margins: elementwise rtol 1e-5 against the torch forest oracle, on the problem of tests/test_gbt.py whose
    oracle margins stay >= 0.5 away from zero (two fp32 summation orders of one margin cannot be asked to agree
    to a relative 1e-5 next to zero; the CPU suite guards that choice and the 2 % cap of the tie rule).
    Probabilities: a softmax moves by at most 2 max|dm| relatively, here 2 * 1e-5 * max|margin|, plus 1e-6
    for its own fp32 evaluation.  Classes: equal wherever the top two margins differ by more than 1e-4."""
    from test_gbt import PREDICT_SHAPE, predict_estimator, predict_problem

    X, y, tt = predict_problem()
    N, _, K = PREDICT_SHAPE
    model = predict_estimator().fit_tensors(X.to(cuda), y.to(cuda), K, thresholds=tt)
    raw, prob, pred = model.predict_all(X.to(cuda))
    assert model.getNumTrees == 60
    a = model.arrs.to("cpu")
    ref = T.forest_predict_torch(X, a.feature, a.threshold, a.left, a.right, a.stats, a.max_depth, normalize=False) \
        + model.init.cpu().view(1, -1)
    rel = ((raw.cpu() - ref).abs() / ref.abs()).max().item()
    print(f"gbt predict: largest elementwise relative margin error {rel:.3e}; |margin| in "
          f"[{ref.abs().min().item():.4f}, {ref.abs().max().item():.4f}]")
    torch.testing.assert_close(raw.cpu(), ref, rtol=1e-5, atol=0)
    torch.testing.assert_close(prob.cpu(), torch.softmax(ref, dim=1), rtol=2e-5 * ref.abs().max().item() + 1e-6, atol=0)
    top = ref.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-4
    excluded = int((~clear).sum())
    print(f"gbt predict: {excluded} of {N} rows excluded by the tie rule")
    assert excluded <= 0.02 * N
    assert torch.equal(pred.cpu()[clear], ref.argmax(dim=1)[clear])
    assert (pred.cpu() == y).double().mean() > 0.7


def test_cli_preset_gbt_on_the_device(cuda, tmp_path):
    """main.py --preset gbt on the GPU (its warm-up branch included), saved and loaded back on the device."""
    import main
    from har.features.raw import write_synthetic_raw
    from har.utils import persist

    p = str(tmp_path / "raw.csv")
    write_synthetic_raw(p, n_windows=120, users=4)
    mdir = tmp_path / "models"
    s = main.run(main.config_from_args(["--raw", p, "--out-dir", str(tmp_path / "out"), "--device", "cuda:0", "--preset",
                                        "gbt", "--gbt-max-iter", "5", "--gbt-max-depth", "3", "--save-models", str(mdir)]))
    assert set(s["models"]) == {"gbt"} and s["models"]["gbt"]["accuracy"] > 0.5
    assert "device_warmup" in s["phases_s"]
    m = persist.load(str(mdir / "gbt"), device=cuda)
    assert m.getNumTrees % 5 == 0 and m.arrs.feature.is_cuda and len(m.trainLossHistory) == 6
    assert m.trainLossHistory[-1] < m.trainLossHistory[0]
