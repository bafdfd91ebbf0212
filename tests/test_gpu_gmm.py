"""The Gaussian-mixture kernels (csrc/kernels/gmm.hip) against their PyTorch definitions in har/ops/gmm.py.

The Mahalanobis products run on the fp32 matrix cores, so q is compared with the fp64 oracle under the
derived, order-independent bound of tests/_gmm_util.py; everything downstream is compared with the fp64
evaluation of the kernel's OWN upstream output, so every stage is held to its own arithmetic."""
import pytest
import torch

from _gmm_util import (ESTEP_SHAPES, MOMENT_SHAPES, R, U, clear_rows, em_history, gen, moment_bounds, operands_case,
                       q_reference, row_weights, softmax_reference)
from _kmeans_util import blobs
from har.models.gmm import GaussianMixture, GaussianMixtureModel
from har.ops import gmm as GM

pytestmark = pytest.mark.gpu


def _dev(cuda, *ts):
    return [None if t is None else t.to(cuda) for t in ts]


def test_rows_per_block_and_grid(cuda):
    assert GM.rows_per_block() == R
    assert GM.grid(1, 43, 6) == 1 and GM.grid(5 * R + 1, 43, 6) == 6 and GM.grid(5 * R + 1, 43, 6, 2) == 2
    # the slab buffer does not grow with N
    assert GM.grid(10 ** 6, 43, 16) == GM.grid(10 ** 8, 43, 16) <= 512
    assert GM.grid(10 ** 6, 128, 64) * 64 * GM.slab_size(128) * 4 <= 256 << 20
    # all accumulators in LDS (one pass over the rows) / component groups (one pass per group)
    assert GM.group(43, 6) == 6 and GM.group(43, 16) == 16 and GM.group(5, 17) == 17
    assert GM.group(128, 3) == 1 and 1 <= GM.group(43, 64) < 64 and GM.group(128, 64) == 1


# ------------------------------------------------------------------ E-step
@pytest.mark.parametrize("N,D,K", ESTEP_SHAPES)
def test_estep_against_fp64_oracle(cuda, N, D, K):
    Z, mu, W, c = operands_case(N, D, K)
    q_ref, bound = q_reference(Z, mu, W)
    pred_ref, clear = clear_rows(q_ref, bound, c)
    e = GM.estep_native(*_dev(cuda, Z, mu, W, c), want_moments=False, want_q=True)
    torch.cuda.synchronize()
    q, r, lse, pred = e.q.cpu(), e.resp.cpu(), e.lse.cpu(), e.pred.cpu()
    # q: the derived bound
    err = (q.double() - q_ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    excluded = 1.0 - clear.double().mean().item()
    print(f"gmm_estep N={N} D={D} K={K}: worst q error / bound {worst:.4f}, excluded share {excluded:.6f}")
    assert bool((err <= bound).all())
    # the epilogue: the fp64 softmax of the kernel's own q
    t, lse_ref, r_ref = softmax_reference(q, c)
    tol = 8.0 * U * (t.abs().max(dim=1).values + 1.0)
    assert bool(((lse.double() - lse_ref).abs() <= tol).all())
    big = r_ref >= 2.0 ** -100
    dlog = (torch.log(r.double().clamp_min(1e-300)) - torch.log(r_ref.clamp_min(1e-300))).abs()
    assert bool((dlog[big] <= tol.view(-1, 1).expand_as(dlog)[big]).all())
    assert bool((r[~big] <= 2.0 ** -99).all())
    assert bool(((r.double().sum(dim=1) - 1.0).abs() <= 4 * 2.0 ** -23).all())     # 4 ulp of 1
    assert torch.equal(pred, r.argmax(dim=1).to(torch.int32))                      # the first argmax of its own r
    # the prediction against the oracle on clear rows; the excluded share is a condition (test_gmm.py)
    assert excluded <= 0.01
    assert torch.equal(pred[clear], pred_ref[clear])
    # the log-likelihood partials
    torch.testing.assert_close(e.loglik.cpu(), lse.double().sum(), rtol=1e-12, atol=1e-12)


def test_exact_ties_zero_weights_and_guards(cuda):
    Z, mu, W, c = operands_case(3 * R + 5, 43, 8, seed=77)
    # duplicates 8 and 16 apart (K = 17 crosses a 16-column tile): the lower index wins
    idx = list(range(8)) + list(range(8)) + [0]
    mu2, W2, c2 = mu[idx].contiguous(), W[idx].contiguous(), c[idx].contiguous()
    e = GM.estep_native(*_dev(cuda, Z, mu2, W2, c2), want_moments=False)
    ref = GM.estep_native(*_dev(cuda, Z, mu, W, c), want_moments=False)
    assert int(e.pred.max()) < 8 and torch.equal(e.pred, ref.pred)
    # zero-weight components are never predicted and get r = 0
    c3 = c.clone()
    c3[[0, 5]] = float("-inf")
    e = GM.estep_native(*_dev(cuda, Z, mu, W, c3), want_moments=False)
    assert not bool(((e.pred == 0) | (e.pred == 5)).any())
    assert float(e.resp[:, [0, 5]].abs().max()) == 0.0 and bool(torch.isfinite(e.lse).all())
    # guard buffers: outputs written inside NaN / -7 filled buffers leave the guards untouched
    N, D, K = 2 * R + 1, 5, 3
    Z, mu, W, c = operands_case(N, D, K)
    mod = GM._native.kernels()
    G, pad = GM.grid(N, D, K), 64
    bufs = {"resp": (N * K, torch.float32), "lse": (N, torch.float32), "pred": (N, torch.int32), "q": (N * K, torch.float32),
            "slabs": (G * K * GM.slab_size(D), torch.float32), "part": (G, torch.float64)}
    t = {}
    for name, (n, dt) in bufs.items():
        fill = -7 if dt == torch.int32 else float("nan")
        t[name] = torch.full((n + 2 * pad,), fill, dtype=dt, device=cuda)
    Zc, muc, Wc, cc = _dev(cuda, Z, mu, W, c)
    ptr = lambda name: t[name][pad:].data_ptr()
    mod.gmm_estep(Zc.data_ptr(), N, D, K, muc.data_ptr(), Wc.data_ptr(), cc.data_ptr(), 0, ptr("resp"), ptr("lse"),
                  ptr("pred"), ptr("q"), ptr("slabs"), ptr("part"), 0, 0, 1, 0, GM._native.stream_ptr())
    torch.cuda.synchronize()
    for name, (n, dt) in bufs.items():
        v = t[name].cpu()
        edge = torch.cat([v[:pad], v[pad + n:]])
        assert bool((edge == -7).all() if dt == torch.int32 else torch.isnan(edge).all()), name
        if name != "slabs":      # (a slab keeps unwritten words below its S2 diagonal)
            assert bool((v[pad:pad + n] != -7).all() if dt == torch.int32 else torch.isfinite(v[pad:pad + n]).all()), name
    plain = GM.estep_native(Zc, muc, Wc, cc, want_q=True)
    assert torch.equal(plain.resp.view(-1), t["resp"][pad:pad + N * K]) and torch.equal(plain.pred, t["pred"][pad:pad + N])


def test_contract_codes(cuda):
    mod = GM._native.kernels()
    Z, mu, W, c = _dev(cuda, *operands_case(10, 4, 2))
    s = GM._native.stream_ptr()
    with pytest.raises(RuntimeError, match="-4"):
        mod.gmm_estep(0, 10, 4, 2, mu.data_ptr(), W.data_ptr(), c.data_ptr(), 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, s)
    for D, K in ((129, 2), (4, 65), (0, 2), (4, 0)):
        with pytest.raises(RuntimeError, match="-2"):
            mod.gmm_estep(Z.data_ptr(), 10, D, K, mu.data_ptr(), W.data_ptr(), c.data_ptr(), 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, s)
    with pytest.raises(RuntimeError, match="-4"):
        mod.gmm_finish(0, 1, 2, 4, 0, 1, 0.0, mu.data_ptr(), W.data_ptr(), c.data_ptr(), 0, 0, 0, s)
    with pytest.raises(RuntimeError, match="-4"):
        mod.gmm_control(0, 1, 1, 0.0, 0, 0, s)
    with pytest.raises(ValueError):
        GM.estep_native(torch.zeros(4, 129, device=cuda), torch.zeros(2, 129, device=cuda),
                        torch.zeros(2, 129, 129, device=cuda), torch.zeros(2, device=cuda))


# ------------------------------------------------------------------ moments
@pytest.mark.parametrize("N,D,K,weighted,max_blocks", MOMENT_SHAPES)
def test_moments_against_fp64_oracle(cuda, N, D, K, weighted, max_blocks):
    Z, mu, W, c = operands_case(N, D, K)
    w = row_weights(N, N + D) if weighted else None
    e = GM.estep_native(*_dev(cuda, Z, mu, W, c, w), max_blocks=max_blocks)
    torch.cuda.synchronize()
    G = e.slabs.shape[0]
    assert G == (max_blocks or -(-N // R)) and e.part.numel() == G
    r = e.resp.cpu()
    Nk, S1, S2 = GM.reduce_slabs(e.slabs.cpu(), K, D)
    Nk_ref, S1_ref, S2_ref = GM.moments_torch(Z, mu, r, w)
    bN, b1, b2 = moment_bounds(Z, mu, r, w)
    for name, got, ref, b in (("N_k", Nk, Nk_ref, bN), ("S1", S1, S1_ref, b1), ("S2", S2, S2_ref, b2)):
        err = (got - ref).abs()
        print(f"gmm moments N={N} D={D} K={K} G={G} {name}: worst error / bound "
              f"{(err / b.clamp_min(1e-300)).max().item():.4f}")
        assert bool((err <= b).all()), name
    wl = e.lse.cpu().double() if w is None else e.lse.cpu().double() * w.double()
    torch.testing.assert_close(e.loglik.cpu(), wl.sum(), rtol=1e-12, atol=1e-12)
    again = GM.estep_native(*_dev(cuda, Z, mu, W, c, w), max_blocks=max_blocks)
    assert torch.equal(GM.reduce_slabs(again.slabs, K, D)[2], GM.reduce_slabs(e.slabs, K, D)[2])
    assert torch.equal(again.part, e.part)


# ------------------------------------------------------------------ finish
def _finish_case(D, K, seed, diag=False, empty=None, rank_deficient=False):
    g = gen(seed)
    N = 40 * D + 50
    Z = torch.randn(N, D, generator=g) @ (torch.randn(D, D, generator=g) * 0.3 + torch.eye(D))
    if rank_deficient:
        Z[:, -1] = Z[:, 0]
    mu = Z[:K].clone()
    r = torch.softmax(torch.randn(N, K, generator=g), dim=1)
    if empty is not None:
        r[:, empty] = 0.0
    Nk, S1, S2 = GM.moments_torch(Z, mu, r)
    W = torch.triu(torch.randn(K, D, D, generator=g) * 0.1, 1) + torch.diag_embed(0.5 + torch.rand(K, D, generator=g))
    return GM.make_slabs(Nk, S1, S2, 3), mu.contiguous(), W.contiguous()


def _residual(Wm, Sigma):
    D = Sigma.shape[-1]
    return torch.linalg.matrix_norm(Wm.transpose(-1, -2) @ Sigma @ Wm - torch.eye(D, dtype=torch.float64))


@pytest.mark.parametrize("D,K,diag,empty,rank_def,reg", [
    (1, 3, False, None, False, 1e-6), (5, 4, False, None, False, 1e-6), (43, 6, False, None, False, 1e-6),
    (128, 2, False, None, False, 1e-6), (43, 3, True, None, False, 1e-6), (5, 4, False, 2, False, 1e-6),
    (5, 2, False, None, True, 1e-3)])
def test_finish_against_fp64_oracle(cuda, D, K, diag, empty, rank_def, reg):
    slabs, mu, W = _finish_case(D, K, 31 * D + K, diag, empty, rank_def)
    ref = GM.finish_torch(*GM.reduce_slabs(slabs, K, D), mu, W, reg, diag)
    mu_d, W_d, slabs_d = _dev(cuda, mu.clone(), W.clone(), slabs)
    c_d = torch.zeros(K, device=cuda)
    Nk_d, pi_d = torch.zeros(K, dtype=torch.float64, device=cuda), torch.zeros(K, dtype=torch.float64, device=cuda)
    GM.finish_native(slabs_d, mu_d, W_d, c_d, Nk_d, pi_d, reg, diag)
    torch.cuda.synchronize()
    torch.testing.assert_close(pi_d.cpu(), ref.pi, rtol=1e-6, atol=0)
    torch.testing.assert_close(Nk_d.cpu(), ref.Nk, rtol=1e-12, atol=0)
    assert bool(ref.updated.all()) == (empty is None)
    torch.testing.assert_close(mu_d.cpu(), ref.mu, rtol=1e-6, atol=0)
    torch.testing.assert_close(c_d.cpu(), ref.c, rtol=1e-6, atol=0)
    for k in range(K):
        if not bool(ref.updated[k]):
            assert torch.equal(W_d.cpu()[k], W[k]) and torch.equal(mu_d.cpu()[k], mu[k]) and float(pi_d[k]) == 0.0
            assert float(c_d[k]) == float("-inf")
            continue
        Wk = W_d.cpu()[k]
        assert float(torch.tril(Wk, -1).abs().sum()) == 0.0
        got = _residual(Wk.double(), ref.Sigma[k]).item()
        own = _residual(ref.W64[k].float().double(), ref.Sigma[k]).item()
        print(f"gmm_finish D={D} k={k} diag={diag}: residual {got:.3e}, the oracle's rounded W {own:.3e}")
        assert got <= 4.0 * own + 1e-12


# ------------------------------------------------------------------ fit
@pytest.fixture(scope="module")
def blob_problem():
    return blobs(2000, 43, 6)


def test_fit_against_fp64_definitions(cuda, blob_problem):
    X, _, _ = blob_problem
    init = X[:6].clone()        # six of the rows (two share a blob): EM needs all 8 iterations
    est = GaussianMixture(k=6, maxIter=8, tol=0.0, device=cuda)
    model = est._fit_tensors(X.to(cuda), initial_means=init)
    mean, std, inv = GM.standardizer(X)
    Z = GM.working_rows(X, mean, inv)
    mu0 = ((init - mean) * inv).contiguous()
    h64, st64 = em_history(Z, mu0, 8)
    h32, _ = em_history(Z, mu0, 8, dtype=torch.float32)
    yard = ((h32 - h64).abs() / h64.abs()).max().item()
    hist = torch.tensor(model.summary.logLikelihoodHistory, dtype=torch.float64)
    got = ((hist - h64).abs() / h64.abs()).max().item()
    print(f"gmm fit: device vs fp64 history {got:.3e}, fp32 vs fp64 definitions on the CPU {yard:.3e}")
    assert model.summary.numIter == 8 and hist.numel() == 8
    assert bool(((hist - h64).abs() <= 10.0 * yard * h64.abs()).all())
    assert float((model._mu.cpu() - st64.mu).abs().max()) <= 1e-4
    # two device fits are bitwise equal
    est2 = GaussianMixture(k=6, maxIter=8, tol=0.0, device=cuda)
    again = est2._fit_tensors(X.to(cuda), initial_means=init)
    assert torch.equal(again._mu, model._mu) and torch.equal(again._W, model._W) and torch.equal(again._c, model._c)
    assert again.summary.logLikelihoodHistory == model.summary.logLikelihoodHistory
    assert again.summary.logLikelihood == model.summary.logLikelihood


def _fit_setup(cuda, X, mu_true, M):
    mean, std, inv = GM.standardizer(X)
    Z = GM.working_rows(X, mean, inv).to(cuda)
    K, D = mu_true.shape
    pi0 = torch.full((K,), 1.0 / K, dtype=torch.float64)
    st = GM.FitState.alloc(((mu_true - mean) * inv).to(cuda), torch.eye(D).expand(K, D, D).to(cuda),
                           GM.component_c(pi0, torch.zeros(K, dtype=torch.float64), D).to(cuda), pi0.to(cuda), M)
    G = GM.grid(Z.shape[0], D, K)
    return Z, st, torch.empty(G, K, GM.slab_size(D), device=cuda), torch.zeros(G, dtype=torch.float64, device=cuda)


def test_fit_loop_issues_no_host_read(cuda, blob_problem):
    X, _, _ = blob_problem
    Z, st, slabs, part = _fit_setup(cuda, X, X[:6].clone(), 8)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # a synchronizing call (any device -> host read) raises
    try:
        for _ in range(8):
            GM.step_native(st, Z, None, 1e-6, False, 0.0, 8, slabs, part)
        GM.estep_native(Z, st.mu, st.W, st.c, None, slabs_out=slabs, part_out=part)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert st.state.tolist() == [8, 0] and bool(torch.isfinite(st.hist).all())


def test_converged_fit_leaves_the_state_untouched(cuda, blob_problem):
    X, _, mu_true = blob_problem
    Z, st, slabs, part = _fit_setup(cuda, X, mu_true, 8)
    for _ in range(2):
        GM.step_native(st, Z, None, 1e-6, False, 1e12, 8, slabs, part)    # any change is within this tol
    assert st.state.tolist() == [2, 1]
    keep = [t.clone() for t in (st.mu, st.W, st.c, st.Nk, st.pi, st.hist, st.state)]
    for _ in range(3):
        GM.step_native(st, Z, None, 1e-6, False, 1e12, 8, slabs, part)
    for a, b in zip(keep, (st.mu, st.W, st.c, st.Nk, st.pi, st.hist, st.state)):
        assert torch.equal(a, b)
    assert float(st.hist[2:].abs().max()) == 0.0
    # maxIter stops the same way
    Z, st, slabs, part = _fit_setup(cuda, X, mu_true, 2)
    for _ in range(4):
        GM.step_native(st, Z, None, 1e-6, False, 0.0, 2, slabs, part)
    assert st.state.tolist() == [2, 0]


# ------------------------------------------------------------------ end to end
def test_end_to_end_from_a_device_table(cuda, blob_problem, tmp_path):
    from har.data.table import Column, Table
    from har.evaluation.evaluators import ClusteringEvaluator
    from har.utils import persist

    X, y, _ = blob_problem
    t = Table([Column("features", "vector", X.double().numpy())])
    model = GaussianMixture(k=6, maxIter=10, seed=2, device=cuda).fit(t)
    out = model.transform(t)
    prob = torch.as_tensor(out["probability"].data)
    pred = torch.as_tensor(out["prediction"].data).long()
    assert prob.shape == (2000, 6) and torch.allclose(prob.sum(1), torch.ones(2000, dtype=torch.float64), atol=1e-6)
    assert torch.equal(pred, prob.argmax(dim=1))
    cm, _, purity = model.label_map(pred, y, 6)
    assert tuple(cm.shape) == (6, 6) and int(cm.sum()) == 2000 and 1.0 / 6.0 <= purity <= 1.0
    ll = model.score_samples(X.to(cuda))
    cpu = persist.load(_saved(model, tmp_path), device="cpu")
    torch.testing.assert_close(ll.cpu(), cpu.score_samples(X), rtol=0, atol=1e-3)
    from har.ops import kmeans as KM

    sil = ClusteringEvaluator(device=cuda).evaluate(out)
    assert sil == pytest.approx(float(KM.silhouette(X, pred, 6, native=False)), rel=1e-5)
    back = persist.load(str(tmp_path / "gmm"), device=cuda)
    assert isinstance(back, GaussianMixtureModel) and torch.equal(back.predict(X.to(cuda)), model.predict(X.to(cuda)))
    assert back.majority_labels == model.majority_labels


def _saved(model, tmp_path):
    from har.utils import persist

    persist.save(model, str(tmp_path / "gmm"))
    return str(tmp_path / "gmm")
