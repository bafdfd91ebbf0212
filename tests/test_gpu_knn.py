"""The k-nearest-neighbour kernels (csrc/kernels/knn.hip) against their PyTorch definitions in har/ops/knn.py.

Integer-valued rows make every product, sum and h exact in fp32: there the lists must EQUAL the oracle, ties
included.  Real-valued rows are held to the rank-consistency bound of tests/_knn_util.py, which holds for
every row (an exact-order rule would have to exclude up to all rows: see ``near_tie_share``), and to the
invariances that follow from the (score, index) order: runs, reference splits, query batches, k prefixes.

Measured on an MI355X (largest error / bound of ``test_rank_consistency_real_valued``): see PARITY.md."""
import pytest
import torch

from _kmeans_util import blobs, gen, mixture
from _knn_util import EXACT_SHAPES, RANK_SHAPES, integer_case, m_of, rank_consistency, real_case, table_of
from har.evaluation.evaluators import MulticlassClassificationEvaluator
from har.models.knn import KNNClassifier
from har.ops import kmeans as KM
from har.ops import knn as KN
from har.tuning.crossval import CrossValidator, ParamGridBuilder

pytestmark = pytest.mark.gpu


def _dev(cuda, *ts):
    return [None if t is None else t.to(cuda) for t in ts]


def _native(cuda, Q, R, h, k, qg=None, rg=None, **kw):
    Qd, Rd, hd, qgd, rgd = _dev(cuda, Q, R, h, qg, rg)
    idx, d2 = KN.neighbors_native(Qd, Rd, hd, k, qgd, rgd, **kw)
    return idx.cpu(), d2.cpu()


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("N,D,k,mcode,grouped", EXACT_SHAPES)
def test_exact_on_integer_rows(cuda, N, D, k, mcode, grouped):
    slab = KN.slab_rows(D)
    M = m_of(mcode, slab)
    Q, R, h, qg, rg = integer_case(N, D, M, 100 * N + D + k, groups=grouped)
    if mcode == "auto3":
        assert KN.auto_splits(N, M, D) >= 3
    want_i, want_d = KN.neighbors_torch(Q, R, h, k, qg, rg)
    idx, d2 = _native(cuda, Q, R, h, k, qg, rg)
    if k > M or mcode == "17" and grouped:
        assert int((want_i < 0).sum()) > 0            # the padding rule is exercised
    assert torch.equal(idx, want_i)
    assert torch.equal(d2, want_d)


@pytest.mark.parametrize("grouped", [False, True])
def test_exact_dense_ties(cuda, grouped):
    Q, R, h, qg, rg = integer_case(65, 3, 500, 77, amax=2, groups=grouped)      # 125 distinct points: ties everywhere
    want_i, want_d = KN.neighbors_torch(Q, R, h, 16, qg, rg)
    for splits in (None, 1, 3):
        idx, d2 = _native(cuda, Q, R, h, 16, qg, rg, splits=splits)
        assert torch.equal(idx, want_i) and torch.equal(d2, want_d)


# ------------------------------------------------------------------ 2. duplicated references
def test_duplicated_references_keep_the_lower_index_first(cuda):
    M0 = 300
    Q, R0, _, _, _ = real_case(65, 43, M0, 5)
    R = torch.cat([R0, R0], 0).contiguous()
    idx, d2 = _native(cuda, Q, R, KM.center_h(R), 16)
    hi = idx >= M0
    assert int(hi.sum()) > 0 and not bool(hi[:, 0].any())
    prev = torch.roll(idx, 1, dims=1)
    assert torch.equal(prev[hi], idx[hi] - M0)          # equal bits: j + M0 sits right behind j
    assert torch.equal(torch.roll(d2, 1, dims=1)[hi], d2[hi])


# ------------------------------------------------------------------ 3. invariances
def test_invariances_real_valued(cuda):
    D = 43
    M = 7 * KN.slab_rows(D) + 1
    Q, R, h, qg, rg = real_case(129, D, M, 9, groups=True)
    base = _native(cuda, Q, R, h, 5, qg, rg)
    again = _native(cuda, Q, R, h, 5, qg, rg)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])
    for splits in (1, 2, 7):
        got = _native(cuda, Q, R, h, 5, qg, rg, splits=splits)
        assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1]), splits
    a = _native(cuda, Q[:50].contiguous(), R, h, 5, qg[:50].contiguous(), rg)
    b = _native(cuda, Q[50:].contiguous(), R, h, 5, qg[50:].contiguous(), rg)
    assert torch.equal(base[0], torch.cat([a[0], b[0]])) and torch.equal(base[1], torch.cat([a[1], b[1]]))
    big = _native(cuda, Q, R, h, 64, qg, rg)
    assert torch.equal(base[0], big[0][:, :5]) and torch.equal(base[1], big[1][:, :5])


# ------------------------------------------------------------------ 4. real-valued accuracy
@pytest.mark.parametrize("N,D,M,k", RANK_SHAPES)
def test_rank_consistency_real_valued(cuda, N, D, M, k):
    Q, R, h, qg, rg = real_case(N, D, M, 1000 * N + 10 * D + k, groups=(N % 2 == 1))
    idx, d2 = _native(cuda, Q, R, h, k, qg, rg)
    worst, _, _ = rank_consistency(idx, d2, Q, R, h, k, qg, rg)
    print(f"knn_search N={N} D={D} M={M} k={k}: largest error / tau {worst:.4f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ 5. vote
@pytest.mark.parametrize("C", [1, 2, 6, 17, 32])
def test_vote_against_fp64_definition_on_the_kernels_lists(cuda, C):
    k = 17
    Q, R, h, qg, rg = real_case(70, 43, 400, 40 + C, groups=True)
    y = torch.randint(0, C, (400,), generator=gen(C)).to(torch.int32)
    Qd, Rd, hd, qgd, rgd, yd = _dev(cuda, Q, R, h, qg, rg, y)
    for weights in ("uniform", "distance"):
        r = KN.search_native(Qd, Rd, hd, k, qgd, rgd, y=yd, C=C, weights=weights)
        idx, d2 = r.idx.cpu(), r.d2.cpu()
        want = KN.vote_torch(idx, d2, y, C, weights)
        alone = KN.vote_native(r.idx, r.d2, yd, C, weights)
        assert torch.equal(alone.raw, r.vote.raw) and torch.equal(alone.pred, r.vote.pred)
        raw, prob, pred = r.vote.raw.cpu(), r.vote.prob.cpu(), r.vote.pred.cpu()
        if weights == "uniform":
            assert torch.equal(raw, want.raw) and torch.equal(pred, want.pred)
        else:
            # positive terms, at most three roundings each (sqrt, divide, add) plus the sum's
            eps = 4.0 * (k + 4) * 2.0 ** -53
            assert bool(((raw - want.raw).abs() <= eps * want.raw).all())
            top = want.raw.topk(min(2, C), dim=1).values
            clear = torch.ones(70, dtype=torch.bool) if C == 1 else (top[:, 0] - top[:, 1]) > 2 * eps * top[:, 0]
            assert torch.equal(pred[clear], want.pred[clear])
        # the ratio of two such sums: both errors, the C adds of the total and the division
        torch.testing.assert_close(prob, want.prob, rtol=2 * 4.0 * (k + 4) * 2.0 ** -53 + (C + 1) * 2.0 ** -53, atol=0)
        # the prefix vote reads the first 5 entries of the wider lists
        pre = KN.vote_native(r.idx, r.d2, yd, C, weights, k=5)
        want5 = KN.vote_torch(idx[:, :5].contiguous(), d2[:, :5].contiguous(), y, C, weights)
        torch.testing.assert_close(pre.raw.cpu(), want5.raw, rtol=4.0 * 9 * 2.0 ** -53, atol=0)


def test_vote_zero_distance_and_padded_rows(cuda):
    C, k = 6, 5
    Q, R, h, _, _ = integer_case(40, 5, 30, 3, amax=3)
    Q[:12] = R[:12]                                              # exact zeros (and their duplicates)
    y = torch.randint(0, C, (30,), generator=gen(8)).to(torch.int32)
    qg = torch.full((40,), -1, dtype=torch.int32)
    qg[20:] = 0                                                  # rows 20..: only 3 admissible references
    rg = torch.zeros(30, dtype=torch.int32)
    rg[:3] = 1
    qg[39], rg2 = 1, rg.clone()
    Qd, Rd, hd, qgd, rgd, yd = _dev(cuda, Q, R, h, qg, rg2, y)
    for weights in ("uniform", "distance"):
        r = KN.search_native(Qd, Rd, hd, k, qgd, rgd, y=yd, C=C, weights=weights)
        idx, d2 = r.idx.cpu(), r.d2.cpu()
        wi, wd = KN.neighbors_torch(Q, R, h, k, qg, rg2)
        assert torch.equal(idx, wi) and torch.equal(d2, wd)
        assert int((d2[:12, 0] == 0).sum()) == 12 and int((idx[20:39, 3:] == -1).sum()) == 19 * 2
        want = KN.vote_torch(idx, d2, y, C, weights)
        torch.testing.assert_close(r.vote.raw.cpu(), want.raw, rtol=4.0 * (k + 4) * 2.0 ** -53, atol=0)
        if weights == "distance":                               # the zero rule: whole numbers only
            assert torch.equal(r.vote.raw.cpu()[:12], want.raw[:12]) and float(want.raw[:12].sum(1).min()) >= 1.0
        assert torch.equal(r.vote.pred.cpu(), want.pred)
    # no valid neighbour at all: uniform probability, class 0
    allq = torch.zeros(40, dtype=torch.int32)
    r = KN.search_native(Qd, Rd, hd, k, allq.to(cuda), torch.zeros(30, dtype=torch.int32, device=cuda), y=yd, C=C)
    assert int((r.idx != -1).sum()) == 0 and bool(torch.isinf(r.d2).all())
    assert torch.equal(r.vote.prob.cpu(), torch.full((40, C), 1.0 / C, dtype=torch.float64))
    assert int(r.vote.pred.abs().sum()) == 0 and float(r.vote.raw.abs().sum()) == 0.0


# ------------------------------------------------------------------ 6. end to end
@pytest.fixture(scope="module")
def blob_problem():
    return blobs(2000, 43, 6)


def test_classifier_matches_cpu_model(cuda, blob_problem):
    X, y, _ = blob_problem
    Xtr, ytr, Xte = X[:1400], y[:1400], X[1400:]
    cpu = KNNClassifier(k=5, device="cpu").fit_tensors(Xtr, ytr, 6)
    raw, _, pred = cpu.predict_all(Xte)
    top = raw.topk(2, dim=1).values
    assert int((top[:, 0] == top[:, 1]).sum()) == 0              # no tied vote in the oracle at this seed
    dev = KNNClassifier(k=5, device=cuda).fit_tensors(Xtr.to(cuda), ytr.to(cuda), 6)
    assert torch.equal(dev.predict(Xte.to(cuda)).cpu(), pred)


def test_crossvalidator_branch_matches_cpu(cuda, blob_problem):
    X, y, _ = blob_problem
    t = table_of(X[:600], y[:600])
    grid = ParamGridBuilder().addGrid("k", [1, 5, 9]).addGrid("weights", ["uniform", "distance"]).build()
    ev = MulticlassClassificationEvaluator(metricName="accuracy")
    out = {}
    for dev in ("cpu", cuda):
        cv = CrossValidator(KNNClassifier(device=dev), grid, ev, numFolds=3, seed=4).fit(t)
        out[str(dev)] = cv.avgMetrics
    # accuracies are exact counts over the fold sizes: the same counts, whatever rounds the division
    assert out["cpu"] == pytest.approx(out[str(cuda)], rel=0, abs=1e-12)
    assert max(out["cpu"]) > 0.9


def test_search_issues_no_host_read(cuda):
    Q, R, h, qg, rg = real_case(129, 43, 1000, 2, groups=True)
    y = torch.randint(0, 6, (1000,), generator=gen(1)).to(torch.int32)
    Qd, Rd, hd, qgd, rgd, yd = _dev(cuda, Q, R, h, qg, rg, y)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # a synchronizing call (any device -> host read) raises
    try:
        r = KN.search_native(Qd, Rd, hd, 10, qgd, rgd, y=yd, C=6, weights="distance")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(r.idx.max()) < 1000


# ------------------------------------------------------------------ 7. guards
def test_range_errors(cuda):
    Q, R, h, _, _ = integer_case(4, 3, 9, 1)
    Qd, Rd, hd = _dev(cuda, Q, R, h)
    for k in (0, 65):
        with pytest.raises(ValueError):
            KN.neighbors_native(Qd, Rd, hd, k)
    big = torch.zeros(4, 257, device=cuda)
    with pytest.raises(ValueError):
        KN.neighbors_native(big, big, torch.zeros(4, device=cuda), 2)
    y = torch.zeros(9, dtype=torch.int32, device=cuda)
    for C in (0, 33):
        with pytest.raises(ValueError):
            KN.search_native(Qd, Rd, hd, 2, y=y, C=C)
    with pytest.raises(ValueError):
        KN.search_native(Qd, Rd, hd, 2, y=y, C=3, weights="rank")
    with pytest.raises(ValueError):
        KN.neighbors_native(Qd, Rd, hd, 2, splits=0)
    with pytest.raises(ValueError):
        KN.neighbors_native(Qd, Rd, hd, 2, torch.zeros(4, dtype=torch.int32, device=cuda), None)


def test_outputs_stay_inside_their_cells(cuda):
    N, k = 65, 5
    Q, R, h, qg, rg = integer_case(N, 43, 300, 6, groups=True)
    Qd, Rd, hd, qgd, rgd = _dev(cuda, Q, R, h, qg, rg)
    pad = 97
    ibuf = torch.full((N * k + 2 * pad,), -7, dtype=torch.int32, device=cuda)
    dbuf = torch.full((N * k + 2 * pad,), float("nan"), dtype=torch.float32, device=cuda)
    iv, dv = ibuf[pad:pad + N * k].view(N, k), dbuf[pad:pad + N * k].view(N, k)
    KN.neighbors_native(Qd, Rd, hd, k, qgd, rgd, idx_out=iv, d2_out=dv)
    wi, wd = KN.neighbors_torch(Q, R, h, k, qg, rg)
    assert torch.equal(iv.cpu(), wi) and torch.equal(dv.cpu(), wd)
    assert bool((ibuf[:pad] == -7).all()) and bool((ibuf[pad + N * k:] == -7).all())
    assert bool(torch.isnan(dbuf[:pad]).all()) and bool(torch.isnan(dbuf[pad + N * k:]).all())
