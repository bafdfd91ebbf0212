"""The DTW kernels (csrc/kernels/dtw.hip) against their PyTorch definition in har/ops/dtw.py.

Integer-valued windows in [-8, 8] keep every fp32 sum an integer below 2^24 ((2 W - 1) * A * 16^2 <= 399 * 9 *
256 < 2^24), so costs and lists must EQUAL the fp64 oracle, ties included.  Real-valued windows are held to the
derived bound ``|dtw_fp32 - dtw| <= gamma dtw``, ``gamma = 2 (2 W + A + 2) 2^-24`` (every term is non-negative, a
cell carries at most A + 2 roundings, a path at most 2 W - 1 adds, ``min`` is monotone), every row of the lists
to rank consistency under it, and to the invariances that follow from the fixed operation sequence of a pair.

Measured on an MI355X (largest error / gamma of ``test_real_valued_bound_and_rank_consistency``): see PARITY.md."""
import numpy as np
import pytest
import torch

from _dtw_util import AMAX, groups, integer_windows, pulse_problem, rank_consistency, real_windows, table_of
from har.models.dtw import DTWClassifier
from har.ops import dtw as DT

pytestmark = pytest.mark.gpu

# (W, A, radius, N code, M code): N / M codes are offsets from the kernel's block sizes (None: one row).
# Every W of {1, 2, 3, 31, 64, 65, 200}, A of {1, 3, 6, 9}, radius of {0, 1, 7, 20, W - 1 capped at 64} and
# every block edge (-1, +0, +1) of both sizes occurs.
EXACT_CASES = [
    (1, 1, 0, None, None), (1, 3, 0, 0, 1), (2, 1, 1, -1, -1), (2, 9, 0, 1, 0), (3, 3, 2, 0, 0),
    (3, 6, 1, 1, 1), (31, 1, 7, -1, 1), (31, 3, 30, 0, -1), (31, 9, 20, 1, None), (64, 3, 63, None, 0),
    (64, 6, 7, 0, 1), (64, 1, 0, 1, -1), (65, 3, 64, -1, 0), (65, 9, 1, 0, None), (65, 1, 20, 1, 1),
    (200, 3, 20, 1, 1), (200, 1, 64, 0, -1), (200, 6, 7, -1, 0), (200, 9, 0, None, 1), (200, 3, 1, 0, 0),
    (31, 2, 12, 1, 1), (64, 4, 33, -1, 1),
]


def _rows(code, block):
    return 1 if code is None else block + code


def _dev(cuda, *ts):
    return [None if t is None else t.to(cuda) for t in ts]


@pytest.fixture(scope="module")
def real_case():
    """One real-valued problem and its fp64 costs, shared by the invariance and accuracy tests."""
    W, A, radius = 50, 3, 5
    Q, R = real_windows(37, W, A, 11), real_windows(301, W, A, 12)
    return Q, R, radius, DT.cost_torch(Q, R, radius)


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("W,A,radius,ncode,mcode", EXACT_CASES)
def test_cost_and_lists_exact_on_integer_windows(cuda, W, A, radius, ncode, mcode):
    assert (2 * W - 1) * A * (2 * AMAX) ** 2 < 2 ** 24
    N, M = _rows(ncode, DT.query_rows()), _rows(mcode, DT.slab_rows())
    Q, R = integer_windows(N, W, A, 1000 * W + 10 * A + radius), integer_windows(M, W, A, 7 + 1000 * W + 10 * A + radius)
    want = DT.cost_torch(Q, R, radius)
    Qd, Rd = _dev(cuda, Q, R)
    got = DT.cost_native(Qd, Rd, radius).cpu()
    assert torch.equal(got, want.float()) and torch.equal(got.double(), want)
    k = 5
    for grouped in (False, True):
        qg, rg = groups(N, M, W + A, ngroups=3) if grouped else (None, None)
        wi, wd = DT.neighbors_torch(Q, R, k, radius, qg, rg)
        idx, d2 = DT.neighbors_native(Qd, Rd, k, radius, *_dev(cuda, qg, rg))
        assert torch.equal(idx.cpu(), wi) and torch.equal(d2.cpu(), wd)


@pytest.mark.parametrize("grouped", [False, True])
def test_exact_dense_ties(cuda, grouped):
    N, M, W, k = 9, 150, 12, 16
    Q, R = integer_windows(N, W, 1, 5, amax=1, lo=0), integer_windows(M, W, 1, 6, amax=1, lo=0)
    qg, rg = groups(N, M, 3, ngroups=4) if grouped else (None, None)
    wi, wd = DT.neighbors_torch(Q, R, k, 2, qg, rg)
    assert int((wd[:, 1:] == wd[:, :-1]).sum()) > N                                # ties are dense
    for splits in (1, 3):
        idx, d2 = DT.neighbors_native(*_dev(cuda, Q, R), k, 2, *_dev(cuda, qg, rg), splits=splits)
        assert torch.equal(idx.cpu(), wi) and torch.equal(d2.cpu(), wd)


# ------------------------------------------------------------------ 2. invariances on real-valued data
def test_invariances(cuda, real_case):
    Q, R, radius, _ = real_case
    Qd, Rd = _dev(cuda, Q, R)
    i1, d1 = DT.neighbors_native(Qd, Rd, 16, radius, splits=1)
    iS, dS = DT.neighbors_native(Qd, Rd, 16, radius, splits=5)
    assert DT.auto_splits(Q.shape[0], R.shape[0]) > 1
    assert torch.equal(i1, iS) and torch.equal(d1, dS)                              # 1 split against many
    ia, da = DT.neighbors_native(Qd[:21].contiguous(), Rd, 16, radius)
    ib, db = DT.neighbors_native(Qd[21:].contiguous(), Rd, 16, radius)
    assert torch.equal(torch.cat([ia, ib]), i1) and torch.equal(torch.cat([da, db]), d1)   # query batches
    i5, d5 = DT.neighbors_native(Qd, Rd, 5, radius)
    assert torch.equal(i5, i1[:, :5]) and torch.equal(d5, d1[:, :5])                # k prefixes
    i2, d2 = DT.neighbors_native(Qd, Rd, 16, radius, splits=1)
    assert torch.equal(i2, i1) and torch.equal(d2, d1)                              # run against rerun
    cost = DT.cost_native(Qd, Rd, radius)
    assert torch.equal(cost, DT.cost_native(Qd, Rd, radius))
    qg, rg = groups(Q.shape[0], R.shape[0], 4)
    for g in ((None, None), (qg, rg)):
        li, ld = DT.lists_from_cost(cost.cpu(), 16, *g)
        si, sd = DT.neighbors_native(Qd, Rd, 16, radius, *_dev(cuda, *g))
        assert torch.equal(si.cpu(), li) and torch.equal(sd.cpu(), ld)              # search against sorted dtw_cost


# ------------------------------------------------------------------ 3. real-valued accuracy
@pytest.mark.parametrize("scale", [1.0, 1e3])
def test_real_valued_bound_and_rank_consistency(cuda, real_case, scale):
    Q, R, radius, c64 = real_case
    if scale != 1.0:
        Q, R = (Q * scale).contiguous(), (R * scale).contiguous()
        c64 = DT.cost_torch(Q, R, radius)
    gamma = DT.gamma(Q.shape[1], Q.shape[2])
    Qd, Rd = _dev(cuda, Q, R)
    got = DT.cost_native(Qd, Rd, radius).cpu().double()
    rel = ((got - c64).abs() / c64).max().item()
    print(f"dtw_cost scale {scale:g}: largest relative error {rel:.3e} = {rel / gamma:.4f} gamma (gamma {gamma:.3e})")
    assert bool(((got - c64).abs() <= gamma * c64).all())
    qg, rg = groups(Q.shape[0], R.shape[0], 4)
    for g in ((None, None), (qg, rg)):
        idx, d2 = DT.neighbors_native(Qd, Rd, 10, radius, *_dev(cuda, *g))
        worst, bad = rank_consistency(idx.cpu(), d2.cpu(), c64, gamma, *g)
        print(f"dtw_search scale {scale:g}: largest listed error {worst:.4f} gamma, {bad} inconsistent rows")
        assert worst <= 1.0 and bad == 0


# ------------------------------------------------------------------ 4. other checks
def test_outputs_stay_inside_their_buffers(cuda):
    N, M, W, A, k = 5, 70, 20, 3, 4
    Q, R = _dev(cuda, integer_windows(N, W, A, 1), integer_windows(M, W, A, 2))
    buf = torch.full((N + 2, M), float("nan"), device=cuda)
    DT.cost_native(Q, R, 3, out=buf[1:N + 1])
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[N + 1]).all())
    assert torch.equal(buf[1:N + 1].cpu().double(), DT.cost_torch(Q.cpu(), R.cpu(), 3))
    ib = torch.full((N + 2, k), -7, dtype=torch.int32, device=cuda)
    db = torch.full((N + 2, k), float("nan"), device=cuda)
    DT.neighbors_native(Q, R, k, 3, idx_out=ib[1:N + 1], d2_out=db[1:N + 1])
    assert bool((ib[0] == -7).all()) and bool((ib[N + 1] == -7).all())
    assert bool(torch.isnan(db[0]).all()) and bool(torch.isnan(db[N + 1]).all())
    wi, wd = DT.neighbors_torch(Q.cpu(), R.cpu(), k, 3)
    assert torch.equal(ib[1:N + 1].cpu(), wi) and torch.equal(db[1:N + 1].cpu(), wd)


def test_search_makes_no_host_read(cuda):
    Q, R = _dev(cuda, integer_windows(6, 20, 3, 1), integer_windows(130, 20, 3, 2))
    y = torch.randint(0, 3, (130,), dtype=torch.int32).to(cuda)
    DT.search_native(Q, R, 3, 2, y=y, C=3)                                          # code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = DT.search_native(Q, R, 3, 2, y=y, C=3, weights="distance", splits=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    w = DT.search_torch(Q.cpu(), R.cpu(), 3, 2, y=y.cpu(), C=3, weights="distance")
    assert torch.equal(r.idx.cpu(), w.idx) and torch.equal(r.vote.pred.cpu(), w.vote.pred)


def test_classifier_equals_cpu_model(cuda):
    from har.evaluation.evaluators import MulticlassClassificationEvaluator
    from har.tuning.crossval import CrossValidator, ParamGridBuilder

    X, y = pulse_problem(8, 3, 40, 4, 3)
    X = X + integer_windows(24, 40, 1, 8, amax=1)
    Xq = pulse_problem(5, 3, 40, 4, 9)[0] + integer_windows(15, 40, 1, 10, amax=1)
    t = table_of(X, y, {"USER": np.arange(24) % 4})
    out = {}
    for dev in ("cpu", cuda):
        est = DTWClassifier(k=3, radius=4, axes=1, weights="distance", device=dev)
        m = est.fit(t)
        raw, prob, pred = m.predict_all(Xq.reshape(15, -1).to(dev))
        grid = ParamGridBuilder().addGrid("k", [1, 3]).addGrid("weights", ["uniform", "distance"]).build()
        cv = CrossValidator(estimator=est, estimatorParamMaps=grid, evaluator=MulticlassClassificationEvaluator(
            metricName="accuracy"), numFolds=3, seed=7).fit(t)
        out[str(dev)] = (raw.cpu(), prob.cpu(), pred.cpu(), est.leave_group_out(t, "USER").cpu(),
                         torch.tensor(cv.avgMetrics))
    for a, b in zip(out["cpu"], out[str(cuda)]):
        assert torch.equal(a, b)


def test_range_errors_before_any_launch(cuda):
    Q, R = _dev(cuda, integer_windows(2, 8, 3, 1), integer_windows(3, 8, 3, 2))
    with pytest.raises(ValueError, match="k in"):
        DT.neighbors_native(Q, R, 65, 1)
    with pytest.raises(ValueError, match="W - 1"):
        DT.cost_native(Q, R, 8)
    with pytest.raises(ValueError, match="radius"):
        DT.cost(torch.zeros(1, 100, 1, device=cuda), torch.zeros(1, 100, 1, device=cuda), 65)
    with pytest.raises(ValueError, match="samples"):
        DT.cost(torch.zeros(1, 513, 1, device=cuda), torch.zeros(1, 513, 1, device=cuda), 0)
    with pytest.raises(ValueError, match="axes"):
        DT.cost(torch.zeros(1, 4, 10, device=cuda), torch.zeros(1, 4, 10, device=cuda), 0)
    with pytest.raises(ValueError, match="differ"):
        DT.cost(Q, torch.zeros(3, 9, 3, device=cuda), 1)
    with pytest.raises(ValueError, match="splits"):
        DT.neighbors_native(Q, R, 1, 1, splits=0)
    with pytest.raises(ValueError, match="fp32"):
        DT.cost_native(Q.double(), R.double(), 1)
    with pytest.raises(ValueError, match="classes"):
        DT.search(Q, R, 1, 1, y=torch.zeros(3, dtype=torch.int32, device=cuda), C=33)
    with pytest.raises(ValueError, match="weights"):
        DT.search(Q, R, 1, 1, y=torch.zeros(3, dtype=torch.int32, device=cuda), C=2, weights="gaussian")
