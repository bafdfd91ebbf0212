"""Edge shapes of the small ETL / evaluation reductions (stats.hip, metrics.hip, roc.hip, rng.hip)
against numpy / pure-Python oracles in fp64 or exact integers.

Tolerances.  Counts, minima, maxima, bins, confusion cells, value counts and Philox buckets are
exact.  A floating sum of n terms must lie within ``4 n 2^-52 sum|terms|`` of ``math.fsum`` of the
same terms — the bound of fp64 recursive summation in any order (n 2^-53 sum|terms| to first
order) with room for a rounding of each term; every term itself is formed from fp32 inputs by the
same IEEE operations in the oracle and in the kernel.  ROC / PR areas are compared with the CPU
curve of ``har.evaluation.metrics.binary_metrics`` at 1e-12: exact integer sums, or fp64 sums of
at most n terms each <= 1."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _bound(n, terms):
    return 4.0 * n * EPS * math.fsum(abs(t) for t in terms)


def _close_sum(got, terms, n, what):
    want = math.fsum(terms)
    assert abs(got - want) <= _bound(n, terms), f"{what}: {got!r} vs fsum {want!r} (bound {_bound(n, terms):.3g})"


# ------------------------------------------------------------------------------------ column_stats
def _stats_f32(X, n, ncols, w):
    """The fp32 kernel on the leading ``ncols`` columns of the row-major ``X [n, ld]``."""
    from har.ops import _native

    mod = _native.kernels()
    ws = torch.empty(max(1, mod.column_stats_workspace(n, ncols)), dtype=torch.float64, device=X.device)
    out = torch.full((5, ncols), float("nan"), dtype=torch.float64, device=X.device)
    mod.column_stats(X.data_ptr(), n, ncols, X.stride(0), _native.ptr(w), out.data_ptr(), ws.data_ptr(),
                     _native.stream_ptr())
    return out.cpu().numpy()


def _check_stats(got, x64, w64, ctr, n, what):
    """``got [5, C]`` vs the fsum oracle over ``x64 [n, C]`` (fp64 copies of the inputs)."""
    for c in range(x64.shape[1]):
        x = x64[:, c]
        ok = (w64 != 0) & ~np.isnan(x)
        xs, wsel = x[ok], w64[ok]
        assert got[0, c] == wsel.sum(), f"{what} col {c}: count"  # small integers: exact
        _close_sum(got[1, c], list(wsel * xs), n, f"{what} col {c}: sum")
        d = xs - ctr[c]
        _close_sum(got[2, c], list(wsel * d * d), n, f"{what} col {c}: sum of squares")
        assert got[3, c] == (xs.min() if xs.size else np.inf), f"{what} col {c}: min"
        assert got[4, c] == (xs.max() if xs.size else -np.inf), f"{what} col {c}: max"


@pytest.mark.parametrize("ncols", [1, 256, 257, 600])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_column_stats_f32_weighted_slice(cuda, n, ncols):
    """Integer row weights 0..3 (zero = row skipped), NaNs sprinkled, an all-NaN column, and the
    matrix a column slice (ld = ncols + 3) whose outside columns hold a poison value."""
    rng = np.random.default_rng(n * 1000 + ncols)
    ld = ncols + 3
    X = rng.standard_normal((n, ld)).astype(np.float32) * 10
    X[rng.random((n, ld)) < 0.05] = np.nan
    X[:, ncols:] = 1e30
    if ncols > 1:
        X[:, ncols - 1] = np.nan
    w = rng.integers(0, 4, n).astype(np.float32)
    got = _stats_f32(torch.from_numpy(X).to(cuda), n, ncols, torch.from_numpy(w).to(cuda))
    _check_stats(got, X[:, :ncols].astype(np.float64), w.astype(np.float64), np.zeros(ncols), n, f"n={n} C={ncols}")
    if ncols > 1:
        assert got[0, ncols - 1] == 0 and got[3, ncols - 1] == np.inf and got[4, ncols - 1] == -np.inf


def test_column_stats_f32_all_zero_weights_and_wrapper(cuda):
    from har.ops.stats import column_stats

    X = torch.randn(257, 5, device=cuda)
    st = column_stats(X, torch.zeros(257, device=cuda)).cpu().numpy()
    assert (st[0] == 0).all() and (st[1] == 0).all() and (st[2] == 0).all()
    assert (st[3] == np.inf).all() and (st[4] == -np.inf).all()
    # the wrapper on a column slice of a wider matrix (it may copy; the numbers are the slice's)
    wide = torch.randn(300, 9, device=cuda)
    got = column_stats(wide[:, 2:6]).cpu().numpy()
    x = wide[:, 2:6].cpu().numpy().astype(np.float64)
    _check_stats(got, x, np.ones(300), np.zeros(4), 300, "wrapper slice")


@pytest.mark.parametrize("ncols", [1, 256, 257, 600])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_column_stats_f64_planes_with_center(cuda, n, ncols):
    from har.data.device_ops import _stats_planes

    rng = np.random.default_rng(n * 7 + ncols)
    X = rng.standard_normal((ncols, n)) * 3 + 1e8 * (np.arange(ncols)[:, None] % 2)  # odd planes: offset 1e8
    X[rng.random((ncols, n)) < 0.05] = np.nan
    if ncols > 1:
        X[ncols - 1] = np.nan
    ctr = np.where(np.arange(ncols) % 2, 1e8, 0.25)
    Xd = torch.from_numpy(X).to(cuda)
    for center in (None, ctr):
        got = _stats_planes(Xd, None if center is None else torch.from_numpy(center).to(cuda)).cpu().numpy()
        _check_stats(got, X.T, np.ones(n), np.zeros(ncols) if center is None else center, n,
                     f"planes n={n} C={ncols} center={center is not None}")
    if ncols > 1:
        assert got[0, ncols - 1] == 0 and got[3, ncols - 1] == np.inf and got[4, ncols - 1] == -np.inf


def test_describe_offset_column_and_empty_column(cuda):
    """Offset 1e8, unit spread: the centred second moment (not sum x^2 - n mean^2, which would lose
    every digit) gives the sample stddev of a math.fsum oracle; a column without any value prints
    on the device what it prints on the host."""
    from har.data.device_ops import describe_device
    from har.data.table import Column, DeviceColumn, Table

    rng = np.random.default_rng(5)
    n = 513
    x = 1e8 + rng.standard_normal(n)
    col = DeviceColumn("x", "double", torch.from_numpy(x).to(cuda), None)
    cnt, mean, std, mn, mx = describe_device([col])
    m = math.fsum(x) / n
    assert cnt[0] == n and mn[0] == x.min() and mx[0] == x.max()
    assert abs(mean[0] - m) <= 4 * n * EPS * 1e8
    # the second pass centres on the mean the first pass returned: the oracle takes the same centre; the sum's
    # relative bound 4 n 2^-52 is halved by the square root, the division and the root add a rounding each
    ref = math.sqrt(math.fsum((v - mean[0]) ** 2 for v in x) / (n - 1))
    assert abs(std[0] - ref) <= (2 * n + 2) * EPS * ref
    assert abs(std[0] - np.std(x - 1e8, ddof=1)) < 1e-6  # and it IS the spread of the data
    empty = np.ones(4, dtype=bool)
    for kind, data in (("double", np.zeros(4)), ("long", np.zeros(4, dtype=np.int64))):
        host = Table([Column("e", kind, data, empty)]).describe()
        t = torch.from_numpy(data).to(cuda)
        dev = Table([DeviceColumn("e", kind, t, torch.from_numpy(empty).to(cuda))]).describe()
        assert dev == host, (kind, dev, host)
        assert host["e"][0] == "0"


# ------------------------------------------------------------------------------------ bin_features
@pytest.mark.parametrize("n", [1, 257])
def test_bin_features_threshold_edges(cuda, n):
    from har.ops import _native

    rng = np.random.default_rng(n)
    nthr = np.array([0, 1, 255], dtype=np.int32)
    F, maxb, ld = 3, 255, 5
    thr = np.full((F, maxb), np.nan, dtype=np.float32)  # (entries past nthr[f] are never read)
    thr[1, 0] = 0.5
    thr[2] = np.sort(rng.standard_normal(maxb).astype(np.float32))
    assert len(np.unique(thr[2])) == maxb
    X = np.full((n, ld), 7e7, dtype=np.float32)
    for f in range(F):
        t = thr[f, :nthr[f]]
        special = np.concatenate([t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)),
                                  np.array([np.inf, -np.inf, np.nan, 0.0, -0.0], dtype=np.float32)]).astype(np.float32)
        # +-inf, NaN and the zeros always; then thresholds, their neighbours and random values as n allows
        col = np.concatenate([special[-5:], rng.permutation(np.concatenate([special[:-5],
                                                                              rng.standard_normal(n).astype(np.float32)]))])
        X[:, f] = col[:n] if n > 1 else (t[:1] if t.size else special[-3:-2])
    Xd = torch.from_numpy(X).to(cuda)
    out = torch.full((F, n), 77, dtype=torch.uint8, device=cuda)
    thr_d, nthr_d = torch.from_numpy(thr).to(cuda), torch.from_numpy(nthr).to(cuda)
    _native.kernels().bin_features(Xd.data_ptr(), n, F, ld, thr_d.data_ptr(), maxb, nthr_d.data_ptr(), out.data_ptr(),
                                   _native.stream_ptr())
    got = out.cpu().numpy()
    for f in range(F):
        x = X[:, f]
        want = np.searchsorted(thr[f, :nthr[f]], x, "left")
        want[np.isnan(x)] = nthr[f]
        np.testing.assert_array_equal(got[f], want.astype(np.uint8), err_msg=f"feature {f}")


def test_bin_features_every_threshold_and_its_neighbours(cuda):
    """All 255 thresholds, each with the fp32 value just below and just above, in one column."""
    from har.ops import _native

    thr = np.sort(np.random.default_rng(3).standard_normal(255).astype(np.float32))
    x = np.concatenate([thr, np.nextafter(thr, np.float32(-np.inf)), np.nextafter(thr, np.float32(np.inf))])
    n = x.size
    Xd = torch.from_numpy(np.ascontiguousarray(x[:, None])).to(cuda)
    out = torch.empty(1, n, dtype=torch.uint8, device=cuda)
    thr_d, nthr_d = torch.from_numpy(thr).to(cuda), torch.tensor([255], dtype=torch.int32, device=cuda)
    _native.kernels().bin_features(Xd.data_ptr(), n, 1, 1, thr_d.data_ptr(), 255, nthr_d.data_ptr(), out.data_ptr(),
                                   _native.stream_ptr())
    np.testing.assert_array_equal(out.cpu().numpy()[0], np.searchsorted(thr, x, "left").astype(np.uint8))


# ------------------------------------------------------------------------------------ confusion matrices
@pytest.mark.parametrize("K", [1, 2, 64])
@pytest.mark.parametrize("n", [1, 256, 257])
def test_confusion_matrix_edges(cuda, n, K):
    from har.ops.metrics import confusion_matrix, confusion_matrix_batched

    rng = np.random.default_rng(n * 100 + K)
    y = rng.integers(0, K, n)
    p = rng.integers(0, K, n)
    want = np.bincount(y * K + p, minlength=K * K).reshape(K, K)
    yd, pd = torch.from_numpy(y).to(cuda), torch.from_numpy(p).to(cuda)
    assert np.array_equal(confusion_matrix(yd, pd, K).cpu().numpy(), want)
    # every row in one cell
    one = confusion_matrix(torch.full_like(yd, K - 1), torch.zeros_like(pd), K).cpu().numpy()
    assert one[K - 1, 0] == n and one.sum() == n
    # batched: a model whose mask selects nothing, one that selects everything, a random one; then B = 1
    P = rng.integers(0, K, (3, n))
    M = np.stack([np.zeros(n, bool), np.ones(n, bool), rng.random(n) < 0.5])
    for rows in ([0, 1, 2], [2]):
        got = confusion_matrix_batched(yd, torch.from_numpy(P[rows]).to(cuda), torch.from_numpy(M[rows]).to(cuda),
                                       K).cpu().numpy()
        for b, r in enumerate(rows):
            ref = np.bincount((y * K + P[r])[M[r]], minlength=K * K).reshape(K, K)
            assert np.array_equal(got[b], ref), (rows, r)


def test_confusion_matrix_refuses_65_classes(cuda):
    """K = 65 needs more LDS counters than the kernels have: both entry points raise, neither launches."""
    from har.ops.metrics import confusion_matrix, confusion_matrix_batched

    z = torch.zeros(8, dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError):
        confusion_matrix(z, z, 65)
    with pytest.raises(RuntimeError):
        confusion_matrix_batched(z, z.view(1, 8), torch.ones(1, 8, dtype=torch.bool, device=cuda), 65)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ value_counts
@pytest.mark.parametrize("n", [0, 1, 70000])
@pytest.mark.parametrize("V", [1, 1402, "max", "max+1"])
def test_value_counts_edges(cuda, n, V):
    """Codes -1 and >= V are ignored.  "max" is the largest vocabulary the launcher accepts (its
    LDS counters, from the device's own limit); one more goes through the device bincount."""
    from har.data.device_ops import value_counts, value_counts_max_v

    vmax = value_counts_max_v(cuda)
    assert 1402 <= vmax <= 32768
    V = vmax if V == "max" else vmax + 1 if V == "max+1" else V
    rng = np.random.default_rng(n + V)
    codes = rng.integers(-1, V + 3, n)
    if n > 1:
        codes[:4] = [-1, V, V - 1, 0]
    got = value_counts(torch.from_numpy(codes).to(cuda), V)
    ok = (codes >= 0) & (codes < V)
    want = np.bincount(codes[ok], minlength=V)
    assert got.dtype == np.int64 and np.array_equal(got, want)


# ------------------------------------------------------------------------------------ regression_moments
@pytest.mark.parametrize("n", [1, 257, 262145])
def test_regression_moments_fsum(cuda, n):
    from har.ops.metrics import regression_moments

    rng = np.random.default_rng(n)
    y = (rng.standard_normal(n) * 50 + 20).astype(np.float32)
    yh = (y + rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    cnt, se, ae, sy, syy = regression_moments(torch.from_numpy(y).to(cuda), torch.from_numpy(yh).to(cuda))
    a, d = y.astype(np.float64), y.astype(np.float64) - yh.astype(np.float64)
    assert cnt == n
    _close_sum(se, list(d * d), n, "sum of squared errors")
    _close_sum(ae, list(np.abs(d)), n, "sum of absolute errors")
    _close_sum(sy, list(a), n, "sum y")
    _close_sum(syy, list(a * a), n, "sum y^2")


# ------------------------------------------------------------------------------------ ROC / PR
def _roc_cases(n, rng):
    """(name, scores in descending sorted order) — the caller shuffles rows."""
    base = np.arange(n, 0, -1).astype(np.float32)  # distinct, descending, exact in fp32
    out = [("all one tie", np.zeros(n, dtype=np.float32))]
    s = base.copy()
    hi = min(n - 1, 4095)
    s[hi - 5:hi + 1] = s[hi - 5]
    out.append((f"tie group ends at {hi}", s))
    if n > 4096:
        s = base.copy()
        s[4096:min(n, 4101)] = s[4096]
        out.append(("tie group starts at 4096", s))
        s = base.copy()
        s[4090:min(n, 4100)] = s[4090]
        out.append(("tie group straddles 4095|4096", s))
    s = base.copy()
    s[:3] = np.inf
    s[-3:] = -np.inf
    out.append(("+inf and -inf scores", s))
    return out


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8192])
def test_roc_pr_auc_streaming_boundary(cuda, n):
    from har.evaluation import metrics as M
    from har.ops.metrics import roc_pr_auc

    rng = np.random.default_rng(n)
    cases = [(name, s, (rng.random(n) < 0.3).astype(np.float32)) for name, s in _roc_cases(n, rng)]
    # all positives inside one tie group (rows 100..139 of the sorted order share a score)
    s = np.arange(n, 0, -1).astype(np.float32)
    s[100:140] = s[100]
    y = np.zeros(n, dtype=np.float32)
    y[105:130] = 1
    cases.append(("all positives in one tie group", s, y))
    for name, s, y in cases:
        perm = rng.permutation(n)
        st, yt = torch.from_numpy(s[perm]), torch.from_numpy(y[perm])
        ref = M.binary_metrics(st, yt)  # CPU fp64 curve
        auroc, aupr = roc_pr_auc(st.to(cuda), yt.to(cuda))
        assert abs(auroc - ref["areaUnderROC"]) <= 1e-12, (n, name, auroc, ref)
        assert abs(aupr - ref["areaUnderPR"]) <= 1e-12, (n, name, aupr, ref)


@pytest.mark.parametrize("B", [1, 3])
def test_roc_pr_auc_batched_empty_and_full_models(cuda, B):
    from har.evaluation import metrics as M
    from har.ops.metrics import roc_pr_auc_batched

    N = 4097
    rng = np.random.default_rng(B)
    score = np.round(rng.standard_normal((3, N)) * 20).astype(np.float32) / 20  # ties
    label = (rng.random(N) < 0.4).astype(np.float32)
    mask = np.stack([np.ones(N, bool), np.zeros(N, bool), rng.random(N) < 0.5])
    rows = [0, 1, 2] if B == 3 else [0]
    roc, pr = roc_pr_auc_batched(torch.from_numpy(score[rows]).to(cuda), torch.from_numpy(label).to(cuda),
                                 torch.from_numpy(mask[rows]).to(cuda))
    for b, r in enumerate(rows):
        ref = M.binary_metrics(torch.from_numpy(score[r][mask[r]]), torch.from_numpy(label[mask[r]]))
        assert abs(roc[b] - ref["areaUnderROC"]) <= 1e-12, (r, roc[b], ref)
        assert abs(pr[b] - ref["areaUnderPR"]) <= 1e-12, (r, pr[b], ref)


# ------------------------------------------------------------------------------------ philox_buckets
def _buckets(cuda, seed, stream, row0, n, thr):
    from har.ops import _native

    t = torch.from_numpy(np.asarray(thr if len(thr) else [0], dtype=np.uint32).view(np.int32).copy()).to(cuda)
    out = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    _native.kernels().philox_buckets(seed, stream, row0, n, t.data_ptr(), len(thr), out.data_ptr(),
                                     _native.stream_ptr())
    return out.cpu().numpy()


def _buckets_cpu(seed, stream, row0, n, thr):
    from har.ops import rng as R

    u = R.uniform_u32(seed, stream, np.arange(row0, row0 + n, dtype=np.uint64)).astype(np.uint64)
    return np.searchsorted(np.asarray(thr, dtype=np.uint64), u, side="right").astype(np.int32)


THR3 = [1 << 30, 3 << 30, 0xF0000000]


def test_philox_buckets_equal_cpu_philox(cuda):
    seed, stream = 0x1234_5678_9ABC_DEF1, 7
    np.testing.assert_array_equal(_buckets(cuda, seed, stream, 0, 1000, THR3), _buckets_cpu(seed, stream, 0, 1000, THR3))
    assert (_buckets(cuda, seed, stream, 0, 1000, []) == 0).all()            # no thresholds: one bucket
    assert (_buckets(cuda, seed, stream, 0, 1000, [0]) == 1).all()           # 0 <= u always
    np.testing.assert_array_equal(_buckets(cuda, seed, stream, 0, 1000, [0xFFFFFFFF]),
                                  _buckets_cpu(seed, stream, 0, 1000, [0xFFFFFFFF]))
    n = 4096 * 256 + 257  # more rows than the grid has lanes: the grid-stride loop runs
    np.testing.assert_array_equal(_buckets(cuda, seed, stream, 0, n, THR3), _buckets_cpu(seed, stream, 0, n, THR3))


@pytest.mark.parametrize("a", [1, 255, 2 ** 32 - 3])
def test_philox_buckets_window_property(cuda, a):
    """A shard's draw is the slice of the global draw: buckets(row0 = a, n) == buckets(a0, a - a0 + n)[a - a0:]
    with a0 = 0 for the small offsets; 2^32 - 3 (its rows cross the low counter word) starts its
    enclosing window 300 rows earlier, and is compared with the CPU Philox as well."""
    seed, stream, n = 2018, 1, 600
    a0 = 0 if a < 2 ** 31 else a - 300
    win = _buckets(cuda, seed, stream, a0, a - a0 + n, THR3)
    got = _buckets(cuda, seed, stream, a, n, THR3)
    np.testing.assert_array_equal(got, win[a - a0:])
    np.testing.assert_array_equal(got, _buckets_cpu(seed, stream, a, n, THR3))
    assert len(np.unique(got)) == 4
