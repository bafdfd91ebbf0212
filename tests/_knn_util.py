"""Shapes, data and the derived rank-consistency bound shared by tests/test_knn.py and tests/test_gpu_knn.py."""
import numpy as np
import torch

from _kmeans_util import gen, mixture
from har.data.table import Column, Table
from har.ops import kmeans as KM
from har.ops import knn as KN

# (N, D, M, k) of the real-valued accuracy test: the five shapes the rank-consistency rule was derived on, a
# one-feature shape and one whose k equals M
RANK_SHAPES = [(65, 3, 2000, 16), (300, 43, 3793, 10), (257, 43, 1000, 32), (64, 130, 513, 64), (129, 43, 4097, 64),
               (17, 1, 40, 5), (63, 5, 64, 64)]

# (N, D, k, M code, grouped) of the exact test; the M codes are placed around the library's slab size s:
# N in {1, 15, 16, 17, 63, 64, 65, 129}, M in {1, 15, 17, s - 1, s, s + 1, 2 s + 1, >= 3 automatic splits},
# D in {1, 3, 4, 5, 43, 130, 256}, k in {1, 2, 5, 16, 17, 64}; k > M and k > the admissible count included
EXACT_SHAPES = [
    (1, 1, 1, "1", False), (15, 3, 2, "15", True), (16, 4, 5, "17", False), (17, 5, 16, "15", True),
    (63, 43, 17, "s-1", False), (64, 43, 64, "s", True), (65, 130, 5, "s+1", False), (129, 256, 16, "2s+1", True),
    (17, 43, 5, "auto3", True), (129, 1, 64, "17", False), (65, 3, 64, "2s+1", False), (16, 130, 64, "s", True),
    (64, 256, 2, "s-1", False), (1, 5, 1, "s+1", True), (63, 4, 17, "1", False), (20, 4, 16, "17", True),
]


def m_of(code: str, slab: int) -> int:
    return {"1": 1, "15": 15, "17": 17, "s-1": slab - 1, "s": slab, "s+1": slab + 1, "2s+1": 2 * slab + 1,
            "auto3": 3 * slab + 5}[code]


def integer_case(N, D, M, seed, amax=8, groups=False, ngroups=3):
    """Integer-valued working rows (every product, sum and h is exact in fp32) and optional groups in
    {-1, 0, ..., ngroups - 1}."""
    g = gen(seed)
    Q = torch.randint(-amax, amax + 1, (N, D), generator=g).float().contiguous()
    R = torch.randint(-amax, amax + 1, (M, D), generator=g).float().contiguous()
    qg = rg = None
    if groups:
        qg = torch.randint(-1, ngroups, (N,), generator=g).to(torch.int32)
        rg = torch.randint(-1, ngroups, (M,), generator=g).to(torch.int32)
    return Q, R, KM.center_h(R), qg, rg


def real_case(N, D, M, seed, groups=False, ngroups=4):
    """Queries and references drawn from ONE Gaussian mixture (``_kmeans_util.mixture``)."""
    X, _ = mixture(N + M, D, seed)
    Q, R = X[:N].contiguous(), X[N:].contiguous()
    qg = rg = None
    if groups:
        g = gen(seed + 1)
        qg = torch.randint(-1, ngroups, (N,), generator=g).to(torch.int32)
        rg = torch.randint(-1, ngroups, (M,), generator=g).to(torch.int32)
    return Q, R, KM.center_h(R), qg, rg


def python_neighbors(Q, R, h, k, qg=None, rg=None):
    """The definition as a plain Python sort of (score, index) pairs (fp64 scores; exact on integer rows)."""
    N, M = Q.shape[0], R.shape[0]
    S = KN.scores_torch(Q, R, h).tolist()
    idx, sc = [], []
    for n in range(N):
        pairs = sorted((S[n][m], m) for m in range(M)
                       if not (qg is not None and int(qg[n]) >= 0 and int(qg[n]) == int(rg[m])))[:k]
        idx.append([p[1] for p in pairs] + [-1] * (k - len(pairs)))
        sc.append([p[0] for p in pairs] + [float("inf")] * (k - len(pairs)))
    return torch.tensor(idx, dtype=torch.int32).view(N, k), torch.tensor(sc, dtype=torch.float64).view(N, k)


def tau(Q, R, h):
    """fp64 [N]: 2 gamma max_m (sum_f |q_f r_f| + h[m]), gamma = 2 (D + 4) 2^-24 — the order-independent
    dot-product bound, doubled as in ``_kmeans_util.tie_rule`` (the matrix core's internal order and rounding
    are unspecified)."""
    D = Q.shape[1]
    gamma = 2.0 * (D + 4) * 2.0 ** -24
    mm = Q.double().abs() @ R.double().abs().t() + h.double().view(1, -1)
    return 2.0 * gamma * mm.max(dim=1).values


def near_tie_share(S, k, t):
    """The share of rows whose first k + 1 oracle scores have an adjacent gap inside the bound."""
    v = torch.sort(S, dim=1).values[:, :k + 1]
    gap = v[:, 1:] - v[:, :-1]
    return float(((gap <= t.view(-1, 1)) & torch.isfinite(v[:, 1:])).any(dim=1).double().mean())


def rank_consistency(idx, d2, Q, R, h, k, qg=None, rg=None):
    """The four requirements on a kernel's lists for real-valued rows; returns the largest error / bound.
    (a) indices valid, distinct, admissible, and as many as there are admissible references (up to k);
    (b) S[n, idx_i] <= S_(k) + tau_n; (c) S[n, idx_{i+1}] >= S[n, idx_i] - tau_n; (d) d2 non-decreasing and
    within 2 tau_n + 2^-22 d2 of the oracle's d2 of that pair."""
    N, M = Q.shape[0], R.shape[0]
    S = KN.scores_torch(Q, R, h, qg, rg)
    t = tau(Q, R, h).view(N, 1)
    idx, d2 = idx.long(), d2.double()
    valid = idx >= 0
    adm = torch.isfinite(S).sum(dim=1)
    # (a)
    assert int(idx.max()) < M and int(idx.min()) >= -1
    assert torch.equal(valid.sum(dim=1), adm.clamp_max(k)), "every admissible reference up to k is listed"
    assert bool((valid[:, :-1] | ~valid[:, 1:]).all()), "the missing entries are the tail"
    srt = torch.sort(torch.where(valid, idx, -1 - torch.arange(k).view(1, k).expand(N, k)), dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "distinct"
    Sg = S.gather(1, idx.clamp_min(0))
    assert bool(torch.isfinite(Sg[valid]).all()), "admissible"
    # (b)
    kth = torch.sort(S, dim=1).values[:, min(k, M) - 1].view(N, 1)
    kth = torch.where(torch.isfinite(kth), kth, torch.full_like(kth, float("inf")))
    eb = torch.where(valid & torch.isfinite(kth), (Sg - kth) / t, torch.zeros_like(Sg))
    # (c)
    both = valid[:, 1:] & valid[:, :-1]
    ec = torch.where(both, (Sg[:, :-1] - Sg[:, 1:]) / t, torch.zeros_like(Sg[:, 1:]))
    # (d)
    assert bool((d2[:, 1:] >= d2[:, :-1]).all()), "d2 non-decreasing"
    assert bool(torch.isinf(d2[~valid]).all())
    ref = (KM.row_norms(Q).view(N, 1) + 2.0 * Sg).clamp_min(0.0).float().double()
    ed = torch.where(valid, (d2 - ref).abs() / (2.0 * t + 2.0 ** -22 * ref), torch.zeros_like(ref))
    worst = max(float(eb.max()), float(ec.max()) if ec.numel() else 0.0, float(ed.max()))
    return worst, S, t.view(N)


def table_of(X, y, extra=None):
    cols = [Column("features", "vector", X.double().numpy()), Column("label", "double", y.double().numpy())]
    for name, v in (extra or {}).items():
        cols.append(Column(name, "double", np.asarray(v, dtype=np.float64)))
    return Table(cols)
