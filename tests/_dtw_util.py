"""Shared data of the DTW tests: exact-arithmetic windows, brute-force path enumeration, the pulse problem."""
import numpy as np
import torch

from har.data.table import Column, Table

AMAX = 8   # integer windows in [-AMAX, AMAX]: (2 W - 1) * A * (2 AMAX)^2 < 2^24 for every W <= 200, A <= 9


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def integer_windows(n, W, A, seed, amax=AMAX, lo=None):
    lo = -amax if lo is None else lo
    return torch.randint(lo, amax + 1, (n, W, A), generator=gen(seed)).float()


def real_windows(n, W, A, seed, scale=1.0):
    return (torch.randn(n, W, A, generator=gen(seed)) * scale).float().contiguous()


def groups(n, m, seed, ngroups=5):
    g = gen(seed)
    qg = torch.randint(-1, ngroups, (n,), generator=g).to(torch.int32)
    rg = torch.randint(-1, ngroups, (m,), generator=g).to(torch.int32)
    return qg, rg


def brute_force(q, r, radius):
    """The minimum over EVERY admissible warping path of the summed cell costs, in Python floats."""
    W, A = q.shape
    c = [[sum((float(q[i, a]) - float(r[j, a])) ** 2 for a in range(A)) for j in range(W)] for i in range(W)]
    best = [float("inf")]

    def walk(i, j, acc):
        if abs(i - j) > radius:
            return
        acc += c[i][j]
        if i == W - 1 and j == W - 1:
            best[0] = min(best[0], acc)
            return
        if i + 1 < W:
            walk(i + 1, j, acc)
        if j + 1 < W:
            walk(i, j + 1, acc)
        if i + 1 < W and j + 1 < W:
            walk(i + 1, j + 1, acc)

    walk(0, 0, 0.0)
    return best[0]


def pulse_problem(n_per_class, classes, W, R, seed, A=1):
    """Class c is an integer pulse of height c + 1 with zero margins of R samples; instances are shifts by at
    most R // 2.  Same-class DTW costs at radius R are 0, other-class costs > 0."""
    g = gen(seed)
    width = W - 2 * R - 2 * (R // 2) - 2
    assert width >= 2
    X = torch.zeros(n_per_class * classes, W, A)
    y = torch.zeros(n_per_class * classes, dtype=torch.int64)
    for t in range(n_per_class * classes):
        c = t % classes
        s = int(torch.randint(-(R // 2), R // 2 + 1, (1,), generator=g))
        lo = R + R // 2 + 1 + s
        X[t, lo:lo + width, :] = float(c + 1)
        y[t] = c
    return X, y


def table_of(X, y, extra=None):
    cols = [Column("features", "vector", X.reshape(X.shape[0], -1).double().numpy()),
            Column("label", "double", y.numpy().astype(np.float64))]
    for name, v in (extra or {}).items():
        cols.append(Column(name, "int", np.asarray(v, dtype=np.int64)))
    return Table(cols)


def rank_consistency(idx, d2, cost64, gamma, qg=None, rg=None):
    """Every row of the lists against the fp64 costs: (largest |d2 - cost| / (gamma cost) over the listed pairs,
    rows where an unlisted admissible pair lies below d2_k / (1 + gamma))."""
    N, M = cost64.shape
    adm = torch.ones(N, M, dtype=torch.bool)
    if qg is not None:
        adm = ~((qg.long().view(-1, 1) >= 0) & (qg.long().view(-1, 1) == rg.long().view(1, -1)))
    worst, bad = 0.0, 0
    for n in range(N):
        listed = idx[n][idx[n] >= 0].long()
        assert len(set(listed.tolist())) == listed.numel() and bool(adm[n, listed].all())
        assert listed.numel() == min(idx.shape[1], int(adm[n].sum()))
        c = cost64[n, listed]
        err = (d2[n, :listed.numel()].double() - c).abs()
        rel = err / (gamma * c).clamp_min(1e-300)
        worst = max(worst, float(rel.max()) if rel.numel() else 0.0)
        assert bool((d2[n, 1:listed.numel()] >= d2[n, :listed.numel() - 1]).all())
        rest = adm[n].clone()
        rest[listed] = False
        if listed.numel() and bool(rest.any()):
            bad += int((cost64[n][rest] < float(d2[n, listed.numel() - 1]) / (1 + gamma)).any())
    return worst, bad
