"""Shapes, data and the derived tie rule shared by tests/test_kmeans.py and tests/test_gpu_kmeans.py."""
import torch

from har.ops import kmeans as KM

CHUNK = 256  # kmeans.hip rows per workgroup (test_gpu_kmeans.py checks it against the library)

# (N, D, K): a covering subset of N in {1, 15, 16, 17, 255, 257, chunk - 1, chunk + 1, 2 chunk + 1},
# D in {1, 3, 4, 5, 43, 64, 130}, K in {1, 2, 15, 16, 17, 33, 255, 256} (K <= N: the centres are K of the rows).
# D = 130 with K >= 255 takes two centre slabs; K (D + 2) * 8 > 48 KB takes the global-atomic accumulation.
ASSIGN_SHAPES = [
    (1, 1, 1), (1, 43, 1), (15, 3, 2), (15, 4, 15), (16, 5, 16), (17, 1, 17), (17, 64, 1),
    (CHUNK - 1, 43, 33), (CHUNK - 1, 130, 255), (CHUNK + 1, 3, 16), (CHUNK + 1, 64, 256), (CHUNK + 1, 43, 15),
    (CHUNK + 1, 130, 256), (2 * CHUNK + 1, 5, 33), (2 * CHUNK + 1, 130, 17), (2 * CHUNK + 1, 1, 2),
    (2 * CHUNK + 1, 43, 256), (2 * CHUNK + 1, 4, 255),
]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def mixture(N, D, seed, comps=5, spread=3.0):
    """Working rows (centred, fp32) of a Gaussian mixture and the component of every row."""
    g = gen(seed)
    mu = torch.randn(comps, D, generator=g) * spread
    c = torch.randint(0, comps, (N,), generator=g)
    X = mu[c] + torch.randn(N, D, generator=g)
    return (X - KM.column_means(X).view(1, D)).contiguous(), c


def centres_of(Xc, K, seed):
    idx = torch.randperm(Xc.shape[0], generator=gen(seed + 7))[:K]
    C = Xc[idx].clone().contiguous()
    return C, KM.center_h(C)


def assign_case(N, D, K):
    Xc, _ = mixture(N, D, 1000 * N + 10 * D + K)
    C, h = centres_of(Xc, K, N + D + K)
    return Xc, C, h


def tie_rule(Xc, C, h):
    """fp64 oracle with the derived tie rule.  A row is clear when its two smallest scores differ by more
    than 2 gamma m, gamma = 2 (D + 4) 2^-24, m = the larger over those two centres of sum_f |x_f c_f| + h[k]
    (the order-independent dot-product bound, doubled: the matrix core's internal order and rounding are
    unspecified).  Returns (assign int32, clear bool, d2 fp64, atol = 2 gamma m fp64)."""
    N, D = Xc.shape
    K = C.shape[0]
    s = KM.scores_torch(Xc, C, h)
    mm = Xc.double().abs() @ C.double().abs().t() + h.double().view(1, K)
    gamma = 2.0 * (D + 4) * 2.0 ** -24
    a = s.argmin(dim=1)
    if K >= 2:
        v, i = s.topk(2, dim=1, largest=False)
        m = mm.gather(1, i).max(dim=1).values
        clear = (v[:, 1] - v[:, 0]) > 2.0 * gamma * m
    else:
        m = mm[:, 0]
        clear = torch.ones(N, dtype=torch.bool)
    smin = s.gather(1, a.view(N, 1)).squeeze(1)
    d2 = (KM.row_norms(Xc) + 2.0 * smin).clamp_min(0.0)
    return a.to(torch.int32), clear, d2, 2.0 * gamma * m


def blobs(N=2000, D=43, comps=6, seed=11, spread=4.0):
    """A separated blob problem in the original (uncentred) coordinates and its labels."""
    g = gen(seed)
    mu = torch.randn(comps, D, generator=g) * spread + 2.0
    y = torch.randint(0, comps, (N,), generator=g)
    return (mu[y] + torch.randn(N, D, generator=g)).contiguous(), y, mu
