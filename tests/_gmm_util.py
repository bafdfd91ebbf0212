"""Shapes, synthetic operands and the derived bounds shared by tests/test_gmm.py and tests/test_gpu_gmm.py."""
import torch

from har.ops import gmm as GM

R = 64  # gmm.hip rows per tile (test_gpu_gmm.py checks it against the library)

# (N, D, K): a covering subset of N in {1, 15, 17, R - 1, R + 1, 2R + 1}, D in {1, 3, 4, 5, 43, 64, 128},
# K in {1, 2, 6, 17, 64} (K <= N: the means are K of the rows)
ESTEP_SHAPES = [
    (1, 1, 1), (1, 43, 1), (15, 3, 2), (15, 128, 6), (17, 4, 17), (17, 64, 2), (R - 1, 5, 6), (R - 1, 43, 17),
    (R - 1, 128, 2), (R + 1, 1, 64), (R + 1, 43, 6), (R + 1, 64, 64), (2 * R + 1, 3, 17), (2 * R + 1, 43, 64),
    (2 * R + 1, 128, 17), (2 * R + 1, 5, 1),
]
# (N, D, K, weighted, max_blocks)
MOMENT_SHAPES = [
    (2 * R + 1, 43, 6, True, 0), (2 * R + 1, 43, 6, False, 0), (R + 1, 5, 17, False, 0), (R - 1, 128, 3, False, 0),
    (5 * R + 1, 43, 6, True, 2),
    # component groups (the accumulators of all K do not fit the LDS): several passes over the tiles
    (3 * R + 1, 128, 3, True, 2), (2 * R + 1, 43, 64, False, 0),
]
U = 2.0 ** -24


def gen(seed):
    return torch.Generator().manual_seed(seed)


def operands_case(N, D, K, seed=None):
    """Synthetic (not fitted) operands: rows randn, mu = K of the rows, W_k upper triangular with a diagonal
    in [0.5, 2] and off-diagonal 0.3 randn / sqrt(D), c uniform in [-5, 0]."""
    g = gen(1000 * N + 10 * D + K if seed is None else seed)
    Z = torch.randn(N, D, generator=g)
    mu = Z[torch.randperm(N, generator=g)[:K]].clone().contiguous()
    W = torch.triu(0.3 * torch.randn(K, D, D, generator=g) / D ** 0.5, 1)
    W = W + torch.diag_embed(0.5 + 1.5 * torch.rand(K, D, generator=g))
    c = -5.0 * torch.rand(K, generator=g)
    return Z.contiguous(), mu, W.contiguous(), c


def row_weights(N, seed):
    """fp32 weights in [0, 2) with about a fifth of them zero."""
    g = gen(seed)
    w = 2.0 * torch.rand(N, generator=g)
    return torch.where(torch.rand(N, generator=g) < 0.2, torch.zeros(N), w).contiguous()


def q_reference(Z, mu, W):
    """(q fp64 [N, K], bound fp64 [N, K]): the oracle and the order-independent error bound of a matrix-core
    evaluation.  gamma = 2 (D + 4) 2^-24 (the doubled dot-product bound of tests/_kmeans_util.py),
    e_j = gamma sum_d (|z_d| + |mu_kd|) |W_k[d, j]| bounds the error of y_j (the fp32 subtract included),
    and |q - q_ref| <= sum_j (2 |y_j| e_j + e_j^2) + gamma q_ref."""
    N, D = Z.shape
    K = mu.shape[0]
    gamma = 2.0 * (D + 4) * U
    Zd = Z.double()
    q = torch.zeros(N, K, dtype=torch.float64)
    b = torch.zeros(N, K, dtype=torch.float64)
    for k in range(K):
        Wd = W[k].double()
        y = (Zd - mu[k].double().view(1, D)) @ Wd
        e = gamma * ((Zd.abs() + mu[k].double().abs().view(1, D)) @ Wd.abs())
        q[:, k] = (y * y).sum(dim=1)
        b[:, k] = (2.0 * y.abs() * e + e * e).sum(dim=1) + gamma * q[:, k]
    return q, b


def clear_rows(q, bound, c):
    """(pred int32 of the fp64 oracle, clear bool): a row is clear when the gap between its two largest t
    exceeds twice (the larger q bound of those two components / 2)."""
    t = c.double().view(1, -1) - 0.5 * q
    pred = t.argmax(dim=1).to(torch.int32)
    if t.shape[1] < 2:
        return pred, torch.ones(t.shape[0], dtype=torch.bool)
    v, i = t.topk(2, dim=1)
    tb = 0.5 * bound.gather(1, i).max(dim=1).values
    return pred, (v[:, 0] - v[:, 1]) > 2.0 * tb


def softmax_reference(q32, c):
    """fp64 (t, lse, r) of the kernel's own fp32 q and the fp32 c."""
    t = c.double().view(1, -1) - 0.5 * q32.double()
    lse = torch.logsumexp(t, dim=1)
    return t, lse, torch.exp(t - lse.view(-1, 1))


def moment_bounds(Z, mu, r, w):
    """Elementwise bounds 2 (N + 4) 2^-24 sum_n w r |.| of N_k, S1 and S2 (fp64)."""
    N, D = Z.shape
    K = mu.shape[0]
    g = 2.0 * (N + 4) * U
    wr = r.double() if w is None else r.double() * w.double().view(-1, 1)
    b1 = torch.zeros(K, D, dtype=torch.float64)
    b2 = torch.zeros(K, D, D, dtype=torch.float64)
    for k in range(K):
        ad = (Z.double() - mu[k].double().view(1, D)).abs()
        b1[k] = (ad * wr[:, k].view(-1, 1)).sum(dim=0)
        b2[k] = (ad * wr[:, k].view(-1, 1)).t() @ ad
    return g * wr.sum(dim=0), g * b1, g * b2


def em_history(Z, mu0, iters, reg=1e-6, diag=False, w=None, dtype=torch.float64):
    """The log-likelihood history (and the final state) of ``iters`` EM steps of the definitions from
    ``mu0`` (working coordinates), equal weights, identity covariances."""
    K, D = mu0.shape
    pi0 = torch.full((K,), 1.0 / K, dtype=torch.float64)
    st = GM.FitState.alloc(mu0, torch.eye(D).expand(K, D, D), GM.component_c(pi0, torch.zeros(K, dtype=torch.float64), D),
                           pi0, iters)
    for _ in range(iters):
        GM.step_torch(st, Z, w, reg, diag, 0.0, iters, dtype)
    return st.hist.clone(), st


def small_problem(N=513, D=5, K=3, seed=3):
    """A well-conditioned mixture problem (more than 40 rows per component per feature)."""
    g = gen(seed)
    mu = 3.0 * torch.randn(K, D, generator=g)
    A = torch.randn(K, D, D, generator=g) * 0.4 + torch.eye(D)
    y = torch.randint(0, K, (N,), generator=g)
    X = mu[y] + torch.einsum("nd,nde->ne", torch.randn(N, D, generator=g), A[y])
    return X.contiguous(), y, mu, A
