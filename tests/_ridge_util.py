"""Fixtures and bounds shared by tests/test_ridge.py and tests/test_gpu_ridge.py."""
import functools

import numpy as np
import torch

from _kmeans_util import blobs, gen
from har.ops import ridge as RD

R = RD.R
EXACT_D = (1, 15, 16, 17, 63, 64, 65, 130)
EXACT_K = (2, 6)
EXACT_N = (1, R - 1, R, R + 1, 3 * R + 5)
EXACT_F = (1, 2, 5)
FIT_ALPHAS = (100.0, 3000.0, 30000.0, 100000.0)   # spread so that the folds' correct counts differ clearly
FIT_CASES = (43, 130)
EXCLUDED_CAP = 0.02


def gamma(n: int, u: float) -> float:
    return n * u / (1.0 - n * u)


GAMMA_R = gamma(R, 2.0 ** -24)       # the standard bound of an R-term fp32 chain


def fold_sizes(N: int, F: int):
    """Sizes with one empty fold, one fold of a single row and sizes straddling R, as far as N rows allow."""
    if F == 1:
        return [N]
    if F == 2:
        return [min(N, R + 1), N - min(N, R + 1)]
    want = [0, 1, R - 1, R + 1]
    out, left = [], N
    for w in want:
        w = min(w, left)
        out.append(w)
        left -= w
    return out + [left]


def exact_case(D: int, K: int, N: int, F: int):
    """Integer rows (|x| <= 7), integer means, power-of-two scales: every chain and every fp64 sum is exact.  The
    row list is a random permutation cut by ``fold_sizes``."""
    g = gen(7919 * D + 31 * K + 3 * N + F)
    X = torch.randint(-7, 8, (N, D), generator=g).float()
    y = torch.randint(0, K, (N,), generator=g).to(torch.int32)
    mean = torch.randint(-2, 3, (D,), generator=g).float()
    inv_std = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (D,), generator=g)]
    rows = torch.randperm(N, generator=g).to(torch.int32)
    off = [0] + [int(v) for v in np.cumsum(fold_sizes(N, F))]
    return X, y, rows, off, mean, inv_std


def real_case(D=65, K=6, N=3 * R + 5, F=2, seed=5):
    g = gen(seed)
    X = (torch.randn(N, D, generator=g) * 3.0 + 1.5).contiguous()
    y = torch.randint(0, K, (N,), generator=g).to(torch.int32)
    mean, inv_std = RD.standardizer(X)
    rows = torch.randperm(N, generator=g).to(torch.int32)
    off = [0, N // 3, N] if F == 2 else [0, N]
    return X, y, rows, off, mean, inv_std


def chain_bound(X, y, rows, off, mean, inv_std, K):
    """(fp64 moments of the same fp32 rows, gamma_R * sum |a_i a_j|) per fold [F, Dq, Dq]."""
    Af, _ = RD.moments_torch(X, y, rows, off, mean, inv_std, K, chain="fp64")
    A = RD.augment(RD.working_rows(X, mean, inv_std), y, K).double().abs()
    B = torch.stack([A[rows[off[f]:off[f + 1]].long()].T @ A[rows[off[f]:off[f + 1]].long()] for f in range(len(off) - 1)])
    return Af, GAMMA_R * B


def spd_batch(D: int, K: int, batch: int, seed: int = 0):
    """Random ``Z^T Z + alpha I`` in fp64 with condition numbers up to about 1e8 and a random border, as the
    [batch, ldn, ldn] image of ``ridge_cholesky`` (lower triangle, border rows D .. D + K - 1), plus (M, Bc)."""
    g = gen(100 * D + K + seed)
    ldn = RD.up64(D + K)
    Sys = torch.zeros(batch, ldn, ldn, dtype=torch.float64)
    Ms, Bs = [], []
    for s in range(batch):
        scale = torch.logspace(0, -4.0 * s / max(batch - 1, 1) if batch > 1 else -4.0, D, dtype=torch.float64)
        Z = torch.randn(2 * D + 3, D, generator=g, dtype=torch.float64) * scale
        M = Z.T @ Z + 1e-9 * torch.eye(D, dtype=torch.float64)
        Bc = torch.randn(D, K, generator=g, dtype=torch.float64)
        Sys[s, :D, :D] = torch.tril(M)
        Sys[s, D:D + K, :D] = Bc.T
        Ms.append(M)
        Bs.append(Bc)
    return Sys, torch.stack(Ms), torch.stack(Bs)


@functools.lru_cache(maxsize=None)
def fit_case(D: int):
    """Blob classes (N = 2,000, K = 6, F = 5, four alphas; close enough that the penalty matters): the inputs,
    the fp64 oracle, the oracle on the chunked fp32 chains, and the tolerance 10 x their difference (W, b)."""
    X, y, _ = blobs(N=2000, D=D, comps=6, seed=11 + D, spread=0.25)
    K, F = 6, 5
    fold = torch.randint(0, F, (2000,), generator=gen(D)).numpy()
    mean, inv_std = RD.standardizer(X)
    o64 = RD.fit_torch(X, y, fold, F, list(FIT_ALPHAS), mean, inv_std, K, chain="fp64")
    o32 = RD.fit_torch(X, y, fold, F, list(FIT_ALPHAS), mean, inv_std, K, chain="fp32")
    diff = max(float((o64.W64 - o32.W64).abs().max()), float((o64.b_all.double() - o32.b_all.double()).abs().max()))
    # never below one fp32 rounding of the largest coefficient: W and b are stored in fp32
    tol = 10.0 * max(diff, 2.0 ** -24 * max(float(o64.W64.abs().max()), float(o64.b_all.abs().max())))
    return {"X": X, "y": y, "fold": fold, "F": F, "K": K, "mean": mean, "inv_std": inv_std, "o64": o64, "o32": o32,
            "diff": diff, "tol": tol}


def oracle_gaps(case):
    """Per (row, alpha): the oracle's top-two decision gap and |raw|_max under the row's own fold's model."""
    o, X, fold, F = case["o64"], case["X"], case["fold"], case["F"]
    A, N = len(FIT_ALPHAS), X.shape[0]
    Z = RD.working_rows(X, case["mean"], case["inv_std"]).double()
    raw = torch.einsum("nd,skd->nsk", Z, o.W64[:F * A]) + o.b_all[:F * A].double().unsqueeze(0)
    raw = raw.view(N, F, A, -1).gather(1, torch.as_tensor(fold).long().view(N, 1, 1, 1).expand(N, 1, A, raw.shape[-1]))
    raw = raw.squeeze(1)
    top = raw.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1], raw.abs().max(dim=-1).values


def excluded_rows(case):
    """bool [N, A]: rows whose oracle gap is below tol (1 + |raw|)."""
    gap, mag = oracle_gaps(case)
    return gap < case["tol"] * (1.0 + mag)
