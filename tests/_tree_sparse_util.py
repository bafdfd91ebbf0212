"""Helpers shared by the one-hot-aware tree tests (tests/test_gpu_tree_sparse.py, tests/test_gpu_rccl.py): a
synthetic hybrid matrix, the dense-path switch and the bitwise forest comparison."""
import hashlib

import numpy as np
import torch

ARRAY_KEYS = ("feature", "threshold", "left", "right", "stats", "gain")


def dense_path(fn):
    """``fn()`` with the one-hot-aware path switched off (``ops.tree.SPARSE_TREES``)."""
    from har.ops import tree as T

    old = T.SPARSE_TREES
    T.SPARSE_TREES = False
    try:
        return fn()
    finally:
        T.SPARSE_TREES = old


def same_arrays(a, b):
    for k in ARRAY_KEYS:
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x, y), k
    assert np.array_equal(a.n_nodes, b.n_nodes)


def arrays_hash(a) -> str:
    """SHA-256 over the bytes of a ForestArrays (shapes included): equal hashes <-> ``same_arrays``."""
    h = hashlib.sha256()
    for k in ARRAY_KEYS:
        t = getattr(a, k).detach().cpu().contiguous()
        h.update(("%s%s%s" % (k, tuple(t.shape), t.dtype)).encode())
        h.update(t.numpy().tobytes())
    h.update(np.asarray(a.n_nodes, dtype=np.int64).tobytes())
    return h.hexdigest()


def synthetic_hybrid(cuda, N=24000, widths=(40, 7, 3), Fd=5, seed=0, all_ones_block=False):
    """A hybrid matrix with some one-hot columns absent (no 1 in any row), the last category dropped
    (-1 rows) and, optionally, a block whose first column is set in every row (no split)."""
    from har.features.hybrid import HybridMatrix

    g = torch.Generator().manual_seed(seed)
    blocks, off, cats = [], 0, []
    for i, w in enumerate(widths):
        c = torch.randint(-1, w - 2, (N,), generator=g)  # columns w-2, w-1 never set
        if all_ones_block and i == len(widths) - 1:
            c = torch.zeros(N, dtype=torch.int64)
        cats.append(torch.where(c >= 0, c + off, c).to(torch.int32))
        blocks.append((off, w))
        off += w
    dense = torch.randn(N, Fd, generator=g)
    dense[:, 0] = torch.randint(0, 4, (N,), generator=g).float()  # few distinct values: midpoints
    dense[::97, 1] = float("nan")
    dense_cols = torch.arange(off, off + Fd, dtype=torch.int32)
    hm = HybridMatrix(dense.to(cuda), dense_cols.to(cuda), torch.stack(cats, 1).contiguous().to(cuda), blocks, off + Fd)
    y = (cats[0] % 3 + (dense[:, 2] > 0).to(torch.int32)).long().clamp_max(3).to(cuda)
    return hm, y
