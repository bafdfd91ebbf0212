"""tree_level.hip kernel by kernel against the numpy oracle of tests/_tree_level_util.py (itself checked
against the CPU builder in tests/test_tree_level_oracle.py), then chained into a teacher-forced level loop.

Every input is dyadic with sums below 2^24, so every comparison is bit equality.  Every output and workspace
is prefilled — outputs with sentinels, workspaces with garbage — and each check compares the WHOLE buffer
with "oracle values where the kernel must write, the prefill everywhere else".  Count modes: "exact" passes
the level's candidate / split count by value; "bound" passes about twice the count as the array stride and
grid bound, and the kernels read the real count from a device int32 (what the level loop does when it runs
without host reads); whatever lies past the real count is then junk the kernels must not touch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _tree_level_util as L
from har.ops import _native

pytestmark = pytest.mark.gpu

MODES = ["exact", "bound"]
SENT = -7777777
SENT_F = np.array([0x7FC0BEEF], dtype=np.uint32).view(np.float32)[0]  # a NaN with a payload
_NP = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32}


def _call():
    return _native.kernels(), _native.stream_ptr()


def expect(shape, dtype):
    """The prefill of ``out`` as numpy: the test writes the oracle's values over the region the kernel owns."""
    return np.full(shape, SENT_F if dtype == torch.float32 else SENT, dtype=_NP[dtype])


def out(dev, shape, dtype=torch.int32):
    return torch.from_numpy(expect(shape, dtype)).to(dev)


def prefix(values, n, dtype):
    """[n] sentinels with ``values`` at the front."""
    e = expect(n, dtype)
    e[:len(values)] = values
    return e


def garbage(dev, n, dtype=torch.int32):
    g = torch.Generator().manual_seed(n)
    t = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    return (t.view(torch.float32) if dtype == torch.float32 else t).to(dev)


def dev_of(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def padded(dev, a, n, fill):
    """``a`` followed by ``fill`` up to n entries, on the device (junk past the real count)."""
    e = np.full(n, fill, dtype=a.dtype)
    e[:len(a)] = a
    return dev_of(dev, e)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def counted(dev, mode, n):
    """(bound or exact count, device pointer of the real count or 0, the tensor that keeps it alive)."""
    if mode == "exact":
        return n, 0, None
    t = torch.tensor([n], dtype=torch.int32, device=dev)
    return 2 * n + 1, t.data_ptr(), t


# ---- tree_root_frontier ----
@pytest.mark.parametrize("K", L.CLASS_COUNTS)
@pytest.mark.parametrize("Tn", L.ROOT_TN)
def test_root_frontier(cuda, Tn, K):
    """Per-thread ranges of 1, 2 and 3 trees and threads that own none; roots that are pure, empty, of weight
    exactly min2, just below it, and ordinary; tree_stride = 3 K with junk in the other nodes' stats."""
    mod, st = _call()
    for min2 in L.MIN2:
        c = L.root_case(Tn, K, min2)
        stats = dev_of(cuda, c.stats)
        stale = (500_000 + np.arange(Tn * c.maxn)).reshape(Tn, c.maxn).astype(np.int32)
        for imp in L.IMPURITIES:
            ct, cn, tlo, scal = out(cuda, Tn + 2), out(cuda, Tn + 2), out(cuda, Tn + 3), out(cuda, 6)
            ci = dev_of(cuda, stale)
            mod.tree_root_frontier(stats.data_ptr(), Tn, K, c.maxn * K, imp, float(min2), c.maxn, ct.data_ptr(),
                                   cn.data_ptr(), tlo.data_ptr(), ci.data_ptr(), scal.data_ptr(), st)
            w_ct, w_cn, w_tlo, col0, w_scal = L.root_frontier(c.stats[:, 0], imp, min2)
            what = f"Tn {Tn} K {K} min2 {min2} impurity {imp}"
            L.same(host(ct), prefix(w_ct, Tn + 2, torch.int32), what + " ct")
            L.same(host(cn), prefix(w_cn, Tn + 2, torch.int32), what + " cn")
            L.same(host(tlo), prefix(w_tlo, Tn + 3, torch.int32), what + " tlo")
            L.same(host(scal), prefix(w_scal, 6, torch.int32), what + " scal")
            w_ci = stale.copy()
            w_ci[col0 >= 0, 0] = col0[col0 >= 0]
            L.same(host(ci), w_ci, what + " cand_idx")
            assert K == 1 or Tn < 5 or 0 < w_scal[1] < Tn  # (K = 1: every root is pure, no candidate)


def test_root_frontier_rejects_empty_problem(cuda):
    mod, st = _call()
    b = out(cuda, 8)
    s = torch.ones(8, device=cuda)
    for Tn, K in ((0, 2), (2, 0)):
        with pytest.raises(RuntimeError, match="contract violation code -2"):
            mod.tree_root_frontier(s.data_ptr(), Tn, K, 4, 0, 2.0, 2, b.data_ptr(), b.data_ptr(), b.data_ptr(),
                                   b.data_ptr(), b.data_ptr(), st)
    L.same(host(b), expect(8, torch.int32), "nothing launched")


# ---- tree_level_group / tree_level_keys ----
def _run_group(cuda, c, mode, nt_max):
    mod, st = _call()
    stride, a_dev, keep = counted(cuda, mode, c.A)
    nch = mod.tree_level_group_chunks(c.N)
    assert nch == -(-c.N // L.GROUP_CH)
    node_of, ci, tlo, W = (dev_of(cuda, x) for x in (c.node_of, c.cand_idx, c.tlo, c.W))
    cnt_ws = garbage(cuda, nch * stride)
    counts, starts = out(cuda, stride), out(cuda, stride)
    rows, row_w = out(cuda, c.T * c.N), out(cuda, c.T * c.N, torch.float32)
    mod.tree_level_group(node_of.data_ptr(), ci.data_ptr(), tlo.data_ptr(), W.data_ptr(), c.T, c.N, c.maxn, stride,
                         nt_max, cnt_ws.data_ptr(), counts.data_ptr(), starts.data_ptr(), rows.data_ptr(),
                         row_w.data_ptr(), a_dev, st)
    want = L.group_ns(c.node_of, c.cand_idx, c.tlo, c.W)
    what = f"group T {c.T} N {c.N} {mode}"
    L.same(host(counts), prefix(want.counts, stride, torch.int32), what + " counts")
    L.same(host(starts), prefix(want.starts, stride, torch.int32), what + " starts")
    L.same(host(rows), prefix(want.rows, c.T * c.N, torch.int32), what + " rows")
    L.same(host(row_w), prefix(want.row_w, c.T * c.N, torch.float32), what + " row_w")
    for name, t, src in (("node_of", node_of, c.node_of), ("cand_idx", ci, c.cand_idx)):
        L.same(host(t), src, what + f" {name} (input)")
    return want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", L.GROUP_SHAPES, ids=str)
def test_level_group(cuda, shape, mode):
    """nt of 1 (no key bits), a power of two and others; candidate-less trees first, in the middle and last;
    a ragged last chunk and last 64-row step; chunk counts that leave idle waves in the last workgroup;
    out-of-bag rows, rows of nodes that are no candidate, a candidate without rows, an inactive chunk,
    64-row steps of one key and of 64 keys.  In bound mode nt_max is the loop's doubled bound too."""
    c = L.group_case(*shape)
    _run_group(cuda, c, mode, c.nt_max if mode == "exact" else min(2 * c.nt_max, 4096))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", L.GROUP_LDS_SHAPES, ids=str)
def test_level_group_at_the_lds_limit(cuda, shape, mode):
    """nt_max = 4096 (4 waves x 4096 counters = 64 KB of LDS), with 4096 candidates and as a bound above the
    real 2500."""
    T, N, cands, nt_max = shape
    want = _run_group(cuda, L.group_case(T, N, cands, 8191), mode, nt_max)
    assert len(want.counts) == cands[0] and want.counts.max() >= 2


def test_level_group_rejects_nt_max_out_of_range(cuda):
    mod, st = _call()
    c = L.group_case(*L.GROUP_SHAPES[2])
    node_of, ci, tlo, W = (dev_of(cuda, x) for x in (c.node_of, c.cand_idx, c.tlo, c.W))
    b = out(cuda, c.T * c.N)
    for nt_max in (4097, 0):
        with pytest.raises(RuntimeError, match="contract violation code -4"):
            mod.tree_level_group(node_of.data_ptr(), ci.data_ptr(), tlo.data_ptr(), W.data_ptr(), c.T, c.N, c.maxn,
                                 c.A, nt_max, b.data_ptr(), b.data_ptr(), b.data_ptr(), b.data_ptr(), b.data_ptr(), 0,
                                 st)
    L.same(host(b), expect(c.T * c.N, torch.int32), "nothing launched")


@pytest.mark.parametrize("shape", L.GROUP_SHAPES, ids=str)
def test_level_keys_and_sort_fallback(cuda, shape):
    """tree_level_keys against the oracle, and the builder's fallback path (a stable sort of those keys; the
    rows of key -1 come first and are skipped by the starts) against the oracle's grouping."""
    mod, st = _call()
    c = L.group_case(*shape)
    node_of, ci = dev_of(cuda, c.node_of), dev_of(cuda, c.cand_idx)
    key = out(cuda, c.T * c.N + 4)
    mod.tree_level_keys(node_of.data_ptr(), ci.data_ptr(), c.T, c.N, c.maxn, key.data_ptr(), st)
    L.same(host(key), prefix(L.level_keys(c.node_of, c.cand_idx).reshape(-1), c.T * c.N + 4, torch.int32), "keys")
    keys, order = torch.sort(key[:c.T * c.N], stable=True)
    Wf = dev_of(cuda, c.W).reshape(-1)
    bounds = torch.searchsorted(keys, torch.arange(c.A + 1, dtype=torch.int32, device=cuda))
    want = L.group_ns(c.node_of, c.cand_idx, c.tlo, c.W)
    first = int(bounds[0])
    L.same(host((order % c.N).to(torch.int32))[first:], want.rows, "sorted rows")
    L.same(host(Wf[order])[first:], want.row_w, "sorted row_w")
    L.same(host((bounds[1:] - bounds[:-1]).to(torch.int32)), want.counts, "sorted counts")
    L.same(host((bounds[:-1] - first).to(torch.int32)), want.starts, "sorted starts")


# ---- tree_level_keys / tree_partition / tree_partition_split at the row-loop shapes ----
@pytest.mark.parametrize("shape", L.PARTITION_SHAPES, ids=str)
def test_keys_and_partitions(cuda, shape):
    """(2, 5), and (3, 700001) where T x N exceeds the 8192 x 256 threads of the largest grid.  Bins 0 and 63,
    rows at the split bin and one above, nodes without a split, rows already done."""
    mod, st = _call()
    c = L.partition_case(*shape)
    n = c.T * c.N
    feature, split_bin, left, ci, bins = (dev_of(cuda, x) for x in (c.feature, c.split_bin, c.left, c.cand_idx, c.bins))
    node_of = dev_of(cuda, prefix(c.node_of.reshape(-1), n + 8, torch.int32))
    key = out(cuda, n + 8)
    mod.tree_level_keys(node_of.data_ptr(), ci.data_ptr(), c.T, c.N, c.maxn, key.data_ptr(), st)
    L.same(host(key), prefix(L.level_keys(c.node_of, c.cand_idx).reshape(-1), n + 8, torch.int32), "keys")
    want = prefix(L.partition(c.node_of, c.feature, c.split_bin, c.left, c.bins).reshape(-1), n + 8, torch.int32)
    assert (want[:n] == -1).any() and (want[:n] >= 0).any()
    a, b = node_of.clone(), node_of.clone()
    mod.tree_partition(a.data_ptr(), feature.data_ptr(), split_bin.data_ptr(), left.data_ptr(), bins.data_ptr(), c.T,
                       c.N, c.maxn, st)
    mod.tree_partition_split(b.data_ptr(), feature.data_ptr(), split_bin.data_ptr(), left.data_ptr(), bins.data_ptr(),
                             c.T, c.N, c.maxn, st)
    L.same(host(a), want, "tree_partition")
    L.same(host(b), want, "tree_partition_split")


# ---- tree_level_decide ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", L.DECIDE_K)
@pytest.mark.parametrize("A", L.DECIDE_A)
def test_level_decide(cuda, A, K, mode):
    """Gains > 0, 0, < 0, NaN, +-inf; children pure, empty, of weight exactly min2 and a quarter below; classes
    with zero count under entropy.  Bound mode: NaN-free junk past the real count, columns >= A untouched."""
    mod, st = _call()
    for min2 in L.MIN2:
        c = L.decide_case(A, K, min2)
        stride, a_dev, keep = counted(cuda, mode, A)
        gain = padded(cuda, c.gain, stride, np.float32(0.75))
        left = padded(cuda, c.left.reshape(-1), stride * K, np.float32(3.0))
        total = padded(cuda, c.total.reshape(-1), stride * K, np.float32(9.0))
        for imp in L.IMPURITIES:
            dec = out(cuda, (5, stride), torch.float32)
            mod.tree_level_decide(stride, gain.data_ptr(), left.data_ptr(), total.data_ptr(), K, imp, float(min2),
                                  dec.data_ptr(), a_dev, st)
            want = expect((5, stride), torch.float32)
            want[:, :A] = L.decide(c.gain, c.left, c.total, imp, min2)
            L.same(host(dec), want, f"decide A {A} K {K} min2 {min2} impurity {imp} {mode}")
            if A >= 255 and K >= 2:
                assert 0 < want[1, :A].sum() < A and 0 < want[2, :A].sum() < A and 0 < want[0, :A].sum() < A


# ---- tree_frontier ----
def _run_frontier(cuda, c, mode, derive):
    mod, st = _call()
    A, Tn = c.A, c.Tn
    stride, a_dev, keep = counted(cuda, mode, A)
    dec_h = np.full((5, stride), 1.0, dtype=np.float32)  # junk past the count: flags that would all fire
    dec_h[:, :A] = c.dec
    dec, tlo, nn, ci = (dev_of(cuda, x) for x in (dec_h, c.tlo, c.n_nodes, c.cand_idx))
    ct, cn = padded(cuda, c.ct, stride, np.int32(0)), padded(cuda, c.cn, stride, np.int32(0))
    nn_next, tlo_next, scal = out(cuda, Tn + 2), out(cuda, Tn + 3), out(cuda, 4)
    pos, q, front = garbage(cuda, stride + 1), garbage(cuda, 2 * stride + 1), garbage(cuda, 2 * stride, torch.float32)
    ti, ni, cl, dsi = (out(cuda, stride, torch.int64) for _ in range(4))
    ct_next, cn_next = out(cuda, 2 * stride), out(cuda, 2 * stride)
    par = out(cuda, 2 * stride) if derive else None
    der = out(cuda, 2 * stride) if derive else None
    mod.tree_frontier(stride, Tn, c.maxn, ct.data_ptr(), cn.data_ptr(), tlo.data_ptr(), dec.data_ptr(),
                      nn.data_ptr(), nn_next.data_ptr(), pos.data_ptr(), ti.data_ptr(), ni.data_ptr(), cl.data_ptr(),
                      dsi.data_ptr(), front.data_ptr(), q.data_ptr(), ct_next.data_ptr(), cn_next.data_ptr(),
                      tlo_next.data_ptr(), ci.data_ptr(), scal.data_ptr(), a_dev, par.data_ptr() if derive else 0,
                      der.data_ptr() if derive else 0, st)
    w = L.frontier(c.ct, c.cn, c.tlo, c.dec, c.n_nodes, c.cand_idx, derive)
    what = f"frontier A {A} {mode} derive {derive}"
    L.same(host(scal), w.scal, what + " scal")
    L.same(host(nn_next), prefix(w.n_nodes_next, Tn + 2, torch.int32), what + " n_nodes_next")
    L.same(host(tlo_next), prefix(w.tlo_next, Tn + 3, torch.int32), what + " tlo_next")
    for name, t in (("ti", ti), ("ni", ni), ("cl", cl), ("dsi", dsi)):
        L.same(host(t), prefix(getattr(w, name), stride, torch.int64), f"{what} {name}")
    L.same(host(ct_next), prefix(w.ct_next, 2 * stride, torch.int32), what + " ct_next")
    L.same(host(cn_next), prefix(w.cn_next, 2 * stride, torch.int32), what + " cn_next")
    L.same(host(ci), w.cand_idx, what + " cand_idx")  # stale entries of untouched nodes survive
    if derive:
        L.same(host(par), prefix(w.parent_of, 2 * stride, torch.int32), what + " parent_of")
        L.same(host(der), prefix(w.derive_from, 2 * stride, torch.int32), what + " derive_from")
    for name, t, src in (("ct", ct, c.ct), ("cn", cn, c.cn), ("n_nodes", nn, c.n_nodes), ("tlo", tlo, c.tlo)):
        L.same(host(t)[:len(src)], src, f"{what} {name} (input)")
    return w


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("A", L.FRONTIER_A)
def test_frontier(cuda, A, mode):
    """The scans' 8-wide and 8192-wide ragged edges (A = 20000: 3 tiles, then 5 over the 40000 children);
    candidate-less trees; per-tree node counters; child flags independent of the split flag; no split at all;
    with and without the derive outputs, sibling pairs of equal weight and pairs with one candidate."""
    for p in L.SPLIT_PROB:
        c = L.frontier_case(A, p)
        for derive in (False, True):
            w = _run_frontier(cuda, c, mode, derive)
            if p == 0.0:
                assert w.scal.tolist() == [0, 0, 0, 0]
            if p == 1.0:
                assert w.scal[0] == A


def test_frontier_rejects_misaligned_and_empty(cuda):
    """The scans read dec / front and write pos / q as 16-byte vectors: a base 4 bytes off is refused (-3), and
    so is A = 0 (-2), on the host, before any launch."""
    mod, st = _call()
    c = L.frontier_case(9, 0.5)
    f = garbage(cuda, 64, torch.float32)
    dec = torch.cat([f[:4], dev_of(cuda, c.dec).reshape(-1)])  # dec proper starts 16 bytes in
    i64 = out(cuda, 64, torch.int64)
    b = out(cuda, 64)
    ci = dev_of(cuda, c.cand_idx)
    ct, cn, tlo, nn = (dev_of(cuda, x) for x in (c.ct, c.cn, c.tlo, c.n_nodes))

    def run(A, dec_ptr, front_ptr, pos_ptr, q_ptr):
        mod.tree_frontier(A, c.Tn, c.maxn, ct.data_ptr(), cn.data_ptr(), tlo.data_ptr(), dec_ptr, nn.data_ptr(),
                          b.data_ptr(), pos_ptr, i64.data_ptr(), i64.data_ptr(), i64.data_ptr(), i64.data_ptr(),
                          front_ptr, q_ptr, b.data_ptr(), b.data_ptr(), b.data_ptr(), ci.data_ptr(), b.data_ptr(), 0, 0,
                          0, st)

    ok = (dec.data_ptr() + 16, f.data_ptr(), b.data_ptr(), b.data_ptr())
    for k in range(4):
        ptrs = list(ok)
        ptrs[k] += 4
        with pytest.raises(RuntimeError, match="contract violation code -3"):
            run(c.A, *ptrs)
    with pytest.raises(RuntimeError, match="contract violation code -2"):
        run(0, *ok)
    L.same(host(b), expect(64, torch.int32), "nothing launched")
    L.same(host(ci), c.cand_idx, "nothing launched")


# ---- tree_commit_level ----
def _run_commit(cuda, c, S_arg, s_real, s_dev):
    mod, st = _call()
    n = max(S_arg, 1)
    ti, ni, cl, dsi = (padded(cuda, x[:s_real], n, np.int64(0)) for x in (c.ti, c.ni, c.cl, c.dsi))
    feat, bin_, gain, rleft, rtotal, thr = (dev_of(cuda, x) for x in (c.feat, c.bin, c.gain, c.rleft, c.rtotal,
                                                                      c.thr_mat))
    d = SimpleNamespace(**{k: dev_of(cuda, getattr(c.arrs, k)) for k in L.FOREST_FIELDS})
    mod.tree_commit_level(S_arg, ti.data_ptr(), ni.data_ptr(), cl.data_ptr(), dsi.data_ptr(), feat.data_ptr(),
                          bin_.data_ptr(), gain.data_ptr(), rleft.data_ptr(), rtotal.data_ptr(), c.K, thr.data_ptr(),
                          c.ldthr, c.maxn, d.feature.data_ptr(), d.split_bin.data_ptr(), d.thresh.data_ptr(),
                          d.left.data_ptr(), d.right.data_ptr(), d.gains.data_ptr(), d.stats.data_ptr(), s_dev, st)
    want = L.commit(c.arrs, c.ti[:s_real], c.ni[:s_real], c.cl[:s_real], c.dsi[:s_real], c.feat, c.bin, c.gain, c.rleft,
                    c.rtotal, c.thr_mat)
    for k in L.FOREST_FIELDS:  # (whole arrays: nodes not committed keep their junk)
        L.same(host(getattr(d, k)), getattr(want, k), f"commit S {s_real} of {S_arg} K {c.K} {k}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", L.CLASS_COUNTS)
@pytest.mark.parametrize("S", L.COMMIT_S)
def test_commit_level(cuda, S, K, mode):
    """One, exactly one workgroup of, and one more than a workgroup of splits; thresholds read with a row
    stride (40) wider than the bins in use; in bound mode the split count comes from the device and the
    records past it (all naming tree 0, node 0) must not be committed."""
    c = L.commit_case(S, K)
    S_arg, s_dev, keep = counted(cuda, mode, S)
    _run_commit(cuda, c, S_arg, S, s_dev)


def test_commit_level_of_no_split_writes_nothing(cuda):
    c = L.commit_case(1, 6)
    _run_commit(cuda, c, 0, 0, 0)
    zero = torch.zeros(1, dtype=torch.int32, device=cuda)
    _run_commit(cuda, c, 4, 0, zero.data_ptr())


# ---- the teacher-forced level loop ----
class _DeviceLoop:
    """The call sequence of models/tree.py ``_levels_device_frontier`` on the real kernels, except the split
    search: every level takes the LevelResult the oracle chain computed on the CPU, so split-search ties cannot
    make the two diverge, and is compared with the oracle's level phase by phase.  ``bound``: arrays, grids
    and nt_max sized by the loop's doubling bounds, the real counts read by the kernels from scal_all."""

    def __init__(self, dev, fs, bound, derive):
        self.dev, self.fs, self.bound, self.derive = dev, fs, bound, derive
        self.mod, self.st = _call()
        Tn, N, maxn, K = L.FIT_T, L.FIT_N, fs.maxn, L.FIT_K
        arrs, node_of, n_nodes, cand_idx = L.fit_state(fs)
        self.arrs = SimpleNamespace(**{k: dev_of(dev, getattr(arrs, k)) for k in L.FOREST_FIELDS})
        self.node_of, self.nn, self.ci = dev_of(dev, node_of), dev_of(dev, n_nodes), dev_of(dev, cand_idx)
        self.W, self.bins, self.thr = dev_of(dev, fs.W), dev_of(dev, fs.bins), dev_of(dev, fs.thr_mat)
        self.scal_all = torch.zeros(4 * (L.FIT_DEPTH + 1), dtype=torch.int32, device=dev)
        self.A, self.nt_max = Tn, 1
        self.ct, self.cn, self.tlo = out(dev, Tn), out(dev, Tn), out(dev, Tn + 1)
        self.mod.tree_root_frontier(self.arrs.stats.data_ptr(), Tn, K, maxn * K, fs.impurity, fs.min2, maxn,
                                    self.ct.data_ptr(), self.cn.data_ptr(), self.tlo.data_ptr(), self.ci.data_ptr(),
                                    self.scal_all.data_ptr(), self.st)
        self.levels = 0

    def level(self, depth, lv):
        dev, fs, mod, st = self.dev, self.fs, self.mod, self.st
        Tn, N, maxn, K, F = L.FIT_T, L.FIT_N, fs.maxn, L.FIT_K, L.FIT_F
        what = f"level {depth}"
        A_real = len(lv.ct)
        if depth == 0:
            L.same(host(self.scal_all[:4]), lv.root.scal, "root scal")
            L.same(host(self.ci), lv.cand_idx, "root cand_idx")
        if self.bound:
            A, nt_max = self.A, self.nt_max
            a_dev = self.scal_all.data_ptr() + 4 * (4 * depth + 1)
        else:
            A, nt_max, a_dev = A_real, max(int(np.diff(lv.tlo).max()), 1), 0
        ct, cn = self.ct[:A], self.cn[:A]
        L.same(host(ct)[:A_real], lv.ct, what + " ct")
        L.same(host(cn)[:A_real], lv.cn, what + " cn")
        L.same(host(self.tlo), lv.tlo, what + " tlo")
        L.same(host(self.nn), lv.n_nodes, what + " n_nodes")
        # grouping
        nch = mod.tree_level_group_chunks(N)
        cnt_ws = garbage(dev, nch * A)
        counts, starts = out(dev, A), out(dev, A)
        rows, row_w = out(dev, Tn * N), out(dev, Tn * N, torch.float32)
        mod.tree_level_group(self.node_of.data_ptr(), self.ci.data_ptr(), self.tlo.data_ptr(), self.W.data_ptr(), Tn, N,
                             maxn, A, nt_max, cnt_ws.data_ptr(), counts.data_ptr(), starts.data_ptr(),
                             rows.data_ptr(), row_w.data_ptr(), a_dev, st)
        L.same(host(counts), prefix(lv.group.counts, A, torch.int32), what + " counts")
        L.same(host(starts), prefix(lv.group.starts, A, torch.int32), what + " starts")
        L.same(host(rows), prefix(lv.group.rows, Tn * N, torch.int32), what + " rows")
        L.same(host(row_w), prefix(lv.group.row_w, Tn * N, torch.float32), what + " row_w")
        # feature subsets
        if fs.m < F:
            feats = out(dev, (A, fs.m))
            mod.tree_feature_subsets(L.FIT_SEED, ct.data_ptr(), cn.data_ptr(), A, F, fs.m, feats.data_ptr(), a_dev, st)
            want = expect((A, fs.m), torch.int32)
            want[:A_real] = lv.feats
            L.same(host(feats), want, what + " feature subsets")
        # the split search's result, from the CPU (junk past the real count)
        gain = padded(dev, lv.res.gain, A, np.float32(0.5))
        left = padded(dev, lv.res.left.reshape(-1), A * K, np.float32(1.0))
        total = padded(dev, lv.res.total.reshape(-1), A * K, np.float32(5.0))
        feat, bin_ = padded(dev, lv.res.feat, A, np.int32(0)), padded(dev, lv.res.bin, A, np.int32(0))
        dec = out(dev, (5, A), torch.float32)
        mod.tree_level_decide(A, gain.data_ptr(), left.data_ptr(), total.data_ptr(), K, fs.impurity, fs.min2,
                              dec.data_ptr(), a_dev, st)
        want = expect((5, A), torch.float32)
        want[:, :A_real] = lv.dec
        L.same(host(dec), want, what + " dec")
        # frontier
        scal = self.scal_all[4 * (depth + 1):4 * (depth + 2)]
        nn_next, tlo_next = out(dev, Tn), out(dev, Tn + 1)
        pos, q, front = garbage(dev, A + 1), garbage(dev, 2 * A + 1), garbage(dev, 2 * A, torch.float32)
        ti, ni, cl, dsi = (out(dev, A, torch.int64) for _ in range(4))
        ct_next, cn_next = out(dev, 2 * A), out(dev, 2 * A)
        par = out(dev, 2 * A) if self.derive else None
        der = out(dev, 2 * A) if self.derive else None
        mod.tree_frontier(A, Tn, maxn, ct.data_ptr(), cn.data_ptr(), self.tlo.data_ptr(), dec.data_ptr(),
                          self.nn.data_ptr(), nn_next.data_ptr(), pos.data_ptr(), ti.data_ptr(), ni.data_ptr(),
                          cl.data_ptr(), dsi.data_ptr(), front.data_ptr(), q.data_ptr(), ct_next.data_ptr(),
                          cn_next.data_ptr(), tlo_next.data_ptr(), self.ci.data_ptr(), scal.data_ptr(), a_dev,
                          par.data_ptr() if self.derive else 0, der.data_ptr() if self.derive else 0, st)
        fr = lv.fr
        L.same(host(scal), fr.scal, what + " scal")
        L.same(host(nn_next), fr.n_nodes_next, what + " n_nodes_next")
        L.same(host(tlo_next), fr.tlo_next, what + " tlo_next")
        for name, t in (("ti", ti), ("ni", ni), ("cl", cl), ("dsi", dsi)):
            L.same(host(t), prefix(getattr(fr, name), A, torch.int64), f"{what} {name}")
        L.same(host(ct_next), prefix(fr.ct_next, 2 * A, torch.int32), what + " ct_next")
        L.same(host(cn_next), prefix(fr.cn_next, 2 * A, torch.int32), what + " cn_next")
        L.same(host(self.ci), fr.cand_idx, what + " cand_idx")
        if self.derive:
            L.same(host(par), prefix(fr.parent_of, 2 * A, torch.int32), what + " parent_of")
            L.same(host(der), prefix(fr.derive_from, 2 * A, torch.int32), what + " derive_from")
        S_real, A_next = int(fr.scal[0]), int(fr.scal[1])
        self.levels += 1
        if S_real == 0:
            return
        # commit + partition
        S, s_dev = (A, scal.data_ptr()) if self.bound else (S_real, 0)
        a = self.arrs
        mod.tree_commit_level(S, ti.data_ptr(), ni.data_ptr(), cl.data_ptr(), dsi.data_ptr(), feat.data_ptr(),
                              bin_.data_ptr(), gain.data_ptr(), left.data_ptr(), total.data_ptr(), K,
                              self.thr.data_ptr(), self.thr.shape[1], maxn, a.feature.data_ptr(),
                              a.split_bin.data_ptr(), a.thresh.data_ptr(), a.left.data_ptr(), a.right.data_ptr(),
                              a.gains.data_ptr(), a.stats.data_ptr(), s_dev, st)
        mod.tree_partition_split(self.node_of.data_ptr(), a.feature.data_ptr(), a.split_bin.data_ptr(),
                                 a.left.data_ptr(), self.bins.data_ptr(), Tn, N, maxn, st)
        for k in L.FOREST_FIELDS:
            L.same(host(getattr(a, k)), getattr(lv.arrs_next, k), f"{what} committed {k}")
        L.same(host(self.node_of), lv.node_of_next, what + " node_of")
        self.nn, self.tlo = nn_next, tlo_next
        if self.bound:
            self.A = min(2 * A, Tn * N)
            self.nt_max = min(2 * nt_max, 4096)
            self.ct, self.cn = ct_next[:self.A], cn_next[:self.A]
        else:
            self.ct, self.cn = ct_next[:A_next], cn_next[:A_next]

    def forest(self):
        arrs = SimpleNamespace(**{k: host(getattr(self.arrs, k)) for k in L.FOREST_FIELDS})
        return arrs, host(self.nn)


def _teacher_forced(cuda, case, mode, derive):
    fs = L.fit_setup(*case)
    loop = _DeviceLoop(cuda, fs, mode == "bound", derive)
    arrs, n_nodes = L.chained_oracle(fs, derive=derive, on_level=loop.level)
    assert loop.levels >= 5
    d_arrs, d_nn = loop.forest()
    L.same(d_nn, n_nodes, "n_nodes")
    L.assert_forest(d_arrs, d_nn, fs.ref, f"device loop {case} {mode}")  # the CPU builder's forest, every depth


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", L.FIT_CASES, ids=str)
def test_teacher_forced_level_loop(cuda, case, mode):
    _teacher_forced(cuda, case, mode, derive=False)


@pytest.mark.parametrize("mode", MODES)
def test_teacher_forced_level_loop_with_derived_siblings(cuda, mode):
    """featureSubsetStrategy "all" with parent_of / derive_from requested: derived nodes get no rows from the
    grouping and their histograms are parent - sibling; the forest is still the CPU builder's."""
    _teacher_forced(cuda, L.FIT_CASES[-1], mode, derive=True)
