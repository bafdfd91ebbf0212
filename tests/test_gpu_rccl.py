"""RCCL under test on the one GPU of the test box (VERDICT r5 "missing" item 1).

``HAR_DIST_FORCE_PG=1`` makes ``parallel.dist.init`` create a 1-rank ``nccl`` process group — RCCL on
ROCm — even though WORLD_SIZE is 1, and marks the context ``forced``: the DP code paths then issue
their collectives through a real RCCL communicator on HBM buffers (over one rank every collective
is an identity, so each DP path must equal its single-process result bit for bit).

What runs through RCCL here: communicator setup (``init_process_group(nccl, device_id=...)``), every
``parallel/comm.py`` entry point on device tensors with no host staging (all-reduce SUM / MAX / MIN,
reduce-scatter, all-gather, broadcast, ``barrier(device_ids)``), host tensors staged through HBM
(``dist.max_over_ranks`` et al.), and on that same group:

* the MLP DP step, sharded (reduce-scatter of G -> Adam on the owned slice -> all-gather of P ->
  one refresh kernel) and all-reduce, bitwise equal to the N = 1 step;
* the segmented graph form of that step (graph(fwd + bwd + reduce) -> eager RCCL -> graph(Adam));
* the LogisticRegression DP bucket (one all-reduce of [gradients | exact losses] per evaluation);
* the forest owner path (``NodeOwner``: packed integer reduce-scatter + all-gather per level);
* ``bench.py --graph 2`` under the forced group (the driver's bench in its DP form).

The reference's combines are Spark's ``treeAggregate`` / ``reduceByKey`` (``Main/main.py:117,215,
300,481``).
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rccl(cuda):
    """A forced 1-rank RCCL group for the module (destroyed at its end)."""
    import torch.distributed as dist

    from har.parallel import dist as hd

    saved = {k: os.environ.get(k) for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HAR_DIST_FORCE_PG",
                                             "HAR_DIST_BACKEND", "MASTER_PORT", "HAR_DIST_SHARE_DEVICE")}
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HAR_DIST_BACKEND", "MASTER_PORT", "HAR_DIST_SHARE_DEVICE"):
        os.environ.pop(k, None)
    os.environ["HAR_DIST_FORCE_PG"] = "1"
    assert not dist.is_initialized()
    ctx = hd.init()
    try:
        yield ctx
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_forced_group_is_rccl(rccl):
    import torch.distributed as dist

    from har.parallel import comm

    assert rccl.forced and rccl.collective and not rccl.is_distributed
    assert rccl.backend == "nccl" and rccl.device.type == "cuda"
    assert dist.is_initialized() and comm.backend() == "nccl" and comm.world_of() == 1 and comm.rank_of() == 0


def test_rccl_comm_entry_points_on_device_buffers(rccl, cuda):
    """Every comm.py entry point on HBM buffers through the RCCL communicator: no staging copy (the
    tensor handed to RCCL is the caller's), values as a 1-rank reduction leaves them."""
    import torch.distributed as dist

    from har.parallel import comm
    from har.parallel import dist as hd

    g = torch.Generator(device=cuda).manual_seed(0)
    x = torch.randn(4099, device=cuda, generator=g)
    ref = x.clone()
    ptr = x.data_ptr()
    assert comm._staged(x, "nccl") is x  # device + contiguous: handed to RCCL as is
    comm.all_reduce(x)
    assert x.data_ptr() == ptr and torch.equal(x, ref)
    for op in (dist.ReduceOp.MAX, dist.ReduceOp.MIN):
        comm.all_reduce(x, op=op)
        assert torch.equal(x, ref)
    # a non-contiguous device view: staged into a contiguous device buffer and copied back
    m = torch.randn(64, 48, device=cuda, generator=g)
    mt = m.t()
    mref = mt.clone()
    comm.all_reduce(mt)
    assert torch.equal(mt, mref) and torch.equal(m, mref.t())
    # reduce-scatter / all-gather into device buffers (world 1: out = in)
    inp = torch.randn(1024, device=cuda, generator=g)
    out = torch.empty(1024, device=cuda)
    comm.reduce_scatter_tensor(out, inp)
    assert torch.equal(out, inp)
    ag = torch.empty(1024, device=cuda)
    comm.all_gather_into_tensor(ag, inp)
    assert torch.equal(ag, inp)
    # in-place all-gather (the sharded optimizer's form: the input is the owned slice of the output)
    full = torch.randn(512, device=cuda, generator=g)
    fref = full.clone()
    comm.all_gather_into_tensor(full, full[:512])
    assert torch.equal(full, fref)
    for dt in (torch.int32, torch.bfloat16, torch.float16):
        t = (torch.arange(300, device=cuda) % 17).to(dt)
        tr = t.clone()
        comm.all_reduce(t)
        assert torch.equal(t, tr), dt
    b = torch.arange(10, dtype=torch.float32, device=cuda)
    comm.broadcast(b, src=0)
    assert torch.equal(b, torch.arange(10, dtype=torch.float32, device=cuda))
    comm.barrier(device=cuda)
    hd.barrier(rccl)
    torch.cuda.synchronize()


def test_rccl_host_scalars_staged_through_hbm(rccl):
    """Host tensors / Python scalars under RCCL: staged to the device, reduced, copied back."""
    import torch.distributed as dist

    from har.parallel import comm
    from har.parallel import dist as hd

    h = torch.tensor([1.5, -2.0, 7.25], dtype=torch.float64)
    assert comm._home(h, "nccl").type == "cuda"
    comm.all_reduce(h, op=dist.ReduceOp.SUM)
    assert h.device.type == "cpu" and h.tolist() == [1.5, -2.0, 7.25]
    assert hd.sum_over_ranks(rccl, 3.5) == 3.5
    assert hd.max_over_ranks(rccl, -1.25) == -1.25
    assert hd.mean_over_ranks(rccl, 8.0) == 8.0
    cnt = torch.tensor([12345678901], dtype=torch.int64)
    comm.all_reduce(cnt, op=dist.ReduceOp.MAX)
    assert int(cnt) == 12345678901


def _mlp_pair(cuda, sharded: bool, B=4096):
    import torch.distributed as dist

    from har.models.mlp import MLPEngine

    old = os.environ.get("HAR_MLP_SHARDED_OPT")
    os.environ["HAR_MLP_SHARDED_OPT"] = "1" if sharded else "0"
    try:
        layers = [43, 256, 256, 6]
        a = MLPEngine(layers, B, cuda, lr=1e-3, seed=4)
        b = MLPEngine(layers, B, cuda, lr=1e-3, seed=4, process_group=dist.group.WORLD, world_size=1, force_dp=True)
    finally:
        if old is None:
            os.environ.pop("HAR_MLP_SHARDED_OPT", None)
        else:
            os.environ["HAR_MLP_SHARDED_OPT"] = old
    assert b.dp and b.sharded == sharded and not a.dp
    return a, b


def _batches(cuda, B, n, in_pad):
    from har.models.mlp import pad_input_bf16

    g = torch.Generator(device=cuda).manual_seed(2)
    out = []
    for _ in range(n):
        X = pad_input_bf16(torch.randn(B, 43, device=cuda, generator=g), in_pad)
        y = torch.randint(0, 6, (B,), device=cuda, generator=g).to(torch.int32)
        out.append((X, y))
    return out


def _assert_same_state(a, b):
    assert torch.equal(a.P, b.P) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert torch.equal(a.Pb, b.Pb) and torch.equal(a.step_count, b.step_count)
    assert torch.equal(a.Pf[: a.Pf.numel() - 256 * 256], b.Pf[: b.Pf.numel() - 256 * 256])  # W0 | W1 fragments


@pytest.mark.parametrize("sharded", [False, True])
def test_rccl_mlp_dp_step_bitwise_equals_single_gpu_step(rccl, cuda, sharded):
    """The DP step on the RCCL group — slab reduction -> G, RCCL reduce-scatter (sharded) or
    all-reduce, Adam (on the owned slice), RCCL all-gather of P + one refresh kernel — gives
    bitwise the parameters, moments, bf16 / fragment copies and step counter of the N = 1 step."""
    B = 4096
    a, b = _mlp_pair(cuda, sharded, B)
    calls = {"rs": 0, "ag": 0, "ar": 0}
    from har.parallel import comm

    real = (comm.reduce_scatter_tensor, comm.all_gather_into_tensor, comm.all_reduce)

    def rs(*x, **k):
        calls["rs"] += 1
        return real[0](*x, **k)

    def ag(*x, **k):
        calls["ag"] += 1
        return real[1](*x, **k)

    def ar(*x, **k):
        calls["ar"] += 1
        return real[2](*x, **k)

    comm.reduce_scatter_tensor, comm.all_gather_into_tensor, comm.all_reduce = rs, ag, ar
    try:
        for X, y in _batches(cuda, B, 3, a.layout.in_pad):
            a.train_step(X, y, B)
            b.train_step(X, y, B)
    finally:
        comm.reduce_scatter_tensor, comm.all_gather_into_tensor, comm.all_reduce = real
    torch.cuda.synchronize()
    assert a.last_path == "step" and b.last_path == "step"
    _assert_same_state(a, b)
    assert int(b.step_count[0]) == 3
    st = b.collective_stats()
    if sharded:
        assert calls == {"rs": 3, "ag": 3, "ar": 0} and st["reduce_scatter"] == 1 and st["all_gather"] == 1
        assert st["kernels"] == 5
    else:
        assert calls == {"rs": 0, "ag": 0, "ar": 3} and st["all_reduce"] == 1 and st["kernels"] == 4
    la, ca = a.last_loss_and_correct()
    lb, cb = b.last_loss_and_correct()
    assert la == lb and ca == cb


@pytest.mark.parametrize("sharded", [False, True])
def test_rccl_mlp_dp_step_segmented_graphs(rccl, cuda, sharded):
    """bench.py --graph 2's form: graph(fwd + bwd + slab reduction) -> eager RCCL collective ->
    graph(Adam) [-> eager all-gather + refresh]: bitwise the eager DP step."""
    B = 4096
    a, b = _mlp_pair(cuda, sharded, B)
    data = _batches(cuda, B, 2, a.layout.in_pad)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    # warm-up (the plan is built, allocations settle) on both engines identically
    for X, y in data:
        a.train_step(X, y, B)
    with torch.cuda.stream(s):
        for X, y in data:
            b.grad_phase(X, y, B)
            b.comm_phase()
            b.apply_phase()
            b.gather_phase()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _assert_same_state(a, b)
    gA = []
    for X, y in data:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            b.grad_phase(X, y, B)
        gA.append(g)
    gB = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gB):
        b.apply_phase()
    for i in range(4):
        X, y = data[i % 2]
        a.train_step(X, y, B)
        gA[i % 2].replay()
        b.comm_phase()
        gB.replay()
        b.gather_phase()
    torch.cuda.synchronize()
    _assert_same_state(a, b)
    assert int(b.step_count[0]) == 6


def test_rccl_logreg_dp_bucket(rccl, cuda):
    """The LR DP path on the RCCL group (ONE all-reduce of the [gradients | exact losses] bucket per
    objective evaluation + the summarizer's): bitwise the same DP fit with an identity reduction."""
    from har.models.logreg import FitSpec, LogisticRegression
    from har.parallel import comm
    from har.parallel import data_parallel as dp

    g = torch.Generator().manual_seed(0)
    mu = torch.randn(4, 12, generator=g) * 1.2
    y = torch.randint(0, 4, (6000,), generator=g)
    X = (mu[y] + torch.randn(6000, 12, generator=g)).to(cuda)
    y = y.to(cuda)
    specs = [FitSpec(None, 0.1, 0.0), FitSpec(None, 0.05, 0.3)]
    n = {"ar": 0}
    real = comm.all_reduce

    def count(*a, **k):
        n["ar"] += 1
        return real(*a, **k)

    comm.all_reduce = count
    try:
        ms = dp.fit_logreg_dp(LogisticRegression(maxIter=15), X, y, specs, 4, rccl)
    finally:
        comm.all_reduce = real
    ref = LogisticRegression(maxIter=15).fit_many(X, y, specs, 4, allreduce=lambda t: None)
    assert n["ar"] >= 10
    for m, r in zip(ms, ref):
        assert torch.equal(m.coefficientMatrix, r.coefficientMatrix)
        assert torch.equal(m.interceptVector, r.interceptVector)
        assert m.summary["objectiveHistory"] == r.summary["objectiveHistory"]


@pytest.mark.parametrize("kind", ["rf", "dt"])
def test_rccl_forest_node_owner(rccl, cuda, kind):
    """The owner-computes level reduction (packed integer reduce-scatter + all-gather of the winners)
    through the RCCL group: the single-process forest bit for bit, collectives really issued."""
    from har.models.tree import DecisionTreeClassifier, RandomForestClassifier
    from har.ops import tree as T
    from har.parallel import data_parallel as dp

    g = torch.Generator().manual_seed(0)
    mu = torch.randn(4, 12, generator=g) * 1.2
    y = torch.randint(0, 4, (12000,), generator=g)
    X = mu[y] + torch.randn(12000, 12, generator=g)
    thr = T.find_thresholds(X.numpy(), 32)

    def est():
        return DecisionTreeClassifier(maxDepth=7, seed=3) if kind == "dt" else RandomForestClassifier(
            numTrees=12, maxDepth=6, seed=5)

    owner = dp.NodeOwner(rccl)
    assert not owner.solo
    m = est().fit_tensors(X.to(cuda), y.to(cuda), 4, row_offset=0, thresholds=thr, owner=owner)
    r = est().fit_tensors(X.to(cuda), y.to(cuda), 4, thresholds=thr)
    assert owner.stats["reduce_scatter"] >= 1 and owner.stats["all_gather"] >= 1, owner.stats
    assert torch.equal(m.arrs.feature, r.arrs.feature)
    assert torch.equal(m.arrs.threshold, r.arrs.threshold)
    assert torch.equal(m.arrs.stats, r.arrs.stats)


@pytest.mark.parametrize("kind", ["dt", "rf"])
def test_rccl_forest_one_hot_aware_path_under_data_parallel(rccl, cuda, kind, monkeypatch):
    """The one-hot-aware tree path in its data-parallel form, which the estimators take by default inside
    ``data_parallel``: thresholds from the hybrid matrix, the rank's row shard of it, the level histograms of
    the one-hot-aware kernel reduce-scattered by node owner and searched from the reduced store.  On the
    forced group, with the path on and off, and without a group: the same forest bit for bit — and the "on"
    fit really hands the kernel its one-hot input at every level."""
    from _tree_sparse_util import dense_path, same_arrays, synthetic_hybrid

    from har.models.tree import DecisionTreeClassifier, RandomForestClassifier
    from har.ops import tree as T
    from har.parallel import data_parallel as dp

    hm, y = synthetic_hybrid(cuda, N=6000)
    X = hm.to_dense()
    assert T.hybrid_tree_ok(hm, 32, 4)

    def est():
        return DecisionTreeClassifier(maxDepth=3, seed=3) if kind == "dt" else RandomForestClassifier(
            numTrees=5, maxDepth=4, seed=5)

    levels = []  # per level call of a fit: did the kernel get the one-hot input?
    for name in ("hist_split_planned_dp", "hist_split_native", "hist_split_planned"):
        def spy(*a, _real=getattr(T, name), _name=name, **k):
            levels.append((_name, k.get("sparse") is not None, k.get("owner") is not None))
            return _real(*a, **k)

        monkeypatch.setattr(T, name, spy)

    def in_group():
        # as DecisionTreeClassifier.fit / RandomForestClassifier.fit inside data_parallel (row shard [0, N))
        e = est()
        h = hm if T.hybrid_tree_ok(hm, e.maxBins, 4) else None
        owner = dp.NodeOwner(rccl)
        assert not owner.solo
        m = e.fit_tensors(X, y, 4, row_offset=0, thresholds=e._thresholds(X, h), owner=owner,
                          hybrid=None if h is None else h.rows(0, hm.n_rows))
        assert owner.stats["reduce_scatter"] >= 1 and owner.stats["all_gather"] >= 1, owner.stats
        return m

    on = in_group()
    seen_on, levels[:] = list(levels), []
    off = dense_path(in_group)
    seen_off, levels[:] = list(levels), []
    solo = est().fit_tensors(X, y, 4, hybrid=hm)
    seen_solo = list(levels)
    assert len(seen_on) >= 2 and all(s and o and n != "hist_split_planned" for n, s, o in seen_on), seen_on
    assert len(seen_off) == len(seen_on) and not any(s for _, s, _ in seen_off), seen_off
    assert seen_solo and all(s and not o for _, s, o in seen_solo), seen_solo
    same_arrays(on.arrs, off.arrs)
    same_arrays(on.arrs, solo.arrs)
    assert int(on.arrs.n_nodes.min()) > 1


@pytest.mark.parametrize("graph", ["2", "-1"])
def test_rccl_bench_graph2_subprocess(cuda, tmp_path, graph):
    """bench.py in its DP form on the forced RCCL group: segmented graphs around the eager RCCL
    reduce-scatter / all-gather of the sharded optimizer (--graph 2, HAR_MLP_SHARDED_OPT=1), and the
    driver's default eager step (--graph -1: what the N > 1 scaling runs execute, one rank per GPU: at
    86k parameters one all-reduce, models/mlp.py SHARD_MIN_PARAMS), one JSON line, the collectives
    recorded."""
    env = dict(os.environ, HAR_DIST_FORCE_PG="1", PYTHONUNBUFFERED="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "HAR_MLP_SHARDED_OPT"):
        env.pop(k, None)
    if graph == "2":
        env["HAR_MLP_SHARDED_OPT"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2",
                        "--graph", graph, "--no-wisdm", "--settle-ms", "0", "--full"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["hip_graph"] == ("segmented" if graph == "2" else "off") and rec["n_gpus"] == 1
    cps = rec["collectives_per_step"]
    ph = rec["phase_ms"]
    if graph == "2":
        assert cps["reduce_scatter"] == 1 and cps["all_gather"] == 1 and cps["kernels"] == 5, cps
        assert ph["allreduce"] is not None and ph["all_gather"] is not None
    else:
        assert cps["all_reduce"] == 1 and cps["reduce_scatter"] == 0 and cps["kernels"] == 4, cps
        assert ph["allreduce"] is not None and ph["all_gather"] is None
    assert rec["dist_backend"] == "nccl"
