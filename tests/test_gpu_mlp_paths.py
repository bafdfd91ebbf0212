"""MLPEngine's step paths as objects (models/mlp_paths.py): the fragment copies are repacked exactly
when a path switch needs it, ``last`` follows what ran (not what was planned), the selector names the
path that then runs, and a CPU engine has no paths but every attribute its readers use."""
import pytest
import torch

from test_gpu_mlp_shapes import GRAD_CASES, PATH_ENV, _inputs

ALL_ON = {"HAR_MLP_FUSED": "1", "HAR_MLP_STEP": "1", "HAR_MLP_SMALL": "1"}
LAYERS, CAP = [33, 256, 256, 5], 64
COMPAT = ("native", "layout", "P", "Pb", "Pf", "G", "m", "v", "slabs", "acts", "dbuf", "dims", "step_count", "step_S",
          "fused_ok", "step_ok", "small_ok", "fslab", "fblock_loss", "fblock_correct", "last_path", "last_fused",
          "last_bwd")


def _engine(monkeypatch, cuda, env=ALL_ON, layers=LAYERS, B=CAP):
    from har.models.mlp import MLPEngine

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return MLPEngine(layers, B, cuda, lr=1e-2, seed=3)


def _batch(cuda, B, seed, layers=LAYERS):
    Xb, y = _inputs(layers, B, seed)
    return Xb.to(cuda), y.to(cuda).to(torch.int32)


@pytest.mark.gpu
def test_fragment_copies_fresh_across_path_switches(cuda, monkeypatch):
    """small -> step -> small -> fused_fwd -> step -> serving on one engine, against an engine that
    rebuilds Pb and the fragment copies from P before every step and before the inference: bitwise
    the same parameters, moments, step counter, logits and classes — stale W1^T is never read.
    With every flag on the small path takes each multiple of 32 rows up to its maximum (512), 64 rows
    included, so the step batches are the first multiple of 64 above it."""
    BS = 576
    a, b = _engine(monkeypatch, cuda, B=BS), _engine(monkeypatch, cuda, B=BS)
    assert BS == a.small.max_batch + 64
    plan = [(32, "small"), (BS, "step"), (32, "small"), (48, "fused_fwd"), (BS, "step")]
    for i, (B, path) in enumerate(plan):
        Xb, y = _batch(cuda, B, 20 + i)
        a.train_step(Xb, y, B)
        b.refresh_bf16()
        b.train_step(Xb, y, B)
        assert a.last_path == path and b.last_path == path, (i, a.last_path, b.last_path)
        for name in ("P", "m", "v", "step_count"):
            assert torch.equal(getattr(a, name), getattr(b, name)), f"{name} differs after step {i} ({path})"
    assert int(a.step_count[0]) == len(plan)
    X = torch.randn(64, LAYERS[0], generator=torch.Generator().manual_seed(5)).to(cuda)
    b.refresh_bf16()
    (za, ca), (zb, cb) = a.infer_fused_f32(X), b.infer_fused_f32(X)
    assert torch.equal(za, zb) and torch.equal(ca, cb)
    assert a._pf_fresh and torch.isfinite(za).all()


@pytest.mark.gpu
def test_last_is_set_by_running_not_by_planning(cuda, monkeypatch):
    eng = _engine(monkeypatch, cuda)
    Xb, y = _batch(cuda, 48, 31)
    eng.train_step(Xb, y, 48)
    want = eng.last_loss_and_correct()
    assert eng.last_path == "fused_fwd" and eng.last_fused and not eng.last_bwd
    plan, nwg, S = eng.step.plan(64)
    assert plan is eng.step.plan(64)[0] and nwg >= 1 and S >= 1
    assert eng.last_path == "fused_fwd" and eng.last_fused and not eng.last_bwd
    assert eng.last_loss_and_correct() == want
    assert want[0] > 0 and 0 <= want[1] <= 48


SHAPES = sorted({(p, tuple(layers), B) for p, layers, B, _ in GRAD_CASES})


@pytest.mark.gpu
@pytest.mark.parametrize("path,layers,B", SHAPES, ids=[f"{p}-{'x'.join(map(str, ls))}-B{B}" for p, ls, B in SHAPES])
def test_selector_names_the_path_that_runs(cuda, monkeypatch, path, layers, B):
    eng = _engine(monkeypatch, cuda, PATH_ENV[path], list(layers), B)
    Xb, y = _batch(cuda, B, 9, list(layers))
    chosen = eng.select(Xb, y)
    assert chosen.name == path and eng.last_path is None  # (asking runs nothing)
    # the estimator's epoch-graph question: the expression fit() evaluated before the paths were objects
    assert eng.graph_ok(Xb, y) == bool((eng.step_ok and B % 64 == 0) or (eng.fused_ok and B % 16 == 0))
    eng.train_step(Xb, y, B)
    assert eng.last_path == path and eng.last is chosen
    assert eng.select(Xb, y, whole_step=False).name == (path if path != "small" else "fused_fwd")
    with pytest.raises(ValueError):
        eng.select(Xb.float(), y)


def test_cpu_engine_has_no_paths():
    from har.models.mlp import MLPEngine

    eng = MLPEngine([5, 32, 32, 3], 8, torch.device("cpu"), seed=1)
    assert eng.paths == [] and eng.last is None and not eng.native
    for name in COMPAT:
        getattr(eng, name)
    assert eng.Pf is None and eng.Pb is None and eng.slabs is None and eng.step_S == 0
    assert not (eng.fused_ok or eng.step_ok or eng.small_ok or eng.last_fused or eng.last_bwd)
    assert eng.last_path is None
    g = torch.Generator().manual_seed(2)
    X, y = torch.randn(8, 5, generator=g), torch.randint(0, 3, (8,), generator=g)
    p0 = eng.P.clone()
    losses = []
    for _ in range(3):
        eng.train_step(X, y, 8)
        losses.append(eng.last_loss)
    assert eng.t_step == 3 and not torch.equal(eng.P, p0)
    assert losses[0] > losses[1] > losses[2] > 0
