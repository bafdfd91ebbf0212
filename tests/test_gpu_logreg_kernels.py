"""The logistic-regression kernels branch by branch against the fp64 oracles of tests/_logreg_util.py.

csrc/kernels/logreg_qn.hip: ``logreg_eval_kernel`` (its four instantiations, dense chunking, preloaded
and grouped one-hot gathers, tiles, launch chunks, ``tstride``, prediction mode, large margins),
``logreg_grad_kernel`` (column blocks, a lone column of more than 256 slices, ragged slice tails, more
than 256 tiles, the fixed-point loss), ``logreg_loss_decode_kernel`` and ``logreg_col_slices_kernel``;
csrc/kernels/logreg_setup.hip: the summarizer (tiles + columns, K >= 64 class sums, the slice search
without ``srow``) and ``logreg_prepare_kernel``.

Every case drives the kernels as the solver does (``DeviceLogregSolver._evaluate`` on hand-filled
``weff``) at the smallest shape that reaches its branch, and asserts that the branch was reached.
Tolerances for ordinary inputs are those of ``test_gpu_logreg.py``: loss rtol 2e-5 / atol 1e-6,
gradient rtol 2e-4 / atol 2e-6, margins 1e-5 / 1e-5, summary 1e-12 / 1e-9, prepare 1e-5 / 1e-6.
Problems, inputs and oracle results are built once per distinct case on the CPU and never modified;
the device matrix is derived afresh for every test, so no test sees another's cached slice index.
"""
import functools
import itertools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _logreg_util as LU
from _logreg_util import f64

pytestmark = pytest.mark.gpu

LOSS_TOL = dict(rtol=2e-5, atol=1e-6)
GRAD_TOL = dict(rtol=2e-4, atol=2e-6)
SENTINEL = -12345.0


# ------------------------------------------------------------------------------------------ harness
def _inputs(p, S, T, seed, scale=0.3, binomial=False):
    """fp32 inputs of one evaluation on the CPU (the oracle reads the same fp32 values as fp64):
    inv_std in [0.5, 1.5], one frozen column, trial points ~ N(0, scale^2)."""
    g = torch.Generator().manual_seed(seed)
    F, K = p.F, p.K
    frozen = (3 * seed + 1) % F
    inv_std = torch.rand(S, F, generator=g) + 0.5
    pmask = torch.ones(S, K, F + 1)
    pmask[:, :, frozen] = 0
    if binomial:
        pmask[:, 0, :] = 0
    rw = torch.ones(S, p.N) if p.rw is None else p.rw
    inv_wsum = (1.0 / rw.double().sum(1)).float()
    xt = torch.randn(S * T, K, F + 1, generator=g) * scale
    return SimpleNamespace(S=S, T=T, inv_std=inv_std, pmask=pmask, inv_wsum=inv_wsum, xt=xt, frozen=frozen)


def _oracle(p, a, dtype=f64):
    return LU.oracle_eval(p.X, p.y, p.rw, a.xt, a.T, a.inv_std, a.pmask, a.inv_wsum, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _built(N, K, widths, Fd, seed, S=2, T=2, weights="frac", binomial=False, mk=()):
    """(problem, inputs, fp64 oracle result) of a case, on the CPU, shared and left unchanged."""
    p = LU.make_problem(N, K, widths, Fd, seed, weights=weights, S=S, **dict(mk))
    a = _inputs(p, S, T, seed, binomial=binomial)
    return p, a, _oracle(p, a)


def _on_device(p, cuda):
    """A fresh device matrix of the problem (nothing cached on it yet)."""
    from har.features.hybrid import from_dense

    hm = from_dense(p.X.to(cuda), p.blocks)
    assert hm is not None and hm.cat.shape[1] == p.C and hm.dense.shape[1] == p.Fd
    return hm


def _solver(cuda, p, a, *, SL=None, allreduce=None, rw=None):
    from har.ops.logreg import DeviceLogregSolver, LogregDesign

    K, F = p.K, p.F
    rw = p.rw if rw is None else rw
    design = LogregDesign(_on_device(p, cuda), p.y.to(cuda), None if rw is None else rw.to(cuda), K)
    if SL is not None:
        design.SL = SL  # before anything caches col_slice on the fresh matrix
    solver = DeviceLogregSolver(design, a.S, a.T, 4, a.inv_std.to(cuda), a.pmask.to(cuda), a.inv_wsum.to(cuda),
                                torch.zeros(a.S, K * (F + 1), device=cuda), None, 1, 1e-6, allreduce=allreduce)
    _fill_weff(solver, p, a)
    return design, solver


def _fill_weff(solver, p, a):
    F, K = p.F, p.K
    spec = torch.arange(a.S * a.T) // a.T
    W = a.xt[:, :, :F] * a.inv_std[spec][:, None, :] * a.pmask[spec][:, :, :F]
    solver.weff.zero_()
    solver.weff[:, :F, :K] = W.transpose(1, 2).to(solver.weff.device)
    solver.weff[:, F, :K] = (a.xt[:, :, F] * a.pmask[spec][:, :, F]).to(solver.weff.device)


def _run(cuda, p, a, tstride=1, **kw):
    design, solver = _solver(cuda, p, a, **kw)
    solver._evaluate(tstride)
    torch.cuda.synchronize()
    return design, solver


def _check(p, a, solver, ref, models=None, loss_tol=LOSS_TOL, grad_tol=GRAD_TOL):
    """loss and gradient of ``models`` vs the oracle; the frozen column's gradient exactly 0."""
    K, F = p.K, p.F
    BT = a.S * a.T
    models = list(range(BT)) if models is None else models
    loss, G = solver.loss.cpu(), solver.G.double().cpu()
    print(f"loss err {float((loss[models] - ref.loss[models]).abs().max()):.3e}  "
          f"grad err {float((G[models] - ref.G[models]).abs().max()):.3e}  max|G| {float(ref.G.abs().max()):.3e}")
    assert bool(torch.isfinite(loss[models]).all()) and bool(torch.isfinite(G[models]).all())
    torch.testing.assert_close(loss[models], ref.loss[models], **loss_tol)
    torch.testing.assert_close(G[models], ref.G[models], **grad_tol)
    assert float(G.view(BT, K, F + 1)[models][:, :, a.frozen].abs().max()) == 0.0
    return loss, G


def _check_residuals(p, a, solver, ref, models):
    """``solver.R`` slot i holds model ``models[i]``: rows vs the oracle, padded classes exactly 0.

    Tolerance: a row's residual is w_i (p - onehot) with w_i = rw_i / wsum.  An fp32 softmax
    probability at these margins (|z| of a few units) is good to well under 2e-6 absolute, so this is
    the gradient's own tolerance (a sum over rows of total weight 1) scaled to one row's weight:
    rtol 2e-4, atol 2e-6 max_i w_i."""
    if solver.R is None:
        assert p.C == 0
        return
    K = p.K
    R = solver.R.double().cpu()[:len(models), :p.N]
    if solver.d.KP > K:
        assert float(R[:, :, K:].abs().max()) == 0.0
    rw = torch.ones(a.S, p.N) if p.rw is None else p.rw
    wmax = float((rw.double() * a.inv_wsum.double()[:, None]).max())
    torch.testing.assert_close(R[:, :, :K], ref.R[models], rtol=2e-4, atol=2e-6 * wmax)


def _case(cuda, N, K, widths, Fd, seed, *, S=2, T=2, weights="frac", binomial=False, SL=None, **mk):
    p, a, ref = _built(N, K, tuple(widths), Fd, seed, S, T, weights, binomial, tuple(sorted(mk.items())))
    design, solver = _run(cuda, p, a, SL=SL)
    _check(p, a, solver, ref)
    _check_residuals(p, a, solver, ref, list(range(S * T)))
    return p, a, design, solver, ref


# ------------------------------------------------------------------------------------------ evaluation + gradient
@pytest.mark.parametrize("K,Fd", [(6, 9), (12, 9), (16, 10), (8, 10), (8, 11), (16, 11), (3, 0), (12, 0)])
def test_eval_instantiations(cuda, K, Fd):
    """<8 | 16, narrow | wide>: KP from K (K = KP exactly at 8 and 16), the narrow tile up to 10 dense
    columns (10 / 11 is the boundary), no dense chunk at all at Fd = 0."""
    p, a, design, solver, ref = _case(cuda, 300, K, (7, 5), Fd, seed=100 + K + Fd)
    assert design.KP == (8 if K <= 8 else 16) and design.Fd == Fd and design.C == 2
    assert (design.Fd <= 10) == (Fd in (0, 9, 10))


@pytest.mark.parametrize("K,Fd", [(6, 31), (6, 32), (6, 33), (6, 64), (6, 65), (6, 70), (12, 33), (12, 65)])
def test_eval_dense_chunks(cuda, K, Fd):
    """One, two and three 32-column LDS chunks, full and ragged, with Fd % 4 != 0 zero padding."""
    p, a, design, solver, ref = _case(cuda, 300, K, (5,), Fd, seed=200 + K + Fd)
    assert design.Fd == Fd > 10 and (Fd + 31) // 32 == {31: 1, 32: 1, 33: 2, 64: 2, 65: 3, 70: 3}[Fd]


@pytest.mark.parametrize("K,C", [(6, 0), (6, 1), (6, 4), (6, 5), (6, 8), (6, 9), (6, 17), (12, 5), (12, 17)])
def test_eval_onehot_gathers(cuda, K, C):
    """C <= 4: the preloaded gather; C > 4: groups of 8 (one full group at 8, ragged last groups at 5, 9
    and 17).  Row 0 holds no category in any block."""
    p, a, design, solver, ref = _case(cuda, 300, K, (6,) * C, 3, seed=300 + K + C)
    assert design.C == C and (design.C > 4) == (C in (5, 8, 9, 17))
    assert bool((design.hm.cat[0] == -1).all()) and design.hm.cat.shape[1] == C
    if C:
        assert int((design.hm.cat >= 0).all(1).sum()) > 0  # and some rows hold one in every block


@pytest.mark.parametrize("N", [1, 63, 255, 256, 257, 513])
def test_eval_tiles(cuda, N):
    """Partial, exact and one-row last tiles of 256 rows."""
    p, a, design, solver, ref = _case(cuda, N, 6, (7, 5), 9, seed=400 + N)
    assert solver.ntiles == (N + 255) // 256


def test_eval_binomial_pivot(cuda):
    p, a, design, solver, ref = _case(cuda, 300, 2, (7, 5), 9, seed=500, binomial=True)
    G = solver.G.view(4, 2, p.F + 1)
    assert float(G[:, 0].abs().max()) == 0.0 and float(G[:, 1].abs().max()) > 0.0


def test_grad_several_column_blocks(cuda):
    """A 600-wide one-hot block with Zipf-like popularity: the first blocks are cut by the 256-slice
    limit, later ones (rare and empty categories) by the 256-column limit."""
    p, a, design, solver, ref = _case(cuda, 3000, 6, (600,), 4, seed=600, zipf=1.0)
    blk, nblk, srow = design.col_blocks()
    assert nblk > 1
    b = blk.cpu().numpy()
    assert LU.oracle_col_blocks_ok(b, srow.cpu().numpy(), design.col_slice().cpu().numpy(),
                                   design.csc_off.cpu().numpy(), design.SL)
    ncol = b[:-1, 1] - b[:-1, 0]
    assert (ncol == 256).any() and (ncol < 256).any()
    assert int((p.X[:, :600].sum(0) == 0).sum()) > 0  # empty categories among the columns


@pytest.mark.parametrize("K,SL", [(6, None), (6, 1), (6, 3), (6, 16), (12, 1), (12, 3)])
def test_grad_lone_many_slice_column(cuda, K, SL):
    """One category holds >= 4200 of 5000 rows: more than 256 slices, so a block of its own walked in
    several rounds of 256 (the later rounds re-read srow).  SL = 1 and 3 leave ragged row groups
    (RG = 8 rows for KP = 8, 4 for KP = 16).  Every case derives a fresh matrix."""
    from har.ops.logreg import SLICE_ROWS

    p, a, design, solver, ref = _case(cuda, 5000, K, (6,), 2, seed=700, SL=SL, popular=((0, (2, 0.9)),),
                                      empty=((0, 4),))
    assert design.SL == (SLICE_ROWS if SL is None else SL)
    rows = int((p.cat[:, 0] == 2).sum())
    assert rows >= 4200
    cs = design.col_slice().cpu().numpy()
    assert cs[3] - cs[2] == -(-rows // design.SL) > 256
    blk, nblk, srow = design.col_blocks()
    b = blk.cpu().numpy()
    assert LU.oracle_col_blocks_ok(b, srow.cpu().numpy(), cs, design.csc_off.cpu().numpy(), design.SL)
    assert [2, 3] in b[:, :2].tolist()  # the popular column is a block of its own
    assert float(solver.G.view(4, K, p.F + 1)[:, :, 4].abs().max()) == 0.0  # the empty category


@functools.lru_cache(maxsize=None)
def _measured(N, K, widths, Fd, seed, S, T, target, zero_tile):
    """A case whose tolerance is measured: (problem, inputs, fp64 oracle, fp32 loss error, fp32 gradient
    error) — the errors of the oracle's own lines run in fp32 torch on the CPU, max over models/entries.
    ``target``: the trial points are scaled so that max |margin| is ``target``; ``zero_tile``: rows
    256..511 get weight 0 in every spec."""
    p = LU.make_problem(N, K, widths, Fd, seed, weights="frac", S=S)
    if zero_tile:
        p.rw[:, 256:512] = 0
    a = _inputs(p, S, T, seed)
    if target:
        a.xt = a.xt * (target / float(_oracle(p, a).Z.abs().max()))
    ref = _oracle(p, a)
    r32 = _oracle(p, a, dtype=torch.float32)
    e_loss = float((r32.loss.double() - ref.loss).abs().max())
    e_grad = float((r32.G.double() - ref.G).abs().max())
    return p, a, ref, e_loss, e_grad


def _check_measured(p, a, solver, ref, e_loss, e_grad):
    loss, G = solver.loss.cpu(), solver.G.double().cpu()
    k_loss, k_grad = float((loss - ref.loss).abs().max()), float((G - ref.G).abs().max())
    print(f"fp32 torch error: loss {e_loss:.3e} grad {e_grad:.3e}; bound 4x: loss {4 * e_loss:.3e} grad "
          f"{4 * e_grad:.3e}; kernel error: loss {k_loss:.3e} grad {k_grad:.3e}; max|loss| "
          f"{float(ref.loss.abs().max()):.3e} max|G| {float(ref.G.abs().max()):.3e}")
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(G).all())
    assert e_loss > 0 and e_grad > 0
    assert k_loss <= 4 * e_loss
    assert k_grad <= 4 * e_grad
    assert float(G.view(a.S * a.T, p.K, p.F + 1)[:, :, a.frozen].abs().max()) == 0.0


def test_grad_more_than_256_tiles(cuda):
    """N = 65,837: 258 row tiles, so the loss sum reads tiles 256 and 257 straight from the slabs.

    Bound: 4x the error of the same objective evaluated in fp32 torch on the CPU against the fp64
    oracle (the factor covers the kernel's different but fixed summation order and its fast exp / log).
    Measured at this shape on the MI355X host (16 CPU threads): fp32 torch loss error 3.5e-08, gradient
    error 1.6e-07 (max |loss| 1.14, max |G| 0.089): bounds 1.4e-07 and 6.5e-07; the kernels' errors were
    2.7e-08 and 7.8e-08.  (The fp32 gradient error is that of one 65,837-long sgemm dot product per
    entry and depends on how the CPU BLAS blocks and threads it; the test measures it where it runs.)"""
    p, a, ref, e_loss, e_grad = _measured(65537 + 300, 3, (5,), 2, 800, 1, 1, 0.0, False)
    design, solver = _run(cuda, p, a)
    assert solver.ntiles == 258 > 256 and design.C == 1 and design.Fd == 2
    _check_measured(p, a, solver, ref, e_loss, e_grad)
    _check_residuals(p, a, solver, ref, [0])


def test_eval_large_margins(cuda):
    """Trial points scaled until max |z| = 60: the shifted softmax stays finite; rows of weight 0 add
    exactly 0 (changing their labels changes no bit of the loss or the gradient) and a tile of all-zero
    weights has a tile loss of exactly 0.

    Bound: 4x the fp32 torch error, as above.  Measured at this shape on the MI355X host: fp32 torch
    loss error 1.5e-06, gradient error 3.1e-07 (max |loss| 11.2, max |G| 0.71): bounds 5.9e-06 and
    1.2e-06; the kernels' errors were 3.8e-07 and 6.0e-08."""
    from har.ops.logreg import DeviceLogregSolver, LogregDesign

    p, a, ref, e_loss, e_grad = _measured(700, 6, (7, 5), 9, 900, 2, 2, 60.0, True)
    assert abs(float(ref.Z.abs().max()) - 60.0) < 1e-3
    design, solver = _run(cuda, p, a)
    _check_measured(p, a, solver, ref, e_loss, e_grad)
    SW = design.Fd * design.KP + design.KP + 1
    assert solver.slab.shape == (4, 3, SW)
    assert float(solver.slab[:, 1, SW - 1].abs().max()) == 0.0 and float(solver.slab[:, 0, SW - 1].abs().min()) > 0.0
    # other labels on the rows that weigh 0 in every spec: not a bit changes
    dead = (p.rw == 0).all(0)
    assert int(dead.sum()) >= 256
    y2 = torch.where(dead, (p.y + 1) % p.K, p.y)
    d2 = LogregDesign(_on_device(p, cuda), y2.to(cuda), p.rw.to(cuda), p.K)
    s2 = DeviceLogregSolver(d2, a.S, a.T, 4, a.inv_std.to(cuda), a.pmask.to(cuda), a.inv_wsum.to(cuda),
                            torch.zeros(a.S, p.K * (p.F + 1), device=cuda), None, 1, 1e-6)
    _fill_weff(s2, p, a)
    s2._evaluate(1)
    assert torch.equal(s2.loss, solver.loss) and torch.equal(s2.G, solver.G)


def test_eval_launch_chunks(cuda, monkeypatch):
    """S T = 6 models in one launch (default residual budget) and in three launches of two
    (model0 = 0, 2, 4; residual slot != model): bitwise the same, both equal to the oracle."""
    p, a, ref = _built(12000, 6, (7, 5), 9, 1000, 3, 2)
    d1, s1 = _run(cuda, p, a)
    assert s1.rchunk == 6 and len(s1._eval_args(1)) == 1
    monkeypatch.setenv("HAR_LR_R_BUDGET_MB", "1")
    d2, s2 = _run(cuda, p, a)
    assert s2.rchunk == 2 and [ev[15] for ev, _ in s2._eval_args(1)] == [0, 2, 4]
    assert torch.equal(s1.loss, s2.loss) and torch.equal(s1.G, s2.G)
    for s in (s1, s2):
        _check(p, a, s, ref)
    _check_residuals(p, a, s1, ref, list(range(6)))
    _check_residuals(p, a, s2, ref, [4, 5])  # the last launch's models in slots 0, 1


def test_eval_tstride_skips_the_other_trials(cuda):
    """tstride = T evaluates trial 0 of every model only; the other trials' outputs are not touched."""
    p, a, ref = _built(300, 6, (7, 5), 9, 1100, 2, 3)
    design, solver = _solver(cuda, p, a)
    solver.G.fill_(SENTINEL)
    solver.loss.fill_(SENTINEL)
    solver._evaluate(a.T)
    torch.cuda.synchronize()
    first, rest = [0, 3], [1, 2, 4, 5]
    # (the sentinel rows would fail _check's frozen-column assertion: it reads the listed models only)
    _check(p, a, solver, ref, models=first)
    _check_residuals(p, a, solver, ref, first)
    assert bool((solver.G[rest] == SENTINEL).all()) and bool((solver.loss[rest] == SENTINEL).all())


def test_eval_is_bitwise_deterministic(cuda):
    p, a, ref = _built(513, 12, (6,) * 5, 33, 1200)
    design, solver = _run(cuda, p, a)
    loss, G, R = solver.loss.clone(), solver.G.clone(), solver.R.clone()
    solver.G.fill_(SENTINEL)
    solver.loss.fill_(SENTINEL)
    solver._evaluate(1)
    assert torch.equal(loss, solver.loss) and torch.equal(G, solver.G) and torch.equal(R, solver.R)
    _check(p, a, solver, ref)


@pytest.mark.parametrize("K,Fd,C", [(12, 9, 5), (6, 33, 0)])
def test_margins_mode(cuda, K, Fd, C):
    """mode = 1: the raw margins of every model; the padded classes come out as exactly 0."""
    from har.ops.logreg import _kp, logreg_margins_native

    p, a, ref = _built(300, K, (6,) * C, Fd, 1300 + K)
    F, KP, BT = p.F, _kp(K), a.S * a.T
    spec = torch.arange(BT) // a.T
    W = torch.zeros(BT, F + 1, KP)
    W[:, :F, :K] = (a.xt[:, :, :F] * a.inv_std[spec][:, None, :] * a.pmask[spec][:, :, :F]).transpose(1, 2)
    W[:, F, :K] = a.xt[:, :, F] * a.pmask[spec][:, :, F]
    out = logreg_margins_native(_on_device(p, cuda), W.to(cuda), K, BT)
    assert out.shape == (BT, p.N, KP)
    torch.testing.assert_close(out[:, :, :K].double().cpu(), ref.Z, rtol=1e-5, atol=1e-5)
    assert float(out[:, :, K:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ loss fixed point
def test_loss_fixed_point_path(cuda):
    """With an all-reduce hook the gradient kernel writes the loss as fixed-point pieces and
    logreg_loss_decode turns them back: the same loss as the plain path within 2^-40, the pieces those
    of the Python mirror."""
    p, a, ref = _built(513, 6, (7, 5), 9, 1400)
    d1, plain = _run(cuda, p, a)
    seen = []
    d2, fx = _run(cuda, p, a, allreduce=lambda bucket: seen.append(bucket.data_ptr()))
    assert seen == [fx.bucket.data_ptr()] and fx.loss_fx.shape == (4, 5)
    assert float((fx.loss - plain.loss).abs().max()) <= 2.0 ** -40
    assert torch.equal(fx.G, plain.G)
    assert fx.loss_fx.cpu().tolist() == [LU.loss_fx_encode(v) for v in plain.loss.cpu().tolist()]
    _check(p, a, fx, ref)


def test_loss_decode_hand_made_rows(cuda):
    from har.ops import _native

    vals = [-3.25 - 2.0 ** -33, 2.0 ** 23 - 2.0 ** -20, 1.75, float("inf")]
    eight = [0.3, -1.7, 2.0 ** -40, 5e6, -5e6 + 0.125, 1e-9, 77.7, -0.001]
    rows = [LU.loss_fx_encode(v) for v in vals]
    rows.append(np.array([LU.loss_fx_encode(v) for v in eight], dtype=np.float32).sum(axis=0).tolist())
    rows.append([0.0, 0.0, 0.0, 0.0, 2.0])  # two ranks flagged
    assert rows[0][3] < 0 and rows[3] == [0.0, 0.0, 0.0, 0.0, 1.0]
    fx = torch.tensor(rows, dtype=torch.float32, device=cuda)
    out = torch.full((len(rows),), SENTINEL, dtype=f64, device=cuda)
    _native.kernels().logreg_loss_decode(fx.data_ptr(), out.data_ptr(), len(rows), _native.stream_ptr())
    got = out.cpu().tolist()
    want = [LU.loss_fx_decode(r) for r in rows]
    assert got[:3] == want[:3] and got[4] == want[4]
    assert np.isnan(got[3]) and np.isnan(got[5]) and np.isnan(want[3])
    for g, v in zip(got[:3], vals[:3]):
        assert abs(g - v) <= 2.0 ** -41
    # (exact rational arithmetic: 5e6 - 5e6 + ... would lose the small terms in a float sum)
    assert abs(Fraction(got[4]) - sum(Fraction(v) for v in eight)) <= 8 * Fraction(1, 2 ** 41)
    exact8 = sum(round(v * 2 ** 40) for v in eight)
    assert got[4] == exact8 / 2 ** 40  # the exact sum of the eight fixed-point values


def test_loss_flag_on_a_nan_row_weight(cuda):
    """A NaN row weight of spec 0: its models' encoded rows are [0, 0, 0, 0, 1] and decode to NaN; the
    models of spec 1 are untouched."""
    p, a, ref = _built(300, 6, (7, 5), 9, 1500)
    rw = p.rw.clone()
    rw[0, 5] = float("nan")
    design, fx = _run(cuda, p, a, allreduce=lambda bucket: None, rw=rw)
    rows = fx.loss_fx.cpu().tolist()
    assert rows[0] == rows[1] == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert rows[2][4] == rows[3][4] == 0.0
    loss = fx.loss.cpu()
    assert bool(torch.isnan(loss[:2]).all())
    torch.testing.assert_close(loss[2:], ref.loss[2:], **LOSS_TOL)


# ------------------------------------------------------------------------------------------ column slices
@pytest.mark.parametrize("SL", [1, 16, 1000])
@pytest.mark.parametrize("F1", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 3101])
def test_col_slices_binding(cuda, F1, SL):
    """The single-workgroup scan in rounds of 1024 columns (the carry between rounds) against the
    integer formula; column lengths include 0, 1, SL - 1, SL and SL + 1."""
    from har.ops import _native

    g = torch.Generator().manual_seed(F1 * 7 + SL)
    special = torch.tensor([0, 1, max(SL - 1, 0), SL, SL + 1, 2 * SL + 1, 5 * SL])
    lens = special[torch.randint(0, len(special), (F1,), generator=g)]
    lens[:min(F1, 5)] = special[:min(F1, 5)]
    lens[-1] = special[(F1 + SL) % 5]  # (the kernel takes any last column, not only the empty intercept one)
    off = torch.zeros(F1 + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(lens, 0)
    assert int(off[-1]) < 2 ** 31
    off_d = off.to(torch.int32).to(cuda)
    out = torch.full((F1 + 1,), -1, dtype=torch.int32, device=cuda)
    _native.kernels().logreg_col_slices(off_d.data_ptr(), F1 - 1, SL, out.data_ptr(), _native.stream_ptr())
    assert np.array_equal(out.cpu().numpy().astype(np.int64), LU.oracle_col_slices(off.numpy(), SL))


# ------------------------------------------------------------------------------------------ summarizer
@functools.lru_cache(maxsize=None)
def _summary_problem(N, Fd, C, K, weighted):
    p = LU.make_problem(N, K, (6,) * C, Fd, 1600 + N, weights="frac" if weighted else "none", S=2,
                        empty=((0, 2),), const_dense=(1 if Fd else None))
    return p, LU.oracle_summary(p.X, p.y, p.rw, K)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N,Fd,C,K", [(1, 3, 1, 2), (255, 0, 2, 6), (256, 9, 2, 6), (257, 33, 1, 12),
                                      (1800, 65, 5, 16)])
def test_summary_kernels(cuda, N, Fd, C, K, weighted):
    """Both summary kernels through LogregDesign.summary(): several dense chunks and none, N around the
    256-row tile, a constant dense column and an empty category."""
    from har.ops.logreg import LogregDesign

    p, want = _summary_problem(N, Fd, C, K, weighted)
    design = LogregDesign(_on_device(p, cuda), p.y.to(cuda), None if p.rw is None else p.rw.to(cuda), K)
    assert design.native and design.S == (2 if weighted else 1)
    got = design.summary().cpu()
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-9)
    F = p.F
    assert float(got[:, 1 + 2].abs().max()) == 0.0 and float(got[:, 1 + F + 2].abs().max()) == 0.0  # empty category
    if Fd:  # the constant column: sums that are exactly 2 and 4 times the weight sum
        j = F - Fd + 1
        assert torch.equal(got[:, 1 + j], 2 * got[:, 0]) and torch.equal(got[:, 1 + F + j], 4 * got[:, 0])


def _summary_direct(cuda, p, K, use_srow, SL=None):
    """The two summary launches through the binding (argument order: ops/logreg.py summary())."""
    from har.ops import _native
    from har.ops.logreg import LogregDesign

    d = LogregDesign(_on_device(p, cuda), p.y.to(cuda), None if p.rw is None else p.rw.to(cuda), K)
    if SL is not None:
        d.SL = SL
    mod, st = _native.kernels(), _native.stream_ptr()
    S_ = d.S
    nt = mod.logreg_summary_tiles(d.N)
    part = torch.empty(S_, max(1, nt), 2 * d.Fd + K + 1, dtype=f64, device=cuda)
    out = torch.full((S_, 1 + 2 * d.F + K), SENTINEL, dtype=f64, device=cuda)
    cs = d.col_slice()
    srow = d.col_blocks()[2]
    for ph in (0, 1):
        mod.logreg_summary(ph, d.dense.data_ptr(), d.dense.stride(0), d.Fd, d.y32.data_ptr(), d.rw_ptr(), d.N, d.F, K,
                           S_, d.col_map.data_ptr(), d.csc_rows.data_ptr(), d.csc_off.data_ptr(), cs.data_ptr(), d.SL,
                           nt, part.data_ptr(), out.data_ptr(), srow.data_ptr() if use_srow else 0, st)
    torch.cuda.synchronize()
    return d, out.cpu()


@pytest.mark.parametrize("K", [64, 100, 255])
def test_summary_many_classes_direct(cuda, K):
    """K >= 64: one 256-row chain per class sum instead of four parts (no Python caller gets here: more
    than 16 classes run the torch objective).  Class sums and weight sum, and the rest of the row."""
    p = LU.make_problem(300, K, (5,), 3, 1700 + K, weights="frac", S=2)
    assert len(torch.unique(p.y)) > 16
    d, got = _summary_direct(cuda, p, K, True)
    want = LU.oracle_summary(p.X, p.y, p.rw, K)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-9)
    assert got.shape == (2, 1 + 2 * p.F + K)
    torch.testing.assert_close(got[:, 1 + 2 * p.F:].sum(1), got[:, 0], rtol=1e-12, atol=1e-9)


def test_summary_slice_search_equals_srow_table(cuda):
    """Without the per-slice row table the column kernel finds a slice's column by binary search (no
    Python caller passes srow = 0): bitwise the same rows, over columns spanning more than 256 slices
    (several rounds), with an empty category in the middle."""
    p = LU.make_problem(5000, 6, (40, 7), 3, 1800, weights="frac", S=2, empty=((0, 11),), popular={0: (20, 0.3)})
    d, a = _summary_direct(cuda, p, 6, True)
    assert int(d.col_slice()[p.F]) > 256
    _, b = _summary_direct(cuda, p, 6, False)
    assert torch.equal(a, b)
    torch.testing.assert_close(a, LU.oracle_summary(p.X, p.y, p.rw, 6), rtol=1e-12, atol=1e-9)


# ------------------------------------------------------------------------------------------ prepare
@pytest.mark.parametrize("binomial,standardization,fit_intercept,weighted",
                         list(itertools.product([False, True], [True, False], [True, False], [False, True])))
def test_prepare_kernel(cuda, binomial, standardization, fit_intercept, weighted):
    """LogisticRegression._setup on the GPU (summary + prepare kernels) against the fp64 oracle; the
    weighted cases add a spec whose weights sum to 0.5 (variance divisor max(wsum - 1, 1) = 1).  The
    design has an empty category and a constant dense column: frozen, every entry exactly 0."""
    from har.models.logreg import FitSpec, LogisticRegression

    K = 2 if binomial else 6
    p = LU.make_problem(300, K, (6, 5), 4, 1900, empty=((0, 2),), weights="frac" if weighted else "none", S=2,
                        const_dense=1)
    regs, alphas = [0.1, 0.3], [0.0, 0.2]
    rws = [None, None] if p.rw is None else [p.rw[0], p.rw[1]]
    if weighted:
        rws.append(p.rw[1] * (0.5 / p.rw[1].double().sum()).float())
        regs, alphas = regs + [0.2], alphas + [0.5]
        assert float(rws[2].double().sum()) <= 1.0
    B = len(rws)
    specs = [FitSpec(None if w is None else w.to(cuda), regs[i], alphas[i]) for i, w in enumerate(rws)]
    est = LogisticRegression(standardization=standardization, fitIntercept=fit_intercept)
    g = est._setup(_on_device(p, cuda), p.y.to(cuda), specs, K, None)
    assert g[0].native and g[1] == binomial and g[2] == K
    rw = torch.ones(B, p.N) if p.rw is None else torch.stack(rws)
    summ = LU.oracle_summary(p.X, p.y, rw, K)
    want = LU.oracle_prepare(summ, regs, alphas, K, K, standardization, fit_intercept, binomial)
    got = [t.double().cpu().reshape(w.shape) for t, w in zip(g[3:], want)]
    for name, t, w in zip(("inv_std", "inv_wsum", "pmask", "l2", "l1", "x0"), got, want):
        print(f"{name}: max abs err {float((t - w).abs().max()):.3e}")
        torch.testing.assert_close(t, w, rtol=1e-5, atol=1e-6, msg=lambda m, n=name: f"{n}: {m}")
    frozen = [2, p.F - p.Fd + 1]
    assert float(got[0][:, frozen].abs().max()) == 0.0
    for t in (got[2], got[3].view(B, K, -1), got[4].view(B, K, -1), got[5]):
        assert float(t[:, :, frozen].abs().max()) == 0.0
    live = [c for c in range(p.F) if c not in frozen]
    assert float(got[0][:, live].min()) > 0.0  # nothing else is frozen (the wsum <= 1 spec included)
