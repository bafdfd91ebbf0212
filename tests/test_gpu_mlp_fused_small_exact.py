"""csrc/kernels/mlp_fused.hip (mlp_fwd_head, mlp_fwd_infer, mlp_fwd_infer_f32) and mlp_small.hip (mlp_small_step)
called directly on the exact-arithmetic data of tests/_mlp_exact_util.py: equalities against the fp64 oracle,
element by element and per workgroup slab, every output inside sentinel-filled guard bands.  The one tolerance is
the loss of the unsaturated tie cases (ln C): the criterion of test_gpu_mlp_head_opt.py."""
import math
from types import SimpleNamespace

import pytest
import torch

import _gemm_util as GU
import _mlp_exact_util as MU
from _mlp_exact_util import bf16, f32, f64

pytestmark = pytest.mark.gpu
i32 = torch.int32


def _mod():
    from har.ops import _native
    return _native.kernels(), _native.stream_ptr()


def _loss_ok(tag, got, B, C):
    got, ref = float(got.to(f64).sum()), B * math.log(C)
    assert math.isfinite(got) and abs(got - ref) <= 1e-4 * ref + 1e-5 * B, f"{tag}: loss {got} vs {ref}"


@pytest.mark.parametrize("k", MU.cases_of("fwd_head") + MU.cases_of("fwd_head", tie=True), ids=MU.case_id)
def test_fwd_head_exact(cuda, k):
    _, B, K0, H, C, tie = k
    mod, s = _mod()
    c, o = MU.get_case(k)
    d, tag = MU.dev_case(c, cuda), MU.case_id(k)
    nwg, w = MU.fwd_head_grid(B), MU.fwd_head_slab_width(H)
    assert mod.mlp_fwd_head_grid(B) == nwg
    h1, dact = GU.guarded(B, H, bf16, cuda, ld=H), GU.guarded(B, H, bf16, cuda, ld=H)
    slab = GU.guarded(nwg, 16 * H + 16, f32, cuda, ld=w)   # (the H floats after dbout are not written)
    loss, corr = GU.guarded(1, nwg, f32, cuda, ld=nwg), GU.guarded(1, nwg, f32, cuda, ld=nwg)
    mod.mlp_fwd_head(d.X.data_ptr(), K0, d.W0.data_ptr(), d.b0.data_ptr(), d.W1.data_ptr(), d.b1.data_ptr(), H,
                     d.Wout.data_ptr(), d.bout.data_ptr(), d.y.data_ptr(), B, C, c.scale, h1.view.data_ptr(),
                     dact.view.data_ptr(), slab.view.data_ptr(), loss.view.data_ptr(), corr.view.data_ptr(), s)
    torch.cuda.synchronize()
    GU.assert_equal(h1.result(), o.h1.to(bf16), tag + " h1")
    GU.assert_equal(dact.result(), o.dact2.to(bf16), tag + " dact2")
    want = torch.zeros(nwg, 16 * H + 16, dtype=f32)
    wl, wc = torch.zeros(nwg, dtype=f64), torch.zeros(nwg, dtype=i32)
    for g in range(nwg):
        rows = MU.fwd_head_rows(B, g)
        gr = MU.grads(c, o, rows)
        want[g, :16 * H], want[g, 16 * H:] = MU.to_f32(gr["Wout"]).reshape(-1), MU.to_f32(gr["bout"])
        wl[g], wc[g] = o.loss[rows].sum(), int(o.correct[rows].sum())
    got = slab.result()
    GU.assert_equal(got, want, tag + " dWout / dbout slabs")
    assert float(got[:, :16 * H].view(nwg, 16, H)[:, C:].abs().sum()) == 0 and float(got[:, 16 * H + C:].abs().sum()) == 0
    GU.assert_equal(corr.out[0].view(i32), wc, tag + " block_correct")
    if tie:
        _loss_ok(tag, loss.result(), B, C)
        assert int(wc.sum()) == int((c.y == 0).sum()) and float(o.dact2.abs().max()) == 0
    else:
        GU.assert_equal(loss.result()[0], MU.to_f32(wl), tag + " block_loss")
    for buf in (h1, dact, slab, loss, corr):
        buf.check(tag)


@pytest.mark.parametrize("k", MU.cases_of("small") + MU.cases_of("small", tie=True), ids=MU.case_id)
def test_small_step_exact(cuda, k):
    _, B, K0, H, C, tie = k
    mod, s = _mod()
    c, o = MU.get_case(k)
    d, tag = MU.dev_case(c, cuda), MU.case_id(k)
    offs = MU.flat_offsets(K0, H)
    total, nt = offs["total"], B // 32
    assert mod.mlp_small_step_max_batch() == 512
    pb = torch.zeros(total, dtype=bf16, device=cuda)
    pb[offs["W0"][0]:offs["W0"][0] + H * K0] = d.W0.reshape(-1)
    pb[offs["W1"][0]:offs["W1"][0] + H * H] = d.W1.reshape(-1)
    wf = GU.guarded(1, H * K0 + 2 * H * H, bf16, cuda, ld=H * K0 + 2 * H * H)
    mod.mlp_pack_frag(pb.data_ptr(), wf.view.data_ptr(), offs["W0"][0], offs["W1"][0], K0, H, s)
    slab = GU.guarded(nt, total, f32, cuda, ld=total)
    loss, corr = GU.guarded(1, nt, f32, cuda, ld=nt), GU.guarded(1, nt, f32, cuda, ld=nt)
    G, P, m, v = (torch.zeros(total, dtype=f32, device=cuda) for _ in range(4))
    step = torch.full((1,), 5, dtype=i32, device=cuda)

    def run(B_):
        mod.mlp_small_step(d.X.data_ptr(), K0, wf.view.data_ptr(), d.b0.data_ptr(), d.b1.data_ptr(), H, d.Wout.data_ptr(),
                           d.bout.data_ptr(), d.y.data_ptr(), B_, C, c.scale, slab.view.data_ptr(), total,
                           *(offs[n][0] for n in ("W0", "b0", "W1", "b1", "Wout", "bout")), loss.view.data_ptr(),
                           corr.view.data_ptr(), step.data_ptr(), G.data_ptr(), P.data_ptr(), m.data_ptr(),
                           v.data_ptr(), pb.data_ptr(), 0.0, 0.9, 0.999, 1e-8, 0.0, step.data_ptr(), s)
        torch.cuda.synchronize()

    if B == 512:   # one tile past the largest batch is refused and writes nothing
        with pytest.raises(RuntimeError, match="contract violation code -2$"):
            run(544)
        torch.cuda.synchronize()
        for buf in (slab, loss, corr):
            assert bool((buf.flat.view(i32) == buf.sentinel).all())
        assert int(step.item()) == 5
    run(B)
    want = torch.stack([MU.flat_grad(c, MU.grads(c, o, slice(r, r + 32))) for r in range(0, B, 32)])
    got = slab.result()
    for name in ("W0", "b0", "W1", "b1", "Wout", "bout"):
        a, shape = offs[name]
        n = int(torch.tensor(shape).prod())
        GU.assert_equal(got[:, a:a + n].reshape(nt, *shape), want[:, a:a + n].reshape(nt, *shape), f"{tag} d{name} slabs")
    assert float(got[:, :H * K0].reshape(nt, H, K0)[:, :, c.F:].abs().sum()) == 0
    wo = offs["Wout"][0]
    assert float(got[:, wo:wo + 16 * H].reshape(nt, 16, H)[:, C:].abs().sum()) == 0 and float(got[:, wo + 16 * H + C:].abs().sum()) == 0
    wc = torch.tensor([int(o.correct[r:r + 32].sum()) for r in range(0, B, 32)], dtype=i32)
    GU.assert_equal(corr.out[0].view(i32), wc, tag + " block_correct")
    if tie:
        _loss_ok(tag, loss.result(), B, C)
        assert int(wc.sum()) == int((c.y == 0).sum())
    else:
        wl = torch.stack([o.loss[r:r + 32].sum() for r in range(0, B, 32)])
        GU.assert_equal(loss.result()[0], MU.to_f32(wl), tag + " block_loss")
    assert int(step.item()) == 6
    for buf in (slab, loss, corr, wf):
        buf.check(tag)


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("K0", [32, 64])
@pytest.mark.parametrize("C,tie", [(6, False), (16, False), (16, True)])
@pytest.mark.parametrize("f32_in", [False, True], ids=["bf16", "f32"])
def test_fwd_infer_exact(cuda, H, K0, C, tie, f32_in):
    B = 48
    mod, s = _mod()
    c, o = MU.get_case(("fwd_head", B, K0, H, C, False))
    if tie:   # the last class repeats class 0: every row whose maximum they are is a tie -> the lower index
        import copy
        c = copy.copy(c)
        c.Wout, c.bout = c.Wout.clone(), c.bout.clone()
        c.Wout[C - 1], c.bout[C - 1] = c.Wout[0], c.bout[0]
        z = o.h2 @ c.Wout[:C].T + c.bout[:C]   # (the hidden layers do not depend on the head)
        o = SimpleNamespace(z=z, argmax=MU.first_argmax(z))
        assert bool((o.z[:, 0] == o.z[:, C - 1]).all()) and bool((o.argmax == 0).any()) and not bool((o.argmax == C - 1).any())
    d = MU.dev_case(c, cuda)
    logits, pred = GU.guarded(B, C, f32, cuda, ld=C), GU.guarded(1, B, f32, cuda, ld=B)
    net = (d.W0.data_ptr(), d.b0.data_ptr(), d.W1.data_ptr(), d.b1.data_ptr(), H, d.Wout.data_ptr(), d.bout.data_ptr(), B, C,
           logits.view.data_ptr(), pred.view.data_ptr(), s)
    if f32_in:   # raw features at a pitch above F, the columns >= F of the source rows poisoned
        ldx = c.F + 5
        Xf = torch.full((B, ldx), 7.0, dtype=f32)
        Xf[:, :c.F] = c.X[:, :c.F].to(f32)
        Xf = Xf.to(cuda)
        mod.mlp_fwd_infer_f32(Xf.data_ptr(), ldx, c.F, K0, *net)
    else:
        mod.mlp_fwd_infer(d.X.data_ptr(), K0, *net)
    torch.cuda.synchronize()
    tag = f"infer H {H} K0 {K0} C {C} tie {tie} f32 {f32_in}"
    GU.assert_equal(logits.result(), MU.to_f32(o.z), tag + " logits")
    GU.assert_equal(pred.out[0].view(i32).cpu(), o.argmax.to(i32), tag + " pred")
    logits.check(tag)
    pred.check(tag)
