"""csrc/kernels/mlp_step.hip (mlp_step_fwd, mlp_step_bwd, mlp_step_fwd_infer) and mlp_pack_frag called directly
through their raw-pointer bindings, on the exact-arithmetic data of tests/_mlp_exact_util.py: every fp32
accumulation is exact in any order, so every output has one correct bit pattern and every comparison is an
equality against the fp64 oracle (no tolerance), element by element, per workgroup slab and per row slice.
Every output lies in a sentinel-filled buffer with guard bands (``_gemm_util.guarded``).

The one exception is the loss of the unsaturated tie cases (ln C is no fp32 sum): the criterion of
test_gpu_mlp_head_opt.py, 1e-4 relative + 1e-5 per row.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import _gemm_util as GU
import _mlp_exact_util as MU
from _mlp_exact_util import bf16, f32, f64

pytestmark = pytest.mark.gpu
H = 256
i32 = torch.int32


def _mod():
    from har.ops import _native
    return _native.kernels(), _native.stream_ptr()


def _same_bits(got, want, tag):
    GU.assert_equal(MU.bits16(got.cpu()), MU.bits16(want.cpu()), tag)


class Net:
    """The case's operands on the device and its fragment copies Wf = [W0 | W1 | W1^T] inside guard bands."""

    def __init__(self, c, dev, w1t=True):
        mod, s = _mod()
        self.c, self.dev, self.d = c, dev, MU.dev_case(c, dev)
        K0 = c.K0
        self.n0, self.n1 = H * K0, H * H
        self.pb = torch.cat([self.d.W0.reshape(-1), self.d.W1.reshape(-1)]).contiguous()
        self.ref = GU.guarded(1, self.n0 + 2 * self.n1, bf16, dev, ld=self.n0 + 2 * self.n1)   # all three copies packed
        mod.mlp_pack_frag(self.pb.data_ptr(), self.ref.view.data_ptr(), 0, self.n0, K0, H, s)
        self.wf = GU.guarded(1, self.n0 + 2 * self.n1, bf16, dev, ld=self.n0 + 2 * self.n1)
        self.wf.out[0, :self.n0 + (2 if w1t else 1) * self.n1] = self.ref.out[0, :self.n0 + (2 if w1t else 1) * self.n1]
        torch.cuda.synchronize()

    def head(self):   # (K0, Wf, b0, b1, H, Wo, bo) of the forwards
        d = self.d
        return (self.c.K0, self.wf.view.data_ptr(), d.b0.data_ptr(), d.b1.data_ptr(), H, d.Wout.data_ptr(), d.bout.data_ptr())


def _fwd(net, scale=None):
    """One mlp_step_fwd into fresh guarded outputs: (dact2, slab, loss, correct)."""
    mod, s = _mod()
    c, dev = net.c, net.dev
    B, nwg = c.B, MU.step_grid(c.B)
    dact2 = GU.guarded(B, H, bf16, dev, ld=H)
    slab = GU.guarded(nwg, MU.step_fwd_slab_width(H), f32, dev, ld=MU.step_fwd_slab_width(H))
    loss, corr = GU.guarded(1, nwg, f32, dev, ld=nwg), GU.guarded(1, nwg, f32, dev, ld=nwg)
    mod.mlp_step_fwd(net.d.X.data_ptr(), *net.head(), net.d.y.data_ptr(), B, c.C, c.scale if scale is None else scale,
                     dact2.view.data_ptr(), slab.view.data_ptr(), loss.view.data_ptr(), corr.view.data_ptr(), s)
    torch.cuda.synchronize()
    return dact2, slab, loss, corr


def _check_fwd(k, cuda):
    kind, B, K0, _, C, tie = k
    c, o = MU.get_case(k)
    tag = MU.case_id(k)
    assert _mod()[0].mlp_step_grid(B) == MU.step_grid(B) and _mod()[0].mlp_step_fwd_slab_width(H) == MU.step_fwd_slab_width(H)
    net = Net(c, cuda, w1t=False)   # the W1^T part holds the sentinel: the forward must write all of it
    dact2, slab, loss, corr = _fwd(net)
    # dact2, element by element
    GU.assert_equal(MU.unswizzle_dact2(dact2.result()), o.dact2.to(bf16), tag + " dact2")
    dact2.check(tag + " dact2")
    # per-workgroup slabs
    nwg = MU.step_grid(B)
    want = torch.zeros(nwg, MU.step_fwd_slab_width(H), dtype=f32)
    wl, wc = torch.zeros(nwg, dtype=f64), torch.zeros(nwg, dtype=i32)
    for w in range(nwg):
        rows = MU.step_fwd_rows(B, w)
        g = MU.grads(c, o, rows)
        want[w, :16 * H] = MU.to_f32(g["Wout"]).reshape(-1)
        want[w, 16 * H:] = MU.to_f32(g["bout"])
        wl[w], wc[w] = o.loss[rows].sum(), int(o.correct[rows].sum())
    got = slab.result()
    GU.assert_equal(got, want, tag + " dWout / dbout slabs")
    assert float(got[:, :16 * H].view(nwg, 16, H)[:, C:].abs().sum()) == 0 and float(got[:, 16 * H + C:].abs().sum()) == 0
    slab.check(tag + " slab")
    GU.assert_equal(corr.out[0].view(i32), wc, tag + " block_correct")
    if tie:   # ln C: the head test's criterion
        got_loss, ref = float(loss.result().to(f64).sum()), B * math.log(C)
        assert math.isfinite(got_loss) and abs(got_loss - ref) <= 1e-4 * ref + 1e-5 * B, f"{tag}: loss {got_loss} vs {ref}"
        assert int(wc.sum()) == int((c.y == 0).sum()) and float(o.dact2.abs().max()) == 0
    else:
        GU.assert_equal(loss.result()[0], MU.to_f32(wl), tag + " block_loss")
    loss.check(tag + " loss")
    corr.check(tag + " correct")
    # Wf: W0 / W1 unchanged, W1^T bit-identical to what mlp_pack_frag writes, nothing beside
    _same_bits(net.wf.out[0], net.ref.out[0], tag + " Wf")
    net.wf.check(tag + " Wf")
    return net, dact2, slab


@pytest.mark.parametrize("k", MU.cases_of("step_fwd"), ids=MU.case_id)
def test_step_fwd_exact(cuda, k):
    _check_fwd(k, cuda)


@pytest.mark.parametrize("k", MU.cases_of("step_fwd", tie=True), ids=MU.case_id)
def test_step_fwd_tie_exact(cuda, k):
    """All logits of a row equal: p = 1 / C, dz = scale (1 / C - onehot(y)), dact2 = 0, the argmax is class 0."""
    _check_fwd(k, cuda)


def _bwd(net, dact2, fslab, stride, tick, gout=True):
    mod, s = _mod()
    c, dev = net.c, net.dev
    offs, S = MU.flat_offsets(c.K0, H), MU.step_slices(c.B)
    slabs = GU.guarded(S, offs["total"], f32, dev, ld=stride)
    gwo, gbo = GU.guarded(16, H, f32, dev, ld=H), GU.guarded(1, 16, f32, dev, ld=16)
    base = slabs.view.data_ptr()
    mod.mlp_step_bwd(dact2.view.data_ptr(), net.d.X.data_ptr(), c.K0, net.wf.view.data_ptr(), H, net.d.b0.data_ptr(), c.B,
                     *(base + 4 * offs[n][0] for n in ("W1", "W0", "b0", "b1")), stride,
                     tick.data_ptr() if tick is not None else 0, fslab.view.data_ptr() if gout else 0,
                     MU.step_fwd_slab_width(H), gwo.view.data_ptr() if gout else 0, gbo.view.data_ptr() if gout else 0, s)
    torch.cuda.synchronize()
    return slabs, gwo, gbo


@pytest.mark.parametrize("k", MU.cases_of("step_bwd"), ids=MU.case_id)
def test_step_bwd_exact(cuda, k):
    _, B, K0, _, C, _ = k
    c, o = MU.get_case(k)
    tag = MU.case_id(k)
    mod, _ = _mod()
    S = MU.step_slices(B)
    assert mod.mlp_step_slices(B) == S
    net, dact2, fslab = _check_fwd(k, cuda)   # teacher-forced from the kernel's own dact2 (== the oracle's)
    offs = MU.flat_offsets(K0, H)
    total, wo = offs["total"], offs["Wout"][0]
    want = torch.stack([MU.flat_grad(c, MU.grads(c, o, slice(*MU.step_bwd_rows(B, s)))) for s in range(S)])
    empty = [s for s in range(S) if MU.step_bwd_rows(B, s)[0] == MU.step_bwd_rows(B, s)[1]]
    assert len(empty) == {64: 0, 128: 0, 1088: 7, 2560: 2, 4160: 3}[B]
    assert all(float(want[s].abs().sum()) == 0 for s in empty)   # an empty slice writes zero partials
    gtot = MU.grads(c, o, slice(0, B))
    runs = []
    for stride in (total, total + 36):
        tick = torch.full((1,), 5, dtype=i32, device=cuda)
        slabs, gwo, gbo = _bwd(net, dact2, fslab, stride, tick)
        t = f"{tag} stride {stride}"
        got = slabs.result()
        for name in ("W1", "W0", "b0", "b1"):
            a, shape = offs[name]
            n = int(torch.tensor(shape).prod())
            GU.assert_equal(got[:, a:a + n].reshape(S, *shape), want[:, a:a + n].reshape(S, *shape), f"{t} d{name} partials")
        w0 = got[:, :H * K0].reshape(S, H, K0)
        assert float(w0[:, :, c.F:].abs().sum()) == 0, t
        # the Wout / bout part of every slab, the gaps between slabs and the guards keep the sentinel
        assert bool((got[:, wo:].contiguous().view(i32) == slabs.sentinel).all()), t
        slabs.check(t + " slabs")
        GU.assert_equal(gwo.result(), MU.to_f32(gtot["Wout"]), t + " gwo")
        GU.assert_equal(gbo.result()[0], MU.to_f32(gtot["bout"]), t + " gbo")
        gwo.check(t + " gwo")
        gbo.check(t + " gbo")
        assert int(tick.item()) == 6, t
        runs.append(got)
    assert torch.equal(runs[0].view(i32), runs[1].view(i32))
    # again: bit-identical; no tick pointer, no forward slabs: gwo / gbo untouched
    slabs, gwo, gbo = _bwd(net, dact2, fslab, total, None, gout=False)
    assert torch.equal(slabs.flat.view(i32), _bwd(net, dact2, fslab, total, None, gout=False)[0].flat.view(i32))
    assert torch.equal(slabs.result()[:, :wo].contiguous().view(i32), runs[0][:, :wo].contiguous().view(i32))
    for g in (gwo, gbo):
        assert bool((g.flat.view(i32) == g.sentinel).all())


INFER = [(B, K0, C) for K0 in (32, 64) for B, C in ((64, 1), (64, 16), (192, 6))]


@pytest.mark.parametrize("B,K0,C,tie", [(*i, False) for i in INFER] + [(*i, True) for i in INFER if i[2] > 1])
def test_step_fwd_infer_exact(cuda, B, K0, C, tie):
    mod, s = _mod()
    c, o = MU.get_case(("step_fwd", B, K0, H, C, False))
    if tie:   # two identical Wout rows and biases: every row whose maximum is one of them is a tie -> the lower index
        import copy
        c = copy.copy(c)
        c.Wout, c.bout = c.Wout.clone(), c.bout.clone()
        hi = 1 if C == 6 else C - 1
        c.Wout[hi], c.bout[hi] = c.Wout[0], c.bout[0]
        z = o.h2 @ c.Wout[:C].T + c.bout[:C]   # (the hidden layers do not depend on the head)
        o = SimpleNamespace(z=z, argmax=MU.first_argmax(z))
        assert bool((o.z[:, 0] == o.z[:, hi]).all()) and int((o.argmax == 0).sum()) >= B // 16 and not bool((o.argmax == hi).any())
    net = Net(c, cuda)
    logits, pred = GU.guarded(B, C, f32, cuda, ld=C), GU.guarded(1, B, f32, cuda, ld=B)
    mod.mlp_step_fwd_infer(net.d.X.data_ptr(), *net.head(), B, C, logits.view.data_ptr(), pred.view.data_ptr(), s)
    torch.cuda.synchronize()
    tag = f"infer B {B} K0 {K0} C {C} tie {tie}"
    GU.assert_equal(logits.result(), MU.to_f32(o.z), tag + " logits")
    GU.assert_equal(pred.out[0].view(i32).cpu(), o.argmax.to(i32), tag + " pred")
    logits.check(tag)
    pred.check(tag)
    _same_bits(net.wf.out[0], net.ref.out[0], tag + " Wf")


@pytest.mark.parametrize("K0", [32, 64])
def test_pack_frag_copies_bits(cuda, K0):
    """W1 = all 65,536 bit patterns (NaNs included: the kernel copies bits), W0 = distinct patterns: each fragment
    copy is a permutation of its source, the W1^T copy is the W1 copy of the transposed matrix, W0 / W1 are found
    at their flat offsets and nothing else is written.  (Where each element goes: the forward equalities above.)"""
    mod, s = _mod()
    g = torch.Generator().manual_seed(K0)
    n0, n1 = H * K0, H * H
    w1 = torch.randperm(65536, generator=g).to(torch.int32).sub(32768).to(torch.int16).view(H, H)
    w0 = (torch.randperm(65536, generator=g)[:n0].to(torch.int32) - 32768).to(torch.int16).view(H, K0)
    o0, o1 = 8, 8 + n0 + 260   # 4-aligned flat offsets with a gap
    outs = []
    for W1 in (w1, w1.T.contiguous()):
        pb = torch.full((o1 + n1 + 8,), 0x1234, dtype=torch.int16)
        pb[o0:o0 + n0], pb[o1:o1 + n1] = w0.reshape(-1), W1.reshape(-1)
        dst = GU.guarded(1, n0 + 2 * n1, bf16, cuda, ld=n0 + 2 * n1)
        mod.mlp_pack_frag(pb.to(cuda).data_ptr(), dst.view.data_ptr(), o0, o1, K0, H, s)
        torch.cuda.synchronize()
        dst.check(f"pack_frag K0 {K0}")
        outs.append(MU.bits16(dst.result()[0]))
    a, b = outs
    assert torch.equal(a[:n0].sort().values, w0.reshape(-1).sort().values)
    for part in (a[n0:n0 + n1], a[n0 + n1:]):
        assert torch.equal(part.sort().values, torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16))
    assert torch.equal(a[n0 + n1:], b[n0:n0 + n1]) and torch.equal(b[n0 + n1:], a[n0:n0 + n1]) and torch.equal(a[:n0], b[:n0])
    assert not torch.equal(a[n0:n0 + n1], a[n0 + n1:])


@pytest.mark.parametrize("w1t", [0, 1])
def test_refresh_writes_w1t_copy_only_when_asked(cuda, w1t):
    """MlpFragSpec.w1t belongs to the reduction / Adam kernel (mlp_pack_frag always writes all three copies): its
    refresh mode with w1t = 0 leaves the W1^T region's sentinel, with w1t = 1 it writes what mlp_pack_frag writes."""
    mod, s = _mod()
    c, _ = MU.get_case(("step_fwd", 64, 32, H, 6, False))
    net = Net(c, cuda)
    n0, n1 = net.n0, net.n1
    n = n0 + n1
    param = net.pb.float()
    pbo = GU.guarded(1, n, bf16, cuda, ld=n)
    dst = GU.guarded(1, n0 + 2 * n1, bf16, cuda, ld=n0 + 2 * n1)
    z = torch.zeros(4, dtype=f32, device=cuda)
    step = torch.ones(1, dtype=i32, device=cuda)
    mod.grad_reduce_adam([], [], [], [], [], n, z.data_ptr(), param.data_ptr(), z.data_ptr(), z.data_ptr(),
                         pbo.view.data_ptr(), 0.0, 0.9, 0.999, 1e-8, 0.0, step.data_ptr(), 0, 8, s, dst.view.data_ptr(), 0, n0,
                         c.K0, H, w1t)
    torch.cuda.synchronize()
    _same_bits(pbo.result()[0], net.pb, "refreshed bf16 copy")
    got, ref = MU.bits16(dst.result()[0]), MU.bits16(net.ref.result()[0])
    assert torch.equal(got[:n], ref[:n])
    if w1t:
        assert torch.equal(got[n:], ref[n:])
    else:
        assert bool((got[n:] == torch.tensor(GU.BF16_SENTINEL, dtype=torch.int16)).all())
    dst.check("refresh")
    pbo.check("refresh pb")
    assert int(step.item()) == 1


# ------------------------------------------------------------------------------------------ argument contract
def _refused(code, call):
    with pytest.raises(RuntimeError, match=f"contract violation code {code}$"):
        call()
    torch.cuda.synchronize()


def test_step_contract(cuda):
    """Refused calls (-2 shapes, -3 16-byte alignment) write nothing; their closest accepted neighbours (B = 64, C = 1
    and 16, K0 = 32 and 64, slab_stride = H H + ..., fslab_w = the slab width) are the cases above."""
    mod, s = _mod()
    k = ("step_fwd", 64, 32, H, 6, False)
    c, o = MU.get_case(k)
    net = Net(c, cuda)
    d, B, C, K0 = net.d, c.B, c.C, c.K0
    nwg, fw, offs = MU.step_grid(B), MU.step_fwd_slab_width(H), MU.flat_offsets(K0, H)
    dact2, slab = GU.guarded(B, H, bf16, cuda, ld=H), GU.guarded(nwg, fw, f32, cuda, ld=fw)
    loss, corr = GU.guarded(1, nwg, f32, cuda, ld=nwg), GU.guarded(1, nwg, f32, cuda, ld=nwg)
    logits, pred = GU.guarded(B, C, f32, cuda, ld=C), GU.guarded(1, B, f32, cuda, ld=B)
    slabs = GU.guarded(1, offs["total"], f32, cuda, ld=offs["total"])
    gwo, gbo = GU.guarded(16, H, f32, cuda, ld=H), GU.guarded(1, 16, f32, cuda, ld=16)
    tick = torch.full((1,), 5, dtype=i32, device=cuda)
    X, wf, b0, b1, wo, bo, y = (t.data_ptr() for t in (d.X, net.wf.view, d.b0, d.b1, d.Wout, d.bout, d.y))

    def fwd(X=X, K0=K0, wf=wf, b0=b0, b1=b1, Hh=H, wo=wo, B=B, C=C, d2=dact2.view.data_ptr(), sl=slab.view.data_ptr()):
        return lambda: mod.mlp_step_fwd(X, K0, wf, b0, b1, Hh, wo, bo, y, B, C, c.scale, d2, sl, loss.view.data_ptr(),
                                        corr.view.data_ptr(), s)

    def infer(X=X, K0=K0, wf=wf, b0=b0, Hh=H, wo=wo, B=B, C=C, lg=logits.view.data_ptr(), pr=pred.view.data_ptr()):
        return lambda: mod.mlp_step_fwd_infer(X, K0, wf, b0, b1, Hh, wo, bo, B, C, lg, pr, s)

    base = slabs.view.data_ptr()
    g = {n: base + 4 * offs[n][0] for n in ("W1", "W0", "b0", "b1")}

    def bwd(d2=dact2.view.data_ptr(), X=X, K0=K0, wf=wf, Hh=H, B=B, gw1=g["W1"], stride=offs["total"],
            fs=slab.view.data_ptr(), fsw=fw, gwo_=gwo.view.data_ptr(), gbo_=gbo.view.data_ptr()):
        return lambda: mod.mlp_step_bwd(d2, X, K0, wf, Hh, b0, B, gw1, g["W0"], g["b0"], g["b1"], stride, tick.data_ptr(),
                                        fs, fsw, gwo_, gbo_, s)

    for f in (fwd, infer, bwd):
        for kw in (dict(B=96), dict(B=32), dict(B=0), dict(K0=48), dict(K0=16), dict(Hh=128)):
            _refused(-2, f(**kw))
        for kw in (dict(X=X + 8), dict(wf=wf + 2)):
            _refused(-3, f(**kw))
    for f in (fwd, infer):
        for kw in (dict(C=0), dict(C=17)):
            _refused(-2, f(**kw))
        _refused(-3, f(wo=wo + 4))
        _refused(-3, f(b0=b0 + 4))
    _refused(-3, fwd(d2=dact2.view.data_ptr() + 8))
    _refused(-3, fwd(sl=slab.view.data_ptr() + 4))
    _refused(-2, infer(lg=0))
    _refused(-2, infer(pr=0))
    for kw in (dict(stride=H * H - 4), dict(fsw=fw - 4), dict(fsw=fw + 2), dict(gwo_=0), dict(gbo_=0)):
        _refused(-2, bwd(**kw))
    for kw in (dict(d2=dact2.view.data_ptr() + 8), dict(gw1=g["W1"] + 4), dict(fs=slab.view.data_ptr() + 8),
               dict(gwo_=gwo.view.data_ptr() + 4), dict(gbo_=gbo.view.data_ptr() + 8)):
        _refused(-3, bwd(**kw))
    # nothing was written
    for buf in (dact2, slab, loss, corr, logits, pred, slabs, gwo, gbo, net.wf):
        bits = buf.flat.view(torch.int16 if buf.dtype == bf16 else i32)
        keep = net.ref.flat.view(torch.int16) if buf is net.wf else torch.full_like(bits, buf.sentinel)
        assert torch.equal(bits, keep)
    assert int(tick.item()) == 5
    # the accepted calls with this very set of buffers
    fwd()()
    bwd()()
    infer()()
    torch.cuda.synchronize()
    GU.assert_equal(MU.unswizzle_dact2(dact2.result()), o.dact2.to(bf16), "dact2")
    want = MU.flat_grad(c, MU.grads(c, o, slice(0, B)))
    wo_ = offs["Wout"][0]
    GU.assert_equal(slabs.result()[0, :wo_], want[:wo_], "partials")
    GU.assert_equal(gwo.result().reshape(-1), want[wo_:wo_ + 16 * H], "gwo")
    GU.assert_equal(logits.result(), MU.to_f32(o.z), "logits")
    for buf in (dact2, slab, loss, corr, logits, pred, slabs, gwo, gbo):
        buf.check("contract neighbours")
    assert int(tick.item()) == 6
