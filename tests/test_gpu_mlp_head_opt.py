"""head_fused (head.hip), grad_reduce_adam and cast_pad_bf16 (mlp.hip) called directly, against fp64
references: the kernels every MLP path (and every world size) shares, so far reached only through whole
training steps."""
import math

import pytest
import torch

import _gemm_util as GU
from _gemm_util import bf16, f32, f64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
HEAD_PAD = 32


# =============================================================================== a. head_fused
def _first_argmax(z):
    """Lowest index among the maxima (the kernel's tie rule)."""
    C = z.shape[1]
    idx = torch.arange(C).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values


def _head_inputs(B, D, C, seed):
    """H: small integers with exact zeros and -0.0; Wout / bias: multiples of 0.25 (the pad rows of Wout hold
    2.0: dz is zero there, so they must not matter).  Every logit is then exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    H = torch.randint(-2, 3, (B, D), generator=g).to(f32)
    H[torch.rand(B, D, generator=g) < 0.3] = 0.0
    H[torch.rand(B, D, generator=g) < 0.1] = -0.0
    W = torch.full((HEAD_PAD, D), 2.0)
    W[:C] = torch.randint(-2, 3, (C, D), generator=g).to(f32) * 0.25 * (torch.rand(C, D, generator=g) < 0.25)
    bias = torch.full((HEAD_PAD,), 2.0)
    bias[:C] = torch.randint(-4, 5, (C,), generator=g).to(f32) * 0.25
    y = torch.randint(0, C, (B,), generator=g)
    return H.to(bf16), W.to(bf16), bias, y


def _bf16_ulp(x):
    """One unit in the last place of bf16 at |x| (0 at 0)."""
    _, e = torch.frexp(x.abs().to(f64))
    return torch.where(x == 0, torch.zeros_like(x, dtype=f64), torch.pow(torch.tensor(2.0, dtype=f64), (e - 8).to(f64)))


def _run_head(cuda, H, W, bias, y, C, scale):
    from har.ops import _native
    mod = _native.kernels()
    B, D = H.shape
    nb = mod.head_fused_blocks(B)
    dl = GU.guarded(B, HEAD_PAD, bf16, cuda, ld=HEAD_PAD)
    dH = GU.guarded(B, D, bf16, cuda, ld=D)
    loss = GU.guarded(1, nb, f32, cuda, ld=nb)
    corr = torch.full((nb + 8,), -7, dtype=torch.int32, device=cuda)
    Hd, Wd, bd, yd = H.to(cuda), W.to(cuda), bias.to(cuda), y.to(torch.int32).to(cuda)
    mod.head_fused(Hd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), yd.data_ptr(), B, D, C, float(scale),
                   dl.view.data_ptr(), dH.view.data_ptr(), loss.view.data_ptr(), corr.data_ptr(),
                   _native.stream_ptr())
    torch.cuda.synchronize()
    corr = corr.cpu()
    assert bool((corr[nb:] == -7).all()), "block_correct written past the workgroups"
    return dl, dH, loss, corr[:nb]


def _check_head(cuda, H, W, bias, y, C, scale, tag):
    B, D = H.shape
    dl, dH, loss, corr = _run_head(cuda, H, W, bias, y, C, scale)
    Hf, Wf = H.to(f64), W.to(f64)
    z = Hf @ Wf[:C].T + bias[:C].to(f64)
    assert torch.equal(z.to(f32).to(f64), z)                       # the logits are exact in fp32
    # dlogits: the criterion of test_softmax_ce_head (rtol 1e-2, atol 1e-5 at scale 1e-3)
    p = torch.softmax(z, 1)
    p[torch.arange(B), y] -= 1
    want = (p * scale).to(bf16).to(f64)
    got_dl = dl.result()
    assert bool(torch.isfinite(got_dl.float()).all()), tag
    torch.testing.assert_close(got_dl[:, :C].to(f64), want, rtol=1e-2, atol=1e-2 * scale, msg=lambda m: f"{tag} dlogits: {m}")
    if C < HEAD_PAD:
        assert float(got_dl[:, C:].float().abs().max()) == 0, f"{tag}: dlogits columns >= C"
    dl.check(tag + " dlogits")                                     # rows >= B untouched
    # loss: rtol 1e-4, atol 1e-5 per row
    ref_loss = float(torch.nn.functional.cross_entropy(z, y, reduction="sum"))
    got_loss = float(loss.result().to(f64).sum())
    assert math.isfinite(got_loss) and abs(got_loss - ref_loss) <= 1e-4 * abs(ref_loss) + 1e-5 * B, \
        f"{tag}: loss {got_loss} vs {ref_loss}"
    loss.check(tag + " loss")
    # correct count: exact (lowest index wins a tie)
    assert int(corr.sum()) == int((_first_argmax(z) == y).sum()), f"{tag}: correct count"
    # dH, teacher-forced with the kernel's own dlogits
    dz = got_dl.to(f64)
    exact = dz @ Wf
    keep = GU.mask_passes(H)
    ref = torch.where(keep, exact.to(bf16).to(f64), torch.zeros_like(exact))
    tol = _bf16_ulp(exact) + 64 * U * (dz.abs() @ Wf.abs())
    got = dH.result().to(f64)
    over = (got - ref).abs() - tol
    r, c = divmod(int(over.argmax()), D)
    assert float(over.max()) <= 0, f"{tag}: dH[{r}, {c}] = {float(got[r, c])} vs {float(ref[r, c])}, " \
                                   f"{float(over.max()):.3e} beyond the tolerance"
    if bool((~keep).any()):
        assert float(got[~keep].abs().max()) == 0, f"{tag}: dH where H is not positive"
    dH.check(tag + " dH")
    return corr, z


HEAD_D = [32, 96, 128, 256, 512]      # runtime-D twice, then each compiled width
HEAD_B = [1, 17, 64, 65, 130]         # under a wave tile, a partial tile, one workgroup, one row over, 3 workgroups
HEAD_C = [1, 6, 16, 17, 32]           # one or both sides of the 16-lane split, the full width
HEAD_CASES = sorted({(D, B, C) for D in HEAD_D for B, C in ((65, 17), (17, 6))} |
                    {(96, B, C) for B in HEAD_B for C in HEAD_C})


@pytest.mark.parametrize("D,B,C", HEAD_CASES)
def test_head_fused_matches_fp64(cuda, D, B, C):
    H, W, bias, y = _head_inputs(B, D, C, seed=D * 1000 + B * 10 + C)
    _check_head(cuda, H, W, bias, y, C, 1.0 / B, f"head D={D} B={B} C={C}")


@pytest.mark.parametrize("D", [320, 512])
def test_head_fused_launches_past_64k_of_lds(cuda, D):
    """(96 (D + 8) + 2560) 2 bytes of dynamic LDS: 65 KB at D = 320 (the first width past 64 KB), 105 KB at
    D = 512.  Three workgroups, so a launch that only worked once would show."""
    assert (96 * (D + 8) + 2560) * 2 > 64 * 1024
    H, W, bias, y = _head_inputs(130, D, 6, seed=D)
    _check_head(cuda, H, W, bias, y, 6, 1.0 / 130, f"head D={D} past 64 KB")


@pytest.mark.parametrize("label_on", ["lower", "higher"])
def test_head_fused_tie_goes_to_the_lowest_index(cuda, label_on):
    """Classes 2 and 4 have identical Wout rows and bias, pushed above the rest: every row's maximum is a tie
    between them.  With the label on class 2 every row counts as correct, with it on class 4 none does."""
    B, D, C = 17, 32, 6
    H, W, bias, y = _head_inputs(B, D, C, seed=3)
    W[4] = W[2]
    bias[2] = bias[4] = 64.0
    y = torch.full((B,), 2 if label_on == "lower" else 4)
    corr, z = _check_head(cuda, H, W, bias, y, C, 1.0 / B, f"head tie, label on the {label_on} index")
    assert bool((z[:, 2] == z[:, 4]).all()) and bool((_first_argmax(z) == 2).all())
    assert int(corr.sum()) == (B if label_on == "lower" else 0)


def test_head_fused_saturated_logits_stay_finite(cuda):
    """Logits of +60 and -60 on one class (exact integers), 0 elsewhere: e^-60 must neither overflow the
    softmax nor turn the loss or dlogits into inf / NaN."""
    B, D, C = 65, 32, 6
    H = torch.zeros(B, D)
    H[0::2, :30] = 2.0
    H[1::2, :30] = -2.0
    W = torch.zeros(HEAD_PAD, D)
    W[1, :30] = 1.0
    bias = torch.zeros(HEAD_PAD)
    y = torch.arange(B) % C
    corr, z = _check_head(cuda, H.to(bf16), W.to(bf16), bias, y, C, 1.0 / B, "head saturated")
    assert sorted(z[:, 1].unique().tolist()) == [-60.0, 60.0]


# ========================================================================== b. grad_reduce_adam
GR_REDUCE, GR_STORE, GR_ADAM, GR_REFRESH = 1, 2, 4, 8
GR_N = 1300                                                   # 6 workgroups of 64 float4, the last partial
GR_REGIONS = [(0, 256), (256, 4), (300, 500), (1000, 296)]    # (start, len): gaps at 260, 800 and 1296
GR_SLABS = [[33, 1, 17, 49], [32, 16, 4, 31], [15, 49, 33, 1], [4, 31, 16, 32], [17, 15, 1, 4]]
HYP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)


def _slabs(S_list, seed, integer=True):
    """Per region an [S, lds] slab matrix, lds = len + 8, the 8 pad columns holding 7.0."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for (start, ln), S in zip(GR_REGIONS, S_list):
        t = torch.full((S, ln + 8), 7.0)
        t[:, :ln] = torch.randint(-4, 5, (S, ln), generator=g).to(f32) if integer else torch.randn(S, ln, generator=g)
        out.append(t)
    return out


def _flat_sum(slabs):
    g = torch.zeros(GR_N, dtype=f64)
    for (start, ln), t in zip(GR_REGIONS, slabs):
        g[start:start + ln] = t[:, :ln].to(f64).sum(0)
    return g


class _Opt:
    """Flat optimizer state in guarded device buffers."""

    def __init__(self, cuda, seed):
        g = torch.Generator().manual_seed(seed)
        self.cuda = cuda
        self.bufs = {k: GU.guarded(1, GR_N, bf16 if k == "pb" else f32, cuda, ld=GR_N) for k in ("G", "p", "m", "v", "pb")}
        self.p0 = torch.randn(GR_N, generator=g)
        self.m0 = torch.randn(GR_N, generator=g) * 0.1
        self.v0 = torch.rand(GR_N, generator=g) * 0.1
        self.bufs["p"].fill(self.p0[None])
        self.bufs["m"].fill(self.m0[None])
        self.bufs["v"].fill(self.v0[None])
        self.bufs["G"].fill(torch.full((1, GR_N), 123.0))
        self.bufs["pb"].fill(torch.full((1, GR_N), 5.0))
        self.step = torch.zeros(4, dtype=torch.int32, device=cuda)

    def call(self, slabs_dev, mode, tick, regions=GR_REGIONS):
        from har.ops import _native
        b = self.bufs
        _native.kernels().grad_reduce_adam(
            src=[t.data_ptr() for t in slabs_dev], start=[r[0] for r in regions], len=[r[1] for r in regions],
            lds=[t.stride(0) for t in slabs_dev], nsl=[t.shape[0] for t in slabs_dev], n=GR_N,
            G=b["G"].view.data_ptr(), param=b["p"].view.data_ptr(), m=b["m"].view.data_ptr(), v=b["v"].view.data_ptr(),
            pb=b["pb"].view.data_ptr(), lr=HYP["lr"], b1=HYP["b1"], b2=HYP["b2"], eps=HYP["eps"], wd=HYP["wd"],
            step=self.step.data_ptr(), tick=tick, mode=mode, stream=_native.stream_ptr())
        torch.cuda.synchronize()

    def get(self, k):
        return self.bufs[k].result()[0]

    def check_guards(self, tag):
        for k, b in self.bufs.items():
            b.check(f"{tag} {k}")
        assert self.step[1:].abs().sum().item() == 0


@pytest.mark.parametrize("S_list", GR_SLABS, ids=lambda s: "S" + "_".join(map(str, s)))
def test_grad_reduce_adam_matches_fp64(cuda, S_list):
    """Slab counts on every boundary of the 8-, 4- and 1-wide loops (per wave: slabs q, q + 4, ...), regions
    with gaps, pitches longer than the regions.  Integer slabs: the reduction is exact.  The two-launch form
    (reduce + store, then Adam from G) must leave the same bits as the one-launch form; three steps against
    an fp64 AdamW under test_adam_step's tolerance; the bf16 copy is the rounded parameter, bit for bit."""
    slabs = _slabs(S_list, seed=sum(S_list))
    dev = [t.to(cuda) for t in slabs]
    gsum = _flat_sum(slabs)
    a, b = _Opt(cuda, 1), _Opt(cuda, 1)
    a.call(dev, GR_REDUCE | GR_STORE, tick=0)
    assert int(a.step[0]) == 0
    GU.assert_equal(a.get("G"), gsum.to(f32), "reduced G")      # gaps: 0
    for k, want in (("p", a.p0), ("m", a.m0), ("v", a.v0)):
        GU.assert_equal(a.get(k), want, f"{k} after reduce + store")
    a.call(dev, GR_ADAM, tick=1)
    b.call(dev, GR_REDUCE | GR_ADAM, tick=1)
    assert int(a.step[0]) == 1 and int(b.step[0]) == 1
    for k in ("p", "m", "v", "pb"):
        GU.assert_equal(b.get(k).view(torch.int16 if k == "pb" else torch.int32),
                        a.get(k).view(torch.int16 if k == "pb" else torch.int32), f"{k}: one launch vs two")
    GU.assert_equal(b.get("G"), torch.full((GR_N,), 123.0), "G without GR_STORE")
    for t in (2, 3):
        b.call(dev, GR_REDUCE | GR_ADAM, tick=1)
        assert int(b.step[0]) == t
    # fp64 AdamW with the hyper-parameters the kernel is handed: floats (1 - float(0.999) is 1.3e-5 off 0.001)
    h = {k: float(torch.tensor(x, dtype=f32)) for k, x in HYP.items()}
    pr, mr, vr = a.p0.to(f64), a.m0.to(f64), a.v0.to(f64)
    for t in (1, 2, 3):
        mr = h["b1"] * mr + (1 - h["b1"]) * gsum
        vr = h["b2"] * vr + (1 - h["b2"]) * gsum * gsum
        upd = (mr / (1 - h["b1"] ** t)) / ((vr / (1 - h["b2"] ** t)).sqrt() + h["eps"])
        pr = pr - h["lr"] * (upd + h["wd"] * pr)
    for k, want in (("p", pr), ("m", mr), ("v", vr)):
        torch.testing.assert_close(b.get(k).to(f64), want, rtol=1e-5, atol=1e-5, msg=lambda m: f"{k}: {m}")
    GU.assert_equal(b.get("pb").view(torch.int16), b.get("p").to(bf16).view(torch.int16), "bf16 copy")
    a.check_guards("two launches")
    b.check_guards("one launch")


def _kernel_order_sum(t):
    """fp32 sum of the slabs [S, n] in the order mlp.hip documents: wave q takes slabs q, q + 4, ...; eight at
    a time as ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)), then four as (x0 + x1) + (x2 + x3), then
    singly; the four waves' partials as (a + b) + (c + d)."""
    S = t.shape[0]
    part = []
    for q in range(4):
        acc = torch.zeros(t.shape[1], dtype=f32)
        s = q
        while s + 28 < S:
            x = [t[s + 4 * j] for j in range(8)]
            acc = acc + (((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7])))
            s += 32
        while s + 12 < S:
            x = [t[s + 4 * j] for j in range(4)]
            acc = acc + ((x[0] + x[1]) + (x[2] + x[3]))
            s += 16
        while s < S:
            acc = acc + t[s]
            s += 4
        part.append(acc)
    return (part[0] + part[1]) + (part[2] + part[3])


@pytest.mark.parametrize("S_list", [[16, 17, 33, 49], [31, 32, 15, 4]], ids=lambda s: "S" + "_".join(map(str, s)))
def test_grad_reduce_sums_in_the_documented_order(cuda, S_list):
    """Gaussian slabs: the stored G equals, bit for bit, the fp32 sum taken in the fixed order the kernel's
    comment promises (what makes the step reproducible and equal across world sizes)."""
    slabs = _slabs(S_list, seed=7, integer=False)
    o = _Opt(cuda, 2)
    o.call([t.to(cuda) for t in slabs], GR_REDUCE | GR_STORE, tick=0)
    want = torch.zeros(GR_N)
    for (start, ln), t in zip(GR_REGIONS, slabs):
        want[start:start + ln] = _kernel_order_sum(t[:, :ln])
    GU.assert_equal(o.get("G").view(torch.int32), want.view(torch.int32), "G")
    o.check_guards("order")


def test_grad_reduce_adam_refresh_tick_and_refusals(cuda):
    slabs = [t.to(cuda) for t in _slabs([4, 1, 4, 1], seed=1)]
    o = _Opt(cuda, 3)
    newp = torch.randn(GR_N, generator=torch.Generator().manual_seed(8))
    o.bufs["p"].fill(newp[None])
    o.call(slabs, GR_REFRESH, tick=0)
    GU.assert_equal(o.get("pb").view(torch.int16), newp.to(bf16).view(torch.int16), "refreshed bf16 copy")
    GU.assert_equal(o.get("p"), newp, "p after refresh")
    GU.assert_equal(o.get("m"), o.m0, "m after refresh")
    GU.assert_equal(o.get("v"), o.v0, "v after refresh")
    GU.assert_equal(o.get("G"), torch.full((GR_N,), 123.0), "G after refresh")
    assert int(o.step[0]) == 0
    o.check_guards("refresh")
    for mode in (GR_REFRESH | GR_ADAM, GR_REFRESH | GR_REDUCE, GR_REFRESH | GR_STORE):
        with pytest.raises(RuntimeError, match="contract violation"):
            o.call(slabs, mode, tick=0)
    unsorted_ = [GR_REGIONS[0], GR_REGIONS[2], GR_REGIONS[1], GR_REGIONS[3]]
    overlap = [(0, 256), (252, 4), (300, 500), (1000, 296)]
    past_end = [(0, 256), (256, 4), (300, 500), (1008, 296)]
    for regions in (unsorted_, overlap, past_end):
        with pytest.raises(RuntimeError, match="contract violation"):
            o.call(slabs, GR_REDUCE | GR_STORE, tick=1, regions=regions)
    assert int(o.step[0]) == 0                                  # a refused call ticks nothing
    GU.assert_equal(o.get("G"), torch.full((GR_N,), 123.0), "G after the refused calls")


# ============================================================================= c. cast_pad_bf16
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "offset8bytes"])
@pytest.mark.parametrize("cin,cout", [(43, 64), (1, 32), (33, 40), (7, 12), (32, 32)])
@pytest.mark.parametrize("rows", [0, 1, 257])
def test_cast_pad_bf16_bit_equal(cuda, rows, cin, cout, offset):
    """fp32 [rows][ldin] -> zero-padded bf16 [rows][cout]: the 16-byte kernel (aligned output, cout % 8 == 0)
    and the scalar one (cout = 12, or the output 8 bytes off), an input pitch of cin + 3 whose padding holds
    7.0, odd cin; bit equal to torch's rounding, nothing written around the output."""
    from har.ops import _native
    g = torch.Generator().manual_seed(rows + cin + cout)
    ldin = cin + 3
    X = torch.full((max(rows, 1), ldin), 7.0)
    X[:, :cin] = torch.randn(max(rows, 1), cin, generator=g) * 3
    if rows:
        X[0, 0], X[-1, cin - 1] = -0.0, float("inf")
        X[rows // 2, cin // 2] = 1.00390625      # a tie of round-to-nearest-even (1 + 2^-8)
    Xd = X.to(cuda)
    X = X[:rows]
    n = rows * cout
    flat = torch.full((2 * GU.GUARD + offset + n,), GU.BF16_SENTINEL, dtype=torch.int16).to(cuda)
    out_ptr = flat.data_ptr() + 2 * (GU.GUARD + offset)
    assert out_ptr % 16 == 2 * offset
    _native.kernels().cast_pad_bf16(Xd.data_ptr(), rows, cin, ldin, out_ptr, cout, _native.stream_ptr())
    torch.cuda.synchronize()
    want = torch.zeros(rows, cout, dtype=bf16)
    want[:, :cin] = X[:, :cin].to(bf16)
    got = flat.cpu()
    GU.assert_equal(got[GU.GUARD + offset:GU.GUARD + offset + n].view(rows, cout), want.view(torch.int16), "cast")
    assert bool((got[:GU.GUARD + offset] == GU.BF16_SENTINEL).all()) and \
        bool((got[GU.GUARD + offset + n:] == GU.BF16_SENTINEL).all()), "wrote around the output"
