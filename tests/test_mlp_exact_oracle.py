"""The exact-arithmetic MLP data and its fp64 oracle (tests/_mlp_exact_util.py) checked on their own, on the
CPU: the oracle against torch.autograd, and for EVERY case the GPU files run (test_gpu_mlp_step_exact.py,
test_gpu_mlp_fused_small_exact.py) the conditions that make each kernel output a single well-defined value.
These are conditions on the generator, not measurements of a kernel."""
import math

import pytest
import torch

import _mlp_exact_util as MU
from _mlp_exact_util import bf16, f32, f64

EXACT_BITS = 24.0


def test_oracle_matches_autograd():
    """With the roundings switched off the oracle is plain backprop of the fp64 network with
    cross_entropy(reduction="sum") * scale."""
    c = MU.make_case(48, 32, 128, 6, seed=3)
    scale = 1.0 / 48
    o = MU.oracle(c, round_bf16=False, scale=scale)
    P = {n: getattr(c, n).clone().requires_grad_(True) for n in ("W0", "b0", "W1", "b1", "Wout", "bout")}
    h1 = torch.relu(c.X @ P["W0"].T + P["b0"])
    h2 = torch.relu(h1 @ P["W1"].T + P["b1"])
    z = h2 @ P["Wout"][:c.C].T + P["bout"][:c.C]
    loss = torch.nn.functional.cross_entropy(z, c.y, reduction="sum")
    ga = torch.autograd.grad(loss * scale, list(P.values()))
    torch.testing.assert_close(o.z, z.detach(), rtol=1e-12, atol=1e-13)
    assert abs(float(o.loss.sum()) - float(loss.detach())) <= 1e-10 * abs(float(loss.detach()))
    got = MU.grads(c, o, slice(0, c.B))
    parts = [MU.grads(c, o, slice(r, r + 16)) for r in range(0, c.B, 16)]
    for name, ref in zip(P, ga):
        assert float(ref.abs().max()) > 0
        torch.testing.assert_close(got[name], ref, rtol=1e-10, atol=1e-12 * float(ref.abs().max()))
        torch.testing.assert_close(sum(p[name] for p in parts), ref, rtol=1e-10, atol=1e-12 * float(ref.abs().max()))
        if name in ("Wout", "bout"):
            assert float(got[name][c.C:].abs().max()) == 0


def test_rne_and_rounding_classes():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, 257.0, -0.0], dtype=f64)
    assert MU.rne_bf16(v).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0, 256.0, -0.0]
    inexact, down, up = MU.needs_rounding(v)
    assert inexact.tolist() == [False, True, True, True, True, False]
    assert down.tolist() == [False, True, False, False, True, False]
    assert up.tolist() == [False, False, True, False, False, False]
    with pytest.raises(AssertionError):
        MU.rne_bf16(torch.tensor([1.0 + 2.0 ** -30], dtype=f64))


def test_layout_rules():
    assert [MU.step_grid(B) for B in (64, 192, 1088, 8256)] == [2, 6, 34, 256]
    assert MU.step_fwd_rows(8256, 1).tolist() == list(range(32, 64)) + list(range(32 * 257, 32 * 258))
    assert MU.step_fwd_rows(8256, 2).tolist() == list(range(64, 96))
    assert [MU.step_slices(B) for B in (64, 128, 1088, 2560, 4160)] == [1, 2, 16, 16, 16]
    assert [MU.step_bwd_rows(1088, s) for s in (0, 7, 8, 9, 15)] == [(0, 128), (896, 1024), (1024, 1088),
                                                                   (1152, 1152), (1920, 1920)]
    assert MU.step_bwd_rows(2560, 13) == (2496, 2560) and MU.step_bwd_rows(4160, 12) == (3840, 4160)
    for B in (64, 128, 1088, 2560, 4160):   # the slices tile the batch
        cover = torch.zeros(B)
        for s in range(MU.step_slices(B)):
            r0, r1 = MU.step_bwd_rows(B, s)
            cover[r0:r1] += 1
        assert bool((cover == 1).all())
    for B in (16, 48, 80, 8256):
        rows = torch.cat([MU.fwd_head_rows(B, w) for w in range(MU.fwd_head_grid(B))])
        assert sorted(rows.tolist()) == list(range(B))
    assert [MU.fwd_head_grid(B) for B in (16, 48, 80)] == [1, 2, 3]
    assert MU.fwd_head_rows(80, 1).tolist() == list(range(64, 80)) and MU.fwd_head_rows(80, 2).numel() == 0
    d = torch.arange(16 * 256, dtype=f32).reshape(16, 256)
    u = MU.unswizzle_dact2(d)
    assert torch.equal(u[:4], d[:4]) and torch.equal(u[8:12], d[8:12])
    assert torch.equal(u[4, :8], d[4, 8:16]) and torch.equal(u[7, 8:16], d[7, :8]) and torch.equal(u[13, 248:], d[13, 240:248])
    assert torch.equal(MU.unswizzle_dact2(u), d)
    offs = MU.flat_offsets(64, 256)
    assert offs["W0"][0] == 0 and offs["W1"][0] == 256 * 64 + 256 and offs["total"] == 256 * 64 + 256 + 65536 + 256 + 4096 + 16
    assert len({MU.case_id(k) for k in MU.CASES}) == len(MU.CASES)


@pytest.mark.parametrize("k", MU.cases_of("step_fwd") + MU.cases_of("step_bwd") + MU.cases_of("fwd_head")
                         + MU.cases_of("small"), ids=MU.case_id)
def test_case_conditions(k):
    kind, B, K0, H, C, _ = k
    c, o = MU.get_case(k)
    # operands: bf16 values; X has zeros, negative zeros and zero padding; the canary is in place
    assert float((c.X == 0).double().mean()) > 0.5 and bool(torch.signbit(c.X[c.X == 0]).any())
    assert c.F < K0 and float(c.X[:, c.F:].abs().max()) == 0 and not bool(torch.signbit(c.X[:, c.F:]).any())
    assert bool((c.Wout[C:] == MU.CANARY).all()) and bool((c.bout[C:] == MU.CANARY).all())
    assert torch.equal(c.Wout * 4, (c.Wout * 4).round()) and torch.equal(c.bout * 4, (c.bout * 4).round())
    assert math.log2(c.scale) == round(math.log2(c.scale))
    # every accumulation is exact in fp32 in any order: per partial, and in total wherever a total is formed
    # (the 8,256-row batch only runs the forward: its slabs are summed by nobody in these tests)
    # (the loss partials are summed on the host, in fp64)
    lrows = MU.partial_rows("step_fwd" if kind == "step_bwd" else kind, B)
    m = MU.margins(c, o, MU.partial_rows(kind, B) + ([slice(0, B)] if B <= 4160 else []), lrows)
    print(MU.case_id(k), {n: round(v, 1) for n, v in m.items()})
    assert max(m.values()) < EXACT_BITS, m
    for t in (o.h1, o.h2, o.dact2, o.dact1, o.dz):
        assert torch.equal(t.to(bf16).to(f64), t)
    assert torch.equal(o.z.to(f32).to(f64), o.z)
    # saturation: one-hot p, dz = scale (onehot(argmax) - onehot(y)), loss = z_max - z_y
    if C > 1:
        top = o.z.topk(2, 1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= MU.GAP
    onehot = lambda i: torch.nn.functional.one_hot(i, MU.NCLS).to(f64)   # noqa: E731
    assert torch.equal(o.p, onehot(o.argmax)[:, :C])
    assert torch.equal(o.dz, c.scale * (onehot(o.argmax) - onehot(c.y)))
    assert torch.equal(o.loss, o.z.max(1).values - o.z[torch.arange(B), c.y])
    # labels
    if C > 1:
        assert float((o.argmax != c.y).double().mean()) >= 1 / 3 and bool(o.correct.any())
        assert bool((c.y == C - 1).any())   # a label on the last real class
    assert o.argmax.unique().numel() == C and c.y.unique().numel() == C
    # every hidden unit is live on some rows and dead on others
    for h in (o.h1, o.h2):
        assert bool(((h > 0).any(0) & (h <= 0).any(0)).all())
    # rounding happens at each of the four points, halfway cases in both directions at h1
    for name in ("h1", "h2") + (("dact2", "dact1") if C > 1 else ()):
        inexact, down, up = MU.needs_rounding(o.pre[name])
        assert int(inexact.sum()) > 0, name
        if name == "h1":
            assert int(down.sum()) > 0 and int(up.sum()) > 0
    if C > 1:
        _, down, up = MU.needs_rounding(o.pre["dact2"])
        assert int(down.sum()) + int(up.sum()) > 0
    # no gradient segment is all zero (C = 1: dz is zero, so all of them are)
    g = MU.grads(c, o, slice(0, B))
    for name, t in g.items():
        # (B = C = 16: every class is the argmax of one row and the label of one row, so dbout sums to zero)
        assert bool((t != 0).any()) == (C > 1 and not (name == "bout" and B == C)), name
        if B <= 4160:
            MU.to_f32(t)
    assert float(g["W0"][:, c.F:].abs().max()) == 0 and float(g["Wout"][C:].abs().sum()) == 0


@pytest.mark.parametrize("k", [k for k in MU.CASES if k[5]], ids=MU.case_id)
def test_tie_case_conditions(k):
    kind, B, K0, H, C, _ = k
    c, o = MU.get_case(k)
    assert C & (C - 1) == 0
    m = MU.margins(c, o, MU.partial_rows(kind, B) + [slice(0, B)])
    print(MU.case_id(k), {n: round(v, 1) for n, v in m.items()})
    assert max(m.values()) < EXACT_BITS, m
    assert bool((o.z == o.z[:, :1]).all()) and bool((o.p == 1.0 / C).all()) and bool((o.argmax == 0).all())
    assert bool((o.h2[:, c.dead2] == 0).all()) and c.dead2.numel() == 32
    live = torch.ones(H, dtype=torch.bool)
    live[c.dead2] = False
    assert bool((c.Wout[:C, live] == c.Wout[:1, live]).all()) and not bool((c.Wout[:C, c.dead2] == c.Wout[:1, c.dead2]).all())
    onehot = torch.nn.functional.one_hot(c.y, MU.NCLS).to(f64)
    want = torch.zeros(B, MU.NCLS, dtype=f64)
    want[:, :C] = 1.0 / C
    assert torch.equal(o.dz, c.scale * (want - onehot))
    assert float(o.dact2.abs().max()) == 0 and float(o.dact1.abs().max()) == 0
    assert int(o.correct.sum()) == int((c.y == 0).sum()) and c.y.unique().numel() == C
    assert abs(float(o.loss.sum()) - B * math.log(C)) < 1e-9
    g = MU.grads(c, o, slice(0, B))
    assert bool((g["Wout"] != 0).any()) and bool((g["bout"] != 0).any())
