"""The GEMM family's test oracle and input builders (tests/_gemm_util.py) checked on their own, and the
argument contract of ops/gemm.py — all on the CPU."""
import pytest
import torch

import _gemm_util as GU
from _gemm_util import bf16, f32, f64

LAYOUTS = [0, 2, 3]
K_MAX_TILE_SWEEP = 2 * 128 + 8   # the largest K of the tile sweep: 2 BK + EPV at BK = 128, bf16
K_NAIVE_BAYES = 1001
NUMERICS_SHAPE = (136, 136, 4104)


@pytest.mark.parametrize("K", [K_MAX_TILE_SWEEP, K_NAIVE_BAYES])
def test_exact_inputs_keep_every_partial_sum_an_fp32_integer(K):
    """Every prefix of every ordering is bounded by sum_k |a b|: below 2^24, so fp32 adds of these integers
    never round; operands, bias and alpha times an integer are representable in bf16 / fp32."""
    A, B, bias = GU.exact_inputs(136, 264, K, seed=1)
    for t in (A, B):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3
        assert torch.equal(t.to(bf16).to(f64), t)
    assert {float(v) for v in A.unique()} == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    assert torch.equal(bias * 4, (bias * 4).round()) and float(bias.abs().max()) <= 2
    worst = float((A.abs() @ B.abs()).max())
    assert worst <= 9 * K and worst + 2 < 2 ** 24
    assert float(A.abs().sum(1).max()) < 2 ** 24                      # the fused row sums
    full = A @ B
    assert torch.equal((GU.ALPHA * full).to(f32).to(f64), GU.ALPHA * full)
    assert torch.equal((full + bias).to(f32).to(f64), full + bias)
    # an fp32 matmul in whatever order torch takes gives the same bits
    assert torch.equal((A.to(f32) @ B.to(f32)).to(f64), full)


@pytest.mark.parametrize("dtype", [bf16, f32], ids=["bf16", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_oracle_is_the_fp64_product_of_the_stored_operands(layout, dtype):
    M, N, K = 24, 40, 72
    A, B, bias = GU.exact_inputs(M, N, K, seed=layout)
    a, lda, b, ldb = GU.store_operands(A, B, layout, dtype, "cpu")
    assert a.shape == ((K, M) if layout & 1 else (M, K)) and b.shape == ((K, N) if layout & 2 else (N, K))
    assert a.stride(0) == lda == a.shape[1] + 8 * GU.epv(dtype) and b.stride(0) == ldb
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    # the padding is there and is not zero
    assert float(a.as_strided((a.shape[0], lda), (lda, 1))[:, a.shape[1]:].abs().min()) == GU.PAD_VALUE
    ref = torch.matmul(A, B)
    o = GU.oracle(a, b, layout, GU.EPI_F32, alpha=GU.ALPHA)
    assert o.C.dtype == f32 and torch.equal(o.C.to(f64), GU.ALPHA * ref)
    assert torch.equal(o.rowsum.to(f64), GU.ALPHA * A.sum(1))
    o = GU.oracle(a, b, layout, GU.EPI_BIAS_F32, bias=bias)
    assert torch.equal(o.C.to(f64), ref + bias)
    rng = GU.split_ranges(K, 32)
    assert rng == [(0, 32), (32, 64), (64, 72)]
    o = GU.oracle(a, b, layout, GU.EPI_F32_SLAB, alpha=GU.ALPHA, k_ranges=rng)
    assert o.C.shape == (3, M, N) and o.rowsum.shape == (3, M)
    assert torch.equal(o.C.to(f64).sum(0), GU.ALPHA * ref)
    assert torch.equal(o.C[2].to(f64), GU.ALPHA * (A[:, 64:] @ B[64:]))
    assert torch.equal(o.rowsum[1].to(f64), GU.ALPHA * A[:, 32:64].sum(1))
    if dtype == bf16:
        o = GU.oracle(a, b, layout, GU.EPI_BIAS, bias=bias)
        assert o.C.dtype == bf16 and torch.equal(o.C, (ref + bias).to(bf16))
        o = GU.oracle(a, b, layout, GU.EPI_BIAS_RELU, bias=bias)
        assert torch.equal(o.C, torch.relu(ref + bias).to(bf16)) and float(o.C.float().min()) == 0
        mask = GU.exact_mask(M, N, seed=5)
        o = GU.oracle(a, b, layout, GU.EPI_RELU_GRAD, mask=mask)
        keep = GU.mask_passes(mask)
        assert torch.equal(o.C[keep], ref.to(bf16)[keep]) and float(o.C[~keep].float().abs().max()) == 0


def test_mask_rule_is_sign_clear_and_not_zero():
    mask = GU.exact_mask(64, 64, seed=2)
    bits = mask.view(torch.int16)
    assert sorted(bits.unique().tolist()) == sorted(GU.MASK_BITS)
    want = {-0x4080: False, -0x8000: False, 0: False, 0x3F80: True, 0x0008: True, 0x0008 - 0x8000: False}
    keep = GU.mask_passes(mask)
    for b, w in want.items():
        assert bool(keep[bits == b].all()) == w and bool(keep[bits == b].any()) == w
    # the denormal is a value, not a zero: the rule differs from "flush, then compare"
    assert float(mask[bits == 0x0008][0]) == 2.0 ** -130


@pytest.mark.parametrize("dtype", [bf16, f32], ids=["bf16", "f32"])
def test_guarded_reports_a_write_outside_the_output(dtype):
    g = GU.guarded(5, 8, dtype, "cpu", slabs=2)
    assert g.ld == 24 and g.view.shape == (12, 24) and g.out.shape == (2, 5, 8) and g.view.data_ptr() % 16 == 0
    assert g.sentinel == (GU.BF16_SENTINEL if dtype == bf16 else 0x7FC00000)
    g.check()
    g.fill(torch.ones(2, 5, 8))
    g.check()
    assert float(g.result().float().sum()) == 80
    for where in [(0, 8), (5, 0), (11, 3)]:       # a pad column, the spare row of slab 0, of slab 1
        h = GU.guarded(5, 8, dtype, "cpu", slabs=2)
        h.view[where] = 1.0
        with pytest.raises(AssertionError):
            h.check()
    h = GU.guarded(5, 8, dtype, "cpu")
    h.flat[3] = 0.0
    with pytest.raises(AssertionError):
        h.check()
    h = GU.guarded(5, 8, dtype, "cpu")
    h.flat[-1] = float("nan") if dtype == f32 else 0.0   # the same NaN is no write; for bf16 0x7FC0 != 0x7FC1
    if dtype == bf16:
        with pytest.raises(AssertionError):
            h.check()
    else:
        h.check()


@pytest.mark.parametrize("dtype", [bf16, f32], ids=["bf16", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fp32_matmul_of_the_numerics_case_is_inside_the_bound(layout, dtype):
    """The bound of the accumulation-numerics GPU test, checked on the reference alone: torch's own fp32
    product of the same rounded Gaussian inputs against the fp64 one."""
    M, N, K = NUMERICS_SHAPE
    A, B = GU.gaussian_inputs(M, N, K, dtype, seed=40 + layout)
    assert torch.equal(A.to(dtype).to(f64), A)
    exact = A @ B
    bound = GU.sum_bound(A, B)
    got = (A.to(f32) @ B.to(f32)).to(f64)
    ratio = float(((got - exact).abs() / bound).max())
    print(f"fp32 matmul error / bound: {ratio:.3e}")
    assert 0 < ratio <= 1.0
    # and the bound still tells one dropped k term (of 4104) from rounding
    dropped = exact - A[:, 7:8] @ B[7:8]
    assert float(((dropped - exact).abs() / bound).max()) > 1


def _call(kw):
    from har.ops.gemm import gemm_bf16
    kw = dict(kw)
    return gemm_bf16(kw.pop("A"), kw.pop("B"), kw.pop("C"), kw.pop("M"), kw.pop("N"), kw.pop("K"), **kw)


@pytest.mark.parametrize("case", GU.contract_cases("cpu"), ids=lambda c: c[0])
def test_gemm_argument_contract_refusals(case):
    """ops/gemm.py refuses what the kernel's 16-byte epilogue vectors and unconditional mask reads cannot
    take, before it looks at the device."""
    _, pattern, kw = case
    with pytest.raises(ValueError, match=pattern):
        _call(kw)


@pytest.mark.parametrize("case", GU.contract_ok_cases("cpu"), ids=lambda c: c[0])
def test_gemm_argument_contract_accepts_the_neighbours(case):
    """The nearest valid calls get past the contract: on host tensors the next refusal is the device's."""
    with pytest.raises(ValueError, match="must be a device tensor"):
        _call(case[1])
