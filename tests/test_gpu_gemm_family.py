"""csrc/kernels/gemm.hip called directly: every tile id at its edges, every epilogue, the tile reordering
of large grids and the production call forms, bit for bit against the fp64 oracle of tests/_gemm_util.py
(integer-valued inputs: no tolerance), one accumulation-numerics case per type and layout against the
any-order fp32 summation bound, and the argument contract of ops/gemm.py on device tensors."""
import pytest
import torch

import _gemm_util as GU
from _gemm_util import (EPI_BIAS, EPI_BIAS_F32, EPI_BIAS_RELU, EPI_F32, EPI_F32_ATOMIC, EPI_F32_SLAB, EPI_RELU_GRAD,
                        bf16, f32, f64)

pytestmark = pytest.mark.gpu

LAYOUTS = [0, 2, 3]
TYPES = [bf16, f32]


def _tiles():
    from har.ops.gemm import TILES
    return TILES


def _gemm(dtype):
    from har.ops.gemm import gemm_bf16, gemm_f32
    return gemm_bf16 if dtype == bf16 else gemm_f32


def _tname(dtype):
    return "bf16" if dtype == bf16 else "f32"


class Case:
    """One (type, layout, tile, shape): the stored operands on the device and the launches of each epilogue."""

    def __init__(self, dev, dtype, layout, tile, M, N, K, seed):
        self.dev, self.dtype, self.layout, self.tile, self.M, self.N, self.K = dev, dtype, layout, tile, M, N, K
        self.A, self.B, self.bias64 = GU.exact_inputs(M, N, K, seed)
        self.a, self.lda, self.b, self.ldb = GU.store_operands(self.A, self.B, layout, dtype, dev)
        self.bias = self.bias64.to(f32).to(dev)
        self.seed = seed
        self.tag = f"{_tname(dtype)} layout {layout} tile {tile} M={M} N={N} K={K}"

    def run(self, epi, C, **kw):
        _gemm(self.dtype)(self.a, self.b, C, M=self.M, N=self.N, K=self.K, layout=self.layout, epi=epi,
                          tile=self.tile, **kw)

    def ref(self, epi, **kw):
        return GU.oracle(self.a, self.b, self.layout, epi, **kw)

    def plain(self, epi, alpha=1.0, bias=False, rowsum=False):
        """EPI_F32 / EPI_BIAS_F32 / EPI_BIAS / EPI_BIAS_RELU."""
        out = GU.guarded(self.M, self.N, bf16 if epi in GU.BF16_EPIS else f32, self.dev)
        rs = GU.guarded(1, self.M, f32, self.dev) if rowsum else None
        self.run(epi, out.view, alpha=alpha, bias=self.bias if bias else None,
                 rowsum=rs.out[0] if rowsum else None)
        o = self.ref(epi, alpha=alpha, bias=self.bias64 if bias else None)
        tag = f"{self.tag} epi {epi}"
        GU.assert_equal(out.result(), o.C, tag)
        out.check(tag)
        if rowsum:
            GU.assert_equal(rs.result()[0], o.rowsum, tag + " rowsum")
            rs.check(tag + " rowsum")

    def relu_grad(self):
        mask = GU.exact_mask(self.M + 1, self.N + 8, self.seed + 1).to(self.dev)[:self.M, :self.N]   # pitch N + 8
        assert mask.stride(0) == self.N + 8
        out = GU.guarded(self.M, self.N, bf16, self.dev)
        self.run(EPI_RELU_GRAD, out.view, mask=mask)
        tag = f"{self.tag} epi relu_grad"
        GU.assert_equal(out.result(), self.ref(EPI_RELU_GRAD, mask=mask).C, tag)
        out.check(tag)

    def atomic(self, k_split, rowsum=False):
        g = torch.Generator().manual_seed(self.seed + 2)
        C0 = torch.randint(-5, 6, (self.M, self.N), generator=g).to(f32)
        out = GU.guarded(self.M, self.N, f32, self.dev)
        out.fill(C0)
        rs = None
        if rowsum:
            rs = GU.guarded(1, self.M, f32, self.dev)
            rs.fill(torch.full((1, self.M), 3.0))
        self.run(EPI_F32_ATOMIC, out.view, alpha=GU.ALPHA, k_split=k_split, rowsum=rs.out[0] if rowsum else None)
        o = self.ref(EPI_F32_ATOMIC, alpha=GU.ALPHA, k_ranges=GU.split_ranges(self.K, k_split))
        tag = f"{self.tag} epi atomic k_split {k_split}"
        GU.assert_equal(out.result(), C0 + o.C, tag)
        out.check(tag)
        if rowsum:
            GU.assert_equal(rs.result()[0], 3.0 + o.rowsum, tag + " rowsum")
            rs.check(tag + " rowsum")

    def slab(self, k_split):
        rng = GU.split_ranges(self.K, k_split)
        out = GU.guarded(self.M, self.N, f32, self.dev, slabs=len(rng))
        rs = GU.guarded(1, self.M, f32, self.dev, slabs=len(rng))
        self.run(EPI_F32_SLAB, out.view, alpha=GU.ALPHA, k_split=k_split, ldc=out.ld, slab_stride=out.slab_stride,
                 rowsum=rs.view, slab_stride_rowsum=rs.slab_stride)
        o = self.ref(EPI_F32_SLAB, alpha=GU.ALPHA, k_ranges=rng)
        tag = f"{self.tag} epi slab k_split {k_split} ({len(rng)} slabs)"
        GU.assert_equal(out.result().view(len(rng), self.M, self.N), o.C, tag)             # every slab
        GU.assert_equal(rs.result().view(len(rng), self.M), o.rowsum, tag + " rowsum")    # every row-sum slab
        out.check(tag)
        rs.check(tag + " rowsum")


# ------------------------------------------------------------------------------------ a. tile edges
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tile", sorted(_tiles()))
@pytest.mark.parametrize("dtype", TYPES, ids=_tname)
def test_gemm_every_tile_at_its_edges_exact(cuda, dtype, tile, layout):
    """Shape 1 = (BM + e, BN + e, 2 BK + e): a partial second tile in M and N, a prefetched second K tile and
    a partial third; shape 2 = (e, e, e): one partial tile whose first K tile is already short.  Every
    epilogue of the type, bit for bit, guards intact.  The shapes come from ops.gemm.TILES, so a table that
    no longer mirrors gemm.hip's shows here as well."""
    BM, BN, BK = _tiles()[tile]
    e = GU.epv(dtype)
    shapes = [(BM + e, BN + e, 2 * BK + e), (e, e, e)]
    for i, (M, N, K) in enumerate(shapes):
        c = Case(cuda, dtype, layout, tile, M, N, K, seed=1000 * tile + 10 * layout + i)
        c.plain(EPI_F32, alpha=GU.ALPHA)
        c.plain(EPI_BIAS_F32, bias=True)
        c.atomic(BK)
        c.slab(BK)
        assert len(GU.split_ranges(K, BK)) == (3 if i == 0 else 1)
        if dtype == bf16:
            c.plain(EPI_BIAS, bias=True)
            c.plain(EPI_BIAS_RELU, bias=True)
            c.relu_grad()


# ------------------------------------------------------------------------------- b. tile reordering
@pytest.mark.parametrize("tile,M,N", [(5, 3 * 32 + 8, 2 * 64 + 8), (20, 64 * 2 + 8, 64 * 3 + 8)])
def test_gemm_reordered_tiles_and_row_sums_exact(cuda, tile, M, N):
    """12 tiles: more than 8 and no multiple of 8, so xcd_remap permutes them and the workgroups of the
    first N tile are not those with blockIdx.x == 0.  The row sums must come out once per row."""
    from har.ops.gemm import tile_counts
    tm, tn = tile_counts(M, N, tile)
    assert tm * tn == 12
    K = 2 * _tiles()[tile][2] + 8
    c = Case(cuda, bf16, 3, tile, M, N, K, seed=77 + tile)
    c.slab(_tiles()[tile][2])
    c.atomic(_tiles()[tile][2], rowsum=True)
    c.plain(EPI_F32, alpha=GU.ALPHA, rowsum=True)


# ------------------------------------------------------------------------------ c. production calls
@pytest.mark.parametrize("B,N,K", [(72, 256, 64), (72, 96, 256), (72, 256, 96)])
def test_gemm_forward_call_exact(cuda, B, N, K):
    """GemmPath.forward_backward's layer product: acts . W^T + b, ReLU, bf16, at fwd_tile's choice."""
    from har.models.mlp_paths import fwd_tile
    c = Case(cuda, bf16, 0, fwd_tile(B, N, K), B, N, K, seed=B + N + K)
    c.plain(EPI_BIAS_RELU, bias=True)


@pytest.mark.parametrize("B,N,K", [(72, 256, 96), (72, 64, 256)])
def test_gemm_dgrad_call_exact(cuda, B, N, K):
    """dact_{i-1} = (dact . W_i) * relu'(acts[i]) at dgrad_tile's choice."""
    from har.models.mlp_paths import dgrad_tile
    c = Case(cuda, bf16, 2, dgrad_tile(B, N, K), B, N, K, seed=B + N + K + 1)
    c.relu_grad()


@pytest.mark.parametrize("M,N", [(32, 96), (32, 32), (64, 64), (256, 96)])
def test_gemm_wgrad_call_exact(cuda, M, N):
    """_Path._wgrad's call: dW = dact^T . act with db as fused row sums, both into the slabs of one flat
    gradient layout (ldc = N, slab stride = the layout's total, the row sums behind the matrix)."""
    from har.models.mlp_paths import wgrad_tile
    from har.ops.gemm import gemm_bf16
    B, ks = 200, 128
    A, Bm, _ = GU.exact_inputs(M, N, B, seed=M + N)
    a, lda, b, ldb = GU.store_operands(A, Bm, 3, bf16, cuda)
    total = M * N + M + 64                       # W | b | other segments of the layout
    splits = (B + ks - 1) // ks
    slabs = torch.full((splits, total), float("nan"), device=cuda)
    gemm_bf16(a, b, slabs.view(-1), M=M, N=N, K=B, layout=3, epi=EPI_F32_SLAB, k_split=ks, ldc=N, slab_stride=total,
              rowsum=slabs.view(-1)[M * N:], slab_stride_rowsum=total, tile=wgrad_tile(M, N))
    o = GU.oracle(a, b, 3, EPI_F32_SLAB, k_ranges=GU.split_ranges(B, ks))
    got = slabs.cpu()
    tag = f"wgrad M={M} N={N} tile {wgrad_tile(M, N)}"
    GU.assert_equal(got[:, :M * N].reshape(splits, M, N), o.C, tag)
    GU.assert_equal(got[:, M * N:M * N + M], o.rowsum, tag + " rowsum")
    assert bool(torch.isnan(got[:, M * N + M:]).all()), tag + ": wrote past the row sums"


def test_gemm_naive_bayes_calls_exact(cuda):
    """naive_bayes.class_moments (onehot^T . [X, X^2]: fp32, layout 3, 32 slabs of auto_k_split) and
    predict_raw ([X, X^2] . Theta^T + b: fp32, layout 0, EPI_BIAS_F32), tiles by auto_tile."""
    from har.ops.gemm import auto_k_split, auto_tile, gemm_f32
    Kp, Fp, n = 8, 88, 1001
    A, Bm, _ = GU.exact_inputs(Kp, Fp, n, seed=5)
    a, lda, b, ldb = GU.store_operands(A, Bm, 3, f32, cuda)
    ks = auto_k_split(Kp, Fp, n)
    rng = GU.split_ranges(n, ks)
    assert auto_tile(Kp, Fp) == 3 and len(rng) == 32 and rng[-1] == (992, 1001)
    out = GU.guarded(Kp, Fp, f32, cuda, slabs=len(rng), ld=Fp)
    gemm_f32(a, b, out.view, M=Kp, N=Fp, K=n, layout=3, epi=EPI_F32_SLAB, k_split=ks, ldc=Fp,
             slab_stride=out.slab_stride)
    GU.assert_equal(out.result(), GU.oracle(a, b, 3, EPI_F32_SLAB, k_ranges=rng).C, "class_moments")
    out.check("class_moments")
    # scoring
    M, N, K = 1001, 8, 88
    A, Bm, bias = GU.exact_inputs(M, N, K, seed=6)
    a, lda, b, ldb = GU.store_operands(A, Bm, 0, f32, cuda)
    assert auto_tile(M, N) == 2
    out = GU.guarded(M, N, f32, cuda, ld=N)
    gemm_f32(a, b, out.view, M=M, N=N, K=K, layout=0, epi=EPI_BIAS_F32, bias=bias.to(f32).to(cuda))
    GU.assert_equal(out.result(), GU.oracle(a, b, 0, EPI_BIAS_F32, bias=bias).C, "predict_raw")
    out.check("predict_raw")


# ---------------------------------------------------------------------- d. accumulation numerics
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", TYPES, ids=_tname)
def test_gemm_accumulation_inside_the_fp32_summation_bound(cuda, dtype, layout):
    """Gaussian inputs (rounded to the kernel's type), K = 4104, automatic tile: every element within
    2 (K + 3) 2^-24 (|A| |B|)[m, n] of the fp64 product of the same inputs.  Largest error / bound measured
    on MI355X when the test was added: 1.8e-4 (bf16), 5.2e-4 (fp32) — the bound is a worst case over K
    aligned roundings, random ones grow like sqrt(K); the ratio is printed for later comparison."""
    M, N, K = 136, 136, 4104
    A, B = GU.gaussian_inputs(M, N, K, dtype, seed=40 + layout)
    a, lda, b, ldb = GU.store_operands(A, B, layout, dtype, cuda)
    out = GU.guarded(M, N, f32, cuda)
    _gemm(dtype)(a, b, out.view, M=M, N=N, K=K, layout=layout, epi=EPI_F32, tile=-1)
    err = (out.result().to(f64) - A @ B).abs()
    ratio = float((err / GU.sum_bound(A, B)).max())
    print(f"gemm {_tname(dtype)} layout {layout} K={K}: max error / bound = {ratio:.3e}")
    out.check("numerics")
    assert ratio <= 1.0


# ---------------------------------------------------------------------------- e. argument contract
def _call(kw):
    from har.ops.gemm import gemm_bf16
    kw = dict(kw)
    return gemm_bf16(kw.pop("A"), kw.pop("B"), kw.pop("C"), kw.pop("M"), kw.pop("N"), kw.pop("K"), **kw)


def test_gemm_argument_contract_on_device_tensors(cuda):
    """The refusals of tests/test_gemm_oracle.py with device tensors (nothing is launched), the valid
    neighbours run, and gemm_dispatch refuses the same pointers and pitches on its own."""
    from har.ops import _native
    for name, pattern, kw in GU.contract_cases(cuda):
        with pytest.raises(ValueError, match=pattern):
            _call(kw)
    for name, kw in GU.contract_ok_cases(cuda):
        _call(kw)
    torch.cuda.synchronize()
    M, N, K = 16, 16, 32
    A = torch.zeros(M, K, dtype=bf16, device=cuda)
    Bn = torch.zeros(K, N, dtype=bf16, device=cuda)
    C = torch.full((M, N), 1.0, dtype=bf16, device=cuda)
    mask = torch.ones(M + 1, N + 8, dtype=bf16, device=cuda)
    fl = torch.zeros(M + 8, device=cuda)

    def native(epi, bias=0, mask=0, rowsum=0, ldc=N, ldm=N + 8):
        _native.kernels().gemm(True, 2, epi, A.data_ptr(), Bn.data_ptr(), C.data_ptr(), bias, mask, rowsum, M, N, K,
                               K, N, ldc, ldm, 0, -1, 0, 0, 1.0, _native.stream_ptr())

    bad = [dict(epi=EPI_RELU_GRAD), dict(epi=EPI_RELU_GRAD, mask=mask.data_ptr() + 8),
           dict(epi=EPI_RELU_GRAD, mask=mask.data_ptr(), ldm=N + 4), dict(epi=EPI_RELU_GRAD, mask=mask.data_ptr(), ldm=8),
           dict(epi=EPI_RELU_GRAD, mask=mask.data_ptr(), ldc=N + 4), dict(epi=EPI_BIAS, ldc=N + 4),
           dict(epi=EPI_BIAS, bias=fl.data_ptr() + 2), dict(epi=EPI_BIAS, bias=fl.data_ptr(), rowsum=fl.data_ptr()),
           dict(epi=EPI_F32, rowsum=fl.data_ptr() + 1)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="contract violation"):
            native(**kw)
    torch.cuda.synchronize()
    assert float(C.float().min()) == 1.0 and float(C.float().max()) == 1.0   # nothing ran
    native(EPI_RELU_GRAD, mask=mask.data_ptr())
    torch.cuda.synchronize()
    assert float(C.float().abs().max()) == 0.0
