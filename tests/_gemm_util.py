"""fp64 oracle and input builders for the direct tests of the MFMA GEMM family (csrc/kernels/gemm.hip),
in plain torch on the CPU.

Two kinds of input:

* ``exact_inputs``: integer-valued operands in [-3, 3], a bias of multiples of 0.25, alpha = 0.5.  For
  every K the tests use per product (K <= 264 for the tile sweep, 1001 for the NaiveBayes shapes) each
  partial sum is an integer of magnitude <= 9 K < 2^24, so every fp32 summation order gives the same,
  exact, value; the bias add and the scaling by 0.5 are exact as well.  The kernel's fp32 results must
  then EQUAL the oracle's, and its bf16 results must equal the oracle's value rounded once to bf16 — no
  tolerance is involved.  (``test_gemm_oracle.py`` asserts the magnitude claim.)
* ``gaussian_inputs``: the accumulation-numerics case, held to the any-order fp32 summation bound
  ``2 (K + 3) 2^-24 (|A| |B|)[m, n]`` (``sum_bound``; factor 2 of margin over the textbook
  ``gamma_K``-style bound, for the unknown rounding of the matrix cores' internal adds).

Operands are laid out by ``stored`` with a pitch larger than the logical row and the padding filled
with a non-zero integer, so a kernel that reads into the padding changes the result; outputs come from
``guarded``: pitch N + 16, 64 guard elements before and after, one spare row, all pre-filled with a
sentinel bit pattern (quiet NaN 0x7FC00000 for fp32, 0x7FC1 for bf16) that ``Guarded.check`` looks for
again afterwards.
"""
from types import SimpleNamespace

import torch

EPI_F32, EPI_F32_ATOMIC, EPI_BIAS_RELU, EPI_BIAS, EPI_RELU_GRAD, EPI_BIAS_F32, EPI_F32_SLAB = range(7)
BF16_EPIS = (EPI_BIAS_RELU, EPI_BIAS, EPI_RELU_GRAD)
f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
ALPHA = 0.5
PAD_VALUE = 2.0          # what the operand padding holds
GUARD = 64               # guard elements before and after an output
BF16_SENTINEL = 0x7FC1   # a NaN no kernel here produces
MASK_BITS = (-0x4080, -0x8000, 0x0000, 0x3F80, 0x0008, 0x0008 - 0x8000)  # as int16, see exact_mask


def epv(dtype) -> int:
    """Elements per 16-byte vector."""
    return 8 if dtype == bf16 else 4


def a_is_mmajor(layout: int) -> bool:
    return bool(layout & 1)


def b_is_nmajor(layout: int) -> bool:
    return bool(layout & 2)


# ------------------------------------------------------------------------------------------ inputs
def exact_inputs(M: int, N: int, K: int, seed: int):
    """Logical A [M, K], B [K, N] (integers in [-3, 3]), bias [N] (multiples of 0.25 in [-2, 2]) in fp64."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-3, 4, (M, K), generator=g).to(f64)
    B = torch.randint(-3, 4, (K, N), generator=g).to(f64)
    bias = torch.randint(-8, 9, (N,), generator=g).to(f64) * 0.25
    return A, B, bias


def exact_mask(M: int, N: int, seed: int):
    """A bf16 [M, N] ReLU mask of the values that separate 'sign bit clear and not zero' from '> 0' done in
    another way: -1, -0.0, +0.0, 1, a bf16 denormal and its negative."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(MASK_BITS, dtype=torch.int16)
    return vals[torch.randint(0, len(MASK_BITS), (M, N), generator=g)].view(bf16)


def mask_passes(mask: torch.Tensor) -> torch.Tensor:
    """The kernels' mask rule on the bf16 bit pattern: sign bit clear and not zero."""
    return mask.contiguous().view(torch.int16) > 0


def gaussian_inputs(M: int, N: int, K: int, dtype, seed: int):
    """Logical Gaussian A [M, K], B [K, N] in fp64, already rounded to ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(dtype).to(f64)
    B = torch.randn(K, N, generator=g).to(dtype).to(f64)
    return A, B


def sum_bound(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Per-element bound on |fp32 sum in any order - exact| of the K products of A [M, K] . B [K, N]."""
    K = A.shape[1]
    return 2.0 * (K + 3) * U * (A.abs().to(f64) @ B.abs().to(f64))


def stored(X: torch.Tensor, transposed: bool, dtype, device):
    """The logical matrix X (or its transpose) as the kernel reads it: rows of pitch ``cols + 8 EPV`` with the
    padding set to PAD_VALUE.  Returns (view of the logical part, pitch); the view's ``stride(0)`` is the
    pitch and its storage is 16-byte aligned."""
    L = (X.T if transposed else X).to(dtype)
    rows, cols = L.shape
    ld = cols + 8 * epv(dtype)
    buf = torch.full((rows, ld), PAD_VALUE, dtype=dtype)
    buf[:, :cols] = L
    buf = buf.to(device)
    return buf[:, :cols], ld


def store_operands(A, B, layout: int, dtype, device):
    """(a_view, lda, b_view, ldb) of logical A [M, K], B [K, N] in the orientation ``layout`` asks for."""
    a, lda = stored(A, a_is_mmajor(layout), dtype, device)          # [K][M] if M-major else [M][K]
    b, ldb = stored(B, not b_is_nmajor(layout), dtype, device)      # [K][N] if N-major else [N][K]
    return a, lda, b, ldb


# ------------------------------------------------------------------------------------------ oracle
def logical(a_stored: torch.Tensor, b_stored: torch.Tensor, layout: int):
    """Logical A [M, K] and B [K, N] in fp64 from the stored orientations."""
    A = a_stored.to(f64).cpu()
    B = b_stored.to(f64).cpu()
    return (A.T if a_is_mmajor(layout) else A), (B if b_is_nmajor(layout) else B.T)


def oracle(A, B, layout, epi, bias=None, mask=None, alpha=1.0, k_ranges=None):
    """fp64 model of one gemm.hip call.  ``A`` / ``B`` are the operands in their STORED orientation (any
    dtype, no padding), ``k_ranges`` the [kb, ke) of each split for the split-K epilogues.  Returns
    ``C`` (rounded once to the epilogue's type; [splits, M, N] for EPI_F32_SLAB, else [M, N] — for
    EPI_F32_ATOMIC the amount ADDED to C) and ``rowsum`` (fp32 ``alpha sum_k A(m, k)``, per split for
    EPI_F32_SLAB), following the epilogue table at the top of gemm.hip."""
    Al, Bl = logical(A, B, layout)
    K = Al.shape[1]
    if epi == EPI_F32_SLAB:
        parts = [Al[:, kb:ke] @ Bl[kb:ke] for kb, ke in k_ranges]
        return SimpleNamespace(C=(alpha * torch.stack(parts)).to(f32),
                               rowsum=(alpha * torch.stack([Al[:, kb:ke].sum(1) for kb, ke in k_ranges])).to(f32))
    if k_ranges is not None:
        assert epi == EPI_F32_ATOMIC and k_ranges[0][0] == 0 and k_ranges[-1][1] == K
    acc = Al @ Bl
    rowsum = (alpha * Al.sum(1)).to(f32)
    if epi in (EPI_F32, EPI_F32_ATOMIC):
        C = (alpha * acc).to(f32)
    elif epi == EPI_BIAS_F32:
        C = (acc + (0 if bias is None else bias.to(f64).cpu())).to(f32)
    elif epi == EPI_BIAS:
        C = (acc + (0 if bias is None else bias.to(f64).cpu())).to(bf16)
    elif epi == EPI_BIAS_RELU:
        C = (acc + (0 if bias is None else bias.to(f64).cpu())).clamp_min(0).to(bf16)
    elif epi == EPI_RELU_GRAD:
        C = torch.where(mask_passes(mask.cpu()), acc, torch.zeros_like(acc)).to(bf16)
    else:
        raise ValueError(epi)
    return SimpleNamespace(C=C, rowsum=rowsum)


def split_ranges(K: int, k_split: int):
    return [(kb, min(K, kb + k_split)) for kb in range(0, K, k_split)]


# ------------------------------------------------------------------------------------------ outputs
class Guarded:
    """An output of ``slabs`` x ``rows`` x ``cols`` inside a sentinel-filled buffer: GUARD elements, then per
    slab rows + 1 rows of pitch ``ld`` (default cols + 16), then GUARD elements.  ``view`` is the
    [slabs * (rows + 1), ld] matrix the kernel is pointed at (``slab_stride`` apart), ``out`` the part a
    correct kernel writes."""

    def __init__(self, rows, cols, dtype, device, slabs=1, ld=None):
        self.rows, self.cols, self.slabs, self.dtype = rows, cols, slabs, dtype
        self.ld = cols + 16 if ld is None else ld
        self.slab_stride = (rows + 1) * self.ld
        self.ibits = torch.int16 if dtype == bf16 else torch.int32
        n = 2 * GUARD + slabs * self.slab_stride
        if dtype == bf16:
            flat = torch.full((n,), BF16_SENTINEL, dtype=torch.int16).view(bf16)
        else:
            flat = torch.full((n,), float("nan"), dtype=dtype)
        self.sentinel = int(flat.view(self.ibits)[0])
        self.flat = flat.to(device)
        self.view = self.flat[GUARD:n - GUARD].view(slabs * (rows + 1), self.ld)
        self.out = self.view.view(slabs, rows + 1, self.ld)[:, :rows, :cols]
        if slabs == 1:
            self.out = self.out[0]

    def fill(self, values):
        """Pre-set the output part (the accumulating epilogue adds to it)."""
        self.out.copy_(values.to(self.dtype).to(self.flat.device))

    def result(self):
        return self.out.cpu().contiguous()

    def check(self, tag=""):
        """Guards, pad columns and the spare rows still hold the sentinel bit pattern."""
        bits = self.flat.cpu().view(self.ibits).clone()
        n = bits.numel()
        inner = bits[GUARD:n - GUARD].view(self.slabs, self.rows + 1, self.ld)
        inner[:, :self.rows, :self.cols] = self.sentinel
        bad = (bits != self.sentinel).nonzero().flatten()
        assert bad.numel() == 0, f"{tag}: {bad.numel()} elements outside the output were written, first at flat " \
                                 f"offset {int(bad[0]) - GUARD} (pitch {self.ld}, rows {self.rows}, cols {self.cols})"


def guarded(rows, cols, dtype, device, slabs=1, ld=None) -> Guarded:
    return Guarded(rows, cols, dtype, device, slabs, ld)


def assert_equal(got: torch.Tensor, want: torch.Tensor, tag: str):
    """torch.equal with a report of where the first difference is."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    diff = ~(got == want)
    idx = diff.nonzero()
    first = tuple(int(i) for i in idx[0])
    rows = sorted({int(i[-2]) for i in idx})[:8] if got.dim() >= 2 else []
    cols = sorted({int(i[-1]) for i in idx})[:8]
    raise AssertionError(f"{tag}: {idx.shape[0]} of {got.numel()} elements differ; first at {first}: got "
                         f"{float(got[first])}, want {float(want[first])}; rows {rows} cols {cols}")


# -------------------------------------------------------------------------------- argument contract
def contract_cases(device):
    """(name, message pattern, kwargs of gemm_bf16) of calls ops/gemm.py must refuse; ``device`` may be the CPU:
    the refusals come before the device check."""
    M, N, K = 16, 16, 32
    A = torch.zeros(M, K, dtype=bf16, device=device)
    B = torch.zeros(N, K, dtype=bf16, device=device)
    Bn = torch.zeros(K, N, dtype=bf16, device=device)
    Cb = torch.zeros(M, N + 16, dtype=bf16, device=device)
    Cn = torch.zeros(M, N + 4, dtype=bf16, device=device)
    Cf = torch.zeros(M, N, dtype=f32, device=device)
    bias = torch.zeros(N + 4, dtype=f32, device=device)
    rs = torch.zeros(M + 4, dtype=f32, device=device)
    wide = torch.zeros(M + 1, N + 16, dtype=bf16, device=device)
    flatm = torch.zeros((M + 1) * (N + 12) + 8, dtype=bf16, device=device)

    class Shifted:  # a tensor whose pointer is off by some bytes (torch refuses to build one of floats)
        def __init__(self, t, nbytes):
            self.t, self.nbytes = t, nbytes

        def data_ptr(self):
            return self.t.data_ptr() + self.nbytes

    fwd = dict(A=A, B=B, C=Cb[:, :N], M=M, N=N, K=K, layout=0)
    dgr = dict(A=A, B=Bn, C=Cb[:, :N], M=M, N=N, K=K, layout=2, epi=EPI_RELU_GRAD)
    f32o = dict(A=A, B=B, C=Cf, M=M, N=N, K=K, layout=0, epi=EPI_F32)
    return [
        ("ldc_mod_8", "ldc", dict(fwd, epi=EPI_BIAS, bias=bias[:N], ldc=N + 4)),
        ("ldc_mod_8_relu", "ldc", dict(fwd, epi=EPI_BIAS_RELU, bias=bias[:N], C=Cn[:, :N])),
        ("ldc_mod_8_relu_grad", "ldc", dict(dgr, mask=wide[:M, :N], ldc=N + 12)),
        ("ldmask_mod_8", "ldmask", dict(dgr, mask=flatm[:(M + 1) * (N + 12)].view(M + 1, N + 12)[:M, :N])),
        ("mask_missing", "needs a mask", dict(dgr)),
        ("mask_misaligned", "mask must be 16-byte aligned", dict(dgr, mask=wide[:M, 4:N + 4])),
        ("mask_narrow", "smaller than the output", dict(dgr, mask=wide[:M, :N - 8])),
        ("mask_short", "smaller than the output", dict(dgr, mask=wide[:M - 1, :N])),
        ("bias_misaligned", "bias must be 4-byte aligned", dict(fwd, epi=EPI_BIAS, bias=Shifted(bias, 2))),
        ("bias_misaligned_f32", "bias must be 4-byte aligned", dict(f32o, epi=EPI_BIAS_F32, bias=Shifted(bias, 1))),
        ("rowsum_misaligned", "rowsum must be 4-byte aligned", dict(f32o, rowsum=Shifted(rs, 2))),
        ("rowsum_bf16_epilogue", "rowsum is not supported", dict(fwd, epi=EPI_BIAS, bias=bias[:N], rowsum=rs[:M])),
        ("rowsum_relu_grad", "rowsum is not supported", dict(dgr, mask=wide[:M, :N], rowsum=rs[:M])),
    ]


def contract_ok_cases(device):
    """Calls that satisfy the contract (the closest neighbours of the refused ones)."""
    M, N, K = 16, 16, 32
    A = torch.zeros(M, K, dtype=bf16, device=device)
    B = torch.zeros(N, K, dtype=bf16, device=device)
    Bn = torch.zeros(K, N, dtype=bf16, device=device)
    Cb = torch.zeros(M, N + 16, dtype=bf16, device=device)
    Cf = torch.zeros(M, N, dtype=f32, device=device)
    bias = torch.zeros(N + 4, dtype=f32, device=device)
    rs = torch.zeros(M + 4, dtype=f32, device=device)
    wide = torch.zeros(M + 1, N + 16, dtype=bf16, device=device)
    return [
        ("bias_offset_4_bytes", dict(A=A, B=B, C=Cb[:, :N], M=M, N=N, K=K, layout=0, epi=EPI_BIAS, bias=bias[1:N + 1])),
        ("relu_grad_wide_mask", dict(A=A, B=Bn, C=Cb[:, :N], M=M, N=N, K=K, layout=2, epi=EPI_RELU_GRAD,
                                     mask=wide[:M, 8:N + 8])),
        ("rowsum_f32", dict(A=A, B=B, C=Cf, M=M, N=N, K=K, layout=0, epi=EPI_F32, rowsum=rs[1:M + 1])),
    ]
