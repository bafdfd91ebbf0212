"""Exact-arithmetic data, an fp64 oracle and the layout rules for the direct tests of the fused MLP kernels
(csrc/kernels/mlp_step.hip, mlp_fused.hip, mlp_small.hip, mlp_pack_frag in mlp.hip), in plain torch on the CPU.

The data (``make_case``) is built so that every fp32 accumulation of every kernel is exact in any order:
all terms of a sum are multiples of one quantum q and sum |terms| < 2^24 q (``margins`` computes the ratios,
tests/test_mlp_exact_oracle.py asserts them).  Each output of each kernel then has ONE correct value:

* X: integers in [-3, 3], more than half of them zero, some -0.0; columns >= F are zero padding.
* W0 / W1: sparse, +-{0.5, 1} / +-{1, 2}; b0 / b1: odd multiples of 2^-6 near minus the unit's median input.  Pre-activations are multiples of
  2^-6 up to a few tens: a share of them needs rounding to bf16 (8 significant bits), an odd multiple of
  2^-6 in [4, 8) is an exact halfway case.  h = RNE_bf16(relu(exact)).
* 16 "code" columns of X carry 3 in the column of the row's code s (<= 1 elsewhere); the layer-1 selector unit
  of code s is live (1.5) on exactly those rows, and gates two layer-2 units: A_s (h2 = 4, Wout[s mod C] =
  192 + 2 s, 0 for the other classes) and two B_s (h2 = 1, dense Wout columns of multiples of 0.25, 32 <= |w| < 64).
  The A units put the logit of class s mod C at least 112 above every other one: exp underflows to 0 in
  fp32, p is one-hot, dz = scale (onehot(argmax) - onehot(y)), the row loss is z_max - z_y.  The B columns
  give dact2 = RNE_bf16(dz . Wout) differences of two such weights: 9 significant bits where the signs differ,
  halfway cases in both directions; through W1 they meet the A column's share at the selector unit, so dact1 needs
  rounding as well.
* Wout rows >= C and bout entries >= C hold the canary 2.0 (a kernel that lets them into a gradient fails).
* ``tie=True`` (C a power of two): every Wout row < C is the same except on units that b1 = -512 keeps dead
  on every row, bout is constant: all logits of a row are equal, p = 1 / C exactly, dact2 = 0.

The oracle (``oracle``) is fp64 forward + backprop with the kernels' rounding points; ``round_bf16=False`` turns it
into plain backprop (checked against torch.autograd).  Gradients come per row range (``grads``).

Each layout rule of the kernels lives in exactly one function here.
"""
from types import SimpleNamespace

import torch

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
NCLS = 16                 # padded classes
NCODE = 16                # selector codes
CANARY = 2.0              # Wout rows / bout entries >= C
SCALE = 2.0 ** -6         # the tests' loss scale (the kernels take it as a free argument)
GAP = 112.0               # top-1 minus top-2 logit at which fp32 exp(z - max) is exactly 0
EXP_ZERO = -104.0         # fp32 exp underflows to 0 below this (2^-150)
DEAD_BIAS = -512.0
FEATURES = {32: 20, 64: 43}  # default real feature counts of the padded widths


# ------------------------------------------------------------------------------------------ layout rules
def step_grid(B: int) -> int:
    """har_mlp_step_grid: workgroups of mlp_fwd3 (32-row tiles, at most 256)."""
    return max(1, min(256, B // 32))


def step_fwd_rows(B: int, wg: int):
    """Row indices of forward workgroup ``wg``: tiles wg + k * grid of 32 rows."""
    idx = [torch.arange(32 * t, 32 * t + 32) for t in range(wg, B // 32, step_grid(B))]
    return torch.cat(idx) if idx else torch.zeros(0, dtype=torch.long)


def step_fwd_slab_width(H: int) -> int:
    """har_mlp_step_fwd_slab_width: dWout rows 0..15 [16][H], dbout [16]."""
    return NCLS * H + NCLS


def step_slices(B: int) -> int:
    """har_mlp_step_slices: row slices of mlp_bwd4 (64-row tiles)."""
    tiles = B // 64
    return max(1, min(64, max(tiles // 4, min(tiles, 16))))


def step_bwd_rows(B: int, s: int):
    """[r0, r1) of backward row slice ``s`` (empty for the trailing slices of some batches)."""
    tiles, S = B // 64, step_slices(B)
    per = (tiles + S - 1) // S
    t0 = s * per
    n = max(0, min(tiles, t0 + per) - t0)
    return 64 * t0, 64 * (t0 + n)


def unswizzle_dact2(d: torch.Tensor) -> torch.Tensor:
    """mlp_step_fwd's dact2 [B][256] -> logical order: the 16-byte chunks (8 bf16) of rows with bit 2 set are
    swapped in pairs (column ^ 8)."""
    B, H = d.shape
    v = d.reshape(B, H // 16, 2, 8)
    odd = ((torch.arange(B, device=d.device) >> 2) & 1).bool()
    return torch.where(odd[:, None, None, None], v.flip(2), v).reshape(B, H)


def fwd_head_grid(B: int) -> int:
    """har_mlp_fwd_head_grid."""
    return max(1, min(256, (B // 16 + 1) // 2))


def fwd_head_rows(B: int, wg: int):
    """Row indices of mlp_fwd_head workgroup ``wg``: 16-row tiles 4 wg + wave + 4 k grid (4 waves)."""
    grid, nt = fwd_head_grid(B), B // 16
    idx = [torch.arange(16 * t, 16 * t + 16) for w in range(4) for t in range(4 * wg + w, nt, 4 * grid)]
    return torch.cat(idx) if idx else torch.zeros(0, dtype=torch.long)


def fwd_head_slab_width(H: int) -> int:
    """mlp_fwd_head's slab pitch: dWout [16][H], dbout [16], and an H-float slot it leaves unwritten."""
    return NCLS * H + NCLS + H


def flat_offsets(K0: int, H: int):
    """The flat parameter layout (W0, b0, W1, b1, Wout, bout) the partial slabs follow: name -> (offset, shape)."""
    o, out = 0, {}
    for name, shape in (("W0", (H, K0)), ("b0", (H,)), ("W1", (H, H)), ("b1", (H,)), ("Wout", (NCLS, H)),
                        ("bout", (NCLS,))):
        out[name] = (o, shape)
        o += int(torch.tensor(shape).prod())
    out["total"] = o
    return out


# ------------------------------------------------------------------------------------------ data
def _pick(g, values, shape):
    v = torch.tensor(values, dtype=f64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _centred_bias(pre, g):
    """Per unit: minus the median of its bias-free pre-activation over the rows (so it is live on some rows and
    dead on others at every batch size), rounded down to an integer, plus a fraction of odd 64ths."""
    frac = (2 * torch.randint(0, 32, (pre.shape[1],), generator=g) + 1).to(f64) / 64
    return -(pre.median(0).values.floor()) - frac


def make_case(B: int, K0: int, H: int, C: int, F: int = None, seed: int = 0, tie: bool = False):
    assert K0 in (32, 64) and H in (128, 256) and 1 <= C <= NCLS and B % 16 == 0
    F = FEATURES[K0] if F is None else F
    assert NCODE <= F <= K0
    g = torch.Generator().manual_seed(1000003 * seed + 8191 * B + 131 * K0 + 17 * H + C + (7 if tie else 0))
    # ---- unit roles (scattered over the hidden units, not aligned with the kernels' 16-unit tiles)
    p1, p2 = torch.randperm(H, generator=g), torch.randperm(H, generator=g)
    sel1, selA, selB = p1[:NCODE], p2[:NCODE], p2[NCODE:3 * NCODE]   # two B units per code
    dead2 = p2[3 * NCODE:3 * NCODE + 32] if tie else p2[:0]
    cols = torch.randperm(F, generator=g)[:NCODE]
    # ---- codes: every 16-row block holds each code once; classes a = code mod C
    code = torch.cat([torch.randperm(NCODE, generator=g) for _ in range(B // 16)])
    # ---- X
    X = torch.randint(-3, 4, (B, K0), generator=g).to(f64) * (torch.rand(B, K0, generator=g) < 0.5)
    X[:, cols] = torch.randint(-1, 2, (B, NCODE), generator=g).to(f64)
    X[torch.arange(B), cols[code]] = 3.0
    X[:, F:] = 0.0
    neg = (X == 0) & (torch.rand(B, K0, generator=g) < 0.25)
    neg[:, F:] = False
    X = torch.where(neg, torch.tensor(-0.0, dtype=f64), X)
    # ---- layer 1
    W0 = _pick(g, [-1, -0.5, 0.5, 1], (H, K0)) * (torch.rand(H, K0, generator=g) < min(1.0, 10.0 / F))
    W0[:, F:] = 0.0
    b0 = _centred_bias(X @ W0.T, g)
    W0[sel1] = 0.0
    W0[sel1, cols] = 1.0
    b0[sel1] = -1.5
    # ---- layer 2
    W1 = _pick(g, [-2, -1, 1, 2], (H, H)) * (torch.rand(H, H, generator=g) < 12.0 / H)
    W1[selA] = 0.0
    W1[selB] = 0.0
    W1[selA, sel1] = 4.0
    W1[selB, sel1.repeat(2)] = 1.0
    h1 = rne_bf16((X @ W0.T + b0).clamp_min(0))
    b1 = _centred_bias(h1 @ W1.T, g)
    b1[selA] = -2.0
    b1[selB] = -0.5
    b1[dead2] = DEAD_BIAS
    # ---- head
    Wout = torch.full((NCLS, H), CANARY, dtype=f64)
    bout = torch.full((NCLS,), CANARY, dtype=f64)
    Wr = _pick(g, [-2, -1, 1, 2], (NCLS, H)) * (torch.rand(NCLS, H, generator=g) < 8.0 / H)
    Wr[:, selA] = 0.0
    # multiples of 0.25 with 32 <= |w| < 64: the difference of two of opposite sign has 9 significant bits
    Wr[:, selB] = (torch.randint(128, 256, (NCLS, 2 * NCODE), generator=g).to(f64) / 4
                   * _pick(g, [-1, 1], (NCLS, 2 * NCODE)))
    Wr[torch.arange(NCODE) % C, selA] = 192.0 + 2 * torch.arange(NCODE).to(f64)
    br = torch.randint(-8, 9, (NCLS,), generator=g).to(f64) / 4
    if tie:
        assert C & (C - 1) == 0, "p = 1 / C is exact for a power of two"
        Wt = _pick(g, [-2, -1, 1, 2], (1, H)) * (torch.rand(1, H, generator=g) < 16.0 / H)
        Wt = Wt.expand(NCLS, H).clone()
        Wt[:, dead2] = torch.randint(-160, 161, (NCLS, dead2.numel()), generator=g).to(f64) / 4
        Wr, br = Wt, torch.full((NCLS,), 0.75, dtype=f64)
    Wout[:C], bout[:C] = Wr[:C], br[:C]
    # ---- labels: two rows of five get the argmax of another such row (sorted by class and shifted by the longest
    # run, so nearly all of them are wrong and every class stays a label); the others keep their argmax.  Then one
    # more row is mislabelled, so that the label counts differ from the argmax counts (dbout != 0).
    a = code % C
    y = a.clone()
    wrong = torch.arange(B) % 5 % 2 == 1
    if tie:
        y = torch.randint(0, C, (B,), generator=g)
        y[:C] = torch.arange(C)      # every class is a label
        if bool((torch.bincount(y, minlength=C) == B // C).all()):   # (not evenly: dbout = scale (B / C - counts))
            y[C] = (y[C] + 1) % C
    elif C > 1:
        w = wrong.nonzero().flatten()
        w = w[torch.argsort(a[w], stable=True)]
        y[w] = a[w.roll(-int(torch.bincount(a[w], minlength=C).max()))]
        spare = (~wrong & (torch.bincount(y, minlength=C)[a] >= 2)).nonzero().flatten()
        if spare.numel():
            y[spare[0]] = (a[spare[0]] + 1) % C
    for t in (W0, W1, Wout, X):
        assert torch.equal(t.to(bf16).to(f64), t), "operands are bf16 values"
    return SimpleNamespace(B=B, K0=K0, H=H, C=C, F=F, tie=tie, X=X, W0=W0, b0=b0, W1=W1, b1=b1, Wout=Wout, bout=bout,
                           y=y, code=code, sel1=sel1, selA=selA, selB=selB, dead2=dead2, scale=SCALE)


# ------------------------------------------------------------------------------------------ oracle
def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp64 values that are exact in fp32 -> nearest bf16 (ties to even), back in fp64."""
    assert torch.equal(x.to(f32).to(f64), x), "the value is not an fp32 number: the construction is broken"
    return x.to(f32).to(bf16).to(f64)


def first_argmax(z: torch.Tensor) -> torch.Tensor:
    """Lowest index at the row maximum."""
    return (z == z.max(1, keepdim=True).values).to(torch.int8).argmax(1)


def oracle(c, round_bf16: bool = True, scale: float = None):
    """fp64 forward and backprop of the case.  With ``round_bf16``: h1, h2, dz, dact2, dact1 rounded once to bf16
    and exp(z - max) flushed to 0 where fp32 underflows; pre = the values before each rounding."""
    scale = c.scale if scale is None else scale
    rnd = rne_bf16 if round_bf16 else (lambda t: t)
    C, B = c.C, c.B
    a1 = (c.X @ c.W0.T + c.b0).clamp_min(0)
    h1 = rnd(a1)
    a2 = (h1 @ c.W1.T + c.b1).clamp_min(0)
    h2 = rnd(a2)
    z = h2 @ c.Wout[:C].T + c.bout[:C]
    mx = z.max(1, keepdim=True).values
    d = z - mx
    e = torch.exp(d)
    if round_bf16:
        e = torch.where(d <= EXP_ZERO, torch.zeros_like(e), e)
    se = e.sum(1, keepdim=True)
    onehot = torch.nn.functional.one_hot(c.y, C).to(f64)
    loss = (mx + torch.log(se)).squeeze(1) - z[torch.arange(B), c.y]
    dzp = torch.zeros(B, NCLS, dtype=f64)
    dzp[:, :C] = (e / se - onehot) * scale
    dz = rnd(dzp)
    d2p = (dz[:, :C] @ c.Wout[:C]) * (h2 > 0)
    dact2 = rnd(d2p)
    d1p = (dact2 @ c.W1) * (h1 > 0)
    dact1 = rnd(d1p)
    amax = first_argmax(z)
    return SimpleNamespace(h1=h1, h2=h2, z=z, argmax=amax, loss=loss, correct=(amax == c.y), dz=dz, dact2=dact2,
                           dact1=dact1, pre=dict(h1=a1, h2=a2, dz=dzp, dact2=d2p, dact1=d1p), p=e / se)


def grads(c, o, rows):
    """The six gradient segments of the rows ``rows`` (a slice or an index tensor), fp64; Wout / bout padded to 16."""
    X, h1, h2, dz, d2, d1 = c.X[rows], o.h1[rows], o.h2[rows], o.dz[rows], o.dact2[rows], o.dact1[rows]
    return {"W0": d1.T @ X, "b0": d1.sum(0), "W1": d2.T @ h1, "b1": d2.sum(0), "Wout": dz.T @ h2, "bout": dz.sum(0)}


def flat_grad(c, g) -> torch.Tensor:
    """``grads`` in the flat parameter layout, fp32."""
    offs = flat_offsets(c.K0, c.H)
    out = torch.zeros(offs["total"], dtype=f64)
    for name, t in g.items():
        o = offs[name][0]
        out[o:o + t.numel()] = t.reshape(-1)
    return to_f32(out)


def to_f32(x: torch.Tensor) -> torch.Tensor:
    assert torch.equal(x.to(f32).to(f64), x), "an oracle value is not exact in fp32"
    return x.to(f32)


# ------------------------------------------------------------------------------------------ exactness margins
def _quantum(*ts) -> float:
    """The largest power of two that divides every value of the tensors."""
    q = 1.0
    v = torch.cat([t.reshape(-1) for t in ts])
    v = v[v != 0]
    while v.numel() and not torch.equal(v / q, (v / q).round()):
        q /= 2
        assert q > 2.0 ** -40
    return q


def _quanta(A) -> torch.Tensor:
    """Per row of A: the largest power of two that divides every value of the row."""
    q = torch.ones(A.shape[0], dtype=f64)
    for _ in range(40):
        bad = ((A / q[:, None]) != (A / q[:, None]).round()).any(1)
        if not bool(bad.any()):
            return q
        q = torch.where(bad, q / 2, q)
    raise AssertionError("no quantum above 2^-40")


def _ratio(A, Bm, bias=None) -> float:
    """max over outputs [m, n] of sum_k |A[m, k] B[k, n]| (+ |bias[n]|) / quantum of those terms (the quantum of
    row m of A times that of column n of B, and the bias's), as log2."""
    s = A.abs() @ Bm.abs()
    q = _quanta(A)[:, None] * _quanta(Bm.T)[None, :]
    if bias is not None:
        s = s + bias.abs()
        q = torch.minimum(q, _quanta(bias[:, None])[None, :])
    return float(torch.log2((s / q).max().clamp_min(1e-300)))


def margins(c, o, partial_rows, loss_rows=()):
    """log2(sum |terms| / quantum) of every accumulation: the forward products, and each gradient and the loss over
    each of ``partial_rows`` / ``loss_rows`` (the kernels' partials; the caller adds the whole batch where a total is formed).
    Below 24: exact in fp32 in any order."""
    C = c.C
    m = {"a1": _ratio(c.X, c.W0.T, c.b0), "a2": _ratio(o.h1, c.W1.T, c.b1),
         "z": _ratio(o.h2, c.Wout[:C].T, c.bout[:C]),
         "dact2": _ratio(o.dz[:, :C], c.Wout[:C]), "dact1": _ratio(o.dact2, c.W1),
         "loss": -1e9}
    ones = torch.ones(c.B, 1, dtype=f64)
    for rows in loss_rows:
        if o.loss[rows].numel():
            m["loss"] = max(m["loss"], float(torch.log2(o.loss[rows].abs().sum().clamp_min(1e-300) / _quantum(o.loss))))
    for rows in partial_rows:
        X, h1, h2, dz, d2, d1 = c.X[rows], o.h1[rows], o.h2[rows], o.dz[rows], o.dact2[rows], o.dact1[rows]
        if X.shape[0] == 0:
            continue
        for name, (A, Bm) in {"W0": (d1.T, X), "b0": (d1.T, ones[rows]), "W1": (d2.T, h1), "b1": (d2.T, ones[rows]),
                              "Wout": (dz.T, h2), "bout": (dz.T, ones[rows])}.items():
            m["d" + name] = max(m.get("d" + name, -1e9), _ratio(A, Bm))
    return m


def needs_rounding(pre: torch.Tensor):
    """(needs rounding, halfway and rounded DOWN to an even neighbour, halfway and rounded UP to an even neighbour)
    of fp64 values to bf16."""
    r = pre.to(f32).to(bf16).to(f64)
    inexact = r != pre
    bits = pre.to(f32).view(torch.int32)
    half = inexact & ((bits & 0xFFFF) == 0x8000)
    return inexact, half & (r.abs() < pre.abs()), half & (r.abs() > pre.abs())


# ------------------------------------------------------------------------------------------ device side
def dev_case(c, dev):
    """The case's operands as the kernels take them."""
    return SimpleNamespace(X=c.X.to(bf16).to(dev), W0=c.W0.to(bf16).to(dev), W1=c.W1.to(bf16).to(dev),
                           Wout=c.Wout.to(bf16).to(dev), b0=c.b0.to(f32).to(dev), b1=c.b1.to(f32).to(dev),
                           bout=c.bout.to(f32).to(dev), y=c.y.to(torch.int32).to(dev))


def bits16(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------ the cases
# (kind, B, K0, H, C, tie) of every case the GPU files run; tests/test_mlp_exact_oracle.py holds each to the
# conditions above.  kind names the kernel whose partials the case must keep exact.
def _cases():
    out = []
    for K0 in (32, 64):
        for C in (1, 2, 6, 15, 16):
            out += [("step_fwd", B, K0, 256, C, False) for B in (64, 192, 1088, 8256)]
        out += [("step_bwd", B, K0, 256, 6 if K0 == 64 else 16, False) for B in (64, 128, 1088, 2560, 4160)]
    for H in (128, 256):
        for C in (1, 6, 16):
            out += [("fwd_head", B, K0, H, C, False) for K0 in (32, 64) for B in (16, 48, 80)]
            out += [("small", B, 64 if (H == 256) != (C == 6) else 32, H, C, False) for B in (32, 96, 512)]
    for C in (2, 4, 8, 16):
        out += [("step_fwd", 64, 64, 256, C, True), ("fwd_head", 48, 32, 128, C, True), ("small", 64, 32, 256, C, True)]
    return out


CASES = _cases()
_cache = {}


def cases_of(kind: str, tie: bool = False):
    return [k for k in CASES if k[0] == kind and k[5] == tie]


def case_id(k) -> str:
    return f"{k[0]}-B{k[1]}-K{k[2]}-H{k[3]}-C{k[4]}" + ("-tie" if k[5] else "")


def get_case(k):
    """(case, oracle) of a CASES entry, built once and shared: treat both as read-only."""
    key = k[1:]
    if key not in _cache:
        c = make_case(k[1], k[2], k[3], k[4], tie=k[5])
        _cache[key] = (c, oracle(c))
    return _cache[key]


def partial_rows(kind: str, B: int):
    """The row sets whose gradients one workgroup / slice of ``kind`` sums."""
    if kind == "step_fwd":
        return [step_fwd_rows(B, w) for w in range(step_grid(B))]
    if kind == "step_bwd":   # its forward's slabs as well
        return [slice(*step_bwd_rows(B, s)) for s in range(step_slices(B))] + partial_rows("step_fwd", B)

    if kind == "fwd_head":
        return [fwd_head_rows(B, w) for w in range(fwd_head_grid(B))]
    if kind == "small":
        return [slice(r, r + 32) for r in range(0, B, 32)]
    raise ValueError(kind)
