"""fp64 oracle of ONE phase-1 (direction + trial points) and ONE phase-2 (pick + history update) step
of the batched L-BFGS / OWL-QN kernels (csrc/kernels/logreg_qn.hip), in plain torch on the CPU.

The math is the one of ``optim.lbfgs.minimize_trials``.  The direction is the textbook two-loop
recursion on the history VECTORS (``q = pg - sum al_j y_j``, ``r = gamma q + sum w_j s_j``), not the
kernel's recursion on the Gram matrices ``SY`` / ``YY`` / ``P1``: an indexing mistake in those shows as a
difference.  Every quantity comes with the error bound the tests hold the kernels to (u = 2^-24):

* ``d``: ``2 (2m + 4) u A_e``, ``A_e = |gamma pg_e| + sum_j |cY_j y_je| + |cS_j s_je|`` (coefficients
  rounded to fp32, a chain of 2m + 1 fp32 fmas; the leading 2 is slack for the fp32 ``pg``);
* ``xtrial``: ``step * bound_d + 2u |value|``; ``weff``: ``|scale| bound_xtrial + 3u |value|``;
* block sums: ``2 (n_l + 2) u sum |terms|`` (``n_l`` fp32 fmas per lane before the fp64 tree) plus the
  propagated elementwise bounds of the inputs; fp64 scalars: the propagated bound of their inputs;
* decisions on fp32 signs (``d * pg >= 0``, ``sgn(xn) != xi``): an element within its own bound of the
  boundary is excluded from the elementwise comparison and its possible contribution added to the
  bounds of the sums.
"""
import math
from types import SimpleNamespace

import torch

U = 2.0 ** -24
QN_MAX_M, QN_MAX_TRIALS, QN_BLOCK, QN_MAX_CHUNKS = 10, 4, 256, 32
NP1, NP2, NP3 = 2 * QN_MAX_M + 1, 3 * QN_MAX_TRIALS + 2, 5 + 3 * QN_MAX_M
f64, f32, i32 = torch.float64, torch.float32, torch.int32

# The single-step input sets: the smallest shapes that reach each path of the two kernels.
#   chunk: elements per phase-1 chunk class ("lt256", "256..768", "gt1536"), tile: LDS W_eff tile
CASES = [
    dict(name="one_chunk_empty", K=3, Fp1=17, B=2, T=4, m=10, head=0, filled=0, nch=1, tile=False, chunk="lt256"),
    dict(name="one_chunk_fill4", K=3, Fp1=17, B=2, T=4, m=10, head=4, filled=4, nch=1, tile=False, chunk="lt256"),
    dict(name="wrapped", K=6, Fp1=44, B=3, T=4, m=10, head=3, filled=10, nch=2, tile=False, chunk="lt256",
         rho0=(7,)),
    dict(name="kp16_m4_full", K=12, Fp1=71, B=2, T=3, m=4, head=1, filled=4, nch=4, tile=False, chunk="lt256",
         rho0=(2,)),
    dict(name="kp16_m4_fill2", K=12, Fp1=71, B=2, T=3, m=4, head=2, filled=2, nch=4, tile=False, chunk="lt256",
         rho0=(1,)),
    dict(name="kp16_m1", K=12, Fp1=71, B=2, T=3, m=1, head=0, filled=1, nch=4, tile=False, chunk="lt256"),
    dict(name="kp8_m3", K=6, Fp1=44, B=2, T=2, m=3, head=0, filled=3, nch=2, tile=False, chunk="lt256"),
    dict(name="chunks32", K=16, Fp1=497, B=2, T=2, m=10, head=9, filled=10, nch=32, tile=False, chunk="256..768"),
    dict(name="tile", K=6, Fp1=44, B=256, T=4, m=10, head=5, filled=7, nch=2, tile=True, chunk="lt256",
         rho0=(3,)),
    dict(name="tile_chunks", K=3, Fp1=257, B=128, T=2, m=5, head=0, filled=5, nch=4, tile=True, chunk="lt256"),
    dict(name="refill", K=5, Fp1=332, B=260, T=1, m=10, head=2, filled=10, nch=1, tile=True, chunk="gt1536"),
]


def case_id(c):
    return c["name"]


def kp_of(K):
    return 8 if K <= 8 else 16


def qn_chunks_rule(D, B, budget=512):
    """har_qn_chunks: at most ``budget`` workgroups over the B models, at most 32 chunks per model, at
    least 256 elements per chunk."""
    return max(1, min(QN_MAX_CHUNKS, budget // max(B, 1), (D + 255) // 256))


def dispatch_path(K, Fp1, B, T, m, nch, init=0):
    """What har_lbfgs_phase launches for this shape: KP, the FULLM instantiation, the LDS W_eff tile, and
    the sizes that decide which prefetch branches run."""
    KP = kp_of(K)
    ccs = (Fp1 + nch - 1) // nch
    wb = (1 if init else T) * KP * ccs * 4
    el1 = ccs * K                                # elements of a (full) phase-1 chunk
    el2 = (K * Fp1 + nch - 1) // nch             # elements of a (full) phase-2 chunk
    cls = lambda n: "lt256" if n < 256 else "256..768" if n <= 768 else "gt1536" if n > 1536 else "769..1536"  # noqa: E731
    return dict(KP=KP, fullm=m == QN_MAX_M, tile=wb <= 64 * 1024 and nch * B >= 256, ccs=ccs, el1=el1, el2=el2,
                chunk=cls(el1), chunk2=cls(el2))


def ring(m, head, filled):
    """History slots, newest first."""
    return [(head - 1 - i) % m for i in range(filled)]


def pseudo_grad(x, g, l1):
    if l1 is None:
        return g.clone()
    gp, gm = g + l1, g - l1
    z = torch.where(gp < 0, gp, torch.where(gm > 0, gm, torch.zeros_like(g)))
    return torch.where(x > 0, gp, torch.where(x < 0, gm, z))


def _dot(a, b):
    return (a * b).sum(-1)


def gram_from_history(st):
    """SY, YY, rho (1 / s.y) and the P1 totals of the state's own S, Y, x, g, in fp64, over the ring slots."""
    B, m = st.B, st.m
    S, Y = st.S.double(), st.Y.double()
    SY = torch.zeros(B, m, m, dtype=f64)
    YY = torch.zeros(B, m, m, dtype=f64)
    P1 = torch.zeros(B, NP1, dtype=f64)
    pg = pseudo_grad(st.x.double(), st.g.double(), None if st.l1 is None else st.l1.double())
    slots = ring(m, st.head, st.filled)
    for i in slots:
        for j in slots:
            SY[:, i, j] = _dot(S[i], Y[j])
            YY[:, i, j] = _dot(Y[i], Y[j])
        P1[:, i] = _dot(S[i], pg)
        P1[:, QN_MAX_M + i] = _dot(Y[i], pg)
    P1[:, 2 * QN_MAX_M] = _dot(pg, pg)
    return SY, YY, P1


def fill_history(st, gen, rho0=()):
    """A consistent history for the state's (m, head, filled): random s_j, y_j = A s_j with a positive
    diagonal A in [0.5, 2] (every s.y > 0), SY / YY / rho / P1 totals from them in fp64; the slots in
    ``rho0`` are marked rejected (rho = 0, pair kept).  Slots outside the ring hold finite junk in S, Y
    (never valid input) and zeros in rho and the Gram matrices."""
    B, D, m = st.B, st.D, st.m
    st.S = (0.05 * torch.randn(m, B, D, generator=gen)).float()
    st.Y = (0.05 * torch.randn(m, B, D, generator=gen)).float()
    for j in ring(m, st.head, st.filled):
        A = 0.5 + 1.5 * torch.rand(B, D, generator=gen)
        st.S[j] = (0.1 * torch.randn(B, D, generator=gen)).float()
        st.Y[j] = (A * st.S[j]).float()
    st.SY, st.YY, st.P1 = gram_from_history(st)
    st.rho = torch.zeros(m, B, dtype=f64)
    for j in ring(m, st.head, st.filled):
        assert bool((st.SY[:, j, j] > 0).all())
        st.rho[j] = 0.0 if j in rho0 else 1.0 / st.SY[:, j, j]
    st.rho0 = tuple(rho0)
    return st


def make_state(K, Fp1, B, T, m, head, filled, l1=False, seed=0, rho0=(), nch=None, c1=1e-4, tol=1e-12, **_):
    """Random optimizer state of B models: fp32 vectors (exact zeros in x and a mixed L1 vector with a
    zero intercept column when ``l1``), a frozen-parameter mask, fp64 scalars, a consistent history."""
    gen = torch.Generator().manual_seed(seed)
    F, D = Fp1 - 1, K * Fp1
    st = SimpleNamespace(K=K, F=F, Fp1=Fp1, B=B, T=T, m=m, head=head, filled=filled, D=D, KP=kp_of(K),
                         nch=nch if nch is not None else qn_chunks_rule(D, B), c1=c1, tol=tol)
    st.x = (0.3 * torch.randn(B, D, generator=gen)).float()
    st.g = (0.5 * torch.randn(B, D, generator=gen)).float()
    st.l2 = (0.01 + 0.05 * torch.rand(B, D, generator=gen)).float()
    st.pmask = (torch.rand(B, D, generator=gen) > 0.1).float()
    st.inv_std = (0.5 + torch.rand(B, F, generator=gen)).float()
    st.l1 = None
    if l1:
        l1v = (0.4 * torch.rand(B, K, Fp1, generator=gen)).float()
        l1v[torch.rand(B, K, Fp1, generator=gen) < 0.2] = 0.0
        l1v[:, :, F] = 0.0  # the intercept is never penalized
        st.l1 = l1v.reshape(B, D).contiguous()
        st.x[torch.rand(B, D, generator=gen) < 0.25] = 0.0
    st.fobj = 1.0 + torch.rand(B, generator=gen, dtype=f64)
    st.step_scale = torch.ones(B, dtype=f32)
    st.active = torch.ones(B, dtype=i32)
    st.fails = torch.zeros(B, dtype=i32)
    st.iters = torch.full((B,), 3, dtype=i32)
    st.steep = torch.zeros(B, dtype=i32)
    return fill_history(st, gen, rho0)


def two_loop_vectors(st, pg, variant=None):
    """The two-loop recursion in vector space.  Returns (d_raw [B, D], A [B, D], gamma [B]) with
    ``d_raw = -r`` before any orthant restriction and ``A`` the sum of absolute terms of its chain.
    ``variant``: a deliberately wrong recursion (the discrimination check)."""
    m, head, filled = st.m, st.head, st.filled
    S, Y, rho = st.S.double(), st.Y.double(), st.rho.clone()
    order = ring(m, head, filled)
    newest = order[0] if order else None
    if variant == "head_off":
        order = ring(m, (head + 1) % m, filled)
        newest = order[0]
    elif variant == "reversed":
        order = order[::-1]
    elif variant == "rho_rejected":
        for j in order:
            rho[j] = torch.where(rho[j] == 0, 1.0 / _dot(S[j], Y[j]), rho[j])
    elif variant == "gamma_oldest":
        newest = order[-1]
    q = pg.clone()
    al = {}
    for j in order:
        a = torch.where(rho[j] != 0, rho[j] * _dot(S[j], q), torch.zeros_like(rho[j]))
        q = q - a[:, None] * Y[j]
        al[j] = a
    if filled == 0:
        gamma = 1.0 / _dot(pg, pg).sqrt().clamp_min(1e-12)
    else:
        yy, sy = _dot(Y[newest], Y[newest]), _dot(S[newest], Y[newest])
        gamma = torch.where((rho[newest] > 0) & (yy > 0), sy / yy.clamp_min(1e-300), torch.ones_like(yy))
    r = gamma[:, None] * q
    A = (gamma[:, None] * pg).abs()
    for j in reversed(order):
        w = torch.where(rho[j] != 0, al[j] - rho[j] * _dot(Y[j], r), torch.zeros_like(rho[j]))
        r = r + w[:, None] * S[j]
        A = A + (gamma * al[j])[:, None].abs() * Y[j].abs() + w[:, None].abs() * S[j].abs()
    return -r, A, gamma


def two_loop_gram(st, pg, variant=None):
    """The same direction from the Gram matrices and the P1 totals alone (coefficient space, fp64): the
    formulation the kernel uses, written out step by step.  ``variant="sy_transposed"`` reads SY
    transposed."""
    m, head, filled = st.m, st.head, st.filled
    SY = st.SY.transpose(1, 2) if variant == "sy_transposed" else st.SY
    YY, P1, rho = st.YY, st.P1, st.rho
    order = ring(m, head, filled)
    B = st.B
    al, w = {}, {}
    for n, i in enumerate(order):  # s_i.q with q = pg - sum_{l before i} al_l y_l
        sq = P1[:, i].clone()
        for l in order[:n]:
            sq = sq - al[l] * SY[:, i, l]
        al[i] = torch.where(rho[i] != 0, rho[i] * sq, torch.zeros(B, dtype=f64))
    if filled == 0:
        gamma = 1.0 / P1[:, 2 * QN_MAX_M].sqrt().clamp_min(1e-12)
    else:
        n0 = order[0]
        gamma = torch.where((rho[n0] > 0) & (YY[:, n0, n0] > 0), SY[:, n0, n0] / YY[:, n0, n0].clamp_min(1e-300),
                            torch.ones(B, dtype=f64))
    rev = order[::-1]
    for n, i in enumerate(rev):  # y_i.r with r = gamma q + sum_{l before i} w_l s_l
        yq = P1[:, QN_MAX_M + i].clone()
        for l in order:
            yq = yq - al[l] * YY[:, i, l]
        yr = gamma * yq
        for l in rev[:n]:
            yr = yr + w[l] * SY[:, l, i]
        w[i] = torch.where(rho[i] != 0, al[i] - rho[i] * yr, torch.zeros(B, dtype=f64))
    r = gamma[:, None] * pg
    S, Y = st.S.double(), st.Y.double()
    for j in order:
        r = r - (gamma * al[j])[:, None] * Y[j] + w[j][:, None] * S[j]
    return -r


def direction(st, variant=None, init=False, space="vectors"):
    """Phase 1 of every model: the direction, the T trial points, W_eff and the P2 sums, with bounds.
    ``space="gram"`` takes the direction from the state's Gram matrices and P1 totals (the chained test:
    the kernel's own inputs, whose agreement with the history is checked apart)."""
    B, D, K, Fp1, F, T, m, KP = st.B, st.D, st.K, st.Fp1, st.F, st.T, st.m, st.KP
    x, g = st.x.double(), st.g.double()
    l1 = None if st.l1 is None else st.l1.double()
    l1on = l1 is not None
    o = SimpleNamespace()
    steep = st.steep.bool()
    if init:
        T = 1
        pg = torch.zeros(B, D, dtype=f64)
        d_raw, A, gamma = torch.zeros(B, D, dtype=f64), torch.zeros(B, D, dtype=f64), torch.zeros(B, dtype=f64)
        step = torch.zeros(B, 1, dtype=f64)
    else:
        pg = pseudo_grad(x, g, l1)
        if variant == "sy_transposed" or space == "gram":
            d_raw, (_, A, gamma) = two_loop_gram(st, pg, variant), two_loop_vectors(st, pg)
        else:
            d_raw, A, gamma = two_loop_vectors(st, pg, variant)
        d_raw = torch.where(steep[:, None], -pg, d_raw)
        A = torch.where(steep[:, None], pg.abs(), A)
        step = st.step_scale.double()[:, None] * torch.pow(2.0, -torch.arange(T, dtype=f64))[None, :]
    o.T, o.pg, o.d_raw, o.A, o.gamma, o.step = T, pg, d_raw, A, gamma, step
    o.bound_d = 2 * (2 * m + 4) * U * A
    d = d_raw
    ex_d = torch.zeros(B, D, dtype=torch.bool)
    if l1on and not init:
        d = torch.where((d_raw * pg < 0) | steep[:, None], d_raw, torch.zeros_like(d_raw))
        ex_d = (pg != 0) & (d_raw.abs() <= o.bound_d) & ~steep[:, None]
    o.d, o.ex_d = d, ex_d
    xt_raw = x[:, None, :] + step[:, :, None] * d[:, None, :]                       # [B, T, D]
    o.bound_xt = step[:, :, None] * o.bound_d[:, None, :] + 2 * U * xt_raw.abs()
    xt = xt_raw
    ex_x = torch.zeros(B, T, D, dtype=torch.bool)
    if l1on and not init:
        xi = torch.where(x != 0, torch.sign(x), torch.sign(-pg))
        xt = torch.where(torch.sign(xt_raw) == xi[:, None, :], xt_raw, torch.zeros_like(xt_raw))
        ex_x = (d != 0)[:, None, :] & (xt_raw.abs() <= o.bound_xt)
    xt_dec = xt                                                                      # what the decrease sees
    act = st.active.bool()[:, None, None]
    xt = torch.where(act, xt, x[:, None, :].expand(B, T, D))
    o.bound_xt = torch.where(act, o.bound_xt, torch.zeros_like(o.bound_xt))
    o.ex = (ex_d[:, None, :] | ex_x) & act
    o.xtrial = xt
    # W_eff in the evaluator's [F + 1][KP] layout
    sc = torch.cat([st.inv_std.double(), torch.ones(B, 1, dtype=f64)], 1)           # [B, F + 1]
    wsc = st.pmask.double().view(B, K, Fp1) * sc[:, None, :]
    w = xt.view(B, T, K, Fp1) * wsc[:, None]
    o.weff = torch.zeros(B, T, Fp1, KP, dtype=f64)
    o.weff[..., :K] = w.transpose(2, 3)
    o.bound_w = torch.zeros_like(o.weff)
    o.bound_w[..., :K] = (wsc[:, None].abs() * o.bound_xt.view(B, T, K, Fp1) + 3 * U * w.abs()).transpose(2, 3)
    o.ex_w = torch.zeros(B, T, Fp1, KP, dtype=torch.bool)
    o.ex_w[..., :K] = o.ex.view(B, T, K, Fp1).transpose(2, 3)
    # the P2 sums, their sums of absolute terms, propagated and excluded-element bounds
    el1 = ((Fp1 + st.nch - 1) // st.nch) * K
    fac = 2 * (math.ceil(el1 / QN_BLOCK) + 2) * U
    hl2 = 0.5 * st.l2.double()
    P2 = torch.zeros(B, NP2, dtype=f64)
    bP2 = torch.zeros(B, NP2, dtype=f64)
    l1z = torch.zeros(B, D, dtype=f64) if l1 is None else l1
    X = x.abs()[:, None, :] + step[:, :, None] * d_raw.abs()[:, None, :]            # any outcome's magnitude
    exf = o.ex.double()
    for t in range(T):
        xn, bx = xt[:, t], o.bound_xt[:, t]
        P2[:, 3 * t] = (hl2 * xn * xn).sum(1)
        bP2[:, 3 * t] = fac * (hl2 * xn * xn).sum(1) + (hl2 * 2 * xn.abs() * bx).sum(1) + \
            (exf[:, t] * 2 * hl2 * X[:, t] ** 2).sum(1)
        P2[:, 3 * t + 1] = (l1z * xn.abs()).sum(1)
        bP2[:, 3 * t + 1] = fac * (l1z * xn.abs()).sum(1) + (l1z * bx).sum(1) + (exf[:, t] * 2 * l1z * X[:, t]).sum(1)
        if l1on and not init:
            dx = xt_dec[:, t] - x
            bxd = step[:, t, None] * o.bound_d + 2 * U * xt_raw[:, t].abs()
            P2[:, 3 * t + 2] = (pg * dx).sum(1)
            bP2[:, 3 * t + 2] = fac * (pg * dx).abs().sum(1) + (pg.abs() * bxd).sum(1) + \
                ((ex_d[:, None, :] | ex_x)[:, t].double() * 2 * pg.abs() * (X[:, t] + x.abs())).sum(1)
    P2[:, 3 * QN_MAX_TRIALS] = (pg * d).sum(1)
    bP2[:, 3 * QN_MAX_TRIALS] = fac * (pg * d).abs().sum(1) + (pg.abs() * o.bound_d).sum(1) + \
        (ex_d.double() * 2 * (pg * d_raw).abs()).sum(1)
    P2[:, 3 * QN_MAX_TRIALS + 1] = (pg * pg).sum(1)
    bP2[:, 3 * QN_MAX_TRIALS + 1] = fac * (pg * pg).sum(1)
    o.P2, o.bound_P2 = P2, bP2
    o.excluded_share = float(o.ex.double().mean()) if o.ex.numel() else 0.0
    return o


def pick_trial(st, P2, loss, init=False):
    """pick / reg / decr of every model from the P2 totals and the trial losses [B, T]."""
    B, T = st.B, (1 if init else st.T)
    pick = torch.full((B,), -1, dtype=torch.int64)
    reg = torch.zeros(B, st.T, dtype=f64)
    decr = torch.zeros(B, st.T, dtype=f64)
    for b in range(B):
        steep = bool(st.steep[b])
        dd = float(-P2[b, 3 * QN_MAX_TRIALS + 1] if steep else P2[b, 3 * QN_MAX_TRIALS])
        s0 = 0.0 if init else float(st.step_scale[b])
        for t in range(T):
            reg[b, t] = P2[b, 3 * t] + P2[b, 3 * t + 1]
            decr[b, t] = P2[b, 3 * t + 2] if st.l1 is not None else (s0 * 2.0 ** -t) * dd
        if init:
            pick[b] = 0
        elif int(st.active[b]):
            if dd >= 0:
                pick[b] = -1 if steep else -2
            else:
                for t in range(T):
                    Ft = float(loss[b, t]) + float(reg[b, t])
                    if math.isfinite(Ft) and Ft <= float(st.fobj[b]) + st.c1 * float(decr[b, t]):
                        pick[b] = t
                        break
    return pick, reg, decr


def update(st, xtrial, P2, loss, G, init=False):
    """Phase 2 of every model.  ``xtrial`` [B, T, D] and ``G`` [B, T, D] are the fp32 inputs the kernel
    reads, ``P2`` [B, NP2] the chunk-summed phase-1 totals, ``loss`` [B, T] the trial data losses.
    Returns the new state pieces and their bounds; quantities of models that take no step keep the old
    value (bound 0)."""
    B, D, m, h = st.B, st.D, st.m, st.head
    o = SimpleNamespace()
    loss = loss.view(B, -1).double()
    o.pick, o.reg, o.decr = pick_trial(st, P2, loss, init)
    take = o.pick >= 0
    ar, p = torch.arange(B), o.pick.clamp_min(0)
    x, g = st.x.double(), st.g.double()
    l1 = None if st.l1 is None else st.l1.double()
    l2 = st.l2.double()
    xn = xtrial.view(B, -1, D)[ar, p].double()
    gt = G.view(B, -1, D)[ar, p].double()
    gn = gt + l2 * xn
    pg = pseudo_grad(xn, gn, l1)
    s, y = xn - x, gn - g
    bg = 2 * U * (gt.abs() + (l2 * xn).abs())
    bs, by, bpg = U * s.abs(), U * y.abs() + bg, U * pg.abs() + bg
    tk = take[:, None]
    o.take = take
    o.x, o.g = torch.where(tk, xn, x), torch.where(tk, gn, g)
    o.bound_g = torch.where(tk, bg, torch.zeros_like(bg))
    el2 = (D + st.nch - 1) // st.nch
    fac = 2 * (math.ceil(el2 / QN_BLOCK) + 2) * U
    ssum = lambda a, b, ba, bb: (_dot(a, b), fac * _dot(a.abs(), b.abs()) + _dot(b.abs(), ba) + _dot(a.abs(), bb))  # noqa: E731
    zero = torch.zeros_like(x)
    o.xx, o.bound_xx = _dot(xn, xn), fac * _dot(xn, xn)
    o.pgpg, o.bound_pgpg = ssum(pg, pg, bpg, bpg)
    # the P1 totals of the NEXT direction (new pg, new pair in its slot); a model that takes no step keeps its own
    o.P1, o.bound_P1 = st.P1.clone(), torch.zeros(B, NP1, dtype=f64)
    P1n, bP1n = torch.zeros(B, NP1, dtype=f64), torch.zeros(B, NP1, dtype=f64)
    P1n[:, 2 * QN_MAX_M], bP1n[:, 2 * QN_MAX_M] = o.pgpg, o.bound_pgpg
    o.S_head, o.Y_head = st.S[h].double(), st.Y[h].double()
    o.bound_S, o.bound_Y = torch.zeros_like(bs), torch.zeros_like(by)
    o.rho_head = torch.zeros(B, dtype=f64)
    o.bound_rho = torch.zeros(B, dtype=f64)
    o.SY, o.YY = st.SY.clone(), st.YY.clone()
    o.bound_SY, o.bound_YY = torch.zeros_like(o.SY), torch.zeros_like(o.YY)
    o.fragile = torch.zeros(B, dtype=torch.bool)  # a decision within its error bound of its boundary
    if not init:
        o.S_head, o.Y_head = torch.where(tk, s, o.S_head), torch.where(tk, y, o.Y_head)
        o.bound_S, o.bound_Y = torch.where(tk, bs, zero), torch.where(tk, by, zero)
        sy, bsy = ssum(s, y, bs, by)
        ss, bss = ssum(s, s, bs, bs)
        yy, byy = ssum(y, y, by, by)
        o.sy, o.bound_sy = sy, bsy
        thr = 1e-10 * (ss.sqrt() * yy.sqrt()).clamp_min(1e-300)
        good = sy > thr
        o.fragile |= take & ((sy - thr).abs() <= bsy + 1e-10 * (bss + byy))
        o.rho_head = torch.where(take & good, 1.0 / sy, o.rho_head)
        o.bound_rho = torch.where(take & good, bsy / (sy.abs() * (sy.abs() - bsy).clamp_min(1e-300)), o.bound_rho)
        SYn, YYn, bSY, bYY = o.SY.clone(), o.YY.clone(), o.bound_SY.clone(), o.bound_YY.clone()
        SYn[:, h, h], bSY[:, h, h], YYn[:, h, h], bYY[:, h, h] = sy, bsy, yy, byy
        slots = ring(m, (h + 1) % m, min(st.filled + 1, m))  # the ring once this pair is in
        for j in range(m):
            Sj, Yj = (s, y) if j == h else (st.S[j].double(), st.Y[j].double())
            bsj, byj = (bs, by) if j == h else (zero, zero)
            P1n[:, j], bP1n[:, j] = ssum(Sj, pg, bsj, bpg)
            P1n[:, QN_MAX_M + j], bP1n[:, QN_MAX_M + j] = ssum(Yj, pg, byj, bpg)
            if j != h:
                SYn[:, h, j], bSY[:, h, j] = ssum(s, Yj, bs, zero)
                SYn[:, j, h], bSY[:, j, h] = ssum(Sj, y, zero, by)
                YYn[:, h, j], bYY[:, h, j] = ssum(y, Yj, by, zero)
                YYn[:, j, h], bYY[:, j, h] = YYn[:, h, j], bYY[:, h, j]
        o.slots = slots
        t3 = take[:, None, None]
        o.SY, o.YY = torch.where(t3, SYn, o.SY), torch.where(t3, YYn, o.YY)
        o.bound_SY, o.bound_YY = torch.where(t3, bSY, o.bound_SY), torch.where(t3, bYY, o.bound_YY)
    else:
        o.slots = []
    o.P1 = torch.where(tk, P1n, o.P1)
    o.bound_P1 = torch.where(tk, bP1n, o.bound_P1)
    # scalars and flags
    F0 = st.fobj.clone()
    Fn = loss[ar, p] + o.reg[ar, p]
    o.fobj = torch.where(take, Fn, F0)
    o.iters, o.fails, o.steep = st.iters.clone(), st.fails.clone(), st.steep.clone()
    o.step_scale, o.active = st.step_scale.clone(), st.active.clone()
    if not init:
        rel = (F0 - Fn).abs() / torch.maximum(torch.maximum(F0.abs(), Fn.abs()), torch.ones_like(F0))
        lhs, rhs = o.pgpg.sqrt(), st.tol * o.xx.sqrt().clamp_min(1.0)
        conv = (rel < st.tol) | (lhs <= rhs)
        blhs = o.bound_pgpg / (2 * lhs.clamp_min(1e-300))
        o.fragile |= take & (((lhs - rhs).abs() <= blhs + 1e-6 * rhs) | ((rel - st.tol).abs() <= 1e-9 * st.tol))
        failed = st.active.bool() & (o.pick == -1)
        o.iters = torch.where(take, st.iters + 1, st.iters)
        o.fails = torch.where(take, torch.zeros_like(st.fails), torch.where(failed, st.fails + 1, st.fails))
        o.steep = torch.where(take, torch.zeros_like(st.steep), torch.where(o.pick == -2, torch.ones_like(st.steep),
                                                                            st.steep))
        o.step_scale = torch.where(take, torch.ones_like(st.step_scale),
                                   torch.where(failed, st.step_scale / 16, st.step_scale))
        o.active = torch.where(take & conv, torch.zeros_like(st.active), st.active)
        o.active = torch.where(failed & (st.fails + 1 >= 2), torch.zeros_like(st.active), o.active)
    return o


def advance(st, up):
    """The state after an update (the oracle's own values rounded to the kernels' storage types), with head /
    filled moved on as the solver loop does."""
    n = SimpleNamespace(**vars(st))
    n.x, n.g = up.x.float(), up.g.float()
    n.S, n.Y, n.rho = st.S.clone(), st.Y.clone(), st.rho.clone()
    n.S[st.head], n.Y[st.head], n.rho[st.head] = up.S_head.float(), up.Y_head.float(), up.rho_head
    n.SY, n.YY, n.P1 = up.SY, up.YY, up.P1
    n.fobj, n.iters, n.fails, n.steep = up.fobj, up.iters, up.fails, up.steep
    n.step_scale, n.active = up.step_scale, up.active
    n.head, n.filled = (st.head + 1) % st.m, min(st.filled + 1, st.m)
    return n


def split_chunks(tot, nch, seed=0):
    """[B, N] totals -> [B, nch, N] chunk partials whose chunk-order fp64 sum is returned with them."""
    gen = torch.Generator().manual_seed(seed)
    B, N = tot.shape
    w = torch.rand(B, nch, 1, generator=gen, dtype=f64) + 0.1
    parts = tot[:, None, :] * (w / w.sum(1, keepdim=True))
    acc = torch.zeros(B, N, dtype=f64)
    for c in range(nch):
        acc = acc + parts[:, c]
    return parts.contiguous(), acc


def device_args(st, dev, hist_rows=2, init=0, fin_it=1):
    """The lbfgs_phase argument dict of bind.cpp's qn_args_from_dict and the device buffers behind it
    (the dict holds raw pointers: keep the buffers alive)."""
    B, T, D, m, nch, KP, Fp1 = st.B, st.T, st.D, st.m, st.nch, st.KP, st.Fp1
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    b = dict(x=st.x.to(dev), g=st.g.to(dev), fobj=st.fobj.to(dev), l2=st.l2.to(dev), pmask=st.pmask.to(dev),
             inv_std=st.inv_std.to(dev).contiguous(), S=st.S.to(dev), Y=st.Y.to(dev), rho=st.rho.to(dev),
             SY=st.SY.to(dev), YY=st.YY.to(dev), P1=torch.full((B, nch, NP1), 7.0, dtype=f64, device=dev),
             P2=z((B, nch, NP2), f64), P3=z((B, nch, NP3), f64), xtrial=z((B * T, D), f32),
             weff=z((B * T, Fp1, KP), f32), reg=z((B * T,), f64), decr=z((B * T,), f64), G=z((B * T, D), f32),
             loss=z((B * T,), f64), step_scale=st.step_scale.to(dev), active=st.active.to(dev),
             fails=st.fails.to(dev), iters=st.iters.to(dev), steep=st.steep.to(dev), pick=z((B,), i32),
             hist=z((hist_rows, B), f64), done=z((B,), i32))
    b["P1"][:, 0] = st.P1.to(dev)  # the totals live in chunk 0's row; the other rows are never read
    b["l1"] = None if st.l1 is None else st.l1.to(dev)
    b = {k: (v if v is None else v.contiguous()) for k, v in b.items()}
    a = dict(B=B, T=T, K=st.K, F=st.F, m=m, head=st.head, filled=st.filled, init=init, nch=nch, fin_it=fin_it, D=D,
             c1=float(st.c1), tol=float(st.tol))
    for k, v in b.items():
        a[k] = 0 if v is None else v.data_ptr()
    return a, b


def ratio(got, want, bound, mask=None):
    """Largest |got - want| / bound over the compared elements (0 / 0 counts as 0, x / 0 as inf)."""
    err = (got.double() - want.double()).abs()
    if mask is not None:
        err = torch.where(mask, torch.zeros_like(err), err)
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.double().expand_as(err))
    r = torch.where(torch.isnan(err), torch.full_like(r, float("inf")), r)
    return float(r.max())
