"""The optimizer half of csrc/kernels/logreg_qn.hip, phase by phase, against the fp64 oracle of
tests/_lbfgs_util.py (pinned on the CPU by tests/test_lbfgs_oracle.py):

* phase 1 (``qn_direction_kernel``): ``xtrial``, ``weff`` and the chunk-summed ``P2``;
* phase 2 (``qn_update_kernel`` + ``qn_finalize``): everything an update leaves behind, and each control
  branch of the pick and of the finalization;
* a chained run of both phases on a device quadratic: the Gram matrices, ``rho`` and the P1 totals the
  kernels maintain are those of the history they hold, at every iteration, over three wraps of the ring;
* history lengths other than 10 through ``DeviceLogregSolver``'s entry points.

Bounds (u = 2^-24) are the derived ones of _lbfgs_util; each test prints its largest error / bound ratio.
"""
import pytest
import torch

import _lbfgs_util as L
from _lbfgs_util import CASES, case_id

pytestmark = pytest.mark.gpu
f64 = torch.float64
EPS = 2.0 ** -52


def _kern():
    from har.ops import _native

    return _native.kernels(), _native.stream_ptr()


def _launch(phase, args, KP):
    mod, s = _kern()
    mod.lbfgs_phase(phase, args, KP, s)
    torch.cuda.synchronize()


def _report(name, ratios):
    worst = max(ratios.items(), key=lambda kv: kv[1])
    print(f"\nQN_RATIO {name}: max {worst[1]:.3f} ({worst[0]}) " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (name, bad)


def _check_path(case, st):
    """The shape takes the path it was chosen for (a mismatch fails, never skips)."""
    mod, _ = _kern()
    assert mod.qn_chunks(st.D, st.B) == case["nch"] == st.nch
    path = L.dispatch_path(st.K, st.Fp1, st.B, st.T, st.m, st.nch)
    assert path["tile"] == case["tile"] and path["chunk"] == case["chunk"] and path["KP"] == st.KP
    assert path["fullm"] == (st.m == L.QN_MAX_M)
    return path


def _phase1_ratios(st, o, b):
    B, T, D = st.B, o.T, st.D
    xt = b["xtrial"].cpu().view(B, st.T, D)[:, :T]
    we = b["weff"].cpu().view(B, st.T, st.Fp1, st.KP)[:, :T]
    assert bool((we[..., st.K:] == 0).all()), "padded classes of W_eff are not exactly zero"
    sums = torch.zeros(B, L.NP2, dtype=f64)
    P2 = b["P2"].cpu()
    for c in range(st.nch):
        sums = sums + P2[:, c]
    return {"xtrial": L.ratio(xt, o.xtrial, o.bound_xt, o.ex), "weff": L.ratio(we, o.weff, o.bound_w, o.ex_w),
            "P2": L.ratio(sums, o.P2, o.bound_P2 + 8 * EPS * o.P2.abs())}, sums


def _update_inputs(st, o, want, seed, delta=0.05, neg_curv=()):
    """Device-side inputs of phase 2 built from the oracle's phase 1: the trial points (rounded to fp32), the
    P2 totals split over the chunks, trial gradients with y = A s (A > 0; < 0 for ``neg_curv`` models) and
    trial losses that make trial ``want[b]`` the first to pass Armijo, by a margin of ``delta`` relative
    (want[b] = T: none passes)."""
    gen = torch.Generator().manual_seed(seed)
    B, T, D = st.B, st.T, st.D
    xt = o.xtrial.float()
    parts, P2 = L.split_chunks(o.P2, st.nch, seed)
    A = 0.5 + 1.5 * torch.rand(B, 1, D, generator=gen, dtype=f64)
    for b in neg_curv:
        A[b] = -A[b]
    x, g, l2 = st.x.double()[:, None], st.g.double()[:, None], st.l2.double()[:, None]
    G = (g + A * (xt.double() - x) - l2 * xt.double()).float()
    _, reg, decr = L.pick_trial(st, P2, torch.zeros(B, T, dtype=f64))
    loss = torch.zeros(B, T, dtype=f64)
    dl = delta if torch.is_tensor(delta) else torch.full((B,), delta, dtype=f64)
    for b in range(B):
        for t in range(T):
            edge = st.fobj[b] + st.c1 * decr[b, t]
            mag = dl[b] * max(1.0, abs(float(edge)), abs(float(reg[b, t])))
            loss[b, t] = edge - reg[b, t] + (mag if t < int(want[b]) else -mag)
    return xt, parts, P2, G, loss


def _phase2_ratios(st, up, b, before, fin_it):
    """Everything phase 2 leaves behind against the oracle's update ``up``."""
    B, m, h = st.B, st.m, st.head
    c = {k: v.cpu() for k, v in b.items() if v is not None}
    assert torch.equal(c["pick"].long(), up.pick), (c["pick"], up.pick)
    assert int(c["done"].abs().max()) == 0
    for k in ("iters", "fails", "steep", "active"):
        assert torch.equal(c[k], getattr(up, k)), (k, c[k], getattr(up, k))
    assert torch.equal(c["step_scale"], up.step_scale)
    assert torch.equal(c["x"], up.x.float()), "x is not the picked trial point / moved without a step"
    r = {}
    T = up.reg.shape[1]
    tiny = 8 * EPS
    r["reg"] = L.ratio(c["reg"].view(B, -1)[:, :T], up.reg, tiny * up.reg.abs() + 1e-300)
    r["decr"] = L.ratio(c["decr"].view(B, -1)[:, :T], up.decr, tiny * up.decr.abs() + 1e-300)
    r["fobj"] = L.ratio(c["fobj"], up.fobj, tiny * (up.fobj.abs() + up.reg.abs().max(1).values) + 1e-300)
    assert torch.equal(c["hist"][fin_it], c["fobj"])
    r["g"] = L.ratio(c["g"], up.g, up.bound_g + 1e-300)
    r["S"] = L.ratio(c["S"][h], up.S_head, up.bound_S + 1e-300)
    r["Y"] = L.ratio(c["Y"][h], up.Y_head, up.bound_Y + 1e-300)
    others = [j for j in range(m) if j != h]
    assert torch.equal(c["S"][others], before["S"][others]) and torch.equal(c["Y"][others], before["Y"][others])
    assert torch.equal(c["rho"][others], before["rho"][others])
    r["rho"] = L.ratio(c["rho"][h], up.rho_head, up.bound_rho + tiny * up.rho_head.abs() + 1e-300)
    sl = up.slots
    if sl:
        ix = torch.tensor(sl)
        sub = lambda a: a[:, ix][:, :, ix]  # noqa: E731
        r["SY"] = L.ratio(sub(c["SY"]), sub(up.SY), sub(up.bound_SY) + tiny * sub(up.SY).abs() + 1e-300)
        r["YY"] = L.ratio(sub(c["YY"]), sub(up.YY), sub(up.bound_YY) + tiny * sub(up.YY).abs() + 1e-300)
        # a model that took no step keeps every Gram entry bit for bit
        keep = ~up.take
        assert torch.equal(c["SY"][keep], before["SY"][keep]) and torch.equal(c["YY"][keep], before["YY"][keep])
    pi = torch.tensor(sl + [L.QN_MAX_M + j for j in sl] + [2 * L.QN_MAX_M])
    r["P1"] = L.ratio(c["P1"][:, 0][:, pi], up.P1[:, pi], up.bound_P1[:, pi] + tiny * up.P1[:, pi].abs() + 1e-300)
    return r


# ---------------------------------------------------------------------------------------------
# single steps on the shape table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_single_step_matches_oracle(cuda, case, l1):
    st = L.make_state(l1=l1, seed=11 + 2 * CASES.index(case) + int(l1), **case)
    path = _check_path(case, st)
    o = L.direction(st)
    a, b = L.device_args(st, cuda)
    if path["tile"]:
        b["weff"].fill_(float("nan"))  # the tile path writes every class of every row itself
    _launch(1, a, st.KP)
    r1, _ = _phase1_ratios(st, o, b)
    # phase 2 on the oracle's own trial points: model b's first acceptable trial is b mod T
    want = [bb % st.T for bb in range(st.B)]
    xt, parts, P2, G, loss = _update_inputs(st, o, want, seed=case["K"])
    up = L.update(st, xt, P2, loss, G)
    assert not bool(up.fragile.any()) and up.pick.tolist() == want
    b["xtrial"].copy_(xt.view(-1, st.D))
    b["P2"].copy_(parts)
    b["G"].copy_(G.view(-1, st.D))
    b["loss"].copy_(loss.view(-1))
    before = {k: b[k].cpu().clone() for k in ("S", "Y", "rho", "SY", "YY")}
    _launch(2, a, st.KP)
    r2 = _phase2_ratios(st, up, b, before, 1)
    _report(f"{case['name']}/{'l1' if l1 else 'l2'}", {**r1, **r2})


BRANCH_SHAPES = [dict(K=3, Fp1=17, T=4, m=10, head=4, filled=4), dict(K=6, Fp1=44, T=4, m=3, head=0, filled=3)]
#        0..3 first acceptable trial t; 4 none (fails 0); 5 none (fails 1: freezes); 6 non-descent; 7 non-descent while
#        steep; 8 inactive; 9 / 10 inf / nan at t = 0; 11 s.y <= 0; 12 rel < tol; 13 |pg| <= tol max(|x|, 1)
NB = 14


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("shape", BRANCH_SHAPES, ids=["m10", "m3"])
def test_update_branches(cuda, shape, l1):
    st = L.make_state(B=NB, l1=l1, seed=40 + shape["m"] + int(l1), tol=1e-2, **shape)
    st.fails[5] = 1
    st.steep[7] = 1
    st.active[8] = 0
    st.step_scale[4] = 0.25
    o = L.direction(st)
    o.P2[6, 12] = 0.3          # pg.d >= 0
    o.P2[7, 13] = 0.0          # steepest descent with a zero pseudo-gradient: dd = -pg.pg >= 0
    T = st.T
    want = [0, 1, 2, 3, T, T, 0, 0, 0, 1, 1, 1, 2, 0]
    delta = torch.full((NB,), 0.05, dtype=f64)
    delta[12] = 1e-5           # accepted with |dF| / max(|F|, 1) far below tol = 1e-2, Armijo margin still 1e-5
    xt, parts, P2, G, loss = _update_inputs(st, o, want, seed=3, delta=delta, neg_curv=(11,))
    loss[9, 0], loss[10, 0] = float("inf"), float("nan")
    # model 13: the new pseudo-gradient vanishes (g_new = -l1 sgn(x_new))
    xn = xt[13, 0].double()
    l1d = torch.zeros_like(xn) if st.l1 is None else st.l1[13].double()
    G[13, 0] = (-l1d * torch.sign(xn) - st.l2[13].double() * xn).float()
    up = L.update(st, xt, P2, loss, G)
    assert not bool(up.fragile.any())
    assert up.pick.tolist() == [0, 1, 2, 3, -1, -1, -2, -1, -1, 1, 1, 1, 2, 0]
    # the oracle takes each branch it was built for
    assert up.fails.tolist()[4:6] == [1, 2] and up.active.tolist()[4:6] == [1, 0]
    assert float(up.step_scale[4]) == 0.25 / 16 and float(up.step_scale[5]) == 1.0 / 16
    assert int(up.steep[6]) == 1 and int(up.steep[7]) == 1 and int(up.fails[7]) == 1
    assert int(up.active[8]) == 0 and float(up.fobj[8]) == float(st.fobj[8])
    assert float(up.rho_head[11]) == 0.0 and float(up.sy[11]) < 0 and bool(up.take[11])
    assert up.active.tolist()[12:] == [0, 0] and up.active.tolist()[:4] == [1, 1, 1, 1]
    a, b = L.device_args(st, cuda)
    b["xtrial"].copy_(xt.view(-1, st.D))
    b["P2"].copy_(parts)
    b["G"].copy_(G.view(-1, st.D))
    b["loss"].copy_(loss.view(-1))
    before = {k: b[k].cpu().clone() for k in ("S", "Y", "rho", "SY", "YY", "g", "P1")}
    _launch(2, a, st.KP)
    r = _phase2_ratios(st, up, b, before, 1)
    stay = [4, 5, 6, 7, 8]  # no step: x (above), g, the pair in slot head and the P1 totals are untouched
    assert torch.equal(b["g"].cpu()[stay], before["g"][stay])
    assert torch.equal(b["S"].cpu()[st.head][stay], before["S"][st.head][stay])
    assert torch.equal(b["P1"].cpu()[stay], before["P1"][stay])
    assert b["rho"].cpu()[st.head][stay].tolist() == [0.0] * 5
    _report(f"branches/m{st.m}/{'l1' if l1 else 'l2'}", r)


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("shape", BRANCH_SHAPES, ids=["m10", "m3"])
def test_init_phases(cuda, shape, l1):
    """init = 1: trial 0 is x itself, fobj = loss + reg, hist[0], the P1 totals of the first direction, and
    no history, counter or flag is written."""
    st = L.make_state(B=3, l1=l1, seed=60 + shape["m"] + int(l1), **shape)
    st.g.zero_()
    o = L.direction(st, init=True)
    a, b = L.device_args(st, cuda, init=1, fin_it=0)
    _launch(1, a, st.KP)
    assert torch.equal(b["xtrial"].cpu().view(st.B, st.T, st.D)[:, 0], st.x)
    r1, sums = _phase1_ratios(st, o, b)
    gen = torch.Generator().manual_seed(1)
    G = torch.zeros(st.B, st.T, st.D)
    G[:, 0] = torch.randn(st.B, st.D, generator=gen)
    loss = torch.rand(st.B, st.T, generator=gen, dtype=f64)
    up = L.update(st, b["xtrial"].cpu().view(st.B, st.T, st.D), sums, loss, G, init=True)
    b["G"].copy_(G.view(-1, st.D))
    b["loss"].copy_(loss.view(-1))
    keep = ("S", "Y", "rho", "SY", "YY", "iters", "fails", "steep", "active", "step_scale")
    before = {k: b[k].cpu().clone() for k in keep}
    _launch(2, a, st.KP)
    c = {k: v.cpu() for k, v in b.items() if v is not None}
    for k in keep:
        assert torch.equal(c[k], before[k]), k
    assert c["pick"].tolist() == [0] * st.B and int(c["done"].abs().max()) == 0
    assert torch.equal(c["x"], st.x) and torch.equal(c["hist"][0], c["fobj"])
    tiny = 8 * EPS
    r = dict(r1)
    r["fobj"] = L.ratio(c["fobj"], up.fobj, tiny * up.fobj.abs())
    r["g"] = L.ratio(c["g"], up.g, up.bound_g + 1e-300)
    r["P1"] = L.ratio(c["P1"][:, 0], up.P1, up.bound_P1 + 1e-300)  # s_j.pg = y_j.pg = 0, pg.pg
    _report(f"init/m{st.m}/{'l1' if l1 else 'l2'}", r)


# ---------------------------------------------------------------------------------------------
# both phases chained on a device quadratic: the state the kernels maintain across iterations
# ---------------------------------------------------------------------------------------------
def _pull(st, b, head, filled):
    n = L.SimpleNamespace(**vars(st))
    for k in ("x", "g", "S", "Y", "rho", "SY", "YY", "fobj", "step_scale", "active", "fails", "iters", "steep"):
        setattr(n, k, b[k].cpu().clone())
    n.P1 = b["P1"].cpu()[:, 0].clone()
    n.head, n.filled = head, filled
    return n


def _gram_invariant(st):
    """SY / YY / rho / P1 totals of the device state against fp64 dots of the device's own S, Y, x, g."""
    SY, YY, P1 = L.gram_from_history(st)
    ab = L.SimpleNamespace(**vars(st))
    ab.S, ab.Y = st.S.abs(), st.Y.abs()
    aSY, aYY, _ = L.gram_from_history(ab)
    pg = L.pseudo_grad(st.x.double(), st.g.double(), None if st.l1 is None else st.l1.double()).abs()
    fac = 2 * (-(-((st.D + st.nch - 1) // st.nch) // L.QN_BLOCK) + 2) * L.U
    sl = L.ring(st.m, st.head, st.filled)
    ix = torch.tensor(sl)
    sub = lambda a: a[:, ix][:, :, ix]  # noqa: E731
    r = {"SY": L.ratio(sub(st.SY), sub(SY), fac * sub(aSY) + 1e-300),
         "YY": L.ratio(sub(st.YY), sub(YY), fac * sub(aYY) + 1e-300)}
    aP1 = torch.stack([(ab.S[j].double() * pg).sum(1) for j in sl] + [(ab.Y[j].double() * pg).sum(1) for j in sl]
                      + [(pg * pg).sum(1)], 1)
    pi = torch.tensor(sl + [L.QN_MAX_M + j for j in sl] + [2 * L.QN_MAX_M])
    r["P1"] = L.ratio(st.P1[:, pi], P1[:, pi], fac * aP1 + 1e-300)
    # rho is 1 / SY[j][j] of the device's own Gram entry, or 0 for a rejected pair
    for j in sl:
        dj = st.SY[:, j, j]
        ok = (st.rho[j] == 0) | ((st.rho[j] * dj - 1).abs() <= 8 * EPS)
        assert bool(ok.all()), ("rho", j)
    return r


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("m", [10, 4])
def test_chained_state_stays_consistent(cuda, m, l1):
    K, Fp1, B, T = 6, 44, 3, 4
    st = L.make_state(K, Fp1, B, T, m, 0, 0, l1=l1, seed=70 + m + int(l1))
    D, n_iter = st.D, 3 * m + 2
    st.S.zero_()
    st.Y.zero_()
    st.g.zero_()
    st.iters.zero_()
    gen = torch.Generator().manual_seed(9)
    qa = torch.exp(torch.log(torch.tensor(0.05)) + torch.rand(B, D, generator=gen) * torch.log(torch.tensor(400.0))).to(cuda)
    qc = torch.randn(B, D, generator=gen).to(cuda)

    def fill(b, n):  # the data loss and gradient of the first n trials of every model, on the device
        xt = b["xtrial"].view(B, T, D)[:, :n]
        r = xt - qc[:, None]
        b["G"].view(B, T, D)[:, :n] = qa[:, None] * r
        b["loss"].view(B, T)[:, :n] = 0.5 * (qa[:, None].double() * r.double() ** 2).sum(2)

    a, b = L.device_args(st, cuda, hist_rows=n_iter + 1, init=1, fin_it=0)
    _launch(1, a, st.KP)
    fill(b, 1)
    _launch(2, a, st.KP)
    a["init"] = 0
    head = filled = 0
    worst = {}
    taken = torch.zeros(B, dtype=torch.int64)
    for it in range(n_iter):
        cur = _pull(st, b, head, filled)
        a.update(head=head, filled=filled, fin_it=it + 1)
        o = L.direction(cur, space="gram")
        _launch(1, a, st.KP)
        r, sums = _phase1_ratios(cur, o, b)
        fill(b, T)
        up = L.update(cur, b["xtrial"].cpu().view(B, T, D), sums, b["loss"].cpu().view(B, T), b["G"].cpu().view(B, T, D))
        assert not bool(up.fragile.any()), it
        before = {k: b[k].cpu().clone() for k in ("S", "Y", "rho", "SY", "YY")}
        _launch(2, a, st.KP)
        r.update(_phase2_ratios(cur, up, b, before, it + 1))
        taken += up.take.long()
        head, filled = (head + 1) % m, min(filled + 1, m)
        for k, v in _gram_invariant(_pull(st, b, head, filled)).items():
            r["inv_" + k] = v
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert all(v <= 1.0 for v in r.values()), (it, r)
    # some model overwrote every slot of its ring at least twice with accepted pairs (a model that reaches
    # the fp32 floor of the quadratic early is rejected and frozen from then on, as designed)
    assert int(taken.max()) > 2 * m, taken
    _report(f"chained/m{m}/{'l1' if l1 else 'l2'}", worst)


# ---------------------------------------------------------------------------------------------
# a history length other than 10 through the solver entry points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.0, 0.4])
def test_solver_with_short_history(cuda, monkeypatch, alpha):
    from har.ops import logreg as LG
    from har.optim import lbfgs
    from test_gpu_logreg import _hybrid_problem

    mod, _ = _kern()
    X, y, hm = _hybrid_problem(cuda, N=1500)
    N, F = X.shape
    K, B, T, m, iters = 6, 2, 4, 4, 14
    D = K * (F + 1)
    g = torch.Generator().manual_seed(4)
    rw = (torch.rand(B, N, generator=g) > 0.2).float().to(cuda)
    inv_std = (torch.rand(B, F, generator=g) + 0.5).to(cuda)
    pmask = torch.ones(B, K, F + 1, device=cuda)
    inv_wsum = 1.0 / rw.sum(1)
    notb = torch.ones(F + 1, device=cuda)
    notb[F] = 0
    reg = torch.tensor([0.05, 0.02], device=cuda)
    l2v = (reg[:, None, None] * (1 - alpha) * pmask * notb).reshape(B, D).contiguous()
    l1v = (reg[:, None, None] * alpha * pmask * notb).reshape(B, D).contiguous() if alpha > 0 else None
    x0 = torch.zeros(B, D, device=cuda)

    def solve(native):
        monkeypatch.setenv("HAR_LR_NATIVE_SOLVE", native)
        design = LG.LogregDesign(hm, y.to(cuda), rw, K)
        s = LG.DeviceLogregSolver(design, B, T, m, inv_std, pmask, inv_wsum, l2v, l1v, iters, 1e-6)
        x, f, _ = s.solve(x0)
        torch.cuda.synchronize()
        return x.clone(), f.clone(), s.hist.clone(), design

    xa, fa, ha, design = solve("1")
    xb, fb, hb, _ = solve("0")
    assert torch.equal(xa, xb) and torch.equal(fa, fb) and torch.equal(ha, hb)

    ref_design = LG.LogregDesign(hm, y.to(cuda), rw.double(), K)

    def evaluate(xt):
        loss, G = ref_design.eval_torch(xt.double().view(-1, K, F + 1), T if xt.shape[0] != B else 1, inv_std.double(),
                                        pmask.double(), inv_wsum.double())
        return loss, G.float()

    ref = lbfgs.minimize_trials(evaluate, x0, l2v, l1v, max_iter=iters, m=m, tol=1e-6, trials=T)
    for bb in range(B):
        assert abs(float(ref.f[bb]) - float(fa[bb])) <= 2e-4 * max(1.0, abs(float(ref.f[bb])))
    assert float(fa.max()) < float(ha[0].min())  # the fit moved
