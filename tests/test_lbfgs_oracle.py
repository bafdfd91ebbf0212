"""Pins the fp64 oracle of the L-BFGS / OWL-QN kernels (tests/_lbfgs_util.py) on the CPU:

* chained from scratch it reproduces ``optim.lbfgs.minimize_trials`` iteration by iteration;
* on every input set of the GPU tests its vector-space direction equals an fp64 coefficient-space
  recursion on the same Gram matrices (the inputs are well conditioned for the kernel's formulation);
* on every input set a deliberately wrong recursion differs by >= 100x the bound the kernels are held to;
* the share of elements excluded for sitting on a sign decision stays under 0.5 %.
"""
import pytest
import torch

import _lbfgs_util as L
from _lbfgs_util import CASES, case_id

f64 = torch.float64


def _load_lbfgs():
    import har  # noqa: F401
    from har.optim import lbfgs

    return lbfgs


def _state(case, l1):
    return L.make_state(l1=l1, seed=11 + 2 * CASES.index(case) + int(l1), **case)


@pytest.fixture(scope="module")
def states():
    return {(c["name"], l1): _state(c, l1) for c in CASES for l1 in (False, True)}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_takes_the_path_it_was_chosen_for(case):
    D = case["K"] * case["Fp1"]
    nch = L.qn_chunks_rule(D, case["B"])
    path = L.dispatch_path(case["K"], case["Fp1"], case["B"], case["T"], case["m"], nch)
    assert nch == case["nch"]
    assert path["tile"] == case["tile"] and path["chunk"] == case["chunk"]
    assert path["fullm"] == (case["m"] == 10) and path["KP"] == (8 if case["K"] <= 8 else 16)
    if case["name"] == "refill":
        assert path["el1"] > 1536 and path["el2"] > 1536
    if case["name"] == "kp16_m4_full":
        # ragged phase-1 chunks (18, 18, 18, 17 columns)
        assert (case["Fp1"] + nch - 1) // nch * (nch - 1) < case["Fp1"] < (case["Fp1"] + nch - 1) // nch * nch


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_vector_and_coefficient_recursions_agree(states, case, l1):
    st = states[(case["name"], l1)]
    pg = L.pseudo_grad(st.x.double(), st.g.double(), None if st.l1 is None else st.l1.double())
    dv, A, _ = L.two_loop_vectors(st, pg)
    dc = L.two_loop_gram(st, pg)
    assert float(((dv - dc).abs() / A.clamp_min(1e-300)).max()) <= 1e-9


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_excluded_share_is_capped(states, case, l1):
    st = states[(case["name"], l1)]
    o = L.direction(st)
    assert o.excluded_share <= 0.005
    # the random histories give descent directions: phase 2's ordinary path is what the GPU cases run
    assert bool((o.P2[:, 12] + o.bound_P2[:, 12] < 0).all())


def _variants(case):
    usable = [j for j in L.ring(case["m"], case["head"], case["filled"]) if j not in case.get("rho0", ())]
    v = []
    if len(usable) >= 2:
        v += ["reversed", "sy_transposed"]
    if case["m"] >= 2 and case["filled"] >= 1:
        v.append("head_off")
    if case.get("rho0"):
        v.append("rho_rejected")
    if case["filled"] >= 2:
        v.append("gamma_oldest")
    return v


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_wrong_recursions_are_discriminated(states, case, l1):
    st = states[(case["name"], l1)]
    right = L.direction(st)
    vs = _variants(case)
    assert vs or case["filled"] == 0 or case["m"] == 1  # nothing to get wrong without two slots of history
    for v in vs:
        wrong = L.direction(st, variant=v)
        r = L.ratio(wrong.xtrial, right.xtrial, right.bound_xt, mask=right.ex | (right.bound_xt == 0))
        assert r >= 100.0, (v, r)


def test_every_wrong_variant_is_exercised():
    seen = {v for c in CASES for v in _variants(c)}
    assert seen == {"reversed", "sy_transposed", "head_off", "rho_rejected", "gamma_oldest"}


# ---------------------------------------------------------------------------------------------
# the oracle, chained from scratch, against minimize_trials on a convex quadratic
# ---------------------------------------------------------------------------------------------
def _quadratic(B, D, seed):
    gen = torch.Generator().manual_seed(seed)
    a = 0.2 + 4.8 * torch.rand(B, D, generator=gen, dtype=f64)
    c = torch.randn(B, D, generator=gen, dtype=f64)

    def evaluate(xt):
        rep = xt.shape[0] // B
        aa, cc = a.repeat_interleave(rep, 0), c.repeat_interleave(rep, 0)
        r = xt.double() - cc
        return 0.5 * (aa * r * r).sum(1), (aa * r).float()

    return evaluate


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_oracle_chain_equals_minimize_trials(l1):
    lbfgs = _load_lbfgs()
    B, K, Fp1, T, m = 2, 4, 30, 4, 3
    D = K * Fp1
    st = L.make_state(K, Fp1, B, T, m, 0, 0, l1=l1, seed=5, tol=1e-12)
    st.S.zero_()
    st.Y.zero_()
    st.iters.zero_()
    evaluate = _quadratic(B, D, 3)
    x0 = st.x.clone()
    # init: the objective and gradient at x0
    o = L.direction(st, init=True)
    loss, G = evaluate(o.xtrial.reshape(B, D).float())
    st.g.zero_()
    up = L.update(st, o.xtrial.float(), o.P2, loss.view(B, 1), G.view(B, 1, D), init=True)
    st.x, st.g, st.fobj, st.P1 = up.x.float(), up.g.float(), up.fobj, up.P1
    n_iter = 3 * m + 2
    prev_x = None
    for n in range(1, n_iter + 1):
        ref = lbfgs.minimize_trials(evaluate, x0, st.l2, st.l1, max_iter=n, m=m, tol=1e-12, trials=T)
        o = L.direction(st)
        xt = o.xtrial.float()
        loss, G = evaluate(xt.reshape(B * T, D))
        up = L.update(st, xt, o.P2, loss.view(B, T), G.view(B, T, D))
        assert bool(up.take.all()), (n, up.pick)
        head = st.head
        st = L.advance(st, up)
        torch.testing.assert_close(st.x, ref.x, rtol=1e-4, atol=2e-6)
        torch.testing.assert_close(st.fobj, ref.f, rtol=1e-5, atol=1e-7)
        assert [float(h[n]) for h in ref.history_per_model] == pytest.approx(st.fobj.tolist(), rel=1e-5, abs=1e-7)
        # S / Y / rho of the pair just stored, from minimize_trials' own iterates
        if prev_x is not None or n == 1:
            xa = (x0 if n == 1 else prev_x).double()
            grad = lambda x: evaluate(x.float())[1].double() + st.l2.double() * x  # noqa: E731
            s_ref, y_ref = ref.x.double() - xa, grad(ref.x.double()) - grad(xa)
            torch.testing.assert_close(st.S[head].double(), s_ref, rtol=1e-3, atol=2e-6)
            torch.testing.assert_close(st.Y[head].double(), y_ref, rtol=1e-3, atol=1e-5)
            sy = (s_ref * y_ref).sum(1)
            if bool((sy.abs() > 1e-6).all()):
                torch.testing.assert_close(st.rho[head], 1.0 / sy, rtol=2e-3, atol=0)
        prev_x = ref.x.clone()
        # the Gram matrices and P1 totals the chain carries are the ones of its own history
        SY, YY, P1 = L.gram_from_history(st)
        for name, a, b in (("SY", st.SY, SY), ("YY", st.YY, YY), ("P1", st.P1, P1)):
            assert float((a - b).abs().max()) <= 1e-5 * max(1e-12, float(b.abs().max())), (n, name)
    assert st.filled == m and n_iter > 3 * m
