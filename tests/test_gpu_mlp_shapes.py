"""The MLP kernels away from the 6-class, 43-feature shape: class-count and input-width edges, ragged
and smallest batches, large logits, ties, the serving kernels' output bounds, and the padding through
the optimizer — every native path (step, fused_fwd, small, gemm) against ONE fp64 oracle that rounds
to bf16 where the kernels do.  The oracle itself is checked against torch.autograd on the CPU."""
import math

import pytest
import torch

GRAD_TOL = 1e-2                       # the criterion of test_mlp_step_matches_torch
LOGIT_RTOL, LOGIT_ATOL = 1e-4, 1e-3   # the tolerances of test_softmax_ce_head
AMBIGUOUS_CAP = 0.02                  # share of rows whose argmax the logits tolerance leaves open


def _bf_round(x):
    """fp32 -> bf16 -> back (the kernels compute in fp32 and store bf16), kept in the input dtype."""
    return x.float().to(torch.bfloat16).to(x.dtype)


def _first_argmax(z):
    """Smallest index at the row maximum (the kernels' tie rule)."""
    C = z.shape[1]
    idx = torch.arange(C, device=z.device).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values


def mlp_oracle(P, layout, Xb, y, scale, round_bf16=True):
    """fp64 forward + backprop of the network a ``FlatLayout`` describes (any number of hidden layers,
    any C <= 32, any in_pad) from the flat parameters ``P``; with ``round_bf16`` the weight copies,
    activations, dlogits and data gradients are rounded to bf16 where the kernels round them.
    Returns logits [B, C], the summed CE loss, the correct count (argmax = first index at the
    maximum) and the gradient of every segment (full padded shapes; loss = sum CE * scale)."""
    L = layout
    C, nh = L.num_classes, len(L.hidden)
    rb = _bf_round if round_bf16 else (lambda t: t)
    P = P.detach().double()
    y = y.long()
    W = {s.name: L.view(P, s.name) for s in L.segments}
    Wb = {k: rb(v) for k, v in W.items() if k.startswith("W")}
    acts = [Xb.double()]
    for i in range(nh):
        acts.append(rb((acts[-1] @ Wb[f"W{i}"].T + W[f"b{i}"]).clamp_min(0)))
    last = acts[-1]
    z = last @ Wb["Wout"][:C].T + W["bout"][:C]
    rows = torch.arange(z.shape[0], device=z.device)
    loss = (torch.logsumexp(z, 1) - z[rows, y]).sum()
    p = torch.softmax(z, 1)
    p[rows, y] -= 1
    dl = rb(p * scale)
    grads = {"Wout": torch.zeros_like(W["Wout"]), "bout": torch.zeros_like(W["bout"])}
    grads["Wout"][:C] = dl.T @ last
    grads["bout"][:C] = dl.sum(0)
    d = rb((dl @ Wb["Wout"][:C]) * (last > 0))
    for i in reversed(range(nh)):
        grads[f"W{i}"], grads[f"b{i}"] = d.T @ acts[i], d.sum(0)
        if i > 0:
            d = rb((d @ Wb[f"W{i}"]) * (acts[i] > 0))
    correct = int((_first_argmax(z) == y).sum())
    return {"logits": z, "loss": float(loss), "correct": correct, "grads": grads}


def _inputs(layers, B, seed, labels="rand"):
    """Seeded CPU batch: padded bf16 rows [B, in_pad] (what the kernels read) and int64 labels."""
    F, C = layers[0], layers[-1]
    in_pad = (F + 31) // 32 * 32
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, F, generator=g)
    Xb = torch.zeros(B, in_pad, dtype=torch.bfloat16)
    Xb[:, :F] = X.to(torch.bfloat16)
    if labels == "rand":
        y = torch.randint(0, C, (B,), generator=g)
    else:  # the real class next to the padding
        y = torch.full((B,), C - 1, dtype=torch.int64)
    return Xb, y


def _ambiguous(z):
    """Rows whose two largest logits lie closer than the logits tolerance (and that tolerance)."""
    if z.shape[1] < 2:
        return torch.zeros(z.shape[0], dtype=torch.bool), torch.zeros(z.shape[0], dtype=z.dtype)
    top = z.topk(2, dim=1).values
    tol = LOGIT_ATOL + LOGIT_RTOL * top[:, 0].abs()
    return (top[:, 0] - top[:, 1]) < tol, tol


# ------------------------------------------------------------------------------------------ cases
def _grad_cases():
    cases = []
    for B in (64, 192):  # the smallest step batch and three 64-row tiles
        cases += [("step", [43, 256, 256, C], B) for C in (1, 2, 15, 16)]
        cases += [("step", [F, 256, 256, 6], B) for F in (1, 32, 33, 64)]
    # fused forward: the smallest batch (one 16-row tile), three tiles, and H = 256 off the step's batches
    cases += [("fused_fwd", [43, 128, 128, 1], 16), ("fused_fwd", [43, 128, 128, 2], 48),
              ("fused_fwd", [43, 256, 256, 15], 48), ("fused_fwd", [43, 128, 128, 16], 16),
              ("fused_fwd", [1, 128, 128, 6], 48), ("fused_fwd", [32, 256, 256, 6], 48),
              ("fused_fwd", [33, 128, 128, 6], 16), ("fused_fwd", [64, 128, 128, 6], 48)]
    cases += [("small", [F, H, H, C], 32) for H in (128, 256) for C in (1, 16) for F in (32, 33)]
    cases += [("gemm", [43, 64, 96, C], 77) for C in (1, 16, 17, 31, 32)]
    cases += [("gemm", [65, 64, 64, 6], 77)]
    cases += [("gemm", [43, 256, 256, 6], B) for B in (1, 7, 200, 3793)]
    # what the generic path exists for: one hidden layer (no dgrad GEMM), three (dgrad chained through both
    # dbuf halves), and last widths whose fused head takes 105 KB / the first 65 KB (past 64 KB) of LDS
    cases += [("gemm", [43, 96, 6], 77), ("gemm", [43, 64, 96, 64, 6], 77), ("gemm", [43, 64, 512, 6], 65),
              ("gemm", [43, 320, 320, 17], 65)]
    return [c + ("rand",) for c in cases]


LABEL_EDGE_CASES = [("step", [43, 256, 256, 15], 64, "last"), ("fused_fwd", [43, 128, 128, 15], 48, "last"),
                    ("small", [33, 128, 128, 15], 32, "last"), ("gemm", [43, 64, 96, 17], 77, "last")]
GRAD_CASES = _grad_cases() + LABEL_EDGE_CASES
ENGINE_SEED, DATA_SEED = 3, 9


def _case_id(c):
    path, layers, B, labels = c
    return f"{path}-{'x'.join(map(str, layers))}-B{B}-{labels}"


PATH_ENV = {
    "step": {"HAR_MLP_FUSED": "1", "HAR_MLP_STEP": "1", "HAR_MLP_SMALL": "0"},
    "fused_fwd": {"HAR_MLP_FUSED": "1", "HAR_MLP_STEP": "0", "HAR_MLP_SMALL": "0"},
    "small": {"HAR_MLP_FUSED": "1", "HAR_MLP_STEP": "1", "HAR_MLP_SMALL": "1"},
    "gemm": {"HAR_MLP_FUSED": "1", "HAR_MLP_STEP": "1", "HAR_MLP_SMALL": "1"},  # routed by the shape alone
}


def _engine(monkeypatch, cuda, path, layers, B, **kw):
    from har.models.mlp import MLPEngine

    for k, v in PATH_ENV[path].items():
        monkeypatch.setenv(k, v)
    return MLPEngine(layers, B, cuda, seed=kw.pop("seed", ENGINE_SEED), **kw)


def _run_batch(eng, path, Xb, y32, B):
    """One batch on the engine's native path; returns the flat gradient (fp64, on the host)."""
    if path == "small":
        # the small path is a whole step whose reduction feeds Adam without storing G: the gradient it
        # applied is the sum of the B / 32 per-tile slabs its kernel wrote (the Adam side of that
        # reduction is what test_mlp_padding_inert_through_adamw compares)
        eng.train_step(Xb, y32, B)
        G = eng.slabs[: B // 32].double().sum(0)
    else:
        eng.forward_backward_native(Xb, y32, 1.0 / B)
        eng.reduce_grads_native()
        G = eng.G.double()
    torch.cuda.synchronize()
    assert eng.last_path == path, f"ran {eng.last_path}, wanted {path}"
    return G.cpu()


# ------------------------------------------------------------------------------ 1. the oracle (CPU)
@pytest.mark.parametrize("layers", [[5, 32, 32, 3], [33, 64, 96, 17], [1, 32, 1]])
def test_oracle_matches_autograd(layers):
    """Without the bf16 roundings the oracle is plain backprop: its gradients equal torch.autograd of
    the fp64 network with cross_entropy(reduction="sum") * scale."""
    from har.models.mlp import FlatLayout, init_params

    L = FlatLayout(layers)
    B, scale = 37, 1.0 / 37
    g = torch.Generator().manual_seed(4)
    P = init_params(L, 7).double()
    for s in L.segments:  # biases off zero, padding kept zero
        if s.name.startswith("b"):
            n = L.num_classes if s.name == "bout" else s.numel
            L.view(P, s.name)[:n] = torch.randn(n, generator=g, dtype=torch.float64) * 0.1
    X = torch.zeros(B, L.in_pad, dtype=torch.float64)
    X[:, :layers[0]] = torch.randn(B, layers[0], generator=g, dtype=torch.float64)
    y = torch.randint(0, layers[-1], (B,), generator=g)
    got = mlp_oracle(P, L, X, y, scale, round_bf16=False)

    Pa = P.clone().requires_grad_(True)
    h = X
    for i in range(len(L.hidden)):
        h = torch.relu(h @ L.view(Pa, f"W{i}").T + L.view(Pa, f"b{i}"))
    C = L.num_classes
    z = h @ L.view(Pa, "Wout")[:C].T + L.view(Pa, "bout")[:C]
    loss = torch.nn.functional.cross_entropy(z, y, reduction="sum")
    (ga,) = torch.autograd.grad(loss * scale, Pa)
    torch.testing.assert_close(got["logits"], z.detach(), rtol=1e-12, atol=1e-13)
    assert abs(got["loss"] - float(loss.detach())) <= 1e-10 * abs(float(loss.detach()))
    assert got["correct"] == int((_first_argmax(z.detach()) == y).sum())
    for s in L.segments:
        ref = L.view(ga, s.name)
        # rtol 1e-10; the atol is fp64 cancellation noise of the sums (1e-14 of the segment's largest entry)
        torch.testing.assert_close(got["grads"][s.name], ref, rtol=1e-10, atol=1e-14 * float(ref.abs().max()))
    if C > 1:
        assert all(float(got["grads"][s.name].abs().max()) > 0 for s in L.segments), "a vacuous comparison"


def test_argmax_ambiguity_share_of_the_seeds():
    """The seeds of the gradient cases: the oracle alone leaves at most 2 % of the rows with an argmax
    the logits tolerance cannot decide, so the correct-count comparison below excludes few rows."""
    from har.models.mlp import FlatLayout, init_params

    for path, layers, B, labels in GRAD_CASES:
        L = FlatLayout(layers)
        Xb, y = _inputs(layers, B, DATA_SEED, labels)
        z = mlp_oracle(init_params(L, ENGINE_SEED), L, Xb, y, 1.0 / B)["logits"]
        amb, _ = _ambiguous(z)
        assert int(amb.sum()) <= AMBIGUOUS_CAP * B, (path, layers, B, int(amb.sum()))


# ------------------------------------------------------ 2. gradients, loss, correct count per path
def _check_against_oracle(eng, G, ref, y, F, B, tag):
    L = eng.layout
    C = L.num_classes
    worst = 0.0
    for name, r in ref["grads"].items():
        a = L.view(G, name)
        rel = float((a - r).norm() / r.norm().clamp_min(1e-12))
        worst = max(worst, rel)
        print(f"MLPSHAPES {tag} {name} rel={rel:.3e}")
        assert rel < GRAD_TOL, f"{tag} {name}: rel err {rel:.3e}"
    # per class: a wrong lane whose class has a small gradient hides in the segment norm
    aw, rw = L.view(G, "Wout")[:C], ref["grads"]["Wout"][:C]
    rel_rows = (aw - rw).norm(dim=1) / rw.norm(dim=1).clamp_min(1e-12)
    ab, rbo = L.view(G, "bout")[:C], ref["grads"]["bout"][:C]
    rel_b = (ab - rbo).abs() / rbo.abs().max().clamp_min(1e-12)
    print(f"MLPSHAPES {tag} Wout_row rel={float(rel_rows.max()):.3e}")
    print(f"MLPSHAPES {tag} bout_elem rel={float(rel_b.max()):.3e}")
    assert float(rel_rows.max()) < GRAD_TOL, f"{tag} Wout class rows: {rel_rows.tolist()}"
    assert float(rel_b.max()) < GRAD_TOL, f"{tag} bout elements: {rel_b.tolist()}"
    # padded class rows / input columns receive exactly zero gradient
    assert L.view(G, "Wout")[C:].abs().sum() == 0 and L.view(G, "bout")[C:].abs().sum() == 0
    if F < L.in_pad:
        assert L.view(G, "W0")[:, F:].abs().sum() == 0
    assert bool(torch.isfinite(G).all())
    lsum, ncorrect = eng.last_loss_and_correct()
    print(f"MLPSHAPES {tag} loss rel={abs(lsum - ref['loss']) / max(abs(ref['loss']), 1e-30):.3e}")
    assert abs(lsum - ref["loss"]) <= 1e-2 * abs(ref["loss"]), f"{tag} loss {lsum} vs {ref['loss']}"
    # correct count: equal on the rows whose argmax the logits tolerance decides; an undecided row can
    # add one only if its label is within the tolerance of the maximum
    z = ref["logits"]
    amb, tol = _ambiguous(z)
    share = float(amb.float().mean())
    hit = _first_argmax(z) == y
    lo = int((hit & ~amb).sum())
    zy = z[torch.arange(B), y]
    hi = lo + int((amb & (zy >= z.max(1).values - tol)).sum())
    assert share <= AMBIGUOUS_CAP, f"{tag}: {share:.2%} of the rows excluded as near ties"
    assert lo <= ncorrect <= hi, f"{tag}: correct {ncorrect}, oracle {lo}..{hi} ({share:.2%} of the rows excluded)"
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRAD_CASES, ids=_case_id)
def test_mlp_path_matches_oracle(cuda, monkeypatch, case):
    """Gradients (per segment, per class row of Wout, per element of bout), exact zeros on the padding,
    loss and correct count of one batch on each native path at the edge shapes."""
    path, layers, B, labels = case
    eng = _engine(monkeypatch, cuda, path, layers, B, lr=1e-3)
    Xb, y = _inputs(layers, B, DATA_SEED, labels)
    P0 = eng.P.detach().cpu().clone()
    G = _run_batch(eng, path, Xb.to(cuda), y.to(cuda).to(torch.int32), B)
    ref = mlp_oracle(P0, eng.layout, Xb, y, 1.0 / B)
    _check_against_oracle(eng, G, ref, y, layers[0], B, _case_id(case))


# ------------------------------------------------------------------------------ 3. analytic cases
ANALYTIC = {"step": ([43, 256, 256], 64), "fused_fwd": ([43, 128, 128], 48), "small": ([43, 128, 128], 32),
            "gemm": ([43, 64, 96], 77)}


def _set_params(eng, bout=None):
    """Zero weights and biases (optionally a given bout), bf16 / fragment copies refreshed."""
    eng.P.zero_()
    if bout is not None:
        eng.layout.view(eng.P, "bout")[:len(bout)] = torch.tensor(bout, device=eng.P.device)
    eng.refresh_bf16()


def _dbout_expected(p, y, C, scale):
    """Sum over the rows of the bf16-rounded (p_c - [y = c]) * scale terms, the terms in fp32 as the
    kernels form them; p: [B, C] fp64 probabilities."""
    onehot = torch.nn.functional.one_hot(y, C).float()
    terms = (p.float() - onehot) * torch.tensor(scale, dtype=torch.float32)
    return terms.to(torch.bfloat16).double().sum(0)


@pytest.mark.gpu
@pytest.mark.parametrize("path,C", [(p, C) for p in ANALYTIC for C in (1, 6, 16)] + [("gemm", 32)])
def test_mlp_zero_weights(cuda, monkeypatch, path, C):
    """All parameters zero: every logit is 0, the prediction is class 0 (the tie rule), the loss is
    B ln C, every weight gradient and hidden bias gradient is exactly 0 and dbout is the sum of the
    bf16-rounded (1/C - [y = c]) * scale."""
    hidden, B = ANALYTIC[path]
    layers = hidden + [C]
    eng = _engine(monkeypatch, cuda, path, layers, B, lr=1e-3)
    _set_params(eng)
    Xb, y = _inputs(layers, B, 21)
    y[:C] = torch.arange(C)  # every class present
    scale = 1.0 / B
    L, G = eng.layout, _run_batch(eng, path, Xb.to(cuda), y.to(cuda).to(torch.int32), B)
    lsum, ncorrect = eng.last_loss_and_correct()
    assert ncorrect == int((y == 0).sum())
    if C == 1:
        assert lsum == 0.0
    else:
        assert abs(lsum - B * math.log(C)) <= 1e-4 * B * math.log(C), (lsum, B * math.log(C))
    for name in ("Wout", "W1", "W0", "b1", "b0"):
        assert L.view(G, name).abs().sum() == 0, name
    want = _dbout_expected(torch.full((B, C), 1.0 / C, dtype=torch.float64), y, C, scale)
    got = L.view(G, "bout")
    assert got[C:].abs().sum() == 0
    if C == 1:
        assert got[0] == 0
    else:
        err = float((got[:C] - want).abs().max())
        print(f"MLPSHAPES zero-{path}-C{C} dbout abs err={err:.3e}")
        assert err <= B * 2.0 ** -24 * scale, (got[:C].tolist(), want.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(ANALYTIC))
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_mlp_large_logits(cuda, monkeypatch, path, sign):
    """Zero weights, bout = sign * [+100, -100, 0, ...]: a softmax that does not subtract the row
    maximum overflows.  sign = +1: random labels; sign = -1: every label is class 0, which sits at -100."""
    hidden, B = ANALYTIC[path]
    C = 6
    layers = hidden + [C]
    eng = _engine(monkeypatch, cuda, path, layers, B, lr=1e-3)
    bout = [sign * 100.0, -sign * 100.0] + [0.0] * (C - 2)
    _set_params(eng, bout)
    Xb, y = _inputs(layers, B, 22)
    y[:C] = torch.arange(C)
    if sign < 0:
        y.zero_()
    scale = 1.0 / B
    L, G = eng.layout, _run_batch(eng, path, Xb.to(cuda), y.to(cuda).to(torch.int32), B)
    lsum, ncorrect = eng.last_loss_and_correct()
    assert bool(torch.isfinite(G).all()) and math.isfinite(lsum)
    z = torch.tensor(bout, dtype=torch.float64).expand(B, C)
    ref_loss = float((torch.logsumexp(z, 1) - z[torch.arange(B), y]).sum())
    assert abs(lsum - ref_loss) <= 1e-4 * ref_loss, (lsum, ref_loss)
    assert ncorrect == int((y == (0 if sign > 0 else 1)).sum())
    want = _dbout_expected(torch.softmax(z, 1), y, C, scale)
    got = L.view(G, "bout")
    err = float((got[:C] - want).abs().max())
    print(f"MLPSHAPES large-{path}-{sign:+.0f} dbout abs err={err:.3e}")
    assert err <= B * 2.0 ** -24 * scale, (got[:C].tolist(), want.tolist())
    assert got[C:].abs().sum() == 0
    for name in ("Wout", "W1", "W0", "b1", "b0"):
        assert L.view(G, name).abs().sum() == 0, name


# ------------------------------------------------------------------------------ 4. serving kernels
GUARD = 64  # elements before and after the outputs (keeps the torch allocation's 256-byte alignment)


def _guarded(B, C, cuda):
    lg = torch.full((B * C + 2 * GUARD,), float("nan"), device=cuda)
    pr = torch.full((B + 2 * GUARD,), -7, dtype=torch.int32, device=cuda)
    return lg, pr


def _check_guarded(lg, pr, B, C, z_ref, tag, check_pred=True):
    torch.cuda.synchronize()
    lg, pr = lg.cpu(), pr.cpu()
    assert bool(torch.isnan(lg[:GUARD]).all()) and bool(torch.isnan(lg[GUARD + B * C:]).all()), f"{tag}: logits guard"
    out = lg[GUARD:GUARD + B * C].view(B, C)
    assert bool(torch.isfinite(out).all()), f"{tag}: an output element was not written"
    print(f"MLPSHAPES infer-{tag} logits abs err={float((out.double() - z_ref).abs().max()):.3e}")
    torch.testing.assert_close(out.double(), z_ref, rtol=LOGIT_RTOL, atol=LOGIT_ATOL)
    if check_pred:
        assert bool((pr[:GUARD] == -7).all()) and bool((pr[GUARD + B:] == -7).all()), f"{tag}: pred guard"
        assert torch.equal(pr[GUARD:GUARD + B].long(), _first_argmax(out)), f"{tag}: pred is not the first argmax"


@pytest.mark.gpu
@pytest.mark.parametrize("H,B", [(256, 64), (128, 16)])
@pytest.mark.parametrize("C", [1, 5, 16])
@pytest.mark.parametrize("F", [32, 33])
def test_mlp_infer_kernels_values_ties_bounds(cuda, monkeypatch, H, B, C, F):
    """mlp_fwd_infer, mlp_fwd_infer_f32 (row stride > F) and, for H = 256, mlp_step_fwd_infer, called
    as infer_fused / infer_fused_f32 call them but with logits / pred in the middle of NaN / -7 filled
    buffers: values vs the oracle, pred = first argmax of the kernel's own logits (one row has two
    equal classes), nothing written outside [B][C] / [B]."""
    from har.ops import _native

    layers = [F, H, H, C]
    eng = _engine(monkeypatch, cuda, "step", layers, B)
    L, mod, s = eng.layout, _native.kernels(), _native.stream_ptr()
    g = torch.Generator().manual_seed(31)
    P = eng.P.detach().cpu().clone()
    L.view(P, "bout")[:C] = torch.randn(C, generator=g) * 0.5
    if C > 2:  # an exact tie: two identical class rows (first index must win where they lead)
        L.view(P, "Wout")[C - 1] = L.view(P, "Wout")[1]
        L.view(P, "bout")[C - 1] = L.view(P, "bout")[1]
    eng.P.copy_(P.to(cuda))
    eng.refresh_bf16()
    ld = F + 5
    Xs = torch.randn(B, ld, generator=g)
    X = Xs[:, :F]
    Xb = torch.zeros(B, L.in_pad, dtype=torch.bfloat16)
    Xb[:, :F] = X.to(torch.bfloat16)
    z_ref = mlp_oracle(P, L, Xb, torch.zeros(B, dtype=torch.int64), 1.0)["logits"]
    w = lambda t, n: L.view(t, n).data_ptr()  # noqa: E731
    Xb_d, Xs_d = Xb.to(cuda), Xs.to(cuda)
    tag = f"H{H}-B{B}-C{C}-F{F}"

    lg, pr = _guarded(B, C, cuda)
    mod.mlp_fwd_infer(Xb_d.data_ptr(), L.in_pad, w(eng.Pb, "W0"), w(eng.P, "b0"), w(eng.Pb, "W1"), w(eng.P, "b1"), H,
                      w(eng.Pb, "Wout"), w(eng.P, "bout"), B, C, lg[GUARD:].data_ptr(), pr[GUARD:].data_ptr(), s)
    _check_guarded(lg, pr, B, C, z_ref, "fwd_infer-" + tag)

    lg, pr = _guarded(B, C, cuda)
    mod.mlp_fwd_infer_f32(Xs_d.data_ptr(), ld, F, L.in_pad, w(eng.Pb, "W0"), w(eng.P, "b0"), w(eng.Pb, "W1"),
                          w(eng.P, "b1"), H, w(eng.Pb, "Wout"), w(eng.P, "bout"), B, C, lg[GUARD:].data_ptr(),
                          pr[GUARD:].data_ptr(), s)
    _check_guarded(lg, pr, B, C, z_ref, "fwd_infer_f32-" + tag)

    if H == 256:
        assert eng.step_ok and eng._pf_fresh
        lg, pr = _guarded(B, C, cuda)
        mod.mlp_step_fwd_infer(Xb_d.data_ptr(), L.in_pad, eng.Pf.data_ptr(), w(eng.P, "b0"), w(eng.P, "b1"), 256,
                               w(eng.Pb, "Wout"), w(eng.P, "bout"), B, C, lg[GUARD:].data_ptr(),
                               pr[GUARD:].data_ptr(), s)
        _check_guarded(lg, pr, B, C, z_ref, "step_fwd_infer-" + tag)


@pytest.mark.gpu
def test_softmax_ce_head_logits_bounds_c17(cuda, monkeypatch):
    """C = 17 takes the GEMM path with the 32-wide head: MLPEngine.logits (77 rows through a 48-row
    engine: two chunks) vs the oracle, and the head kernel as logits() calls it with its output in the
    middle of a NaN-filled buffer."""
    from har.ops import _native
    from har.ops.gemm import EPI_BIAS_RELU, gemm_bf16

    layers, N, B = [43, 64, 96, 17], 77, 48
    eng = _engine(monkeypatch, cuda, "gemm", layers, B)
    assert not eng.fused_ok
    L, C = eng.layout, 17
    g = torch.Generator().manual_seed(32)
    X = torch.randn(N, 43, generator=g)
    Xb = torch.zeros(N, L.in_pad, dtype=torch.bfloat16)
    Xb[:, :43] = X.to(torch.bfloat16)
    z_ref = mlp_oracle(eng.P.cpu(), L, Xb, torch.zeros(N, dtype=torch.int64), 1.0)["logits"]
    out = eng.logits(X.to(cuda))
    assert out.shape == (N, C)
    torch.testing.assert_close(out.double().cpu(), z_ref, rtol=LOGIT_RTOL, atol=LOGIT_ATOL)
    Xb_d = Xb.to(cuda)
    for r0, r1 in ((0, B), (B, N)):
        n = r1 - r0
        acts = [Xb_d[r0:r1]] + [a[:n] for a in eng.acts[1:]]
        for i in range(2):
            gemm_bf16(acts[i], L.view(eng.Pb, f"W{i}"), acts[i + 1], M=n, N=eng.dims[i + 1], K=eng.dims[i], layout=0,
                      epi=EPI_BIAS_RELU, bias=L.view(eng.P, f"b{i}"))
        lg, pr = _guarded(n, C, cuda)
        _native.kernels().softmax_ce_head(acts[-1].data_ptr(), L.view(eng.Pb, "Wout").data_ptr(),
                                          L.view(eng.P, "bout").data_ptr(), 0, n, eng.dims[-1], C, 1.0, 0, 0, 0,
                                          lg[GUARD:].data_ptr(), _native.stream_ptr())
        _check_guarded(lg, pr, n, C, z_ref[r0:r1], f"softmax_ce_head-rows{r0}-{r1}", check_pred=False)


# --------------------------------------------------------- 5. padding inert through the optimizer
OPT_CASES = {"step": ([33, 256, 256, 5], 64), "fused_fwd": ([33, 128, 128, 5], 48), "small": ([33, 128, 128, 5], 32),
             "gemm": ([33, 64, 96, 5], 77)}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(OPT_CASES))
def test_mlp_padding_inert_through_adamw(cuda, monkeypatch, path):
    """Three train_steps with weight decay at C = 5, F = 33: the padded class rows / bias entries / input
    columns stay exactly zero in P and Pb, and the parameters follow three oracle AdamW steps.

    Tolerance: eps = 1 keeps the Adam update a Lipschitz function of the gradient (|d upd / d g| <=
    (1 + max|g| / eps) / eps), so the GRAD_TOL gradient criterion bounds the drift of a segment by
    lr / eps * (1 + max|g| / eps) * GRAD_TOL * sum_t |g_t|_F; the factor 1.5 covers the second-order
    term (the later gradients are taken at parameters that already differ by the first drift, bf16
    copies included).  On top of it the tolerance of test_adam_step (rtol = atol = 1e-5 per element)."""
    layers, B = OPT_CASES[path]
    F, C = layers[0], layers[-1]
    lr, b1, b2, eps, wd = 0.1, 0.9, 0.999, 1.0, 0.01
    eng = _engine(monkeypatch, cuda, path, layers, B, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    L = eng.layout
    Xb, y = _inputs(layers, B, DATA_SEED)
    Xb_d, y_d = Xb.to(cuda), y.to(cuda).to(torch.int32)
    P = eng.P.detach().cpu().double()
    P0 = P.clone()
    m, v = torch.zeros_like(P), torch.zeros_like(P)
    gsum = {s.name: 0.0 for s in L.segments}
    gmax = 0.0
    for t in range(1, 4):
        eng.train_step(Xb_d, y_d, B)
        assert eng.last_path == path
        grads = mlp_oracle(P, L, Xb, y, 1.0 / B)["grads"]
        g = torch.zeros_like(P)
        for s in L.segments:
            L.view(g, s.name).copy_(grads[s.name])
            gsum[s.name] += float(grads[s.name].norm())
            gmax = max(gmax, float(grads[s.name].abs().max()))
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        upd = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps)
        P = P - lr * (upd + wd * P)
    torch.cuda.synchronize()
    assert int(eng.step_count[0]) == 3
    Pk, Pb = eng.P.detach().cpu().double(), eng.Pb.detach().cpu().double()
    for flat, what in ((Pk, "P"), (Pb, "Pb")):
        assert L.view(flat, "Wout")[C:].abs().sum() == 0, what
        assert L.view(flat, "bout")[C:].abs().sum() == 0, what
        assert L.view(flat, "W0")[:, F:].abs().sum() == 0, what
    assert torch.equal(eng.Pb.cpu(), eng.P.to(torch.bfloat16).cpu())
    for s in L.segments:
        a, r, r0 = L.view(Pk, s.name), L.view(P, s.name), L.view(P0, s.name)
        drift = float((a - r).norm())
        bound = 1.5 * lr / eps * (1 + gmax / eps) * GRAD_TOL * gsum[s.name] + 1e-5 * (float(r.norm()) + s.numel ** 0.5)
        moved = float((r - r0).norm())
        print(f"MLPSHAPES adamw-{path} {s.name} drift={drift:.3e} bound={bound:.3e} moved={moved:.3e}")
        assert moved > 2 * bound, f"{s.name}: the bound does not resolve the update"
        assert drift <= bound, f"{path} {s.name}: |P - oracle| = {drift:.3e} > {bound:.3e}"
