"""The MLP step's backward (mlp_bwd4, LDS-DMA tile staging) at the smallest batches that reach each
case of its tile pipeline, for both padded input widths, against the fp64 manual backprop of
test_gpu_kernels.py::test_mlp_step_matches_torch (same rounding points, same tolerance).

Batches (64-row tiles, har_mlp_step_slices slices, dact2 double-buffered, X in a four-slot ring):
    64    one tile: prologue fills only
    128   two slices of one tile
    1088  17 tiles: slices of 2, one of 1, seven empty (clamped fills only)
    2560  40 tiles: slices of 3 (both dact2 buffer parities + the clamped tail), two empty
    4160  65 tiles: slices of 5 (every X slot refilled, odd last iteration), three empty
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCHES = [64, 128, 1088, 2560, 4160]
FEATURES = [43, 20]  # padded to 64 / 32 input columns


def _bf_round(x):
    return x.to(torch.bfloat16).float()


def _run(cuda, F, B, seed=3):
    from har.models.mlp import MLPEngine, pad_input_bf16

    eng = MLPEngine([F, 256, 256, 6], B, cuda, lr=1e-3, seed=seed)
    g = torch.Generator(device=cuda).manual_seed(9 + B + F)
    X = torch.randn(B, F, device=cuda, generator=g)
    y = torch.randint(0, 6, (B,), device=cuda, generator=g)
    Xb = pad_input_bf16(X, eng.layout.in_pad)
    assert eng.layout.in_pad == (64 if F > 32 else 32)
    y32 = y.to(torch.int32)
    eng.forward_backward_native(Xb, y32, 1.0 / B)
    eng.reduce_grads_native()
    assert eng.last_path == "step"
    return eng, Xb, y, y32


@pytest.mark.parametrize("F", FEATURES)
@pytest.mark.parametrize("B", BATCHES)
def test_bwd_stage_matches_fp64(cuda, B, F):
    eng, Xb, y, _ = _run(cuda, F, B)
    L = eng.layout
    P = eng.P.double()
    W = {s.name: L.view(P, s.name) for s in L.segments}
    Wb = {k: _bf_round(v.float()).double() for k, v in W.items()}
    C = L.num_classes
    h0 = Xb.double()
    h1 = _bf_round((h0 @ Wb["W0"].T + W["b0"]).clamp_min(0).float()).double()
    h2 = _bf_round((h1 @ Wb["W1"].T + W["b1"]).clamp_min(0).float()).double()
    z = h2 @ Wb["Wout"][:C].T + W["bout"][:C]
    p = torch.softmax(z, 1)
    p[torch.arange(B), y] -= 1
    dl = _bf_round((p / B).float()).double()
    ref = {"Wout": dl.T @ h2, "bout": dl.sum(0)}
    dh2 = _bf_round(((dl @ Wb["Wout"][:C]) * (h2 > 0)).float()).double()
    ref["W1"], ref["b1"] = dh2.T @ h1, dh2.sum(0)
    dh1 = _bf_round(((dh2 @ Wb["W1"]) * (h1 > 0)).float()).double()
    ref["W0"], ref["b0"] = dh1.T @ h0, dh1.sum(0)
    G = eng.G.double()
    errs = {}
    for name, r in ref.items():
        a = L.view(G, name)
        a = a[:C] if name in ("Wout", "bout") else a
        errs[name] = float((a - r).norm() / r.norm().clamp_min(1e-12))
    print(f"B {B} F {F}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, rel in errs.items():
        assert rel < 1e-2, f"{name}: rel err {rel:.3e}"
    # padded input columns receive exactly zero gradient
    assert L.view(G, "W0")[:, F:].abs().max() == 0


@pytest.mark.parametrize("F,B", [(43, 4160), (20, 2560)])
def test_bwd_stage_deterministic(cuda, F, B):
    eng, Xb, _, y32 = _run(cuda, F, B)
    g0 = eng.G.clone()
    eng.forward_backward_native(Xb, y32, 1.0 / B)
    eng.reduce_grads_native()
    assert eng.last_path == "step"
    assert torch.equal(g0, eng.G)
