#!/usr/bin/env python3
"""Timing probe of the HIP forward-backward (csrc/kernels/hmm_fb.hip); its output is kept as
profiles/r12/hmm_fb_probe.txt.

    python tools/hmm_fb_probe.py --shape 1      # T = 10,000,000, K = 6, one sequence
    python tools/hmm_fb_probe.py --shape 2      # 65,536 sequences of 152 windows, K = 6 (+ the torch definition on the device)
    python tools/hmm_fb_probe.py --shape 3      # T = 1,000,000, K = 32 (+ the phase-1 A/B: (i, j) lanes vs f64 MFMA)

The shapes are those of tools/hmm_probe.py.  Run each as its own process under its own ``timeout``.  Every
figure is the median of 3 timed runs (HIP events) after one warm-up.  Per phase the probe also prints the bytes
the phase must move and that volume over the HBM bandwidth as a floor.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from har.models.hmm import HMMSmoother  # noqa: E402
from har.ops import hmm as H  # noqa: E402

HBM_BYTES_PER_S = 8.0e12   # MI355X peak HBM3E bandwidth
SHAPES = {1: (10_000_000, 6, 1), 2: (65_536 * 152, 6, 65_536), 3: (1_000_000, 32, 1)}


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def phase_bytes(T, K, S, L, want_xi):
    """Bytes each phase must move at least once (reads + writes)."""
    C = (T + L - 1) // L
    mats, vecs = C * (K * K + 1) * 8, C * (K + 1) * 8
    return {
        "flags": T + 8 * S,
        "chunk_products": 8 * T * K + T + mats,                  # B once, flags, the chunk products
        "prefix_scan": 2 * mats + 2 * vecs,                      # products up and down, the vectors
        "suffix_scan": mats + 2 * vecs,                          # the same products down again
        "chunk_pass": 8 * T * K + T + 8 * T * K + 2 * vecs + 16 * S + (C * K * K * 8 if want_xi else 0),
        "reductions": 24 * S + (C * K * K * 8 if want_xi else 0),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True, choices=sorted(SHAPES))
    a = ap.parse_args()
    T, K, S = SHAPES[a.shape]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(a.shape)
    # emissions of a plausible classifier: labels in runs of 8, a softmax that is right ~80% of the time
    y = torch.repeat_interleave(torch.randint(0, K, ((T + 7) // 8,), device=dev, generator=g), 8)[:T]
    logits = torch.randn(T, K, device=dev, generator=g) * 1.5
    logits[torch.arange(T, device=dev), y] += 2.5
    model = HMMSmoother(stay=0.9).fit_stay(K)
    E = model.emission_scores(torch.softmax(logits, 1))
    del logits
    raw_acc = float((E.argmax(1) == y).double().mean())
    B = H.emission_likelihoods(E)
    del E
    P, p0 = model.P.to(dev), model.p0.to(dev)
    off = torch.arange(0, T + 1, T // S, dtype=torch.int64)
    off_d = off.to(dev)
    L = H.chunk_len()
    print(f"== shape {a.shape}: T = {T:,}, K = {K}, S = {S:,}  (L = {L}, scan group = {H.scan_group()})")
    mod = H._native.kernels()
    out = (torch.empty(T, K, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float64, device=dev),
           torch.empty(K, K, dtype=torch.float64, device=dev))
    ws = torch.empty(int(mod.hmm_fb_workspace_bytes(T, K, S, L, True)), dtype=torch.uint8, device=dev)

    def run(want_xi=True, phases=None, variant="auto"):
        return H.forward_backward_native(B, P, p0, off, want_xi=want_xi, out=out, workspace=ws, phases=phases,
                                         offsets_device=off_d, variant=variant)

    total = timed(run)
    acc = float((out[0].argmax(1) == y).double().mean())
    print(f"-- gamma + loglik + xi: {total:.3f} ms  ({T / total / 1e3:.1f} M windows/s), workspace {ws.numel() / 2**20:.1f} MiB; "
          f"argmax accuracy {raw_acc:.4f} -> posterior argmax {acc:.4f}")
    print(f"-- gamma + loglik only: {timed(lambda: run(False)):.3f} ms")
    if K > 8:
        for v in ("lanes", "mfma"):
            whole = timed(lambda: run(variant=v))
            ph1 = timed(lambda: run(phases=(1, 1), variant=v))
            print(f"-- phase 1 A/B, {v:5s}: chunk products {ph1:9.3f} ms, whole run {whole:9.3f} ms")
        run()
    print(f"-- phases with xi (ms; bytes the phase must move; that volume at {HBM_BYTES_PER_S / 1e12:.0f} TB/s)")
    nbytes = phase_bytes(T, K, S, L, True)
    ssum = 0.0
    for p, name in enumerate(H.FB_PHASES):
        ms = timed(lambda: run(phases=(p, p)))
        ssum += ms
        print(f"{p} {name:15s} {ms:9.3f} ms   {nbytes[name] / 1e6:10.1f} MB   floor {nbytes[name] / HBM_BYTES_PER_S * 1e3:7.3f} ms")
    print(f"  sum of phases   {ssum:9.3f} ms")
    if a.shape == 2:
        want = None

        def torch_fb():
            nonlocal want
            want = H.forward_backward_torch(B, P, p0, off, want_xi=True)

        ms = timed(torch_fb)
        run()
        eta = 16.0 * (K + 4) * T * 2.0 ** -53
        err = max(float(((out[0] - want[0]).abs() / want[0]).max()), float(((out[2] - want[2]).abs() / want[2]).max()),
                  float(((out[1] - want[1]).abs() / (1 + want[1].abs())).max()))
        print(f"-- forward_backward_torch on the device, vectorised across the {S:,} sequences: {ms:.3f} ms "
              f"({ms / total:.1f}x the kernels); largest error / eta against it: {err / eta:.3g}")
        if not err <= eta:
            sys.exit(1)


if __name__ == "__main__":
    main()
