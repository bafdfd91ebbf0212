#!/usr/bin/env python3
"""Timing probe of the HIP Viterbi decode (csrc/kernels/hmm.hip); its output is kept as profiles/r9/hmm_probe.txt.

    python tools/hmm_probe.py --shape 1      # T = 10,000,000, K = 6, one sequence (the 1B-sample pass's windows)
    python tools/hmm_probe.py --shape 2      # 65,536 sequences of 152 windows, K = 6 (+ viterbi_torch on the device)
    python tools/hmm_probe.py --shape 3      # T = 1,000,000, K = 32

Run each shape as its own process under its own ``timeout``.  Every figure is the median of 3 timed runs
(HIP events) after one warm-up.  Per phase the probe also prints the bytes the phase must move and that
volume over the HBM bandwidth as a floor, and an A/B over the chunk length L.
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


def phase_bytes(T, K, S, L):
    """Bytes each phase must move at least once (reads + writes)."""
    C = (T + L - 1) // L
    mats, vecs = C * K * K * 8, C * K * 8
    return {
        "flags": T + 8 * S,
        "chunk_matrices": 4 * T * K + T + mats,                 # E once, flags, the chunk matrices
        "chunk_scan": 2 * mats + 2 * vecs,                      # matrices up and down, the vectors
        "forward": 4 * T * K + T + T * K + vecs + C * K,        # E a second time, flags, psi written, maps
        "map_scan": 2 * C * K + C,
        "backtrace": T * K + 4 * T,                             # psi read (whole lines), path written
        "scores": 16 * S,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True, choices=sorted(SHAPES))
    ap.add_argument("--chunks", default="16,32,64,128,256", help="chunk lengths of the A/B")
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
    A, pi = model.qA.to(dev), model.qpi.to(dev)
    off = torch.arange(0, T + 1, T // S, dtype=torch.int64)
    off_d = off.to(dev)
    L0 = H.chunk_len()
    print(f"== shape {a.shape}: T = {T:,}, K = {K}, S = {S:,}  (default L = {L0}, scan group = {H.scan_group()})")
    mod = H._native.kernels()
    path = torch.empty(T, dtype=torch.int32, device=dev)
    score = torch.empty(S, dtype=torch.int64, device=dev)

    def decode(L, phases=None, ws=None):
        return H.viterbi_native(E, A, pi, off, chunk=L, out=(path, score), workspace=ws, phases=phases,
                                offsets_device=off_d)

    print("-- chunk length A/B (whole decode, device time, ms)")
    for L in [int(x) for x in a.chunks.split(",")]:
        ws = torch.empty(int(mod.hmm_workspace_bytes(T, K, S, L)), dtype=torch.uint8, device=dev)
        ms = timed(lambda: decode(L, ws=ws))
        print(f"L = {L:4d}: {ms:9.3f} ms   workspace {ws.numel() / 2**20:8.1f} MiB")
        del ws
    ws = torch.empty(int(mod.hmm_workspace_bytes(T, K, S, L0)), dtype=torch.uint8, device=dev)
    total = timed(lambda: decode(L0, ws=ws))
    raw_acc = float((E.argmax(1) == y).double().mean())
    acc = float((path.long() == y).double().mean())
    print(f"-- L = {L0}: whole decode {total:.3f} ms  ({T / total / 1e3:.1f} M windows/s); "
          f"argmax accuracy {raw_acc:.4f} -> decoded {acc:.4f}")
    print("   (the 1B-sample window pass this would follow takes 12.73 ms)")
    print(f"-- phases at L = {L0} (ms; bytes the phase must move; that volume at {HBM_BYTES_PER_S / 1e12:.0f} TB/s)")
    nbytes = phase_bytes(T, K, S, L0)
    ssum = 0.0
    for p, name in enumerate(H.PHASES):
        ms = timed(lambda: decode(L0, phases=(p, p), ws=ws))
        ssum += ms
        print(f"{p} {name:15s} {ms:9.3f} ms   {nbytes[name] / 1e6:10.1f} MB   floor {nbytes[name] / HBM_BYTES_PER_S * 1e3:7.3f} ms")
    print(f"  sum of phases   {ssum:9.3f} ms")
    if a.shape == 2:
        want = None

        def torch_decode():
            nonlocal want
            want = H.viterbi_torch(E, A, pi, off)

        ms = timed(torch_decode)
        decode(L0, ws=ws)
        same = torch.equal(want[0], path) and torch.equal(want[1], score)
        print(f"-- viterbi_torch on the device, vectorised across the {S:,} sequences: {ms:.3f} ms "
              f"({ms / total:.1f}x the kernels); results equal: {same}")
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
