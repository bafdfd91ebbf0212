#!/usr/bin/env python3
"""Timing probe of the HIP stream filter (csrc/kernels/sosfilt.hip); its output is kept as
profiles/r20/sosfilt_probe.txt.

    python tools/sosfilt_probe.py --shape 1      # 13,107,200 x 3 samples = 65,536 windows of 200 (+ split, zero-phase, L A/B)
    python tools/sosfilt_probe.py --shape 2      # 100,000,000 x 3 samples
    python tools/sosfilt_probe.py --shape 3      # 30,000,000 x 9 samples = 60,000 windows of 500

Run each shape as its own process under its own ``timeout``.  The filter is the 3rd-order 0.3 Hz Butterworth low
pass (two sections).  Every figure is the median of 5 timed runs (HIP events) after one warm-up.  Per phase the
probe prints the bytes the phase must move at least once and that volume over the HBM bandwidth as a floor.
No hardware-counter run is made here.
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

from har.ops import sosfilt as F  # noqa: E402

HBM_BYTES_PER_S = 8.0e12   # MI355X peak HBM3E bandwidth
SHAPES = {1: (13_107_200, 3, 20.0), 2: (100_000_000, 3, 20.0), 3: (30_000_000, 9, 50.0)}


def timed(fn, reps=5):
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


def phase_bytes(S, A, ns, L, G, mode="filter", comp=False):
    """Bytes each phase must move at least once (reads + writes)."""
    n = F.scan_levels(S, L, G)
    st = 2 * ns * 8 * A                                        # one element's states
    OA = 2 * A if mode == "split" else A
    scan = sum(2 * m * st + 2 * m for m in n)                  # up: every level's states read and rewritten, flags
    scan += sum(m * st for m in n[1:])                         # up: the totals one level up
    scan += sum(2 * m * st + m + n[i + 1] * st for i, m in enumerate(n[:-1]))   # down
    return {
        "chunk_state": 4 * S * A + n[0] * (st + 1),
        "carry_scan": scan,
        "apply": 4 * S * A * (2 if comp else 1) + n[0] * st + 4 * S * OA,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True, choices=sorted(SHAPES))
    ap.add_argument("--chunks", default="32,64,128", help="chunk lengths of the A/B")
    a = ap.parse_args()
    S, A, hz = SHAPES[a.shape]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(a.shape)
    x = torch.randn(S, A, device=dev, generator=g).mul_(3.0).add_(9.8)
    sos = F.butter_sos(3, 0.3, hz)
    ns = sos.shape[0]
    mod = F._native.kernels()
    L0, G0 = F.chunk_len(), F.scan_group()
    print(f"== shape {a.shape}: S = {S:,} samples x {A} axes, {ns} sections  (default L = {L0}, G = {G0}, "
          f"{len(F.scan_levels(S, L0, G0))} scan levels)")
    out = torch.empty(S, A, device=dev)

    def run(L=L0, mode="filter", out_t=out, phases=None, ws=None, src=x, reverse=False, comp=None):
        return F.sosfilt_native(src, sos, None, "step", reverse, mode, comp=comp, chunk=L, out=out_t, workspace=ws, phases=phases)

    print("-- chunk length A/B (whole filter, device time, ms)")
    for L in [int(v) for v in a.chunks.split(",")]:
        ws = torch.empty(int(mod.sosfilt_workspace_bytes(S, A, ns, L, G0)), dtype=torch.uint8, device=dev)
        ms = timed(lambda: run(L, ws=ws))
        print(f"L = {L:4d}: {ms:9.3f} ms   workspace {ws.numel() / 2**20:8.1f} MiB")
        del ws
    ws = torch.empty(int(mod.sosfilt_workspace_bytes(S, A, ns, L0, G0)), dtype=torch.uint8, device=dev)

    def report(title, mode, fn_phase, comp=False):
        nbytes = phase_bytes(S, A, ns, L0, G0, mode, comp)
        total = timed(lambda: fn_phase(None))
        tb = sum(nbytes.values())
        print(f"-- {title}: {total:.3f} ms  ({S * A / total / 1e6:.1f} G sample-axes/s; {tb / 1e6:.1f} MB at "
              f"{HBM_BYTES_PER_S / 1e12:.0f} TB/s = {tb / HBM_BYTES_PER_S * 1e3:.3f} ms, ratio {total / (tb / HBM_BYTES_PER_S * 1e3):.2f})")
        ssum = 0.0
        for p, name in enumerate(F.PHASES):
            ms = timed(lambda: fn_phase((p, p)))
            ssum += ms
            floor = nbytes[name] / HBM_BYTES_PER_S * 1e3
            print(f"{p} {name:12s} {ms:9.3f} ms   {nbytes[name] / 1e6:10.1f} MB   floor {floor:7.3f} ms   ratio {ms / floor:6.2f}")
        print(f"  sum of phases {ssum:9.3f} ms")

    report(f"filter, L = {L0}", "filter", lambda ph: run(ws=ws, phases=ph))
    if a.shape == 1:
        out2 = torch.empty(S, 2 * A, device=dev)
        report("split [x - y | y]", "split", lambda ph: run(mode="split", out_t=out2, ws=ws, phases=ph))
        fwd = run(ws=ws).clone()
        report("zero-phase, second (reversed) pass into split", "split",
               lambda ph: run(mode="split", out_t=out2, ws=ws, phases=ph, src=fwd, reverse=True, comp=x), comp=True)

        def both():
            run(ws=ws, out_t=fwd)
            run(mode="split", out_t=out2, ws=ws, src=fwd, reverse=True, comp=x)

        print(f"-- zero-phase split, both passes: {timed(both):.3f} ms")


if __name__ == "__main__":
    main()
