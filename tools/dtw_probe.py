#!/usr/bin/env python3
"""Time of ``dtw_search`` (search + merge, HIP-event medians) against the fp32 PyTorch definition on the same
device and against the VALU floor.

For every shape the search of N queries against M references runs ``--repeats`` times after a warm-up, under
``torch.cuda.set_sync_debug_mode("error")``, and the median is reported.  The PyTorch figure is the fp32
recurrence of ``har/ops/dtw.py`` (``cost_torch_fp32``: vectorised across pairs, sequential over cells) on a
subset of ``--torch-pairs`` pairs, scaled to N x M pairs.  The VALU floor is cells x instructions per cell:
``W (2 R + 1) - R (R + 1)`` cells of a pair, ``2 A + 2`` vector instructions of a cell (A subtractions, one
multiply, A - 1 fma, one min3, one add — the cell of the test-free column in the listing of ``tools/isa_cost.py``),
one wave64 instruction per 2 cycles per SIMD, 1024 SIMDs at 2.4 GHz.  Sets no bar.

    python tools/dtw_probe.py [--out profiles/r19/dtw_probe.txt]
"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from har.ops import dtw as DT  # noqa: E402

# (N, M, W, A, radius, k)
SHAPES = [(1625, 3793, 200, 3, 20, 5), (4096, 65536, 200, 3, 20, 10), (1024, 8192, 128, 9, 16, 5)]
SIMDS, HZ, ISSUE_CYCLES = 1024, 2.4e9, 2


def next_profile_dir():
    base = os.path.join(ROOT, "profiles")
    nums = [int(m.group(1)) for d in os.listdir(base) for m in [re.fullmatch(r"r(\d+)", d)] if m]
    return os.path.join(base, f"r{max(nums, default=0) + 1:02d}")


def event_ms(fn, repeats, guard=False):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if guard:
            torch.cuda.set_sync_debug_mode("error")
        try:
            e0.record()
            fn()
            e1.record()
        finally:
            if guard:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def floor_ms(N, M, W, A, R):
    cells = W * (2 * R + 1) - R * (R + 1)
    return N * M / 64.0 * cells * (2 * A + 2) * ISSUE_CYCLES / (SIMDS * HZ) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-pairs", type=int, default=16 * 1024)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"dtw_search on {torch.cuda.get_device_name(0)}: HIP-event medians of {a.repeats} runs (measured); "
             "torch fp32 scaled from a subset (measured on the subset); VALU floor computed, not measured"]
    for N, M, W, A, R, k in SHAPES:
        g = torch.Generator().manual_seed(N + M)
        Q = torch.randn(N, W, A, generator=g).to(dev)
        Rf = torch.randn(M, W, A, generator=g).to(dev)
        reps = a.repeats if N * M < 1 << 26 else max(1, a.repeats // 2)
        ms = event_ms(lambda: DT.neighbors_native(Q, Rf, k, R), reps, guard=True)
        nq = 16
        mr = max(1, min(M, a.torch_pairs // nq))
        tms = event_ms(lambda: DT.cost_torch_fp32(Q[:nq], Rf[:mr], R), 1) * (N * M) / (nq * mr)
        fl = floor_ms(N, M, W, A, R)
        lines.append(f"N={N} M={M} W={W} A={A} R={R} k={k} splits={DT.auto_splits(N, M)}: kernel {ms:.2f} ms "
                     f"({N * M / ms / 1e3:.1f} M pairs/s) | torch fp32 {tms:.0f} ms scaled from {nq} x {mr} pairs "
                     f"({tms / ms:.0f} x) | VALU floor {fl:.2f} ms ({ms / fl:.2f} x the floor)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = a.out or os.path.join(next_profile_dir(), "dtw_probe.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
