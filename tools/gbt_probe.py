#!/usr/bin/env python3
"""Fit time of the GBT kernels against the PyTorch definitions on the same device.

Shape: 60,000 x 43 rows, K = 6, 100 rounds at depth 6 (class-conditional Gaussian features).  Reports
the wall time of ``GBTClassifier.fit_tensors`` through the HIP kernels (warm-up fit, then the median
of ``--repeats`` fits, each bracketed by device synchronisation), the time per kernel (HIP events
around every launch of one more instrumented fit) and the same fit on the torch definitions of
``har/ops/gbt.py`` running on the device (a warm-up of 3 rounds, then the median of ``--repeats``
fits as well).  Sets no bar.

    python tools/gbt_probe.py [--out profiles/r8/gbt_probe.txt] [--rows 60000] [--rounds 100] [--depth 6]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from har.models import gbt as M  # noqa: E402
from har.ops import gbt as G  # noqa: E402
from har.ops import tree as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r8", "gbt_probe.txt"))
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--features", type=int, default=43)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    mu = torch.randn(a.classes, a.features, generator=g)
    y = torch.randint(0, a.classes, (a.rows,), generator=g)
    X = (mu[y] + 2.0 * torch.randn(a.rows, a.features, generator=g)).to(dev)
    y = y.to(dev)
    tt = T.ThresholdTable.from_any(T.thresholds_for(X, 32, seed=0))

    def fit(rounds, native=True):
        est = M.GBTClassifier(maxIter=rounds, maxDepth=a.depth, seed=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = est._fit_tensors(X, y, a.classes, thresholds=tt, native=native)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, m

    lines = [f"GBT fit probe: {a.rows} x {a.features}, K = {a.classes}, {a.rounds} rounds, depth {a.depth}, "
             f"device {torch.cuda.get_device_name(0)}"]
    fit(3)  # warm-up: code objects, allocator
    times = []
    for _ in range(a.repeats):
        t, model = fit(a.rounds)
        times.append(t)
    lines.append(f"kernels: fit {statistics.median(times) * 1e3:.1f} ms (median of {a.repeats}: "
                 + ", ".join(f"{t * 1e3:.1f}" for t in times) + f"), final training loss {model.trainLossHistory[-1]:.6f}")

    # per kernel: HIP events around every launch of one more fit
    spans = {}
    names = ("grad_native", "hist_native", "split_native", "partition_native", "update_native")
    orig = {n: getattr(G, n) for n in names}

    def wrap(n):
        def f(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = orig[n](*args, **kw)
            e1.record()
            spans.setdefault(n, []).append((e0, e1))
            return r
        return f

    for n in names:
        setattr(G, n, wrap(n))
    try:
        t_inst, _ = fit(a.rounds)
    finally:
        for n in names:
            setattr(G, n, orig[n])
    torch.cuda.synchronize()
    total = 0.0
    for n in names:
        ms = sum(e0.elapsed_time(e1) for e0, e1 in spans.get(n, []))
        total += ms
        lines.append(f"  har_gbt_{n.split('_')[0]:<10} {len(spans.get(n, [])):6d} launches  {ms:9.2f} ms  "
                     f"({ms * 1e3 / max(1, len(spans.get(n, []))):8.1f} us each)")
    lines.append(f"  sum of kernel spans {total:.1f} ms of the instrumented fit's {t_inst * 1e3:.1f} ms")

    fit(3, native=False)
    ttimes = []
    for _ in range(a.repeats):
        t, mt = fit(a.rounds, native=False)
        ttimes.append(t)
    lines.append(f"torch definitions on the device: fit {statistics.median(ttimes) * 1e3:.1f} ms (median of {a.repeats}: "
                 + ", ".join(f"{t * 1e3:.1f}" for t in ttimes) + f"), final training loss {mt.trainLossHistory[-1]:.6f}")
    lines.append(f"ratio of the medians, torch / kernels: {statistics.median(ttimes) / statistics.median(times):.1f}x")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
