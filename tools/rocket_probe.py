#!/usr/bin/env python3
"""Time of the rocket kernel (``har_rocket_features``) against the torch definition on the same device.

For every shape the kernel is timed between two HIP events after warm-up runs, the median of ``--repeats``
runs is reported together with the rate in windows per second and the useful work it stands for: per window
``84 n_dil W`` convolution values of ``4 m`` flops each (``m``: the mean axis-subset size) plus ``q`` compares.
The torch form is ``rocket_features_torch`` on the device (float64, chunked); it is timed once on a slice of
``--torch-windows`` windows and scaled to the shape, which the record says.  Before timing, the kernel's counts
on an integer-valued copy of the slice are checked for equality with the definition.  Sets no bar.

    python tools/rocket_probe.py [--out profiles/r17/rocket_probe.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from har.ops import rocket as R  # noqa: E402

# (n_windows, window, axes, stride)
SHAPES = [(65536, 200, 3, 200), (131071, 200, 3, 100), (60000, 500, 9, 500)]


def problem(nw, W, A, stride, dev):
    g = torch.Generator().manual_seed(nw + W + A)
    s = torch.randn((nw - 1) * stride + W, A, generator=g)
    p = R.fit_rocket_params(s[: 512 * W], W, W, 1680, seed=1)
    return s.to(dev), p


def kernel_ms(s, p, W, stride, repeats):
    nw = R._window_count(s.shape[0], W, stride)
    out = torch.empty(nw, p.n_features, dtype=torch.float32, device=s.device)
    for _ in range(3):
        R.rocket_features_into(s, p, W, stride, out, 0)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        R.rocket_features_into(s, p, W, stride, out, 0)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def torch_ms(s, p, W, stride, n):
    part = s[: (n - 1) * stride + W]
    R.rocket_features_torch(part[: 8 * W], p, W, stride)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    R.rocket_features_torch(part, p, W, stride)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def check_exact(s, p, W, stride, n):
    part = torch.round(s[: (n - 1) * stride + W] * 64.0).contiguous()      # integer-valued: the sums are exact
    pi = R.RocketParams(W, p.axes, p.masks, torch.round(p.biases * 64.0) + 0.5)
    out = torch.empty(n, pi.n_features, dtype=torch.float32, device=s.device)
    counts = torch.empty(n, pi.n_features, dtype=torch.int32, device=s.device)
    R.rocket_features_into(part, pi, W, stride, out, 0, counts)
    return bool(torch.equal(counts, R.rocket_counts_torch(part, pi, W, stride)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--torch-windows", type=int, default=2048)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rocket_probe: no GPU (the probe measures the HIP kernel; there is no fallback)")
    dev = torch.device("cuda:0")
    lines = [f"rocket_probe: {torch.cuda.get_device_name(0)}, HIP-event medians of {a.repeats} runs after 3 warm-up runs",
             "windows x W x A @ stride | F | kernel ms (min..max) | windows/s | conv Gflop/s | torch fp64 ms "
             f"(measured on {a.torch_windows} windows, scaled) | ratio | counts exact on integer copy"]
    for nw, W, A, stride in SHAPES:
        s, p = problem(nw, W, A, stride, dev)
        ok = check_exact(s, p, W, stride, min(nw, 256))
        med, lo, hi = kernel_ms(s, p, W, stride, a.repeats)
        n_t = min(nw, a.torch_windows)
        t_ms = torch_ms(s, p, W, stride, n_t) * (nw / n_t)
        m = float(sum(bin(int(v)).count("1") for v in p.masks.flatten())) / p.masks.numel()
        flops = nw * R.N_KERNELS * len(p.dilations) * W * (4.0 * m + p.q)
        lines.append(f"{nw} x {W} x {A} @ {stride} | {p.n_features} | {med:.3f} ({lo:.3f}..{hi:.3f}) | "
                     f"{nw / med * 1e3:.4g} | {flops / med / 1e6:.1f} | {t_ms:.1f} | {t_ms / med:.1f}x | {ok}")
    lines.append("not measured: the kernel under rocprofv3 (VALU / LDS counters), the share of the VALU peak, "
                 "an MFMA formulation, end-to-end main.py --preset rocket on the device")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
