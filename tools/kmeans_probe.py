#!/usr/bin/env python3
"""Per-iteration time of the K-means kernels against the PyTorch definitions on the same device.

For every shape, one Lloyd iteration = ``kmeans_assign`` (scores, argmin, fixed-point sums, cost partials) +
``kmeans_update``; ``--iters`` iterations are enqueued back to back between two HIP events (tolerance -1:
the fit never freezes), after a warm-up run, and the median of ``--repeats`` runs is reported.  The kernel
loop runs under ``torch.cuda.set_sync_debug_mode("error")``: any device -> host read inside it would raise.
The same loop then runs on the torch definitions of ``har/ops/kmeans.py`` (``native=False``; their update
reads its two state words on the host, as the CPU path does).  The silhouette is timed the same way:
``silhouette_native`` (moments + kernel) against the fp64 O(N K) definition.  Sets no bar.

    python tools/kmeans_probe.py [--out profiles/r10/kmeans_probe.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from har.ops import kmeans as KM  # noqa: E402

SHAPES = [(65536, 43, 6), (65536, 43, 64), (1000000, 43, 16), (65536, 172, 32)]


def problem(N, D, K, dev):
    g = torch.Generator().manual_seed(N + D + K)
    mu = torch.randn(max(K, 2), D, generator=g) * 3.0
    c = torch.randint(0, mu.shape[0], (N,), generator=g)
    X = (mu[c] + torch.randn(N, D, generator=g)).to(dev)
    Xc = (X - KM.column_means(X).view(1, D)).contiguous()
    C0 = Xc[torch.randperm(N, generator=g)[:K].to(dev)].contiguous()
    return Xc, C0, KM.feature_scales(Xc), KM.norm_scale(KM.row_norms(Xc))


def lloyd_ms(Xc, C0, scale, nscale, native, iters, guard):
    st = KM.FitState.alloc(C0, iters)
    nb = max(1, -(-Xc.shape[0] // KM.rows_per_block()))
    part = torch.zeros(nb, dtype=torch.float64, device=Xc.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if guard:
        torch.cuda.set_sync_debug_mode("error")
    try:
        e0.record()
        for _ in range(iters):
            r = KM.assign(Xc, st.C, st.h, native, scale=scale, nscale=nscale, acc=st.acc, want_assign=False,
                          want_cost=True, part_out=part)
            KM.update(st, scale, r.part, -1.0, iters, native)
        e1.record()
    finally:
        if guard:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, float(st.cost_hist[iters - 1])


def timed(fn, repeats):
    fn()  # warm-up: code objects, allocator
    out = [fn() for _ in range(repeats)]
    return statistics.median(v[0] for v in out), out[-1][1]


def sil_ms(Xc, lab, K, native):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    s = KM.silhouette_native(Xc, lab, K) if native else KM.silhouette_rows_torch(Xc, lab, K).mean()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), float(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "kmeans_probe.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"K-means probe: {a.iters} iterations per run, median of {a.repeats} runs after a warm-up run, "
             f"device {torch.cuda.get_device_name(0)}",
             "kernel loops ran under torch.cuda.set_sync_debug_mode('error'): no device -> host read between the "
             "first and the last launch"]
    for N, D, K in SHAPES:
        Xc, C0, scale, nscale = problem(N, D, K, dev)
        kt, npass, lds_acc, nbytes = KM.native_plan(D, K)
        k_ms, k_cost = timed(lambda: lloyd_ms(Xc, C0, scale, nscale, True, a.iters, True), a.repeats)
        t_ms, t_cost = timed(lambda: lloyd_ms(Xc, C0, scale, nscale, False, a.iters, False), a.repeats)
        lab = KM.assign(Xc, C0, KM.center_h(C0), True, want_cost=False).assign
        ks_ms, ks = timed(lambda: sil_ms(Xc, lab, K, True), a.repeats)
        ts_ms, ts = timed(lambda: sil_ms(Xc, lab, K, False), a.repeats)
        lines.append(f"{N} x {D}, K = {K} (slab {kt} centres x {npass}, accumulators in "
                     f"{'LDS' if lds_acc else 'global memory'}, {nbytes} B LDS):")
        lines.append(f"  assign + update per iteration: kernels {k_ms * 1e3:9.1f} us   torch definitions {t_ms * 1e3:10.1f} us"
                     f"   ratio {t_ms / k_ms:6.1f}x   (cost after {a.iters}: {k_cost:.6e} / {t_cost:.6e})")
        lines.append(f"  silhouette:                    kernels {ks_ms * 1e3:9.1f} us   torch definition  {ts_ms * 1e3:10.1f} us"
                     f"   ratio {ts_ms / ks_ms:6.1f}x   (value {ks:.6f} / {ts:.6f})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
