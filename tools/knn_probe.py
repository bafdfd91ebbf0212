#!/usr/bin/env python3
"""Per-kernel time of the k-nearest-neighbour kernels against the torch form on the same device.

For every shape ``knn_search`` (scores on the fp32 matrix cores fused with the running top-k; the automatic
reference split) and ``knn_merge_vote`` (merge of the splits' lists, d2, distance-weighted vote over 6 classes)
are each timed between two HIP events after a warm-up run; the median of ``--repeats`` runs is reported,
with the ratio of the search to the fp32-MFMA floor ``2 N M Dp / 157 TFLOP/s`` (Dp = D rounded up to 4).  The
kernel pair runs under ``torch.cuda.set_sync_debug_mode("error")``: a device -> host read between the two
launches would raise.  The torch form is ``h - Q @ R.T`` followed by ``topk``: it materialises the N x M fp32
scores, and where they (and topk's workspace) do not fit the device's free memory the probe says so instead
of timing it.  Sets no bar.

    python tools/knn_probe.py [--out profiles/r16/knn_probe.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from har.ops import _native  # noqa: E402
from har.ops import knn as KN  # noqa: E402

SHAPES = [(1625, 3793, 43, 5), (65536, 65536, 43, 10), (4096, 1000000, 43, 10), (65536, 65536, 172, 32)]
PEAK_FP32_MFMA = 157e12
CLASSES = 6


def problem(N, M, D, dev):
    g = torch.Generator().manual_seed(N + M + D)
    mu = torch.randn(8, D, generator=g) * 3.0
    X = mu[torch.randint(0, 8, (N + M,), generator=g)] + torch.randn(N + M, D, generator=g)
    mean, std = KN.standardizer(X)
    Z = KN.working_rows(X, mean, std).to(dev)
    Q, R = Z[:N].contiguous(), Z[N:].contiguous()
    y = torch.randint(0, CLASSES, (M,), generator=g).to(torch.int32).to(dev)
    return Q, R, KN.reference_h(R), y


def kernels_ms(Q, R, h, y, k, S):
    mod = _native.kernels()
    N, D = Q.shape
    M = R.shape[0]
    dev = Q.device
    ps = torch.empty(S, N, k, dtype=torch.float32, device=dev)
    pi = torch.empty(S, N, k, dtype=torch.int32, device=dev)
    idx = torch.empty(N, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(N, k, dtype=torch.float32, device=dev)
    raw = torch.empty(N, CLASSES, dtype=torch.float64, device=dev)
    prob = torch.empty_like(raw)
    pred = torch.empty(N, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    st = _native.stream_ptr()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev[0].record()
        mod.knn_search(Q.data_ptr(), N, R.data_ptr(), h.data_ptr(), M, D, k, S, 0, 0, ps.data_ptr(), pi.data_ptr(), st)
        ev[1].record()
        mod.knn_merge_vote(ps.data_ptr(), pi.data_ptr(), S, Q.data_ptr(), D, N, k, k, idx.data_ptr(), d2.data_ptr(),
                           y.data_ptr(), M, CLASSES, 1, raw.data_ptr(), prob.data_ptr(), pred.data_ptr(), st)
        ev[2].record()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return (ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])), idx


def torch_ms(Q, R, h, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    s = h.view(1, -1) - Q @ R.t()
    i = torch.topk(s, k, dim=1, largest=False).indices
    e1.record()
    torch.cuda.synchronize()
    return (e0.elapsed_time(e1),), i


def timed(fn, repeats):
    fn()  # warm-up: code objects, allocator
    out = [fn() for _ in range(repeats)]
    n = len(out[0][0])
    return [statistics.median(o[0][j] for o in out) for j in range(n)], out[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "knn_probe.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"kNN probe: median of {a.repeats} runs after a warm-up run, device {torch.cuda.get_device_name(0)}",
             "the kernel pair ran under torch.cuda.set_sync_debug_mode('error'): no device -> host read between the "
             "launches", f"floor = 2 N M Dp / {PEAK_FP32_MFMA / 1e12:.0f} TFLOP/s (fp32 MFMA peak)"]
    for N, M, D, k in SHAPES:
        Q, R, h, y = problem(N, M, D, dev)
        S = KN.auto_splits(N, M, D)
        (s_ms, v_ms), idx = timed(lambda: kernels_ms(Q, R, h, y, k, S), a.repeats)
        floor_ms = 2.0 * N * M * ((D + 3) // 4 * 4) / PEAK_FP32_MFMA * 1e3
        lines.append(f"{N} x {M} x {D}, k = {k} (slab {KN.slab_rows(D)} rows, {S} splits):")
        lines.append(f"  knn_search     {s_ms * 1e3:11.1f} us   floor {floor_ms * 1e3:9.1f} us   ratio to floor {s_ms / floor_ms:6.1f}x")
        lines.append(f"  knn_merge_vote {v_ms * 1e3:11.1f} us")
        need = 4 * N * M * 3  # the scores, the product before the subtraction, topk's workspace
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            lines.append(f"  torch form (h - Q @ R.T, topk): not timed, {need / 2**30:.1f} GiB of scores and workspace "
                         f"do not fit the {free / 2**30:.1f} GiB free")
            continue
        try:
            (t_ms,), ti = timed(lambda: torch_ms(Q, R, h, k), a.repeats)
        except torch.OutOfMemoryError:
            lines.append("  torch form (h - Q @ R.T, topk): not timed, out of device memory")
            continue
        same = float((ti == idx.long()).double().mean())
        lines.append(f"  torch form     {t_ms * 1e3:11.1f} us   (h - Q @ R.T, topk; {4 * N * M / 2**30:.2f} GiB of scores)   "
                     f"ratio {t_ms / (s_ms + v_ms):6.1f}x   equal list entries {same:.6f}")
        del ti
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
