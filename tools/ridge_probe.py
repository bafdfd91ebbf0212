#!/usr/bin/env python3
"""Per-kernel time of the ridge classifier's kernels against the torch form on the same device.

For every shape (N rows x D columns, K = 6, F = 5, 10 alphas) the moments (``ridge_gram`` + ``ridge_gram_reduce``),
the systems fill, the batched Cholesky and the back substitution are each timed between two HIP events after a
warm-up run; the median of ``--repeats`` runs is reported, with ``ridge_gram`` against its fp32-MFMA floor ``N
Dq^2 / 157 TFLOP/s`` and the factorisation against ``S D^3 / 3`` at the fp64 matrix rate (``--fp64-tflops``).  The
whole fit (``fit_native``: one host read) is timed by the wall clock around a synchronised call.  The torch form
is ``Z.T @ Z`` in fp64 with ``torch.linalg.cholesky`` / ``cholesky_solve`` on the device for the same number of
systems; where that call is unavailable the probe says so.  Sets no bar.

    python tools/ridge_probe.py [--out profiles/r18/ridge_probe.txt] [--shapes 2000x1680,65536x1680]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from har.ops import _native  # noqa: E402
from har.ops import ridge as RD  # noqa: E402

SHAPES = [(2000, 1680), (65536, 1680), (131071, 1680), (65536, 9996)]
PEAK_FP32_MFMA = 157e12
K, F = 6, 5


def problem(N, D, dev):
    g = torch.Generator(device=dev).manual_seed(N + D)
    y = torch.randint(0, K, (N,), device=dev, generator=g)
    X = torch.rand(N, D, device=dev, generator=g) + 0.05 * y.view(-1, 1).float()
    fold = np.random.RandomState(N).randint(0, F, N)
    return X.contiguous(), y, fold


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def probe(N, D, dev, repeats, fp64_tflops, lines):
    X, y, fold = problem(N, D, dev)
    alphas = RD.default_alphas()
    mean, inv_std = RD.standardizer(X[: min(N, 8192)])
    p = RD.prepare_native(X, y, fold, F, alphas, mean, inv_std)
    A, S, ldn, Dq = len(alphas), RD.num_systems(F, len(alphas)), RD.up64(D + K), D + K + 1
    per = max(1, min(S, RD.WORKSPACE_BYTES // (ldn * ldn * 8)))
    mod = _native.kernels()
    out = {}
    t_gram = timed(lambda: out.__setitem__("m", RD.moments_native(X, p["y32"], p["rows"], p["off"], p["mean"],
                                                                  p["inv_std"], K)), repeats)
    Af, Aall = out["m"]
    Sys = torch.empty(per, ldn, ldn, dtype=torch.float64, device=dev)
    info = torch.zeros(S, dtype=torch.int32, device=dev)
    W64 = torch.empty(S, K, ldn, dtype=torch.float64, device=dev)
    W = torch.empty(S, K, D, dtype=torch.float32, device=dev)
    b = torch.empty(S, K, dtype=torch.float32, device=dev)
    args = RD._solve_args(Af, Aall, p["alphas_t"], D, K, F, A, 0, per, Sys, info, W64, W, b)
    t_sys = timed(lambda: mod.ridge_solve(0, *args), repeats)

    def chol():
        mod.ridge_solve(0, *args)
        mod.ridge_solve(1, *args)
    t_chol = timed(chol, repeats) - t_sys
    t_back = timed(lambda: mod.ridge_solve(2, *args), repeats)
    del Sys, W64
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    RD.fit_native(X, y, fold, F, alphas, mean, inv_std, K)
    torch.cuda.synchronize()
    t_fit = (time.perf_counter() - t0) * 1e3
    floor = N * Dq * Dq / PEAK_FP32_MFMA * 1e3
    cfloor = per * D ** 3 / 3 / (fp64_tflops * 1e12) * 1e3
    lines.append(f"{N} x {D} (K = {K}, F = {F}, {A} alphas, {S} systems, {per} per batch)")
    lines.append(f"  ridge_gram + reduce   {t_gram:10.3f} ms   fp32-MFMA floor {floor:.3f} ms ({t_gram / floor:.1f}x)")
    lines.append(f"  ridge_systems         {t_sys:10.3f} ms   ({per} systems)")
    lines.append(f"  cholesky              {t_chol:10.3f} ms   {per} D^3 / 3 at {fp64_tflops:g} TFLOP/s: {cfloor:.3f} ms "
                 f"({t_chol / max(cfloor, 1e-9):.1f}x)")
    lines.append(f"  ridge_backsolve       {t_back:10.3f} ms")
    lines.append(f"  fit_native (wall)     {t_fit:10.3f} ms")
    try:
        free = torch.cuda.mem_get_info()[0]
        if N * D * 8 + S * D * D * 8 * 2 > free * 0.8:
            raise RuntimeError("the fp64 rows and systems do not fit the free device memory")
        Z = RD.working_rows(X, p["mean"], p["inv_std"]).double()
        T = RD.augment(Z[:, :1].float(), y, K)[:, 1:1 + K].double()

        def torch_form():
            G = Z.T @ Z
            M = G.unsqueeze(0) + p["alphas_t"].view(-1, 1, 1) * torch.eye(D, dtype=torch.float64, device=dev)
            L = torch.linalg.cholesky(M.repeat(F + 1, 1, 1))
            return torch.cholesky_solve((Z.T @ T).expand(L.shape[0], D, K), L)
        lines.append(f"  torch form (fp64)     {timed(torch_form, repeats):10.3f} ms   (Z.T @ Z, linalg.cholesky of {S} "
                     f"systems, cholesky_solve; no centring, no scoring)")
    except Exception as e:  # noqa: BLE001
        lines.append(f"  torch form: unavailable ({type(e).__name__}: {str(e)[:120]})")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "ridge_probe.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fp64-tflops", type=float, default=78.6)
    ap.add_argument("--shapes", default=None)
    a = ap.parse_args(argv)
    shapes = SHAPES if not a.shapes else [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    dev = torch.device("cuda:0")
    lines = [f"ridge probe on {torch.cuda.get_device_name(0)}: HIP-event medians of {a.repeats}"]
    for N, D in shapes:
        try:
            probe(N, D, dev, a.repeats, a.fp64_tflops, lines)
        except Exception as e:  # noqa: BLE001
            lines.append(f"{N} x {D}: not measured ({type(e).__name__}: {str(e)[:160]})")
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
