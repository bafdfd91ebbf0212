#!/usr/bin/env python3
"""Per-iteration time of the Gaussian-mixture kernels against the PyTorch definitions on the same device.

For every shape, one EM iteration = ``gmm_estep`` (Mahalanobis products, softmax, moment slabs, log-likelihood
partials) + ``gmm_finish`` + ``gmm_control``; ``--iters`` iterations are enqueued back to back between two
HIP events (tolerance 0: the fit does not freeze), after a warm-up run, and the median of ``--repeats`` runs
is reported.  The kernel loop runs under ``torch.cuda.set_sync_debug_mode("error")``: any device -> host read
inside it would raise.  The same loop then runs on the torch definitions of ``har/ops/gmm.py`` (fp64, as
the oracle evaluates; their control step reads its two state words on the host, as the CPU path does).
Sets no bar.

    python tools/gmm_probe.py [--out profiles/r13/gmm_probe.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from har.ops import gmm as GM  # noqa: E402

SHAPES = [(65536, 43, 6), (1000000, 43, 16), (65536, 128, 32)]


def problem(N, D, K, dev):
    g = torch.Generator().manual_seed(N + D + K)
    mu = torch.randn(max(K, 2), D, generator=g) * 3.0
    c = torch.randint(0, mu.shape[0], (N,), generator=g)
    X = (mu[c] + torch.randn(N, D, generator=g)).to(dev)
    mean, _, inv = GM.standardizer(X)
    Z = GM.working_rows(X, mean, inv)
    return Z, Z[torch.randperm(N, generator=g)[:K].to(dev)].contiguous()


def em_ms(Z, mu0, native, iters, guard):
    K, D = mu0.shape
    dev = Z.device
    pi0 = torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev)
    st = GM.FitState.alloc(mu0, torch.eye(D, device=dev).expand(K, D, D),
                           GM.component_c(pi0, torch.zeros(K, dtype=torch.float64, device=dev), D), pi0, iters)
    G = GM.grid(Z.shape[0], D, K)
    slabs = torch.empty(G, K, GM.slab_size(D), dtype=torch.float32, device=dev)
    part = torch.zeros(G, dtype=torch.float64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if guard:
        torch.cuda.set_sync_debug_mode("error")
    try:
        e0.record()
        for _ in range(iters):
            if native:
                GM.step_native(st, Z, None, 1e-6, False, 0.0, iters, slabs, part)
            else:
                GM.step_torch(st, Z, None, 1e-6, False, 0.0, iters)
        e1.record()
    finally:
        if guard:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    it = int(st.state[0])
    return e0.elapsed_time(e1) / iters, float(st.hist[it - 1])


def timed(fn, repeats):
    fn()  # warm-up: code objects, allocator
    out = [fn() for _ in range(repeats)]
    return statistics.median(v[0] for v in out), out[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "gmm_probe.txt"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"Gaussian-mixture probe: {a.iters} iterations per run, median of {a.repeats} runs after a warm-up run, "
             f"device {torch.cuda.get_device_name(0)}",
             "kernel loops ran under torch.cuda.set_sync_debug_mode('error'): no device -> host read between the "
             "first and the last launch",
             "no counter run was made: what binds gmm_estep (LDS reads, the slab read-modify-write or the matrix "
             "cores) is unmeasured"]
    for N, D, K in SHAPES:
        Z, mu0 = problem(N, D, K, dev)
        k_ms, k_ll = timed(lambda: em_ms(Z, mu0, True, a.iters, True), a.repeats)
        t_ms, t_ll = timed(lambda: em_ms(Z, mu0, False, a.iters, False), a.repeats)
        lines.append(f"{N} x {D}, K = {K} ({GM.grid(N, D, K)} workgroups / slabs of {GM.slab_size(D) * K * 4} B):")
        lines.append(f"  E-step + finish + control per iteration: kernels {k_ms * 1e3:10.1f} us   torch definitions (fp64) "
                     f"{t_ms * 1e3:11.1f} us   ratio {t_ms / k_ms:6.1f}x   (log-likelihood after {a.iters}: "
                     f"{k_ll:.6e} / {t_ll:.6e})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
