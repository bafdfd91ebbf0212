"""Spectral feature kernel probe (HIP events, us per launch) on three shapes:
65,536 x 200 x 3 at stride 200, the same stream at stride 100 (131,071 windows) and 60k x 500 x 9.

Per shape: (a) the spectral kernel; (b) the same features with torch ops on the device — fp32
``torch.fft.rfft`` over the unfolded windows plus a torch epilogue, what one would write without the
kernel; (c) the time-feature kernel on the same stream, for scale.  Also the distance of (a) from the
fp32 matrix-core floor: rows x W x 2 (W // 2) x 2 flop at 157 TF.

Run once under a time limit, e.g. ``timeout 600 python tools/spectral_probe.py``."""
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from har.data.synth import StreamSpec, generate_stream  # noqa: E402
from har.features.spectral import NBANDS, spectral_features  # noqa: E402
from har.features.window import window_count, window_features  # noqa: E402

dev = torch.device("cuda:0")
PEAK_F32_MFMA = 157e12


def torch_spectral(s, W, stride, hz):
    """the features with library ops: rfft of every window, then the epilogue (fp32 throughout)"""
    x = s.unfold(0, W, stride)                                # [nw, A, W] view
    K = W // 2
    P = torch.fft.rfft(x, dim=-1)[..., 1:K + 1].abs().square()
    k = torch.arange(1, K + 1, device=s.device)
    onehot = torch.nn.functional.one_hot(((k - 1) * NBANDS) // K, NBANDS).float()
    f = k.float() * (hz / W)
    total = P.sum(-1)
    live = (x.max(-1).values > x.min(-1).values) & (total > 0)
    p = P / torch.where(live, total, torch.ones_like(total))[..., None]
    bands = p @ onehot
    dom = f[P.argmax(-1)]
    cen = p @ f
    ent = -torch.xlogy(p, p).sum(-1) / math.log(K)
    nw, A = total.shape
    row = torch.cat([bands.reshape(nw, A * NBANDS), dom, cen, ent], 1)
    mask = torch.cat([live[..., None].expand(nw, A, NBANDS).reshape(nw, A * NBANDS), live, live, live], 1)
    return torch.where(mask, row, torch.zeros_like(row))


def timed(fn, reps=10):
    """us per launch (HIP events around `reps` back-to-back calls, best of 3)"""
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    return best


s3, _ = generate_stream(65536, StreamSpec(), dev)
s9, _ = generate_stream(60000, StreamSpec(axes=9, window=500, hz=50.0), dev)
shapes = [(s3, 200, 200, 20.0), (s3, 200, 100, 20.0), (s9, 500, 500, 50.0)]

a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
t0 = time.time()
while time.time() - t0 < 0.5:  # steady clocks before the first timed launch
    for _ in range(20):
        a @ a
    torch.cuda.synchronize()

for s, W, stride, hz in shapes:
    A = s.shape[1]
    nw = window_count(s.shape[0], W, stride)
    got, ref = spectral_features(s, W, stride, hz), torch_spectral(s, W, stride, hz)
    nb = NBANDS * A
    err = float((got[:, :nb] - ref[:, :nb]).abs().max())
    us_k = timed(lambda: spectral_features(s, W, stride, hz))
    us_t = timed(lambda: torch_spectral(s, W, stride, hz), reps=3)
    us_w = timed(lambda: window_features(s, W, stride, hz))
    floor_us = nw * A * W * 2 * (W // 2) * 2 / PEAK_F32_MFMA * 1e6
    print(f"{nw} windows x {W} x {A} stride {stride}: spectral kernel {us_k:9.1f} us ({us_k / floor_us:.2f}x the "
          f"{floor_us:.0f} us fp32-MFMA floor) | torch rfft + epilogue {us_t:9.1f} us ({us_t / us_k:.1f}x) | "
          f"window kernel {us_w:8.1f} us | max |band fraction - torch| {err:.2e}")
torch.cuda.synchronize()
print("ok")
