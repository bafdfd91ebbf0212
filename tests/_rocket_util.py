"""Shared inputs of the rocket tests: hand-built parameters, the real-valued cases and the near-tie rule."""
import functools

import torch

from har.ops.rocket import (N_KERNELS, RocketParams, _range_mask, fit_rocket_params, rocket_conv_torch,
                            rocket_dilations)

# the real-valued cases of tests/test_gpu_rocket.py: (n_windows, window, axes)
REAL_CASES = ((67, 200, 3), (5, 600, 6))


def hand_masks(window, axes):
    """int32 [n_dil, 84]: runs of 1..axes adjacent axes (cyclically), every subset size present at every dilation."""
    n_dil = len(rocket_dilations(window))
    m = torch.empty(n_dil, N_KERNELS, dtype=torch.int32)
    for e in range(n_dil):
        for k in range(N_KERNELS):
            size, first = 1 + (k + e) % axes, (k // axes) % axes
            m[e, k] = sum(1 << ((first + i) % axes) for i in range(size))
    return m


def hand_params(window, axes, q=3):
    """Half-integer biases spread over the range an integer stream in [-512, 512] reaches."""
    n_dil = len(rocket_dilations(window))
    k = torch.arange(N_KERNELS).view(1, -1, 1)
    e = torch.arange(n_dil).view(-1, 1, 1)
    i = torch.arange(q).view(1, 1, -1)
    b = ((k * 37 + e * 101 + i * 853) % 3001 - 1500).float() + 0.5
    return RocketParams(window, axes, hand_masks(window, axes), b)


def int_stream(n_windows, window, stride, axes, lo=-512, hi=512, seed=0, extra=3):
    g = torch.Generator().manual_seed(seed + 7919 * window + 31 * stride + axes)
    S = (n_windows - 1) * stride + window + extra     # `extra` samples past the last window: never read
    return torch.randint(lo, hi + 1, (S, axes), generator=g).float()


@functools.lru_cache(maxsize=None)
def real_case(n_windows, window, axes):
    """(Gaussian fp32 stream on the CPU, fitted parameters), stride == window."""
    g = torch.Generator().manual_seed(1000 * axes + window)
    s = torch.randn(n_windows * window, axes, generator=g)
    return s, fit_rocket_params(s, window, window, 1680, seed=5)


def gamma(axes):
    """Relative bound on the fp32 evaluation of C: at most 9 A + 4 roundings of 2^-24 each, doubled."""
    return 2.0 * (9 * axes + 4) * 2.0 ** -24


def ambiguity(stream, params, window, stride):
    """(count64, n_amb, n_counted), int64 [n_windows, F] each: the float64 counts, the number of counted
    positions with |C64[t] - b| <= gamma S[t] (S: the sum of |w_j x| over the taps and axes used), and the
    number of counted positions."""
    dev = stream.device
    C = rocket_conv_torch(stream, params, window, stride)                  # [n, n_dil * 84, W]
    S = rocket_conv_torch(stream, params, window, stride, absolute=True)
    b = params.on(dev)[1].double().view(-1, params.q)                      # [n_dil * 84, q]
    rng = torch.cat([_range_mask(e, d, window, dev) for e, d in enumerate(params.dilations)])   # [n_dil * 84, W]
    rng = rng[None, :, None, :]
    diff = C[:, :, None, :] - b[None, :, :, None]
    n = C.shape[0]
    count = ((diff > 0) & rng).sum(-1).reshape(n, -1)
    amb = ((diff.abs() <= gamma(stream.shape[1]) * S[:, :, None, :]) & rng).sum(-1).reshape(n, -1)
    counted = rng.expand(n, -1, params.q, -1).sum(-1).reshape(n, -1)
    return count, amb, counted
