"""Shared by the StreamFilter tests: the kernels' algorithm restated in numpy fp64, the exact-arithmetic probes
and the real-valued designs.  Nothing here runs the code under test except ``state_space`` (the cascade's
transition matrix, which the kernel front-end uses too)."""
import numpy as np
import torch

from har.ops import sosfilt as F

# user sections whose arithmetic is exact in fp64 on integer inputs in [-8, 8] with init="zero":
# name -> (sections, longest segment the outputs stay below 2^24 for; None = any)
EXACT_PROBES = {
    "delay4": ([[0, 0, 1, 1, 0, 0], [0, 0, 1, 1, 0, 0]], None),
    "fir_into_sum": ([[1, -2, 3, 1, 0, 0], [2, 0, -1, 1, -1, 0]], None),
    "running_sum": ([[1, 0, 0, 1, -1, 0]], None),
    "double_sum": ([[1, 0, 0, 1, -2, 1]], 1000),
}

# (btype, order, cutoff Hz, hz)
REAL_DESIGNS = [("low", 3, 0.3, 20.0), ("low", 3, 0.3, 100.0), ("low", 3, 20.0, 50.0), ("high", 4, 0.3, 100.0)]


# The 8th-order 0.25 Hz / 200 Hz Butterworth low pass as second-order sections, written out (the values
# ``scipy.signal.butter(8, 0.25, "low", fs=200.0, output="sos")`` returns): powers of its transition matrix reach
# about 1e16, so the conditioning guard must refuse it.
ORDER8_SOS = [
    [5.54312871217679e-20, 1.108625742435358e-19, 5.54312871217679e-20, 1.0, -1.9846505710226259, 0.9847117842084645],
    [1.0, 2.0, 1.0, 1.0, -1.9869628914041506, 0.9870241759095955],
    [1.0, 2.0, 1.0, 1.0, -1.9912497091584618, 0.9913111258835405],
    [1.0, 2.0, 1.0, 1.0, -1.996878657765821, 0.9969402481062868],
]


def probe_sos(name):
    return torch.tensor(EXACT_PROBES[name][0], dtype=torch.float64)


def int_stream(S, A, seed):
    rng = np.random.default_rng(seed)
    return torch.as_tensor(rng.integers(-8, 9, size=(S, A)).astype(np.float32))


def real_stream(S, A, seed):
    """9.8 + 3 N(0, 1): a signal riding on gravity."""
    g = torch.Generator().manual_seed(seed)
    return (9.8 + 3.0 * torch.randn(S, A, generator=g, dtype=torch.float64)).float()


def offsets(starts, S):
    """int64 [0, ..., S] from any collection of start positions (0 added, duplicates and out-of-range dropped)."""
    s = sorted({0, *[int(v) for v in starts if 0 < int(v) < S]})
    return torch.tensor(s + [S], dtype=torch.int64)


def chunked_state_space(x, sos, seg_offsets=None, init="step", reverse=False, L=64):
    """fp64 numpy [S, A]: the chunked evaluation — every chunk of L samples (in scan order) from a zero state, the
    incoming state of chunk c + 1 as ``M^L z_in(c) + u(c)`` (or ``u(c)`` alone when a segment starts inside chunk
    c), then every chunk again from its incoming state.  All chunks advance together, one sample per step."""
    x = np.asarray(x, dtype=np.float64)
    S, A = x.shape
    off = np.array([0, S]) if seg_offsets is None else np.asarray(seg_offsets, dtype=np.int64)
    s = torch.as_tensor(sos, dtype=torch.float64).numpy()
    ns = s.shape[0]
    zi = F.sos_zi(sos).numpy() if init == "step" else np.zeros((ns, 2))
    starts = off[:-1]
    if reverse:
        x, starts = x[::-1], S - off[1:][::-1]
    C = -(-S // L)
    xp = np.zeros((C * L, A))
    xp[:S] = x
    xp = xp.reshape(C, L, A)
    is_start = np.zeros(C * L, dtype=bool)
    is_start[starts] = True
    is_start = is_start.reshape(C, L)
    P = np.linalg.matrix_power(F.state_space(sos)[0], L)

    def run(z):
        z = z.copy()
        y = np.empty((C, L, A))
        for i in range(L):
            v = xp[:, i, :]
            st = is_start[:, i]
            if st.any():
                for j in range(ns):
                    z[st, :, 2 * j] = zi[j, 0] * v[st]
                    z[st, :, 2 * j + 1] = zi[j, 1] * v[st]
            for j in range(ns):
                b0, b1, b2, _, a1, a2 = s[j]
                w = b0 * v + z[:, :, 2 * j]
                z[:, :, 2 * j] = (b1 * v - a1 * w) + z[:, :, 2 * j + 1]
                z[:, :, 2 * j + 1] = b2 * v - a2 * w
                v = w
            y[:, i, :] = v
        return y, z

    _, u = run(np.zeros((C, A, 2 * ns)))
    reset = is_start.any(1)
    zin = np.zeros((C, A, 2 * ns))
    for c in range(1, C):
        zin[c] = u[c - 1] if reset[c - 1] else zin[c - 1] @ P.T + u[c - 1]
    y = run(zin)[0].reshape(C * L, A)[:S]
    return y[::-1].copy() if reverse else y


def flip_segments(x, off):
    """Every segment of a host tensor reversed in place of itself."""
    out = x.clone()
    o = off.tolist()
    for a, b in zip(o[:-1], o[1:]):
        out[a:b] = x[a:b].flip(0)
    return out
