"""Raw accelerometer ingest -> the WISDM *transformed* table, on the device.

The reference starts from WISDM's pre-windowed table (``Main/main.py:16-20``,
``wisdm_data.csv:1``: ``UID, USER, X0..Z9, XAVG.., XPEAK.., XABSDEV.., XSTDDEV..,
RESULTANT, ACTIVITY``).  The transform that produced it (Kwapisz et al. 2010: 10-s
windows, per axis 10-bin distribution / average / time between peaks / average
absolute deviation / standard deviation, average resultant) is not in the
reference.  This module runs it on raw samples so ``main.py --raw`` covers the whole
pipeline from sensor rows:

1. read ``user,activity,timestamp,x,y,z`` rows — a CSV with that header, or the
   WISDM v1.1 raw text layout (no header, ``;`` line terminators) — with the native
   host CSV parser;
2. segment the stream into maximal runs of one (user, activity) in file order, and
   place windows of ``round(hz * window_sec)`` samples every
   ``round(window * (1 - overlap))`` samples inside each run (a window never spans
   two users or activities);
3. featurize every window with the HIP window kernel (``window.hip``: LDS-staged
   samples, wave reductions), or its PyTorch oracle on the CPU; under
   ``torch.distributed`` each rank featurizes the windows that START in its
   contiguous shard of the samples, fetching the ``window - 1`` samples past its end
   from the next rank (``parallel.stream.exchange_halo``), and the rows are
   all-gathered;
4. emit the 46 WISDM columns with their names and types (``*PEAK`` as strings, ``?``
   when a window has fewer than two peaks — the missing marker of the original
   table), so ``features.wisdm.prepare`` and the rest of ``main.py`` run unchanged.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ..data.table import Column, Table
from .window import NBINS, window_features, window_features_torch

AXES = ("X", "Y", "Z")
WISDM43 = ([f"{a}{i}" for a in AXES for i in range(NBINS)] + [a + "AVG" for a in AXES] + [a + "PEAK" for a in AXES]
           + [a + "ABSDEV" for a in AXES] + [a + "STDDEV" for a in AXES] + ["RESULTANT"])
ACTIVITIES = ("Walking", "Jogging", "Upstairs", "Downstairs", "Sitting", "Standing")


def sample_cols(window: int):
    """Names of the raw-sample columns of ``raw_to_table(samples=True)``, time-major."""
    return [f"RAW{i}_{a}" for i in range(window) for a in AXES]


def read_raw(path: str):
    """(user int64 [S], activity object [S], timestamp int64 [S], xyz float32 [S, 3])."""
    from ..data.csv_io import parse_csv_bytes

    with open(path, "rb") as f:
        buf = f.read()
    first = buf.split(b"\n", 1)[0].strip().lower()
    header = first.startswith(b"user")
    if b";" in buf[:4096]:  # WISDM raw text: "33,Jogging,49105962326000,-0.69,12.68,0.50;"
        buf = buf.replace(b";", b"")
    t = parse_csv_bytes(buf, header=header)
    cols = t.columns
    if len(cols) < 6:
        raise ValueError(f"{path}: expected user,activity,timestamp,x,y,z columns, got {cols}")
    c = [t[n] for n in cols[:6]]
    ok = np.ones(t.count(), dtype=bool)
    for col in (c[0], c[2], c[3], c[4], c[5]):
        if col.kind == "string":
            raise ValueError(f"{path}: column {col.name} is not numeric")
        if col.missing is not None:
            ok &= ~col.missing
    xyz = np.stack([c[3].data, c[4].data, c[5].data], 1).astype(np.float32)
    ok &= np.isfinite(xyz).all(1)
    act = np.asarray([str(v) for v in c[1].data], dtype=object)
    return c[0].data.astype(np.int64)[ok], act[ok], c[2].data.astype(np.int64)[ok], xyz[ok]


def run_offsets(user: np.ndarray, activity: np.ndarray) -> np.ndarray:
    """int64 [runs + 1]: the first sample of every maximal run of one (user, activity) in file order, then the
    sample count (``[0]`` for an empty stream) — the segments of ``window_starts`` and of a stream filter."""
    n = len(user)
    if n == 0:
        return np.zeros(1, np.int64)
    _, acode = np.unique(activity.astype(str), return_inverse=True)
    change = np.ones(n, dtype=bool)
    change[1:] = (user[1:] != user[:-1]) | (acode[1:] != acode[:-1])
    return np.append(np.nonzero(change)[0], n).astype(np.int64)


def window_starts(user: np.ndarray, activity: np.ndarray, window: int, stride: int) -> Tuple[np.ndarray, np.ndarray]:
    """(start sample of every window, index of its segment's first sample); windows stay inside
    maximal runs of one (user, activity)."""
    n = len(user)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    off = run_offsets(user, activity)
    seg_lo, seg_hi = off[:-1], off[1:]
    nwin = np.where(seg_hi - seg_lo >= window, (seg_hi - seg_lo - window) // stride + 1, 0)
    seg_of = np.repeat(np.arange(len(seg_lo)), nwin)
    k = np.arange(int(nwin.sum())) - np.repeat(np.cumsum(nwin) - nwin, nwin)
    return seg_lo[seg_of] + k * stride, seg_lo[seg_of]


def featurize_starts(xyz: torch.Tensor, starts: torch.Tensor, window: int, hz: float) -> torch.Tensor:
    """[n, 43] WISDM features of the windows at ``starts`` (sample indices into ``xyz`` [S, 3])."""
    if starts.numel() == 0:
        return torch.zeros(0, len(WISDM43), dtype=torch.float32, device=xyz.device)
    idx = (starts.view(-1, 1) + torch.arange(window, device=xyz.device).view(1, -1)).reshape(-1)
    win = xyz.index_select(0, idx).contiguous()                 # windows back to back: stride == window
    f = window_features(win, window, window, hz) if win.is_cuda else window_features_torch(win, window, window, hz)
    return f[:, :len(WISDM43)]


def rocket_starts(xyz: torch.Tensor, starts: torch.Tensor, window: int, model) -> torch.Tensor:
    """[n, F] rocket features (``features.rocket.RocketModel``) of the windows at ``starts``: the same gather
    as ``featurize_starts``, the windows back to back."""
    if starts.numel() == 0:
        return torch.zeros(0, model.num_features, dtype=torch.float32, device=xyz.device)
    idx = (starts.view(-1, 1) + torch.arange(window, device=xyz.device).view(1, -1)).reshape(-1)
    return model.transform(xyz.index_select(0, idx).contiguous(), stride=window)


def fit_rocket(xyz_host: np.ndarray, starts: np.ndarray, hz: float, window_sec: float, overlap: float,
               num_features: int, seed: int = 2018):
    """Fit a ``RocketModel`` on ALL windows of the file (features only, never labels).  The fit runs on the
    host whatever the device and the rank count, so every rank and every device draw the same parameters."""
    from .rocket import RocketFeaturizer

    fz = RocketFeaturizer(hz=hz, seconds=window_sec, overlap=overlap, num_features=num_features, seed=seed)
    idx = (starts.reshape(-1, 1) + np.arange(fz.window).reshape(1, -1)).reshape(-1)
    model = fz.fit(torch.as_tensor(xyz_host[idx]))
    model.stride = fz.stride
    return model


def _featurize_dp(ctx, xyz_host: np.ndarray, starts: np.ndarray, window: int, hz: float, device,
                  rocket=None) -> torch.Tensor:
    """Rank r featurizes the windows starting in its contiguous sample shard; the last window of a
    shard may run into the next rank's samples: one halo exchange of window - 1 samples."""
    from ..parallel import comm
    from ..parallel.stream import exchange_halo, shard_lengths

    S = xyz_host.shape[0]
    lo, hi = (S * ctx.rank) // ctx.world_size, (S * (ctx.rank + 1)) // ctx.world_size
    local = torch.as_tensor(xyz_host[lo:hi]).to(device)
    lens = shard_lengths(ctx, local.shape[0], local.device)
    ext = torch.cat([local, exchange_halo(ctx, local, window - 1, lens)], 0)
    mine = starts[(starts >= lo) & (starts < hi)] - lo
    f = featurize_starts(ext, torch.as_tensor(mine, device=device), window, hz)
    if rocket is not None:
        f = torch.cat([f, rocket_starts(ext, torch.as_tensor(mine, device=device), window, rocket)], 1)
    counts = [int(((starts >= (S * r) // ctx.world_size) & (starts < (S * (r + 1)) // ctx.world_size)).sum())
              for r in range(ctx.world_size)]
    pad = torch.zeros(max(counts), f.shape[1], dtype=f.dtype, device=f.device)
    pad[: f.shape[0]] = f
    allf = torch.zeros(ctx.world_size * pad.shape[0], f.shape[1], dtype=f.dtype, device=f.device)
    comm.all_gather_into_tensor(allf, pad, group=ctx.group)
    allf = allf.view(ctx.world_size, -1, f.shape[1])
    return torch.cat([allf[r, :counts[r]] for r in range(ctx.world_size)], 0)


def raw_to_table(path: str, hz: float = 20.0, window_sec: float = 10.0, overlap: float = 0.0, device=None,
                 ctx=None, rocket=None, samples: bool = False, filter=None) -> Table:
    """Raw rows -> the WISDM transformed table (one row per window, columns of ``wisdm_data.csv:1``).

    ``rocket``: a feature count (a ``RocketModel`` is fitted on all windows of the file, see ``fit_rocket``) or
    a fitted ``RocketModel`` (serving); its ``RKT*`` double columns are appended and the model is returned as
    the table's ``rocket_model`` attribute.  ``None``: the table is exactly the WISDM one.

    ``samples``: append the samples of every window as ``RAW{i}_{X,Y,Z}`` double columns, time-major (sample i
    axis a is column ``3 i + a`` of them: the flattened window of ``ops/dtw.py``).

    ``filter``: a 3-axis ``features.filter.StreamFilter`` (``lowpass``, ``gravity``, ``body``, ``sos``) applied to
    the samples before the windows are placed, every (user, activity) run on its own; everything downstream —
    features, rocket columns, sample columns — then sees the filtered stream.  Under data parallelism every rank
    filters the whole stream before it is sharded.  The filtered samples come back to the host once (the rocket
    fit, the sample columns and the rank shards are cut from the host array) and are uploaded again for the
    featurizer: fine for a file that was parsed on the host anyway, a round trip a device-resident stream should
    avoid by calling ``StreamFilter.transform`` and the window kernels on the device tensor directly.  With
    ``device=None`` (or a CPU device) the filter is the per-sample PyTorch definition: exact, and slow on long runs."""
    user, act, ts, xyz = read_raw(path)
    if filter is not None:
        if filter.out_axes(len(AXES)) != len(AXES):
            raise ValueError(f"the WISDM table has three axes: a {filter.kind!r} filter does not fit (use lowpass, "
                             "gravity, body or sos)")
        fdev = torch.device(device) if device is not None else torch.device("cpu")
        if len(xyz):
            xyz = filter.transform(torch.as_tensor(xyz).to(fdev), torch.as_tensor(run_offsets(user, act))).cpu().numpy()
    window = int(round(hz * window_sec))
    stride = max(1, int(round(window * (1.0 - overlap))))
    if window < 3:
        raise ValueError("window must hold at least 3 samples")
    starts, _ = window_starts(user, act, window, stride)
    dev = torch.device(device) if device is not None else torch.device("cpu")
    if rocket is not None and not hasattr(rocket, "transform"):
        if len(starts) == 0:
            raise ValueError(f"{path}: no whole window to fit the rocket transform on")
        rocket = fit_rocket(xyz, starts, hz, window_sec, overlap, int(rocket))
    if rocket is not None and rocket.window != window:
        raise ValueError(f"the rocket model is for windows of {rocket.window} samples, not {window}")
    if ctx is not None and ctx.is_distributed:
        F = _featurize_dp(ctx, xyz, starts, window, hz, dev, rocket)
    else:
        xd, sd = torch.as_tensor(xyz).to(dev), torch.as_tensor(starts, device=dev)
        F = featurize_starts(xd, sd, window, hz)
        if rocket is not None:
            F = torch.cat([F, rocket_starts(xd, sd, window, rocket)], 1)
    F = F.double().cpu().numpy()
    n = len(starts)
    cols = [Column("UID", "int", np.arange(n, dtype=np.int64)), Column("USER", "int", user[starts])]
    for j, name in enumerate(WISDM43):
        if name.endswith("PEAK"):  # WISDM: integer milliseconds, '?' when < 2 peaks
            v = F[:, j]
            s = np.asarray(["?" if not np.isfinite(p) else str(int(round(p))) for p in v], dtype=object)
            cols.append(Column(name, "string", s))
        else:
            cols.append(Column(name, "double", F[:, j].copy()))
    cols.append(Column("ACTIVITY", "string", np.asarray(act[starts], dtype=object)))
    if rocket is not None:
        for j, name in enumerate(rocket.names):
            cols.append(Column(name, "double", F[:, len(WISDM43) + j].copy()))
    if samples:   # the same gather as ``featurize_starts``, on the host: windows back to back
        idx = (starts.reshape(-1, 1) + np.arange(window).reshape(1, -1)).reshape(-1)
        S = xyz[idx].reshape(n, window * len(AXES)).astype(np.float64)
        for j, name in enumerate(sample_cols(window)):
            cols.append(Column(name, "double", S[:, j].copy()))
    table = Table(cols)
    if rocket is not None:
        table.rocket_model = rocket
    return table


def write_synthetic_raw(path: str, n_windows: int = 400, users: int = 6, seed: int = 2018, hz: float = 20.0,
                        window_sec: float = 10.0, wisdm_txt: bool = False) -> dict:
    """A raw ``user,activity,timestamp,x,y,z`` file from the synthetic stream generator
    (``data.synth``: class-conditional dynamics, activity runs of 8 windows); activity runs are
    dealt to ``users`` round robin and every (user, activity) run is recorded contiguously."""
    from ..data.synth import StreamSpec, generate_stream

    spec = StreamSpec(num_classes=6, axes=3, hz=hz, window=int(round(hz * window_sec)), seed=seed)
    s, y = generate_stream(n_windows, spec)
    W = spec.window
    runs = np.arange(n_windows) // spec.run_windows
    user_of_window = 1 + runs % users
    rows = []
    step_ns = int(round(1e9 / hz))
    for w in range(n_windows):
        u, a = int(user_of_window[w]), ACTIVITIES[int(y[w])]
        for i in range(W):
            x0, x1, x2 = s[w * W + i].tolist()
            rows.append(f"{u},{a},{(w * W + i) * step_ns},{x0:.6g},{x1:.6g},{x2:.6g}")
    with open(path, "w") as f:
        if wisdm_txt:
            f.write(";\n".join(rows) + ";\n")
        else:
            f.write("user,activity,timestamp,x,y,z\n" + "\n".join(rows) + "\n")
    return {"samples": n_windows * W, "window": W, "labels": y.numpy()}
