"""Spectral window features (K22): layout, the float64 definition on hand-made windows, pivot
independence, short windows (K < 8), the combined featurizer and the sharded stream."""
import math
import os
import socket
import tempfile

import torch
import torch.multiprocessing as mp

from har.features.spectral import (NBANDS, n_spectral_features, spectral_feature_names, spectral_features,
                                   spectral_features_torch, spectral_power_torch)
from har.features.window import WindowFeaturizer, feature_names, n_features

NINE = ["AX", "AY", "AZ", "GX", "GY", "GZ", "MX", "MY", "MZ"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _stream(n=3001, seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g).cumsum(0) * 0.1


def _same(a, b):
    """bit-equal, NaN (``*PEAK`` below two peaks) matching NaN"""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_layout():
    assert NBANDS == 8 and n_spectral_features(3) == 33 and n_spectral_features(9) == 99
    names = spectral_feature_names()
    assert len(names) == 33
    assert names[:9] == [f"XBAND{b}" for b in range(8)] + ["YBAND0"]
    assert names[24:] == ["XDOMFREQ", "YDOMFREQ", "ZDOMFREQ", "XCENTROID", "YCENTROID", "ZCENTROID",
                          "XSPECENT", "YSPECENT", "ZSPECENT"]
    fz = WindowFeaturizer(spectral=True)
    assert fz.names == feature_names() + names and len(fz.names) == 28 * 3 + 4 == 88
    fz9 = WindowFeaturizer(spectral=True, axis_names=NINE)
    assert len(fz9.names) == 28 * 9 + 4 * 3 == 264 and fz9.names[n_features(9)] == "AXBAND0"
    assert WindowFeaturizer().names == feature_names()  # the default is unchanged


def _hand_window(W=40):
    t = torch.arange(W, dtype=torch.float64)
    x = torch.sin(2 * math.pi * t / 10)             # period 10 samples: bin 4 of 40, 2.0 Hz at 20 Hz
    y = torch.full((W,), 9.81, dtype=torch.float64)
    z = torch.zeros(W, dtype=torch.float64)
    z[0] = 1.0                                      # unit impulse: a flat spectrum
    return torch.stack([x, y, z], 1)


def test_definitions_on_one_window():
    W, hz, K = 40, 20.0, 20
    f = spectral_features_torch(_hand_window(W), W, W, hz)
    assert f.shape == (1, 33) and f.dtype == torch.float32
    f = f[0].double()
    bands = f[:24].reshape(3, 8)
    dom, cen, ent = f[24:27], f[27:30], f[30:33]
    # x: a pure tone in bin 4 -> band ((4 - 1) * 8) // 20 = 1
    assert float(dom[0]) == 2.0
    want = torch.zeros(8, dtype=torch.float64)
    want[1] = 1.0
    assert (bands[0] - want).abs().max() < 1e-6
    assert float(ent[0]) < 1e-6 and abs(float(cen[0]) - 2.0) < 1e-6
    # y: constant -> all 11 features are 0
    assert float(bands[1].abs().max()) == 0.0 and float(dom[1]) == 0.0 and float(cen[1]) == 0.0 and float(ent[1]) == 0.0
    # z: flat spectrum -> every band holds (its bins) / K of the energy, entropy 1, lowest bin dominant or tied
    k = torch.arange(1, K + 1)
    counts = torch.bincount(((k - 1) * 8) // K, minlength=8).double()
    assert (bands[2] - counts / K).abs().max() < 1e-6
    assert abs(float(ent[2]) - 1.0) < 1e-6
    assert abs(float(cen[2]) - float((k.double() * hz / W).mean())) < 1e-5
    P = spectral_power_torch(_hand_window(W), W, W)
    assert P.shape == (1, 3, K) and P.dtype == torch.float64
    assert (P[0, 2] - 1.0).abs().max() < 1e-12 and int(P[0, 0].argmax()) == 3


def test_pivot_independence():
    g = torch.Generator().manual_seed(0)
    s = torch.randn(400, 3, generator=g, dtype=torch.float64).cumsum(0) * 0.1
    a = spectral_features_torch(s, 97, 31, 50.0)
    b = spectral_features_torch(s + 1000.0, 97, 31, 50.0)
    assert a.shape == b.shape and a.shape[0] > 5
    assert float((a.double() - b.double()).abs().max()) <= 1e-6


def test_short_windows():
    g = torch.Generator().manual_seed(1)
    s = torch.randn(40, 3, generator=g, dtype=torch.float64)
    # W = 5: K = 2, bins 1, 2 -> bands 0 and 4; every other band is empty
    f = spectral_features_torch(s, 5, 2, 20.0).double()
    bands = f[:, :24].reshape(-1, 3, 8)
    assert float(bands[..., [1, 2, 3, 5, 6, 7]].abs().max()) == 0.0
    assert ((bands[..., 0] + bands[..., 4]) - 1.0).abs().max() < 1e-6
    assert bool(((f[:, 24:27] - 4.0).abs() < 1e-6).logical_or((f[:, 24:27] - 8.0).abs() < 1e-6).all())
    assert float(f[:, 30:33].min()) >= 0.0 and float(f[:, 30:33].max()) <= 1.0 + 1e-6
    # W = 3: K = 1 -> all energy in band 0, dominant = centroid = hz / 3, entropy 0
    f = spectral_features_torch(s, 3, 1, 20.0).double()
    bands = f[:, :24].reshape(-1, 3, 8)
    assert (bands[..., 0] - 1.0).abs().max() < 1e-6 and float(bands[..., 1:].abs().max()) == 0.0
    assert (f[:, 24:30] - 20.0 / 3).abs().max() < 1e-5
    assert float(f[:, 30:33].abs().max()) == 0.0


def test_cpu_front_end_and_combined_rows():
    s = _stream(1200)
    assert torch.equal(spectral_features(s, 200, 100, 20.0), spectral_features_torch(s, 200, 100, 20.0))
    fz = WindowFeaturizer(hz=20.0, seconds=10.0, overlap=0.5, spectral=True)
    rows = fz.transform(s)
    assert rows.shape == (11, 88)
    assert torch.equal(rows[:, 55:], spectral_features_torch(s, 200, 100, 20.0))
    assert _same(rows[:, :55], WindowFeaturizer(hz=20.0, seconds=10.0, overlap=0.5).transform(s))


def test_combined_mlp_rows_cpu():
    from har.features.window import window_features_mlp, window_spectral_features_mlp

    s = _stream(1200)
    g = torch.Generator().manual_seed(2)
    mean, inv_std = torch.randn(88, generator=g), torch.rand(88, generator=g) + 0.5
    rows = window_spectral_features_mlp(s, 200, 100, 20.0, mean, inv_std, 96)
    assert rows.shape == (11, 96) and rows.dtype == torch.bfloat16
    assert torch.count_nonzero(rows[:, 88:]) == 0
    assert torch.equal(rows[:, :55], window_features_mlp(s, 200, 100, 20.0, mean[:55], inv_std[:55], 64)[:, :55])
    want = ((spectral_features_torch(s, 200, 100, 20.0) - mean[55:]) * inv_std[55:]).to(torch.bfloat16)
    assert torch.equal(rows[:, 55:88], want)


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from har.parallel import dist as hd
    from har.parallel.stream import sharded_window_features

    ctx = hd.init(device="cpu")
    S = _stream()
    cut = 1555  # not on a window / stride boundary: windows straddle the cut, both shards longer than the halo
    local = S[:cut] if rank == 0 else S[cut:]
    fz = WindowFeaturizer(hz=20.0, seconds=10.0, overlap=0.5, spectral=True)
    feats, first = sharded_window_features(ctx, local, fz)
    torch.save((feats, first), os.path.join(out_dir, f"spec_{rank}.pt"))
    hd.shutdown(ctx)


def test_sharded_combined_rows_equal_single():
    """gloo, world 2: the combined [time | spectral] rows of a 50%-overlap featurizer over two shards equal
    the single-process rows exactly, windows that straddle the cut included."""
    d = tempfile.mkdtemp()
    mp.spawn(_worker, args=(2, _free_port(), d), nprocs=2, join=True)
    outs = [torch.load(os.path.join(d, f"spec_{r}.pt"), weights_only=True) for r in range(2)]
    full = WindowFeaturizer(hz=20.0, seconds=10.0, overlap=0.5, spectral=True).transform(_stream())
    (f0, first0), (f1, first1) = outs
    assert first0 == 0 and first1 == f0.shape[0] and f0.shape[1] == f1.shape[1] == 88
    # rank 0 owns the windows starting before the cut: those from 1400 and 1500 run into rank 1's samples
    assert f0.shape[0] == 16 and f0.shape[0] + f1.shape[0] == full.shape[0] == 29
    got = torch.cat([f0, f1])
    assert torch.equal(got[:, 55:], full[:, 55:])
    assert _same(got, full)
