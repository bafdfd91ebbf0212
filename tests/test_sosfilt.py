"""StreamFilter on the CPU: the Butterworth designer against its closed-form response and scipy, the definition
(``har.ops.sosfilt``) against ``scipy.signal``, segments, the chunked restatement of the kernels' algorithm
(``_sosfilt_util.chunked_state_space``) against the definition, the conditioning guard, and the command lines."""
import csv
import math

import numpy as np
import pytest
import torch

from _sosfilt_util import (EXACT_PROBES, ORDER8_SOS, REAL_DESIGNS, chunked_state_space, flip_segments, int_stream, offsets, probe_sos,
                           real_stream)
from har.features.filter import StreamFilter
from har.ops import sosfilt as F


def _response(sos, f, hz):
    z1 = np.exp(-2j * np.pi * f / hz)
    h = 1.0 + 0j
    for b0, b1, b2, _, a1, a2 in sos.tolist():
        h *= (b0 + b1 * z1 + b2 * z1 * z1) / (1.0 + a1 * z1 + a2 * z1 * z1)
    return abs(h)


def _polys(sos):
    b, a = np.array([1.0]), np.array([1.0])
    for r in sos.numpy():
        b, a = np.polymul(b, np.trim_zeros(r[:3], "b")), np.polymul(a, np.trim_zeros(r[3:], "b"))
    return b, a


# ------------------------------------------------------------------ 1. the designer
@pytest.mark.parametrize("btype", ["low", "high"])
def test_butter_sos_closed_form_response(btype):
    for n in (1, 2, 3, 4):
        for fc in (0.3, 2.0, 5.0):
            for hz in (20.0, 50.0):
                sos = F.butter_sos(n, fc, hz, btype)
                assert sos.dtype == torch.float64 and tuple(sos.shape) == ((n + 1) // 2, 6)
                assert bool((sos[:, 3] == 1).all())
                if n % 2:
                    assert sos[0, 2] == 0 and sos[0, 5] == 0            # the first-order section
                for frac in (0.03, 0.2, 0.45, 0.7, 0.9):                 # of the Nyquist frequency
                    f = frac * hz / 2
                    ratio = math.tan(math.pi * f / hz) / math.tan(math.pi * fc / hz)
                    if btype == "high":
                        ratio = 1.0 / ratio
                    want = 1.0 / math.sqrt(1.0 + ratio ** (2 * n))
                    assert _response(sos, f, hz) == pytest.approx(want, rel=1e-12), (n, fc, hz, frac)


def test_butter_sos_arguments():
    for bad in (dict(order=0), dict(order=5), dict(cutoff_hz=0.0), dict(cutoff_hz=10.0), dict(btype="band")):
        kw = dict(order=3, cutoff_hz=0.3, hz=20.0, btype="low")
        kw.update(bad)
        with pytest.raises(ValueError):
            F.butter_sos(**kw)


def test_butter_sos_against_scipy():
    sg = pytest.importorskip("scipy.signal")
    for btype in ("low", "high"):
        for n in (1, 2, 3, 4):
            for fc, hz in ((0.3, 20.0), (0.3, 100.0), (5.0, 50.0), (20.0, 50.0)):
                b, a = _polys(F.butter_sos(n, fc, hz, btype))
                wb, wa = sg.butter(n, fc, btype, fs=hz)
                np.testing.assert_allclose(b, wb, rtol=1e-10, atol=0)
                np.testing.assert_allclose(a, wa, rtol=1e-10, atol=0)


# ------------------------------------------------------------------ 2. the definition against scipy
def test_zi_and_definition_against_scipy():
    sg = pytest.importorskip("scipy.signal")
    x = real_stream(3000, 3, 1)
    x64 = x.double().numpy()
    for btype, n, fc, hz in REAL_DESIGNS + [("low", 4, 2.0, 20.0)]:
        sos = F.butter_sos(n, fc, hz, btype)
        got_zi, want_zi = F.sos_zi(sos).numpy(), sg.sosfilt_zi(sos.numpy())
        nz = want_zi != 0
        np.testing.assert_allclose(got_zi[nz], want_zi[nz], rtol=1e-12, atol=0)
        # zero states in scipy (the s2 of a first-order section; every section after the first of a high pass, whose
        # DC gain is zero): a relative bound says nothing there, one rounding of the largest coefficient is the
        # absolute one
        assert np.abs(got_zi[~nz]).max(initial=0.0) <= 2.0 ** -52 * float(sos.abs().max())
        assert bool(nz[0, 0]) and (btype == "low" or not bool(nz[1:].any()))
        y = F.sosfilt_torch(x, sos, None, "zero", out_dtype=torch.float64).numpy()
        want = sg.sosfilt(sos.numpy(), x64, axis=0)
        assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
        zi = sg.sosfilt_zi(sos.numpy())[:, :, None] * x64[0][None, None, :]
        want, _ = sg.sosfilt(sos.numpy(), x64, axis=0, zi=zi)
        y = F.sosfilt_torch(x, sos, None, "step", out_dtype=torch.float64).numpy()
        assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
        yy = F.sosfiltfilt_torch(x, sos).double().numpy()
        want = sg.sosfiltfilt(sos.numpy(), x64, axis=0, padtype=None, padlen=0)
        assert np.abs(yy - want).max() <= 2.0 ** -22 * np.abs(want).max()


def test_definition_output_type_and_empty():
    sos = F.butter_sos(3, 0.3, 20.0)
    x = real_stream(50, 2, 2)
    y = F.sosfilt_torch(x, sos)
    assert y.dtype == torch.float32 and tuple(y.shape) == (50, 2)
    assert torch.equal(y, F.sosfilt_torch(x, sos, out_dtype=torch.float64).float())
    assert tuple(F.sosfilt(x[:0], sos).shape) == (0, 2) and tuple(F.sosfilt(x[:0], sos, mode="split").shape) == (0, 4)


def test_no_start_up_transient_on_a_constant():
    c = torch.full((400, 3), 9.81, dtype=torch.float32) * torch.tensor([1.0, -0.5, 0.02])
    off = offsets([1, 57, 58, 200], 400)
    for hz in (20.0, 100.0):
        assert torch.equal(StreamFilter(hz, "gravity").transform(c, off), c)
        assert bool((StreamFilter(hz, "body").transform(c, off) == 0).all())
        z = StreamFilter(hz, "split", zero_phase=True).transform(c, off)
        assert torch.equal(z[:, 3:], c) and bool((z[:, :3] == 0).all())
    y = F.sosfilt_torch(c, F.butter_sos(3, 0.3, 20.0), None, "zero")
    assert float((y[0] - c[0]).abs().max()) > 1.0                              # what init="step" removes


# ------------------------------------------------------------------ 3. segments and direction
@pytest.mark.parametrize("init", ["step", "zero"])
def test_segments_equal_pieces(init):
    x = real_stream(700, 3, 3)
    off = offsets([1, 2, 64, 65, 300, 699], 700)
    sos = F.butter_sos(3, 0.3, 20.0)
    for reverse in (False, True):
        got = F.sosfilt_torch(x, sos, off, init, reverse)
        o = off.tolist()
        want = torch.cat([F.sosfilt_torch(x[a:b], sos, None, init, reverse) for a, b in zip(o[:-1], o[1:])], 0)
        assert torch.equal(got, want)
    got = F.sosfiltfilt_torch(x, sos, off)
    o = off.tolist()
    assert torch.equal(got, torch.cat([F.sosfiltfilt_torch(x[a:b], sos) for a, b in zip(o[:-1], o[1:])], 0))


def test_reverse_is_the_flipped_forward_pass():
    x = real_stream(300, 2, 4)
    off = offsets([100, 101, 250], 300)
    sos = F.butter_sos(2, 2.0, 20.0, "high")
    want = flip_segments(F.sosfilt_torch(flip_segments(x, off), sos, off, "step"), off)
    assert torch.equal(F.sosfilt_torch(x, sos, off, "step", True), want)


def test_seg_offsets_are_validated():
    x = real_stream(10, 1, 5)
    sos = F.butter_sos(1, 1.0, 20.0)
    for bad in ([0, 5], [1, 10], [0, 5, 5, 10], [0, 7, 5, 10]):
        with pytest.raises(ValueError):
            F.sosfilt_torch(x, sos, torch.tensor(bad, dtype=torch.int64))
    with pytest.raises(ValueError):
        F.sosfilt_torch(x, sos, torch.tensor([0, 10], dtype=torch.int32))
    with pytest.raises(ValueError):
        F.sosfilt_torch(x, sos, None, "ramp")


# ------------------------------------------------------------------ 4. the chunked form
@pytest.mark.parametrize("name", sorted(EXACT_PROBES))
def test_chunked_form_is_exact_on_the_probes(name):
    sos = probe_sos(name)
    limit = EXACT_PROBES[name][1]
    S = 3 * 64 + 5 if limit else 2500
    x = int_stream(S, 3, 6)
    off = offsets([1, 63, 64, 65, 70, 71, 128], S) if limit else offsets([700, 701], S)
    for reverse in (False, True):
        want = F.sosfilt_torch(x, sos, off, "zero", reverse, out_dtype=torch.float64)
        assert float(want.abs().max()) < 2.0 ** 24
        for L in (8, 64):
            got = torch.from_numpy(chunked_state_space(x, sos, off, "zero", reverse, L))
            assert torch.equal(got, want)


def test_chunked_form_on_real_data():
    """Two fp64 evaluation orders differ by d (printed; 1e-14 .. 3e-11 here), far below half an fp32 ulp of the
    signal, so their fp32 roundings agree — except where a value lies within d of a rounding boundary (d / ulp is
    about 1e-4 per value for the worst design: 7 of 90,000 values here, at most one in 5,000 is allowed), and there
    they are neighbours."""
    x = real_stream(3000, 3, 7)
    off = offsets([1000, 1001, 2100], 3000)
    flips = total = 0
    for btype, n, fc, hz in REAL_DESIGNS + [("low", 4, 2.0, 20.0)]:
        sos = F.butter_sos(n, fc, hz, btype)
        for o in (None, off):
            want = F.sosfilt_torch(x, sos, o, "step", out_dtype=torch.float64)
            got = torch.from_numpy(chunked_state_space(x, sos, o, "step", False, 64))
            d = float((got - want).abs().max())
            print(f"{btype} {n} at {fc} / {hz}: max |chunked - sequential| = {d:.3g}")
            assert d <= 2.0 ** -27 * float(want.abs().max())
            g32, w32 = got.float(), want.float()
            ne = g32 != w32
            flips, total = flips + int(ne.sum()), total + ne.numel()
            if bool(ne.any()):  # neighbours, and the fp64 value sits on the boundary between them
                assert bool((torch.nextafter(torch.minimum(g32, w32), torch.maximum(g32, w32))[ne]
                             == torch.maximum(g32, w32)[ne]).all())
                mid = (g32.double() + w32.double()) / 2
                assert bool(((want - mid).abs()[ne] <= d).all())
    print(f"fp32 roundings that differ: {flips} of {total}")
    assert flips <= total // 5000


def test_state_space_is_the_cascade():
    sos = F.butter_sos(4, 2.0, 20.0)
    M, v, c, d = F.state_space(sos)
    assert M.shape == (4, 4)
    x = real_stream(200, 1, 8)
    z = np.zeros(4)
    y = np.empty(200)
    for t in range(200):
        y[t] = c @ z + d * float(x[t, 0])
        z = M @ z + v * float(x[t, 0])
    want = F.sosfilt_torch(x, sos, None, "zero", out_dtype=torch.float64)[:, 0].numpy()
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------ 5. limits
def test_guard_refuses_an_order_8_design():
    x = real_stream(16, 3, 9)
    s8 = torch.tensor(ORDER8_SOS, dtype=torch.float64)
    assert F.power_growth(s8) > 2.0 ** 20
    with pytest.raises(ValueError, match="ill-conditioned"):
        F.check_range(x, s8)
    with pytest.raises(ValueError, match="ill-conditioned"):
        F.sosfilt(x, s8)
    with pytest.raises(ValueError, match="ill-conditioned"):
        StreamFilter(200.0, "sos", sos=s8)
    assert F.power_growth(F.butter_sos(3, 0.3, 100.0)) < 2.0 ** 20


def test_range_limits():
    sos = F.butter_sos(3, 0.3, 20.0)
    with pytest.raises(ValueError, match="axes"):
        F.sosfilt(torch.zeros(4, 10), sos)
    with pytest.raises(ValueError, match="fp32"):
        F.sosfilt(torch.zeros(4, 3, dtype=torch.float64), sos)
    with pytest.raises(ValueError, match="sections"):
        F.sosfilt(torch.zeros(4, 3), torch.cat([sos, sos, sos]))
    bad = sos.clone()
    bad[0, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        F.sosfilt(torch.zeros(4, 3), bad)
    with pytest.raises(ValueError, match="samples"):
        F.check_range(torch.zeros(1, 3).expand(F.MAX_SAMPLES, 3), sos)               # a stride-0 view: no memory
    with pytest.raises(ValueError, match="mode"):
        F.sosfilt(torch.zeros(4, 3), sos, mode="both")


# ------------------------------------------------------------------ 6. the front-end
def test_stream_filter_kinds_and_persistence(tmp_path):
    from har.utils import persist

    x = real_stream(500, 3, 10)
    grav = StreamFilter(20.0, "gravity")
    assert grav.cutoff == 0.3 and StreamFilter(20.0, "lowpass").cutoff == 5.0
    g = grav.transform(x)
    assert torch.equal(g, F.sosfilt_torch(x, F.butter_sos(3, 0.3, 20.0)))
    assert torch.equal(StreamFilter(20.0, "body").transform(x), x - g)
    sp = StreamFilter(20.0, "split")
    assert sp.out_axes(3) == 6 and torch.equal(sp.transform(x), torch.cat([x - g, g], 1))
    assert sp.names() == ["BODY_X", "BODY_Y", "BODY_Z", "GRAV_X", "GRAV_Y", "GRAV_Z"]
    assert grav.names(("a", "b")) == ["GRAV_a", "GRAV_b"] and StreamFilter(20.0, "lowpass").names() == ["X", "Y", "Z"]
    user = StreamFilter(20.0, "sos", sos=F.butter_sos(2, 1.0, 20.0, "high"), init="zero")
    assert torch.equal(user.transform(x), F.sosfilt_torch(x, user.sos, None, "zero"))
    zp = StreamFilter(20.0, "body", cutoff=0.5, order=2, zero_phase=True)
    assert torch.equal(zp.transform(x), x - F.sosfiltfilt_torch(x, F.butter_sos(2, 0.5, 20.0)))
    for f in (grav, sp, user, zp):
        persist.save(f, str(tmp_path / f.uid))
        r = persist.load(str(tmp_path / f.uid))
        assert isinstance(r, StreamFilter) and r.kind == f.kind and r.zero_phase == f.zero_phase and r.init == f.init
        assert r.sos.dtype == torch.float64 and torch.equal(r.sos, f.sos)           # the same coefficient bits
        assert torch.equal(r.transform(x), f.transform(x))
        st = f.to_state()
        assert torch.equal(StreamFilter.from_state(st, st).sos, f.sos)
    with pytest.raises(ValueError):
        StreamFilter(20.0, "bandpass")
    with pytest.raises(ValueError):
        StreamFilter(20.0, "sos")


# ------------------------------------------------------------------ 7. the table and the command lines
def test_raw_table_filter_and_cli_end_to_end(tmp_path):
    import main
    import predict
    from har.features.raw import ACTIVITIES, featurize_starts, raw_to_table, read_raw, run_offsets, window_starts, write_synthetic_raw

    p = str(tmp_path / "raw.csv")
    info = write_synthetic_raw(p, n_windows=96, users=4, hz=10.0, window_sec=4.0)
    W = info["window"]
    user, act, _, xyz = read_raw(p)
    off = run_offsets(user, act)
    assert off[0] == 0 and off[-1] == len(user) and len(off) - 1 == 96 // 8
    plain = raw_to_table(p, hz=10.0, window_sec=4.0)
    body = StreamFilter(10.0, "body")
    t = raw_to_table(p, hz=10.0, window_sec=4.0, filter=body)
    assert t.columns == plain.columns and t.count() == plain.count() == 96
    starts, _ = window_starts(user, act, W, W)
    want = featurize_starts(body.transform(torch.as_tensor(xyz), torch.as_tensor(off)), torch.as_tensor(starts), W, 10.0)
    assert np.array_equal(np.asarray(t["XAVG"].data), want[:, 30].double().numpy())
    assert float(np.abs(np.asarray(t["XAVG"].data)).max()) < float(np.abs(np.asarray(plain["XAVG"].data)).max())
    with pytest.raises(ValueError, match="three axes"):
        raw_to_table(p, hz=10.0, window_sec=4.0, filter=StreamFilter(10.0, "split"))

    for argv in (["--filter", "body"], ["--filter-cutoff", "1"], ["--filter-zero-phase"], ["--filter-order", "2"]):
        with pytest.raises(SystemExit):
            main.config_from_args(argv)                                            # an error without --raw
    with pytest.raises(SystemExit):
        main.config_from_args(["--raw", p, "--filter", "split"])
    for argv in (["--filter-zero-phase"], ["--filter", "body", "--filter-order", "5"],
                 ["--filter", "body", "--filter-cutoff", "5"]):                    # no kind; order and cutoff (hz / 2) out of range
        with pytest.raises(SystemExit):
            main.config_from_args(["--raw", p, "--hz", "10"] + argv)
    c = main.config_from_args(["--raw", p, "--filter", "gravity", "--filter-zero-phase", "--filter-order", "2",
                               "--filter-cutoff", "0.4"])
    assert (c.filter, c.filter_zero_phase, c.filter_order, c.filter_cutoff) == ("gravity", True, 2, 0.4)
    c = main.config_from_args(["--raw", p])
    assert (c.filter, c.filter_zero_phase, c.filter_order, c.filter_cutoff) == ("", False, 3, 0.0)
    base = ["--raw", p, "--hz", "10", "--window-sec", "4", "--classifiers", "lr", "--encoding", "numeric43", "--device", "cpu"]
    out0, m0 = tmp_path / "out0", tmp_path / "models0"
    s0 = main.run(main.config_from_args(base + ["--out-dir", str(out0), "--save-models", str(m0)]))
    assert not (m0 / "filter").exists() and "conditioned" not in (out0 / "result.txt").read_text()
    assert sorted(q.name for q in m0.iterdir()) == ["lr", "pipeline"]               # the artefacts it wrote before
    out, mdir = tmp_path / "out", tmp_path / "models"
    s = main.run(main.config_from_args(base + ["--filter", "body", "--filter-cutoff", "0.5", "--filter-order", "2", "--filter-zero-phase",
                                               "--out-dir", str(out), "--save-models", str(mdir)]))
    assert (mdir / "filter" / "metadata.json").exists()
    assert "Samples conditioned by StreamFilter(body, hz=10, cutoff=0.5 Hz, sections=1, zero-phase)" in (out / "result.txt").read_text()
    rec = s["models"]["lr"]
    assert s["n_train"] == s0["n_train"] and s["n_test"] == s0["n_test"]
    from har.utils import persist

    f = persist.load(str(mdir / "filter"))
    assert f.kind == "body" and f.zero_phase and torch.equal(f.sos, F.butter_sos(2, 0.5, 10.0))
    r = predict.main(["--models", str(mdir), "--model", "lr", "--raw", p, "--device", "cpu", "--out", str(tmp_path / "p.csv")])
    assert r["rows"] == 96
    with open(tmp_path / "p.csv") as fh:
        rows = list(csv.reader(fh))[1:]
    pred = np.array([row[3] for row in rows])
    truth = np.array([ACTIVITIES[int(v)] for v in info["labels"]])
    from har.data.split import split_ids

    test = split_ids(96, [0.7, 0.3], 2018) == 1
    assert float((pred[test] == truth[test]).mean()) == pytest.approx(rec["accuracy"], abs=1e-12)
    assert r["accuracy"] == pytest.approx(float((pred == truth).mean()), abs=1e-12)
