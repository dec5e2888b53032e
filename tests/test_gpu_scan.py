"""The band scan on the GPU (include/fmd.h fmd_scan_*, pvr.rtl.radiofm_amd/scan.py): the spectrum against scipy's
Welch, byte input against float input, bit reproducibility over rows / capture counts / launch forms / streams,
accumulation and reset, the slot and candidate rule against a numpy restatement, detection of synthetic stations,
scan_stations end to end, a full-size run and a decoder run that the scan must not disturb."""
from importlib import import_module

import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

FS = 2.4e6


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def scanmod(pkg):
    return import_module(pkg.__name__ + ".scan")


def _welch(x, N):
    """scipy's Welch (float64) scaled and shifted as include/fmd.h defines the spectrum."""
    from scipy import signal
    _, p = signal.welch(x.astype(np.complex128), FS, window="hann", nperseg=N, noverlap=N // 2, detrend=False,
                        return_onesided=False, scaling="density")
    return np.fft.fftshift(p * FS / N)


def _rule(P, T, hw=100e3, sep=150e3, thr=10.0, q=0.2):
    """numpy restatement of include/fmd.h's slot / floor / candidate rule on one spectrum P (float64)."""
    N = P.size
    fr = (np.arange(N) - N / 2) * FS / N
    ks = np.arange(T) - T // 2
    f = -ks * FS / T
    elig = np.abs(f) + hw <= FS / 2
    fb = np.sort(P)[int(np.floor(float(np.float32(q)) * (N - 1)))]
    pw = np.array([P[np.abs(fr - fk) <= hw].sum() for fk in f])
    cnt = np.array([(np.abs(fr - fk) <= hw).sum() for fk in f])
    with np.errstate(divide="ignore"):
        slot_db = np.where(elig, 10 * np.log10(pw), -np.inf)
        snr = 10 * np.log10(pw / (fb * cnt))
    cands = []
    for j in range(T):
        if not elig[j] or snr[j] < np.float32(thr):
            continue
        ok = all(pw[j] > pw[m] if m < j else pw[j] >= pw[m]
                 for m in range(T) if m != j and elig[m] and abs(f[m] - f[j]) <= sep)
        if ok:
            cands.append(j)
    cands.sort(key=lambda j: f[j])
    return 10 * np.log10(fb), slot_db, [int(ks[j]) for j in cands]


def _stations_capture(fmsig, stations, n, start=0):
    x = np.zeros(2 * n, np.float32)
    for p in stations:
        x += fmsig.generate_f32(p, start, n)
    return x.view(np.complex64)


def _noise(rng, G, n, sigma=0.01):
    return (rng.standard_normal((G, 2 * n)) * sigma).astype(np.float32).view(np.complex64)


def test_spectrum_matches_scipy_welch(scanmod, fmsig):
    rng = np.random.default_rng(1)
    worst_db, worst_abs = 0.0, 0.0
    for N in (256, 1024, 4096):
        for G in (1, 37):
            for n in (65536, 50000):
                x = _noise(rng, G, n, 0.003)
                for g in range(G):  # a station per capture at a per-capture offset, a tone in some
                    p = fmsig.default_params(FS, f_offset=-900e3 + 50e3 * g, amp=0.3, noise_sigma=0.0, seed=g)
                    x[g] += fmsig.generate_f32(p, 0, n).view(np.complex64)
                    if g % 3 == 0:
                        x[g] += (0.1 * np.exp(2j * np.pi * (0.31 + 0.001 * g) * np.arange(n))).astype(np.complex64)
                s = scanmod.Scan(FS, G, nfft=N)
                s.accumulate_host(x)
                psd = s.result()["psd"].astype(np.float64)
                s.close()
                for g in (0, G - 1):
                    ref = _welch(x[g], N)
                    peak = ref.max()
                    assert np.abs(psd[g] - ref).max() <= 1e-6 * peak, (N, G, n, g)
                    m = ref >= peak * 1e-5  # within 50 dB of the strongest bin
                    db = np.abs(10 * np.log10(psd[g][m] / ref[m])).max()
                    assert db <= 1e-3, (N, G, n, g, db)
                    worst_db = max(worst_db, db)
                    worst_abs = max(worst_abs, np.abs(psd[g] - ref).max() / peak)
    print("spectrum vs scipy (float64): worst %.2e dB within 50 dB of the peak, worst %.2e x peak overall"
          % (worst_db, worst_abs))


def test_byte_input_gives_the_bits_of_float_input(scanmod, fmsig):
    import torch
    G, n = 3, 40000
    u8 = np.stack([fmsig.generate_u8(fmsig.default_params(FS, f_offset=(g - 1) * 400e3, seed=7 + g), 0, n)
                   for g in range(G)])
    f32 = np.stack([fmsig.u8_to_f32(u8[g]) for g in range(G)])
    for N in (256, 1024, 4096):
        a = scanmod.Scan(FS, G, nfft=N)
        a.accumulate_host_u8(u8)
        b = scanmod.Scan(FS, G, nfft=N)
        b.accumulate_host(f32)
        ra, rb = a.result(), b.result()
        assert np.array_equal(ra["psd"].view(np.uint32), rb["psd"].view(np.uint32)), N
        assert np.array_equal(ra["slot_db"].view(np.uint32), rb["slot_db"].view(np.uint32)), N
        # the device entry point with a row stride longer than a capture
        d = torch.zeros((G, 2 * (n + 64)), dtype=torch.uint8, device="cuda")
        d[:, :2 * n] = torch.from_numpy(u8).cuda()
        c = scanmod.Scan(FS, G, nfft=N)
        c.accumulate_device(d.data_ptr(), n + 64, n, u8=True)
        torch.cuda.synchronize()
        assert np.array_equal(c.result()["psd"].view(np.uint32), rb["psd"].view(np.uint32)), N
        for s in (a, b, c):
            s.close()


def test_bits_do_not_depend_on_row_capture_count_or_stream(scanmod, fmsig):
    import torch
    n = 16384
    x = _stations_capture(fmsig, [fmsig.default_params(FS, f_offset=300e3, seed=3)], n)
    one = scanmod.Scan(FS, 1)
    one.accumulate_host(x)
    ref = one.result()["psd"][0].copy()
    one.reset()
    one.accumulate_host(x)
    assert np.array_equal(one.result()["psd"][0].view(np.uint32), ref.view(np.uint32))  # two runs
    one.close()
    G = 4096
    d = (torch.randn((G, 2 * n), device="cuda") * 0.05)
    d[G - 1] = torch.from_numpy(x.view(np.float32)).cuda()
    torch.cuda.synchronize()
    for stream in (None, torch.cuda.Stream()):
        big = scanmod.Scan(FS, G)
        if stream is None:
            big.accumulate_device(d.data_ptr(), n, n)
        else:
            with torch.cuda.stream(stream):
                big.accumulate_device(d.data_ptr(), n, n, stream=stream.cuda_stream)
            stream.synchronize()
        got = big.result()["psd"][G - 1]
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), stream
        big.close()


def test_accumulation_over_calls_and_reset(scanmod):
    rng = np.random.default_rng(5)
    N = 1024
    sizes = (65536, 20000, 3000)
    xs = [_noise(rng, 2, n, 0.02) for n in sizes]
    for x in xs:
        x[1] += (0.2 * np.exp(2j * np.pi * 0.123 * np.arange(x.shape[1]))).astype(np.complex64)
    s = scanmod.Scan(FS, 2, nfft=N)
    for x in xs:
        s.accumulate_host(x)
    psd = s.result()["psd"].astype(np.float64)
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32).astype(np.float64)
    for g in range(2):
        acc, K = np.zeros(N), 0
        for x in xs:
            seg = (x.shape[1] - N) // (N // 2) + 1
            for k in range(seg):
                acc += np.abs(np.fft.fft(w * x[g, k * N // 2:k * N // 2 + N].astype(np.complex128))) ** 2
            K += seg
        ref = np.fft.fftshift(acc / K / (N * np.sum(w * w)))
        peak = ref.max()
        assert np.abs(psd[g] - ref).max() <= 1e-6 * peak
        m = ref >= 1e-5 * peak
        assert np.abs(10 * np.log10(psd[g][m] / ref[m])).max() <= 1e-3
    # reset starts over: one call after it gives the bits of a fresh object
    s.reset()
    s.accumulate_host(xs[1])
    fresh = scanmod.Scan(FS, 2, nfft=N)
    fresh.accumulate_host(xs[1])
    assert np.array_equal(s.result()["psd"].view(np.uint32), fresh.result()["psd"].view(np.uint32))
    with pytest.raises(Exception, match="fmd error -3"):
        s.accumulate_host(xs[0][:, :N - 2])  # shorter than one segment: FMD_ERR_SIZE


@pytest.mark.parametrize("T,kw", [(24, {}), (64, {}), (24, {"half_width_hz": 75e3, "threshold_db": 12.0,
                                                              "floor_quantile": 0.5, "nfft": 2048})])
def test_slots_floor_and_candidates_follow_the_rule(scanmod, fmsig, T, kw):
    rng = np.random.default_rng(T)
    G, n = 6, 65536
    x = _noise(rng, G, n, 0.004)
    amps = (0.3, 0.05, 0.12, 0.02)
    for g in range(G):
        for i, off in enumerate(rng.choice(np.arange(-10, 11) * 107e3, size=3, replace=False)):
            p = fmsig.default_params(FS, f_offset=float(off), amp=amps[(g + i) % 4] * (1 + 0.1 * g), noise_sigma=0.0,
                                     seed=100 * g + i)
            x[g] += fmsig.generate_f32(p, 0, n).view(np.complex64)
    s = scanmod.Scan(FS, G, table_size=T, **kw)
    s.accumulate_host(x)
    r = s.result()
    rule_kw = {k: kw[k] for k in ("half_width_hz", "threshold_db", "floor_quantile") if k in kw}
    rule_kw = {{"half_width_hz": "hw", "threshold_db": "thr", "floor_quantile": "q"}[k]: v for k, v in rule_kw.items()}
    for g in range(G):
        floor_db, slot_db, cands = _rule(r["psd"][g].astype(np.float64), T, **rule_kw)
        assert abs(r["floor_db"][g] - floor_db) <= 1e-4
        fin = np.isfinite(slot_db)
        assert np.array_equal(fin, np.isfinite(r["slot_db"][g]))
        assert np.abs(r["slot_db"][g][fin] - slot_db[fin]).max() <= 1e-4
        assert [c["shift"] for c in r["candidates"][g]] == cands, g
        assert int(r["counts"][g]) == len(cands)
    # a clipped list still reports the true count
    r2 = s.result(max_cand=1)
    assert all(len(c) <= 1 for c in r2["candidates"]) and np.array_equal(r2["counts"], r["counts"])


def _detection_stations(fmsig):
    """stereo + RDS, mono, weak (~20 dB over the slot floor), two 200 kHz apart, one at +1.0 MHz"""
    return [fmsig.default_params(FS, f_offset=-700e3, amp=0.2, noise_sigma=0.004, seed=1, pi=0x7001),
            fmsig.mono_params(FS, f_offset=400e3, amp=0.2, noise_sigma=0.004, seed=2),
            fmsig.default_params(FS, f_offset=700e3, amp=0.03, noise_sigma=0.0, seed=3, pi=0x7003),
            fmsig.default_params(FS, f_offset=-300e3, amp=0.1, noise_sigma=0.0, seed=4, pi=0x7004),
            fmsig.default_params(FS, f_offset=-100e3, amp=0.1, noise_sigma=0.0, seed=5, pi=0x7005),
            fmsig.default_params(FS, f_offset=1.0e6, amp=0.1, noise_sigma=0.0, seed=6, pi=0x7006)]


@pytest.mark.parametrize("T", [24, 64])
def test_detection_of_synthetic_stations(scanmod, fmsig, T):
    """Slots of +-75 kHz: with the default +-100 kHz, the slot between two stations 200 kHz apart sums half of each
    (an FM station of 75 kHz deviation is about flat over +-75 kHz) and ties with them."""
    n = 65536
    st = _detection_stations(fmsig)
    rng = np.random.default_rng(9)
    s = scanmod.Scan(FS, 2, table_size=T, half_width_hz=75e3)
    for call in range(4):
        x = np.stack([_stations_capture(fmsig, st, n, call * n), _noise(rng, 1, n, 0.004)[0]])
        s.accumulate_host(x)
    r = s.result()
    got = [c["shift"] for c in r["candidates"][0]]
    offs = sorted(p.f_offset for p in st)
    assert len(got) == len(offs), got
    step = FS / T
    for c, f in zip(r["candidates"][0], offs):
        # the station's own step; at T = 64 a station between two steps may land on either (flat-topped spectrum)
        assert abs(c["offset_hz"] - f) <= (0.0 if T == 24 else step), (got, f)
    weak = [c for c in r["candidates"][0] if abs(c["offset_hz"] - 700e3) <= step][0]
    assert 14.0 <= weak["snr_db"] <= 26.0, weak
    assert r["candidates"][1] == []  # noise only


def test_scan_stations_end_to_end(scanmod, fmsig):
    n, G = 65536, 8
    sets = []
    grid = [-900e3, -600e3, -300e3, 0.0, 300e3, 600e3, 900e3]  # 300 kHz apart
    for g in range(G):
        offs = [grid[(g + 2 * i) % 7] for i in range(2 + g % 3)]
        st = [fmsig.default_params(FS, f_offset=f, amp=0.2, noise_sigma=0.003, seed=50 * g + i, pi=0x4000 + 16 * g + i,
                                   ps="ST%d_%d" % (g, i)) for i, f in enumerate(offs[:-1])]
        last = dict(f_offset=offs[-1], amp=0.2, noise_sigma=0.003, seed=50 * g + 9)
        st.append(fmsig.mono_params(FS, **last) if g % 2 == 0 else
                  fmsig.default_params(FS, pi=0x4000 + 16 * g + 9, ps="ST%d_9" % g, **last))
        sets.append(st)
    # capture 7: the seek test's stations (tests/test_gpu_configs.py), the mono one that seek passes over included
    sets[7] = [fmsig.default_params(FS, f_offset=-700e3, amp=0.2, noise_sigma=0.004, seed=81, pi=0x7001),
               fmsig.default_params(FS, f_offset=-200e3, amp=0.2, noise_sigma=0.004, seed=82, pi=0x7002),
               fmsig.default_params(FS, f_offset=500e3, amp=0.2, noise_sigma=0.004, seed=83, pi=0x7003),
               fmsig.mono_params(FS, f_offset=100e3, amp=0.2, noise_sigma=0.004, seed=84)]

    def source(call):
        return np.stack([_stations_capture(fmsig, st, n, call * n) for st in sets])

    out = scanmod.scan_stations(source, G, FS, table_size=24, center_hz=98.0e6)
    for g, st in enumerate(sets):
        want = sorted(st, key=lambda p: p.f_offset)
        got = out[g]
        assert [round(s["freq_hz"] - 98.0e6) for s in got] == [round(p.f_offset) for p in want], (g, got)
        for s, p in zip(got, want):
            assert s["shift"] == -int(round(p.f_offset / 100e3))
            mono = p.a_pilot == 0.0
            assert s["stereo"] == (not mono), (g, s)
            if mono:
                assert s["pi"] is None
            else:
                assert s["pi"] == p.pi, (g, s)
                assert s["ps"] == p.ps.decode("latin1"), (g, s)
    # no candidates at all: no decode, empty lists
    rng = np.random.default_rng(3)
    quiet = scanmod.scan_stations(lambda call: _noise(rng, 2, n, 0.004), 2, FS, scan_calls=2, confirm_calls=2)
    assert quiet == [[], []]


def test_full_size_from_the_device_generator(scanmod, fmsig):
    import torch
    G, n = 8192, 65536
    offs = [(-1000e3 + 25e3 * (g % 81)) for g in range(G)]
    params = [fmsig.default_params(FS, f_offset=offs[g], amp=0.25, noise_sigma=0.005, seed=g) for g in range(G)]
    gen = fmsig.DeviceGenerator(params)
    d = torch.empty((G, n, 2), dtype=torch.float32, device="cuda")
    gen.generate(d, 0, n)
    torch.cuda.synchronize()
    s = scanmod.Scan(FS, G)
    s.accumulate_device(d.data_ptr(), n, n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = s.result()
    rows = [0, 1, 2, 77, 1000, 4095, 4096, 6000, 8190, 8191]
    for g in rows:
        ref = _welch(d[g].cpu().numpy().view(np.complex64).reshape(-1), 1024)
        peak = ref.max()
        assert np.abs(r["psd"][g] - ref).max() <= 1e-6 * peak, g
    step = FS / 64
    for g in range(G):
        if abs(offs[g]) + 75e3 > FS / 2 - 100e3:  # too close to the edge for an eligible slot of its own
            continue
        cs = r["candidates"][g]
        assert len(cs) == 1 and abs(cs[0]["offset_hz"] - offs[g]) <= step, (g, cs)


def test_scan_between_process_calls_does_not_disturb_the_decoder(pkg, scanmod, fmsig):
    import torch
    G, k, n, calls = 4, 3, 65536, 10  # the first groups complete in the 7th call
    shifts = np.array([[-7, 2, 5]] * G, np.int32).reshape(-1)
    st = [fmsig.default_params(FS, f_offset=f, amp=0.2, noise_sigma=0.004, seed=int(f) & 0xffff, pi=0x2000 + i)
          for i, f in enumerate((700e3, -200e3, -500e3))]
    caps = [torch.from_numpy(np.stack([_stations_capture(fmsig, st, n, c * n)] * G).view(np.float32)).cuda()
            for c in range(calls)]

    def run(with_scan):
        b = pkg.Batch(pkg.make_params(FS, 0.0, 48000.0, 15000.0, 11, table_size=24), G * k, tuning_shifts=shifts)
        b.set_channels_per_capture(k)
        stream = torch.cuda.Stream()
        s = scanmod.Scan(FS, G, table_size=24) if with_scan else None
        a_stride = b.max_audio_floats(n)
        audio, status, groups = [], [], []
        for c in range(calls):
            d_audio = torch.zeros((G * k, a_stride), dtype=torch.float32, device="cuda")
            if s is not None:
                s.accumulate_device(caps[c].data_ptr(), n, n, stream=stream.cuda_stream)
            nf = b.process_device(caps[c].data_ptr(), n, n, d_audio.data_ptr(), a_stride, stream=stream.cuda_stream)
            if s is not None:
                s.accumulate_device(caps[c].data_ptr(), n, n, stream=stream.cuda_stream)
            groups.append(b.collect_rds_array(stream=stream.cuda_stream))
            stream.synchronize()
            audio.append(d_audio[:, :nf].cpu().numpy())
            status.append([(b.status(ch).stereo_detected, b.status(ch).pilot_level, b.status(ch).tuning_offset)
                           for ch in range(G * k)])
        if s is not None:
            assert sum(len(c) for c in s.result()["candidates"]) == 3 * G
            s.close()
        b.close()
        return audio, status, groups

    a0, s0, g0 = run(False)
    a1, s1, g1 = run(True)
    for c in range(calls):
        assert np.array_equal(a0[c].view(np.uint32), a1[c].view(np.uint32)), c
        assert s0[c] == s1[c]
        assert np.array_equal(g0[c], g1[c])
    assert sum(len(g) for g in g0) > 0
