"""CPU-only checks of the band scan's specification (include/fmd.h, fmd_scan_*; tests/scan_spec.py) and of the
preconditions the GPU tests (tests/test_gpu_scan_edges.py) rely on: the numpy Welch is scipy's, the comb probe puts
every bin within reach of the relative bound and a correct single-precision FFT meets that bound with margin, the
rule geometries hold the ties / bin-less slots / odd rasters their tests are about, and the rule is the one
tests/test_gpu_scan.py states."""
import numpy as np
import pytest

import scan_spec as sp

FS = 2.4e6
NFFTS, COMB_ROWS, COMB_SEGMENTS, COMB_TAIL = sp.NFFTS, sp.COMB_ROWS, sp.COMB_SEGMENTS, sp.COMB_TAIL
GEOMETRIES, comb_seed, comb_samples = sp.GEOMETRIES, sp.comb_seed, sp.comb_samples


def _scipy_welch(x, N, fs=FS):
    """scipy's Welch (float64) scaled and shifted as include/fmd.h defines the spectrum (as test_gpu_scan.py's)"""
    from scipy import signal
    _, p = signal.welch(x.astype(np.complex128), fs, window="hann", nperseg=N, noverlap=N // 2, detrend=False,
                        return_onesided=False, scaling="density")
    return np.fft.fftshift(p * fs / N)


@pytest.mark.parametrize("N", NFFTS)
def test_welch_is_scipys(fmsig, N):
    """One call of 50 000 samples (a remainder behind the last segment at every N): a station at 0.3 over noise of
    sigma 0.003, as test_gpu_scan.py's captures.  With scipy's own (unrounded) window the two agree to float64
    rounding: 1e-12 x peak, and 1e-9 dB on the bins within 50 dB of the peak.  The spec's own window is rounded to
    float32 as the device's table is: each window value moves by at most 2^-24 relative, so a bin moves by at most
    about 4 x 2^-24 = 2.4e-7 of the peak.  The bound is 5e-7 x peak, and on the bins within 20 dB of the peak
    5e-7 / 1e-2 -> 2.2e-4 dB."""
    from scipy import signal
    n = 50000
    rng = np.random.default_rng(N)
    x = (rng.standard_normal(2 * n) * 0.003).astype(np.float32).view(np.complex64)
    p = fmsig.default_params(FS, f_offset=-350e3, amp=0.3, noise_sigma=0.0, seed=N)
    x = x + fmsig.generate_f32(p, 0, n).view(np.complex64)
    assert (n - N) % (N // 2) != 0
    ref = _scipy_welch(x, N)
    peak = ref.max()
    exact = sp.welch([x], N, w=signal.get_window("hann", N))
    assert np.abs(exact - ref).max() <= 1e-12 * peak
    m = ref >= 1e-5 * peak
    assert np.abs(10 * np.log10(exact[m] / ref[m])).max() <= 1e-9
    got = sp.welch([x], N)
    assert np.abs(got - ref).max() <= 5e-7 * peak
    m = ref >= 1e-2 * peak
    assert np.abs(10 * np.log10(got[m] / ref[m])).max() <= 2.2e-4
    # the same segments, the tail dropped: a call cut to its whole segments gives the same spectrum
    S = sp.segments(n, N)
    assert np.array_equal(sp.welch([x[:(S - 1) * (N // 2) + N]], N), got)


def test_welch_over_calls_is_the_sum_of_the_calls_segments():
    """Nothing carries over between calls: K counts every call's own segments, each call starts a new segment 0."""
    N = 256
    rng = np.random.default_rng(2)
    calls = [(rng.standard_normal(2 * n) * 0.1).astype(np.float32).view(np.complex64) for n in (256, 700, 3000, 383)]
    w = sp.window(N)
    acc, K = np.zeros(N), 0
    for x in calls:
        for k in range((x.size - N) // (N // 2) + 1):
            acc += np.abs(np.fft.fft(w * x[k * N // 2:k * N // 2 + N].astype(np.complex128))) ** 2
            K += 1
    assert K == 1 + 4 + 22 + 1
    ref = np.fft.fftshift(acc / K / (N * np.sum(w * w)))
    got = sp.welch(calls, N)
    assert np.abs(got - ref).max() <= 1e-13 * ref.max()
    with pytest.raises(ValueError):
        sp.welch([calls[0][:N - 2]], N)


@pytest.mark.parametrize("N", NFFTS)
def test_comb_reaches_every_bin_and_single_precision_meets_the_bound(N):
    """The GPU test's bound is 1e-3 dB on every bin within 50 dB of the peak.  Every bin of the comb lies within
    20 dB, and a correct single-precision FFT (scipy.fft on complex64) stays within 1e-4 dB of the double one."""
    import scipy.fft

    def fft32(a):
        return scipy.fft.fft(a.astype(np.complex64), axis=-1)

    n = comb_samples(N)
    assert sp.segments(n, N) == COMB_SEGMENTS and (n - N) % (N // 2) == COMB_TAIL
    for row in COMB_ROWS:
        x = sp.comb(N, n, comb_seed(N, row))
        assert x.dtype == np.complex64 and x.shape == (n,)
        assert 0.02 <= np.abs(x).max() <= 0.0501
        assert np.array_equal(x[:N], x[N:2 * N])  # periodic in N
        ref = sp.welch([x], N)
        span = 10 * np.log10(ref.max() / ref.min())
        assert span <= 20.0, (N, row, span)
        assert span >= 6.0, (N, row, span)  # and the levels do differ: a permutation of bins would show
        assert np.unique(ref).size == N
        db = np.abs(10 * np.log10(sp.welch([x], N, fft=fft32) / ref)).max()
        assert db <= 1e-4, (N, row, db)
        # neighbouring bins differ by far more than the bound, in the median
        step = np.abs(10 * np.log10(ref[1:] / ref[:-1]))
        assert np.median(step) >= 0.1


def _identical_pairs(t):
    e, blo, bhi = t["eligible"], t["blo"], t["bhi"]
    return sum(1 for j in range(t["T"] - 1) if e[j] and e[j + 1] and blo[j] == blo[j + 1] and bhi[j] == bhi[j + 1])


def test_rule_geometries_hold_what_their_gpu_tests_are_about():
    for name, (fs, N, T, hw) in GEOMETRIES.items():
        t = sp.slot_tables(fs, N, T, hw, 150e3)
        assert t["contiguous"], name
        assert np.array_equal(t["shifts"], np.arange(T) - T // 2)
        assert np.all(np.diff(t["f"]) < 0)  # slot 0 is the highest frequency
        assert np.all(t["nlo"] <= np.arange(T)) and np.all(t["nhi"] >= np.arange(T))
        assert np.all(t["count"][t["eligible"]] >= 1)
    t = sp.slot_tables(*GEOMETRIES["ties"][:3], GEOMETRIES["ties"][3], 150e3)
    assert int(t["eligible"].sum()) == 939 and _identical_pairs(t) == 470
    assert t["T"] > 3 * 256  # the slot kernel's 256 threads make four trips
    t = sp.slot_tables(*GEOMETRIES["full"][:3], GEOMETRIES["full"][3], 150e3)
    assert int(t["eligible"].sum()) == 939 and int(t["count"].max()) == 341
    t = sp.slot_tables(*GEOMETRIES["narrow"][:3], GEOMETRIES["narrow"][3], 150e3)
    binless = t["formula"] & (t["count"] == 0)
    assert int(binless.sum()) == 24 and not np.any(t["eligible"] & binless)
    assert np.all(t["blo"][binless] > t["bhi"][binless])
    assert int(t["eligible"].sum()) == 75
    for name in ("odd", "unaligned"):
        fs, N, T, hw = GEOMETRIES[name]
        t = sp.slot_tables(fs, N, T, hw, 150e3)
        # not aligned: the slot centres are no whole number of bins apart, so bin counts differ between slots
        assert (N / T) != int(N / T)
        assert np.unique(t["count"][t["eligible"]]).size > 1, name
    assert GEOMETRIES["odd"][2] % 2 == 1
    t = sp.slot_tables(2.048e6, 512, 25, 100e3, 150e3)
    assert t["shifts"][0] == -12 and t["shifts"][-1] == 12  # -floor(T/2) .. -floor(T/2) + T - 1


def test_rule_is_the_one_test_gpu_scan_states(fmsig):
    """The inputs of test_gpu_scan.py's rule test (noise of sigma 0.004, three stations per capture), their float64
    Welch spectrum rounded to float32 as the device delivers it, through that file's _rule and through the spec."""
    import test_gpu_scan as old
    n = 65536
    for T, kw in [(24, {}), (64, {}), (24, {"half_width_hz": 75e3, "threshold_db": 12.0, "floor_quantile": 0.5,
                                           "nfft": 2048})]:
        rng = np.random.default_rng(T)
        G = 2
        x = old._noise(rng, G, n, 0.004)
        amps = (0.3, 0.05, 0.12, 0.02)
        for g in range(G):
            for i, off in enumerate(rng.choice(np.arange(-10, 11) * 107e3, size=3, replace=False)):
                p = fmsig.default_params(FS, f_offset=float(off), amp=amps[(g + i) % 4] * (1 + 0.1 * g),
                                         noise_sigma=0.0, seed=100 * g + i)
                x[g] += fmsig.generate_f32(p, 0, n).view(np.complex64)
        N = kw.get("nfft", 1024)
        hw, thr, q = kw.get("half_width_hz", 100e3), kw.get("threshold_db", 10.0), kw.get("floor_quantile", 0.2)
        t = sp.slot_tables(FS, N, T, hw, 150e3)
        for g in range(G):
            P = sp.welch([x[g]], N).astype(np.float32).astype(np.float64)
            floor_db, slot_db, cands = old._rule(P, T, hw=hw, thr=thr, q=q)
            r = sp.rule(P, t, thr, q)
            assert abs(r["floor_db"] - floor_db) <= 1e-12
            fin = np.isfinite(slot_db)
            assert np.array_equal(fin, np.isfinite(r["slot_db"])) and np.array_equal(fin, t["eligible"])
            assert np.abs(r["slot_db"][fin] - slot_db[fin]).max() <= 1e-9  # pairwise against sequential sums
            assert [c["shift"] for c in r["candidates"]] == cands and r["count"] == len(cands)
            assert len(cands) >= 1 and r["near_threshold"] == []
            for c in r["candidates"]:
                assert c["offset_hz"] == float(np.float32(-c["shift"] * FS / T))
                assert abs(c["power_db"] - r["slot_db"][c["slot"]]) <= 1e-5


def _tied_groups(t):
    """runs of neighbouring eligible slots with one bin set: [(first slot, last slot)]"""
    sets = list(zip(t["blo"], t["bhi"]))
    out, j = [], 0
    while j < t["T"]:
        k = j
        while k + 1 < t["T"] and t["eligible"][j] and t["eligible"][k + 1] and sets[k + 1] == sets[j]:
            k += 1
        if k > j:
            out.append((j, k))
        j = k + 1
    return out


def test_where_an_exact_tie_can_win():
    """Two slots tie exactly when their bin sets are equal.  On the (2.4e6, 256, 1024, 100e3) raster a slot is
    200 kHz / 9375 Hz = 21.33 bins wide and the raster has four slots per bin: three slots in four hold 21 bins, in
    runs of three with one set, and the fourth holds 22, both its neighbours' sets and one bin more.  With a
    spectrum that is positive everywhere the 22-bin slot beside a tied run is stronger than the run, so on that
    raster a tie is computed and compared but never wins.  With half_width 101.25 kHz (21.6 bins) it is the 22-bin
    slots that come in runs of three, between single 21-bin slots that hold less: there the strongest slots tie."""
    fs, N, T, hw = GEOMETRIES["ties"]
    t = sp.slot_tables(fs, N, T, hw, 150e3)
    groups = _tied_groups(t)
    assert len(groups) == 235 and all(b - a == 2 for a, b in groups)
    for a, b in groups:
        for m in (a - 1, b + 1):  # the neighbours of a run hold the run's bins and one more (or are ineligible)
            if t["eligible"][m]:
                assert t["blo"][m] <= t["blo"][a] and t["bhi"][m] >= t["bhi"][a] and t["count"][m] == t["count"][a] + 1
        assert t["eligible"][a - 1] or t["eligible"][b + 1]
    fs, N, T, hw = GEOMETRIES["ties_win"]
    t = sp.slot_tables(fs, N, T, hw, 150e3)
    groups = _tied_groups(t)
    assert len(groups) >= 200
    for a, b in groups:
        for m in (a - 1, b + 1):
            if t["eligible"][m]:
                assert t["blo"][m] >= t["blo"][a] and t["bhi"][m] <= t["bhi"][a] and t["count"][m] == t["count"][a] - 1
    # a spectrum that is strong on one run's bins: the run ties, the smallest shift of it is the candidate
    j0 = groups[len(groups) // 2][0]
    P = np.random.default_rng(4).uniform(1e-9, 2e-9, N).astype(np.float32).astype(np.float64)
    P[t["blo"][j0]:t["bhi"][j0] + 1] *= 1e5
    r = sp.rule(P, t, 10.0, 0.2)
    assert len(r["candidates"]) == 1
    j = r["candidates"][0]["slot"]
    same = [m for m in range(T) if t["eligible"][m] and r["power"][m] == r["power"][j]]
    assert same == [j0, j0 + 1, j0 + 2] and j == j0 and r["tie_winners"] == [j]
    assert r["candidates"][0]["shift"] == min(int(t["shifts"][m]) for m in same)


def test_binless_slots_are_never_listed():
    """On the narrow raster a slot without a bin reports -inf and is no candidate whatever the spectrum."""
    fs, N, T, hw = GEOMETRIES["narrow"]
    t = sp.slot_tables(fs, N, T, hw, 150e3)
    r = sp.rule(np.linspace(1e-6, 1e-3, N), t, 3.0, 0.2)
    binless = t["count"] == 0
    assert np.all(np.isneginf(r["slot_db"][binless])) and np.all(np.isneginf(r["snr_db"][binless]))
    assert r["candidates"] and not any(binless[c["slot"]] for c in r["candidates"])
