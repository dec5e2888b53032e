"""The band scan (include/fmd.h fmd_scan_*) at every FFT size, in both launch forms and at the raster's edges, held
against its numpy definition (tests/scan_spec.py; preconditions in tests/test_scan_spec_cpu.py):

  - every bin of the spectrum at N = 256 .. 4096 (comb probes: every bin has a level of its own and lies within
    reach of the relative bound), per-capture walk (G >= 512) and (capture, chunk) workgroups + reduce (G < 512);
  - segment counts around the sub-group count P = 4096 / N and the chunk of 16, with and without a remainder;
  - accumulation over growing calls on a caller's stream (the split form's scratch regrows), with a finish between;
  - nothing outside `samples` reaches the result (NaN / infinity / 0 / 255 in the pad and the unused tails);
  - fmd_scan_finish_device (subsets of outputs, clipped lists, sentinels) and fmd_scan_reset queued on a stream;
  - the slot / floor / candidate rule on T = 1024, odd T, rasters not aligned to the bins, bin-less slots and ties.

Bounds: the spectrum within 1e-3 dB on every bin within 50 dB of the peak and within 1e-6 x peak everywhere, the
rule's dB outputs within 1e-4 dB (tests/test_gpu_scan.py's); forms, entry points and streams agree bit for bit."""
from importlib import import_module

import numpy as np
import pytest

import scan_spec as sp
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

FS = 2.4e6
ROWS = 512            # the smallest capture count of the per-capture walk
PICK = (0, 255, 511)  # the rows that also go through the split form
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def scanmod(pkg):
    return import_module(pkg.__name__ + ".scan")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ptr(t, row=0, sample=0):
    """device address of sample `sample` of row `row` of a [rows, stride, 2] (or [rows, 2 stride]) tensor"""
    return t.data_ptr() + (row * t.stride(0) + 2 * sample) * t.element_size()


def _host(t, row, n, at=0):
    """samples at .. at + n of a row of a [rows, stride, 2] float32 device tensor, as complex64 on the host"""
    return t[row, at:at + n].cpu().numpy().reshape(-1).view(np.complex64)


def _within_bounds(psd, ref, tag, every_bin=False):
    """the project's spectrum bounds; -> (worst dB, worst fraction of the peak)"""
    psd = psd.astype(np.float64)
    peak = ref.max()
    assert np.all(np.isfinite(psd)), tag
    m = ref >= 1e-5 * peak  # within 50 dB of the strongest bin
    if every_bin:
        assert m.all(), tag  # precondition: the relative bound applies to all N bins
    frac = np.abs(psd - ref).max() / peak
    with np.errstate(divide="ignore"):
        db = np.abs(10 * np.log10(psd[m] / ref[m])).max()
    assert frac <= 1e-6, (tag, frac)
    assert db <= 1e-3, (tag, db)
    return db, frac


def _scan_psd(scanmod, G, N, ptr, stride, samples, stream=None, **kw):
    """one call through a new scan of G captures -> psd [G, N]"""
    s = scanmod.Scan(FS, G, nfft=N)
    s.accumulate_device(ptr, stride, samples, stream=stream.cuda_stream if stream else None, **kw)
    if stream:
        stream.synchronize()
    psd = s.result()["psd"]
    s.close()
    return psd


def _tone_rows(torch, rows, stride, seed, sigma=0.01, amp=0.2):
    """[rows, stride, 2] float32 on the device: noise plus a tone per row at a frequency of its own"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.randn((rows, stride, 2), generator=g, device="cuda", dtype=torch.float32) * sigma
    f = (torch.arange(rows, device="cuda", dtype=torch.float64) * 0.6180339887 + 0.137) % 1.0 - 0.5
    t = torch.arange(stride, device="cuda", dtype=torch.float64)
    for a in range(0, rows, 64):  # in blocks of rows: the float64 phase table stays small
        ph = 2 * np.pi * ((f[a:a + 64, None] * t[None, :]) % 1.0)
        d[a:a + 64, :, 0] += (amp * torch.cos(ph)).float()
        d[a:a + 64, :, 1] += (amp * torch.sin(ph)).float()
    torch.cuda.synchronize()
    return d


# ---- a. every bin, every size, both forms ---------------------------------------------------------------------
@pytest.mark.parametrize("N", sp.NFFTS)
def test_every_bin_at_every_size_in_both_forms(scanmod, torch, N):
    n = sp.comb_samples(N)  # 7 segments and 37 samples
    stride = n + 1          # even
    x = np.zeros((ROWS, stride), np.complex64)
    for g in range(ROWS):
        x[g, :n] = sp.comb(N, n, sp.comb_seed(N, g))
    d = torch.from_numpy(x.view(np.float32).reshape(ROWS, stride, 2)).cuda()
    walk = _scan_psd(scanmod, ROWS, N, _ptr(d), stride, n)
    worst_db = worst_frac = 0.0
    for g in sp.COMB_ROWS:
        db, frac = _within_bounds(walk[g], sp.welch([x[g, :n]], N), (N, g), every_bin=True)
        worst_db, worst_frac = max(worst_db, db), max(worst_frac, frac)
    for rows in ((0, 1, 255), (1, 255, 511)):
        d3 = d[list(rows)].contiguous()
        split = _scan_psd(scanmod, 3, N, _ptr(d3), stride, n)
        for i, g in enumerate(rows):
            assert np.array_equal(_bits(split[i]), _bits(walk[g])), (N, g)
    print("comb, N = %4d, every bin, both forms: worst %.2e dB, worst %.2e x peak" % (N, worst_db, worst_frac))


# ---- b. segment counts around the sub-group and chunk sizes -----------------------------------------------------
@pytest.mark.parametrize("N", sp.NFFTS)
def test_segment_counts_around_subgroups_and_chunks(scanmod, torch, N):
    P = 4096 // N
    counts = sorted({1, P, P + 1, 15, 16, 17, 33} | ({P - 1} if P > 1 else set()))
    hop = N // 2
    stride = 32 * hop + N + hop  # even, >= every `samples` below
    d = _tone_rows(torch, ROWS, stride, seed=N)
    d3 = d[list(PICK)].contiguous()
    host = {g: _host(d, g, stride) for g in PICK}
    worst_db = worst_frac = 0.0
    for S in counts:
        for rem in (0, hop - 1):
            n = (S - 1) * hop + N + rem
            assert sp.segments(n, N) == S and n <= stride
            walk = _scan_psd(scanmod, ROWS, N, _ptr(d), stride, n)
            three = _scan_psd(scanmod, 3, N, _ptr(d3), stride, n)
            for i, g in enumerate(PICK):
                one = _scan_psd(scanmod, 1, N, _ptr(d, g), stride, n)
                assert np.array_equal(_bits(one[0]), _bits(walk[g])), (N, S, rem, g)
                assert np.array_equal(_bits(three[i]), _bits(walk[g])), (N, S, rem, g)
                db, frac = _within_bounds(walk[g], sp.welch([host[g][:n]], N), (N, S, rem, g))
                worst_db, worst_frac = max(worst_db, db), max(worst_frac, frac)
    # fewer samples than a segment: refused, in both forms, and the totals stay
    for G, buf in ((ROWS, d), (3, d3)):
        s = scanmod.Scan(FS, G, nfft=N)
        s.accumulate_device(_ptr(buf), stride, 3 * N)
        torch.cuda.synchronize()
        before = s.result()["psd"].copy()
        with pytest.raises(Exception, match="fmd error -3"):
            s.accumulate_device(_ptr(buf), stride, N - 2)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(s.result()["psd"]), _bits(before)), (N, G)
        s.close()
    print("N = %4d, S in %s: worst %.2e dB, worst %.2e x peak" % (N, counts, worst_db, worst_frac))


# ---- c. accumulation in both forms, growing calls, on a caller's stream ------------------------------------------
@pytest.mark.parametrize("N", sp.NFFTS)
def test_accumulation_over_growing_calls_on_a_stream(scanmod, torch, N):
    sizes = [n for n in (N, 3000, 20000, 65536) if n >= N] + [2 * N + 11]
    assert sizes == sorted(sizes[:-1]) + [sizes[-1]] and sizes[-1] < sizes[-2]
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + n + (n & 1))  # every call's first sample at an even offset
    stride = starts[-1]
    d = _tone_rows(torch, ROWS, stride, seed=7 * N)
    stream = torch.cuda.Stream()
    side = torch.empty((ROWS, N), dtype=torch.float32, device="cuda")  # the finish in the middle writes here

    def run(G, finish_after=None):
        s = scanmod.Scan(FS, G, nfft=N)
        for i, (at, n) in enumerate(zip(starts, sizes)):  # queued back to back: no host wait of the test's between
            s.accumulate_device(_ptr(d, 0, at), stride, n, stream=stream.cuda_stream)
            if i == finish_after:
                s.finish_device(psd=side.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        psd = s.result()["psd"]
        s.close()
        return psd

    split, walk = run(2), run(ROWS)
    assert np.array_equal(_bits(split), _bits(walk[:2])), N
    for G in (2, ROWS):
        again = run(G, finish_after=2)
        assert np.array_equal(_bits(again[:2]), _bits(split)), (N, G)
    worst_db = worst_frac = 0.0
    for g in (0, 1):
        calls = [_host(d, g, n, at) for at, n in zip(starts, sizes)]
        db, frac = _within_bounds(split[g], sp.welch(calls, N), (N, g))
        worst_db, worst_frac = max(worst_db, db), max(worst_frac, frac)
    # the walk form's last row too (against the definition: the split form never saw it)
    calls = [_host(d, ROWS - 1, n, at) for at, n in zip(starts, sizes)]
    _within_bounds(walk[ROWS - 1], sp.welch(calls, N), (N, ROWS - 1))
    print("N = %4d, calls of %s: worst %.2e dB, worst %.2e x peak" % (N, sizes, worst_db, worst_frac))


# ---- d. nothing outside `samples` is read into the result --------------------------------------------------------
@pytest.mark.parametrize("N", sp.NFFTS)
@pytest.mark.parametrize("G", [3, ROWS])
def test_pad_and_unused_tail_do_not_reach_the_result(scanmod, torch, N, G):
    hop = N // 2
    S = 18  # two chunks, the second partial
    used = (S - 1) * hop + N
    n = used + hop - 1
    stride = n + 67  # even
    assert stride % 2 == 0 and sp.segments(n, N) == S
    # float: NaN and +-infinity behind the last whole segment and in the pad
    clean = _tone_rows(torch, G, used, seed=N + G)
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")], device="cuda").repeat(2 * stride // 3 + 1)
    d = bad[:2 * stride].reshape(1, stride, 2).repeat(G, 1, 1).contiguous()
    d[:, :used] = clean
    torch.cuda.synchronize()
    want = _scan_psd(scanmod, G, N, _ptr(clean), used, used)
    got = _scan_psd(scanmod, G, N, _ptr(d), stride, n)
    assert np.all(np.isfinite(got))
    assert np.array_equal(_bits(got), _bits(want)), (N, G)
    # bytes: 0 and 255 there
    g = torch.Generator(device="cuda").manual_seed(N + G)
    cb = torch.randint(96, 160, (G, 2 * used), generator=g, device="cuda", dtype=torch.uint8)
    db = torch.tensor([0, 255, 255, 0, 0], device="cuda", dtype=torch.uint8).repeat(2 * stride // 5 + 1)
    db = db[:2 * stride].reshape(1, -1).repeat(G, 1).contiguous()
    db[:, :2 * used] = cb
    torch.cuda.synchronize()
    want = _scan_psd(scanmod, G, N, cb.data_ptr(), used, used, u8=True)
    got = _scan_psd(scanmod, G, N, db.data_ptr(), stride, n, u8=True)
    assert np.all(np.isfinite(got)) and got.max() > 0
    assert np.array_equal(_bits(got), _bits(want)), (N, G, "u8")


# ---- e. fmd_scan_finish_device and fmd_scan_reset on a stream ----------------------------------------------------
def _station_captures(fmsig, fs, G, n, seed, sigma=0.004, per_capture=3, margin=250e3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((G, 2 * n)) * sigma).astype(np.float32).view(np.complex64)
    amps = (0.3, 0.05, 0.12, 0.08)
    grid = np.arange(-int((fs / 2 - margin) // 107e3), int((fs / 2 - margin) // 107e3) + 1) * 107e3
    for g in range(G):
        for i, off in enumerate(rng.choice(grid[::3], size=per_capture, replace=False)):  # >= 321 kHz apart
            p = fmsig.default_params(fs, f_offset=float(off), amp=amps[(g + i) % 4] * (1 + 0.1 * g), noise_sigma=0.0,
                                     seed=100 * g + i)
            x[g] += fmsig.generate_f32(p, 0, n).view(np.complex64)
    return x


def test_finish_device_outputs_subsets_clipping_and_sentinels(pkg, scanmod, torch, fmsig):
    G, N, T, n = 4, 1024, 64, 16384
    x = _station_captures(fmsig, FS, G, n, seed=11)
    s = scanmod.Scan(FS, G, table_size=T, nfft=N)
    s.accumulate_host(x)
    host = s.result()
    assert host["counts"].max() >= 2 and host["counts"].min() >= 1  # a list that max_cand = 1 clips
    csz = pkg.SCAN_CANDIDATE_DTYPE.itemsize
    hcand = np.zeros((G, T), pkg.SCAN_CANDIDATE_DTYPE)
    for g in range(G):
        for i, c in enumerate(host["candidates"][g]):
            hcand[g, i] = tuple(c[k] for k in pkg.SCAN_CANDIDATE_DTYPE.names)
    full = {k: np.ascontiguousarray(host[k]).view(np.uint8).reshape(-1)
            for k in ("psd", "slot_db", "floor_db", "counts")}
    assert host["counts"].dtype == np.uint32
    sizes = {"psd": 4 * G * N, "slot_db": 4 * G * T, "floor_db": 4 * G, "counts": 4 * G}
    guard = 64
    stream = torch.cuda.Stream()
    cases = [(("psd", "slot_db", "floor_db", "cand", "counts"), T), (("psd",), 0), (("cand",), T), (("counts",), 0),
             (("slot_db", "floor_db"), 0), (("cand", "counts"), 1), (("cand", "counts"), 0), (("cand",), 1),
             (("psd", "cand", "counts"), 2)]
    for names, max_cand in cases:
        with torch.cuda.stream(stream):
            bufs = {k: torch.full(((G * max_cand * csz if k == "cand" else sizes[k]) + guard,), SENTINEL,
                                  dtype=torch.uint8, device="cuda") for k in names}
            s.finish_device(max_cand=max_cand, stream=stream.cuda_stream, **{k: b.data_ptr() for k, b in bufs.items()})
        stream.synchronize()
        for k, b in bufs.items():
            got = b.cpu().numpy()
            assert np.all(got[-guard:] == SENTINEL), (names, max_cand, k)
            got = got[:-guard]
            if k != "cand":
                assert np.array_equal(got, full[k]), (names, max_cand, k)
                continue
            got = got.reshape(G, max_cand * csz)
            for g in range(G):
                kept = min(int(host["counts"][g]), max_cand)  # the lowest-frequency candidates, in order
                assert np.array_equal(got[g, :kept * csz], hcand[g, :kept].view(np.uint8).reshape(-1)), (names, g)
                assert np.all(got[g, kept * csz:] == SENTINEL), (names, max_cand, g)
    # a finish does not disturb the totals
    assert np.array_equal(_bits(s.result()["psd"]), _bits(host["psd"]))
    s.close()


@pytest.mark.parametrize("G", [3, ROWS])
def test_reset_queued_on_a_stream_between_two_calls(scanmod, torch, G):
    N, n = 512, 6000
    d = _tone_rows(torch, G, 2 * n, seed=G)
    stream = torch.cuda.Stream()
    s = scanmod.Scan(FS, G, nfft=N)
    s.accumulate_device(_ptr(d), 2 * n, n, stream=stream.cuda_stream)
    s.reset(stream=stream.cuda_stream)
    s.accumulate_device(_ptr(d, 0, n), 2 * n, n - 100, stream=stream.cuda_stream)
    stream.synchronize()
    got = s.result()["psd"]
    s.close()
    want = _scan_psd(scanmod, G, N, _ptr(d, 0, n), 2 * n, n - 100, stream=stream)
    assert np.array_equal(_bits(got), _bits(want))
    _within_bounds(got[G - 1], sp.welch([_host(d, G - 1, n - 100, n)], N), G)


# ---- f. the rule on other rasters ---------------------------------------------------------------------------------
RULE_KW = {"ties": {}, "ties_win": {}, "narrow": {"threshold_db": 6.0}, "odd": {"floor_quantile": 0.35},
           "unaligned": {"threshold_db": 12.0, "floor_quantile": 0.5}, "full": {}}


@pytest.mark.parametrize("name", list(sp.GEOMETRIES))
def test_rule_on_other_rasters(scanmod, fmsig, name):
    fs, N, T, hw = sp.GEOMETRIES[name]
    kw = RULE_KW[name]
    thr, q = kw.get("threshold_db", 10.0), kw.get("floor_quantile", 0.2)
    G, n = 4, 32768
    x = _station_captures(fmsig, fs, G, n, seed=T + N, margin=hw + 150e3)
    s = scanmod.Scan(fs, G, table_size=T, nfft=N, half_width_hz=hw, **kw)
    s.accumulate_host(x)
    r = s.result()
    s.close()
    t = sp.slot_tables(fs, N, T, hw, 150e3)
    assert np.array_equal(r["shifts"], t["shifts"])
    winners = 0
    for g in range(G):
        ref = sp.rule(r["psd"][g].astype(np.float64), t, thr, q)
        assert ref["near_threshold"] == [], (name, g)  # preconditions: the rule's outcome is not a matter of rounding,
        assert ref["count"] >= 1, (name, g)            # and there is something to list
        assert abs(float(r["floor_db"][g]) - ref["floor_db"]) <= 1e-4, (name, g)
        fin = np.isfinite(ref["slot_db"])
        assert np.array_equal(fin, t["eligible"])
        assert np.array_equal(np.isneginf(r["slot_db"][g]), ~fin), (name, g)
        assert np.abs(r["slot_db"][g][fin] - ref["slot_db"][fin]).max() <= 1e-4, (name, g)
        got = r["candidates"][g]
        assert int(r["counts"][g]) == ref["count"] and len(got) == ref["count"], (name, g)
        for c, w in zip(got, ref["candidates"]):
            assert c["shift"] == w["shift"] and c["offset_hz"] == w["offset_hz"], (name, g, c, w)
            assert abs(c["power_db"] - w["power_db"]) <= 1e-4, (name, g, c, w)
            assert abs(c["snr_db"] - w["snr_db"]) <= 1e-4, (name, g, c, w)
        assert [c["offset_hz"] for c in got] == sorted(c["offset_hz"] for c in got)
        if name in ("ties", "ties_win"):
            assert ref["ties"], (name, g)  # exact ties are compared
        for j in ref["tie_winners"]:  # an exact tie at the top goes to the smaller shift
            same = [m for m in range(T) if t["eligible"][m] and ref["power"][m] == ref["power"][j]]
            assert t["shifts"][j] == min(t["shifts"][m] for m in same)
            assert int(t["shifts"][j]) in [c["shift"] for c in got]
            assert not any(int(t["shifts"][m]) in [c["shift"] for c in got] for m in same if m != j)
        winners += len(ref["tie_winners"])
        if name == "narrow":
            binless = t["formula"] & (t["count"] == 0)
            assert binless.sum() == 24 and np.all(np.isneginf(r["slot_db"][g][binless]))
            assert not any(binless[c["shift"] + T // 2] for c in got)
    if name == "ties_win":
        assert winners >= 1  # precondition: a candidate that won an exact tie (impossible on "ties": see the CPU test)
