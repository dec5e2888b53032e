"""Every channel's demodulated multiplex (MPX) beside the audio (FMD_MPX_*, include/fmd.h): the FM PLL's output at the
baseband rate, transposed into one row per channel by k_mpx_out, as float or as 16-bit integers.

The contract needs no tolerance.  FMD_MPX_F32 is the float the oracle's `baseband` tap holds (m_BufferBaseband,
FmDecode.cpp:433), bit for bit; FMD_MPX_S16 is mpx16() of it, s = saturate_int16(round_half_even(x * 8192.0f)), NaN
gives 0 -- x * 2^13 is exact in float32, so every sample has one right value.  Expected values are the CPU oracle's
tap or mpx16() of it; where the channel count is beyond the oracle's reach they are the rows of the product's own
130-channel float batch, itself compared with the oracle in the same test; never the output under test.  Every
comparison is an equality.
"""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package
from feed_spec import mpx16

pytestmark = pytest.mark.gpu

N = 65536
FILL16 = 0x5A5A
FILL32 = 0x5A5A5A5A


def value_sets():
    """every tie (k + 0.5) / 8192 and every integer k / 8192, k = -32769 ... 32768; +-0, the smallest denormal,
    +-inf, NaN, +-3.4e38, the scale's landmarks; 10^6 random 32-bit patterns as floats"""
    k = np.arange(-32769, 32769, dtype=np.float64)
    ties = ((k + 0.5) / 8192.0).astype(np.float32)
    ints = (k / 8192.0).astype(np.float32)
    edges = np.array([0.0, -0.0, np.float32(1e-45), -np.float32(1e-45), np.inf, -np.inf, np.nan, -np.nan, 3.4e38,
                      -3.4e38, 2.5, -2.5, 4.0, -4.0, 0.5 / 8192, 1.5 / 8192, 2.5 / 8192, 32767.5 / 8192,
                      -32768.5 / 8192, 1e-38, -1e-38], dtype=np.float32)
    rnd = np.random.default_rng(13).integers(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return {"ties": ties, "integers": ints, "edges": edges, "random": rnd}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same_row(got, want_float, what):
    """a delivered row against the oracle's floats: the bits (float row) or mpx16 (int16 row)"""
    want_float = np.asarray(want_float, np.float32)
    if got.dtype == np.int16:
        g, w = got.reshape(-1).astype(np.int64), mpx16(want_float).reshape(-1).astype(np.int64)
    else:
        g, w = _bits(got).reshape(-1).astype(np.int64), _bits(want_float).reshape(-1).astype(np.int64)
    assert g.shape == w.shape, (what, got.shape, want_float.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad.size, [(int(i), int(g[i]), int(w[i]), float(want_float.reshape(-1)[i]))
                                            for i in bad[:6]])


def _station(fmsig, fs, **kw):
    """the default stereo + RDS station as tests/test_gpu_pcm_formats.py builds it"""
    return fmsig.default_params(fs, noise_sigma=0.005, **kw)


def _status_tuple(b, c):
    s = b.status(c)
    vals = (s.tuning_offset, s.interface_level, s.baseband_level, s.pilot_level) + tuple(b.audio_level(c))
    return (s.stereo_detected, s.rds_state) + tuple(int(np.float32(v).view(np.uint32)) for v in vals)


def _shifts(Cn):
    return np.array([(10, 9, 10, 11)[c % 4] for c in range(Cn)], np.int32)


_BLOCKS = {}


def _shared_rows(fmsig, fs, sizes, **kw):
    """the blocks of one station, call after call (computed once per stream)"""
    key = (fs, tuple(sizes), tuple(sorted(kw.items())))
    if key not in _BLOCKS:
        p, rows, start = _station(fmsig, fs, **kw), [], 0
        for n in sizes:
            rows.append(fmsig.generate_f32(p, start, n)[None, :])
            start += n
        _BLOCKS[key] = rows
    return _BLOCKS[key]


_TAPS = {}


def _oracle_taps(oracle, fs, D, shift, rows, key):
    """the oracle's baseband tap of every call for one tuner shift on the shared capture `rows` (once per stream)"""
    key = (key, fs, D, int(shift))
    if key not in _TAPS:
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=int(shift))
        out = []
        for r in rows:
            o.process_stream(r[0])
            out.append(o.taps()["baseband"])
        _TAPS[key] = out
    return _TAPS[key]


class _Rows:
    """pre-filled multiplex rows on the device: [C, stride] elements of the format"""

    def __init__(self, Cn, stride, fmt):
        import torch
        self.s16 = np.dtype(fmt) == np.int16
        self.t = torch.empty((Cn, stride), dtype=torch.int16 if self.s16 else torch.int32, device="cuda")
        self.stride = stride
        self.fill()

    def fill(self):
        import torch
        self.t.fill_(FILL16 if self.s16 else FILL32)
        torch.cuda.current_stream().synchronize()  # (this stream only: calls in flight stay in flight)

    def ptr(self):
        return self.t.data_ptr()

    def host(self, m):
        """(the rows' first m elements in the format, whether everything behind them still holds the fill)"""
        a = self.t.cpu().numpy()
        rest = a[:, m:]
        clean = bool((rest == (FILL16 if self.s16 else FILL32)).all())
        return (a[:, :m].copy() if self.s16 else a[:, :m].copy().view(np.float32)), clean


def _run(pkg, Cn, shifts, rows, sizes, mpx_seq, fs=2.4e6, D=11, mode=2, lag=2, nbuf=6, setup=None, edit=None,
         cmap=None, pcm_seq=None, in_seq=None, every_status=False):
    """One batch with device buffers, calls submitted back to back; call k's multiplex goes to one of nbuf rotating
    pre-filled buffers and is read as soon as fmd_batch_wait_lagged(lag) covers it.  rows[k]: [G, 2 n] float IQ of
    call k (G = 1: one shared capture; converted to in_seq[k]'s dtype where given).  Returns per call the audio, the
    multiplex rows (None where mpx_seq[k] is None) and whether the rows were untouched behind M; the status tuples and
    the RDS groups."""
    import torch
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn, tuning_shifts=shifts,
                  record_callbacks=False)
    b.set_concurrency(mode)
    if setup:
        setup(b)
    if cmap is not None:
        b.set_capture_map(cmap, rows[0].shape[0])
    assert b.mpx_rate() == fs / D
    st = torch.cuda.current_stream().cuda_stream
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    m_stride = (b.max_mpx_samples(max(sizes)) + 7) // 8 * 8 + 24
    ring = [{np.dtype(f): _Rows(Cn, m_stride, f) for f in set(mpx_seq[i::nbuf]) if f is not None}
            for i in range(nbuf)]
    keep, outs, nfs, nms = [], [], [], []
    mpx, clean, status = [None] * len(sizes), [True] * len(sizes), {}
    consumed = 0

    def consume(upto):  # calls [consumed, upto) are complete
        nonlocal consumed
        for k in range(consumed, upto):
            if mpx_seq[k] is not None:
                mpx[k], clean[k] = ring[k % nbuf][np.dtype(mpx_seq[k])].host(nms[k])
        consumed = max(consumed, upto)

    for k, n in enumerate(sizes):
        if edit:
            edit(b, k)
        dt = np.dtype(in_seq[k]) if in_seq else np.dtype(np.float32)
        n_al = (n + 1) // 2 * 2
        x = np.zeros((rows[k].shape[0], 2 * n_al), dt)
        x[:, :2 * n] = _convert(rows[k], dt)
        d_iq = torch.from_numpy(x).cuda()
        pcm = pcm_seq[k] if pcm_seq else np.float32
        d_out = torch.zeros((Cn, a_stride), dtype=torch.int16 if np.dtype(pcm) == np.int16 else torch.float32,
                            device="cuda")
        keep.append(d_iq)
        outs.append(d_out)
        iq_stride = n_al if (cmap is not None or rows[k].shape[0] > 1) else 0
        fmt = {np.dtype(np.float32): pkg.FMD_IQ_F32, np.dtype(np.uint8): pkg.FMD_IQ_U8,
               np.dtype(np.int16): pkg.FMD_IQ_S16}[dt]
        if mpx_seq[k] is None:
            nfs.append(b.process_device(d_iq.data_ptr(), iq_stride, n, d_out.data_ptr(), a_stride, st, fmt=fmt,
                                        pcm=pcm))
            nms.append(0)
        else:
            if k >= nbuf:
                assert consumed > k - nbuf  # the buffer's last call has been read
                ring[k % nbuf][np.dtype(mpx_seq[k])].fill()
            nf, nm = b.process_device(d_iq.data_ptr(), iq_stride, n, d_out.data_ptr(), a_stride, st, fmt=fmt, pcm=pcm,
                                      d_mpx_ptr=ring[k % nbuf][np.dtype(mpx_seq[k])].ptr(), mpx_stride=m_stride,
                                      mpx=mpx_seq[k])
            nfs.append(nf)
            nms.append(nm)
        if mode == 2 and not every_status:
            if k >= lag:
                b.wait(stream=st, lag=lag)
                torch.cuda.current_stream().synchronize()
                consume(k - lag + 1)
        else:
            b.wait(stream=st)
            torch.cuda.synchronize()
            consume(k + 1)
            if every_status:
                status[k] = [_status_tuple(b, c) for c in range(Cn)]
    b.wait(stream=st)
    torch.cuda.synchronize()
    consume(len(sizes))
    audio = [outs[k][:, :nfs[k]].cpu().numpy() for k in range(len(sizes))]
    status["end"] = [_status_tuple(b, c) for c in range(0, Cn, max(1, Cn // 64))]
    groups = b.collect_rds_array(cap=65536, stream=st)
    b.close()
    return {"audio": audio, "mpx": mpx, "clean": clean, "nm": nms, "status": status,
            "groups": np.sort(groups, order=["channel", "call_index"])}


def _convert(rows, dt):
    if dt == np.dtype(np.float32):
        return rows
    if dt == np.dtype(np.int16):
        return np.clip(np.rint(rows.astype(np.float64) * 32767), -32768, 32767).astype(np.int16)
    return np.clip(np.rint((rows.astype(np.float64) + 1.0) * 127.5), 0, 255).astype(np.uint8)


def _as_float_iq(oracle, x, dt):
    """the float block the library decodes for an input block of dtype dt"""
    if dt == np.dtype(np.uint8):
        return oracle.convert_u8(x)
    if dt == np.dtype(np.int16):
        return x.astype(np.float32) * np.float32(2.0 ** -15)
    return x


def _baseband_lengths(sizes, D):
    """the decimator's outputs per call (DownConvert.cpp:112-132)"""
    pos, out = 0, []
    for n in sizes:
        m = (n - pos + D - 1) // D
        out.append(m)
        pos = pos + m * D - n
    return out


# ---------------------------------------------------------------------------------------------------------------
# 1. every value through the device build of the conversion

@pytest.mark.parametrize("name", ["ties", "integers", "edges", "random"])
def test_device_build_of_the_conversion_equals_mpx16(pkg, name):
    x = value_sets()[name]
    got, zero = pkg.debug_math(9, x)
    want = mpx16(x).astype(np.float32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad.size, [(float(x[i]), float(got[i]), float(want[i])) for i in bad[:8]])
    assert not zero.any()
    if name == "random":
        assert np.isnan(x).any() and (np.abs(x) < np.float32(1.2e-38)).any() and (np.abs(want) == 32768).any()


# ---------------------------------------------------------------------------------------------------------------
# 2. single decoder against the oracle

@pytest.mark.parametrize("fs,D,dev", [(2.4e6, 11, None), (2.4e6, 6, 300e3), (1.0e6, 4, 300e3)],
                         ids=["2p4M-D11", "2p4M-D6-dev300k", "1p0M-D4-dev300k"])
def test_single_decoder_equals_the_oracles_baseband(pkg, oracle, fmsig, fs, D, dev):
    """cFmDecoder surface, 12 calls of 65 536 samples: ProcessStreamWithMpx's float row is the oracle's baseband tap
    bit for bit, its int16 row is mpx16 of the tap; audio, UECP frames, PS name and stereo flag equal those of a
    decoder that never asked for the multiplex.  The streams hold what makes the comparison bite (asserted from the
    oracle's floats): ties, saturation at both ends (D 6), both row lengths, and samples on which round-half-away,
    truncation and a scale of 16384 each give another integer."""
    p = _station(fmsig, fs, **({"dev": dev} if dev else {}))
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    d32 = pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    d16 = pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    dn = pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    assert d32.batch_view().mpx_rate() == fs / D
    taps = []
    for blk in range(12):
        x = fmsig.generate_f32(p, blk * N, N)
        ref = o.process_stream(x)
        tap = o.taps()["baseband"]
        a32, m32 = d32.ProcessStreamWithMpx(x.view(np.complex64))
        a16, m16 = d16.ProcessStreamWithMpx(x.view(np.complex64), mpx=np.int16)
        an = dn.ProcessStream(x.view(np.complex64))
        assert m32.dtype == np.float32 and m16.dtype == np.int16
        _same_row(m32, tap, "float row of block %d" % blk)
        _same_row(m16, tap, "int16 row of block %d" % blk)
        assert _bits_equal(a32, ref) and _bits_equal(a16, ref) and _bits_equal(an, ref), blk
        taps.append(tap)
    for d in (d32, d16):
        assert d.sink.frames.get(0, []) == o.uecp_frames() == dn.sink.frames.get(0, [])
        assert (d.sink.names.get(0) or "") == o.channel_name() == (dn.sink.names.get(0) or "")
        assert d.StereoDetected() == bool(o.status().stereo) == dn.StereoDetected()
    # the data, from the oracle's floats
    lens = [t.size for t in taps]
    assert lens == _baseband_lengths([N] * 12, D)
    if D == 11:
        assert lens[5] == lens[10] == 5957 and set(lens) == {5957, 5958}  # calls 6 and 11
    elif D == 6:
        assert set(lens) == {10922, 10923}
    else:
        assert set(lens) == {16384}
    x = np.concatenate(taps)
    y = x.astype(np.float64) * 8192.0  # exact
    want = mpx16(x).astype(np.int64)
    n_tie = int(((y - np.floor(y)) == 0.5).sum())
    r = np.rint(y)
    n_hi, n_lo = int((r > 32767).sum()), int((r < -32768).sum())
    away = np.clip(np.sign(y) * np.floor(np.abs(y) + 0.5), -32768, 32767).astype(np.int64)
    trunc = np.clip(np.trunc(y), -32768, 32767).astype(np.int64)
    s16384 = np.clip(np.rint(x.astype(np.float64) * 16384.0), -32768, 32767).astype(np.int64)
    differ = [int((v != want).sum()) for v in (away, trunc, s16384)]
    print("samples %d ties %d saturated high %d low %d; half-away / truncation / 16384 differ on %s"
          % (x.size, n_tie, n_hi, n_lo, differ))
    assert n_tie >= 1
    if D == 6:
        assert n_hi >= 1 and n_lo >= 1
    assert all(n >= 1 for n in differ), differ


# ---------------------------------------------------------------------------------------------------------------
# 3. ragged rows

@pytest.mark.parametrize("n", [8192, N])
@pytest.mark.parametrize("Cn", [1, 63, 65, 130])
def test_ragged_rows_hold_their_samples_and_nothing_else(pkg, oracle, fmsig, Cn, n):
    """Batches that end inside a wave, at a wave and one channel behind it, calls whose baseband length leaves 0 to 3
    (float) and 0 to 7 (int16) samples behind the last 16-byte group and ends inside a tile, an odd length among
    them (2.4 MS/s and D 11: 5957 in call 6, 745 / 744 with calls of 8192); strides above the length, rows pre-filled:
    every row is the oracle's in its M elements and untouched behind them, in both formats."""
    fs, D = 2.4e6, 11
    sizes = [n] * (6 if n == N else 4)
    rows, shifts = _shared_rows(fmsig, fs, sizes), _shifts(Cn)
    want_m = _baseband_lengths(sizes, D)
    assert any(m % 2 for m in want_m) and len(set(want_m)) == 2
    for fmt in (np.float32, np.int16):
        r = _run(pkg, Cn, shifts, rows, sizes, [fmt] * len(sizes), mode=1)
        assert r["nm"] == want_m
        assert all(r["clean"]), r["clean"]
        for k in range(len(sizes)):
            assert r["mpx"][k].shape == (Cn, want_m[k])
            for s in sorted(set(int(v) for v in shifts)):
                tap = _oracle_taps(oracle, fs, D, s, rows, ("ragged", n))[k]
                ch = np.flatnonzero(shifts == s)
                _same_row(r["mpx"][k][ch], np.broadcast_to(tap, (ch.size, tap.size)), (fmt, k, s))
    assert {m % 4 for m in want_m} | {m % 8 for m in want_m} >= ({1, 0} if n == 8192 else {1, 2, 5, 6})


def test_refused_rows_leave_the_batch_as_it_was(pkg, oracle, fmsig):
    """A misaligned pointer, a stride that is no multiple of 4 / 8 elements, a stride below the call's length and a
    format outside the enum give FMD_ERR_ARG and a sentence; the next call -- with a channel reset pending across the
    refusals -- delivers what the oracle delivers for an uninterrupted stream."""
    import torch
    fs, D, Cn = 2.4e6, 11, 2
    sizes = [N, N, N]
    rows = _shared_rows(fmsig, fs, sizes)
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn, record_callbacks=False)
    o = [oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D) for _ in range(Cn)]
    a_stride = (b.max_audio_floats(N) + 7) // 8 * 8
    audio = torch.zeros((Cn, a_stride), dtype=torch.float32, device="cuda")
    assert b.max_mpx_samples(N) == 5958 and b.max_mpx_samples(8192) == 745
    for k, n in enumerate(sizes):
        iq = torch.from_numpy(rows[k]).cuda()
        if k == 1:
            b.reset_channels([1])
            o[1].reset()
        m = _baseband_lengths(sizes, D)[k]
        for fmt, per in ((np.float32, 4), (np.int16, 8)):
            good = _Rows(Cn, 6016, fmt)
            esz = 2 if per == 8 else 4
            with pytest.raises(pkg.FmdError, match="fmd error -1: .*16-byte aligned"):
                b.process_device(iq.data_ptr(), 0, n, audio.data_ptr(), a_stride, d_mpx_ptr=good.ptr() + esz,
                                 mpx_stride=6000, mpx=fmt)
            with pytest.raises(pkg.FmdError, match="fmd error -1: .*multiple of 4"):
                b.process_device(iq.data_ptr(), 0, n, audio.data_ptr(), a_stride, d_mpx_ptr=good.ptr(),
                                 mpx_stride=6000 + per // 2, mpx=fmt)
            with pytest.raises(pkg.FmdError, match="fmd error -1: .*smaller than the call's baseband length"):
                b.process_device(iq.data_ptr(), 0, n, audio.data_ptr(), a_stride, d_mpx_ptr=good.ptr(),
                                 mpx_stride=(m - 1) // per * per, mpx=fmt)
            assert len(pkg.lib().fmd_last_error().split()) >= 5
            nf, nm = C.c_uint(), C.c_uint()
            assert pkg.lib().fmd_batch_process_device_mpx(b._h, iq.data_ptr(), 0, 0, n, audio.data_ptr(), 0, a_stride,
                                                          C.byref(nf), good.ptr(), 2, 6016, C.byref(nm), None) == -1
            assert good.host(0)[1]  # nothing was written
        good = _Rows(Cn, 5960, np.int16 if k == 1 else np.float32)
        nf, nm = b.process_device(iq.data_ptr(), 0, n, audio.data_ptr(), a_stride, d_mpx_ptr=good.ptr(),
                                  mpx_stride=5960, mpx=np.int16 if k == 1 else np.float32)
        torch.cuda.synchronize()
        got, clean = good.host(nm)
        assert nm == m and clean
        a = audio[:, :nf].cpu().numpy()
        for c in range(Cn):
            assert _bits_equal(a[c], o[c].process_stream(rows[k][0])), (k, c)
            _same_row(got[c], o[c].taps()["baseband"], (k, c))
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. calls in flight

_FLIGHT_SIZES = [N, N, 30001, N, N, 8193, N, N, N, 20001, N, N]


@pytest.fixture(scope="module")
def serial_rows(pkg, fmsig):
    """the 130-channel batch in serial mode (everything on the caller's stream), float rows of every call"""
    rows, shifts = _shared_rows(fmsig, 2.4e6, _FLIGHT_SIZES), _shifts(130)
    return _run(pkg, 130, shifts, rows, _FLIGHT_SIZES, [np.float32] * 12, mode=0)


@pytest.mark.parametrize("lag", [1, 2, 3])
@pytest.mark.parametrize("how", ["default", "split_post", "lpf_late0", "lpf_late1", "lpf_late2"])
def test_rows_of_calls_in_flight(pkg, oracle, fmsig, serial_rows, how, lag):
    """130 channels, concurrency 2, 12 calls into 6 rotating pre-filled buffers, float and int16 rows alternating, each
    read as soon as fmd_batch_wait_lagged(lag) covers its call: every row of every call equals the serial-mode
    batch's, and both equal the oracle (every channel: four tuner shifts on one capture, channels 0, 64 and 129 among
    them); the audio is the serial batch's too.  With the post chain on two streams and with each stream layout."""
    fs, D, Cn = 2.4e6, 11, 130
    sizes = _FLIGHT_SIZES
    rows, shifts = _shared_rows(fmsig, fs, sizes), _shifts(Cn)
    setup = {"default": None, "split_post": lambda b: b.debug_set("split_post", 1),
             "lpf_late0": lambda b: b.debug_set("lpf_late", 0), "lpf_late1": lambda b: b.debug_set("lpf_late", 1),
             "lpf_late2": lambda b: b.debug_set("lpf_late", 2)}[how]
    seq = [np.float32 if k % 2 == 0 else np.int16 for k in range(len(sizes))]
    r = _run(pkg, Cn, shifts, rows, sizes, seq, mode=2, lag=lag, nbuf=6, setup=setup)
    assert r["nm"] == serial_rows["nm"] == _baseband_lengths(sizes, D)
    assert all(r["clean"]) and all(serial_rows["clean"])
    for k in range(len(sizes)):
        _same_row(r["mpx"][k], serial_rows["mpx"][k], ("against the serial batch", k))
        assert _bits_equal(r["audio"][k], serial_rows["audio"][k]), k
        for c in (0, 64, 129, 1, 3):
            tap = _oracle_taps(oracle, fs, D, shifts[c], rows, "flight")[k]
            _same_row(serial_rows["mpx"][k][c], tap, ("serial batch against the oracle", k, c))
            _same_row(r["mpx"][k][c], tap, ("against the oracle", k, c))
    assert r["status"]["end"] == serial_rows["status"]["end"]
    assert len(r["groups"]) > 0 and np.array_equal(r["groups"], serial_rows["groups"])


# ---------------------------------------------------------------------------------------------------------------
# 5. the benchmark's dispatch

@pytest.mark.parametrize("sizes", [[16384] * 3, [N] * 2], ids=["3x16384", "2x65536"])
def test_dispatch_4160_channels(pkg, oracle, fmsig, sizes):
    """4160 channels on one shared capture, calls in flight: the whole-CU serial stage and k_halfband_chain without
    mixed rows (and, with calls of 65 536, the ring resampler beside the writer).  Every channel equals the channel of
    the same tuner shift in a 130-channel batch, whose channels are held against the oracle here."""
    fs, D, Cn = 2.4e6, 11, 4160
    rows = _shared_rows(fmsig, fs, sizes)
    small = _run(pkg, 130, _shifts(130), rows, sizes, [np.float32] * len(sizes))
    for c in range(4):
        for k in range(len(sizes)):
            _same_row(small["mpx"][k][c], _oracle_taps(oracle, fs, D, _shifts(4)[c], rows, ("4160", len(sizes)))[k],
                      ("130 channels against the oracle", k, c))
    shifts = _shifts(Cn)
    for fmt in (np.float32, np.int16):
        r = _run(pkg, Cn, shifts, rows, sizes, [fmt] * len(sizes), nbuf=3)
        assert r["nm"] == small["nm"] and all(r["clean"])
        for k in range(len(sizes)):
            _same_row(r["mpx"][k], small["mpx"][k][np.arange(Cn) % 4], (fmt, k))
            assert _bits_equal(r["audio"][k], small["audio"][k][np.arange(Cn) % 4]), k


def test_dispatch_16384_channels_as_sub_batches(pkg, oracle, fmsig):
    """A shell over two sub-batches, 2 calls of 8192 samples: every sub-batch's rows start ch0 * stride elements into
    the caller's buffer -- the first and the last channel of each sub-batch (and every other one) are compared."""
    fs, D, Cn = 2.4e6, 11, 16384
    sizes = [8192, 8192]
    rows = _shared_rows(fmsig, fs, sizes)
    small = _run(pkg, 130, _shifts(130), rows, sizes, [np.float32] * 2)
    for c in range(4):
        for k in range(2):
            _same_row(small["mpx"][k][c], _oracle_taps(oracle, fs, D, _shifts(4)[c], rows, "shell")[k], (k, c))
    for fmt in (np.float32, np.int16):
        r = _run(pkg, Cn, _shifts(Cn), rows, sizes, [fmt] * 2, nbuf=3)
        assert r["nm"] == small["nm"] and all(r["clean"])
        for k in range(2):
            for c in (0, 8191, 8192, 16383):
                _same_row(r["mpx"][k][c], small["mpx"][k][c % 4], (fmt, k, c))
            _same_row(r["mpx"][k], small["mpx"][k][np.arange(Cn) % 4], (fmt, k))


# ---------------------------------------------------------------------------------------------------------------
# 6. the format belongs to the call

def test_a_format_per_call_changes_nothing_else(pkg, oracle, fmsig):
    """Calls alternate no / float / int16 multiplex with float / int16 audio and byte / int16 / float IQ: audio,
    status record and audio meter after EVERY call and the RDS groups equal those of a batch that never asked for
    the multiplex; the rows of channel 0 equal the oracle fed the converted blocks."""
    fs, D, Cn = 2.4e6, 11, 3
    sizes = [N, 30001, N, 8193, N, N, 20001, N, N, N, 33333, N]
    ps = [_station(fmsig, fs, seed=40 + c, pi=0x4200 + c, **({"dev": 150e3} if c == 1 else {})) for c in range(Cn)]
    rows, start = [], 0
    for n in sizes:
        rows.append(np.stack([fmsig.generate_f32(ps[c], start, n) for c in range(Cn)]))
        start += n
    mpx_seq = [(None, np.float32, np.int16)[k % 3] for k in range(len(sizes))]
    pcm_seq = [(np.float32, np.int16)[k % 2] for k in range(len(sizes))]
    in_seq = [(np.uint8, np.int16, np.int16, np.uint8)[k % 4] for k in range(len(sizes))]
    kw = dict(pcm_seq=pcm_seq, in_seq=in_seq, every_status=True)
    plain = _run(pkg, Cn, None, rows, sizes, [None] * len(sizes), **kw)
    r = _run(pkg, Cn, None, rows, sizes, mpx_seq, **kw)
    assert {(m, np.dtype(p), np.dtype(i)) for m, p, i in zip(mpx_seq, pcm_seq, in_seq)} >= {
        (f, np.dtype(p), np.dtype(i)) for f in (np.float32, np.int16) for p in (np.float32, np.int16)
        for i in (np.uint8, np.int16)}
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    for k, n in enumerate(sizes):
        assert r["audio"][k].dtype == plain["audio"][k].dtype and r["audio"][k].shape == plain["audio"][k].shape
        assert np.array_equal(np.ascontiguousarray(r["audio"][k]).view(np.uint16),
                              np.ascontiguousarray(plain["audio"][k]).view(np.uint16)), k
        assert r["status"][k] == plain["status"][k], k
        o.process_stream(_as_float_iq(oracle, _convert(rows[k][0], np.dtype(in_seq[k])), np.dtype(in_seq[k])))
        if mpx_seq[k] is None:
            assert r["mpx"][k] is None and r["nm"][k] == 0
        else:
            assert r["clean"][k]
            _same_row(r["mpx"][k][0], o.taps()["baseband"], k)
    assert r["status"]["end"] == plain["status"]["end"]
    assert len(plain["groups"]) > 0 and np.array_equal(r["groups"], plain["groups"])


# ---------------------------------------------------------------------------------------------------------------
# 7. edited channels

@pytest.mark.parametrize("fmt", [np.float32, np.int16], ids=["f32", "s16"])
def test_reset_and_retuned_channels_deliver_the_decoder_they_now_are(pkg, oracle, fmsig, fmt):
    """130 channels with calls in flight, retuning enabled (the silent twin's multiplex is not written): in front of
    call 2 one channel is reset and one retuned, in front of call 3 another pair.  The reset channel's rows are those
    of the oracle decoder that was Reset() there, the retuned channel's those of a decoder of the new shift that heard
    zeros until then; their neighbours in the same wave are unchanged."""
    fs, D, Cn = 2.4e6, 11, 130
    sizes = [N, N, 30001, N, N]
    rows, shifts = _shared_rows(fmsig, fs, sizes), _shifts(Cn)
    reset_at, retune_at = {5: 2, 70: 3}, {6: (2, 9), 129: (3, 11)}  # channel: call (, new shift)

    def edit(b, k):
        for c, (at, sh) in retune_at.items():
            if at == k:
                b.retune([c], [sh])
        for c, at in reset_at.items():
            if at == k:
                b.reset_channels([c])

    r = _run(pkg, Cn, shifts, rows, sizes, [fmt] * len(sizes), setup=lambda b: b.enable_retune(), edit=edit)
    assert all(r["clean"])
    for c in (4, 5, 6, 7, 69, 70, 71, 128, 129):
        sh = retune_at[c][1] if c in retune_at else int(shifts[c])
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=sh)
        for k, n in enumerate(sizes):
            if reset_at.get(c) == k:
                o.reset()
            if c in retune_at and k < retune_at[c][0]:  # a decoder of the new shift that received zeros until now
                o.process_stream(np.zeros(2 * n, np.float32))
                continue
            o.process_stream(rows[k][0])
            _same_row(r["mpx"][k][c], o.taps()["baseband"], (c, k))
    # a retuned channel before its retune is the decoder of its old shift
    for c, (at, sh) in retune_at.items():
        for k in range(at):
            _same_row(r["mpx"][k][c], _oracle_taps(oracle, fs, D, shifts[c], rows, "edits")[k], (c, k))


def test_switched_channels_deliver_the_spliced_stream(pkg, oracle, fmsig):
    """130 channels on 3 captures through a shuffled capture map, calls in flight: three channels move to another
    capture in front of call 2 -- their rows are the oracle's on the spliced stream, their neighbours' unchanged."""
    fs, D, Cn, G = 2.4e6, 11, 130, 3
    sizes = [N, N, 30001, N]
    sts = [_station(fmsig, fs, seed=300 + g, pi=0x7100 + g) for g in range(G)]
    rows, start = [], 0
    for n in sizes:
        rows.append(np.stack([fmsig.generate_f32(sts[g], start, n) for g in range(G)]))
        start += n
    shifts = _shifts(Cn)
    cmap = np.random.default_rng(7).permutation(Cn) % G
    moved = {0: int((cmap[0] + 1) % G), 64: int((cmap[64] + 2) % G), 129: int((cmap[129] + 1) % G)}

    def edit(b, k):
        if k == 2:
            b.switch_captures(np.array(list(moved), np.uint32), np.array(list(moved.values()), np.uint32))

    seq = [np.float32, np.int16, np.int16, np.float32]
    r = _run(pkg, Cn, shifts, rows, sizes, seq, cmap=cmap, edit=edit)
    assert all(r["clean"])
    for c in (0, 1, 63, 64, 65, 128, 129):
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=int(shifts[c]))
        for k in range(len(sizes)):
            g = moved[c] if (c in moved and k >= 2) else int(cmap[c])
            o.process_stream(rows[k][g])
            _same_row(r["mpx"][k][c], o.taps()["baseband"], (c, k))


# ---------------------------------------------------------------------------------------------------------------
# 8. host entry point and Python

def test_host_entry_point_takes_any_stride(pkg, oracle, fmsig):
    """fmd_batch_process_host_mpx copies rows: an odd stride and an unaligned pointer are fine; Batch.process_host_fmt
    (mpx=...) returns (audio, rows); formats alternate, calls without the multiplex in between; a stride below the
    call's length is refused and changes nothing."""
    fs, D, Cn = 2.4e6, 11, 3
    ps = [_station(fmsig, fs, seed=70 + c, **({"dev": 300e3} if c == 1 else {})) for c in range(Cn)]
    refs = [oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D) for _ in range(Cn)]
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn)
    assert b.mpx_rate() == fs / D == pytest.approx(218181.8, abs=0.05)
    start = 0
    for k, n in enumerate([N, 20001, 8192, 33333, N, N]):
        x = np.stack([fmsig.generate_f32(ps[c], start, n) for c in range(Cn)])
        start += n
        want_a = [refs[c].process_stream(x[c]) for c in range(Cn)]
        want_m = [refs[c].taps()["baseband"] for c in range(Cn)]
        m = want_m[0].size
        if k % 3 == 0:
            s16 = k == 3
            stride = b.max_mpx_samples(n) + 3  # odd
            buf = np.full(Cn * stride + 1, FILL16 if s16 else FILL32, np.int16 if s16 else np.int32)
            out = buf[1:]  # 2- / 4-byte aligned only
            a_stride = b.max_audio_floats(n)
            audio = np.zeros((Cn, a_stride), np.float32)
            nf, nm = C.c_uint(), C.c_uint()
            args = (b._h, x.ctypes.data, pkg.FMD_IQ_F32, n, n, audio.ctypes.data, pkg.FMD_PCM_F32, a_stride,
                    C.byref(nf), out.ctypes.data, pkg.FMD_MPX_S16 if s16 else pkg.FMD_MPX_F32)
            assert pkg.lib().fmd_batch_process_host_mpx(*args, m - 1, C.byref(nm)) == -1
            assert b"smaller than the call's baseband length" in pkg.lib().fmd_last_error()
            rc = pkg.lib().fmd_batch_process_host_mpx(*args, stride, C.byref(nm))
            assert rc >= 0, pkg.lib().fmd_last_error()
            assert nm.value == m
            got = out.reshape(Cn, stride)
            for c in range(Cn):
                _same_row(got[c, :m] if s16 else got[c, :m].view(np.float32), want_m[c], (k, c))
                assert _bits_equal(audio[c, :nf.value], want_a[c]), (k, c)
            assert (got[:, m:] == (FILL16 if s16 else FILL32)).all() and buf[0] == (FILL16 if s16 else FILL32)
        elif k % 3 == 1:
            a, rows = b.process_host_fmt(x, mpx=np.int16 if k == 1 else np.float32,
                                         pcm=np.int16 if k == 4 else None)
            assert rows.shape == (Cn, m) and rows.dtype == (np.int16 if k == 1 else np.float32)
            for c in range(Cn):
                _same_row(rows[c], want_m[c], (k, c))
                if k == 1:
                    assert _bits_equal(a[c], want_a[c]), (k, c)
        else:
            a = b.process_host_fmt(x)
            for c in range(Cn):
                assert _bits_equal(a[c], want_a[c]), (k, c)
    b.close()
