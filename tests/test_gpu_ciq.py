"""Every channel's IF-filtered IQ beside the other outputs (FMD_CIQ_*, the call record of include/fmd.h): the rows of
the tuner and decimating IF filter, copied into one row per channel by k_ciq_out, as float pairs or as pairs of 16-bit
integers.

The contract needs no tolerance.  FMD_CIQ_F32 is the complex float the oracle's `demod` tap holds (m_BufferIF behind
cDownsampleFilter::Process), bit for bit; FMD_CIQ_S16 is mpx16() of its real and imaginary parts.  Expected values are
the CPU oracle's tap; where the channel count is beyond the oracle's reach they are the rows of the product's own
130-channel float batch, itself compared with the oracle in the same test; never the output under test.  Buffers are
pre-filled and everything behind a row's M samples, and every row the call does not deliver, must still hold the fill.
Every comparison is an equality.
"""
import ctypes as C

import numpy as np
import pytest

import edit_model as em
from __graft_entry__ import load_package
from feed_spec import mpx16

pytestmark = pytest.mark.gpu

N = 65536
FILL16 = 0x5A5A
FILL32 = 0x5A5A5A5A


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_rows(got, want, what):
    """delivered rows against the oracle's complex floats: the bits (complex64 rows) or mpx16 of both parts (int16
    rows [.., 2])"""
    want = np.ascontiguousarray(want, np.complex64)
    if got.dtype == np.int16:
        w = np.stack([mpx16(want.real), mpx16(want.imag)], axis=-1).astype(np.int64)
        g = got.astype(np.int64)
    else:
        assert got.dtype == np.complex64, got.dtype
        w = want.view(np.uint32).astype(np.int64)
        g = np.ascontiguousarray(got).view(np.uint32).astype(np.int64)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, (what, bad.size, [(int(i), int(g.reshape(-1)[i]), int(w.reshape(-1)[i])) for i in bad[:6]])


def _station(fmsig, fs, **kw):
    return fmsig.default_params(fs, noise_sigma=0.005, **kw)


def _status_tuple(b, c):
    s = b.status(c)
    vals = (s.tuning_offset, s.interface_level, s.baseband_level, s.pilot_level) + tuple(b.audio_level(c))
    return (s.stereo_detected, s.rds_state) + tuple(int(np.float32(v).view(np.uint32)) for v in vals)


def _shifts(Cn):
    return np.array([(10, 9, 10, 11)[c % 4] for c in range(Cn)], np.int32)


_BLOCKS, _TAPS = {}, {}


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


def _oracle_taps(oracle, fs, D, shift, rows, key):
    """the oracle's demod tap of every call for one tuner shift on the shared capture `rows` (once per stream)"""
    key = (key, fs, D, int(shift))
    if key not in _TAPS:
        o = oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, tuning_shift=int(shift))
        out = []
        for r in rows:
            o.process_stream(r[0])
            out.append(o.taps()["demod"])
        o.close()
        _TAPS[key] = out
    return _TAPS[key]


def _want_all(oracle, fs, D, shifts, rows, key, k):
    """[C, M] complex64: the oracle's rows of call k for every channel of `shifts`"""
    per = {int(s): _oracle_taps(oracle, fs, D, s, rows, key)[k] for s in set(int(v) for v in shifts)}
    return np.stack([per[int(s)] for s in shifts])


class _Rows:
    """pre-filled channel IQ rows on the device: [rows, stride] complex samples of the format"""

    def __init__(self, n_rows, stride, fmt):
        import torch
        self.s16 = np.dtype(fmt) == np.int16
        self.t = torch.empty((n_rows, 2 * stride), dtype=torch.int16 if self.s16 else torch.int32, device="cuda")
        self.stride = stride
        self.fill()

    def fill(self):
        import torch
        self.t.fill_(FILL16 if self.s16 else FILL32)
        torch.cuda.current_stream().synchronize()  # (this stream only: calls in flight stay in flight)

    def ptr(self):
        return self.t.data_ptr()

    def host(self, n_rows, m):
        """(the first m samples of the first n_rows rows in the format, whether everything else still holds the fill)"""
        a = self.t.cpu().numpy()
        fill = FILL16 if self.s16 else FILL32
        clean = bool((a[:n_rows, 2 * m:] == fill).all() and (a[n_rows:] == fill).all())
        got = a[:n_rows, :2 * m].copy()
        return (got.reshape(n_rows, m, 2) if self.s16 else got.view(np.complex64)), clean


def _convert(rows, dt):
    if dt == np.dtype(np.float32):
        return rows
    if dt == np.dtype(np.int16):
        return np.clip(np.rint(rows.astype(np.float64) * 32767), -32768, 32767).astype(np.int16)
    return np.clip(np.rint((rows.astype(np.float64) + 1.0) * 127.5), 0, 255).astype(np.uint8)


def _as_float_iq(oracle, x, dt):
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


def _run(pkg, Cn, shifts, rows, sizes, ciq_seq, fs=2.4e6, D=11, mode=2, lag=2, nbuf=6, setup=None, sel_seq=None,
         cmap=None, pcm_seq=None, in_seq=None, every_status=False):
    """One batch with device buffers, calls submitted back to back; call k's channel IQ goes to one of nbuf rotating
    pre-filled buffers and is read as soon as fmd_batch_wait_lagged(lag) covers it.  sel_seq[k] (where given): the
    selection set in front of call k (None: every channel).  Returns per call the audio, the rows (None where ciq_seq[k]
    is None), whether the buffer was untouched everywhere else, the counts; the status tuples and the RDS groups."""
    import torch
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn, tuning_shifts=shifts,
                  record_callbacks=False)
    b.set_concurrency(mode)
    if setup:
        setup(b)
    if cmap is not None:
        b.set_capture_map(cmap, rows[0].shape[0])
    st = torch.cuda.current_stream().cuda_stream
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    q_stride = (b.max_mpx_samples(max(sizes)) + 3) // 4 * 4 + 12
    ring = [{np.dtype(f): _Rows(Cn, q_stride, f) for f in set(ciq_seq[i::nbuf]) if f is not None} for i in range(nbuf)]
    keep, outs, nfs, nqs, nrows = [], [], [], [], []
    ciq, clean, status = [None] * len(sizes), [True] * len(sizes), {}
    consumed = 0

    def consume(upto):  # calls [consumed, upto) are complete
        nonlocal consumed
        for k in range(consumed, upto):
            if ciq_seq[k] is not None:
                ciq[k], clean[k] = ring[k % nbuf][np.dtype(ciq_seq[k])].host(nrows[k], nqs[k])
        consumed = max(consumed, upto)

    for k, n in enumerate(sizes):
        if sel_seq is not None:
            b.select_ciq(sel_seq[k])
            assert b.ciq_selection().tolist() == (list(range(Cn)) if sel_seq[k] is None else list(sel_seq[k]))
        nrows.append(Cn if sel_seq is None or sel_seq[k] is None else len(sel_seq[k]))
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
        if ciq_seq[k] is None:
            nfs.append(b.process_device(d_iq.data_ptr(), iq_stride, n, d_out.data_ptr(), a_stride, st, fmt=fmt,
                                        pcm=pcm))
            nqs.append(0)
        else:
            if k >= nbuf:
                assert consumed > k - nbuf  # the buffer's last call has been read
                ring[k % nbuf][np.dtype(ciq_seq[k])].fill()
            nf, nq = b.process_device(d_iq.data_ptr(), iq_stride, n, d_out.data_ptr(), a_stride, st, fmt=fmt, pcm=pcm,
                                      d_ciq_ptr=ring[k % nbuf][np.dtype(ciq_seq[k])].ptr(), ciq_stride=q_stride,
                                      ciq=ciq_seq[k])
            nfs.append(nf)
            nqs.append(nq)
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
    return {"audio": audio, "ciq": ciq, "clean": clean, "nq": nqs, "status": status,
            "groups": np.sort(groups, order=["channel", "call_index"])}


# ---------------------------------------------------------------------------------------------------------------
# 1. single decoder against the oracle

@pytest.mark.parametrize("fs,D", [(2.4e6, 11), (1.0e6, 4)], ids=["2p4M-D11", "1p0M-D4"])
def test_single_decoder_equals_the_oracles_demod_tap(pkg, oracle, fmsig, fs, D):
    """fmd_process_stream_call through FmDecoder.ProcessStreamWithChannelIq, 8 calls of 65 536 samples: the float row is
    the oracle's demod tap bit for bit, the int16 row mpx16 of its parts; audio, UECP frames and the stereo flag equal
    those of a decoder that never asked for the rows."""
    p = _station(fmsig, fs)
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    d32, d16, dn = (pkg.FmDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D) for _ in range(3))
    lens = []
    for blk in range(8):
        x = fmsig.generate_f32(p, blk * N, N)
        ref = o.process_stream(x)
        tap = o.taps()["demod"]
        a32, q32 = d32.ProcessStreamWithChannelIq(x.view(np.complex64))
        a16, q16 = d16.ProcessStreamWithChannelIq(x.view(np.complex64), ciq=np.int16)
        an = dn.ProcessStream(x.view(np.complex64))
        assert q32.dtype == np.complex64 and q16.dtype == np.int16 and q16.shape == (tap.size, 2)
        _same_rows(q32, tap, "float row of block %d" % blk)
        _same_rows(q16, tap, "int16 row of block %d" % blk)
        assert _bits_equal(a32, ref) and _bits_equal(a16, ref) and _bits_equal(an, ref), blk
        lens.append(tap.size)
    assert lens == _baseband_lengths([N] * 8, D)
    for d in (d32, d16):
        assert d.sink.frames.get(0, []) == o.uecp_frames() == dn.sink.frames.get(0, [])
        assert d.StereoDetected() == bool(o.status().stereo) == dn.StereoDetected()
    # a selection is the batch's, not the decoder's
    with pytest.raises(pkg.FmdError, match="fmd error -4: fmd_batch_select_ciq"):
        d32.batch_view().select_ciq([0])


# ---------------------------------------------------------------------------------------------------------------
# 2. the record call without the rows is the _feed call

def test_record_without_ciq_is_the_feed_entry_point(pkg, fmsig):
    """Two batches, the same six calls with audio (int16 / float), multiplex and feed: one through
    fmd_batch_process_device_feed, one through fmd_batch_process_device_call with ciq.p == NULL.  Every output, count and
    status tuple is equal, and both profiled timelines have the same calls and stages (fmd_batch_debug_timeline)."""
    import torch
    fs, D, Cn = 2.4e6, 11, 1024  # (the timeline exists from 1024 channels on: the whole-CU serial stage)
    sizes = [N, 30001, 8193, N, 20001, N]
    rows, shifts = _shared_rows(fmsig, fs, sizes), _shifts(Cn)
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for record in (False, True):
        b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn, tuning_shifts=shifts,
                      record_callbacks=False)
        b.set_concurrency(2)
        b.set_feed(2)
        b.set_profiling(1)
        a_stride, m_stride = (b.max_audio_floats(N) + 63) // 64 * 64, 5960
        f_stride = (b.max_feed_samples(N) + 8) // 8 * 8
        out = []
        for k, n in enumerate(sizes):
            s16 = k % 2 == 1
            iq = torch.from_numpy(rows[k]).cuda()
            audio = torch.zeros((Cn, a_stride), dtype=torch.int16 if s16 else torch.float32, device="cuda")
            mpx = torch.full((Cn, m_stride), 77, dtype=torch.int16 if s16 else torch.float32, device="cuda")
            feed = torch.full((Cn, f_stride), 77, dtype=torch.float32 if s16 else torch.int16, device="cuda")
            fmts = (pkg.FMD_PCM_S16 if s16 else pkg.FMD_PCM_F32, pkg.FMD_MPX_S16 if s16 else pkg.FMD_MPX_F32,
                    pkg.FMD_FEED_F32 if s16 else pkg.FMD_FEED_S16)
            nf, nm, nfeed, nq = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint(9)
            if record:
                b.process_call(pkg.make_call(iq.data_ptr(), pkg.FMD_IQ_F32, 0, n, stream=st,
                                             audio=pkg.make_rows(audio.data_ptr(), fmts[0], a_stride, nf),
                                             mpx=pkg.make_rows(mpx.data_ptr(), fmts[1], m_stride, nm),
                                             feed=pkg.make_rows(feed.data_ptr(), fmts[2], f_stride, nfeed),
                                             ciq=pkg.make_rows(None, k % 2, 0, nq)))
                assert nq.value == 0
            else:
                rc = pkg.lib().fmd_batch_process_device_feed(
                    b._h, iq.data_ptr(), pkg.FMD_IQ_F32, 0, n, audio.data_ptr(), fmts[0], a_stride, C.byref(nf),
                    mpx.data_ptr(), fmts[1], m_stride, C.byref(nm), feed.data_ptr(), fmts[2], f_stride,
                    C.byref(nfeed), st)
                assert rc == 0, pkg.lib().fmd_last_error()
            b.wait(stream=st)
            torch.cuda.synchronize()
            out.append((nf.value, nm.value, nfeed.value, audio.cpu().numpy().tobytes(), mpx.cpu().numpy().tobytes(),
                        feed.cpu().numpy().tobytes(), [_status_tuple(b, c) for c in range(0, Cn, 16)]))
        tl = b.debug_timeline()
        groups = np.sort(b.collect_rds_array(cap=65536, stream=st), order=["channel", "call_index"])
        b.close()
        res.append((out, tl, groups))
    (feed_out, feed_tl, feed_g), (rec_out, rec_tl, rec_g) = res
    for k in range(len(sizes)):
        assert feed_out[k][:3] == rec_out[k][:3] and feed_out[k][0] > 0 and feed_out[k][1] > 0, k
        assert feed_out[k][3:] == rec_out[k][3:], k
    assert feed_tl.shape == rec_tl.shape == (len(sizes), 10)
    assert np.array_equal(np.sign(feed_tl), np.sign(rec_tl))  # the same stages were launched and timed in both
    assert np.array_equal(feed_g, rec_g)


# ---------------------------------------------------------------------------------------------------------------
# 3. ragged rows

RAGGED = [88, 89, 97, 100, 150, 170, 301, 1001, 3663, 8191, 12345, 40000]


@pytest.mark.parametrize("Cn", [1, 63, 65, 130])
def test_ragged_rows_hold_their_samples_and_nothing_else(pkg, oracle, fmsig, Cn):
    """Batches that end inside a wave, at a wave and one channel behind it, tuner shifts 9 / 10 / 11 mixed on one shared
    capture, twelve calls from fmd_batch_min_samples() = 88 to 40 000 samples: rows of M = 8 (the shortest this geometry
    has: two 16-byte groups of int16 pairs) to 3636 samples, M odd and M = 1, 2, 3 mod 4 among them -- the partial-group
    path of both formats.  Every row is the oracle's in its M samples and untouched behind them; the buffer has no row
    at or above the channel count to write to, and the words behind its last row's M samples are checked too."""
    fs, D = 2.4e6, 11
    rows, shifts = _shared_rows(fmsig, fs, RAGGED), _shifts(Cn)
    want_m = _baseband_lengths(RAGGED, D)
    assert min(want_m) == 8 and {m % 4 for m in want_m} == {0, 1, 2, 3} and any(m % 2 for m in want_m)
    for fmt in (np.complex64, np.int16):
        r = _run(pkg, Cn, shifts, rows, RAGGED, [fmt] * len(RAGGED), mode=1, nbuf=len(RAGGED))
        assert r["nq"] == want_m
        assert all(r["clean"]), r["clean"]
        for k in range(len(RAGGED)):
            _same_rows(r["ciq"][k], _want_all(oracle, fs, D, shifts, rows, "ragged", k), (fmt, k))


def test_refused_rows_leave_the_batch_as_it_was(pkg, oracle, fmsig):
    """A misaligned pointer, a stride that is no multiple of 2 / 4 samples, a stride below the call's length and a
    format outside the enum give FMD_ERR_ARG and a sentence and write nothing; the next call -- with a channel reset
    pending across the refusals -- delivers what the oracle delivers for an uninterrupted stream."""
    import torch
    fs, D, Cn = 2.4e6, 11, 2
    sizes = [N, N, N]
    rows = _shared_rows(fmsig, fs, sizes)
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn, record_callbacks=False)
    o = [oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D) for _ in range(Cn)]
    a_stride = (b.max_audio_floats(N) + 7) // 8 * 8
    audio = torch.zeros((Cn, a_stride), dtype=torch.float32, device="cuda")
    for k, n in enumerate(sizes):
        iq = torch.from_numpy(rows[k]).cuda()
        if k == 1:
            b.reset_channels([1])
            o[1].reset()
        m = _baseband_lengths(sizes, D)[k]
        for fmt, per in ((np.complex64, 2), (np.int16, 4)):
            good = _Rows(Cn, 6016, fmt)
            args = (iq.data_ptr(), 0, n, audio.data_ptr(), a_stride)
            with pytest.raises(pkg.FmdError, match="fmd error -1: .*16-byte aligned"):
                b.process_device(*args, d_ciq_ptr=good.ptr() + 8 // per * 2, ciq_stride=6000, ciq=fmt)
            with pytest.raises(pkg.FmdError, match="fmd error -1: .*multiple of 2"):
                b.process_device(*args, d_ciq_ptr=good.ptr(), ciq_stride=6000 + per // 2, ciq=fmt)
            with pytest.raises(pkg.FmdError, match="fmd error -1: .*smaller than the call's baseband length"):
                b.process_device(*args, d_ciq_ptr=good.ptr(), ciq_stride=(m - 1) // per * per, ciq=fmt)
            assert b"fmd_batch_process_device_call" in pkg.lib().fmd_last_error()
            nq = C.c_uint(5)
            call = pkg.make_call(iq.data_ptr(), 0, 0, n, audio=pkg.make_rows(audio.data_ptr(), 0, a_stride),
                                 ciq=pkg.make_rows(good.ptr(), 2, 6016, nq))
            assert pkg.lib().fmd_batch_process_device_call(b._h, C.byref(call)) == -1
            assert good.host(Cn, 0)[1]  # nothing was written
        fmt = np.int16 if k == 1 else np.complex64
        good = _Rows(Cn, 5960, fmt)
        nf, nq = b.process_device(iq.data_ptr(), 0, n, audio.data_ptr(), a_stride, d_ciq_ptr=good.ptr(),
                                  ciq_stride=5960, ciq=fmt)
        torch.cuda.synchronize()
        got, clean = good.host(Cn, nq)
        assert nq == m and clean
        a = audio[:, :nf].cpu().numpy()
        for c in range(Cn):
            assert _bits_equal(a[c], o[c].process_stream(rows[k][0])), (k, c)
            _same_rows(got[c], o[c].taps()["demod"], (k, c))
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. calls in flight

_FLIGHT_SIZES = [16384, 8193, 30001, 12345, 8192] * 4


def _flight_selection(k, Cn=130):
    """the selection in front of call k: every channel, a few rows out of every wave in an order of their own, none"""
    if k % 4 == 0:
        return None
    if k % 4 == 3:
        return []
    return [129, (7 * k) % 64, 64 + k, 0 if k % 2 else 128, 65 + (5 * k) % 60, 1 + k % 3]


@pytest.mark.parametrize("how,mode,lag", [(h, 2, g) for h in ("default", "split_post", "lpf_late0", "lpf_late1",
                                                               "lpf_late2") for g in (1, 2, 3)]
                         + [("default", 0, 0), ("default", 1, 0)])
def test_rows_of_calls_in_flight(pkg, oracle, fmsig, how, mode, lag):
    """130 channels, 20 calls into 6 rotating pre-filled buffers, complex64 and int16 rows alternating, the selection
    changed in front of every call (every channel / six rows in an order of their own / none), each call's rows read as
    soon as fmd_batch_wait_lagged(lag) covers it: every delivered row equals the oracle's row of THAT call -- the calls
    differ in size and content, so rows of the other buffer parity or of the call's successor do not pass -- and rows
    the call does not deliver keep the fill.  With the post chain on two streams, with each stream layout, and in
    concurrency 0 and 1."""
    fs, D, Cn = 2.4e6, 11, 130
    sizes = _FLIGHT_SIZES
    rows, shifts = _shared_rows(fmsig, fs, sizes), _shifts(Cn)
    setup = {"default": None, "split_post": lambda b: b.debug_set("split_post", 1),
             "lpf_late0": lambda b: b.debug_set("lpf_late", 0), "lpf_late1": lambda b: b.debug_set("lpf_late", 1),
             "lpf_late2": lambda b: b.debug_set("lpf_late", 2)}[how]
    seq = [np.complex64 if k % 2 == 0 else np.int16 for k in range(len(sizes))]
    sel = [_flight_selection(k) for k in range(len(sizes))]
    r = _run(pkg, Cn, shifts, rows, sizes, seq, mode=mode, lag=lag, nbuf=6, setup=setup, sel_seq=sel)
    want_m = _baseband_lengths(sizes, D)
    assert all(r["clean"]), r["clean"]
    for k in range(len(sizes)):
        want = _want_all(oracle, fs, D, shifts, rows, "flight", k)
        if sel[k] is not None:
            want = want[sel[k]] if sel[k] else want[:0]
        assert r["nq"][k] == (want_m[k] if sel[k] is None or sel[k] else 0), k
        assert r["ciq"][k].shape[0] == want.shape[0]
        if want.shape[0]:
            _same_rows(r["ciq"][k], want, (how, mode, lag, k))
    assert len(r["groups"]) > 0


# ---------------------------------------------------------------------------------------------------------------
# 5. large batches

def test_dispatch_4160_channels(pkg, oracle, fmsig):
    """4160 channels on one shared capture, three calls of 16 384 samples in flight (the whole-CU serial stage, the
    half-band chain without mixed rows): every channel's rows, in both formats, equal the rows of the channel of the same
    tuner shift in a 130-channel float batch, whose channels are held against the oracle here."""
    fs, D, Cn = 2.4e6, 11, 4160
    sizes = [16384] * 3
    rows = _shared_rows(fmsig, fs, sizes)
    small = _run(pkg, 130, _shifts(130), rows, sizes, [np.complex64] * 3)
    for k in range(3):
        _same_rows(small["ciq"][k], _want_all(oracle, fs, D, _shifts(130), rows, "4160", k), ("130 channels", k))
    for fmt in (np.complex64, np.int16):
        r = _run(pkg, Cn, _shifts(Cn), rows, sizes, [fmt] * 3, nbuf=3)
        assert r["nq"] == small["nq"] and all(r["clean"])
        for k in range(3):
            _same_rows(r["ciq"][k], small["ciq"][k][np.arange(Cn) % 4], (fmt, k))
            assert _bits_equal(r["audio"][k], small["audio"][k][np.arange(Cn) % 4]), k


def test_dispatch_16384_channels_as_sub_batches(pkg, oracle, fmsig):
    """A shell over two sub-batches, calls of 8192 samples: call 0 delivers every channel (each sub-batch's rows start
    ch0 * stride samples into the caller's buffer), calls 1 and 2 a selection whose rows come from both sub-batches,
    interleaved and in an order of their own, as complex64 and as int16."""
    fs, D, Cn = 2.4e6, 11, 16384
    sizes = [8192] * 3
    rows = _shared_rows(fmsig, fs, sizes)
    small = _run(pkg, 130, _shifts(130), rows, sizes, [np.complex64] * 3)
    for k in range(3):
        _same_rows(small["ciq"][k], _want_all(oracle, fs, D, _shifts(130), rows, "shell", k), ("130 channels", k))
    pick = [8192, 0, 16383, 8191, 9001, 63, 8193, 64, 12000, 4097]
    r = _run(pkg, Cn, _shifts(Cn), rows, sizes, [np.complex64, np.complex64, np.int16], nbuf=3,
             sel_seq=[None, pick, pick[::-1]])
    assert r["nq"] == small["nq"] and all(r["clean"])
    _same_rows(r["ciq"][0], small["ciq"][0][np.arange(Cn) % 4], "every channel")
    _same_rows(r["ciq"][1], small["ciq"][1][np.array(pick) % 4], "selected, complex64")
    _same_rows(r["ciq"][2], small["ciq"][2][np.array(pick[::-1]) % 4], "selected, int16")


# ---------------------------------------------------------------------------------------------------------------
# 6. the format belongs to the call; byte and int16 input

def test_a_format_per_call_changes_nothing_else(pkg, oracle, fmsig):
    """Calls alternate no / complex64 / int16 rows with float / int16 audio and byte / int16 IQ: audio, status record and
    audio meter after EVERY call and the RDS groups equal those of a batch that never asked for the rows; the rows of
    channel 0 equal the oracle fed the converted blocks."""
    fs, D, Cn = 2.4e6, 11, 3
    sizes = [N, 30001, N, 8193, N, N, 20001, N, N, N, 33333, N]
    ps = [_station(fmsig, fs, seed=40 + c, pi=0x4200 + c) for c in range(Cn)]
    rows, start = [], 0
    for n in sizes:
        rows.append(np.stack([fmsig.generate_f32(ps[c], start, n) for c in range(Cn)]))
        start += n
    ciq_seq = [(None, np.complex64, np.int16)[k % 3] for k in range(len(sizes))]
    pcm_seq = [(np.float32, np.int16)[k % 2] for k in range(len(sizes))]
    in_seq = [(np.uint8, np.int16)[(k // 3) % 2] for k in range(len(sizes))]
    kw = dict(pcm_seq=pcm_seq, in_seq=in_seq, every_status=True)
    plain = _run(pkg, Cn, None, rows, sizes, [None] * len(sizes), **kw)
    r = _run(pkg, Cn, None, rows, sizes, ciq_seq, **kw)
    o = oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D)
    seen = set()
    for k, n in enumerate(sizes):
        assert _bits_equal(r["audio"][k], plain["audio"][k]), k
        assert r["status"][k] == plain["status"][k], k
        o.process_stream(_as_float_iq(oracle, _convert(rows[k][0], np.dtype(in_seq[k])), np.dtype(in_seq[k])))
        if ciq_seq[k] is None:
            assert r["ciq"][k] is None and r["nq"][k] == 0
        else:
            assert r["clean"][k]
            _same_rows(r["ciq"][k][0], o.taps()["demod"], k)
            seen.add((np.dtype(ciq_seq[k]), np.dtype(in_seq[k])))
    assert len(seen) == 4  # both row formats behind both input formats
    assert r["status"]["end"] == plain["status"]["end"]
    assert len(plain["groups"]) > 0 and np.array_equal(r["groups"], plain["groups"])


# ---------------------------------------------------------------------------------------------------------------
# 7. maps and edits: the rows follow the slot

_EDIT_SCRIPT = em._steps(em.F, em.F, (3663, [("reset", [0, 5])]), (em.F, [("retune", [3, 6], [em.LOUD, em.BSIDE], [0, 1])]),
                         (301, [("switch", [0, 4], [1, 1])]), (em.F, [("save_load",)]),
                         (8191, [("move", [0, 1], [7, 2], 0, 0), ("switch", [7, 2], [1, 0])]), em.F, 12345)


def test_edited_slots_deliver_the_decoder_they_now_are(pkg, oracle, fmsig):
    """8 slots over two captures through a capture map, retuning enabled (the silent twin delivers no rows): resets, a
    retune to a capture, a capture switch, a save / destroy / load between two calls that deliver rows, and an export
    and import of two slots into two others, in front of calls of 301 to 65 536 samples.  Every slot's rows in every
    call are the demod tap of the oracle decoder tests/edit_model.py follows for that slot; formats alternate."""
    import torch
    script, shifts, cmap = _EDIT_SCRIPT, em.SHIFTS_2CAP, [0] * 8
    streams = em.main_streams(fmsig, em.total_samples(script), two=True)
    model = em.Model(oracle, streams, script, shifts, cmap, taps=("demod",))
    Cn = len(shifts)
    st = torch.cuda.current_stream().cuda_stream

    def make():
        b = pkg.Batch(em._params(pkg), Cn, tuning_shifts=np.array(shifts, np.int32), record_callbacks=False)
        b.enable_retune()
        b.set_capture_map(cmap, 2)
        return b

    b, pos = make(), 0
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = torch.zeros((Cn, a_stride), dtype=torch.float32, device="cuda")
    for k, (n, edits) in enumerate(script):
        for e in edits:
            if e[0] == "reset":
                b.reset_channels(list(e[1]))
            elif e[0] == "retune":
                b.retune(list(e[1]), list(e[2]), captures=list(e[3]))
            elif e[0] == "switch":
                b.switch_captures(list(e[1]), list(e[2]))
            elif e[0] == "move":
                b.import_channels(list(e[2]), b.export_channels(list(e[1])))
            else:
                blob = b.save_state()
                b.close()
                b = make()
                b.load_state(blob)
        n_al = (n + 1) // 2 * 2
        x = np.zeros((2, 2 * n_al), np.float32)
        x[:, :2 * n] = streams.block(pos, n)
        pos += n
        iq = torch.from_numpy(x).cuda()
        fmt = np.int16 if k % 2 else np.complex64
        good = _Rows(Cn, 5972, fmt)
        nf, nq = b.process_device(iq.data_ptr(), n_al, n, audio.data_ptr(), a_stride, st, d_ciq_ptr=good.ptr(),
                                  ciq_stride=5972, ciq=fmt)
        b.wait(stream=st)
        torch.cuda.synchronize()
        got, clean = good.host(Cn, nq)
        assert clean, k
        a = audio[:, :nf].cpu().numpy()
        for c in range(Cn):
            m = model.at(k, c)
            _same_rows(got[c], m["taps"]["demod"], ("slot", c, "call", k, n))
            assert _bits_equal(a[c], m["audio"]), (k, c)
    b.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. host entry point and Python

def test_host_entry_point_takes_any_stride(pkg, oracle, fmsig):
    """fmd_batch_process_host_call copies rows: an odd stride and an unaligned pointer are fine; Batch.process_host_fmt
    (ciq=...) returns the rows last, also beside the multiplex and with a selection; a stride below the call's length
    is refused and changes nothing."""
    fs, D, Cn = 2.4e6, 11, 3
    ps = [_station(fmsig, fs, seed=70 + c) for c in range(Cn)]
    refs = [oracle.OracleDecoder(fs, -0.15 * fs, 48000.0, 15000.0, D) for _ in range(Cn)]
    b = pkg.Batch(pkg.make_params(fs, -0.15 * fs, 48000.0, 15000.0, D), Cn)
    start = 0
    for k, n in enumerate([N, 20001, 8192, 33333, N]):
        x = np.stack([fmsig.generate_f32(ps[c], start, n) for c in range(Cn)])
        start += n
        want_a = [refs[c].process_stream(x[c]) for c in range(Cn)]
        want_q = [refs[c].taps()["demod"] for c in range(Cn)]
        want_m = [refs[c].taps()["baseband"] for c in range(Cn)]
        m = want_q[0].size
        if k % 3 == 0:
            s16 = k == 3
            stride = b.max_mpx_samples(n) + 3  # odd
            buf = np.full(2 * Cn * stride + 1, FILL16 if s16 else FILL32, np.int16 if s16 else np.int32)
            out = buf[1:]  # 2- / 4-byte aligned only
            a_stride = b.max_audio_floats(n)
            audio = np.zeros((Cn, a_stride), np.float32)
            nf, nq = C.c_uint(), C.c_uint()
            call = pkg.make_call(x.ctypes.data, pkg.FMD_IQ_F32, n, n,
                                 audio=pkg.make_rows(audio.ctypes.data, pkg.FMD_PCM_F32, a_stride, nf),
                                 ciq=pkg.make_rows(out.ctypes.data, int(s16), m - 1, nq))
            assert pkg.lib().fmd_batch_process_host_call(b._h, C.byref(call)) == -1
            assert b"smaller than the call's baseband length" in pkg.lib().fmd_last_error()
            call.ciq.stride = stride
            rc = pkg.lib().fmd_batch_process_host_call(b._h, C.byref(call))
            assert rc >= 0, pkg.lib().fmd_last_error()
            assert nq.value == m
            got = out.reshape(Cn, 2 * stride)
            for c in range(Cn):
                row = got[c, :2 * m].copy()
                _same_rows(row.reshape(m, 2) if s16 else row.view(np.complex64), want_q[c], (k, c))
                assert _bits_equal(audio[c, :nf.value], want_a[c]), (k, c)
            assert (got[:, 2 * m:] == (FILL16 if s16 else FILL32)).all() and buf[0] == (FILL16 if s16 else FILL32)
        elif k % 3 == 1:
            b.select_ciq([2, 0] if k == 4 else None)
            a, mpx, rows = b.process_host_fmt(x, mpx=np.float32, ciq=np.int16 if k == 1 else np.complex64)
            pick = [2, 0] if k == 4 else [0, 1, 2]
            assert rows.shape[:2] == (len(pick), m) and mpx.shape == (Cn, m)
            for i, c in enumerate(pick):
                _same_rows(rows[i], want_q[c], (k, c))
            for c in range(Cn):
                assert _bits_equal(a[c], want_a[c]) and _bits_equal(mpx[c], want_m[c]), (k, c)
        else:
            a = b.process_host_fmt(x)
            for c in range(Cn):
                assert _bits_equal(a[c], want_a[c]), (k, c)
    b.close()
