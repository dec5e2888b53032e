"""The polyphase channeliser on the GPU (fmd_chan_*, include/fmd.h; csrc/fmd_k_chan.hip.h) against its definition.

Accuracy is held against tests/chan_spec.py's `truth` (the definition in float64) with the gate of that file: a row's
RMS error at most 1.0 x, its maximum error at most 2 x that of the reference's own float32 arithmetic on the same row
(`reference_rows`, computed in the same test).  Everything else is equality of float bits between runs of the device:
one call or ragged calls, alone or among other captures and rows, another stream, the host entry, integer input,
set_shifts with calls in flight, reset, refused calls, poison.  The end-to-end test decodes four stations of one
capture through channeliser -> FMD_IN_CIQ_F32 call on one stream, against the CPU oracle.
"""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest

import chan_spec as cs
import split_spec as ss
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

FS = 9.6e6
SENTINEL = 0x5A5A5A5A
# (N, D, K): K < N; small; the 2.4 MS/s case; 9.6 MS/s; N 100; K not a multiple of N; 19.2 MS/s (a tile above 64 KiB
# of LDS)
GEOMETRIES = [(8, 3, 5), (16, 5, 9), (24, 11, 88), (96, 44, 352), (100, 40, 320), (128, 50, 500), (192, 88, 704)]
GEOMETRY_IDS = ["N%dD%dK%d" % g for g in GEOMETRIES]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def chan(pkg):
    return import_module(pkg.__name__ + ".chan")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _shifts(N):
    """3 x 5 shifts: 0, N / 2, negatives, beyond +-N, a duplicate inside a capture"""
    return np.array([[0, N // 2, -1, 3, -(N // 3)],
                     [N // 2, 1, -2, N + 5, 0],
                     [-(N // 2), 2, 2, -N - 1, 7]], np.int32)


def _sizes(D, K, tile):
    """one stream of call sizes: 1, around D, K, around the kernel's tile, one big call"""
    return [1, 1, D - 1, D, D + 1, K, 3, tile - 1, tile, tile + 1, 40000, 1, 7]


@functools.lru_cache(maxsize=None)
def _capture(g, n, seed=0):
    rng = np.random.default_rng(1000 * seed + g)
    return (rng.standard_normal((n, 2)) * 0.3).astype(np.float32)


def _stream(G, n, seed=0):
    return np.stack([_capture(g, n, seed) for g in range(G)])  # [G, n, 2]


def _cut(x, sizes):
    e = np.cumsum([0] + list(sizes))
    return [x[:, a:b] for a, b in zip(e[:-1], e[1:])]


def _make(chan, geom, shifts, **kw):
    N, D, K = geom
    shifts = np.asarray(shifts, np.int32)
    return chan.Channeliser(FS, N, D, shifts.shape[0], shifts, filter_order=K, **kw)


def _device_block(x, pad=0):
    """[G, n, 2] float32 (or integer IQ [G, 2 n]) on the device, rows `pad` elements longer than the call and a
    whole number of sample pairs apart (the call's alignment rule)"""
    import torch
    a = np.ascontiguousarray(x).reshape(x.shape[0], -1)
    pad += -(a.shape[1] + pad) % 4
    buf = np.zeros((a.shape[0], a.shape[1] + pad), a.dtype)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).cuda()[:, :a.shape[1]]


def _prepare(ch, x):
    """a call's device buffers: (input on the device, out tensor pre-filled with the sentinel, samples)"""
    import torch
    n = x.shape[1] if x.ndim == 3 else x.shape[1] // 2
    d = _device_block(x)
    out = torch.full((ch.rows, 2 * ch.out_stride(n)), SENTINEL, dtype=torch.int32,
                     device="cuda").view(torch.float32).view(torch.complex64)
    return d, out, n


def _submit(ch, x, stream=None):
    import torch
    d, out, n = _prepare(ch, x)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    _, m = ch.process(d, n, out=out, stream=stream.cuda_stream if stream is not None else None)
    return out, m, d


def _rows(out, m):
    """(rows [rows, m] complex64, tails untouched?)"""
    a = out.cpu().numpy()
    return a[:, :m], bool(np.all(np.ascontiguousarray(a[:, m:]).view(np.uint32) == SENTINEL))


def _run(chan, geom, shifts, blocks, stream=None):
    """the blocks through a new channeliser: [G, B, total outputs] complex64; counts and untouched tails checked"""
    import torch
    N, D, K = geom
    shifts = np.asarray(shifts, np.int32)
    ch = _make(chan, geom, shifts)
    outs = [_submit(ch, x, stream=stream) for x in blocks]
    torch.cuda.synchronize()
    q, rows = 0, []
    for x, (o, m, _) in zip(blocks, outs):
        n = x.shape[1] if x.ndim == 3 else x.shape[1] // 2
        assert m == ss.count(q, n, D), (q, n, m)
        got, tails = _rows(o, m)
        assert tails, q
        rows.append(got)
        q += n
    ch.close()
    return np.concatenate(rows, axis=1).reshape(shifts.shape[0], shifts.shape[1], -1)


@functools.lru_cache(maxsize=None)
def _total(geom):
    N, D, K = geom
    return sum(_sizes(D, K, 32 * D))


@functools.lru_cache(maxsize=None)
def _yardstick(geom):
    """(truth, reference's rows) of the 3 x 5 channeliser over the geometry's stream, computed once: [3, 5, outputs]"""
    N, D, K = geom
    x = _stream(3, _total(geom))
    sh = _shifts(N)
    return (np.stack([cs.truth(x[g], N, D, sh[g], filter_order=K) for g in range(3)]),
            np.stack([cs.reference_rows(x[g], N, D, sh[g], filter_order=K) for g in range(3)]))


_ragged_cache = {}


def _ragged_rows(chan, geom):
    """the device's rows of the 3 x 5 channeliser over the ragged calls, once per geometry"""
    if geom not in _ragged_cache:
        N, D, K = geom
        ch = _make(chan, geom, _shifts(N))
        assert ch.rows == 15 and ch.out_rate == FS / D and ch.tile_samples == 32 * D
        assert _same(ch.taps(), cs.taps(K, 0.6 / D)[1:])
        ch.close()
        _ragged_cache[geom] = _run(chan, geom, _shifts(N), _cut(_stream(3, _total(geom)), _sizes(D, K, 32 * D)))
    return _ragged_cache[geom]


# ---------------------------------------------------------------------------------------------------------------
# accuracy: geometries x shapes, ragged call sizes

@pytest.mark.parametrize("shape", [(1, 1), (3, 5)], ids=["1x1", "3x5"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=GEOMETRY_IDS)
def test_rows_are_no_less_accurate_than_the_reference_arithmetic(chan, geom, shape):
    N, D, K = geom
    G, B = shape
    tr, ref = _yardstick(geom)
    if shape == (3, 5):
        got = _ragged_rows(chan, geom)
    else:
        got = _run(chan, geom, _shifts(N)[:1, :1], _cut(_stream(1, _total(geom)), _sizes(D, K, 32 * D)))
    assert got.shape == tr[:G, :B].shape and got.shape[2] >= 180
    r_rms, r_max = cs.gate(got.reshape(G * B, -1), ref[:G, :B].reshape(G * B, -1), tr[:G, :B].reshape(G * B, -1),
                           "N=%d D=%d K=%d %dx%d" % (N, D, K, G, B))
    print("chan N=%d D=%d K=%d %dx%d: error / reference's error: rms %.2f..%.2f max %.2f..%.2f"
          % (N, D, K, G, B, r_rms.min(), r_rms.max(), r_max.min(), r_max.max()))


# ---------------------------------------------------------------------------------------------------------------
# bits: call sizes, geometry, stream, entry point

@pytest.mark.parametrize("geom", GEOMETRIES, ids=GEOMETRY_IDS)
def test_a_rows_bits_depend_on_its_capture_and_shift_alone(pkg, chan, geom):
    import torch
    N, D, K = geom
    total = _total(geom)
    x = _stream(3, total)
    sh = _shifts(N)
    full = _ragged_rows(chan, geom)
    # one call
    assert _same(_run(chan, geom, sh, [x]), full)
    # other call sizes, one capture alone, one row alone (another row index, another B), another stream
    other = _cut(x, cs.ragged(total, [777, 2, 32 * D + 1, 5000]))
    side = torch.cuda.Stream()
    for g in range(3):
        assert _same(_run(chan, geom, sh[g:g + 1], [b[g:g + 1] for b in other])[0], full[g]), g
    assert _same(_run(chan, geom, sh[1:2, 3:4], [b[1:2] for b in other])[0, 0], full[1, 3])
    assert _same(_run(chan, geom, sh[2:3], [b[2:3] for b in other], stream=side)[0], full[2])
    # the duplicate shift of capture 2 gives the same row twice
    assert _same(full[2, 1], full[2, 2])
    # host entry: an unaligned pointer (4 bytes off), odd strides on both sides, two captures
    ch = _make(chan, geom, sh[:2])
    lib, q, parts = pkg.lib(), 0, []
    for n in (4001, total - 4001):
        stride_in = n + 1 if (n + 1) % 2 else n + 2
        raw = np.zeros(8 * 2 * stride_in + 4, np.uint8)
        src = raw[4:].view(np.float32).reshape(2, stride_in, 2)
        src[:, :n] = x[:2, q:q + n]
        m_max = ch.max_out_samples(n)
        stride_out = m_max | 1
        raw_out = np.zeros(8 * 10 * stride_out + 4, np.uint8)
        cnt = C.c_uint()
        rc = lib.fmd_chan_process_host(ch._h, src.ctypes.data, 0, stride_in, n, raw_out[4:].ctypes.data, stride_out,
                                       C.byref(cnt))
        assert rc == 0, lib.fmd_last_error()
        assert cnt.value == ss.count(q, n, D)
        parts.append(raw_out[4:].view(np.complex64).reshape(10, stride_out)[:, :cnt.value].copy())
        q += n
    ch.close()
    assert _same(np.concatenate(parts, axis=1).reshape(2, 5, -1), full[:2])


# ---------------------------------------------------------------------------------------------------------------
# input formats

def _quantised(dt, G, n):
    x = _stream(G, n, seed=3).reshape(G, -1)
    if dt == np.uint8:
        return np.clip(np.rint((x.astype(np.float64) + 1.0) * 127.5), 0, 255).astype(np.uint8)
    info = np.iinfo(dt)
    return np.clip(np.rint(x.astype(np.float64) * info.max), info.min, info.max).astype(dt)


def _host_convert(oracle, q):
    if q.dtype == np.uint8:
        return oracle.convert_u8(q.reshape(-1)).reshape(q.shape)
    return q.astype(np.float32) * np.float32(2.0 ** -15 if q.dtype == np.int16 else 2.0 ** -7)


@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.int16], ids=["u8", "s8", "s16"])
def test_integer_input_gives_the_bits_of_the_float_call_on_the_converted_block(chan, oracle, dt):
    """ragged calls, so the single-sample edges and the history of every format run; then one capture alone"""
    geom = GEOMETRIES[2]
    N, D, K = geom
    sizes = [4099, 31, 1, 6001]
    for G, B in ((3, 2), (1, 3)):
        sh = _shifts(N)[:G, :B]
        q = _quantised(dt, G, sum(sizes))
        xf = _host_convert(oracle, q).reshape(G, -1, 2)
        got_i = _run(chan, geom, sh, [q[:, 2 * a:2 * b] for a, b in zip(np.cumsum([0] + sizes[:-1]), np.cumsum(sizes))])
        got_f = _run(chan, geom, sh, _cut(xf, sizes))
        assert _same(got_i, got_f), (G, B)
        assert np.abs(got_f).max() > 0.01


# ---------------------------------------------------------------------------------------------------------------
# set_shifts, reset

def test_set_shifts_between_calls_in_flight_equals_fresh_channelisers(chan):
    """Ten calls submitted back to back behind a stretch of other work on the stream, so that no call has started
    when the last one is submitted; set_shifts in front of calls 3 and 7.  Every table upload finds the earlier ones
    still in flight and must not disturb them: from those calls on every row is that of a channeliser that had the
    new shifts from the start, the earlier calls keep the old ones.  Then reset: the rows of a new channeliser."""
    import torch
    geom = GEOMETRIES[3]
    N, D, K = geom
    G, B = 2, 3
    s0 = _shifts(N)[:G, :B].copy()
    s3, s7 = s0.copy(), s0.copy()
    s3[0, 1], s3[1, 2] = 40, -5
    s7[:] = s3
    s7[0, 1], s7[1, 0] = -33, 17
    sizes = [30000, 17, 40960, 1, 29999, 41000, 31, 10240, 50000, 77]
    x = _stream(G, sum(sizes), seed=4)
    blocks = _cut(x, sizes)
    ch = _make(chan, geom, s0)
    ready = [_prepare(ch, b) for b in blocks]
    a = torch.randn((8192, 8192), dtype=torch.float32, device="cuda")
    b = a @ a  # (the first product also loads the BLAS library: not part of the stretch)
    torch.cuda.synchronize()
    for _ in range(6):
        b = a @ a
    blocker = torch.cuda.Event()
    blocker.record()
    counts = []
    for i in range(10):
        if i == 3:
            ch.set_shifts(s3)
        if i == 7:
            ch.set_shifts(s7)
        d, out, n = ready[i]
        counts.append(ch.process(d, n, out=out)[1])
    in_flight = not blocker.query()
    torch.cuda.synchronize()
    assert in_flight, "the stretch of other work ended before the last call was submitted: nothing was in flight"
    fresh = {k: _run(chan, geom, s, blocks) for k, s in ((0, s0), (3, s3), (7, s7))}
    at = 0
    for i, ((_, o, _), m) in enumerate(zip(ready, counts)):
        got, tails = _rows(o, m)
        assert tails, i
        k = 0 if i < 3 else 3 if i < 7 else 7
        assert _same(got.reshape(G, B, -1), fresh[k][:, :, at:at + m]), i
        at += m
    # the untouched rows never changed, the retuned ones did
    assert _same(fresh[7][0, 0], fresh[0][0, 0]) and not _same(fresh[7][0, 1], fresh[0][0, 1])
    ch.reset()
    again = []
    for blk in blocks[:3]:
        o, m, _ = _submit(ch, blk)
        again.append(_rows(o, m)[0])
    n3 = sum(r.shape[1] for r in again)
    assert _same(np.concatenate(again, axis=1).reshape(G, B, -1), fresh[7][:, :, :n3])
    ch.close()


# ---------------------------------------------------------------------------------------------------------------
# refused calls of a live channeliser

def test_bad_calls_are_refused_with_a_sentence_and_leave_the_channeliser_as_it_was(pkg, chan):
    import torch
    geom = GEOMETRIES[2]
    N, D, K = geom
    G, B = 2, 2
    sh = _shifts(N)[:G, :B]
    x = _stream(G, 2001, seed=8)
    blocks = _cut(x, [1000, 1001])
    want = _run(chan, geom, sh, blocks)
    ch = _make(chan, geom, sh)
    out0, m0, _ = _submit(ch, blocks[0])
    assert _same(_rows(out0, m0)[0].reshape(G, B, -1), want[:, :, :m0])
    n = 1001
    d, out, _ = _prepare(ch, blocks[1])
    din, dout, stride_in, stride_out = d.data_ptr(), out.data_ptr(), d.stride(0) // 2, out.stride(0)
    lib, cnt = pkg.lib(), C.c_uint(12345)
    host_in = np.zeros((G, 2 * n), np.float32)
    host_out = np.zeros((G * B, stride_out), np.complex64)
    ERR_ARG, ERR_SIZE = -1, -3
    dev = lambda *a: lib.fmd_chan_process_device(ch._h, *a, C.byref(cnt), None)
    host = lambda *a: lib.fmd_chan_process_host(ch._h, *a, C.byref(cnt))
    m1 = ss.count(1000, n, D)
    assert m1 == 91  # (so 88 and 89 are short)
    cases = [
        (lambda: dev(din, 0, stride_in, 0, dout, stride_out), ERR_SIZE, b"samples"),
        (lambda: dev(din, 0, stride_in, 16777217, dout, stride_out), ERR_SIZE, b"samples"),
        (lambda: host(host_in.ctypes.data, 0, n, 0, host_out.ctypes.data, stride_out), ERR_SIZE, b"samples"),
        (lambda: dev(din, 0, n - 1, n, dout, stride_out), ERR_ARG, b"in_capture_stride"),
        (lambda: host(host_in.ctypes.data, 0, n - 1, n, host_out.ctypes.data, stride_out), ERR_ARG,
         b"in_capture_stride"),
        (lambda: dev(din, 0, stride_in, n, dout, 88), ERR_ARG, b"out_row_stride"),
        (lambda: host(host_in.ctypes.data, 0, n, n, host_out.ctypes.data, 89), ERR_ARG, b"out_row_stride"),
        (lambda: dev(din + 8, 0, stride_in, n, dout, stride_out), ERR_ARG, b"d_in"),
        (lambda: dev(din, 0, stride_in + 1, n, dout, stride_out), ERR_ARG, b"in_capture_stride"),
        (lambda: dev(din, 0, stride_in, n, dout + 8, stride_out), ERR_ARG, b"d_out"),
        (lambda: dev(din, 0, stride_in, n, dout, stride_out + 1), ERR_ARG, b"out_row_stride"),
        (lambda: dev(din, 4, stride_in, n, dout, stride_out), ERR_ARG, b"iq_format"),
        (lambda: dev(din, 16, stride_in, n, dout, stride_out), ERR_ARG, b"FMD_REAL"),
        (lambda: dev(din, 32, stride_in, n, dout, stride_out), ERR_ARG, b"FMD_IN_CIQ"),
        (lambda: host(host_in.ctypes.data, 33, n, n, host_out.ctypes.data, stride_out), ERR_ARG, b"FMD_IN_CIQ"),
    ]
    for i, (call, code, word) in enumerate(cases):
        assert call() == code, i
        msg = lib.fmd_last_error()
        assert word in msg and len(msg.split()) >= 5, msg
    with pytest.raises(pkg.FmdError, match="n_rows"):
        ch.set_shifts([1, 2, 3])
    assert cnt.value == 12345  # no refused call wrote a count
    torch.cuda.synchronize()
    assert bool(np.all(out.cpu().numpy().view(np.uint32) == SENTINEL))  # ... or a row
    _, m = ch.process(d, n, out=out)
    got1, tails = _rows(out, m)
    assert m == m1 and tails and _same(got1.reshape(G, B, -1), want[:, :, m0:])
    ch.close()


# ---------------------------------------------------------------------------------------------------------------
# poison

def test_non_finite_input_poisons_the_outputs_whose_window_holds_it_and_nothing_else(chan):
    """capture 1 of three holds a NaN and infs: at a tile's edge, inside the history the next call carries, in a
    call's last sample and in a call of one sample.  Output q is non-finite, in every row of capture 1, exactly where
    one of x[q - K .. q - 1] is; every other output and every other capture keep the bits of the clean run."""
    geom = GEOMETRIES[3]
    N, D, K = geom
    G, B = 3, 3
    sh = _shifts(N)[:, :B]
    tile = 32 * D
    sizes = [2 * tile + 40, K - 5, 3 * tile, 1, 5000]
    total = sum(sizes)
    clean = _stream(G, total, seed=6).copy()
    bad = clean.copy()
    e = np.cumsum([0] + sizes)
    at = [tile - 1, tile, sizes[0] - 3, e[3] - 1, e[3]]
    bad[1, at[0]] = (np.nan, 0.25)           # a tile's last input sample
    bad[1, at[1]] = (0.5, np.inf)            # ... and the next tile's first
    bad[1, at[2]] = (np.inf, 0.5)            # inside the carried history of call 1 (shorter than K)
    bad[1, at[3]] = (0.1, np.nan)            # the last sample of a call
    bad[1, at[4]] = (-np.inf, 0.0)           # a call of one sample
    got_bad = _run(chan, geom, sh, _cut(bad, sizes))
    got_clean = _run(chan, geom, sh, _cut(clean, sizes))
    q = np.arange(0, total, D)
    poisoned = np.zeros(q.size, bool)
    for p in at:
        poisoned |= (q - K <= p) & (p <= q - 1)
    assert poisoned.any() and not poisoned[-50:].any()
    for b in range(B):
        v = got_bad[1, b]
        assert not np.isfinite(v[poisoned]).any(), b
        assert _same(v[~poisoned], got_clean[1, b][~poisoned]), b
    for g in (0, 2):
        assert _same(got_bad[g], got_clean[g]), g
    assert np.isfinite(got_clean).all()


# ---------------------------------------------------------------------------------------------------------------
# end to end: channeliser -> FMD_IN_CIQ_F32 call on one stream

def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def test_four_stations_of_one_capture_decode_like_the_oracle(pkg, chan, oracle, fmsig):
    """fs 2.4 MS/s, N 24, D 11, K 88: four stations in one capture, six calls of 65536 samples; every call a
    FMD_IN_CIQ_F32 device call that reads the channeliser's row buffer on the same stream.  The yardstick is the same
    batch fed the definition's rows (float64, rounded to float32): the parent's code, not the code under test.
    Per station rms(A_chan - A_oracle) <= 4 rms(A_truth - A_oracle): 2 from the triangle inequality (the rows lie
    within the reference's error of the truth), 2 for the decoder's gain differing between the two perturbations.
    Measured on an MI355X (audio RMS against the oracle, channeliser / truth rows, per station): see
    docs/MEASUREMENTS.md, "Polyphase channeliser"."""
    import torch
    fs, N, D, K = 2.4e6, 24, 11, 88
    n_in, calls = 65536, 6
    offsets = [0.8e6, 0.3e6, -0.4e6, -0.9e6]
    shifts = chan.plan_bins(fs, N, offsets)
    S = len(offsets)
    wide = np.zeros(2 * n_in * calls, np.float32)
    for k, f in enumerate(offsets):
        p = fmsig.default_params(fs, f_offset=f, amp=0.2, noise_sigma=0.002, seed=500 + k, pi=0x7200 + k,
                                 ps="CHAN%d" % k)
        wide = wide + fmsig.generate_f32(p, 0, n_in * calls)
    wide = wide.reshape(calls, 1, n_in, 2)
    tr = cs.truth(wide.reshape(-1, 2), N, D, shifts, filter_order=K).astype(np.complex64)
    orc = [oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, table_size=N, tuning_shift=s) for s in shifts]

    def batch():
        return pkg.Batch(pkg.make_params(fs, 0.0, 48000.0, 15000.0, D, table_size=N), S,
                         tuning_shifts=np.array(shifts, np.int32))

    ch = chan.Channeliser(fs, N, D, 1, [shifts], filter_order=K)
    b_chan, b_truth = batch(), batch()
    a_stride = (b_chan.max_audio_floats(n_in) + 63) // 64 * 64
    stream = torch.cuda.current_stream().cuda_stream
    runs = {"chan": (b_chan, [], [], []), "truth": (b_truth, [], [], [])}
    at = 0
    for j in range(calls):
        d = _device_block(wide[j])
        rows, m = ch.process(d, n_in, stream=stream)
        assert m == ss.count(j * n_in, n_in, D)
        padded = np.zeros((S, (m + 1) // 2 * 2), np.complex64)  # (rows an even stride apart, as the call wants them)
        padded[:, :m] = tr[:, at:at + m]
        t_rows = torch.from_numpy(padded).cuda()[:, :m]
        at += m
        for name, r in (("chan", rows[:, :m]), ("truth", t_rows)):
            b, audio, counts, keep = runs[name]
            a = torch.zeros((S, a_stride), dtype=torch.float32, device="cuda")
            cnt = C.c_uint()
            b.process_call(ciq_in=r, audio=pkg.make_rows(a.data_ptr(), pkg.FMD_PCM_F32, a_stride, cnt), stream=stream)
            audio.append(a)
            counts.append(cnt)
            keep.append((d, r))
    groups = {}
    for name, (b, _, _, _) in runs.items():
        b.wait(stream=stream)
        groups[name] = b.collect_rds_array()
    torch.cuda.synchronize()
    assert at == tr.shape[1]
    want = [np.concatenate([o.process_stream(wide[j][0].reshape(-1)) for j in range(calls)]) for o in orc]
    for c in range(S):
        got = {name: np.concatenate([a[c, :n.value].cpu().numpy() for a, n in zip(audio, counts)])
               for name, (_, audio, counts, _) in runs.items()}
        assert got["chan"].shape == got["truth"].shape == want[c].shape and want[c].size > 10000
        e_chan, e_truth = _rms(got["chan"] - want[c]), _rms(got["truth"] - want[c])
        print("chan end to end, station %+.1f MHz: audio rms %.3g; rms(A_chan - A_oracle) %.3g, "
              "rms(A_truth - A_oracle) %.3g" % (offsets[c] / 1e6, _rms(want[c]), e_chan, e_truth))
        assert _rms(want[c]) > 1e-3 and e_truth > 0
        assert e_chan <= 4 * e_truth, (c, e_chan, e_truth)
        so = orc[c].status()
        st_c, st_t = b_chan.status(c), b_truth.status(c)
        assert bool(st_c.stereo_detected) == bool(so.stereo), c
        for field, ref in (("pilot_level", so.pilot_level), ("tuning_offset", so.tuning_offset)):
            ref = np.float32(ref)
            yard = max(abs(float(np.float32(getattr(st_t, field))) - float(ref)), float(np.spacing(np.abs(ref))))
            miss = abs(float(np.float32(getattr(st_c, field))) - float(ref))
            print("  %s: oracle %.9g, channeliser off by %.3g, truth rows off by %.3g"
                  % (field, float(ref), miss, yard))
            assert miss <= 4 * yard, (c, field, miss, yard)
        # (six calls are too short for an RDS group on either side: the batch invents none)
        assert [g for g in groups["chan"] if int(g["channel"]) == c] == [] == [bl for _, bl in orc[c].rds_groups()], c
    b_chan.close()
    b_truth.close()
    ch.close()
