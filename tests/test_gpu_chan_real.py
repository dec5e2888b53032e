"""The real-sampled channeliser and the int16 rows on the GPU (fmd_chan_create_real, fmd_chan_process_*_fmt,
include/fmd.h; k_chan_real and the S16 store stage, csrc/fmd_k_chan.hip.h).

N <= 256: a real channeliser's rows are held, bit for bit, against a COMPLEX channeliser fed the pairs (v, +0) -- the
float kernels the parent shipped, not the code under test; zeros are compared with ==, NaN matches NaN
(chan_real_spec.same_but_zero_signs).  N in 257..512 has no twin: the accuracy gate of tests/chan_spec.py against the
definition in float64, and equality of bits between runs.  S16 rows equal the numpy conversion (feed_spec.mpx16 of both
parts) of the float rows of the same calls on a second channeliser of the same geometry.  The end-to-end test decodes
four stations of one real capture through real channeliser -> S16 rows -> FMD_IN_CIQ_S16 call on one stream.
"""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest

import chan_real_spec as crs
import chan_spec as cs
import split_spec as ss
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

FS = 9.6e6
SENTINEL = 0x5A5A5A5A
F32 = np.float32
# (N, D, K): an odd half; odd N; K < N; the 2.4 MS/s case; N 200; 19.2 MS/s (a complex tile above 64 KiB of LDS)
TWIN_GEOMETRIES = [(6, 2, 7), (7, 3, 10), (8, 3, 5), (24, 11, 88), (200, 92, 736), (192, 88, 704)]
# N above 256: the first such N (odd, K barely above N); N 500; the largest, 51.2 MS/s
BIG_GEOMETRIES = [(257, 100, 300), (500, 230, 1840), (512, 235, 1880)]
IDS = lambda g: "N%dD%dK%d" % g


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def chan(pkg):
    return import_module(pkg.__name__ + ".chan")


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _twin(got, want):
    """the contract of N <= 256: bits, zeros by ==, NaN matches NaN"""
    return got.shape == want.shape and crs.same_but_zero_signs(got.view(F32), want.view(F32))


def _shifts(N):
    """tests/test_gpu_chan.py's: 0, N / 2, negatives, beyond +-N, a duplicate inside a capture"""
    return np.array([[0, N // 2, -1, 3, -(N // 3)],
                     [N // 2, 1, -2, N + 5, 0],
                     [-(N // 2), 2, 2, -N - 1, 7]], np.int32)


def _sizes(D, K, tile):
    """call sizes whose starts meet every residue mod 4 at once: 1, around D, K, around the tile, one big call"""
    return [1, 1, 1, D - 1, D, D + 1, K, 2, tile - 1, tile, tile + 1, 40000, 1, 7]


@functools.lru_cache(maxsize=None)
def _capture(g, n, seed, dt):
    """one capture's real samples: float noise, or integers -- every int8 value once in front, int16 with both ends"""
    rng = np.random.default_rng(1000 * seed + g)
    v = (rng.standard_normal(n) * 0.3).astype(F32)
    if dt == "f32":
        return v
    if dt == "s8":
        q = np.clip(np.rint(v.astype(np.float64) * 127), -128, 127).astype(np.int8)
        q[:256] = rng.permutation(np.arange(-128, 128)).astype(np.int8)
        return q
    q = np.clip(np.rint(v.astype(np.float64) * 32767), -32768, 32767).astype(np.int16)
    q[:4] = [-32768, 32767, -1, 1]
    return q


def _stream(G, n, seed=0, dt="f32"):
    return np.stack([_capture(g, n, seed, dt) for g in range(G)])  # [G, n]


def _zero_q(v):
    """[G, n] real samples -> what the complex twin takes: [G, n, 2] float32 or [G, 2 n] integers, Q = 0"""
    z = np.zeros(v.shape + (2,), v.dtype)
    z[..., 0] = v
    return z if v.dtype == np.float32 else z.reshape(v.shape[0], -1)


def _cut(x, sizes, per=1):
    e = np.cumsum([0] + list(sizes))
    return [x[:, per * a:per * b] for a, b in zip(e[:-1], e[1:])]


def _make(chan, geom, shifts, real, **kw):
    N, D, K = geom
    shifts = np.asarray(shifts, np.int32)
    return chan.Channeliser(FS, N, D, shifts.shape[0], shifts, filter_order=K, real=real, **kw)


def _device_block(x):
    """[G, ...] on the device, captures a multiple of 4 elements apart (four real samples, two float IQ samples, two
    integer IQ samples): the calls' alignment rule"""
    import torch
    a = np.ascontiguousarray(x).reshape(x.shape[0], -1)
    pad = -a.shape[1] % 4 + 4
    buf = np.zeros((a.shape[0], a.shape[1] + pad), a.dtype)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).cuda()[:, :a.shape[1]]


def _samples(ch, x):
    return x.shape[1] if (ch.real or x.ndim == 3) else x.shape[1] // 2


def _out(ch, n, rows=None, extra=0):
    """a row tensor pre-filled with the sentinel: complex64 [rows, stride] or int16 [rows, stride, 2]"""
    import torch
    stride = ch.out_stride(n, rows) + extra
    if rows is np.int16:
        t = torch.full((ch.rows, stride), SENTINEL, dtype=torch.int32, device="cuda")
        return t.view(torch.int16).view(ch.rows, stride, 2)
    return torch.full((ch.rows, 2 * stride), SENTINEL, dtype=torch.int32,
                      device="cuda").view(torch.float32).view(torch.complex64)


def _submit(ch, x, rows=None, stream=None, extra=0):
    import torch
    n = _samples(ch, x)
    d = _device_block(x)
    out = _out(ch, n, rows, extra)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    _, m = ch.process(d, n, out=out, rows=rows, stream=stream.cuda_stream if stream is not None else None)
    return out, m, d


def _rows(out, m):
    """(rows [rows, m] complex64 or [rows, m, 2] int16, tails untouched?)"""
    a = out.cpu().numpy()
    tail = np.ascontiguousarray(a[:, m:])
    if a.dtype == np.int16:
        return a[:, :m], bool(np.all(tail.view(np.uint16) == 0x5A5A))
    return a[:, :m], bool(np.all(tail.view(np.uint32) == SENTINEL))


def _run(chan, geom, shifts, blocks, real, stream=None, rows=None, **kw):
    """the blocks through a new channeliser: [G, B, total outputs (, 2)]; counts and untouched tails checked.  rows:
    one format for all calls, or a list of one per call"""
    import torch
    N, D, K = geom
    shifts = np.asarray(shifts, np.int32)
    ch = _make(chan, geom, shifts, real, **kw)
    fmts = rows if isinstance(rows, list) else [rows] * len(blocks)
    outs = [_submit(ch, x, rows=f, stream=stream) for x, f in zip(blocks, fmts)]
    torch.cuda.synchronize()
    q, got = 0, []
    for x, (o, m, _) in zip(blocks, outs):
        n = _samples(ch, x)
        assert m == ss.count(q, n, D), (q, n, m)
        r, tails = _rows(o, m)
        assert tails, q
        got.append(r)
        q += n
    ch.close()
    if isinstance(rows, list):
        return got
    return np.concatenate(got, axis=1).reshape((shifts.shape[0], shifts.shape[1], -1) + got[0].shape[2:])


# ---------------------------------------------------------------------------------------------------------------
# 1. N <= 256: the bits of the zero-Q complex twin

@pytest.mark.parametrize("dt", ["f32", "s8", "s16"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5)], ids=["1x1", "3x5"])
@pytest.mark.parametrize("geom", TWIN_GEOMETRIES, ids=IDS)
def test_a_real_channelisers_rows_are_its_zero_q_complex_twins(chan, geom, shape, dt):
    N, D, K = geom
    G, B = shape
    sizes = _sizes(D, K, 32 * D)
    starts = np.cumsum([0] + sizes[:-1])
    assert set(int(s) % 4 for s in starts) == {0, 1, 2, 3}
    total = sum(sizes)
    v = _stream(G, total, seed=1, dt=dt)
    sh = _shifts(N)[:G, :B]
    real_ragged = _run(chan, geom, sh, _cut(v, sizes), real=True)
    twin = _run(chan, geom, sh, _cut(_zero_q(v), sizes, per=1 if dt == "f32" else 2), real=False)
    assert real_ragged.shape == twin.shape == (G, B, ss.count(0, total, D))
    assert np.abs(twin).max() > 0.01 and np.isfinite(twin).all()
    assert _twin(real_ragged, twin)
    zeros = int(np.sum(real_ragged.view(F32) == 0))
    # one call of the total
    assert _same(_run(chan, geom, sh, [v], real=True), real_ragged)
    print("chan real N=%d D=%d K=%d %dx%d %s: %d outputs a row equal the twin's bits (%d parts are zeros)"
          % (N, D, K, G, B, dt, twin.shape[2], zeros))


# ---------------------------------------------------------------------------------------------------------------
# 2. N above 256

@functools.lru_cache(maxsize=None)
def _big_case(geom):
    N, D, K = geom
    sizes = _sizes(D, K, 32 * D)
    total = max(sum(sizes), 181 * D)
    sizes = sizes + ([total - sum(sizes)] if total > sum(sizes) else [])
    v = _stream(2, total, seed=2)
    sh = _shifts(N)[:2, :3]
    tr = np.stack([crs.truth(v[g], N, D, sh[g], filter_order=K) for g in range(2)])
    ref = np.stack([crs.reference_rows(v[g], N, D, sh[g], filter_order=K) for g in range(2)])
    return sizes, total, v, sh, tr, ref


_big_rows = {}


def _big_ragged(chan, geom):
    if geom not in _big_rows:
        sizes, total, v, sh, _, _ = _big_case(geom)
        _big_rows[geom] = _run(chan, geom, sh, _cut(v, sizes), real=True)
    return _big_rows[geom]


@pytest.mark.parametrize("geom", BIG_GEOMETRIES, ids=IDS)
def test_n_above_256_is_no_less_accurate_than_the_reference_arithmetic(chan, geom):
    N, D, K = geom
    sizes, total, v, sh, tr, ref = _big_case(geom)
    got = _big_ragged(chan, geom)
    assert got.shape == tr.shape and got.shape[2] >= 180
    r_rms, r_max = cs.gate(got.reshape(6, -1), ref.reshape(6, -1), tr.reshape(6, -1), "real N=%d D=%d K=%d" % geom)
    print("chan real N=%d D=%d K=%d 2x3: error / reference's error: rms %.2f..%.2f max %.2f..%.2f"
          % (N, D, K, r_rms.min(), r_rms.max(), r_max.min(), r_max.max()))


@pytest.mark.parametrize("geom", BIG_GEOMETRIES, ids=IDS)
def test_n_above_256_a_rows_bits_depend_on_its_capture_and_shift_alone(pkg, chan, geom):
    import torch
    N, D, K = geom
    sizes, total, v, sh, _, _ = _big_case(geom)
    full = _big_ragged(chan, geom)
    assert _same(_run(chan, geom, sh, [v], real=True), full)
    other = _cut(v, cs.ragged(total, [777, 2, 32 * D + 1, 5000]))
    side = torch.cuda.Stream()
    assert _same(_run(chan, geom, sh[1:2, 2:3], [b[1:2] for b in other], real=True)[0, 0], full[1, 2])
    assert _same(_run(chan, geom, sh[:1], [b[:1] for b in other], real=True, stream=side)[0], full[0])
    # host entry: an unaligned pointer (2 bytes off a float), odd strides on both sides, two captures
    ch = _make(chan, geom, sh, real=True)
    lib, q, parts = pkg.lib(), 0, []
    for n in (4001, total - 4001):
        stride_in = n | 1
        raw = np.zeros(4 * 2 * stride_in + 2, np.uint8)
        src = raw[2:].view(np.float32).reshape(2, stride_in)
        src[:, :n] = v[:, q:q + n]
        stride_out = ch.max_out_samples(n) | 1
        raw_out = np.zeros(8 * 6 * stride_out + 4, np.uint8)
        cnt = C.c_uint()
        rc = lib.fmd_chan_process_host(ch._h, src.ctypes.data, 16, stride_in, n, raw_out[4:].ctypes.data, stride_out,
                                       C.byref(cnt))
        assert rc == 0, lib.fmd_last_error()
        assert cnt.value == ss.count(q, n, D)
        parts.append(raw_out[4:].view(np.complex64).reshape(6, stride_out)[:, :cnt.value].copy())
        q += n
    ch.close()
    assert _same(np.concatenate(parts, axis=1).reshape(2, 3, -1), full)


# ---------------------------------------------------------------------------------------------------------------
# 3. int16 rows, both kinds

def _loud(D):
    """an out_scale that puts a part's RMS near 2.2 for noise of 0.3 RMS (the rows' power is 4 scale^2 0.09 x 1.2 / D):
    some parts pass +-4.0, most do not"""
    return 4.8 * float(np.sqrt(D))


def _s16_case(geom, real):
    """2 x 3 rows, a loud out_scale so that outputs pass +-4.0, a NaN in capture 1; call counts odd, even and 0"""
    N, D, K = geom
    tile = 32 * D
    sizes = [tile + 3 * D, 2 * D + 1, 1, 3 * tile - D, K, 9 * D + 2, tile, 5 * D, 4 * D, 7 * D + 1]
    total = sum(sizes)
    v = _stream(2, total, seed=5).copy()
    v[1, sizes[0] + 5] = np.nan
    return sizes, (v if real else _zero_q(v)), _shifts(N)[:2, :3]


@pytest.mark.parametrize("geom,real", [((24, 11, 88), False), ((24, 11, 88), True), ((500, 230, 1840), True)],
                         ids=["N24-complex", "N24-real", "N500-real"])
def test_int16_rows_are_the_conversion_of_the_float_rows(chan, geom, real):
    N, D, K = geom
    sizes, x, sh = _s16_case(geom, real)
    blocks = _cut(x, sizes)
    f32 = _run(chan, geom, sh, blocks, real=real, out_scale=_loud(D), rows=[None] * len(sizes))
    s16 = _run(chan, geom, sh, blocks, real=real, out_scale=_loud(D), rows=[np.int16] * len(sizes))
    counts = [r.shape[1] for r in f32]
    assert any(c % 2 for c in counts) and any(c and c % 2 == 0 for c in counts) and 0 in counts
    allf = np.concatenate(f32, axis=1)
    parts = np.ascontiguousarray(allf).view(F32)
    assert np.isnan(parts).any() and (parts > 4.0).any() and (parts < -4.0).any()
    assert (np.abs(parts) < 3.0).any()
    for i, (a, b) in enumerate(zip(s16, f32)):
        assert a.dtype == np.int16 and _same(a, crs.rows_s16(b)), i
    alls = np.concatenate(s16, axis=1)
    assert (alls == 32767).any() and (alls == -32768).any()
    assert np.all(alls[np.isnan(parts.reshape(alls.shape))] == 0)


def test_the_row_format_changes_per_call_with_ten_calls_in_flight(chan):
    """ten calls, float and int16 rows in turn, submitted behind a stretch of other work; int16 strides 4 k with room
    behind the count; every call's rows are those of a channeliser that only ever wrote float rows"""
    import torch
    geom = (24, 11, 88)
    N, D, K = geom
    sizes, x, sh = _s16_case(geom, True)
    blocks = _cut(x, sizes)
    fmts = [np.int16 if i % 2 == 0 else None for i in range(10)]
    want = _run(chan, geom, sh, blocks, real=True, out_scale=_loud(D), rows=[None] * 10)
    ch = _make(chan, geom, sh, True, out_scale=_loud(D))
    ready = [(_device_block(b), _out(ch, b.shape[1], f, extra=8 if f is np.int16 else 2)) for b, f in zip(blocks, fmts)]
    assert all(o.stride(0) // 2 % 4 == 0 for (d, o), f in zip(ready, fmts) if f is np.int16)
    a = torch.randn((8192, 8192), dtype=torch.float32, device="cuda")
    b = a @ a
    torch.cuda.synchronize()
    for _ in range(6):
        b = a @ a
    blocker = torch.cuda.Event()
    blocker.record()
    counts = [ch.process(d, blk.shape[1], out=o, rows=f)[1] for (d, o), blk, f in zip(ready, blocks, fmts)]
    in_flight = not blocker.query()
    torch.cuda.synchronize()
    assert in_flight, "the stretch of other work ended before the last call was submitted: nothing was in flight"
    for i, ((_, o), m, f) in enumerate(zip(ready, counts, fmts)):
        got, tails = _rows(o, m)
        assert tails and m == want[i].shape[1], i
        assert _same(got, crs.rows_s16(want[i]) if f is np.int16 else want[i]), i
    ch.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. set_shifts, reset, refusals on live handles

def test_set_shifts_between_calls_in_flight_and_reset_on_a_real_channeliser(chan):
    import torch
    geom = (200, 92, 736)
    N, D, K = geom
    G, B = 2, 3
    s0 = _shifts(N)[:G, :B].copy()
    s3, s7 = s0.copy(), s0.copy()
    s3[0, 1], s3[1, 2] = 40, -5
    s7[:] = s3
    s7[0, 1], s7[1, 0] = -33, 17
    sizes = [30000, 17, 40960, 1, 29999, 41000, 31, 10240, 50000, 77]
    v = _stream(G, sum(sizes), seed=4)
    blocks = _cut(v, sizes)
    ch = _make(chan, geom, s0, True)
    ready = [(_device_block(b), _out(ch, b.shape[1])) for b in blocks]
    a = torch.randn((8192, 8192), dtype=torch.float32, device="cuda")
    b = a @ a
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
        d, out = ready[i]
        counts.append(ch.process(d, sizes[i], out=out)[1])
    in_flight = not blocker.query()
    torch.cuda.synchronize()
    assert in_flight, "the stretch of other work ended before the last call was submitted: nothing was in flight"
    fresh = {k: _run(chan, geom, s, blocks, real=True) for k, s in ((0, s0), (3, s3), (7, s7))}
    at = 0
    for i, ((_, o), m) in enumerate(zip(ready, counts)):
        got, tails = _rows(o, m)
        assert tails, i
        k = 0 if i < 3 else 3 if i < 7 else 7
        assert _same(got.reshape(G, B, -1), fresh[k][:, :, at:at + m]), i
        at += m
    assert _same(fresh[7][0, 0], fresh[0][0, 0]) and not _same(fresh[7][0, 1], fresh[0][0, 1])
    ch.reset()
    again = []
    for blk in blocks[:3]:
        o, m, _ = _submit(ch, blk)
        again.append(_rows(o, m)[0])
    n3 = sum(r.shape[1] for r in again)
    assert _same(np.concatenate(again, axis=1).reshape(G, B, -1), fresh[7][:, :, :n3])
    ch.close()


@pytest.mark.parametrize("real", [True, False], ids=["real", "complex"])
def test_bad_calls_on_live_handles_are_refused_and_leave_the_channeliser_as_it_was(pkg, chan, real):
    import torch
    geom = (24, 11, 88)
    N, D, K = geom
    G, B = 2, 2
    sh = _shifts(N)[:G, :B]
    v = _stream(G, 2001, seed=8)
    x = v if real else _zero_q(v)
    blocks = _cut(x, [1000, 1001])
    want = _run(chan, geom, sh, blocks, real=real, rows=np.int16)
    ch = _make(chan, geom, sh, real)
    out0, m0, _ = _submit(ch, blocks[0], rows=np.int16)
    assert _same(_rows(out0, m0)[0].reshape(G, B, -1, 2), want[:, :, :m0])
    n = 1001
    d = _device_block(blocks[1])
    out = _out(ch, n, np.int16)
    per = d.element_size() * (1 if real else 2)              # bytes of an input sample
    din, dout = d.data_ptr(), out.data_ptr()
    stride_in, stride_out = d.stride(0) // (1 if real else 2), out.stride(0) // 2
    assert stride_out % 4 == 0 and stride_in % (4 if real else 2) == 0
    lib, cnt = pkg.lib(), C.c_uint(12345)
    mine, other = (16, 0) if real else (0, 16)
    ERR_ARG = -1
    dev = lambda *a: lib.fmd_chan_process_device_fmt(ch._h, *a, C.byref(cnt), None)
    old = lambda *a: lib.fmd_chan_process_device(ch._h, *a, C.byref(cnt), None)
    host_in = np.zeros((G, 2 * n), np.float32)
    host_out = np.zeros((G * B, stride_out, 2), np.int16)
    host = lambda *a: lib.fmd_chan_process_host_fmt(ch._h, *a, C.byref(cnt))
    kind = b"real one" if real else b"complex one"
    m1 = ss.count(1000, n, D)
    assert m1 == 91
    cases = [
        (lambda: dev(din, other, stride_in, n, dout, 1, stride_out), kind),            # the other kind's formats
        (lambda: dev(din, other | 3, stride_in, n, dout, 0, stride_out), kind),
        (lambda: old(din, other, stride_in, n, dout, stride_out), kind),
        (lambda: host(host_in.ctypes.data, other, n, n, host_out.ctypes.data, 1, stride_out), kind),
        (lambda: dev(din, 32, stride_in, n, dout, 1, stride_out), b"FMD_IN_CIQ"),
        (lambda: dev(din, 4, stride_in, n, dout, 1, stride_out), b"iq_format"),
        (lambda: dev(din, mine, stride_in, n, dout, 2, stride_out), b"out_format"),    # bad out_format
        (lambda: dev(din, mine, stride_in, n, dout, -1, stride_out), b"out_format"),
        (lambda: dev(din, mine, stride_in, n, dout, 33, stride_out), b"out_format"),
        (lambda: host(host_in.ctypes.data, mine, n, n, host_out.ctypes.data, 7, stride_out), b"out_format"),
        (lambda: dev(din, mine, stride_in, n, dout, 1, stride_out + 2), b"multiple of 4"),  # S16 stride
        (lambda: dev(din, mine, stride_in, n, dout, 1, stride_out + 1), b"multiple of 4"),
        (lambda: dev(din, mine, stride_in, n, dout, 1, 88), b"out_row_stride"),        # shorter than the count
        (lambda: dev(din, mine, stride_in, n, dout + 8, 1, stride_out), b"d_out"),     # misaligned pointers
        (lambda: dev(din + per, mine, stride_in, n, dout, 1, stride_out), b"d_in"),
        (lambda: dev(din, mine, stride_in + (2 if real else 1), n, dout, 1, stride_out), b"in_capture_stride"),
        (lambda: dev(din, mine, n - 1, n, dout, 1, stride_out), b"in_capture_stride"),
    ]
    if real:  # two samples off: enough for IQ pairs, not for four real samples
        cases.append((lambda: dev(din + 2 * per, mine, stride_in, n, dout, 1, stride_out), b"four real samples"))
    for i, (call, word) in enumerate(cases):
        assert call() == ERR_ARG, i
        msg = lib.fmd_last_error()
        assert word in msg and len(msg.split()) >= 5, (i, msg)
    if not real:  # (pinned by tests/test_gpu_chan.py too: a live complex channeliser names FMD_REAL)
        assert dev(din, 16, stride_in, n, dout, 0, stride_out) == ERR_ARG and b"FMD_REAL" in lib.fmd_last_error()
    assert cnt.value == 12345
    torch.cuda.synchronize()
    assert bool(np.all(out.cpu().numpy().view(np.uint16) == 0x5A5A))
    _, m = ch.process(d, n, out=out, rows=np.int16)
    got1, tails = _rows(out, m)
    assert m == m1 and tails and _same(got1.reshape(G, B, -1, 2), want[:, :, m0:])
    ch.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. poison

def test_non_finite_samples_poison_the_outputs_whose_window_holds_them_and_nothing_else(chan):
    geom = (200, 92, 736)
    N, D, K = geom
    G, B = 3, 3
    sh = _shifts(N)[:, :B]
    tile = 32 * D
    sizes = [2 * tile + 41, K - 5, 3 * tile, 1, 5000]
    total = sum(sizes)
    clean = _stream(G, total, seed=6).copy()
    bad = clean.copy()
    e = np.cumsum([0] + sizes)
    at = [tile - 1, tile, sizes[0] - 3, e[3] - 1, e[3]]
    for p, val in zip(at, (np.nan, np.inf, -np.inf, np.nan, np.inf)):
        bad[1, p] = val   # a tile's last sample, the next one's first, in a short call's history, a call's last, a call of 1
    got_bad = _run(chan, geom, sh, _cut(bad, sizes), real=True)
    got_clean = _run(chan, geom, sh, _cut(clean, sizes), real=True)
    q = np.arange(0, total, D)
    poisoned = np.zeros(q.size, bool)
    for p in at:
        poisoned |= (q - K <= p) & (p <= q - 1)
    assert poisoned.any() and not poisoned[-40:].any()
    for b in range(B):
        w = got_bad[1, b]
        assert not np.isfinite(w[poisoned]).any(), b
        assert _same(w[~poisoned], got_clean[1, b][~poisoned]), b
    for g in (0, 2):
        assert _same(got_bad[g], got_clean[g]), g
    assert np.isfinite(got_clean).all()


# ---------------------------------------------------------------------------------------------------------------
# 6. end to end: real capture -> real channeliser -> int16 rows -> FMD_IN_CIQ_S16 call, one stream, no copy

def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def test_four_stations_of_one_real_capture_decode_like_the_oracle(pkg, chan, oracle, fmsig):
    """fs 4.8 MS/s real, N 48, D 22, K 176: the real part of four generated stations, planned by plan_bins_real from
    their RF frequencies (one in an even Nyquist zone: a negative offset); six calls of 65536 samples, every call's
    int16 rows read by a FMD_IN_CIQ_S16 device call on the same stream.  The yardstick is the same batch fed the
    definition's rows (float64, rounded to complex64, quantised by the numpy conversion): the parent's code.  Per
    station rms(A_chan - A_oracle) <= 4 rms(A_truth - A_oracle), the oracle decoding the (v, 0) stream directly;
    stereo flag equal; pilot level and tuning offset within 4 x the yardstick's miss.  Measured on an MI355X: see
    docs/MEASUREMENTS.md, "Real-sampled channeliser"."""
    import torch
    fs, N, D, K = 4.8e6, 48, 22, 176
    n_in, calls = 65536, 6
    rf = [2 * fs + 0.9e6, 3 * fs - 1.4e6, 0.4e6, 4 * fs + 1.9e6]     # zones 5, 6 (even: folds negative), 1, 9
    offsets = [0.9e6, -1.4e6, 0.4e6, 1.9e6]
    shifts = chan.plan_bins_real(fs, N, rf)
    assert shifts == chan.plan_bins(fs, N, offsets) == [-9, 14, -4, -19]
    S = len(rf)
    wide = np.zeros(2 * n_in * calls, np.float32)
    for k, f in enumerate(offsets):
        p = fmsig.default_params(fs, f_offset=f, amp=0.4, noise_sigma=0.002, seed=700 + k, pi=0x7300 + k,
                                 ps="REAL%d" % k)
        wide = wide + fmsig.generate_f32(p, 0, n_in * calls)
    v = np.ascontiguousarray(wide.reshape(-1, 2)[:, 0])            # the real capture
    vz = crs.pairs(v)                                              # (v, 0): what the oracle decodes
    tr = crs.rows_s16(crs.truth(v, N, D, shifts, filter_order=K).astype(np.complex64))
    orc = [oracle.OracleDecoder(fs, 0.0, 48000.0, 15000.0, D, table_size=N, tuning_shift=s) for s in shifts]

    def batch():
        return pkg.Batch(pkg.make_params(fs, 0.0, 48000.0, 15000.0, D, table_size=N), S,
                         tuning_shifts=np.array(shifts, np.int32))

    ch = chan.Channeliser(fs, N, D, 1, [shifts], filter_order=K, real=True)
    b_chan, b_truth = batch(), batch()
    a_stride = (b_chan.max_audio_floats(n_in) + 63) // 64 * 64
    stream = torch.cuda.current_stream().cuda_stream
    runs = {"chan": (b_chan, [], [], []), "truth": (b_truth, [], [], [])}
    at = 0
    for j in range(calls):
        d = _device_block(v[None, j * n_in:(j + 1) * n_in])
        rows, m = ch.process(d, n_in, stream=stream, rows=np.int16)
        assert m == ss.count(j * n_in, n_in, D) and rows.dtype == torch.int16 and rows.stride(0) % 8 == 0
        padded = np.zeros((S, (m + 3) // 4 * 4, 2), np.int16)
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
    for name, (b, _, _, _) in runs.items():
        b.wait(stream=stream)
    torch.cuda.synchronize()
    assert at == tr.shape[1]
    want = [np.concatenate([o.process_stream(vz[j * n_in:(j + 1) * n_in].reshape(-1)) for j in range(calls)])
            for o in orc]
    for c in range(S):
        got = {name: np.concatenate([a[c, :n.value].cpu().numpy() for a, n in zip(audio, counts)])
               for name, (_, audio, counts, _) in runs.items()}
        assert got["chan"].shape == got["truth"].shape == want[c].shape and want[c].size > 5000
        e_chan, e_truth = _rms(got["chan"] - want[c]), _rms(got["truth"] - want[c])
        print("chan real end to end, station %+.1f MHz (RF %.1f MHz): audio rms %.3g; rms(A_chan - A_oracle) %.3g, "
              "rms(A_truth - A_oracle) %.3g" % (offsets[c] / 1e6, rf[c] / 1e6, _rms(want[c]), e_chan, e_truth))
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
    b_chan.close()
    b_truth.close()
    ch.close()
