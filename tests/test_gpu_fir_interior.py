"""The interior body of the headline IF FIR's tiles (k_if_fir_mt3, fmd_k_if.hip.h) against the edge body and the oracle.

A tile inside a call -- full, no history in front, every load inside the channel's row -- takes a body without clamps
and range tests and with the tuner product in three packed operations; the first and the last one or two tiles of a call
take the body every tile took before.  `fir_ro` -2 of fmd_batch_debug_set sends every tile through the edge body (the
sign of that key and not a key of its own: the library's key table is held to 14 keys).  Three outputs per lane
(`fir_ro` 3 / -3) have the edge body only -- both bodies together cost that form a wave per SIMD -- and run here as the
same two launches against the oracle.

The kernel can go wrong at tile boundaries, not at size: small batches at the reference geometry (2.4 MS/s, D = 11, 88
taps, table of 64), the two-tile form forced by `fir_nt` = 2.  Every case runs the same sequence of calls twice, interior
on and off, and is compared two ways:
  * every channel's IF output (the `demod` stage tap) and audio, bit for bit between the two runs;
  * the three stations' first channels against the CPU oracle over the whole sequence.  Calls carry the decimator phase,
    so the sequence moves `pos` through its residues and the window's aligned start through both parities.
No tolerance anywhere: the interior body does the same IEEE operations on the same operands in the same order.

The sequence: about a hundred short calls of 4160 ... 4352 samples (three to four tiles of 128 outputs: within that
range the last full tile changes from edge to interior, a call ends exactly on a tile at 4224, and the second tile of a
workgroup is the partial one), a few odd lengths among them; two full calls of 65 536; 150 samples (no interior tile at
all); and, after fmd_batch_reset, a short and a full call.
"""
import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

FS, D, N = 2.4e6, 11, 65536
K = 3  # stations: channel c (capture c with shared captures) carries station c % K
SHORT = list(range(4160, 4353, 2))
for _i, _odd in ((5, 4161), (31, 4223), (34, 4225), (60, 4299), (97, 4351)):
    SHORT.insert(_i, _odd)
SEQUENCE = SHORT + [N, N, 150, "reset", 4224, N]
FORMATS = {"f32": np.float32, "u8": np.uint8, "s8": np.int8, "s16": np.int16}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def stations(fmsig):
    """The K stations' float IQ over the whole sequence (interleaved I, Q), and their RTL-SDR bytes: generated once."""
    total = sum(n for n in SEQUENCE if n != "reset")
    ps = [fmsig.default_params(FS, noise_sigma=0.01, seed=71 + s, pi=0x7100 + s) for s in range(K)]
    return {"f32": np.stack([fmsig.generate_f32(p, 0, total) for p in ps]),
            "u8": np.stack([fmsig.generate_u8(p, 0, total) for p in ps])}


def _input(stations, fmt):
    """[K, 2 * total] of the format's dtype"""
    if fmt in ("f32", "u8"):
        return stations[fmt]
    dt = FORMATS[fmt]
    info = np.iinfo(dt)
    scale = 32767 if dt == np.int16 else 127
    return np.clip(np.rint(stations["f32"].astype(np.float64) * scale), info.min, info.max).astype(dt)


def _to_f32(oracle, q):
    """the contract's host conversion of one row"""
    if q.dtype == np.float32:
        return q
    if q.dtype == np.uint8:
        return oracle.convert_u8(q)
    return q.astype(np.float32) * np.float32(2.0 ** -15 if q.dtype == np.int16 else 2.0 ** -7)


_REFERENCE = {}


@pytest.fixture(scope="module")
def reference(oracle, stations):
    """fmt -> per call [(demod tap, audio)] * K of the oracle: computed once per format, shared, never written to"""
    def get(fmt):
        if fmt not in _REFERENCE:
            x = _input(stations, fmt)
            decs = [oracle.OracleDecoder(FS, -0.15 * FS, 48000.0, 15000.0, D) for _ in range(K)]
            out, start = [], 0
            for n in SEQUENCE:
                if n == "reset":
                    for o in decs:
                        o.reset()
                    continue
                row = []
                for s in range(K):
                    a = decs[s].process_stream(_to_f32(oracle, x[s, 2 * start:2 * (start + n)]))
                    row.append((decs[s].taps()["demod"].copy(), a))
                out.append(row)
                start += n
            _REFERENCE[fmt] = out
        return _REFERENCE[fmt]
    return get


def _taps(pkg, b, channels, buf):
    """[channels, M] complex64: the demod tap of the last call"""
    rows = []
    for c in range(channels):
        n = pkg.lib().fmd_batch_get_tap(b._h, pkg.TAPS["demod"], c, buf.ctypes.data, buf.size)
        assert n >= 0
        rows.append(buf[:2 * n].copy())
    return np.stack(rows)


def _run(pkg, stations, fmt, channels, ro, interior, cpc=1, cmap=None, concurrency=None):
    """The sequence through one batch with host calls; returns per call (taps [C, 2M] float32, audio [C, n])."""
    x = _input(stations, fmt)
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), channels, record_callbacks=False)
    if concurrency is not None:
        b.set_concurrency(concurrency)
    b.debug_set("fir_nt", 2)
    b.debug_set("fir_ro", ro if interior else -ro)
    rows = channels
    if cpc > 1:
        b.set_channels_per_capture(cpc)
        rows = channels // cpc
    if cmap is not None:
        b.set_capture_map(cmap, int(max(cmap)) + 1)
        rows = int(max(cmap)) + 1
    b.enable_taps()
    buf = np.zeros(2 * 8192, dtype=np.float32)
    out, start = [], 0
    for n in SEQUENCE:
        if n == "reset":
            b.reset()
            continue
        iq = x[np.arange(rows) % K, 2 * start:2 * (start + n)]
        a = b.process_host_fmt(iq)
        out.append((_taps(pkg, b, channels, buf), a.copy()))
        start += n
    b.close()
    return out


def _check(pkg, stations, reference, fmt, channels, ro, station_of=None, **kw):
    station_of = station_of or (lambda c: c % K)
    on = _run(pkg, stations, fmt, channels, ro, True, **kw)
    off = _run(pkg, stations, fmt, channels, ro, False, **kw)
    ref = reference(fmt)
    assert len(on) == len(off) == len(ref)
    first = {station_of(c): c for c in reversed(range(channels))}  # the first channel of every station
    assert sorted(first) == list(range(K))
    for k, ((t1, a1), (t0, a0)) in enumerate(zip(on, off)):
        assert _same(t1, t0), "IF output, call %d" % k
        assert _same(a1, a0), "audio, call %d" % k
        for s, c in first.items():
            assert _same(t1[c], ref[k][s][0].view(np.float32)), "IF output against the oracle, call %d channel %d" % (
                k, c)
            assert _same(a1[c], ref[k][s][1]), "audio against the oracle, call %d channel %d" % (k, c)


@pytest.mark.parametrize("ro", [2, 3])
@pytest.mark.parametrize("channels", [72, 7], ids=["72ch-xcd-map", "7ch-channel-major"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_interior_and_edge_tiles_give_the_same_bits(pkg, stations, reference, fmt, channels, ro):
    """Every input format, both block maps (72 channels: a multiple of 8, blocks dealt over the XCDs; 7: channel-major),
    two and three outputs per lane."""
    _check(pkg, stations, reference, fmt, channels, ro)


def test_channels_sharing_captures(pkg, stations, reference):
    """fmd_batch_set_channels_per_capture: 8 consecutive channels tune the same capture."""
    _check(pkg, stations, reference, "f32", 72, 2, station_of=lambda c: (c // 8) % K, cpc=8)


def test_capture_map_form(pkg, stations, reference):
    """fmd_batch_set_capture_map: the MAP form of the kernel, the walk table names each block's channel and capture."""
    cmap = (np.arange(72) * 5 + 3) % 9  # 9 captures, channels scattered over them
    _check(pkg, stations, reference, "s16", 72, 2, station_of=lambda c: int(cmap[c]) % K, cmap=cmap)


def test_concurrency_0(pkg, stations, reference):
    """calls not overlapped (one stream)"""
    _check(pkg, stations, reference, "u8", 72, 2, concurrency=0)


def test_overlapped_calls_consumed_a_call_late(pkg, stations, reference):
    """Concurrency 2, device calls submitted back to back and their outputs consumed one call late: audio of every
    channel equal between the two runs and the stations' first channels equal to the oracle's."""
    import torch
    channels, lag = 72, 1
    x = stations["f32"]
    ref = reference("f32")
    idx = torch.arange(channels, device="cuda") % K
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for interior in (True, False):
        b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), channels, record_callbacks=False)
        b.set_concurrency(2)
        b.debug_set("fir_nt", 2)
        b.debug_set("fir_ro", 2 if interior else -2)
        a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
        keep, outs, start, pending = [], [], 0, 0
        for n in SEQUENCE:
            if n == "reset":
                b.wait(stream=st)
                b.reset()
                pending = 0
                continue
            n_al = (n + 1) // 2 * 2
            q = np.zeros((K, 2 * n_al), dtype=np.float32)
            q[:, :2 * n] = x[:, 2 * start:2 * (start + n)]
            d_iq = torch.from_numpy(q).cuda()[idx].contiguous()
            d_out = torch.zeros((channels, a_stride), dtype=torch.float32, device="cuda")
            keep.append(d_iq)
            nf = b.process_device(d_iq.data_ptr(), n_al, n, d_out.data_ptr(), a_stride, st)
            outs.append((d_out, nf))
            pending += 1
            if pending > lag:
                b.wait(stream=st, lag=lag)
            start += n
        b.wait(stream=st)
        torch.cuda.synchronize()
        runs.append([o[:, :nf].cpu().numpy() for o, nf in outs])
        b.close()
    for k, (a1, a0) in enumerate(zip(*runs)):
        assert _same(a1, a0), "audio, call %d" % k
        for s in range(K):
            assert _same(a1[s], ref[k][s][1]), "audio against the oracle, call %d station %d" % (k, s)
