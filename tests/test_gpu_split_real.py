"""The real band splitter on the GPU (fmd_split_create_real, FMD_REAL_*; csrc/fmd_k_split.hip.h, DESIGN.md section
9.14) against its definition: the rows of a real capture are tests/split_spec.py's on (convert(v), +0) pairs
(tests/split_real_spec.py), and the rows of a complex splitter of the same parameters fed those pairs.

Every comparison is equality of the float bits (NaN for NaN where the input holds non-finite values): no tolerance
but the one reception check of the end-to-end test, which compares two runs of the CPU oracle.  Rows are pre-filled
with a sentinel, and what lies behind a call's count must still be the sentinel.
"""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest

import split_real_spec as rs
import split_spec as ss
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

FS = 19.2e6
SENTINEL = 0x5A5A5A5A
# (R, K, T, cutoff, out_scale); 0 = the default.  The two compile-time forms; odd R; a window shorter than one
# four-sample load; the generic form at the largest K and T; the largest R with the smallest tile (there the real
# tile, a 4-byte raw window, is larger than the complex one)
GEOMETRIES = [(4, 32, 96, 0.0, 0.0), (8, 64, 192, 0.5 / 8, 1.0), (3, 24, 7, 0.5 / 3, 0.3), (2, 2, 64, 0.0, 0.5),
              (8, 1024, 1024, 0.0, 0.0), (64, 512, 64, 0.0, 0.0)]
GEOMETRY_IDS = ["R4K32T96", "R8K64T192", "R3K24T7", "R2K2T64", "R8K1024T1024", "R64K512T64"]
DTYPES = {"f32": np.float32, "s8": np.int8, "s16": np.int16}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def split(pkg):
    return import_module(pkg.__name__ + ".split")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _same_or_nan(got, want):
    """NaN where `want` has NaN, its bits otherwise (per float)"""
    g, w = np.ascontiguousarray(got).view(np.float32), np.ascontiguousarray(want).view(np.float32)
    if g.shape != w.shape:
        return False
    nan = np.isnan(w)
    return bool(np.all(np.isnan(g[nan])) and np.array_equal(g[~nan].view(np.uint32), w[~nan].view(np.uint32)))


def _shifts(G, B, T):
    """a shift per row: both signs, beyond +-T too, not the same for any two rows of a capture"""
    return np.array([[(7 * b - 11 * g + 3) * (-1) ** (g + b) for b in range(B)] for g in range(G)], np.int32)


def _sizes(R, K, tile):
    """one stream of call sizes: around K and R, one big call, then the kernel's tile with every residue of the
    four-sample load in front of and behind it"""
    return [1, 1, 3, K - 1, K, K + 1, R - 1, 2, 40000, 1, tile - 1, tile, tile + 1, tile + 2, tile + 3, 1, 3]


@functools.lru_cache(maxsize=None)
def _capture(g, n, seed=0, dt="f32"):
    rng = np.random.default_rng(1000 * seed + g)
    x = (rng.standard_normal(n) * 0.3).astype(np.float32)
    if dt == "f32":
        return x
    info = np.iinfo(DTYPES[dt])
    return np.clip(np.rint(x.astype(np.float64) * info.max), info.min, info.max).astype(DTYPES[dt])


def _blocks(G, sizes, seed=0, dt="f32"):
    """per call [G, n] real samples"""
    total = sum(sizes)
    x = np.stack([_capture(g, total, seed, dt) for g in range(G)])
    e = np.cumsum([0] + list(sizes))
    return [x[:, a:b] for a, b in zip(e[:-1], e[1:])]


def _models(geom, shifts, cls=rs.RealSplitSpec):
    R, K, T, cutoff, scale = geom
    return [cls(R, sh, filter_order=K, cutoff=cutoff, table_size=T, out_scale=scale) for sh in shifts]


def _push(models, x):
    """[G, n] -> [G B, count]"""
    return np.concatenate([m.push(x[g]) for g, m in enumerate(models)])


@functools.lru_cache(maxsize=None)
def _reference(geom, tile, dt="f32", G=3, B=5):
    """the model's rows of the G x B splitter over the geometry's call sizes, computed once: per call [G, B, count]"""
    R, K, T = geom[:3]
    models = _models(geom, _shifts(3, 5, T)[:G, :B])
    return [_push(models, x).reshape(G, B, -1) for x in _blocks(G, _sizes(R, K, tile), dt=dt)]


def _make(split, geom, shifts, real=True, **kw):
    R, K, T, cutoff, scale = geom
    shifts = np.asarray(shifts, np.int32)
    return split.Splitter(FS, R, shifts.shape[0], shifts, filter_order=K, cutoff=cutoff, table_size=T,
                          out_scale=scale, real=real, **kw)


def _device_block(x, pad=0):
    """[G, n] real samples (or [G, n, 2] float32 IQ) on the device, rows `pad` elements longer than the call and a
    multiple of four elements apart (the real call's alignment rule; two IQ samples of a complex one)"""
    import torch
    a = np.ascontiguousarray(x).reshape(x.shape[0], -1)
    pad += -(a.shape[1] + pad) % 4
    buf = np.zeros((a.shape[0], a.shape[1] + pad), a.dtype)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).cuda()[:, :a.shape[1]]


def _prepare(sp, x, pad=0):
    """a call's device buffers: (input on the device, out tensor pre-filled with the sentinel, samples)"""
    import torch
    n = x.shape[1]
    d = _device_block(x, pad)
    out = torch.full((sp.rows, 2 * sp.out_stride(n)), SENTINEL, dtype=torch.int32,
                     device="cuda").view(torch.float32).view(torch.complex64)
    return d, out, n


def _submit(sp, x, stream=None, pad=0):
    """one call: returns (out tensor pre-filled with the sentinel, count, input)"""
    import torch
    d, out, n = _prepare(sp, x, pad)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    _, m = sp.process(d, n, out=out, stream=stream.cuda_stream if stream is not None else None)
    return out, m, d


def _rows(out, m):
    """(rows [rows, m] complex64, tails untouched?)"""
    a = out.cpu().numpy()
    return a[:, :m], bool(np.all(np.ascontiguousarray(a[:, m:]).view(np.uint32) == SENTINEL))


def _call(sp, x, **kw):
    """one call's rows, tails checked"""
    out, m, _ = _submit(sp, x, **kw)
    got, tails = _rows(out, m)
    assert tails
    return got


def _zero_q(x):
    """[G, n] float32 -> [G, n, 2] float32 with Q = +0"""
    z = np.zeros(x.shape + (2,), np.float32)
    z[..., 0] = x
    return z


# ---------------------------------------------------------------------------------------------------------------
# 1. the definition over ragged calls

def _ragged(split, geom, G, B, dt):
    R, K, T = geom[:3]
    sp = _make(split, geom, _shifts(3, 5, T)[:G, :B])
    assert sp.real and sp.rows == G * B and sp.out_rate == FS / R and sp.tile_samples % R == 0
    sizes = _sizes(R, K, sp.tile_samples)
    ref = _reference(geom, sp.tile_samples, dt, *((3, 5) if dt == "f32" else (G, B)))
    q = 0
    for i, x in enumerate(_blocks(G, sizes, dt=dt)):
        out, m, _ = _submit(sp, x)
        assert m == ss.count(q, sizes[i], R) == ref[i].shape[2], (i, m)
        got, tails = _rows(out, m)
        assert tails, i
        assert _same(got, ref[i][:G, :B].reshape(G * B, -1)), (i, sizes[i])
        q += sizes[i]
    sp.close()


@pytest.mark.parametrize("shape", [(1, 1), (3, 5)], ids=["1x1", "3x5"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=GEOMETRY_IDS)
def test_rows_equal_the_definition_over_ragged_calls(split, geom, shape):
    _ragged(split, geom, shape[0], shape[1], "f32")


@pytest.mark.parametrize("dt", ["s8", "s16"])
@pytest.mark.parametrize("geom", [GEOMETRIES[0], GEOMETRIES[1], GEOMETRIES[2]], ids=GEOMETRY_IDS[:3])
def test_integer_rows_equal_the_definition_over_ragged_calls(split, geom, dt):
    _ragged(split, geom, 2, 3, dt)


def test_the_real_tile_is_never_smaller_than_the_complex_one(split):
    """a 4-byte raw window leaves room for more outputs where LDS bounds the generic form's tile; the compile-time
    forms and the geometries that fit 256 outputs either way keep them"""
    tiles = {}
    for geom, name in zip(GEOMETRIES, GEOMETRY_IDS):
        T = geom[2]
        sp_r, sp_c = _make(split, geom, _shifts(1, 1, T)), _make(split, geom, _shifts(1, 1, T), real=False)
        tiles[name] = (sp_r.tile_samples, sp_c.tile_samples)
        sp_r.close()
        sp_c.close()
    assert all(r >= c for r, c in tiles.values()), tiles
    assert tiles["R4K32T96"] == (1024, 1024) and tiles["R8K64T192"] == (2048, 2048), tiles
    assert tiles["R64K512T64"][0] > tiles["R64K512T64"][1], tiles


# ---------------------------------------------------------------------------------------------------------------
# 2. the same bits as the complex path fed zero-Q pairs, poison included

@pytest.mark.parametrize("geom", [GEOMETRIES[0], GEOMETRIES[5]], ids=[GEOMETRY_IDS[0], GEOMETRY_IDS[5]])
def test_rows_equal_a_complex_splitters_on_zero_q_pairs_and_poison_stays_in_its_capture(split, geom):
    R, K, T = geom[:3]
    G, B = 3, 2
    shifts = _shifts(3, 5, T)[:G, :B]
    shifts[1, 0] = 0                                  # (a table that holds exact zeros and ones)
    probe = _make(split, geom, shifts)
    tile = probe.tile_samples
    probe.close()
    sizes = [2 * tile + 41, K - 5, 3 * tile + 2, 1, 503 + 2 * K]
    clean = [x.copy() for x in _blocks(G, sizes, seed=6)]
    bad = [x.copy() for x in clean]
    den = np.float32(1e-41)
    bad[0][1, 5:9] = np.float32(-0.0)
    bad[0][1, tile - 1] = np.nan                      # a tile's last input sample
    bad[0][1, tile] = den                             # ... and the next tile's first
    bad[0][1, sizes[0] - 3] = np.inf                  # inside the carried history of call 1 (shorter than K)
    bad[1][1, 2] = np.float32(-3e-39)
    bad[2][1, 7] = np.float32(3e38)
    bad[2][1, sizes[2] - 1] = np.nan                  # the last sample of a call
    bad[3][1, 0] = -np.inf                            # a call of one sample
    bad[4][1, 100:140] = den
    bad[4][1, 140:150] = np.float32(-0.0)

    def run(blocks, real):
        sp = _make(split, geom, shifts, real=real)
        rows = [_call(sp, x if real else _zero_q(x)).reshape(G, B, -1) for x in blocks]
        sp.close()
        return rows

    real_bad, real_clean, cplx_bad = run(bad, True), run(clean, True), run(bad, False)
    models = _models(geom, shifts)
    seen_nan = seen_finite = False
    for i, x in enumerate(bad):
        assert _same_or_nan(real_bad[i], cplx_bad[i]), i
        want = models[1].push(x[1])
        assert _same_or_nan(real_bad[i][1], want), i
        seen_nan |= bool(np.isnan(want.view(np.float32)).any())
        seen_finite |= bool(np.isfinite(want.view(np.float32)).any())
        for g in (0, 2):
            assert _same(real_bad[i][g], real_clean[i][g]), (i, g)
            assert _same(real_bad[i][g], models[g].push(x[g])), (i, g)
    assert seen_nan and seen_finite
    # the poison dies out with the history
    assert _same(real_bad[4][1][:, -3:], real_clean[4][1][:, -3:])


# ---------------------------------------------------------------------------------------------------------------
# 3. integer exactness

@pytest.mark.parametrize("dt", ["s8", "s16"])
def test_integer_input_gives_the_bits_of_the_float_call_on_the_converted_block(split, dt):
    """every int8 value, a sweep of int16 values with both ends; three ragged calls, captures an odd number of
    four-sample groups apart; then one shared capture (G = 1, stride 0)"""
    geom = GEOMETRIES[0]
    R, K, T = geom[:3]
    sizes = [4099, 31, 6001]
    total = sum(sizes)
    if dt == "s8":
        values = np.arange(-128, 128).astype(np.int8)
    else:
        values = np.unique(np.concatenate([np.arange(-32768, 32768, 13), [-32768, -32767, -1, 0, 1, 32766, 32767]])
                           ).astype(np.int16)
    for G, B in ((3, 2), (1, 3)):
        rng = np.random.default_rng(77 + G)
        q = np.stack([rng.permutation(np.resize(values, total)) for _ in range(G)])
        assert all(np.unique(q[g]).size == values.size for g in range(G))
        xf = np.stack([rs.convert(q[g]) for g in range(G)])
        shifts = _shifts(3, 5, T)[:G, :B]
        sp_i, sp_f = _make(split, geom, shifts), _make(split, geom, shifts)
        models = _models(geom, shifts)
        at = 0
        for n in sizes:
            pad = 4 * ((n + 11) // 4 | 1) - n         # the capture stride: 4 * an odd number, >= n + 8
            got_i = _call(sp_i, q[:, at:at + n], pad=pad)
            got_f = _call(sp_f, xf[:, at:at + n], pad=pad)
            assert _same(got_f, _push(models, xf[:, at:at + n])) and _same(got_i, got_f), (G, n)
            at += n
        sp_i.close()
        sp_f.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. state and edits

def test_set_shifts_between_calls_in_flight_equals_fresh_real_splitters(split):
    """Ten calls submitted back to back behind a stretch of other work on the stream, set_shifts in front of calls 3
    and 7: from those calls on the rows are those of real splitters that had the new shifts from the start (the
    carried state is the raw history alone), the other rows keep their bits."""
    import torch
    geom = GEOMETRIES[0]
    R, K, T = geom[:3]
    G, B = 2, 3
    s0 = _shifts(3, 5, T)[:G, :B].copy()
    s3, s7 = s0.copy(), s0.copy()
    s3[0, 1], s3[1, 2] = 40, -5
    s7[:] = s3
    s7[0, 1], s7[1, 0] = -33, 17
    sizes = [30000, 17, 40960, 1, 29999, 41000, 31, 10240, 50000, 77]
    blocks = _blocks(G, sizes, seed=4)
    sp = _make(split, geom, s0)
    ready = [_prepare(sp, x) for x in blocks]
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
            sp.set_shifts(s3)
        if i == 7:
            sp.set_shifts(s7)
        d, out, n = ready[i]
        counts.append(sp.process(d, n, out=out)[1])
    in_flight = not blocker.query()
    versions = sp.debug_table_versions()
    torch.cuda.synchronize()
    del b
    assert in_flight, "the stretch of other work ended before the last call was submitted: nothing was in flight"
    assert versions == 3, versions
    fresh = {0: _models(geom, s0), 3: _models(geom, s3), 7: _models(geom, s7)}
    want = {k: [_push(ms, x).reshape(G, B, -1) for x in blocks] for k, ms in fresh.items()}
    for i, ((_, o, _), m) in enumerate(zip(ready, counts)):
        got, tails = _rows(o, m)
        assert tails, i
        k = 0 if i < 3 else 3 if i < 7 else 7
        assert _same(got.reshape(G, B, -1), want[k][i]), i
    assert _same(want[7][9][0, 0], want[0][9][0, 0]) and not _same(want[7][9][0, 1], want[0][9][0, 1])
    sp.close()


def test_reset_gives_the_rows_of_a_new_real_splitter(split):
    geom = GEOMETRIES[2]
    T = geom[2]
    shifts = _shifts(3, 5, T)[:2, :2]
    blocks = _blocks(2, [1000, 7, 2001], seed=5)
    sp = _make(split, geom, shifts)
    first = [_call(sp, x) for x in blocks]
    sp.reset()
    again = [_call(sp, x) for x in blocks]
    models = _models(geom, shifts)
    for i, x in enumerate(blocks):
        want = _push(models, x)
        assert _same(first[i], want) and _same(again[i], want), i
    sp.close()


def test_a_real_captures_rows_do_not_depend_on_the_geometry_or_the_stream(split):
    import torch
    geom = GEOMETRIES[1]
    T = geom[2]
    shifts = _shifts(3, 5, T)
    sizes = [1001, 5, 4097, 2 * 2048 + 1]
    blocks = _blocks(3, sizes, seed=2)
    side = torch.cuda.Stream()

    def run(caps, bands, stream=None):
        sp = _make(split, geom, shifts[caps][:, bands])
        outs = [_submit(sp, x[caps], stream=stream) for x in blocks]
        torch.cuda.synchronize()
        rows = [_rows(o, m)[0].reshape(len(caps), len(bands), -1) for o, m, _ in outs]
        sp.close()
        return rows

    full = run([0, 1, 2], [0, 1, 2, 3, 4])
    for g in range(3):
        one_capture = run([g], [0, 1, 2, 3, 4])
        one_row = run([g], [3])
        other_stream = run([g], [0, 1, 2, 3, 4], stream=side)
        for i in range(len(sizes)):
            assert _same(one_capture[i][0], full[i][g]), (g, i)
            assert _same(one_row[i][0, 0], full[i][g, 3]), (g, i)
            assert _same(other_stream[i][0], full[i][g]), (g, i)


# ---------------------------------------------------------------------------------------------------------------
# 5. refused calls of a live splitter

def test_refusals_leave_a_real_and_a_complex_splitter_as_they_were(pkg, split):
    """every refusal has a sentence naming its field, launches nothing and writes no count; the good call behind each
    one has the model's bits as if the bad one had not been made"""
    import torch
    geom = GEOMETRIES[0]
    R, K, T = geom[:3]
    G, B = 2, 2
    ERR_ARG, ERR_SIZE = -1, -3
    shifts = _shifts(3, 5, T)[:G, :B]
    lib, cnt = pkg.lib(), C.c_uint(12345)
    n = 1001
    real_cases = [  # (format, pointer offset in samples, stride: None = the tensor's, samples, code, words)
        (pkg.FMD_IQ_F32, 0, None, n, ERR_ARG, (b"real splitter", b"iq_format")),
        (pkg.FMD_IQ_S16, 0, None, n, ERR_ARG, (b"real splitter", b"iq_format")),
        (pkg.FMD_IQ_U8, 0, None, n, ERR_ARG, (b"real splitter", b"iq_format")),
        (17, 0, None, n, ERR_ARG, (b"iq_format must be one of FMD_IQ_F32",)),
        (pkg.FMD_REAL_F32, 2, None, n, ERR_ARG, (b"d_in", b"four real samples")),
        (pkg.FMD_REAL_F32, 0, -2, n, ERR_ARG, (b"in_capture_stride", b"four real samples")),
        (pkg.FMD_REAL_F32, 0, n - 1, n, ERR_ARG, (b"in_capture_stride", b"shorter")),
        (pkg.FMD_REAL_F32, 0, None, 0, ERR_SIZE, (b"samples",)),
        (pkg.FMD_REAL_F32, 0, None, 16777217, ERR_SIZE, (b"samples",)),
    ]
    blocks = _blocks(G, [n] * (len(real_cases) + 1), seed=8)
    sp = _make(split, geom, shifts)
    models = _models(geom, shifts)
    assert _same(_call(sp, blocks[0]), _push(models, blocks[0]))
    for i, (fmt, off, stride, samples, code, words) in enumerate(real_cases):
        x = blocks[i + 1]
        d, out, _ = _prepare(sp, x, pad=8)
        stride = d.stride(0) if stride is None else d.stride(0) + stride if stride < 0 else stride
        rc = lib.fmd_split_process_device(sp._h, d.data_ptr() + 4 * off, fmt, stride, samples, out.data_ptr(),
                                          out.stride(0), C.byref(cnt), None)
        msg = lib.fmd_last_error()
        assert rc == code, (i, rc, msg)
        assert all(w in msg for w in words) and len(msg.split()) >= 5, (i, msg)
        assert cnt.value == 12345, i
        torch.cuda.synchronize()
        assert bool(np.all(out.cpu().numpy().view(np.uint32) == SENTINEL)), i
        _, m = sp.process(d, n, out=out)
        got, tails = _rows(out, m)
        assert tails and _same(got, _push(models, x)), i
    # the host entry point checks the kind too
    host_out = np.zeros((G * B, 512), np.complex64)
    rc = lib.fmd_split_process_host(sp._h, np.zeros((G, 2 * n), np.float32).ctypes.data, pkg.FMD_IQ_F32, n, n,
                                    host_out.ctypes.data, 512, C.byref(cnt))
    assert rc == ERR_ARG and b"real splitter" in lib.fmd_last_error() and cnt.value == 12345
    x = blocks[0]
    assert _same(sp.process_host(x), _push(models, x))
    # the Python layer: the splitter's kind decides what a dtype means
    with pytest.raises(pkg.FmdError, match="real-sample"):
        sp.process(torch.zeros((G, 64), dtype=torch.complex64, device="cuda"), 64)
    with pytest.raises(pkg.FmdError, match="real-sample"):
        sp.process(torch.zeros((G, 64), dtype=torch.uint8, device="cuda"), 64)
    with pytest.raises(pkg.FmdError, match="real-sample"):
        sp.process_host(np.zeros((G, 64), np.complex64))
    with pytest.raises(pkg.FmdError, match="real-sample"):
        sp.process_host(np.zeros((G, 64), np.uint8))
    assert _same(_call(sp, blocks[1]), _push(models, blocks[1]))
    sp.close()

    # a complex splitter refuses FMD_REAL_* and goes on as it was
    spc = _make(split, geom, shifts, real=False)
    cmodels = _models(geom, shifts, cls=ss.SplitSpec)
    cblocks = [_zero_q(b) + np.float32(0.125) for b in blocks[:4]]   # (Q is not zero here)
    for i, fmt in enumerate((pkg.FMD_REAL_F32, pkg.FMD_REAL_S8, pkg.FMD_REAL_S16)):
        x = cblocks[i]
        d, out, _ = _prepare(spc, x, pad=8)
        rc = lib.fmd_split_process_device(spc._h, d.data_ptr(), fmt, d.stride(0) // 2, n, out.data_ptr(),
                                          out.stride(0), C.byref(cnt), None)
        msg = lib.fmd_last_error()
        assert rc == ERR_ARG and b"complex splitter" in msg and b"iq_format" in msg, (fmt, rc, msg)
        assert cnt.value == 12345
        torch.cuda.synchronize()
        assert bool(np.all(out.cpu().numpy().view(np.uint32) == SENTINEL)), fmt
        _, m = spc.process(d, n, out=out)
        got, tails = _rows(out, m)
        assert tails and _same(got, _push(cmodels, x)), fmt
    spc.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. the host entry point

@pytest.mark.parametrize("dt", ["f32", "s8", "s16"])
def test_host_call_gives_the_device_calls_bits_at_an_odd_row_stride_and_an_unaligned_pointer(split, dt):
    geom = GEOMETRIES[2]
    T = geom[2]
    shifts = _shifts(3, 5, T)[:2, :3]
    blocks = _blocks(2, [999, 3, 4001, 1], seed=7, dt=dt)
    sp_d, sp_h, sp_o = (_make(split, geom, shifts) for _ in range(3))
    for i, x in enumerate(blocks):
        want = _call(sp_d, x)
        got = sp_h.process_host(x)
        # one element behind an aligned buffer: no multiple of four samples, for int8 no multiple of anything
        shifted = np.zeros(x.size + 1, x.dtype)[1:].reshape(x.shape)
        shifted[:] = x
        assert shifted.ctypes.data % (4 * x.itemsize) != 0
        got_odd = sp_o.process_host(shifted, out_stride=(want.shape[1] | 1) + 2)
        assert _same(got, want) and _same(got_odd, want), i
    for s in (sp_d, sp_h, sp_o):
        s.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. end to end: a real capture, mirrors included -> splitter -> capture map -> batch on one stream

def test_four_stations_of_a_real_capture_decode_like_the_oracle_behind_the_model(pkg, split, oracle, fmsig):
    import torch
    fs, R, T = 9.6e6, 4, 96                      # tuner raster 100 kHz; bands at 2.4 MS/s
    n_in, calls = 4 * 16384, 6
    band_shifts = [-20, 28]                      # centres +2.0 MHz and -2.8 MHz
    stations = [(2.0e6, 0, 0), (1.2e6, 0, 8), (-2.8e6, 1, 0), (-3.6e6, 1, 8)]  # (offset, band, shift in the band)
    wide = np.zeros(2 * n_in * calls, np.float32)
    for k, (f, _, _) in enumerate(stations):
        p = fmsig.default_params(fs, f_offset=f, amp=0.2, noise_sigma=0.002, seed=500 + k, pi=0x7200 + k,
                                 ps="REAL%d" % k)
        wide = wide + fmsig.generate_f32(p, 0, n_in * calls)
    wide = wide.reshape(calls, n_in, 2)
    real = np.ascontiguousarray(wide[:, :, 0])   # the I part alone: every station and its mirror
    model = rs.RealSplitSpec(R, band_shifts, table_size=T)
    cmodel = ss.SplitSpec(R, band_shifts, table_size=T)
    sp = split.Splitter(fs, R, 1, [band_shifts], table_size=T, real=True)
    D, Tb = 11, 24                               # the batch at 2.4 MS/s: raster 100 kHz
    b = pkg.Batch(pkg.make_params(fs / R, 0.0, 48000.0, 15000.0, D, table_size=Tb), len(stations),
                  tuning_shifts=np.array([s for _, _, s in stations], np.int32))
    b.set_capture_map(np.array([band for _, band, _ in stations], np.uint32), 2)

    def decoders():
        return [oracle.OracleDecoder(fs / R, 0.0, 48000.0, 15000.0, D, table_size=Tb, tuning_shift=s)
                for _, _, s in stations]

    orc, orc_c = decoders(), decoders()
    n_band = n_in // R
    a_stride = (b.max_audio_floats(n_band) + 63) // 64 * 64
    stream = torch.cuda.current_stream().cuda_stream
    audio, counts, keep = [], [], []
    for j in range(calls):
        d = _device_block(real[j][None, :])
        bands, m = sp.process(d, n_in, stream=stream)
        assert m == n_band
        a = torch.zeros((len(stations), a_stride), dtype=torch.float32, device="cuda")
        counts.append(b.process_device(bands.data_ptr(), bands.stride(0), m, a.data_ptr(), a_stride, stream))
        audio.append(a)
        keep.append((d, bands))
    b.wait(stream=stream)
    groups = b.collect_rds_array()
    torch.cuda.synchronize()
    want_audio = [[] for _ in stations]
    for j in range(calls):
        y, yc = model.push(real[j]), cmodel.push(wide[j])
        for c, (_, band, _) in enumerate(stations):
            want_audio[c].append(orc[c].process_stream(y[band].view(np.float32)))
            orc_c[c].process_stream(yc[band].view(np.float32))
    for c in range(len(stations)):
        for j in range(calls):
            got = audio[j][c, :counts[j]].cpu().numpy()
            assert _same(got, want_audio[c][j]), (c, j)
        st, so, sc = b.status(c), orc[c].status(), orc_c[c].status()
        assert (bool(st.stereo_detected), np.float32(st.tuning_offset), np.float32(st.interface_level),
                np.float32(st.pilot_level)) == (bool(so.stereo), np.float32(so.tuning_offset),
                                                np.float32(so.if_level), np.float32(so.pilot_level)), c
        # received, not only reproduced: the pilot behind the real capture (half the amplitude, the mirrors of all
        # four stations beside it) is the pilot behind the complex capture of the same stations, within 2 %
        print("station %d: pilot_level real %.4f, complex %.4f" % (c, so.pilot_level, sc.pilot_level))
        assert sc.pilot_level > 0.05 and abs(so.pilot_level - sc.pilot_level) <= 0.02 * sc.pilot_level, c
        # (41 ms of signal: neither side has detected stereo or completed an RDS group; the batch invents neither)
        got_groups = [tuple(int(v) for v in bl) for ch, _, bl in groups if int(ch) == c]
        assert got_groups == [bl for _, bl in orc[c].rds_groups()], c
    b.close()
    sp.close()
