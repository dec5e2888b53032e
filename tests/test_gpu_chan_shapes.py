"""The channeliser's kernels (k_chan, k_chan_real, csrc/fmd_k_chan.hip.h) and its host table (chan_upload_table) held
to tests/chan_model.py -- the kernels' arithmetic in numpy, proved on the CPU by tests/test_chan_model_cpu.py -- in
bits, at the shapes the other channeliser tests never create: more than 16 rows a capture (rows 8 .. 15 of a block, a
second and a fifth row block, a wave that takes a second block, a partly filled last block), a second capture of such a
channeliser, set_shifts that moves rows between blocks, int16 rows and integer input there, odd N on the complex
kernel, N of 2 .. 5, complex N 255 and 256, real N 511, D 2 and 256, K 2 and 4096.

Every stream is 200 D + 7 samples from q = 0 in ragged calls (chan_model.call_sizes).  Complex rows equal the model's
bits; real rows equal them but for the sign of a zero (chan_real_spec.same_but_zero_signs).  Every output buffer has
two guard rows behind the last row and a guard tail behind every row's count, filled with a sentinel that must stay.
A failure names geometry, shape, capture, row and the first differing output, and says whether the row is the model's
row of another (capture, row): the signature of a table or row-mapping fault."""
from importlib import import_module

import numpy as np
import pytest

import chan_model as cm
import chan_spec as cs
import split_spec as ss
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

FS = 9.6e6
SENTINEL = 0x5A5A5A5A
F32 = np.float32
ANCHOR = (24, 11, 88)
GUARD_ROWS, GUARD_TAIL = 2, 4
KIND = lambda real: "real" if real else "complex"


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def chan(pkg):
    return import_module(pkg.__name__ + ".chan")


def _what(geom, G, B, real, note=""):
    return "%s %s %dx%d%s" % (cm.geom_id(geom), KIND(real), G, B, note and " " + note)


def _cut(x, sizes, per=1):
    e = np.cumsum([0] + list(sizes))
    return [x[:, per * a:per * b] for a, b in zip(e[:-1], e[1:])]


def _device_block(x):
    """[G, ...] on the device, captures a multiple of 4 elements apart (four real samples, two IQ samples)"""
    import torch
    a = np.ascontiguousarray(x).reshape(x.shape[0], -1)
    pad = -a.shape[1] % 4 + 4
    buf = np.zeros((a.shape[0], a.shape[1] + pad), a.dtype)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).cuda()[:, :a.shape[1]]


def _samples(ch, x):
    return x.shape[1] if (ch.real or x.ndim == 3) else x.shape[1] // 2


def _out(ch, n, rows=None):
    """(the whole buffer, the tensor of the call's rows): rows + GUARD_ROWS rows of out_stride + GUARD_TAIL samples,
    all sentinel"""
    import torch
    stride = ch.out_stride(n, rows) + GUARD_TAIL
    total = ch.rows + GUARD_ROWS
    if rows is np.int16:
        whole = torch.full((total, stride), SENTINEL, dtype=torch.int32, device="cuda")
        t = whole.view(torch.int16).view(total, stride, 2)
    else:
        whole = torch.full((total, 2 * stride), SENTINEL, dtype=torch.int32, device="cuda")
        t = whole.view(torch.float32).view(torch.complex64)
    return whole, t[:ch.rows]


def _run(chan, geom, shifts, blocks, real, what, rows=None, stream=None, out_scale=0, new_shifts=None, change_at=None):
    """the blocks through a new channeliser, no synchronise between the calls: [G, B, total outputs (, 2)].  Checks
    every call's count, guard tails and guard rows.  new_shifts / change_at: set_shifts in front of call change_at."""
    import torch
    N, D, K = geom
    shifts = np.asarray(shifts, np.int32)
    G, B = shifts.shape
    ch = chan.Channeliser(FS, N, D, G, shifts, filter_order=K, real=real, out_scale=out_scale)
    assert ch.rows == G * B and ch.tile_samples == 32 * D
    calls = []
    for i, x in enumerate(blocks):
        if change_at is not None and i == change_at:
            ch.set_shifts(new_shifts)
        n = _samples(ch, x)
        d = _device_block(x)
        whole, out = _out(ch, n, rows)
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        _, m = ch.process(d, n, out=out, rows=rows, stream=stream.cuda_stream if stream is not None else None)
        calls.append((n, m, whole, d))
    torch.cuda.synchronize()
    q, got = 0, []
    for i, (n, m, whole, _) in enumerate(calls):
        assert m == ss.count(q, n, D), "%s call %d: %d outputs for %d samples behind %d" % (what, i, m, n, q)
        a = whole.cpu().numpy().reshape(G * B + GUARD_ROWS, -1)           # int32 words, 2 a float sample, 1 an int16 one
        per = 1 if rows is np.int16 else 2
        body = a[:G * B]
        assert np.all(body[:, per * m:] == SENTINEL), "%s call %d: a row's guard tail behind %d outputs is touched" % (
            what, i, m)
        assert np.all(a[G * B:] == SENTINEL), "%s call %d: the guard rows behind row %d are touched" % (what, i, G * B - 1)
        r = np.ascontiguousarray(body[:, :per * m])
        if m == 0:
            got.append(np.zeros((G * B, 0, 2), np.int16) if rows is np.int16 else np.zeros((G * B, 0), np.complex64))
        else:
            got.append(r.view(np.int16).reshape(G * B, m, 2) if rows is np.int16 else r.view(np.complex64))
        q += n
    ch.close()
    return np.concatenate(got, axis=1).reshape((G, B, -1) + got[0].shape[2:]), [m for _, m, _, _ in calls]


_device_cache = {}


def _device_rows(chan, geom, G, B, real, shift_rows=None):
    """the device's float rows of the G x B channeliser over the geometry's ragged calls, once per case"""
    N, D, K = geom
    x, sh, _, _ = cm.case(geom, G, B, real, shift_rows=shift_rows)
    key = (geom, G, B, real, sh.tobytes())
    if key not in _device_cache:
        _device_cache[key] = _run(chan, geom, sh, _cut(x, cm.call_sizes(D, K)), real, _what(geom, G, B, real))[0]
    return _device_cache[key]


def _hold(chan, geom, G, B, real, shift_rows=None):
    _, _, want, floor = cm.case(geom, G, B, real, shift_rows=shift_rows)
    assert cm.normal(floor), floor
    got = _device_rows(chan, geom, G, B, real, shift_rows)
    cm.assert_rows(got, want, _what(geom, G, B, real), zero_signs=real)
    return got


# ---------------------------------------------------------------------------------------------------------------
# a. the anchor: the shape the other channeliser tests hold against the definition

@pytest.mark.parametrize("real", [False, True], ids=KIND)
def test_a_the_anchor_shapes_rows_are_the_models_bits(chan, real):
    """(24, 11, 88), 3 x 5 rows with the shifts of tests/test_gpu_chan.py.  If this fails the model is wrong about the
    matrix instruction: nothing else in this file means anything until it passes."""
    got = _hold(chan, ANCHOR, 3, 5, real, shift_rows=cm.anchor_shifts(24))
    assert got.shape[2] >= 200 and np.abs(got).max() > 0.01
    assert cm.first_difference(got[2, 1], got[2, 2]) is None             # the duplicate shift: the same row twice


# ---------------------------------------------------------------------------------------------------------------
# b. many rows

MANY_B = [16, 17, 33, 70]


@pytest.mark.parametrize("real", [False, True], ids=KIND)
@pytest.mark.parametrize("B", MANY_B, ids=lambda b: "2x%d" % b)
@pytest.mark.parametrize("geom", cm.MANY, ids=cm.geom_id)
def test_b_every_row_of_many_is_the_models_bits_and_those_of_a_lone_row(chan, geom, B, real):
    N, D, K = geom
    got = _hold(chan, geom, 2, B, real)
    x, sh, _, _ = cm.case(geom, 2, B, real)
    # the header's claim across blocks: row (g, b) is the one row of a 1 x 1 channeliser with its shift on its capture
    rng = np.random.default_rng(100 * N + B)
    picks = sorted(set(b for b in (0, 7, 8, 15, 16, B - 1) if b < B) | set(int(b) for b in rng.choice(B, 2, replace=False)))
    other = _cut(x, cs.ragged(x.shape[1], [777, 2, 32 * D + 1, 5000]))
    for i, b in enumerate(picks):
        g = i % 2
        what = _what(geom, 2, B, real, "capture %d row %d against a 1x1 channeliser of shift %d" % (g, b, sh[g, b]))
        lone, _ = _run(chan, geom, sh[g:g + 1, b:b + 1], [blk[g:g + 1] for blk in other], real, what)
        at = cm.first_difference(got[g, b], lone[0, 0])
        assert at is None, "%s: first differing output %d (%r, alone %r)" % (what, at, got[g, b][at], lone[0, 0][at])


@pytest.mark.parametrize("real", [False, True], ids=KIND)
def test_b_seventy_rows_in_one_call_and_on_a_side_stream(chan, real):
    import torch
    geom, G, B = ANCHOR, 2, 70
    x, sh, want, _ = cm.case(geom, G, B, real)
    ragged = _device_rows(chan, geom, G, B, real)
    one, counts = _run(chan, geom, sh, [x], real, _what(geom, G, B, real, "one call"))
    assert counts == [want.shape[2]]
    cm.assert_rows(one, want, _what(geom, G, B, real, "one call"), zero_signs=real)
    side, _ = _run(chan, geom, sh, _cut(x, cm.call_sizes(11, 88)), real, _what(geom, G, B, real, "side stream"),
                   stream=torch.cuda.Stream())
    cm.assert_rows(side, want, _what(geom, G, B, real, "side stream"), zero_signs=real)
    assert one.tobytes() == ragged.tobytes() == side.tobytes()             # between device runs: bits, zeros too


# ---------------------------------------------------------------------------------------------------------------
# c. int16 rows past a block

def _loud(D):
    """tests/test_gpu_chan_real.py's: an out_scale that puts a part's RMS near 2.2 for noise of 0.3 RMS: some parts
    pass +-4.0, most do not"""
    return 4.8 * float(np.sqrt(D))


def _s16_sizes(D, K):
    """the ragged calls, the last one cut so that its count is odd"""
    sizes = cm.call_sizes(D, K)
    starts = np.cumsum([0] + sizes[:-1])
    if ss.count(int(starts[-1]), sizes[-1], D) % 2 == 0:
        sizes = sizes[:-1] + [D, sizes[-1] - D]
    return sizes


@pytest.mark.parametrize("real", [False, True], ids=KIND)
@pytest.mark.parametrize("B", [33, 70], ids=lambda b: "2x%d" % b)
def test_c_int16_rows_past_a_block_are_the_conversion_of_the_models_rows(chan, B, real):
    geom, G = ANCHOR, 2
    N, D, K = geom
    x, sh, want, floor = cm.case(geom, G, B, real, out_scale=_loud(D))
    assert cm.normal(floor)
    sizes = _s16_sizes(D, K)
    what = _what(geom, G, B, real, "int16 rows")
    got, counts = _run(chan, geom, sh, _cut(x, sizes), real, what, rows=np.int16, out_scale=_loud(D))
    assert counts[-1] % 2 == 1 and any(c and c % 2 == 0 for c in counts), counts   # the 4-byte and the 8-byte store
    want16 = cm.rows_s16(want)
    assert got.dtype == np.int16 and got.shape == want16.shape == (G, B, want.shape[2], 2)
    cm.assert_rows(got, want16, what)
    full = (want16 == 32767) | (want16 == -32768)
    assert (want16 == 32767).any() and (want16 == -32768).any() and full.mean() < 0.25
    assert full[:, 16:].any()                                              # saturated samples past the first block


# ---------------------------------------------------------------------------------------------------------------
# d. set_shifts past a block

@pytest.mark.parametrize("real", [False, True], ids=KIND)
def test_d_set_shifts_moves_rows_between_blocks_with_calls_in_flight(chan, real):
    geom, G, B = ANCHOR, 2, 37
    N, D, K = geom
    x, sh, old, _ = cm.case(geom, G, B, real)
    rot = np.roll(sh, 19, axis=1)
    _, _, new, _ = cm.case(geom, G, B, real, shift_rows=rot)
    sizes = cm.call_sizes(D, K)
    assert len(sizes) == 8
    what = _what(geom, G, B, real, "set_shifts in front of call 4")
    got, counts = _run(chan, geom, sh, _cut(x, sizes), real, what, new_shifts=rot, change_at=4)
    cut = sum(counts[:4])
    assert 0 < cut < old.shape[2] - 100
    cm.assert_rows(got[:, :, :cut], old[:, :, :cut], what + ", before", zero_signs=real)
    cm.assert_rows(got[:, :, cut:], new[:, :, cut:], what + ", after", zero_signs=real)
    assert len(cm.row_faults(got[:, :, cut:], old[:, :, cut:], what)) >= G * (B - 3)   # the change is no no-op


# ---------------------------------------------------------------------------------------------------------------
# e. N and limit edges

@pytest.mark.parametrize("geom,real", [(g, False) for g in cm.EDGE] + [(g, True) for g in cm.REAL_EDGE],
                         ids=lambda v: cm.geom_id(v) if isinstance(v, tuple) else KIND(v))
def test_e_n_and_limit_edges_are_the_models_bits(chan, geom, real):
    """N 2 .. 5 (every prefetch index clamped), odd N on the complex kernel, complex N 255 / 256, real N 511, D 2 and
    256, K 2 and 4096; 2 x 17 rows: a second, partly filled row block at each.  None of these geometries is refused
    for its LDS footprint."""
    _hold(chan, geom, 2, 17, real)


# ---------------------------------------------------------------------------------------------------------------
# f. integer input past a block

def test_f_int16_iq_input_past_a_block_is_the_model_on_the_converted_block(chan):
    geom, G, B = ANCHOR, 2, 33
    N, D, K = geom
    xf, sh, _, _ = cm.case(geom, G, B, False)
    q = np.clip(np.rint(xf.astype(np.float64) * 32767), -32768, 32767).astype(np.int16)      # [G, n, 2]
    q[:, :2] = [[-32768, 32767], [-1, 1]]
    conv = q.astype(F32) * F32(2.0 ** -15)
    res = [cm.run(conv[g], N, D, K, sh[g]) for g in range(G)]
    assert all(cm.normal(r.floor) for r in res)
    what = _what(geom, G, B, False, "int16 IQ input")
    got, _ = _run(chan, geom, sh, _cut(q.reshape(G, -1), cm.call_sizes(D, K), per=2), False, what)
    cm.assert_rows(got, np.stack([r.rows for r in res]), what)
