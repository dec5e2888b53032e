"""CPU-only checks of the band splitter's specification (include/fmd.h, fmd_split_*; tests/split_spec.py): the numpy
model is the CPU oracle's cFineTuner + cDownsampleFilter bit for bit (its `demod` tap) over ragged call sizes, a
retune of the model is a fresh model from the next call on, the comparison can fail, and plan_bands covers a band."""
import numpy as np
import pytest

import split_spec as ss

# (fs, R, T, K, shift)
GEOMETRIES = [(9.6e6, 4, 96, 32, -7), (9.6e6, 4, 96, 64, 11), (19.2e6, 8, 192, 64, 30), (10e6, 4, 100, 48, 3),
              (9.6e6, 3, 64, 24, 5), (9.6e6, 8, 100, 200, -49), (9.6e6, 2, 64, 2, 1), (9.6e6, 3, 7, 24, 3),
              (19.2e6, 8, 1024, 1024, -300)]


def call_sizes(R, K):
    return [1, 1, 3, K - 1, K, K + 1, R - 1, 2, 40000, 1, 255, 256, 257, 4096, 4099, 8192, 1001, 5000]


def _iq(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * 0.3).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _oracle_rows(oracle, fs, R, T, K, shift, blocks):
    dec = oracle.OracleDecoder(fs, 0.0, downsample=R, table_size=T, if_filter_order=K, tuning_shift=shift)
    out = []
    for x in blocks:
        dec.process_stream(x.reshape(-1))
        out.append(dec.taps()["demod"])
    dec.close()
    return out


def _blocks(R, K, seed=1):
    sizes = call_sizes(R, K)
    x = _iq(sum(sizes), seed)
    edges = np.cumsum([0] + sizes)
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("fs,R,T,K,shift", GEOMETRIES)
def test_model_is_the_oracles_demod_tap_bit_for_bit(oracle, fs, R, T, K, shift):
    blocks = _blocks(R, K, seed=K + T)
    model = ss.SplitSpec(R, [shift], filter_order=K, table_size=T, out_scale=1.0)
    assert model.cutoff == 0.6 / R
    ref = _oracle_rows(oracle, fs, R, T, K, shift, blocks)
    q = 0
    for i, (x, want) in enumerate(zip(blocks, ref)):
        got = model.push(x)[0]
        assert got.size == ss.count(q, len(x), R) == want.size < 32717, (i, got.size, want.size)
        assert np.array_equal(_bits(got), _bits(want)), (i, len(x))
        q += len(x)


def test_set_shifts_equals_a_fresh_model_from_the_next_call(oracle):
    R, K, T = 4, 32, 96
    blocks = _blocks(R, K, seed=5)[:12]
    a = ss.SplitSpec(R, [-7, 3], filter_order=K, table_size=T)
    fresh = ss.SplitSpec(R, [11, 3], filter_order=K, table_size=T)
    for i, x in enumerate(blocks):
        if i == 6:
            a.set_shifts([11, 3])
        ya, yf = a.push(x), fresh.push(x)
        assert np.array_equal(_bits(ya[1]), _bits(yf[1])), i
        if i >= 6:
            assert np.array_equal(_bits(ya[0]), _bits(yf[0])), i
    # ... and the retuned row did differ before the retune (the two shifts are two bands)
    b = ss.SplitSpec(R, [-7], filter_order=K, table_size=T)
    c = ss.SplitSpec(R, [11], filter_order=K, table_size=T)
    x = np.concatenate(blocks)
    assert not np.array_equal(_bits(b.push(x)), _bits(c.push(x)))


@pytest.mark.parametrize("wrong", ["forget_history", "forget_phase"])
def test_a_model_without_history_or_phase_differs_from_the_oracle(oracle, wrong):
    fs, R, T, K, shift = 9.6e6, 4, 96, 32, -7
    blocks = _blocks(R, K, seed=9)
    ref = _oracle_rows(oracle, fs, R, T, K, shift, blocks)
    model = ss.SplitSpec(R, [shift], filter_order=K, table_size=T, out_scale=1.0, **{wrong: True})
    same = []
    for x, want in zip(blocks, ref):
        got = model.push(x)[0]
        same.append(got.size == want.size and np.array_equal(_bits(got), _bits(want)))
    assert not all(same), wrong


def test_count_is_the_multiples_of_r_inside_the_call():
    for R in (2, 3, 8):
        q = 0
        for n in (1, 1, 3, R - 1, R, R + 1, 17, 1000):
            assert ss.count(q, n, R) == sum(1 for k in range(q, q + n) if k % R == 0)
            q += n


def test_plan_bands_covers_every_station_once_on_the_raster():
    from importlib import import_module

    from __graft_entry__ import load_package
    split = import_module(load_package().__name__ + ".split")
    fs, R, T = 19.2e6, 8, 192
    step = fs / T                                 # 100 kHz
    cutoff = 0.6 / R
    usable = (1.0 - cutoff * R) * fs / R - 100e3  # alias-free half width minus the station's own 100 kHz
    rng = np.random.default_rng(3)
    stations = np.sort(rng.choice(np.arange(-90, 91), size=60, replace=False)) * 100e3 + 12.5e3
    shifts, where = split.plan_bands(fs, R, T, stations, usable)
    assert len(where) == len(stations) and len(set(shifts)) == len(shifts)
    centres = [-s * step for s in shifts]
    for f, (band, off) in zip(stations, where):
        assert 0 <= band < len(shifts)
        assert abs(off) <= usable + 1e-6
        assert abs(centres[band] + off - f) < 1e-3
        # covered once: no other band's assignment is made, and the centre is a whole number of tuner steps
    assert all(isinstance(s, int) and abs(s) <= T // 2 for s in shifts)
    # greedy cover: no more bands than the span needs, +1
    assert len(shifts) <= int(np.ceil((stations[-1] - stations[0]) / (2 * usable))) + 1
    with pytest.raises(ValueError):
        split.plan_bands(fs, R, 4, stations, 1e3)  # a raster coarser than the usable width cannot cover
