"""Why a real band splitter may leave out the tuner's products with the zero part (include/fmd.h,
fmd_split_create_real): tests/split_real_spec.py's `ShortcutSpec` -- one multiply per part --
equals the definition, `SplitSpec.push` on (v, +0) pairs, in every output bit (NaN for NaN), over inputs that hold
zeros of both signs, all-zero blocks, and non-finite, denormal and overflowing samples.  And `plan_bands_real`: where
the stations of a real capture land, in any Nyquist zone.
"""
from importlib import import_module

import numpy as np
import pytest

import split_real_spec as rs
from __graft_entry__ import load_package

# (R, K, T)
GEOMETRIES = [(2, 2, 64), (3, 24, 7), (4, 32, 96), (8, 64, 192)]
KINDS = ["s16", "f32_signed_zeros", "all_zero", "poison"]


def _input(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "s16":
        v = rng.integers(-32768, 32768, n).astype(np.int16)
        v[rng.random(n) < 0.2] = 0
        v[:2] = (-32768, 32767)
        return v
    x = (rng.standard_normal(n) * 0.3).astype(np.float32)
    if kind == "f32_signed_zeros":
        x[rng.random(n) < 0.2] = np.float32(-0.0)
        x[rng.random(n) < 0.1] = np.float32(0.0)
    elif kind == "all_zero":
        x[:] = 0.0
        x[1::2] = np.float32(-0.0)
    elif kind == "poison":
        bad = np.array([np.inf, -np.inf, np.nan, 1e-41, -3e-39, 3e38, -3e38, -0.0], np.float32)
        at = rng.random(n) < 0.05
        x[at] = bad[rng.integers(0, bad.size, int(at.sum()))]
        x[0] = np.float32(3e38)
    return x


def _same_or_nan(got, want):
    g, w = np.ascontiguousarray(got).view(np.float32), np.ascontiguousarray(want).view(np.float32)
    if g.shape != w.shape:
        return False
    nan = np.isnan(w)
    return bool(np.all(np.isnan(g[nan])) and np.array_equal(g[~nan].view(np.uint32), w[~nan].view(np.uint32)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "R%dK%dT%d" % g)
def test_the_shortcut_has_the_definitions_bits(geom, kind):
    R, K, T = geom
    shifts = [0, 1, -5, T + 3, T // 2]   # (shift 0 and T / 2: tables with exact zeros and both signs of one)
    model = rs.RealSplitSpec(R, shifts, filter_order=K, table_size=T, out_scale=-0.75)
    short = rs.ShortcutSpec(R, shifts, filter_order=K, table_size=T, out_scale=-0.75)
    sizes = [1, 3, K - 1, K, K + 1, 3000]
    v = _input(kind, sum(sizes), 17 * R + KINDS.index(kind))
    at, outputs, nans = 0, 0, 0
    for n in sizes:
        want, got = model.push(v[at:at + n]), short.push(v[at:at + n])
        assert _same_or_nan(got, want), (n, at)
        outputs += want.size
        nans += int(np.isnan(want.view(np.float32)).sum())
        at += n
    assert outputs > 0 and (kind == "poison") == (nans > 0)


def test_the_pairs_are_the_converted_sample_and_plus_zero():
    v = np.array([-128, -1, 0, 1, 127], np.int8)
    p = rs.pairs(v)
    assert np.array_equal(p[:, 0], np.array([-1.0, -2.0 ** -7, 0.0, 2.0 ** -7, 127 / 128.0], np.float32))
    assert np.array_equal(p[:, 1].view(np.uint32), np.zeros(5, np.uint32))   # +0.0, not -0.0
    w = np.array([-32768, 32767], np.int16)
    assert np.array_equal(rs.convert(w), np.array([-1.0, 32767 / 32768.0], np.float32))
    f = np.array([-0.0, np.inf], np.float32)
    assert np.array_equal(rs.convert(f).view(np.uint32), f.view(np.uint32))
    with pytest.raises(TypeError):
        rs.convert(np.zeros(4, np.uint8))


# ---------------------------------------------------------------------------------------------------------------
# plan_bands_real

@pytest.fixture(scope="module")
def split():
    return import_module(load_package().__name__ + ".split")


@pytest.mark.parametrize("fs", [19.2e6, 122.88e6])
def test_stations_of_any_nyquist_zone_land_on_their_signed_offset(split, fs):
    """zone 1 (0 .. fs/2) and zone 3 (fs .. 3 fs/2): f - 0 and f - fs, positive; zone 2 (fs/2 .. fs): f - fs,
    negative -- always un-inverted, f - round(f / fs) fs"""
    d = [0.11 * fs, 0.23 * fs, 0.37 * fs]                        # distances from the zone's lower edge
    rf = [x for x in d] + [fs / 2 + x for x in d] + [fs + x for x in d]
    want = np.array(d + [x - fs / 2 for x in d] + d)
    R, T = 8, 192
    usable = 0.4 * fs / R - 100e3
    shifts, where = split.plan_bands_real(fs, R, T, rf, usable)
    got = np.array([-shifts[b] * fs / T + o for b, o in where])   # band centre + offset inside the band
    assert np.allclose(got, want, rtol=0, atol=1e-3), (got, want)
    assert np.all(got[:3] > 0) and np.all(got[3:6] < 0) and np.all(got[6:] > 0)
    assert np.all(np.abs(got) < fs / 2)
    # the plan is plan_bands' on those offsets
    rf64 = np.asarray(rf, np.float64)
    off = rf64 - np.floor(rf64 / fs + 0.5) * fs
    assert (shifts, where) == split.plan_bands(fs, R, T, off, usable)
    assert all(abs(o) <= usable + 1e-6 for _, o in where)


@pytest.mark.parametrize("fs", [19.2e6, 122.88e6])
def test_a_station_on_its_own_mirror_is_refused(split, fs):
    usable = 0.4 * fs / 8 - 100e3
    for rf in (100e3, fs - 150e3, fs, 2 * fs + 199e3, fs / 2, fs / 2 - 199e3, fs / 2 + 150e3, 1.5 * fs - 10e3):
        with pytest.raises(ValueError, match="mirror"):
            split.plan_bands_real(fs, 8, 192, [0.3 * fs, rf], usable)
    # just outside the guard, and with a smaller guard, it is planned
    split.plan_bands_real(fs, 8, 192, [201e3, fs / 2 - 201e3], usable)
    split.plan_bands_real(fs, 8, 192, [100e3], usable, guard_hz=50e3)
    with pytest.raises(ValueError):
        split.plan_bands_real(0.0, 8, 192, [1e6], usable)
