"""CPU-only checks of the real-sampled channeliser's specification and of the int16 rows (tests/chan_real_spec.py;
include/fmd.h, fmd_chan_create_real and the _fmt entry points): the definition on (v, +0) input; the S16 conversion on
ties, +-4.0, NaN and infinities; a model of the two kernels' fma chains that shows why a real channeliser's rows are
the bits of its complex twin's -- and where the sign of a zero is not --; plan_bins_real."""
from importlib import import_module

import numpy as np
import pytest

import chan_real_spec as crs
import chan_spec as cs
from __graft_entry__ import load_package

F32 = np.float32


@pytest.fixture(scope="module")
def chan():
    return import_module(load_package().__name__ + ".chan")


# ---------------------------------------------------------------------------------------------------------------
# the definition

@pytest.mark.parametrize("geom", [(7, 3, 10), (24, 11, 88), (500, 230, 1840)], ids=lambda g: "N%d_D%d_K%d" % g)
def test_the_definition_on_real_samples_is_the_channelisers_on_v_and_zero(geom):
    """truth of real samples = chan_spec.truth of (v, +0); for a real input the rows of shifts s and -s are complex
    conjugates of each other (the spectrum of a real signal), which the complex definition does not have; and the
    polyphase identity holds for N above 256 too"""
    N, D, K = geom
    rng = np.random.default_rng(N)
    v = (0.3 * rng.standard_normal(max(4000, 12 * D))).astype(F32)
    sh = [1, -1, N // 3, -(N // 3), 0]
    tr = crs.truth(v, N, D, sh, filter_order=K)
    z = np.stack([v, np.zeros_like(v)], axis=1)
    assert np.array_equal(tr, cs.truth(z, N, D, sh, filter_order=K))
    scale = np.abs(tr).max()
    assert scale > 0.01
    assert np.abs(tr[0] - np.conj(tr[1])).max() < 1e-12 * scale and np.abs(tr[2] - np.conj(tr[3])).max() < 1e-12 * scale
    assert np.abs(tr[4].imag).max() < 1e-12 * scale
    bank = cs.Pfb(N, D, sh, filter_order=K)
    got = np.concatenate([bank.push(crs.pairs(v[a:b])) for a, b in ((0, 1), (1, D + 2), (D + 2, v.size))], axis=1)
    assert got.shape == tr.shape and np.abs(got - tr).max() < 1e-9 * scale
    # integer samples: converted as the I part of the matching FMD_IQ_*
    q8 = np.arange(-128, 128).astype(np.int8)
    assert np.array_equal(crs.convert(q8), np.arange(-128, 128, dtype=F32) / F32(128.0))
    q16 = np.array([-32768, -1, 0, 1, 32767], np.int16)
    assert np.array_equal(crs.convert(q16), q16.astype(np.float64) / 32768.0)
    assert not np.signbit(crs.pairs(q16)[..., 1]).any()


# ---------------------------------------------------------------------------------------------------------------
# int16 rows

def test_int16_rows_are_the_rounded_saturated_parts():
    """saturate(round_half_even(x * 8192)) per part, NaN 0, infinities saturate; ties, +-4.0 and the last values
    inside the range"""
    u = 1.0 / 8192.0
    x = np.array([0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u, -2.5 * u, 0.0, -0.0, u, -u, 3.99987793, -4.0, 4.0,
                  4.0 - 0.5 * u, -4.0 - 0.5 * u, 4.0 - 1.5 * u, 1e30, -1e30, np.inf, -np.inf, np.nan, 1e-40], F32)
    want = np.array([0, 2, 2, 0, -2, -2, 0, 0, 1, -1, 32767, -32768, 32767, 32767, -32768, 32766, 32767, -32768,
                     32767, -32768, 0, 0], np.int16)
    rows = np.stack([x, x[::-1]], axis=1).copy().view(np.complex64).reshape(2, -1)  # (re, im) = (x[i], x[-1 - i])
    got = crs.rows_s16(rows)
    assert got.shape == (2, x.size // 2, 2) and got.dtype == np.int16
    assert np.array_equal(got[..., 0].reshape(-1), want)
    assert np.array_equal(got[..., 1].reshape(-1), want[::-1])
    # every integer comes back from its own float, and the half steps around it round to even
    k = np.arange(-32768, 32768)
    assert np.array_equal(crs.rows_s16((k * u).astype(np.complex64))[..., 0], k.astype(np.int16))
    half = crs.rows_s16(((k[:-1] + 0.5) * u).astype(np.complex64))[..., 0].astype(np.int64)
    assert np.array_equal(half, k[:-1] + (k[:-1] & 1))


# ---------------------------------------------------------------------------------------------------------------
# the chains

def test_fma32_rounds_once():
    """against exact rational arithmetic, values chosen so that float64 -> float32 would round twice"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(F32)
    b = rng.standard_normal(4000).astype(F32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 3, 4000)).astype(F32)
    # ties of the float32 grid that the product's low bits break: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24
    a[:4] = b[:4] = F32(1.0 + 2.0 ** -12)
    c[:4] = [0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -23]
    got = crs.fma32(a, b, c)
    for i in list(range(4)) + list(range(4, 4000, 7)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F32(float(exact))           # (double rounding possible: take the neighbours and pick the nearest exactly)
        cands = {float(lo), float(np.nextafter(lo, F32(np.inf))), float(np.nextafter(lo, F32(-np.inf)))}
        best = min(cands, key=lambda t: (abs(Fraction(t) - exact), int(np.float32(t).view(np.uint32)) & 1))
        assert float(got[i]) == best, (i, a[i], b[i], c[i])
    for i in range(4):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert abs(Fraction(float(got[i])) - exact) <= Fraction(2) ** -24
    # signed zeros as the hardware's fma has them
    assert np.signbit(crs.fma32(F32(-1.0), F32(0.0), F32(-0.0))) and not np.signbit(crs.fma32(-1.0, 0.0, 0.0))
    assert np.signbit(crs.fma32(F32(1e-30), F32(-1e-30), F32(0.0)))  # an underflow keeps the product's sign


def _twiddles(N, s):
    r = np.arange(N)
    return np.exp(2j * np.pi * ((s * r) % N) / N).astype(np.complex64)


@pytest.mark.parametrize("N", [2, 3, 6, 7, 8, 24, 25])
def test_deleting_the_zero_terms_and_padding_an_odd_half_keeps_every_nonzero_results_bits(N):
    """blocks of 64 outputs: noise; noise with signed zeros among the branch sums; all zeros of both signs; a block at
    denormal scale, where products underflow.  Every result that is not a zero has the complex chain's bits; results
    that are zeros are zeros in both."""
    rng = np.random.default_rng(N)
    noise = rng.standard_normal((64, N)).astype(F32)
    holes = noise.copy()
    holes[rng.random((64, N)) < 0.4] = 0.0
    holes[rng.random((64, N)) < 0.2] = -0.0
    zeros = np.where(rng.random((64, N)) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    tiny = (noise * F32(1e-38)).astype(F32)
    dust = (noise * F32(1e-44)).astype(F32)
    nonzero = 0
    for s in (0, 1, -1, N // 2, N // 3 + 1):
        W = _twiddles(N, s)
        for U in (noise, holes, zeros, tiny, dust):
            for got, want in zip(crs.chain_real(W, U), crs.chain_complex(W, U)):
                assert crs.same_but_zero_signs(got, want), (N, s)
                nz = got != 0
                assert np.array_equal(got[nz].view(np.uint32), want[nz].view(np.uint32))
                nonzero += int(nz.sum())
    assert nonzero > 1000


def test_the_sign_of_a_zero_output_can_differ_when_a_partial_sum_underflows():
    """the one exception of the contract, shown to arise: N = 2, both halves one branch long.  The product underflows
    to -0; the complex chain then adds (-Wim) * (+0) = -0 and keeps -0, the real chain's padded k adds +0 * +0 and
    gives +0.  (Such W are not twiddles of a channeliser, whose small entries are ~6e-17; with branch sums below
    1e-29 those underflow the same way.)"""
    W = np.array([1e-30 + 0.5j, 1e-30 + 0.5j], np.complex64)
    U = np.array([[-1e-30, -1e-30]], F32)
    (re_r, _), (re_c, _) = crs.chain_real(W, U), crs.chain_complex(W, U)
    assert re_r[0] == 0 and re_c[0] == 0
    assert np.signbit(re_c[0]) and not np.signbit(re_r[0])
    assert crs.same_but_zero_signs(re_r, re_c)
    # and the comparison has teeth
    assert not crs.same_but_zero_signs(np.array([1.0], F32), np.array([np.nextafter(F32(1.0), F32(2.0))], F32))
    assert not crs.same_but_zero_signs(np.array([0.0], F32), np.array([1e-45], F32))
    assert crs.same_but_zero_signs(np.array([np.nan], F32), np.array([np.nan], F32))


# ---------------------------------------------------------------------------------------------------------------
# plan_bins_real

def test_plan_bins_real_folds_zones_and_applies_the_raster(chan):
    fs, N = 4.8e6, 48                      # raster 100 kHz; zone 1: 0 .. 2.4 MHz, zone 2: 2.4 .. 4.8, zone 3: 4.8 .. 7.2
    # an odd zone folds to a positive offset, an even zone to a negative one
    assert chan.plan_bins_real(fs, N, [0.9e6]) == [-9]
    assert chan.plan_bins_real(fs, N, [4.8e6 + 0.9e6]) == [-9]
    assert chan.plan_bins_real(fs, N, [4.8e6 - 1.1e6]) == [11]
    assert chan.plan_bins_real(fs, N, [2 * 4.8e6 - 0.3e6, 4 * 4.8e6 + 2.0e6]) == [3, -20]
    assert chan.plan_bins_real(fs, N, [0.9e6]) == chan.plan_bins(fs, N, [0.9e6])
    # the FM band from one ADC: 51.2 MS/s real, N 512; 87.5 .. 108 MHz lies in zone 4 (76.8 .. 102.4) and zone 5
    got = chan.plan_bins_real(51.2e6, 512, [87.6e6, 100.0e6, 107.9e6])
    assert got == [148, 24, -55]
    for f, s in zip([87.6e6, 100.0e6, 107.9e6], got):
        assert abs((f - round(f / 51.2e6) * 51.2e6) + s * 51.2e6 / 512) < 1.0
    # on its own mirror: within guard_hz of 0 or fs / 2
    for f in (0.1e6, 4.8e6 - 0.1e6, 2.4e6 + 0.1e6, 2.4e6 - 0.15e6, 3 * 4.8e6):
        with pytest.raises(ValueError, match="mirror"):
            chan.plan_bins_real(fs, N, [f])
    assert chan.plan_bins_real(fs, N, [0.1e6], guard_hz=50e3) == [-1]
    # off the raster
    with pytest.raises(ValueError, match="off the raster"):
        chan.plan_bins_real(fs, N, [0.95e6])
    assert chan.plan_bins_real(fs, N, [0.9e6 + 900.0]) == [-9]
    with pytest.raises(ValueError, match="off the raster"):
        chan.plan_bins_real(fs, N, [0.9e6 + 900.0], tolerance_hz=500.0)
    # N 500: 50 MS/s real
    assert chan.plan_bins_real(50e6, 500, [88.0e6, 101.3e6, 74.7e6]) == [120, -13, -247]
    with pytest.raises(ValueError):
        chan.plan_bins_real(0.0, 48, [1e6])
