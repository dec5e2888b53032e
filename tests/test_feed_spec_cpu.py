"""CPU-only checks of the mono feed's specification (include/fmd.h, FMD_FEED_*; tests/feed_spec.py): the low-pass
design the feed uses has the lengths and the response the contract names, and the specification carried over ragged
calls equals the specification over the whole stream, counts per call included."""
import numpy as np
import pytest

import feed_spec as fs
from __graft_entry__ import load_package

RATE = 48000.0


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def feed_taps(pkg, D, rate=RATE):
    f = np.float32(rate)
    fo = np.float32(f / np.float32(D))
    return pkg.design_lp_kaiser(1.0, 60.0, float(np.float32(0.425) * fo), float(np.float32(0.575) * fo), float(f))


def response_db(h, freqs, rate=RATE):
    w = np.asarray(freqs, np.float64) / rate
    H = np.exp(-2j * np.pi * np.outer(w, np.arange(len(h)))) @ np.asarray(h, np.float64)
    return 20.0 * np.log10(np.maximum(np.abs(H), 1e-300))


@pytest.mark.parametrize("D,T", [(2, 49), (3, 73)])
def test_taps_have_the_contract_length_and_response(pkg, D, T):
    h = feed_taps(pkg, D)
    assert h.dtype == np.float32 and h.size == T
    fo = RATE / D
    stop = response_db(h, np.linspace(0.575 * fo, RATE / 2, 4001))
    band = response_db(h, np.linspace(0.0, 0.425 * fo, 4001))
    print("D", D, "taps", h.size, "stop band max dB", stop.max(), "pass band dB", band.min(), band.max())
    assert stop.max() <= -55.0
    assert band.max() <= 0.05 and band.min() >= -0.05


@pytest.mark.parametrize("D", [4, 5, 6])
def test_other_divisors_are_cut_off_by_the_design_cap(pkg, D):
    """what fmd_batch_set_feed refuses: the design asks for more than its 75 taps, and the capped filter's stop band
    is far from 55 dB"""
    h = feed_taps(pkg, D)
    assert h.size == 75
    fo = RATE / D
    assert response_db(h, np.linspace(0.575 * fo, RATE / 2, 4001)).max() > -40.0


@pytest.mark.parametrize("D", [2, 3])
def test_ragged_calls_equal_the_whole_stream(pkg, D):
    h = feed_taps(pkg, D)
    rng = np.random.default_rng(5 + D)
    sizes = [1, 2, 3, 5, 1, 47, 48, 49, 72, 73, 74, 1, 1, 1, 437, 13, 14, 15, 16, 2, 131]
    audio = rng.standard_normal((3, 2 * sum(sizes))).astype(np.float32)
    whole = fs.outputs(fs.mono(audio), h, D, 0, fs.count(0, sum(sizes), D))
    spec = fs.FeedSpec(h, D, rows=3)
    got, g0 = [], 0
    for A in sizes:
        y = spec.push(audio[:, 2 * g0:2 * (g0 + A)])
        # the count of the call: the multiples of D among its frames
        assert y.shape[1] == len([g for g in range(g0, g0 + A) if g % D == 0]) == fs.count(g0, A, D)
        got.append(y)
        g0 += A
    got = np.concatenate(got, axis=1)
    assert got.shape == whole.shape
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))


def test_the_loop_is_the_scalar_definition(pkg):
    """the vectorised loop of feed_spec.outputs against the definition written out sample by sample"""
    h = feed_taps(pkg, 3)
    x = np.random.default_rng(1).standard_normal(200).astype(np.float32)
    y = fs.outputs(x[None, :], h, 3, 0, fs.count(0, x.size, 3))[0]
    for n in (0, 1, 7, 24, 25, 66):
        acc = np.float32(0.0)
        for k in range(h.size):
            g = 3 * n - k
            acc = np.float32(acc + np.float32(h[k] * (x[g] if g >= 0 else np.float32(0.0))))
        assert acc.view(np.uint32) == y[n].view(np.uint32)


def test_s16_is_the_audio_rule():
    v = np.array([1.0, -1.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, 3.0, -3.0, np.nan, np.inf, -np.inf], np.float32)
    assert fs.s16(v).tolist() == [32767, -32768, 0, 2, 2, 32767, -32768, 0, 32767, -32768]
