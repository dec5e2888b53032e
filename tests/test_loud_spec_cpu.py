"""CPU-only checks of the loudness meter's definition (include/fmd.h, "ITU-R BS.1770 loudness blocks") as
tests/loud_spec.py restates it: the design against the table of BS.1770-4, the known answers of the float64 twin, the
accuracy of the float32 definition against that twin, and that the specification tells the three nearest wrong forms
apart.  The gates of fmd_loudness_window / fmd_loudness_integrated are in tests/test_loud_cabi_cpu.py."""
import numpy as np
import pytest

import loud_spec as ls

RATES = (38000.0, 44100.0, 48000.0, 96000.0)
BLOCKS = 12


def test_the_design_at_48_khz_is_the_table_of_bs1770_4():
    d = np.abs(ls.design(48000.0) - ls.BS1770_48K).max()
    print("largest difference from the table: %.3g" % d)
    assert d <= 1e-12


def _sine(fs, f, amp, n):
    return amp * np.sin(2.0 * np.pi * f * np.arange(n) / fs)


def _left_only(rows):
    """[rows, n] float64 signals -> [rows, 2 n] interleaved with a silent right channel"""
    a = np.zeros((rows.shape[0], 2 * rows.shape[1]), np.float64)
    a[:, 0::2] = rows
    return a


def test_known_answers_of_the_float64_twin():
    """a full-scale 997 Hz sine in L alone reads -3.01 LKFS, the same at -20 dB reads -23.01 (EBU Tech 3341 cases 1, 2
    with one channel: a sine's mean square is half its peak's, the K-weighting is 0 dB near 1 kHz)"""
    fs = 48000.0
    x = np.stack([_sine(fs, 997.0, 1.0, 48000), _sine(fs, 997.0, 0.1, 48000)])
    m = ls.Meter(fs, 2, dtype=np.float64)
    blocks = m.push(_left_only(x))
    assert len(blocks) == 10 and m.bf == 4800
    for row, want in ((0, -3.01), (1, -23.01)):
        got = ls.window(blocks[2:, row], m.bf)
        print("row %d: %.4f LKFS" % (row, got))
        assert abs(got - want) <= 0.01


def _signals(fs, n):
    rng = np.random.default_rng(1770)
    walk = np.cumsum(rng.standard_normal(n)) * 0.002
    return np.stack([_sine(fs, 997.0, 1.0, n), _sine(fs, 997.0, 0.1, n), rng.standard_normal(n) * 0.25,
                     rng.standard_normal(n) * 1e-3, _sine(fs, 50.0, 1.0, n), walk])


NAMES = ("997 Hz 0 dB", "997 Hz -20 dB", "noise 0.25", "noise 1e-3", "50 Hz", "random walk")


@pytest.mark.parametrize("fs", RATES)
def test_the_float32_definition_is_within_0_05_lu_of_its_float64_twin(fs):
    """Every block from the third on, six signals.  The gate is half of EBU Tech 3341's +-0.1 LU.  Measured with
    these signals: at most 8.2e-4 LU for the sines and the noise, and for the random walk 0.0024 / 0.0066 / 0.0075 /
    0.043 LU at the four rates -- the walk at 96 kHz uses 85 % of the gate.  How far a walk wanders under the 38 Hz
    high-pass decides its figure (another realisation gave 0.013); this one is numpy.random.default_rng(1770)'s
    PCG64 stream, which numpy keeps stable across versions for standard_normal only by policy, not by promise."""
    bf = ls.default_block_frames(fs)
    x = _left_only(_signals(fs, BLOCKS * bf)).astype(np.float32)  # both meters hear the same float samples
    b32 = ls.Meter(fs, 6, dtype=np.float32).push(x)
    m64 = ls.Meter(fs, 6, dtype=np.float64)
    m64.push(x)
    assert len(b32) == BLOCKS == len(m64.last64)
    worst = np.zeros(6)
    for j in range(2, BLOCKS):
        l32 = ls.loudness(b32[j]["z_l"].astype(np.float64) + b32[j]["z_r"].astype(np.float64), bf)
        l64 = ls.loudness(m64.last64[j].sum(axis=1), bf)
        worst = np.maximum(worst, np.abs(l32 - l64))
    print("fs %g: " % fs + ", ".join("%s %.3g" % (n, w) for n, w in zip(NAMES, worst)))
    assert (worst <= 0.05).all()


@pytest.mark.parametrize("variant", ["fma", "df1", "sum64"])
def test_the_specification_rejects_the_nearest_wrong_forms(variant):
    """fused multiply-add, direct form I and block sums in float64 each give other bits than the definition"""
    fs = 48000.0
    x = _left_only(_signals(fs, 2000)[[0, 2, 5]]).astype(np.float32)
    want = ls.bits(ls.Meter(fs, 3, block_frames=500).push(x))
    got = ls.bits(ls.Meter(fs, 3, block_frames=500, variant=variant).push(x))
    assert want.shape == got.shape == (4, 3, 4)
    differ = (want != got).any(axis=(0, 2))
    print(variant, "rows that differ:", differ)
    assert differ.all()
    # the peaks are no part of any of the three
    assert np.array_equal(want[..., 2:], got[..., 2:])


def test_nan_leaves_the_peak_and_poisons_the_sum():
    x = np.zeros((1, 64), np.float32)
    x[0, 0::2] = 0.5
    x[0, 20] = np.nan
    b = ls.Meter(48000.0, 1, block_frames=16).push(x)
    assert len(b) == 2
    assert np.isnan(b["z_l"][0, 0]) and b["peak_l"][0, 0] == np.float32(0.5) and b["z_r"][0, 0] == 0.0
    assert np.isnan(b["z_l"][1, 0])  # the filter's state carries it on


def test_blocks_do_not_depend_on_how_the_frames_are_cut_into_calls():
    fs = 48000.0
    x = _left_only(_signals(fs, 1500)[[2, 5]]).astype(np.float32)
    whole = ls.Meter(fs, 2, block_frames=97).push(x)
    m, parts = ls.Meter(fs, 2, block_frames=97), []
    for lo, hi in ((0, 1), (1, 97), (97, 98), (98, 700), (700, 1500)):
        parts.append(m.push(x[:, 2 * lo:2 * hi]))
    assert [len(p) for p in parts] == [0, 1, 0, 6, 8]
    assert np.array_equal(ls.bits(whole), ls.bits(np.concatenate(parts)))
