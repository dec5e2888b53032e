"""CPU-only checks of the polyphase channeliser's specification (include/fmd.h, fmd_chan_*; tests/chan_spec.py): the
definition in float64 agrees with the reference's float32 arithmetic (sign and factor 2 of the tuner included); the
polyphase identity equals the definition over ragged calls at every geometry, and each deliberately wrong variant of
it misses by orders of magnitude; the accuracy yardstick -- the reference's own error against the definition -- is
measured, and a float32 model with every product and sum rounded (unfused, the bins as one sequential chain: the worst
plausible kernel form) stays inside the gate the GPU tests apply; plan_bins."""
from importlib import import_module

import numpy as np
import pytest

import chan_spec as cs
from __graft_entry__ import load_package

# (N, D, K): K < N; small; the 2.4 MS/s case; 9.6 MS/s; K not a multiple of N; 20 MS/s at N 200; the largest N
GEOMS = [(8, 3, 5), (16, 5, 9), (24, 11, 88), (96, 44, 352), (128, 50, 500), (200, 88, 704), (256, 117, 936)]
SAMPLES = 8000


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return (0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def _shifts(N):
    return [0, N // 2, -1, 3, -(N // 3)]


@pytest.fixture(scope="module", params=GEOMS, ids=lambda g: "N%d_D%d_K%d" % g)
def case(request):
    """one capture per geometry with truth and the reference's rows, computed once"""
    N, D, K = request.param
    x = _noise(max(SAMPLES, 181 * D), 1000 + N)
    sh = _shifts(N)
    return dict(N=N, D=D, K=K, x=x, sh=sh, truth=cs.truth(x, N, D, sh, filter_order=K),
                ref=cs.reference_rows(x, N, D, sh, filter_order=K))


def test_truth_is_the_reference_arithmetic_in_float64(case):
    """sign, factor 2, tap order and phase of the definition: the reference's float32 rows lie within float32
    rounding of it"""
    tr, ref = case["truth"], case["ref"]
    assert tr.shape == ref.shape and tr.shape[1] >= 180
    scale = np.sqrt(np.mean(np.abs(tr) ** 2))
    rms, mx = cs.errors(ref, tr)
    assert np.all(rms < 2e-6 * scale) and np.all(mx < 2e-5 * scale), (rms / scale, mx / scale)


def test_polyphase_identity_equals_the_definition_over_ragged_calls(case):
    N, D, K, x = case["N"], case["D"], case["K"], case["x"]
    tr = case["truth"]
    scale = np.abs(tr).max()
    sizes = cs.ragged(x.size, [1, D - 1, D, D + 1, K, 32 * D - 1, 32 * D, 32 * D + 1, 777])
    good = cs.Pfb(N, D, case["sh"], filter_order=K)
    wrong = {w: cs.Pfb(N, D, case["sh"], filter_order=K, wrong=w)
             for w in ("no_rotation", "forget_history", "restart_phase")}
    at, outs, bad = 0, [], {w: [] for w in wrong}
    for n in sizes:
        outs.append(good.push(x[at:at + n]))
        for w, p in wrong.items():
            bad[w].append(p.push(x[at:at + n]))
        at += n
    got = np.concatenate(outs, axis=1)
    assert got.shape == tr.shape
    assert np.abs(got - tr).max() <= 1e-12 * scale
    for w in wrong:
        b = np.concatenate(bad[w], axis=1)
        # (restart_phase also delivers another count; compare what both have)
        m = min(b.shape[1], tr.shape[1])
        assert np.abs(b[:, :m] - tr[:, :m]).max() > 1e-3 * scale, w


def test_the_yardstick_and_a_fully_rounded_float32_bank(case, capsys):
    """e_ref per row, and the gate on the worst plausible float32 form of the bank"""
    N, D, K, x = case["N"], case["D"], case["K"], case["x"]
    model = cs.Pfb(N, D, case["sh"], filter_order=K, dtype=np.float32).push(x)
    rms_ref, mx_ref = cs.errors(case["ref"], case["truth"])
    r_rms, r_mx = cs.gate(model, case["ref"], case["truth"], "float32 bank N=%d D=%d K=%d" % (N, D, K))
    with capsys.disabled():
        print("\nchan yardstick N=%d D=%d K=%d: e_ref rms %.3g..%.3g max %.3g..%.3g; rounded bank / e_ref: rms "
              "%.2f..%.2f max %.2f..%.2f" % (N, D, K, rms_ref.min(), rms_ref.max(), mx_ref.min(), mx_ref.max(),
                                             r_rms.min(), r_rms.max(), r_mx.min(), r_mx.max()))


def test_the_gate_refuses_a_row_less_accurate_than_the_reference(case):
    tr, ref = case["truth"], case["ref"]
    worse = (tr + 1.5 * (ref.astype(np.complex128) - tr)).astype(np.complex128)
    with pytest.raises(AssertionError, match="RMS error"):
        cs.gate(worse, ref, tr)


def test_defaults():
    assert cs.defaults(11) == (88, 0.6 / 11, np.float32(1.0))
    assert cs.defaults(11, 40, 0.1, 0.5) == (40, 0.1, np.float32(0.5))


@pytest.fixture(scope="module")
def chan():
    return import_module(load_package().__name__ + ".chan")


def test_plan_bins_gives_the_shift_of_every_station(chan):
    # 9.6 MS/s, 96 bins: the 100 kHz raster; a station at +f sits on bin f / 100 kHz and takes shift -bin
    assert chan.plan_bins(9.6e6, 96, [0.0, 100e3, -100e3, 4.7e6, -4.8e6, 300.4e3]) == [0, -1, 1, -47, 48, -3]
    # 2.4 MS/s, 24 bins, the end-to-end case
    assert chan.plan_bins(2.4e6, 24, [0.8e6, 0.3e6, -0.4e6, -0.9e6]) == [-8, -3, 4, 9]
    # the shift is the one whose tuner centre -shift fs / N is the station
    for f, s in zip([0.8e6, -0.9e6], chan.plan_bins(2.4e6, 24, [0.8e6, -0.9e6])):
        assert -s * 2.4e6 / 24 == pytest.approx(f)


def test_plan_bins_refuses_a_station_off_the_raster_with_a_sentence(chan):
    with pytest.raises(ValueError, match=r"station at 151500 Hz.*off the raster"):
        chan.plan_bins(9.6e6, 96, [100e3, 151.5e3])
    assert chan.plan_bins(9.6e6, 96, [100.9e3]) == [-1]
    with pytest.raises(ValueError, match="outside the capture"):
        chan.plan_bins(2.4e6, 24, [1.3e6])
    with pytest.raises(ValueError, match="n_bins"):
        chan.plan_bins(2.4e6, 1, [0.0])
