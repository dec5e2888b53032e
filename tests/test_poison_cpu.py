"""Non-finite, overflowing and denormal IQ on the CPU oracle alone: the comparison rule has teeth, the capture layout
of tests/poison.py is not vacuous, a reset leaves what the GPU tests rely on, and the edit model (tests/edit_model.py)
says which edits revive a poisoned slot.  Reference: cFmDecoder::Reset (FmDecode.cpp) leaves the resampler's and the
RDS chain's state behind; oracle/fmd_oracle.c follows it."""
import numpy as np
import pytest

import poison as P


@pytest.fixture(scope="module")
def ref(oracle, fmsig):
    return P.reference(oracle, fmsig)


def _flip_nan_signs(a):
    a = np.array(a, copy=True)
    u = a.view(np.uint32)
    u[np.isnan(a)] ^= np.uint32(0x80000000)
    return a


def test_comparator_teeth(ref):
    """Six forgeries made of the oracle's own outputs are all rejected; the unforged copy with every NaN's sign bit
    flipped is accepted."""
    g = 0  # +Inf in I at sample 30000 of call 1
    audio = ref[g][1]["audio"]
    k, on = P.audio_onset([audio])
    assert on >= 2 and on + 2 <= audio.size and np.isnan(audio[on:]).all()
    assert P.same_class(audio.copy(), audio)
    assert P.same_class(_flip_nan_signs(audio), audio) and not np.array_equal(
        _flip_nan_signs(audio).view(np.uint32), audio.view(np.uint32))

    early = audio.copy()
    early[on - 2:on] = np.nan  # the onset one frame (L, R) earlier
    late = audio.copy()
    late[on:on + 2] = audio[on - 2:on]  # one frame later
    ulp = audio.copy()
    ulp.view(np.uint32)[on - 1] += 1  # the clean neighbour off by one ulp
    zeroed = audio.copy()
    zeroed[on + 10] = 0.0  # a NaN replaced by 0
    forged = {"early": early, "late": late, "ulp": ulp, "zeroed": zeroed}

    demod = np.concatenate([ref[q][P.LAYOUT[q].call]["taps"]["demod"].view(np.float32) for q in range(0, 16, 2)])
    inf_at = np.flatnonzero(np.isinf(demod))
    assert inf_at.size, "no infinity in the demod taps of the Inf captures"
    neg = demod.copy()
    neg[inf_at[0]] = -neg[inf_at[0]]  # -Inf for +Inf (or the reverse)
    assert P.same_class(_flip_nan_signs(demod), demod)
    assert not P.same_class(neg, demod)

    gd = [q for q, cp in enumerate(P.LAYOUT) if cp.kind == "denormal"][0]
    small = ref[gd][1]["taps"]["demod"].view(np.float32)
    den = np.flatnonzero((np.abs(small) < np.finfo(np.float32).tiny) & (small != 0))
    assert den.size > small.size // 2, "the denormal capture's demod tap is not in the denormal range"
    flushed = small.copy()
    flushed[den[0]] = np.copysign(np.float32(0), small[den[0]])  # a denormal flushed to a zero of its sign
    assert not P.same_class(flushed, small)
    zero_sign = np.zeros(4, np.float32)
    assert not P.same_class(-zero_sign, zero_sign)  # the signs of zeros

    for name, f in forged.items():
        assert not P.same_class(f, audio), name
        assert P.mismatches(f, audio).size in (1, 2), name
    # integers: equal outright; shape and type are part of the comparison
    pcm = np.arange(8, dtype=np.int16)
    assert P.same_class(pcm.copy(), pcm) and not P.same_class(pcm + (np.arange(8) == 3).astype(np.int16), pcm)
    assert not P.same_class(audio[:-2], audio) and not P.same_class(audio.astype(np.float64), audio)


def test_layout_is_not_vacuous(ref):
    """assert_not_vacuous on the oracle's record of every capture; the onset moves with the poison across captures
    0 .. 15 (one baseband row = 11 samples per capture), and the kinds that must stay finite do, while touching the
    values they are there for."""
    P.assert_not_vacuous(ref)
    onsets = [P.audio_onset([r["audio"] for r in ref[g]]) for g in range(16)]
    assert all(k == 1 for k, _ in onsets)
    floats = [f for _, f in onsets]
    assert floats == sorted(floats) and len(set(floats)) >= 4, floats
    rows = [int(np.flatnonzero(~np.isfinite(ref[g][1]["taps"]["baseband"]))[0]) for g in range(16)]
    assert rows == list(range(rows[0], rows[0] + 16)), rows  # one baseband row per capture
    kind = {cp.kind: g for g, cp in enumerate(P.LAYOUT)}
    for name in ("big", "denormal", "fade") + P.DEGENERATE + ("clean",):
        for r in ref[kind[name]]:
            for t in P.STAGES:
                assert np.isfinite(r["taps"][t].view(np.float32)).all(), (name, t)
    # "big" overflows a level, not the signal; "denormal" and "fade" put denormals into the IF filter's output; the
    # fade ends in exact zeros
    assert np.isinf(ref[kind["big"]][3]["status"].if_level)
    tiny = np.finfo(np.float32).tiny
    for name in ("denormal", "fade"):
        d = np.concatenate([r["taps"]["demod"].view(np.float32) for r in ref[kind[name]]])
        assert ((np.abs(d) < tiny) & (d != 0)).sum() > 1000, name
    last = ref[kind["fade"]][3]["taps"]["demod"].view(np.float32)
    assert not last.any()


@pytest.mark.parametrize("g", [0, 1, 7, 20, 27, 32])
def test_reset_leaves_the_decoder_poisoned(oracle, fmsig, ref, g):
    """After reset() in front of the last call the baseband is finite from its first sample, the resamplers and the RDS
    low-pass give a few NaNs and then none, and the RDS PLL, the matched filter, the sync tap and the audio stay
    non-finite for the whole call."""
    rows = P.captures(fmsig)
    rec = P.run_oracle(oracle, rows[g], P.SIZES, resets=(3,))
    for k in range(3):
        assert P.same_class(rec[k]["audio"], ref[g][k]["audio"])
    t, audio = rec[3]["taps"], rec[3]["audio"]
    assert np.isfinite(t["baseband"]).all() and np.isfinite(t["demod"].view(np.float32)).all()
    assert np.isfinite(t["pilot38"]).all()
    for name in ("mono_rs", "stereo_rs", "rds_lpf"):
        bad = np.flatnonzero(~np.isfinite(t[name].view(np.float32)))
        assert 0 < bad.size < t[name].view(np.float32).size // 4, (name, bad.size)
        assert bad[-1] - bad[0] < 2 * bad.size, (name, bad[:4], bad[-4:])  # one stretch at the head of the call
    for name in ("rds_pll", "rds_mf", "rds_sync"):
        assert not np.isfinite(t[name]).any(), name
    assert audio.size and not np.isfinite(audio).any()


def test_edit_model_on_poisoned_streams(oracle, fmsig):
    """A retune and an import of a clean decoder revive a poisoned slot; a reset, a capture switch to a clean capture
    and a whole-batch reset do not; a clean slot switched to a poisoned capture turns NaN there, and a poisoned decoder
    imported over a clean slot stays poisoned."""
    script, streams, model, shifts, cmaps = P.edit_case(oracle, fmsig)
    r = P.EDIT_ROLES
    last = len(script) - 1

    def finite(c, k, b=0):
        return bool(np.isfinite(model.at(k, c, b)["audio"]).all())

    def dead(c, k, b=0):
        return not np.isfinite(model.at(k, c, b)["audio"]).any()

    for c in range(P.EDIT_C):
        assert finite(c, 0), c
        poisoned = c % 4 in (0, 2)
        a1 = model.at(1, c)["audio"]
        assert np.isnan(a1).any() and np.isfinite(a1).any() if poisoned else np.isfinite(a1).all(), c
    for i, c in enumerate(r["reset"]):
        k = 2 if c in (0, 2, 64, 128) else 3
        assert dead(c, k) and dead(c, last), c
        assert np.isfinite(model.at(k, c)["taps"]["baseband"]).all(), c
        lpf = model.at(k, c)["taps"]["rds_lpf"].view(np.float32)
        assert np.isnan(lpf).any() and np.isfinite(lpf[-100:]).all(), c
    for c in r["retune"]:
        k = 2 if c in (8, 68) else 3
        assert all(finite(c, j) for j in range(k, last + 1)), c
    for c in r["to_clean"]:
        assert dead(c, last - 2) and dead(c, last), c
    for c in r["to_poison"]:
        assert finite(c, 2) and dead(c, 4) and dead(c, last), c
        a3 = model.at(3, c)["audio"]
        assert np.isnan(a3).any() and np.isfinite(a3).any(), c
    for c, k in zip(r["import"], (3, 4)):
        assert np.isnan(model.at(k - 1, c)["audio"][-2:]).all() and all(finite(c, j) for j in range(k, last + 1)), c
    for c, k in zip((2, 3), (2, 5)):  # batch 1's slots that took a poisoned decoder
        assert finite(c, k - 1, 1) and dead(c, k, 1) and dead(c, last, 1), c
    for c in (0, 1, 4, 7):  # the rest of batch 1 never saw a poison
        assert all(finite(c, j, 1) for j in range(last + 1)), c
    # the early reset moved those slots' ring origins and nothing else: same audio as their unreset twins up to call 1
    assert P.same_class(model.at(0, 2)["audio"], model.at(0, 10)["audio"])
    assert not P.same_class(model.at(1, 2)["audio"], model.at(1, 10)["audio"])


def test_audio_meter_restatement(oracle, fmsig, ref):
    """poison.audio_meter is the oracle receiver's meter, bit for bit, on a clean station (the receiver itself stays out
    of the poisoned runs: its status casts a float level to int, which the reference leaves undefined for NaN)."""
    rows = P.captures(fmsig)
    rx = oracle.OracleReceiver(P.FS, P.OFFSET, P.D)
    assert rx.demux_read()[0] == -11
    level = np.float32(0)
    for k in range(len(P.SIZES)):
        rx.write_iq(np.ascontiguousarray(P.call_rows(rows[42], k)))
        pkt = rx.demux_read()
        while pkt[0] != 1:
            pkt = rx.demux_read()
        mean, rms, level = P.audio_meter(ref[42][k]["audio"], level)
        assert P.same_class(np.array(rx.audio_level(), np.float32), np.array([mean, rms, level], np.float32)), k
    rx.close()
    nan = P.audio_meter(ref[0][1]["audio"], 0.25)
    assert np.isnan(nan[0]) and np.isnan(nan[1]) and np.isnan(nan[2])
