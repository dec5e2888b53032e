"""CPU-only checks of tests/chan_model.py, the bit model of the channeliser's kernels, before the device meets it
(tests/test_gpu_chan_shapes.py): its rows pass the accuracy gate of tests/chan_spec.py at every geometry and row count
the GPU tests use; it agrees in bits with the restatements of the two MFMA chains in tests/chan_real_spec.py; its
deliberately faulty variants change bits, in the rows named here; and the shift lists hold what they should."""
import numpy as np
import pytest

import chan_model as cm
import chan_real_spec as crs
import chan_spec as cs

F32 = np.float32
BIG_B = [(255, 100, 800), (256, 128, 1024)] + cm.MANY      # 70 rows a capture; 17 elsewhere
GATE_CASES = ([(g, False) for g in cm.EDGE] + [(g, True) for g in cm.REAL_EDGE]
              + [(g, False) for g in cm.MANY] + [(g, True) for g in cm.MANY])
CASE_ID = lambda c: cm.geom_id(c[0]) + ("-real" if c[1] else "-complex")


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# the accuracy gate

@pytest.mark.parametrize("case", GATE_CASES, ids=CASE_ID)
def test_the_models_rows_are_no_less_accurate_than_the_reference_arithmetic(case):
    """every row of both captures: RMS error at most 1.0 x, maximum error at most 2.0 x the reference's own float32
    arithmetic's (chan_spec.gate).  (8, 3, 2) reaches exactly 1.00: every operation there is exact.  The worst ratios
    per geometry are in docs/MEASUREMENTS.md, "Channeliser bit model"."""
    geom, real = case
    N, D, K = geom
    B = 70 if geom in BIG_B else 17
    x, sh, rows, floor = cm.case(geom, 2, B, real)
    assert rows.shape[:2] == (2, B) and rows.shape[2] >= 200 and rows.dtype == np.complex64
    # (16, 2, 4096): the stream is a tenth of the filter's length, only the taps' thin end meets a sample
    assert np.isfinite(rows.view(F32)).all() and np.abs(rows).max() > (1e-4 if K > cm.stream_samples(D) else 0.01)
    assert cm.normal(floor), "a product or sum of the model was a subnormal: %g" % floor
    truth, ref = (crs.truth, crs.reference_rows) if real else (cs.truth, cs.reference_rows)
    worst = [0.0, 0.0]
    for g in range(2):
        tr = truth(x[g], N, D, sh[g], filter_order=K)
        rf = ref(x[g], N, D, sh[g], filter_order=K)
        r_rms, r_max = cs.gate(rows[g], rf, tr, "model %s capture %d" % (CASE_ID(case), g))
        worst = [max(worst[0], r_rms.max()), max(worst[1], r_max.max())]
    print("chan model %s 2x%d: error / reference's error, worst row: rms %.2f max %.2f; smallest magnitude %.3g"
          % (CASE_ID(case), B, worst[0], worst[1], floor))


# ---------------------------------------------------------------------------------------------------------------
# agreement with chan_real_spec's chains

@pytest.mark.parametrize("geom", [(2, 2, 5), (3, 2, 7), (6, 2, 7), (7, 3, 10), (8, 3, 5), (24, 11, 88)], ids=cm.geom_id)
def test_the_model_is_the_two_restated_chains_on_its_own_branch_sums(geom):
    """(v, +0) input: the real model's rows are chain_real's bits, the complex model's are chain_complex's, both on the
    model's own branch sums; and the two models' rows are the same but for the signs of zeros (the merged twin tests'
    statement about the device)"""
    N, D, K = geom
    v = cm.capture(0, cm.stream_samples(D), 3, real=True)
    sh = cm.shift_list(N, 0, 7)
    real = cm.run(v, N, D, K, sh, real=True)
    cplx = cm.run(crs.pairs(v), N, D, K, sh, real=False)
    assert real.U.shape == (1, real.rows.shape[1], N) and cplx.U.shape == (2,) + real.U.shape[1:]
    assert _bits_equal(cplx.U[0], real.U[0]) and not cplx.U[1].any() and not np.signbit(cplx.U[1]).any()
    for b, s in enumerate(sh):
        wre, wim = cm.twiddles(N, s)
        W = (wre.astype(np.complex64) + 1j * wim.astype(np.complex64)).astype(np.complex64)
        for got, chain in ((real, crs.chain_real), (cplx, crs.chain_complex)):
            re, im = chain(W, real.U[0])
            assert _bits_equal(np.ascontiguousarray(got.rows[b].real), re), (b, chain.__name__)
            assert _bits_equal(np.ascontiguousarray(got.rows[b].imag), im), (b, chain.__name__)
    assert crs.same_but_zero_signs(real.rows.view(F32), cplx.rows.view(F32))
    assert cm.first_difference(real.rows[0], cplx.rows[0], zero_signs=True) is None
    assert cm.normal(min(real.floor, cplx.floor))


def test_the_twiddles_are_the_hosts():
    """the angle reduced in integers, any shift taken mod N, cos and sin rounded once from double"""
    for N in (2, 3, 24, 255, 256, 511):
        for s in (0, 1, -1, N // 2, N + 5, -3 * N - 2):
            wre, wim = cm.twiddles(N, s)
            k = ((s % N) * np.arange(N)) % N
            assert wre.dtype == F32 and wre.shape == (N,)
            assert np.abs(wre - np.cos(2 * np.pi * k / N)).max() < 6e-8 and np.abs(wim - np.sin(2 * np.pi * k / N)).max() < 6e-8
            assert _bits_equal(wre, cm.twiddles(N, s + 7 * N)[0]) and _bits_equal(wim, cm.twiddles(N, s - N)[1])
            assert wre[0] == 1 and wim[0] == 0 and not np.signbit(wim[0])


# ---------------------------------------------------------------------------------------------------------------
# teeth: each fault fails the equality the GPU tests use (chan_model.row_faults)

def _faulty(geom, B, wrong, real=False, g=1):
    """(faulty rows, right rows) [1, B, outputs] of capture g of the 2 x B shape"""
    N, D, K = geom
    x, sh, rows, _ = cm.case(geom, 2, B, real)
    bad = cm.run(x[g], N, D, K, sh[g], real=real, wrong=wrong).rows
    return bad[None], rows[g][None], sh[g]


def _failing_rows(bad, good, zero_signs=False):
    return [b for b in range(good.shape[1]) if cm.first_difference(bad[0, b], good[0, b], zero_signs) is not None]


@pytest.mark.parametrize("geom,real", [((2, 2, 5), False), ((3, 2, 7), False), ((8, 3, 2), False), ((2, 2, 5), True),
                                       ((3, 2, 7), True)], ids=lambda v: cm.geom_id(v) if isinstance(v, tuple) else str(v))
def test_teeth_a_dropped_tap_k_changes_every_row_where_k_is_small(geom, real):
    """The table's last tap is the thin end of the window: c[K] is 2e-9 .. 2e-8 at K = 2 .. 7.  There it is above half
    an ulp of a branch sum often enough: every row of both captures fails."""
    for g in (0, 1):
        bad, good, _ = _faulty(geom, 17, "drop_tap_k", real, g)
        assert _failing_rows(bad, good, zero_signs=real) == list(range(17)), g
        assert len(cm.row_faults(bad, good, "drop_tap_k", zero_signs=real)) == 17


def test_a_dropped_tap_k_is_below_rounding_at_k_88():
    """c[88] = -8.8e-11 at (24, 11, 88): the tap's product is under half an ulp of its branch sum nearly everywhere (one
    part of one row in 17 x 201 outputs changes in the complex form, none in the real one).  Equality of bits cannot
    see that fault at the broadcast geometries; the geometries with K of 2 .. 11 are in the GPU tests for it."""
    for real in (False, True):
        bad, good, _ = _faulty((24, 11, 88), 17, "drop_tap_k", real)
        assert len(_failing_rows(bad, good, zero_signs=real)) <= 1
    assert abs(float(cs.taps(88, 0.6 / 11)[88])) < 1e-10 < 1e-9 < abs(float(cs.taps(5, 0.3)[5]))


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_teeth_a_branch_walk_that_ignores_q_mod_n_changes_every_row_but_not_output_0(real):
    bad, good, _ = _faulty((24, 11, 88), 17, "ignore_qm", real)
    assert _failing_rows(bad, good, zero_signs=real) == list(range(17))
    # q = 0 and q = 264 = 11 x 24 have q mod N = 0: outputs 0 and 24 are right, output 1 is the first wrong one
    assert all(cm.first_difference(bad[0, b], good[0, b]) == 1 for b in range(17))
    assert _bits_equal(bad[0, :, 24], good[0, :, 24])


@pytest.mark.parametrize("geom,real", [((9, 4, 32), False), ((255, 100, 800), False), ((5, 3, 11), True),
                                       ((511, 230, 1840), True)], ids=lambda v: cm.geom_id(v) if isinstance(v, tuple) else str(v))
def test_teeth_halves_split_at_n_plus_1_over_2_change_every_row_of_an_odd_n(geom, real):
    bad, good, sh = _faulty(geom, 17, "split_up", real)
    failing = _failing_rows(bad, good, zero_signs=real)
    # (a row whose twiddles are all +-1 or 0 can add up the same either way at small N; every other row fails)
    assert len(failing) >= 15 and set(range(17)) - set(failing) <= {b for b in range(17) if sh[b] % geom[0] == 0}, failing


def test_teeth_the_split_fault_is_invisible_at_even_n():
    """why odd N is among the GPU shapes: at an even N both splits are the same chains"""
    for real in (False, True):
        bad, good, _ = _faulty((24, 11, 88), 17, "split_up", real)
        assert _failing_rows(bad, good) == []


def test_teeth_twiddles_in_row_b_xor_1_fail_every_row_whose_neighbour_has_another_shift():
    N = 24
    bad, good, sh = _faulty((N, 11, 88), 17, "row_xor_1")
    want = [b for b in range(17) if b == 16 or sh[b] % N != sh[b ^ 1] % N]
    assert _failing_rows(bad, good) == want and len(want) == 17
    assert not bad[0, 16].any()                               # row 16's neighbour 17 is an empty slot: zeros
    faults = cm.row_faults(bad, good, "row_xor_1")
    # (row 16 repeats row 1's shift; output 0 has no sample in its window yet and is zero in every row)
    assert "IS the model's row of (capture, row) [(0, 1), (0, 16)]" in faults[0]
    assert "capture 0 row 0 differs from the model first at output 1 " in faults[0] and "no other row" in faults[16]


def test_teeth_block_0s_table_in_every_block_fails_rows_16_up_and_leaves_rows_0_to_15_alone():
    """the fault no test with at most 16 rows a capture can see"""
    N = 24
    for B in (33, 70):
        bad, good, sh = _faulty((N, 11, 88), B, "block_0")
        want = [b for b in range(16, B) if sh[b] % N != sh[b % 16] % N]
        assert _failing_rows(bad, good) == want and len(want) >= B - 16 - 3 and min(want) == 16
        assert _bits_equal(bad[0, :16], good[0, :16])
    x = cm.capture(0, cm.stream_samples(11), 0)
    five = cm.anchor_shifts(N)[0]
    assert _bits_equal(cm.run(x, N, 11, 88, five, wrong="block_0").rows, cm.rows(x, N, 11, 88, five))
    faults = cm.row_faults(bad, good, "block_0")
    assert "IS the model's row of (capture, row)" in faults[0] and "(0, 0)" in faults[0]


def test_the_comparison_tells_a_wrong_sample_from_a_wrong_row():
    _, _, rows, _ = cm.case((24, 11, 88), 2, 17)
    got = rows.copy()
    assert cm.row_faults(got, rows, "x") == []
    got[1, 8, 130] = np.nextafter(got[1, 8, 130].real, F32(9)) + 1j * got[1, 8, 130].imag
    got[0, 3] = rows[1, 4]
    faults = cm.row_faults(got, rows, "N24 2x17")
    assert len(faults) == 2
    assert faults[0].startswith("N24 2x17: capture 0 row 3 differs from the model first at output 1 ")
    assert "IS the model's row of (capture, row) [(1, 4)]" in faults[0]
    assert "capture 1 row 8 differs from the model first at output 130" in faults[1] and "no other row" in faults[1]
    with pytest.raises(AssertionError, match="2 of 34 rows differ"):
        cm.assert_rows(got, rows, "N24 2x17")
    # zeros: a sign is a difference unless asked otherwise; int16 rows compare as they are
    z = np.zeros((1, 1, 4), np.complex64)
    nz = (-z.view(F32)).view(np.complex64)
    assert len(cm.row_faults(nz, z, "z")) == 1 and cm.row_faults(nz, z, "z", zero_signs=True) == []
    s = cm.rows_s16(rows)
    t = s.copy()
    t[1, 16, 7, 1] ^= 1
    assert s.shape == rows.shape + (2,) and "capture 1 row 16 differs from the model first at output 7" in cm.row_faults(t, s, "s")[0]


# ---------------------------------------------------------------------------------------------------------------
# the shift lists of the GPU tests

@pytest.mark.parametrize("N,B", [(24, 16), (24, 17), (24, 33), (24, 37), (24, 70), (192, 16), (192, 70), (2, 17), (3, 17),
                                 (9, 17), (16, 17), (255, 17), (256, 17), (511, 17)])
def test_the_shift_lists_hold_every_residue_negatives_values_beyond_n_and_one_duplicate(N, B):
    sh = cm.shifts(N, 2, B)
    assert sh.shape == (2, B) and sh.dtype == np.int32
    for g in range(2):
        res = sh[g].astype(np.int64) % N
        if B >= N:
            assert set(res.tolist()) == set(range(N))
        assert (sh[g] < 0).any() and (sh[g] >= N).any() and (np.abs(sh[g]) > N).any()
        assert sh[g, B - 1] == sh[g, 1]
        if B <= N + 1:                                        # (beyond N + 1 rows residues repeat of need)
            assert len(set(res.tolist())) == B - 1
        if B > 16:
            assert (B - 1) // 16 != 1 // 16                   # the pair lies in two row blocks
    assert not np.array_equal(sh[0], sh[1])
    rot = np.roll(sh, 19, axis=1)                             # the rotation of the set_shifts test: rows change block
    if B == 37:
        assert all((b // 16) != (((b + 19) % B) // 16) for b in (0, 10, 20)) and not np.array_equal(rot % N, sh % N)


def test_the_call_sizes_end_at_the_stream_and_meet_the_tile_edges():
    for N, D, K in cm.EDGE + cm.REAL_EDGE + cm.MANY:
        sizes = cm.call_sizes(D, K)
        assert sum(sizes) == cm.stream_samples(D) and min(sizes) >= 1 and sizes[0] == 1
        if 98 * D + K + 1 < cm.stream_samples(D):
            assert sizes[:7] == [1, D - 1, D + 1, K, 32 * D - 1, 32 * D, 32 * D + 1] and len(sizes) == 8
