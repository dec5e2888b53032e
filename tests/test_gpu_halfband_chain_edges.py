"""k_halfband_chain at the ends of its step lists: call sizes picked so that stage 0's input ends in the last, the
second-last and the third-last step of the call's last stretch (where a wave's window of fifteen rows reaches past
the input: the slack rows behind the input buffers), for 1, 2, 3 and 8 stretches; a batch whose last channel group
is ragged; a channel reset in the middle.  Every case against the CPU oracle through the RDS taps and the audio,
bit for bit, like tests/test_gpu_halfband_chain.py.

The sizes are chosen with a copy of the host's planning (hbf_plan, csrc/fmd_batch.hip) that runs without a GPU:
test_plan_of_the_chosen_sizes asserts what each size exercises."""
import numpy as np
import pytest

from __graft_entry__ import load_package

FS, D = 2.4e6, 11
H0, L1H, L2H, RING, NSET, SLACK = 7, 22, 42, 64, 4, 32  # the 15 / 23 / 43-tap chain; HBF_RING, HBF_NSET, HBF_SLACK

# baseband samples per call (the call is 11 times as long: the decimator's phase stays 0) -> stretches, steps of the
# last stretch behind the last one in which stage 0 has outputs
CASES = {364: (1, 0), 449: (1, 1), 417: (1, 2), 541: (2, 0), 505: (2, 1), 669: (2, 2), 813: (3, 0), 761: (3, 1),
         1005: (3, 2), 2173: (8, 0), 2041: (8, 1), 2053: (8, 2)}


def plan(n_in, S):
    """hbf_plan's step lists: per stretch [(a_lo, a_n, b_lo, b_n, c_lo, c_n)]"""
    n0 = (n_in + 1) // 2
    n1 = (n0 + 1) // 2
    n2 = (n1 + 1) // 2
    per = (n2 + S - 1) // S
    out = []
    for a in range(0, n2, per):
        st = []
        e = min(n2, a + per)
        last = e == n2
        need1 = n1 if last else 2 * (e - 1) + 1
        need0 = n0 if last else 2 * (need1 - 1) + 1
        d2, d1 = a, max(0, 2 * a - L2H)
        d0 = max(0, 2 * d1 - L1H)
        while d2 < e or d1 < need1 or d0 < need0:
            a_hi = max(d0, min(d0 + 16, need0, 2 * d1 - L1H + RING))
            b_hi = max(d1, min(d1 + 8, need1, (a_hi - 1) // 2 + 1 if a_hi > 0 else 0, 2 * d2 - L2H + RING))
            c_hi = max(d2, min(d2 + 4, e, (b_hi - 1) // 2 + 1 if b_hi > 0 else 0))
            assert (a_hi, b_hi, c_hi) != (d0, d1, d2)
            st.append((d0, a_hi - d0, d1, b_hi - d1, d2, c_hi - d2))
            d0, d1, d2 = a_hi, b_hi, c_hi
        while len(st) % NSET:
            st.append((d0, 0, d1, 0, d2, 0))
        out.append(st)
    return out


def stretches_of(n_in, groups=1, ncu=256):
    """the library's choice (fmd_batch_process.inc.hpp)"""
    n2 = (((n_in + 1) // 2 + 1) // 2 + 1) // 2
    return max(1, min(8, (2 * ncu + groups // 2) // groups, n2 // 32))


def plan_stats(n_in, S):
    p = plan(n_in, S)
    last_row = 2 * H0 + n_in - 1
    partial = sum(1 for st in p for s in st if 0 < s[1] < 16)   # steps in which some wave's group is not full
    over = [2 * (s[0] + 4 * w) + 2 * (3 + H0) - last_row for st in p for s in st for w in range(4)]
    over = [x for x in over if x > 0]                           # windows that reach past the last input row
    after = len(p[-1]) - 1 - max(i for i, s in enumerate(p[-1]) if s[1] > 0)
    return len(p), partial, len(over), max(over, default=0), after


def test_plan_of_the_chosen_sizes():
    seen = set()
    for n_in, (S, after) in CASES.items():
        got_S, partial, n_over, worst, got_after = plan_stats(n_in, stretches_of(n_in))
        print(n_in, "stretches", got_S, "steps with a partial group", partial, "windows past the input", n_over,
              "by at most", worst, "rows; steps behind stage 0's last", got_after)
        assert (got_S, got_after) == (S, after), n_in
        assert partial >= S and n_over >= 3 and 0 < worst <= SLACK, n_in
        seen.add(worst)
    assert SLACK in seen  # the bound is reached
    # ... and never passed, whatever the call size
    for n_in in range(336, 2400):
        assert plan_stats(n_in, stretches_of(n_in))[3] <= SLACK, n_in
    # the ragged batch below: three channel groups, three stretches
    assert stretches_of(813, groups=3) == 3


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _batch(pkg, C, chain=1):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C)
    b.debug_set("halfband_chain", chain)  # before the first call: starts the oscillator sequence too
    b.debug_set("nomix", 1)
    return b


@pytest.mark.gpu
def test_chain_ends_of_stretches_bit_exact(oracle, fmsig):
    """One decoder, every size of CASES in turn (each call starts from the delay lines the one before left: tail1 /
    tail2 and the history rows), a full-size call in between."""
    pkg = load_package()
    p = fmsig.default_params(FS, noise_sigma=0.01, seed=43)
    o = oracle.OracleDecoder(FS, -0.15 * FS, 48000.0, 15000.0, D)
    b = _batch(pkg, 1)
    b.enable_taps()
    pos = 0
    sizes = [11 * m for m in CASES]
    sizes = sizes[:6] + [65536 // 11 * 11] + sizes[6:]
    for blk, n in enumerate(sizes):
        iq = fmsig.generate_f32(p, pos, n)
        pos += n
        a_ref = o.process_stream(iq)
        a_gpu = b.process_host(iq.view(np.complex64), shared=True)[0]
        taps = o.taps()
        for name in ("rds_lpf", "rds_pll", "rds_mf"):
            g, r = b.tap(name), taps[name]
            assert g.shape == r.shape, (blk, name, g.shape, r.shape)
            assert _bits_equal(g.view(np.float32), r.view(np.float32)), (blk, n, name)
        assert _bits_equal(a_gpu, a_ref), (blk, n)
    b.close()


@pytest.mark.gpu
def test_chain_ragged_group_and_reset_bit_exact(oracle, fmsig):
    """130 channels (the last group of lanes holds two), three stretches; channels 64 and 129 are reset in front of
    the third call and decode like decoders after cFmDecoder::Reset() from there on."""
    pkg = load_package()
    C, n, calls, reset_at, reset = 130, 11 * 813, 5, 2, [64, 129]
    base = [fmsig.default_params(FS, noise_sigma=0.01, seed=500 + k, pi=0x5000 + k, ps="EDGES%03d" % k)
            for k in range(3)]
    b = _batch(pkg, C)
    b.enable_taps(True)
    watch = [0, 1, 2, 63, 64, 128, 129]
    refs = {c: oracle.OracleDecoder(FS, -0.15 * FS, 48000.0, 15000.0, D) for c in watch}
    for blk in range(calls):
        src = [fmsig.generate_f32(q, blk * n, n) for q in base]
        iq = np.stack([src[c % 3] for c in range(C)]).view(np.complex64).reshape(C, n)
        if blk == reset_at:
            b.reset_channels(reset)
            for c in reset:
                refs[c].reset()
        a = b.process_host(iq)
        for c in watch:
            a_ref = refs[c].process_stream(src[c % 3])
            taps = refs[c].taps()
            for name in ("rds_lpf", "rds_pll", "rds_mf"):
                g, r = b.tap(name, c), taps[name]
                assert g.shape == r.shape, (blk, c, name, g.shape, r.shape)
                assert _bits_equal(g.view(np.float32), r.view(np.float32)), (blk, c, name)
            assert _bits_equal(a[c], a_ref), (blk, c)
    b.close()


@pytest.mark.gpu
def test_chain_and_per_stage_on_different_inputs_differ(fmsig):
    """Negative control: the comparison has teeth -- the chain form and the per-stage form fed different inputs do
    not give the same RDS low-pass rows or the same audio."""
    pkg = load_package()
    n = 11 * 813
    out = []
    for chain, seed in ((1, 43), (0, 44)):
        b = _batch(pkg, 1, chain)
        b.enable_taps()
        iq = fmsig.generate_f32(fmsig.default_params(FS, noise_sigma=0.01, seed=seed), 0, n)
        audio = b.process_host(iq.view(np.complex64), shared=True)[0].copy()
        out.append((audio, b.tap("rds_lpf").copy()))
        b.close()
    assert out[0][1].shape == out[1][1].shape
    assert not _bits_equal(out[0][1].view(np.float32), out[1][1].view(np.float32))
    assert not _bits_equal(out[0][0], out[1][0])
