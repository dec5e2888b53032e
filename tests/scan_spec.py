"""The band scan's definition (include/fmd.h, fmd_scan_*) restated in numpy float64: what the scan tests hold the
device's spectrum, slot powers, floor and candidate lists against.  It reads neither the package nor the reference.

  spectrum   per call S = (n - N) // (N/2) + 1 segments of N samples at a hop of N/2 (the tail is dropped, nothing
             carries over); periodic Hann window rounded to float32 as the host table is;
             P[i] = sum over all K segments of all calls |FFT(w x)|^2 / (K N sum w^2), fft-shifted: bin i at
             (i - N/2) fs / N
  slots      shift k = -floor(T/2) + j, centre f = -k fs / T; bins with |f_bin - f| <= half_width; eligible when
             |f| + half_width <= fs / 2 and the slot holds a bin; neighbours: the slots with |f' - f| <= min_sep
  rule       floor bin = the floor(q (N-1))-th smallest P; slot power = its bins added one after another in bin
             order (double); snr = 10 log10(power / (floor bin x bin count)); candidate: eligible, snr >= threshold,
             power >= every eligible neighbour's and > that of those with a smaller shift; by increasing frequency
"""
import numpy as np

NEAR_THRESHOLD_DB = 1e-6


def window(N):
    """the periodic Hann window as the device holds it: computed in double, rounded to float32"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(np.float32).astype(np.float64)


def segments(n, N):
    """S of a call of n samples (0: the call is refused)"""
    return (n - N) // (N // 2) + 1 if n >= N else 0


def welch(calls, N, fft=None, w=None):
    """calls: the per-call sample arrays (complex) of ONE capture -> P [N] float64, fft-shifted.  fft: the transform
    of a [S, N] complex128 block of windowed segments along its last axis (default numpy's, in double); w: another
    window than the device's (float64 [N])."""
    fft = fft or (lambda a: np.fft.fft(a, axis=-1))
    w = window(N) if w is None else np.asarray(w, np.float64)
    hop = N // 2
    acc, K = np.zeros(N), 0
    for x in calls:
        x = np.asarray(x).reshape(-1).astype(np.complex128)
        S = segments(x.size, N)
        if S <= 0:
            raise ValueError("a call shorter than one segment")
        idx = np.arange(S)[:, None] * hop + np.arange(N)[None, :]
        X = np.asarray(fft(x[idx] * w[None, :])).astype(np.complex128)
        acc += (X.real ** 2 + X.imag ** 2).sum(axis=0)
        K += S
    return np.fft.fftshift(acc / (float(K) * float(N) * float(np.sum(w * w))))


def slot_tables(fs, N, T, half_width=100e3, min_sep=150e3):
    """The raster of T slots on an N-bin spectrum: shifts [T], f (centres, Hz) [T], offset_hz (f as float32) [T],
    formula (|f| + half_width <= fs/2) [T], eligible (formula and at least one bin) [T], blo / bhi (first and last
    bin, blo > bhi: none) [T], count [T], contiguous (the bins of every slot form one run) and nlo / nhi (first and
    last slot within min_sep, the slot itself included) [T]."""
    fs, hw, sep = float(fs), float(half_width), float(min_sep)
    first = -(T // 2)
    shifts = first + np.arange(T)
    f = (-shifts).astype(np.float64) * fs / float(T)
    fb = (np.arange(N, dtype=np.float64) - float(N // 2)) * fs / float(N)
    inside = np.abs(fb[None, :] - f[:, None]) <= hw                # [T, N]
    count = inside.sum(axis=1)
    blo = np.where(count > 0, inside.argmax(axis=1), N)
    bhi = np.where(count > 0, N - 1 - inside[:, ::-1].argmax(axis=1), -1)
    contiguous = bool(np.all((count == 0) | (bhi - blo + 1 == count)))
    formula = np.abs(f) + hw <= fs / 2.0
    near = np.abs(f[None, :] - f[:, None]) <= sep                  # [T, T]
    nlo = near.argmax(axis=1)
    nhi = T - 1 - near[:, ::-1].argmax(axis=1)
    return {"fs": fs, "N": int(N), "T": int(T), "half_width": hw, "min_sep": sep, "shifts": shifts.astype(np.int32),
            "f": f, "offset_hz": f.astype(np.float32), "formula": formula, "eligible": formula & (count > 0),
            "blo": blo.astype(np.int64), "bhi": bhi.astype(np.int64), "count": count.astype(np.int64),
            "contiguous": contiguous, "nlo": nlo.astype(np.int64), "nhi": nhi.astype(np.int64)}


def slot_powers(P, tables):
    """every slot's bins added one after another, in bin order, in double (0.0 for a slot without a bin)"""
    P = np.asarray(P, np.float64)
    blo, count = tables["blo"], tables["count"]
    pw = np.zeros(tables["T"])
    for k in range(int(count.max(initial=0))):
        m = count > k
        pw[m] = pw[m] + P[blo[m] + k]
    return pw


def rule(P, tables, threshold_db=10.0, q=0.2):
    """The floor / slot / candidate rule on ONE spectrum P [N] (the values of a float32 spectrum, held in double).
    Returns floor_db, slot_db [T] (-inf: ineligible), power [T], snr_db [T] (-inf: ineligible), candidates (dicts
    with shift, offset_hz, power_db, snr_db: the last three rounded to float32, by increasing frequency), count,
    near_threshold (the eligible slots j whose snr_db lies within 1e-6 dB of the threshold), ties (the pairs
    (j, m), j < m, of eligible slots within min_sep of each other whose powers are exactly equal) and tie_winners
    (the candidates' slots j that have such an m above them: they won by the smaller shift)."""
    P = np.asarray(P, np.float64)
    N, T = tables["N"], tables["T"]
    assert P.shape == (N,)
    elig, cnt, nlo, nhi = tables["eligible"], tables["count"], tables["nlo"], tables["nhi"]
    thr = float(np.float32(threshold_db))
    fb = float(np.sort(P)[int(np.floor(float(np.float32(q)) * float(N - 1)))])
    pw = slot_powers(P, tables)
    with np.errstate(divide="ignore", invalid="ignore"):
        slot_db = np.where(elig, 10.0 * np.log10(pw), -np.inf)
        snr = np.where(elig, 10.0 * np.log10(pw / (fb * np.maximum(cnt, 1))), -np.inf)
    near = [int(j) for j in range(T) if elig[j] and abs(snr[j] - thr) <= NEAR_THRESHOLD_DB]
    ties, won, cands = [], [], []
    for j in range(T):
        if not elig[j]:
            continue
        ms = [m for m in range(int(nlo[j]), int(nhi[j]) + 1) if m != j and elig[m]]
        ties += [(j, m) for m in ms if m > j and pw[m] == pw[j]]
        if not snr[j] >= thr:
            continue
        if all((pw[j] > pw[m]) if m < j else (pw[j] >= pw[m]) for m in ms):
            cands.append(j)
            if any(m > j and pw[m] == pw[j] for m in ms):
                won.append(j)
    cands.sort(reverse=True)  # slot T-1 has the largest shift, the lowest frequency
    out = [{"slot": int(j), "shift": int(tables["shifts"][j]), "offset_hz": float(tables["offset_hz"][j]),
            "power_db": float(np.float32(10.0 * np.log10(pw[j]))), "snr_db": float(np.float32(snr[j]))}
           for j in cands]
    return {"floor_db": 10.0 * np.log10(fb), "slot_db": slot_db, "power": pw, "snr_db": snr, "candidates": out,
            "count": len(out), "near_threshold": near, "ties": ties, "tie_winners": won}


def comb(N, n, seed, span_db=12.0, peak=0.05):
    """A probe in which every bin has a level of its own: one period is the inverse FFT of N bins with independent
    levels uniform in 0 .. -span_db dB and random phases, scaled to max |x| = peak, tiled to n samples, complex64."""
    rng = np.random.default_rng(seed)
    level = 10.0 ** (-rng.uniform(0.0, span_db, N) / 20.0)
    phase = rng.uniform(0.0, 2.0 * np.pi, N)
    x = np.fft.ifft(level * np.exp(1j * phase))
    x *= peak / np.abs(x).max()
    reps = -(-n // N)
    return np.tile(x, reps)[:n].astype(np.complex64)


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------
NFFTS = (256, 512, 1024, 2048, 4096)
COMB_ROWS = (0, 1, 255, 511)   # the rows of a 512-row comb batch that are compared with welch()
COMB_SEGMENTS, COMB_TAIL = 7, 37

# (fs, N, T, half_width) of the rule tests.  "ties_win" is "ties" with slots of 21.6 bins instead of 21.33: see
# test_scan_spec_cpu.py::test_where_an_exact_tie_can_win
GEOMETRIES = {"ties": (2.4e6, 256, 1024, 100e3), "narrow": (10e6, 256, 100, 15e3), "odd": (2.048e6, 512, 25, 100e3),
              "unaligned": (1.92e6, 2048, 24, 75e3), "full": (2.4e6, 4096, 1024, 100e3),
              "ties_win": (2.4e6, 256, 1024, 101.25e3)}


def comb_seed(N, row):
    return 100003 * (N // 256) + row


def comb_samples(N):
    return (COMB_SEGMENTS - 1) * (N // 2) + N + COMB_TAIL
