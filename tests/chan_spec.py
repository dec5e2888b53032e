"""The polyphase channeliser's definition (include/fmd.h, fmd_chan_*) in numpy: what the channeliser tests hold the
device's rows against.

  q counts a capture's input samples since create / reset; x[q] = 0 for q < 0; c = the Lanczos table of order K
  y_s[q] = out_scale * sum_{j = 1 .. K} x[q - j] c[j] 2 exp(+2 pi i s ((q - j) mod N) / N)   for q a multiple of D

`truth` is that sum in float64 with the float32 taps and input taken as data.  `reference_rows` is the reference's own
float32 arithmetic (tests/split_spec.py with T = N, R = D: tuner, then the tap sum in order).  `Pfb` restates the
polyphase identity the kernel computes,
  u_q[r] = sum over j with (q - j) = r (mod N) of c[j] x[q - j],    y_s[q] = 2 out_scale sum_r u_q[r] e^{2 pi i s r / N},
in float64 or, as a model of a kernel's rounding, float32 with every product and sum rounded and the bins summed as a
sequential chain; its deliberately wrong variants show that the comparisons have teeth.  The accuracy gate: a row is no
less accurate than the reference's arithmetic -- its RMS error against `truth` at most 1.0 x the reference's on that
row, its maximum error at most 2 x the reference's maximum (the maximum is a noisy statistic).
"""
import numpy as np

from oracle import oracle_py

import split_spec

F32 = np.float32
RMS_FACTOR, MAX_FACTOR = 1.0, 2.0


def defaults(decimation, filter_order=0, cutoff=0.0, out_scale=0.0):
    """fmd_chan_params' zero-means-default rules"""
    D = int(decimation)
    return int(filter_order) or 8 * D, float(cutoff) or 0.6 / D, F32(out_scale) if out_scale else F32(1.0)


def taps(K, cutoff):
    """c[0 .. K] in float32 (c[1 .. K] are the taps)"""
    return oracle_py.design_lanczos(K, cutoff)[:K + 1].astype(F32)


def as_complex128(x):
    return split_spec.to_f32_pairs(x).astype(np.float64).view(np.complex128).reshape(-1)


def truth(x, n_bins, decimation, shifts, filter_order=0, cutoff=0.0, out_scale=0.0):
    """[rows, n_out] complex128: the definition over one capture's whole stream x (from q = 0)."""
    N, D = int(n_bins), int(decimation)
    K, cutoff, scale = defaults(D, filter_order, cutoff, out_scale)
    c = taps(K, cutoff).astype(np.float64)
    x = as_complex128(x)
    qs = np.arange(0, x.size, D)
    n = np.arange(x.size)
    out = np.zeros((len(shifts), qs.size), np.complex128)
    for i, s in enumerate(shifts):
        rot = 2.0 * np.exp(2j * np.pi * ((int(s) * (n % N)) % N) / N)
        t = np.concatenate([np.zeros(K, np.complex128), x * rot])       # t[K + q] = tuned x[q]
        win = np.lib.stride_tricks.sliding_window_view(t, K)[qs]          # win[o][i] = tuned x[q - K + i]
        out[i] = float(scale) * (win @ c[K:0:-1])
    return out


def reference_rows(x, n_bins, decimation, shifts, filter_order=0, cutoff=0.0):
    """[rows, n_out] complex64: the reference's float32 arithmetic (cFineTuner of table size N, cDownsampleFilter)."""
    K, cutoff, _ = defaults(decimation, filter_order, cutoff)
    return split_spec.SplitSpec(decimation, shifts, filter_order=K, cutoff=cutoff, table_size=n_bins,
                                out_scale=1.0).push(x)


class Pfb:
    """The polyphase identity for ONE capture, carried over ragged calls.  dtype float64: the identity itself; float32:
    every product and sum rounded to float32, the branch sums and the bins as sequential chains.
    wrong = "no_rotation" (the branch index ignores q mod N), "forget_history", "restart_phase": deliberately wrong."""

    def __init__(self, n_bins, decimation, shifts, filter_order=0, cutoff=0.0, out_scale=0.0, dtype=np.float64,
                 wrong=None):
        self.N, self.D = int(n_bins), int(decimation)
        self.K, self.cutoff, self.scale = defaults(decimation, filter_order, cutoff, out_scale)
        self.real = np.dtype(dtype)
        self.cplx = np.dtype(np.complex128 if self.real == np.float64 else np.complex64)
        self.c = taps(self.K, self.cutoff).astype(self.real)
        self.wrong = wrong
        self.shifts = [int(s) for s in shifts]
        r = np.arange(self.N)
        self.W = np.stack([np.exp(2j * np.pi * ((s * r) % self.N) / self.N) for s in self.shifts]).astype(self.cplx)
        self.q = 0
        self.hist = np.zeros(self.K, self.cplx)

    def push(self, x):
        N, D, K = self.N, self.D, self.K
        x = as_complex128(x).astype(self.cplx)
        q0 = 0 if self.wrong == "restart_phase" else self.q
        w = np.concatenate([self.hist, x])                       # w[i] = x[q0 - K + i]
        qs = np.arange(-((-q0) // D) * D, q0 + x.size, D, dtype=np.int64)
        j = np.arange(1, K + 1)
        win = w[(qs - q0 + K)[:, None] - j[None, :]]             # win[o][j - 1] = x[q - j]
        res = ((0 if self.wrong == "no_rotation" else qs[:, None]) - j[None, :]) % N
        res = np.broadcast_to(res, win.shape)
        U = np.zeros((qs.size, N), self.cplx)
        if self.real == np.float64:
            V = win * self.c[1:][None, :]
            for r in range(N):
                U[:, r] = (V * (res == r)).sum(axis=1)
            out = (2.0 * float(self.scale)) * (self.W @ U.T)
        else:
            for jj in range(K):                                   # j ascending, a rounded multiply and add per tap
                v = (win[:, jj] * self.c[jj + 1]).astype(self.cplx)
                o = np.arange(qs.size)
                U[o, res[:, jj]] = (U[o, res[:, jj]] + v).astype(self.cplx)
            out = np.zeros((len(self.shifts), qs.size), self.cplx)
            for r in range(N):                                    # the bins: a sequential chain over r
                out = (out + (self.W[:, r][:, None] * U[:, r][None, :]).astype(self.cplx)).astype(self.cplx)
            out = (out * F32(2.0 * float(self.scale))).astype(self.cplx)
        self.q += x.size
        self.hist = np.zeros(K, self.cplx) if self.wrong == "forget_history" else w[-K:].copy()
        return out


def errors(rows, tr):
    """(RMS, maximum) of |rows - tr| per row, in float64"""
    e = np.abs(np.asarray(rows).astype(np.complex128) - tr)
    return np.sqrt(np.mean(e * e, axis=1)), e.max(axis=1)


def gate(rows, ref, tr, what=""):
    """Assert the accuracy gate per row; returns (rms / rms_ref, max / max_ref) per row for the record."""
    rms, mx = errors(rows, tr)
    rms_ref, mx_ref = errors(ref, tr)
    assert tr.shape[1] >= 180, "the gate wants at least 180 outputs per row"
    assert np.all(rms_ref > 0) and np.all(mx_ref > 0)
    for r in range(tr.shape[0]):
        assert rms[r] <= RMS_FACTOR * rms_ref[r], "%s row %d: RMS error %.4g above %g x the reference's %.4g" % (
            what, r, rms[r], RMS_FACTOR, rms_ref[r])
        assert mx[r] <= MAX_FACTOR * mx_ref[r], "%s row %d: maximum error %.4g above %g x the reference's %.4g" % (
            what, r, mx[r], MAX_FACTOR, mx_ref[r])
    return rms / rms_ref, mx / mx_ref


def ragged(total, sizes):
    """call sizes that walk `sizes` in turn and end exactly at total"""
    out, i = [], 0
    while total > 0:
        n = min(int(sizes[i % len(sizes)]), total)
        out.append(n)
        total -= n
        i += 1
    return out
