"""The band splitter's definition (include/fmd.h, fmd_split_*) restated in numpy float32: what every splitter test
holds the device's rows against, sample for sample, with no tolerance.

  q counts a capture's input samples since create / reset; x[q] = 0 for q < 0
  t[q] = x[q] * lut[q mod T]        re = a.re*b.re - a.im*b.im, im = a.re*b.im + a.im*b.re, every operation rounded
  y    = sum_{j = 1 .. K} t[q - j] * c[j]   for every q that is a multiple of R: real and imaginary sums apart, from
                                    0.0f, j ascending, a multiply then an add per tap, each rounded
  out  = y * out_scale              (each part)
  a call of n samples behind q0 delivers the q with q0 <= q < q0 + n

c = the Lanczos table of order K (entries 1 .. K) and lut = the tuner table of (T, shift), both from the CPU oracle's
design functions.  `SplitSpec` carries the raw history (the last K input samples) and q from call to call; the tuner
is applied to the carried samples again in every call, so `set_shifts` needs nothing else.
"""
import numpy as np

from oracle import oracle_py

F32 = np.float32


def defaults(decimation, filter_order=0, cutoff=0.0, table_size=0, out_scale=0.0):
    """fmd_split_params' zero-means-default rules"""
    R = int(decimation)
    return (int(filter_order) or 8 * R, float(cutoff) or 0.6 / R, int(table_size) or 64,
            F32(out_scale) if out_scale else F32(0.5))


def count(q0, n, R):
    """outputs of a call of n samples behind q0 samples: the multiples of R in [q0, q0 + n)"""
    return -((-(q0 + n)) // R) - (-((-q0) // R))


def to_f32_pairs(x):
    """a capture block as float32 [n, 2] (complex64, or interleaved float32)"""
    x = np.ascontiguousarray(x)
    if x.dtype == np.complex64:
        x = x.view(F32)
    return np.asarray(x, F32).reshape(-1, 2)


class SplitSpec:
    """The rows of ONE capture: one row per entry of `shifts`.  forget_history / forget_phase: deliberately wrong
    models (the history is dropped / every call starts at phase 0), for the tests that show the comparison has
    teeth."""

    def __init__(self, decimation, shifts, filter_order=0, cutoff=0.0, table_size=0, out_scale=0.0,
                 forget_history=False, forget_phase=False):
        self.R = int(decimation)
        self.K, self.cutoff, self.T, self.scale = defaults(decimation, filter_order, cutoff, table_size, out_scale)
        self.c = oracle_py.design_lanczos(self.K, self.cutoff)[:self.K + 1].astype(F32)
        self.forget_history, self.forget_phase = forget_history, forget_phase
        self.set_shifts(shifts)
        self.reset()

    def reset(self):
        self.q = 0
        self.hist = np.zeros((self.K, 2), F32)

    def set_shifts(self, shifts):
        self.shifts = [int(s) for s in np.atleast_1d(shifts)]
        self.luts = [oracle_py.design_tuner_lut(self.T, s).reshape(self.T, 2).astype(F32) for s in self.shifts]

    def taps(self):
        return self.c[1:].copy()

    def push(self, x):
        """a call's input block -> [rows, n_out] complex64"""
        x = to_f32_pairs(x)
        n, K, R, T = x.shape[0], self.K, self.R, self.T
        q0 = 0 if self.forget_phase else self.q
        w = np.concatenate([self.hist, x])                    # w[i] = x[q0 - K + i]
        qs = np.arange(-((-q0) // R) * R, q0 + n, R, dtype=np.int64)  # the call's output positions
        at = qs - q0 + K                                      # index of x[q] in w
        li = (np.arange(q0 - K, q0 + n, dtype=np.int64)) % T  # q mod T of every window sample
        out = np.zeros((len(self.luts), qs.size), np.complex64)
        with np.errstate(all="ignore"):
            for r, lut in enumerate(self.luts):
                b = lut[li]
                tre = ((w[:, 0] * b[:, 0]).astype(F32) - (w[:, 1] * b[:, 1]).astype(F32)).astype(F32)
                tim = ((w[:, 0] * b[:, 1]).astype(F32) + (w[:, 1] * b[:, 0]).astype(F32)).astype(F32)
                are = np.zeros(qs.size, F32)
                aim = np.zeros(qs.size, F32)
                for j in range(1, K + 1):
                    are = (are + (tre[at - j] * self.c[j]).astype(F32)).astype(F32)
                    aim = (aim + (tim[at - j] * self.c[j]).astype(F32)).astype(F32)
                o = out[r].view(F32).reshape(-1, 2)
                o[:, 0] = (are * self.scale).astype(F32)
                o[:, 1] = (aim * self.scale).astype(F32)
        self.q += n
        self.hist = np.zeros((K, 2), F32) if self.forget_history else w[-K:].copy()
        return out
