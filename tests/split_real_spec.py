"""The real band splitter's definition (include/fmd.h, fmd_split_create_real): a real capture's rows are the rows of
tests/split_spec.py's `SplitSpec` on the complex samples (convert(v), +0.0).  There is no second model: `RealSplitSpec`
only forms the pairs.  `ShortcutSpec` restates what the kernel does instead -- one multiply per part, the products with
the zero part never formed -- for tests/test_split_real_spec_cpu.py to hold against the definition bit for bit.
"""
import numpy as np

import split_spec as ss

F32 = np.float32


def convert(v):
    """a block of real samples as float32: float32 as is, int8 v * 2^-7, int16 v * 2^-15 (both exact)"""
    v = np.ascontiguousarray(v).reshape(-1)
    if v.dtype == np.float32:
        return v
    if v.dtype == np.int8:
        return v.astype(F32) * F32(2.0 ** -7)
    if v.dtype == np.int16:
        return v.astype(F32) * F32(2.0 ** -15)
    raise TypeError("no real-sample format for dtype %s" % v.dtype)


def pairs(v):
    """(convert(v), +0.0) as float32 [n, 2]"""
    x = np.zeros((np.asarray(v).size, 2), F32)
    x[:, 0] = convert(v)
    return x


class RealSplitSpec(ss.SplitSpec):
    """The rows of ONE real capture: SplitSpec.push on (v, +0) pairs."""

    def push(self, v):
        return super().push(pairs(v))


class ShortcutSpec:
    """The kernel's arithmetic: t = (v lut.re, v lut.im), a float of history per sample; taps, scale and count as in
    the definition."""

    def __init__(self, decimation, shifts, filter_order=0, cutoff=0.0, table_size=0, out_scale=0.0):
        m = ss.SplitSpec(decimation, shifts, filter_order, cutoff, table_size, out_scale)
        self.R, self.K, self.T, self.scale, self.c, self.luts = m.R, m.K, m.T, m.scale, m.c, m.luts
        self.q = 0
        self.hist = np.zeros(self.K, F32)

    def push(self, v):
        v = convert(v)
        n, K, R, T = v.size, self.K, self.R, self.T
        q0 = self.q
        w = np.concatenate([self.hist, v])
        qs = np.arange(-((-q0) // R) * R, q0 + n, R, dtype=np.int64)
        at = qs - q0 + K
        li = np.arange(q0 - K, q0 + n, dtype=np.int64) % T
        out = np.zeros((len(self.luts), qs.size), np.complex64)
        with np.errstate(all="ignore"):
            for r, lut in enumerate(self.luts):
                b = lut[li]
                tre = (w * b[:, 0]).astype(F32)
                tim = (w * b[:, 1]).astype(F32)
                are = np.zeros(qs.size, F32)
                aim = np.zeros(qs.size, F32)
                for j in range(1, K + 1):
                    are = (are + (tre[at - j] * self.c[j]).astype(F32)).astype(F32)
                    aim = (aim + (tim[at - j] * self.c[j]).astype(F32)).astype(F32)
                o = out[r].view(F32).reshape(-1, 2)
                o[:, 0] = (are * self.scale).astype(F32)
                o[:, 1] = (aim * self.scale).astype(F32)
        self.q += n
        self.hist = w[-K:].copy()
        return out
