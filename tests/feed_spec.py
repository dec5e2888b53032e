"""The mono feed's definition (include/fmd.h, FMD_FEED_*) restated in numpy float32: what every feed test holds the
device's rows against, sample for sample, with no tolerance.

  x[g] = (L[g] + R[g]) * 0.5f                     for audio frame g of the calls that asked for the feed; 0 for g < 0
  y[n] = sum_{k = 0 .. T - 1} h[k] * x[n D - k]   from acc = 0, k ascending, acc = acc + h[k] * x: two roundings a tap
  a call whose frames are g0 .. g0 + A - 1 delivers the n with g0 <= n D < g0 + A

`FeedSpec` carries the history from call to call the way the definition says (it keeps every frame: tests are short).
"""
import numpy as np

F32 = np.float32


def s16(y):
    """fmd_f32_to_s16: saturate_int16(round_half_even(y * 32768.0f)), NaN gives 0"""
    v = np.asarray(y, F32) * F32(32768.0)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(v), -32768.0, 32767.0)
    return np.where(np.isnan(v), 0, r).astype(np.int16)


def mpx16(x):
    """FMD_MPX_S16 and both parts of FMD_CIQ_S16: saturate_int16(round_half_even(x * 8192.0f)), NaN gives 0"""
    y = np.asarray(x, F32) * F32(8192.0)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(y), -32768.0, 32767.0)
    return np.where(np.isnan(y), 0, r).astype(np.int16)


def mono(audio):
    """x of interleaved L, R float32 rows [..., 2 A] -> [..., A]: (L + R) * 0.5f in float32"""
    a = np.asarray(audio, F32)
    return ((a[..., 0::2] + a[..., 1::2]) * F32(0.5)).astype(F32)


def count(g0, A, D):
    """samples of a call of A frames behind g0 frames"""
    return -((-(g0 + A)) // D) - (-((-g0) // D))


def outputs(x, taps, D, n_first, n_count):
    """y[n_first .. n_first + n_count) over the frames x[..., 0 .. G) (x[g] = 0 for g < 0): a float32 loop over k"""
    x = np.asarray(x, F32)
    h = np.asarray(taps, F32)
    T = h.size
    xp = np.concatenate([np.zeros(x.shape[:-1] + (T - 1,), F32), x], axis=-1)
    at = (T - 1) + D * (n_first + np.arange(n_count, dtype=np.int64))
    acc = np.zeros(x.shape[:-1] + (n_count,), F32)
    for k in range(T):
        acc = (acc + (h[k] * xp[..., at - k]).astype(F32)).astype(F32)
    return acc


class FeedSpec:
    """the feed of [rows] channels, call after call"""

    def __init__(self, taps, D, rows=1):
        self.h = np.asarray(taps, F32).copy()
        self.D = int(D)
        self.x = np.zeros((rows, 0), F32)

    @property
    def g(self):
        return self.x.shape[-1]

    def push(self, audio):
        """a call's interleaved float audio [rows, 2 A] -> its feed samples [rows, n] (float32)"""
        g0 = self.g
        xs = mono(np.asarray(audio, F32).reshape(self.x.shape[0], -1))
        A = xs.shape[-1]
        self.x = np.concatenate([self.x, xs], axis=-1)
        first = -((-g0) // self.D)
        return outputs(self.x, self.h, self.D, first, count(g0, A, self.D))
