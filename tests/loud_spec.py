"""The loudness meter's definition (include/fmd.h, "ITU-R BS.1770 loudness blocks") restated in numpy.

design(fs): the ten coefficients in float64 (b0 b1 b2 a1 a2 of the high shelf, then of the high-pass).  Meter: the
two biquads per channel in transposed direct form II, every multiply, add and subtract rounded on its own, the block
sums and sample peaks, over any number of rows at once -- frame by frame, so a row costs nothing and a frame about
forty numpy operations.  dtype float32 is the definition the device computes bit for bit; float64 is its twin, for
the accuracy of the definition itself.  `variant` builds the three forms the definition is NOT (the tests show that
each is told apart): "fma" (the products are not rounded before the sums), "df1" (direct form I) and "sum64" (block
sums kept in float64).  loudness / integrated restate the host arithmetic in float64."""
import numpy as np

BS1770_48K = np.array([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                       1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])
LOUD_BLOCK_DTYPE = np.dtype([("z_l", "<f4"), ("z_r", "<f4"), ("peak_l", "<f4"), ("peak_r", "<f4")])


def design(fs):
    out = np.zeros(10, np.float64)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    out[0:5] = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
                2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    out[5:10] = (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    return out


def default_block_frames(fs):
    return int(np.floor(fs / 10.0 + 0.5))


class Meter:
    def __init__(self, fs, rows, block_frames=0, dtype=np.float32, variant=None):
        self.t = np.dtype(dtype).type
        self.coef = design(fs).astype(np.float32).astype(dtype)  # rounded once to float, whatever runs on them
        self.bf = int(block_frames) if block_frames else default_block_frames(fs)
        self.variant = variant
        self.zt = np.float64 if variant == "sum64" else dtype
        # L and R go through everything side by side: the last axis is the audio channel
        self.s = np.zeros((2, 2, rows, 2), dtype)  # [stage][s1, s2]
        self.h = np.zeros((2, 4, rows, 2), dtype)  # direct form I only: [stage][x1, x2, y1, y2]
        self.z = np.zeros((rows, 2), self.zt)
        self.peak = np.zeros((rows, 2), dtype)
        self.g = 0
        self.rows = rows
        self.last64 = []

    def _biquad(self, st, x):
        b0, b1, b2, a1, a2 = self.coef[5 * st:5 * st + 5]
        if self.variant == "df1":
            h = self.h[st]
            y = (b0 * x + b1 * h[0]) + b2 * h[1]
            y = (y - a1 * h[2]) - a2 * h[3]
            h[1], h[3] = h[0], h[2]
            h[0], h[2] = x, y
            return y
        s = self.s[st]
        if self.variant == "fma":  # a product that feeds a sum is not rounded (float32 pairs multiply exactly in float64)
            w, t = np.float64, self.t
            y = (w(b0) * x.astype(w) + s[0].astype(w)).astype(t)
            s1 = (w(b1) * x.astype(w) - (a1 * y).astype(w)).astype(t) + s[1]
            s2 = (w(b2) * x.astype(w) - (a2 * y).astype(w)).astype(t)
        else:
            y = b0 * x + s[0]
            s1 = (b1 * x - a1 * y) + s[1]
            s2 = b2 * x - a2 * y
        s[0], s[1] = s1, s2
        return y

    def push(self, audio):
        """audio: [rows, 2 A] interleaved L, R (what a call delivers as float).  Returns the blocks the call completes:
        a structured array [blocks, rows]; self.last64 holds the same blocks' sums unrounded ([rows, 2] each)."""
        a = np.ascontiguousarray(audio).astype(self.t, copy=False)
        assert a.shape[0] == self.rows and a.shape[1] % 2 == 0
        a = a.reshape(self.rows, -1, 2)
        done, self.last64 = [], []
        with np.errstate(all="ignore"):
            for i in range(a.shape[1]):
                x = a[:, i, :]
                y2 = self._biquad(1, self._biquad(0, x))
                self.z = self.z + (y2 * y2).astype(self.zt)
                self.peak = np.fmax(self.peak, np.abs(x))
                self.g += 1
                if self.g % self.bf == 0:
                    rec = np.zeros(self.rows, LOUD_BLOCK_DTYPE)
                    rec["z_l"], rec["z_r"] = self.z[:, 0].astype(np.float32), self.z[:, 1].astype(np.float32)
                    rec["peak_l"], rec["peak_r"] = self.peak[:, 0].astype(np.float32), self.peak[:, 1].astype(np.float32)
                    done.append(rec)
                    self.last64.append(self.z.astype(np.float64))
                    self.z = np.zeros_like(self.z)
                    self.peak = np.zeros_like(self.peak)
        if not done:
            return np.zeros((0, self.rows), LOUD_BLOCK_DTYPE)
        return np.stack(done)


def bits(blocks):
    """[..., 4] uint32: the records' bits"""
    a = np.ascontiguousarray(blocks, dtype=LOUD_BLOCK_DTYPE)
    return a.view(np.uint32).reshape(a.shape + (4,))


def loudness(z_sum, frames):
    """-0.691 + 10 log10(z_sum / frames) in float64 (z_sum: both channels' sums added)"""
    with np.errstate(all="ignore"):
        return -0.691 + 10.0 * np.log10(np.float64(z_sum) / np.float64(frames))


def window(blocks, block_frames):
    """fmd_loudness_window restated: the sums in block order, z_l then z_r of each"""
    s = np.float64(0.0)
    for r in blocks:
        s = s + np.float64(r["z_l"])
        s = s + np.float64(r["z_r"])
    return loudness(s, len(blocks) * block_frames)


def integrated(blocks, block_frames):
    """fmd_loudness_integrated restated: windows of four blocks stepping by one; a window's power is the sum over its
    blocks in order of (z_l + z_r), over 4 Bf; the gates' means run over the surviving windows in order."""
    n = len(blocks)
    if n < 4:
        return -np.inf
    p = []
    for w in range(n - 3):
        s = np.float64(0.0)
        for r in blocks[w:w + 4]:
            s = s + (np.float64(r["z_l"]) + np.float64(r["z_r"]))
        p.append(s / (4.0 * np.float64(block_frames)))
    gate = 10.0 ** ((-70.0 + 0.691) / 10.0)
    s1 = [v for v in p if v > gate]
    if not s1:
        return -np.inf
    m = np.float64(0.0)
    for v in s1:
        m = m + v
    rel = (m / np.float64(len(s1))) * 10.0 ** (-10.0 / 10.0)
    s2 = [v for v in s1 if v > rel]
    if not s2:
        return -np.inf
    m = np.float64(0.0)
    for v in s2:
        m = m + v
    return -0.691 + 10.0 * np.log10(m / np.float64(len(s2)))
