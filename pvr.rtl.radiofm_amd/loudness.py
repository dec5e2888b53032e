"""EBU R 128 / ITU-R BS.1770-4 figures from the loudness blocks of a batch (Batch.collect_loudness): momentary,
short-term and integrated loudness in LUFS, through the library's own host arithmetic (fmd_loudness_window,
fmd_loudness_integrated; include/fmd.h).  `blocks` is one channel's records in block order, a one-dimensional array of
LOUD_BLOCK_DTYPE (a column of what collect_loudness returns); block_frames is Batch.loudness_block_frames().  With the
default 100 ms block, four blocks are the 400 ms window of momentary loudness and thirty the 3 s of short-term loudness.
Loudness range and true peak are out of scope."""
import numpy as np

from . import LOUD_BLOCK_DTYPE, lib


def _records(blocks):
    a = np.ascontiguousarray(blocks, dtype=LOUD_BLOCK_DTYPE)
    if a.ndim != 1:
        raise ValueError("one channel's blocks: a one-dimensional array of LOUD_BLOCK_DTYPE")
    return a


def window(blocks, block_frames):
    """-0.691 + 10 log10 of the mean square of both channels over all of `blocks`."""
    a = _records(blocks)
    if a.size == 0:
        raise ValueError("no blocks")
    return float(lib().fmd_loudness_window(a.ctypes.data, a.size, int(block_frames)))


def _sliding(blocks, block_frames, n):
    a = _records(blocks)
    return np.array([window(a[i:i + n], block_frames) for i in range(a.size - n + 1)], dtype=np.float64)


def momentary(blocks, block_frames):
    """float64[len - 3]: the loudness of every window of four consecutive blocks."""
    return _sliding(blocks, block_frames, 4)


def short_term(blocks, block_frames):
    """float64[len - 29]: the loudness of every window of thirty consecutive blocks."""
    return _sliding(blocks, block_frames, 30)


def integrated(blocks, block_frames):
    """The gated loudness of the whole stretch (absolute gate -70 LUFS, relative gate -10 LU); -inf when nothing
    passes."""
    a = _records(blocks)
    return float(lib().fmd_loudness_integrated(a.ctypes.data if a.size else None, a.size, int(block_frames)))
