"""The RDS bit slicer and block synchroniser restated on the oracle's taps (helper of the block-observation tests).

The oracle delivers whole groups only, but it exposes the matched-filter row (`rds_mf`) and the bit-sync resonator row
(`rds_sync`) of every call.  From those two rows the peak slicer (RDSProcess.cpp:144-179) and the block machine
(ProcessNewRdsBit / CheckBlock, RDSProcess.cpp:272-431) are integer work: this module restates them and keeps what
the reference's machine computes and drops -- every block decision (include/fmd.h fmd_rds_block) and the reception
counters (fmd_rds_quality).  That the restatement is the reference's machine is checked where it can be: its groups
are the oracle's, call by call (tests/test_rds_sync_spec.py).

The slicer is vectorised, with float32 carry-in of the last sync value, slope, data sample and bit; the per-bit
machine is plain Python (a few thousand bits per stream).
"""
import numpy as np

BLOCK_DTYPE = np.dtype([("channel", "<u4"), ("call_index", "<u4"), ("bit_index", "<u4"), ("raw", "<u4"),
                        ("word", "<u2"), ("sample", "<u2"), ("position", "u1"), ("status", "u1"), ("state", "u1"),
                        ("corrected", "u1")])
QUALITY_FIELDS = ("bits", "candidates", "blocks", "corrected", "failed", "sync_acquired", "sync_lost", "groups")

# RDSProcess.cpp:13-17 (BLK_OFFSET_TBL: A, B, C, D, A, B, C', D) and :19-23 (PARCKH)
OFFSETS = (0x3D8, 0x3D4, 0x25C, 0x258, 0x3D8, 0x3D4, 0x3CC, 0x258)
POSITION_OF = (0, 1, 2, 3, 0, 1, 4, 3)
PARCKH = (0x2DC, 0x16E, 0x0B7, 0x287, 0x39F, 0x313, 0x355, 0x376, 0x1BB, 0x201, 0x3DC, 0x1EE, 0x0F7, 0x2A7, 0x38F, 0x31B)
BITSYNC, BLOCKSYNC, GROUPDECODE, GROUPRESYNC = 0, 1, 2, 3
M32 = 0xFFFFFFFF


def check_block(in_bits, offset, fec):
    """CheckBlock (RDSProcess.cpp:377-431) -> (in_bits afterwards, syndrome returned, syndrome before the error
    correction, bits flipped).  in_bits is the 32-bit shift register."""
    tb = in_bits & 0x3FFFFFF
    syn = tb >> 16
    for i in range(16):
        if tb & 0x8000:
            syn ^= PARCKH[i]
        tb <<= 1
    syn ^= offset
    pre, flips = syn, 0
    if syn and fec:
        mask = 1 << 25
        for _ in range(16):
            if syn & 0x200:
                if (syn & 0x1F) == 0:
                    in_bits ^= mask
                    flips += 1
                    syn <<= 1
                else:
                    syn <<= 1
                    syn ^= 0x5B9
            else:
                syn <<= 1
            mask >>= 1
        syn &= 0x3FF
    return in_bits, syn, pre, flips


def check_block_vec(raw, offset, fec):
    """check_block on arrays: raw (26-bit blocks), offset (syndromes of the offset words), fec (bool) ->
    (block afterwards, syndrome returned, syndrome before the error correction, bits flipped)"""
    bits = np.asarray(raw, np.int64) & 0x3FFFFFF
    syn = bits >> 16
    for i in range(16):
        syn = syn ^ np.where((bits >> (15 - i)) & 1, PARCKH[i], 0)
    syn = syn ^ np.asarray(offset, np.int64)
    pre = syn.copy()
    on = (syn != 0) & np.asarray(fec, bool)
    flips = np.zeros_like(bits)
    for i in range(16):
        top = (syn & 0x200) != 0
        trap = top & ((syn & 0x1F) == 0)
        bits = np.where(on & trap, bits ^ (1 << (25 - i)), bits)
        flips = flips + (on & trap)
        nxt = syn << 1
        nxt = np.where(top & ~trap, nxt ^ 0x5B9, nxt)
        syn = np.where(on, nxt, syn)
    syn = np.where(on, syn & 0x3FF, syn)
    return bits, syn, pre, flips


class Machine:
    """What cRDSRxSignalProcessor::Reset (RDSProcess.cpp:92-118) starts over: slicer carry and block machine, but not
    the shift register and not the block words."""

    def __init__(self):
        self.in_bits = 0
        self.bd = [0, 0, 0, 0]
        self.restart()

    def restart(self):
        self.last_sync = np.float32(0)
        self.last_slope = np.float32(0)
        self.last_data = np.float32(0)
        self.last_bit = 0
        self.state, self.block, self.bitpos, self.boff = BITSYNC, 0, 0, 0


class SyncSpec:
    """One channel: records, counters and groups of the calls it is fed, call by call."""

    def __init__(self, channel=0):
        self.channel = channel
        self.m = Machine()
        self.q = dict.fromkeys(QUALITY_FIELDS, 0)
        self.records = []   # tuples in BLOCK_DTYPE's field order
        self.groups = []    # (call_index, (A, B, C, D))

    def reset_machine(self):
        """a reset / retune / capture switch of the decoder: the counters run on"""
        self.m.restart()

    def replace_machine(self, other):
        """an imported or loaded decoder: `other`'s machine (a SyncSpec), this slot's counters"""
        import copy
        self.m = copy.deepcopy(other.m)

    def quality(self):
        return tuple(self.q[f] & M32 for f in QUALITY_FIELDS)

    # ---- the slicer (:144-179), vectorised ----
    def _slice(self, mf, sync):
        m = self.m
        mf = np.ascontiguousarray(mf, dtype=np.float32)
        sync = np.ascontiguousarray(sync, dtype=np.float32)
        if len(sync) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        s = np.concatenate([[m.last_sync], sync]).astype(np.float32)
        slope = (s[1:] - s[:-1]).astype(np.float32)
        prev = np.concatenate([[m.last_slope], slope[:-1]]).astype(np.float32)
        fire = (slope < 0) & ((prev * slope).astype(np.float32) < 0)
        dprev = np.concatenate([[m.last_data], mf[:-1]]).astype(np.float32)
        at = np.nonzero(fire)[0]
        raw = (dprev[at] >= 0).astype(np.int64)
        before = np.concatenate([[m.last_bit], raw[:-1]]).astype(np.int64) if len(raw) else raw
        m.last_sync, m.last_slope, m.last_data = s[-1], slope[-1], mf[-1]
        if len(raw):
            m.last_bit = int(raw[-1])
        return at, raw ^ before

    # ---- the machine (:272-431), per bit ----
    def call(self, call_index, mf, sync, mode=2):
        """One call's taps.  mode as fmd_batch_set_rds_blocks: 0 the machine only, 1 and the counters, 2 and records."""
        at, bits = self._slice(mf, sync)
        m, q = self.m, self.q
        for sample, nb in zip(at.tolist(), bits.tolist()):
            if mode:
                q["bits"] += 1
            m.in_bits = ((m.in_bits << 1) | nb) & M32
            raw = m.in_bits & 0x3FFFFFF
            state = m.state
            rec = None
            emit = False
            if state == BITSYNC:
                _, syn, _, _ = check_block(m.in_bits, OFFSETS[0], False)
                if syn == 0:
                    rec = (0, 0, 0)
                    if mode:
                        q["candidates"] += 1
                    m.bitpos, m.boff = 0, 0
                    m.bd[0] = (m.in_bits >> 10) & 0xFFFF
                    m.block, m.state = 1, BLOCKSYNC
            else:
                m.bitpos += 1
                if m.bitpos < 26:
                    continue
                m.bitpos = 0
                if state == GROUPRESYNC:  # (unreachable with BLOCK_ERROR_LIMIT 0: writes and counts nothing)
                    m.block += 1
                    if m.block > 3:
                        m.block, m.state = 0, GROUPDECODE
                    continue
                idx = m.block + m.boff
                m.in_bits, syn, pre, flips = check_block(m.in_bits, OFFSETS[idx], state == GROUPDECODE)
                status = 2 if syn else (1 if pre else 0)
                rec = (POSITION_OF[idx], status, flips)
                if mode:
                    q["blocks"] += 1
                    q["corrected"] += status == 1
                    q["failed"] += status == 2
                    q["sync_acquired"] += status != 2 and state == BLOCKSYNC and m.block >= 3
                    q["sync_lost"] += status == 2 and state == GROUPDECODE
                if syn:
                    m.state = BITSYNC  # BLOCKSYNC: back at once; GROUPDECODE: BLOCK_ERROR_LIMIT is 0
                else:
                    word = (m.in_bits >> 10) & 0xFFFF
                    m.bd[m.block] = word
                    m.boff = 4 if (m.block == 1 and (word & 0x0800)) else 0
                    if state == BLOCKSYNC:
                        if m.block >= 3:
                            m.block, m.state, emit = 0, GROUPDECODE, True
                        else:
                            m.block += 1
                    else:
                        m.block += 1
                        if m.block > 3:
                            m.block, emit = 0, True
            if emit:
                self.groups.append((call_index, tuple(m.bd)))
                if mode:
                    q["groups"] += 1
            if rec is not None and mode == 2:
                self.records.append((self.channel, call_index, q["bits"] & M32, raw, (m.in_bits >> 10) & 0xFFFF,
                                     sample, rec[0], rec[1], state, rec[2]))

    def records_array(self):
        return np.array(self.records, dtype=BLOCK_DTYPE) if self.records else np.zeros(0, BLOCK_DTYPE)
