"""Cost of saving, loading and moving channel state at the headline geometry (8192 channels x 65 536 samples,
2.4 MS/s, D = 11, overlapped calls consumed two calls late, as bench.py runs them).  Prints one JSON line: blob bytes
per channel, wall time of save_state and load_state, and the cost of a call with an import of R channels in front of
it against plain calls of the same run.

An import needs a blob whose clock is the batch's, so the blob is exported from the batch itself (synchronous, not
timed) in front of every measured block; a block is BLOCK overlapped calls, with or without the import in front of its
first call, plain and import blocks alternating.

    python tools/state_bench.py --cycles 12
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

N, FS, D, LAG, BLOCK = 65536, 2.4e6, 11, 2, 6


def make(pkg, C):
    b = pkg.Batch(pkg.make_params(FS, 0.0, 48000.0, 15000.0, D), C, tuning_shifts=np.zeros(C, np.int32),
                  record_callbacks=False)
    b.set_concurrency(2)
    return b


class Loop:
    def __init__(self, pkg, C):
        self.b = make(pkg, C)
        torch.manual_seed(1)
        self.C = C
        self.iq = (0.1 * torch.randn((C, N, 2), dtype=torch.float32, device="cuda")).contiguous()
        self.a_stride = (self.b.max_audio_floats(N) + 63) // 64 * 64
        self.audio = [torch.empty((C, self.a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 2)]
        self.s = torch.cuda.current_stream().cuda_stream
        self.j = 0

    def calls(self, n):
        for _ in range(n):
            self.b.process_device(self.iq.data_ptr(), N, N, self.audio[self.j % len(self.audio)].data_ptr(),
                                  self.a_stride, self.s)
            self.j += 1
            self.b.wait(stream=self.s, lag=LAG)
        self.b.wait(stream=self.s)
        torch.cuda.synchronize()
        self.b.collect_rds()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8192)
    ap.add_argument("--cycles", type=int, default=12)
    ap.add_argument("--imports", default="1,64,8192")
    args = ap.parse_args()
    pkg = load_package()
    C = args.channels
    lp = Loop(pkg, C)
    lp.calls(8)
    res = {"channels": C, "samples": N, "block_calls": BLOCK, "cycles": args.cycles}
    # ---- save / load ----
    t = time.perf_counter()
    blob = lp.b.save_state()
    res["save_state_ms"] = (time.perf_counter() - t) * 1e3
    res["blob_bytes"] = len(blob)
    res["blob_bytes_per_channel"] = len(blob) / C
    t = time.perf_counter()
    lp.b.save_state()
    res["save_state_again_ms"] = (time.perf_counter() - t) * 1e3
    dst = make(pkg, C)
    t = time.perf_counter()
    dst.load_state(blob)
    res["load_state_ms"] = (time.perf_counter() - t) * 1e3
    dst.close()
    del blob
    # ---- imports in front of a block of overlapped calls ----
    rng = np.random.default_rng(7)
    for r in [int(x) for x in args.imports.split(",") if x]:
        r = min(r, C)
        plain, moved, host = [], [], []
        for cyc in range(2 * args.cycles):
            ch = np.sort(rng.choice(C, size=r, replace=False)).astype(np.uint32)
            part = lp.b.export_channels(ch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if cyc % 2:
                lp.b.import_channels(np.roll(ch, 1), part)
                host.append((time.perf_counter() - t0) * 1e3)
            lp.calls(BLOCK)
            (moved if cyc % 2 else plain).append((time.perf_counter() - t0) * 1e3)
        res["import%d_plain_block_ms" % r] = float(np.median(plain))
        res["import%d_block_ms" % r] = float(np.median(moved))
        res["import%d_cost_ms" % r] = float(np.median(moved) - np.median(plain))
        res["import%d_host_call_ms" % r] = float(np.median(host))
        res["import%d_blob_bytes" % r] = len(part)
    res["plain_ms_per_step"] = res["import1_plain_block_ms"] / BLOCK if "import1_plain_block_ms" in res else None
    lp.b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
