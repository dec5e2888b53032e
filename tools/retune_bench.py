"""Cost of fmd_batch_retune_channels at the headline geometry (8192 channels x 65 536 samples, 2.4 MS/s, D = 11,
overlapped calls consumed two calls late, as bench.py runs them).  Prints one JSON line: ms per step with retuning
off, enabled without edits (the silent twin's cost), and with R channels retuned in front of every call.

    python tools/retune_bench.py --steps 240 --warmup 8
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

N, FS, D, LAG = 65536, 2.4e6, 11, 2


def run(pkg, C, steps, warmup, enable, R):
    b = pkg.Batch(pkg.make_params(FS, 0.0, 48000.0, 15000.0, D), C, tuning_shifts=np.zeros(C, np.int32),
                  record_callbacks=False)
    if enable:
        b.enable_retune()
    b.set_concurrency(2)
    torch.manual_seed(1)
    iq = (0.1 * torch.randn((C, N, 2), dtype=torch.float32, device="cuda")).contiguous()
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = [torch.empty((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 2)]
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    t0 = None
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if R:
            ch = np.sort(rng.choice(C, size=R, replace=False)).astype(np.uint32)
            b.retune(ch, rng.integers(-32, 32, size=R).astype(np.int32))
        b.process_device(iq.data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s)
        if j >= LAG:
            b.wait(stream=s, lag=LAG)
        if j % 8 == 7:
            b.collect_rds(lag=LAG)
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    b.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--edits", default="1,64,1024,8192")
    args = ap.parse_args()
    pkg = load_package()
    res = {"channels": args.channels, "samples": N, "steps": args.steps}
    res["off_ms_per_step"] = run(pkg, args.channels, args.steps, args.warmup, False, 0)
    res["enabled_idle_ms_per_step"] = run(pkg, args.channels, args.steps, args.warmup, True, 0)
    res["twin_overhead"] = res["enabled_idle_ms_per_step"] / res["off_ms_per_step"] - 1.0
    for r in [int(x) for x in args.edits.split(",") if x]:
        ms = run(pkg, args.channels, args.steps, args.warmup, True, r)
        res["R%d_ms_per_step" % r] = ms
        res["R%d_us_per_call_over_idle" % r] = (ms - res["enabled_idle_ms_per_step"]) * 1e3
    print(json.dumps(res))


if __name__ == "__main__":
    main()
