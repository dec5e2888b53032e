"""Cost of fmd_batch_reset_channels at the headline geometry (8192 channels x 65 536 samples, 2.4 MS/s, D = 11,
overlapped calls consumed two calls late, as bench.py runs them).  Prints one JSON line of ms per step:
  - no reset at all (the default path);
  - R channels reset in front of every call (R = 1, 64, 8192): the cost of a call with resets;
  - the steady state after one reset in front of the second call, when the batch's ring phases are non-zero:
    one channel per wave reset (every wave mixed: the per-lane form of the RDS ring filters), and every channel
    reset (one origin for all: the uniform form with a shifted phase).

    python tools/reset_bench.py --steps 240 --warmup 8
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


def run(pkg, C, steps, warmup, per_call=0, once=None):
    b = pkg.Batch(pkg.make_params(FS, 0.0, 48000.0, 15000.0, D), C, tuning_shifts=np.zeros(C, np.int32),
                  record_callbacks=False)
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
        if once is not None and j == 1:  # (the first call's phases are 0: an origin there changes nothing)
            b.reset_channels(once)
        if per_call:
            b.reset_channels(np.sort(rng.choice(C, size=per_call, replace=False)).astype(np.uint32))
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
    ap.add_argument("--resets", default="1,64,8192")
    args = ap.parse_args()
    assert args.warmup >= 2, "the one-time resets go in front of the second call"
    C = args.channels
    pkg = load_package()
    res = {"channels": C, "samples": N, "steps": args.steps}
    res["off_ms_per_step"] = run(pkg, C, args.steps, args.warmup)
    for r in [int(x) for x in args.resets.split(",") if x]:
        ms = run(pkg, C, args.steps, args.warmup, per_call=min(r, C))
        res["R%d_ms_per_step" % r] = ms
        res["R%d_us_per_call_over_off" % r] = (ms - res["off_ms_per_step"]) * 1e3
    res["after_one_per_wave_ms_per_step"] = run(pkg, C, args.steps, args.warmup,
                                                once=np.arange(0, C, 64, dtype=np.uint32))
    res["after_all_ms_per_step"] = run(pkg, C, args.steps, args.warmup, once=np.arange(C, dtype=np.uint32))
    res["off_again_ms_per_step"] = run(pkg, C, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
