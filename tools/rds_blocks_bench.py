"""What the block observation costs (fmd_batch_set_rds_blocks, include/fmd.h): calls with the
observation off, counting and recording, on one box, every mode visited twice in alternation in one process.

  8192 channels x 65 536 samples, 2.4 MS/s, D = 11, a device-resident float input row per channel, overlapped calls
  (concurrency 2) consumed two calls late as bench.py runs them; the block records are collected at lag 3 every step
  (fmd_batch_collect_rds_blocks), the groups as bench.py collects them.  ms per step per visit.

  The kernel's own time: the "rds_serial" stage of the per-stage profile (RDS PLL, matched filter and bit recovery,
  calls run one after the other: the stage alone on the device) per mode -- the modes differ in the bit recovery
  only, so the difference between two modes is the observing form's.  This is the stage's time, not the bit
  recovery kernel's own, which this tool does not measure -- neither alone nor inside the pipeline, where the stage
  has no events of its own; what the modes cost there is the difference of the step times above.

One JSON line, also written to profiles/rds_blocks.json.

    python tools/rds_blocks_bench.py --steps 240 --warmup 8
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from tools import fmsig_py  # noqa: E402

N, LAG, BLOCK_LAG, RING, C = 65536, 2, 3, 3, 8192
FS, D = 2.4e6, 11
MODES = {"off": 0, "count": 1, "record": 2}
VISITS = list(MODES) * 2


def make_batch(pkg, mode):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    if mode:
        b.set_rds_blocks(mode)
    return b


def run_steps(pkg, iq, mode, steps, warmup):
    b = make_batch(pkg, mode)
    b.set_concurrency(2)
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = [torch.empty((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 3)]
    s = torch.cuda.current_stream().cuda_stream
    t0, records, lost = None, 0, 0
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s)
        if j >= LAG:
            b.wait(stream=s, lag=LAG)
            b.collect_rds_array(cap=4 * C, stream=s, lag=LAG)
        if mode == 2 and j >= BLOCK_LAG:
            r, n_lost = b.collect_rds_blocks(cap=8 * C, lag=BLOCK_LAG, stream=s)
            records += len(r)
            lost += n_lost
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    b.close()
    return ms, records, lost


def run_stage(pkg, iq, mode, calls=16):
    b = make_batch(pkg, mode)
    b.set_profiling(2)
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = torch.empty((C, a_stride), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for j in range(calls):
        b.process_device(iq[j % RING].data_ptr(), N, N, audio.data_ptr(), a_stride, s)
        b.wait(stream=s)
        b.collect_rds_array(cap=4 * C, stream=s)
        if mode == 2:
            b.collect_rds_blocks(cap=8 * C, stream=s)
    torch.cuda.synchronize()
    ms, _n = b.stage_ms()
    b.close()
    return ms["rds_serial"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rds_blocks.json"))
    args = ap.parse_args()
    pkg = load_package()
    gen = fmsig_py.DeviceGenerator([fmsig_py.channel_params(FS, c) for c in range(C)], "cuda")
    iq = torch.empty((RING, C, N, 2), dtype=torch.float32, device="cuda")
    for r in range(RING):
        gen.generate(iq[r], r * N, N)
    torch.cuda.synchronize()
    res = {"tool": "rds_blocks_bench", "channels": C, "samples": N, "sample_rate_if": FS, "downsample": D, "lag": LAG,
           "block_lag": BLOCK_LAG, "steps": args.steps, "warmup": args.warmup, "order_of_visits": VISITS}
    visits = {m: [] for m in MODES}
    stage = {m: [] for m in MODES}
    for m in VISITS:
        ms, records, lost = run_steps(pkg, iq, MODES[m], args.steps, args.warmup)
        visits[m].append(round(ms, 4))
        stage[m].append(round(run_stage(pkg, iq, MODES[m]), 4))
        if m == "record":
            res["records_per_step"] = round(records / max(1, args.steps + args.warmup - BLOCK_LAG), 1)
            res["records_lost"] = lost
    res["ms_per_step"] = visits
    res["rds_serial_stage_alone_ms"] = stage
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
